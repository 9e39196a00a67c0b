"""Ranged writes (include/sdfs_write.h): DedupFileChannel.writeFile for batches of byte ranges.

CPU: the host split (sdfs_cdc_write_split) against the plain-Python model (tests/write_model.py,
restated from DedupFileChannel.java:274-359 and WritableCacheBuffer.java:523-563; byte painting) on
hand-worked and seeded random batches, its capacity and argument rules, and the split's own text as
a host program under AddressSanitizer and UBSan (tests/cpu/write_split_check.cpp).  GPU: the stage
kernel against numpy at every alignment pair, the ragged insert list against the uniform entry
point and a host model, and ``HipFileWriter.write_ranges`` end to end through the writer, the reader
and the index: every route, growth, dedup through the accelerator, the overflow round, damaged
slots, MD5.  Everything is bit-exact.
Parity status: pinned by the reference's own request walk (no fixtures); the three stated
divergences (one flush per batch, FULL without a read, replaced slots release their pairs) are
what the byte model and the recount check."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from sdfs_amd import _lib
from tests import test_extent as TE  # the end-to-end base: _base, _dev, _named_counts, _refcounts
from tests import write_model as WM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PB = TE.PB
L, NBUF = TE.L, TE.NBUF


# ------------------------------------------------------------------------------------------- CPU

def _same_as_model(files, requests, cl, blob_bytes=1 << 40):
    from sdfs_amd.write import split_writes

    got = WM.as_lists(split_writes(files, requests, cl, blob_bytes))
    want = WM.split(files, requests, cl, blob_bytes)
    for k in want:
        assert got[k] == want[k], k
    return got


def test_split_hand_worked_cases():
    cl = 1000
    one = [(0, 4, 3500)]
    # inside one buffer
    g = _same_as_model(one, [(0, 1100, 200, 7)], cl)
    assert g["pieces"] == [(0, 100, 200, 7, 0)] and g["runs"] == [(0, 100, 200, 0, 1)] and g["rows"] == [1]
    assert g["row_full"] == [0] and g["file_len"] == [3500] and g["n_written"] == [200]
    # across two boundaries, a full buffer in the middle
    g = _same_as_model(one, [(0, 950, 1100, 16)], cl)
    assert g["pieces"] == [(0, 950, 50, 16, 0), (1, 0, 1000, 66, 0), (2, 0, 50, 1066, 0)]
    assert g["row_full"] == [0, 1, 0] and g["rows"] == [0, 1, 2]
    # an exact aligned buffer
    g = _same_as_model(one, [(0, 2000, 1000, 0)], cl)
    assert g["pieces"] == [(0, 0, 1000, 0, 0)] and g["row_full"] == [1] and g["rows"] == [2]
    # a later request inside an earlier one: three visible pieces, one run
    g = _same_as_model(one, [(0, 100, 300, 0), (0, 200, 50, 500)], cl)
    assert g["pieces"] == [(0, 100, 100, 0, 0), (0, 200, 50, 500, 1), (0, 250, 150, 150, 0)]
    assert g["runs"] == [(0, 100, 300, 0, 3)]
    # a later request covering an earlier one: one
    g = _same_as_model(one, [(0, 200, 50, 500), (0, 100, 300, 0)], cl)
    assert g["pieces"] == [(0, 100, 300, 0, 1)]
    # two touching requests: one run of two pieces
    g = _same_as_model(one, [(0, 10, 20, 0), (0, 30, 5, 100)], cl)
    assert g["pieces"] == [(0, 10, 20, 0, 0), (0, 30, 5, 100, 1)] and g["runs"] == [(0, 10, 25, 0, 2)]
    # a write that starts past EOF moves the length; it is never clipped
    g = _same_as_model(one, [(0, 3900, 100, 0)], cl)
    assert g["file_len"] == [4000] and g["n_written"] == [100] and g["rows"] == [3]
    # len == 0 writes nothing and moves no length
    g = _same_as_model(one, [(0, 3900, 0, 0)], cl)
    assert g["file_len"] == [3500] and g["pieces"] == [] and g["rows"] == [] and g["n_written"] == [0]
    # two files in one image
    g = _same_as_model([(0, 2, 10), (2, 2, 1500)], [(1, 990, 20, 0), (0, 5, 10, 20)], cl)
    assert g["rows"] == [0, 2, 3] and g["file_len"] == [15, 1500]
    assert g["pieces"] == [(0, 5, 10, 20, 1), (1, 990, 10, 0, 0), (2, 0, 10, 10, 0)]


@pytest.mark.parametrize("cl", [64, 4096, 262144])
def test_split_random_batches_equal_the_model(cl):
    rng = np.random.default_rng(cl)
    for _ in range(120):
        files, first = [], int(rng.integers(0, 4))
        for _f in range(int(rng.integers(1, 4))):
            n = int(rng.integers(1, 6))
            files.append((first, n, int(rng.integers(0, n * cl + 1))))
            first += n + int(rng.integers(0, 3))
        reqs = []
        for _r in range(int(rng.integers(1, 41))):
            f = int(rng.integers(0, len(files)))
            room = files[f][1] * cl
            pos = int(rng.integers(0, room))
            ln = int(rng.integers(0, 2 * cl + 2)) if rng.random() < .5 else int(rng.integers(0, 40))
            if rng.random() < .2:
                pos = pos // cl * cl
            if reqs and rng.random() < .25 and reqs[-1][0] == f:
                pos = min(reqs[-1][1] + reqs[-1][2], room - 1)  # touching the one before
            reqs.append((f, pos, min(ln, room - pos), int(rng.integers(0, 1 << 20))))
        _same_as_model(files, reqs, cl)


def _raw_split(files, requests, cl, blob_bytes, pcap, rcap, wcap, guard=4):
    """The C entry point with arrays of the given capacities plus ``guard`` entries of 0xEE after each."""
    f = np.asarray(files, np.uint64).reshape(-1, 3)
    q = np.asarray(requests, np.uint64).reshape(-1, 4)
    mk = lambda n, dt: np.full((n + guard) * np.dtype(dt).itemsize, 0xEE, np.uint8).view(dt)  # noqa: E731
    a = dict(piece_row=mk(pcap, np.uint32), piece_start=mk(pcap, np.uint32), piece_len=mk(pcap, np.uint32),
             piece_req=mk(pcap, np.uint32), piece_src_off=mk(pcap, np.uint64), run_row=mk(rcap, np.uint32),
             run_pos=mk(rcap, np.uint32), run_len=mk(rcap, np.uint32), run_first_piece=mk(rcap, np.uint32),
             run_n_pieces=mk(rcap, np.uint32), row_slot=mk(wcap, np.uint64), row_full=mk(wcap, np.uint8))
    nw, fl = mk(len(q), np.int64), mk(len(f), np.uint64)
    plan = _lib.WritePlan(piece_cap=pcap, run_cap=rcap, row_cap=wcap, **{k: v.ctypes.data for k, v in a.items()})
    rc = _lib.load().sdfs_cdc_write_split(f.ctypes.data, len(f), q.ctypes.data, len(q), cl, blob_bytes, nw.ctypes.data,
                                          fl.ctypes.data, ctypes.byref(plan))
    return rc, plan, a, nw, fl


def test_split_ecap_reports_the_counts_and_writes_nothing_else():
    files, reqs = [(0, 4, 0)], [(0, 100, 300, 0), (0, 200, 50, 500), (0, 900, 1200, 0)]
    rc, plan, a, nw, fl = _raw_split(files, reqs, 1000, 1 << 20, 8, 8, 8)
    assert rc == _lib.OK and (plan.n_pieces, plan.n_runs, plan.n_rows) == (6, 4, 3)
    for caps in [(5, 8, 8), (8, 3, 8), (8, 8, 2), (0, 0, 0)]:
        rc, plan, a, nw, fl = _raw_split(files, reqs, 1000, 1 << 20, *caps)
        assert rc == _lib.ECAP and (plan.n_pieces, plan.n_runs, plan.n_rows) == (6, 4, 3)
        for v in list(a.values()) + [nw, fl]:
            assert (v.view(np.uint8) == 0xEE).all()
    # exact room: the guard entries after the arrays are intact
    rc, plan, a, nw, fl = _raw_split(files, reqs, 1000, 1 << 20, 6, 4, 3)
    assert rc == _lib.OK
    for k, v in a.items():
        n = {"p": 6, "r": 3 if k.startswith("row") else 4}[k[0]]
        assert (v[n:].view(np.uint8) == 0xEE).all(), k
    assert (nw[3:].view(np.uint8) == 0xEE).all() and (fl[1:].view(np.uint8) == 0xEE).all()
    assert nw[:3].tolist() == [300, 50, 1200] and fl[0] == 2100


def test_split_refuses_bad_batches():
    def rc(files, reqs, cl=1000, blob=1 << 20):
        with pytest.raises(WM.Invalid):
            WM.split(files, reqs, cl, blob)
        return _raw_split(files, reqs, cl, blob, 8, 8, 8)[0]

    one = [(0, 4, 100)]
    assert rc(one, [(1, 0, 10, 0)]) == _lib.EINVAL                      # a file >= n_files
    assert rc(one, [(0, 0, 10, 5)], blob=14) == _lib.EINVAL             # src_off + len passes the blob
    assert rc(one, [(0, 3999, 2, 0)]) == _lib.EINVAL                    # needs slot 4 of 4: grow the image first
    assert rc([(0, 4, 0), (3, 2, 0)], [(0, 0, 1, 0), (1, 0, 1, 0)]) == _lib.EINVAL  # two written files share slot 3
    assert rc(one, [(0, 2 ** 64 - 4, 10, 0)]) == _lib.EINVAL            # file_pos + len overflows
    assert rc([(2 ** 64 - 2, 4, 0)], [(0, 0, 1, 0)]) == _lib.EINVAL     # first_slot + n_slots overflows
    assert rc(one, [(0, 0, 1, 0)], cl=0) == _lib.EINVAL
    assert rc(one, [(0, 0, 1, 0)], cl=2 ** 31) == _lib.EINVAL
    assert _raw_split([(0, 2 ** 40, 0)], [(0, 0, 2 ** 33, 0)], 1, 2 ** 40, 8, 8, 8)[0] == _lib.EINVAL  # > 2^32 - 2 pieces
    # the same files, only one of them written: accepted
    assert _raw_split([(0, 4, 0), (3, 2, 0)], [(0, 0, 1, 0), (1, 0, 0, 0)], 1000, 64, 8, 8, 8)[0] == _lib.OK


def test_split_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "write_split_check"
    src = os.path.join(ROOT, "tests", "cpu", "write_split_check.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    src, "-o", str(exe)], check=True, timeout=240)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert r.stdout.rstrip().endswith("OK"), r.stdout[-3000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and not r.stderr.strip(), r.stderr[-6000:]


def test_device_entry_points_refuse_bad_arguments_before_the_device():
    lib = _lib.load()
    assert lib.sdfs_cdc_write_stage(0, 4, None, 0, None, None, None, 100, None, 0, None, None, 0, None, None) == _lib.EINVAL
    assert lib.sdfs_cdc_write_stage(0, 0, None, 0, None, None, None, 0, None, 0, None, None, 0, None, None) == _lib.EINVAL
    assert lib.sdfs_cdc_write_stage(0, 0, None, 0, None, None, None, 100, None, 0, None, None, 0, None, None) == _lib.OK
    assert lib.sdfs_cdc_map_inserts_from_runs(0, 0, 1, None, None, None, None, 1, 100, None, None, None, 0, None,
                                              None) == _lib.EINVAL


# ------------------------------------------------------------------------------------------- GPU

def _md5_base():
    """TE._base's store through the MD5 engine (hash_len 16)."""
    import torch

    from sdfs_amd import HipVariableMD5HashEngine
    from sdfs_amd.archive import HipBufferWriter
    from sdfs_amd.device import DeviceBatch
    from sdfs_amd.index import HipHashesMap
    from sdfs_amd.meta import slot_bytes

    e = HipVariableMD5HashEngine()
    batch = DeviceBatch(e, nbuf=NBUF, buf_len=L)
    batch.fill_streams(first_stream=5150, bufs_per_stream=2)
    ix = HipHashesMap(1 << 13)
    wr = HipBufferWriter(ix, hash_len=16, compress=True, blocksz=[200000, 260000, 150000])
    m, arcs = wr.write(batch, PB)
    torch.cuda.synchronize()
    return dict(engine=e, ix=ix, wr=wr, m=m, arcs=arcs, data=batch.data.cpu().numpy().copy(),
                slot_len=slot_bytes(16, L, 4095), aes=False, hash_len=16)


def _open(w, nslots=NBUF):
    """The file writer over a base, and the image grown to nslots slots."""
    import torch

    from sdfs_amd.read import HipBufferReader
    from sdfs_amd.write import HipFileWriter

    hl = w.get("hash_len", 32)
    rd = HipBufferReader(L, hl, aes=TE._KEY if w["aes"] else None, record_ivs=w["aes"], engine=w["engine"])
    fw = HipFileWriter(w["wr"], rd, w["engine"], L)
    m = torch.zeros(nslots * w["slot_len"], dtype=torch.uint8, device="cuda:0")
    m[: NBUF * w["slot_len"]].copy_(w["m"])
    return fw, rd, m


def _blob(requests_wo_src, seed, gap=3):
    """Random bytes for the requests [(file, pos, len)], each at an odd offset -> (requests, blob)."""
    rng = np.random.default_rng(seed)
    at, reqs = gap, []
    for f, pos, ln in requests_wo_src:
        reqs.append((f, pos, ln, at))
        at += ln + gap
    return reqs, rng.integers(0, 256, at + 16, dtype=np.uint8)


def _write(w, fw, m, nslots, files, reqs, blob, accel=True, ivs=None):
    import torch

    a = w["arcs"]
    res = fw.write_ranges(m, nslots, w["slot_len"], files, reqs, TE._dev(blob), PB + int(a.store_off.shape[0]), a.store,
                          a.store_off, a.store_len, a.raw_len, PB, accel=accel, store_ivs=a.record_ivs(), ivs=ivs)
    torch.cuda.synchronize()
    return res


def _read_files(w, rd, res, m, nslots, files, skip_slots=()):
    """Every file read whole, buffer by buffer, through the concatenated directory -> [bytearray]
    (a buffer of skip_slots reads as None and is left as zeros)."""
    import torch

    a = w["arcs"]
    store, off, ln, raw, ivs = res.directory(a.store, a.store_off, a.store_len, a.raw_len, a.record_ivs())
    reqs, at = [], 0
    for f, (first, n, flen) in enumerate(files):
        for p in range(0, flen, L):
            if first + p // L in skip_slots:
                continue
            reqs.append((f, p, min(L, flen - p), at))
            at += min(L, flen - p)
    out, n_read, status, _ = rd.read_ranges(m, nslots, w["slot_len"], files, reqs, store, off, ln, raw, PB, store_ivs=ivs)
    torch.cuda.synchronize()
    assert not status.any(), status.tolist()
    host = out.cpu().numpy()
    got = [bytearray(flen) for _, _, flen in files]
    for (f, p, n, o), nr in zip(reqs, n_read.tolist()):
        assert nr == n
        got[f][p:p + n] = host[o:o + n].tobytes()
    return got


def _clean_recount(w, m, nslots):
    r = w["ix"].recount(m, nslots, w["slot_len"], hash_len=w.get("hash_len", 32))
    c = r.counts.tolist()
    assert c[1] == 0 and c[2] == 0 and c[3] == 0 and c[4] == 0 and c[7] == 0, c  # missed, corrupt, under, over, listed


def _done(w, rd):
    rd.destroy()
    w["wr"].destroy()
    w["ix"].destroy()
    w["engine"].destroy()


def _check(w, rd, res, m, nslots, files, reqs, blob, old_bytes, want_status=None):
    from sdfs_amd.write import split_writes

    model = WM.split(files, reqs, L, len(blob))
    assert res.n_written.tolist() == model["n_written"] and res.file_len.tolist() == model["file_len"]
    assert res.status.tolist() == (want_status or [0] * len(reqs))
    assert res.n_pieces == len(model["pieces"]) and res.n_runs == len(model["runs"])
    new_files = [(first, n, fl) for (first, n, _), fl in zip(files, model["file_len"])]
    want = WM.apply(old_bytes, reqs, blob)
    got = _read_files(w, rd, res, m, nslots, new_files)
    for g, x in zip(got, want):
        x = bytes(x) + bytes(len(g) - len(x))
        assert len(g) == len(x) and g == x, next(i for i in range(len(g)) if g[i] != x[i])
    _clean_recount(w, m, nslots)
    return got


MIXED = [(0, 100003, 5000),                 # unaligned inside one buffer (pos % 64 = 35)
         (0, L + 150001, 2 * L + 777),      # ACCEL head, FULL middle, ACCEL tail
         (0, 4 * L, L),                     # an exact aligned buffer
         (0, 5 * L + 1000, 3000), (0, 5 * L + 2000, 500),      # overlapping: the later wins
         (0, 6 * L + 50000, 1000), (0, 6 * L + 51000, 2000),   # touching: one run
         (0, 7 * L + 12345, 1),             # one byte
         (0, 7 * L + 20, 0)]                # nothing


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["lz4", "aes"])
def test_gpu_mixed_batch_both_routes(variant):
    from sdfs_amd import write as W

    reqs, blob = _blob(MIXED, 11)
    assert reqs[0][1] % 64 and reqs[0][3] % 4
    files = [(0, NBUF, NBUF * L)]
    got = {}
    for accel in (True, False):
        w = TE._base(variant)
        fw, rd, m = _open(w)
        res = _write(w, fw, m, NBUF, files, reqs, blob, accel=accel)
        part = W.ROUTE_ACCEL if accel else W.ROUTE_MATERIALISE
        assert res.row_route.tolist() == [part, part, W.ROUTE_FULL, part, W.ROUTE_FULL, part, part, part]
        assert res.n_runs == 8 and res.n_pieces == 11 and len(res.archives) == 1
        got[accel] = _check(w, rd, res, m, NBUF, files, reqs, blob, [bytearray(w["data"].tobytes())])
        _done(w, rd)
    assert got[True] == got[False]


@pytest.mark.gpu
def test_gpu_growth_and_a_request_past_the_image():
    import torch

    from sdfs_amd import write as W

    w = TE._base("lz4")
    fw, rd, m = _open(w, 12)
    files = [(0, 12, NBUF * L)]
    reqs, blob = _blob([(0, 9 * L + L // 2, 5000)], 12)
    res = _write(w, fw, m, 12, files, reqs, blob)
    assert res.row_route.tolist() == [W.ROUTE_MATERIALISE] and res.rows.tolist() == [9]
    assert res.file_len.tolist() == [9 * L + L // 2 + 5000]
    assert not m[8 * w["slot_len"]: 9 * w["slot_len"]].any()  # slot 8 stays empty and reads as zeros
    _check(w, rd, res, m, 12, files, reqs, blob, [bytearray(w["data"].tobytes())])
    # a request that needs slot 12: refused before anything changes
    m_before, store_before = m.clone(), w["arcs"].store.clone()
    keys = sorted(TE._named_counts(w, [(m[: NBUF * w["slot_len"]], NBUF)]))
    ref_before = TE._refcounts(w["ix"], keys)
    bad, blob2 = _blob([(0, 100, 10), (0, 12 * L - 5, 10)], 13)
    with pytest.raises(_lib.SdfsCdcError) as e:
        _write(w, fw, m, 12, [(0, 12, res.file_len[0])], bad, blob2)
    assert e.value.code == _lib.EINVAL
    torch.cuda.synchronize()
    assert torch.equal(m, m_before) and torch.equal(w["arcs"].store, store_before)
    assert TE._refcounts(w["ix"], keys) == ref_before
    _done(w, rd)


@pytest.mark.gpu
def test_gpu_dedup_through_the_accelerator_and_sweep():
    w = TE._base("lz4")
    fw, rd, m = _open(w)
    before = TE._named_counts(w, [(w["m"], NBUF)])
    files = [(0, NBUF, NBUF * L)]
    RL = 65536
    blob = np.concatenate([np.zeros(5, np.uint8), w["data"][30000:30000 + RL]])  # bytes that are stored already
    reqs = [(0, 3 * L + 100003, RL, 5)]
    res = _write(w, fw, m, NBUF, files, reqs, blob)
    assert int(res.info["run_dup"].sum().item()) > 0  # the run found its interior chunks
    _check(w, rd, res, m, NBUF, files, reqs, blob, [bytearray(w["data"].tobytes())])
    named = TE._named_counts(w, [(m, NBUF)])
    keys = sorted(set(named) | set(before))
    pos, ref = TE._refcounts(w["ix"], keys)
    assert ref == [named.get(k, 0) for k in keys]
    dead = {k for k in keys if k not in named}
    assert dead and all(p >= PB for p in pos)  # overwritten fingerprints sit at count 0 until the sweep
    digests, _, left = w["ix"].sweep()
    assert {d.tobytes() for d in digests.cpu().numpy()} == dead and left == 0
    _done(w, rd)


@pytest.mark.gpu
def test_gpu_overflow_round():
    from sdfs_amd import write as W

    w = TE._base("lz4")
    fw, rd, m = _open(w)
    files = [(0, NBUF, NBUF * L)]
    reqs, blob = _blob([(0, 1000 + 4000 * i, 16) for i in range(60)] + [(0, 3 * L + 777, 3001)], 14)
    res = _write(w, fw, m, NBUF, files, reqs, blob)
    assert res.row_route.tolist() == [W.ROUTE_ACCEL_MATERIALISE, W.ROUTE_ACCEL]
    assert res.info["insert_status"][0] == _lib.EXT_OVERFLOW and len(res.archives) == 2
    assert res.pos_bases[1] == res.pos_bases[0] + int(res.archives[0].store_off.shape[0])
    _check(w, rd, res, m, NBUF, files, reqs, blob, [bytearray(w["data"].tobytes())])
    # the round-1 run records of the overflowing row: released, at count 0 until the sweep
    k = int(res.info["run_first"][60].item())
    assert k >= 60
    pos, ref = w["ix"].get_digests(res.info["run_hash"][:k].contiguous())
    assert ref.tolist() == [0] * k and min(pos.tolist()) >= PB
    _done(w, rd)


@pytest.mark.gpu
def test_gpu_bad_slots_fail_alone():
    import torch

    from sdfs_amd import write as W

    w = TE._base("lz4")
    fw, rd, m = _open(w)
    sl = w["slot_len"]
    good = m.clone()
    m[2 * sl + 5: 2 * sl + 9] = TE._dev(np.array([0, 0, 3, 0xE8], np.uint8))  # slot 2: 1 000 pairs, more than it holds
    m[3 * sl + 9 + 32 + 8 + 12 + 3] += 5                # slot 3, pair 0, nlen: five bytes into pair 1
    damaged = m.clone()
    files = [(0, NBUF, NBUF * L)]
    reqs, blob = _blob([(0, 2 * L - 100, 300), (0, 2 * L + 5000, 64), (0, 3 * L + 4099, 3000), (0, 5 * L + 77, 1234)], 15)
    res = _write(w, fw, m, NBUF, files, reqs, blob)
    assert res.status.tolist() == [_lib.WRITE_SLOT, _lib.WRITE_SLOT, _lib.WRITE_SLOT, 0]
    assert res.row_route.tolist() == [W.ROUTE_ACCEL, W.ROUTE_FAIL, W.ROUTE_ACCEL, W.ROUTE_ACCEL]
    assert res.info["row_status"].tolist() == [0, _lib.WRITE_SLOT, _lib.WRITE_SLOT, 0]
    assert torch.equal(m[2 * sl: 4 * sl], damaged[2 * sl: 4 * sl])  # both rows keep their images
    assert not torch.equal(m[sl: 2 * sl], damaged[sl: 2 * sl]) and not torch.equal(m[5 * sl: 6 * sl], damaged[5 * sl: 6 * sl])
    # every other request of the batch is applied (a request with a status: to its other rows)
    want = WM.apply([bytearray(w["data"].tobytes())], reqs, blob)[0]
    want[2 * L: 4 * L] = w["data"][2 * L: 4 * L].tobytes()
    got = _read_files(w, rd, res, m, NBUF, files, skip_slots=(2, 3))[0]
    got[2 * L: 4 * L] = want[2 * L: 4 * L]
    assert got == want
    # with the damage undone the image names every count exactly: the failed rows moved none
    m[2 * sl: 4 * sl].copy_(good[2 * sl: 4 * sl])
    _clean_recount(w, m, NBUF)
    _done(w, rd)


STAGE_LENS = [1, 3, 15, 16, 17, 63, 64, 65, 4095, 65535, 65536, 65537, 262144]


@pytest.mark.gpu
def test_gpu_stage_kernel_against_numpy():
    import torch

    from sdfs_amd.write import stage_pieces

    rng = np.random.default_rng(16)
    blob = rng.integers(0, 256, 262144 + 64, dtype=np.uint8)
    src, dst, ln, at = [], [], [], 0
    for n in STAGE_LENS:
        for sa in range(16):
            for da in range(16):
                at = (at + 64 + 15) // 16 * 16 + da  # a guard of at least 64 bytes before every extent
                src.append(sa + int(rng.integers(0, 2)) * 16)
                dst.append(at)
                ln.append(n)
                at += n
    total = at + 64
    want = np.full(total, 0xA5, np.uint8)
    for s, d, n in zip(src, dst, ln):
        want[d:d + n] = blob[s:s + n]
    # one entry past the blob: flagged, its destination untouched
    src.append(len(blob) - 10)
    dst.append(dst[0])
    ln.append(11)
    stage = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_req = TE._dev(np.arange(len(ln), dtype=np.int32) % 7)
    req_status = torch.zeros(7, dtype=torch.int32, device="cuda:0")
    st = stage_pieces(TE._dev(blob), TE._dev(np.asarray(src, np.int64)), TE._dev(np.asarray(dst, np.int64)),
                      TE._dev(np.asarray(ln, np.int32)), 262144, stage, piece_req=d_req, req_status=req_status)
    torch.cuda.synchronize()
    assert st.tolist() == [0] * (len(ln) - 1) + [_lib.WRITE_BOUNDS]
    assert req_status.tolist() == [_lib.WRITE_BOUNDS if r == (len(ln) - 1) % 7 else 0 for r in range(7)]
    got = stage.cpu().numpy()
    assert (got == want).all(), int(np.flatnonzero(got != want)[0])  # the guards of 0xA5 included
    # 4 096 pieces of 16 bytes in one launch
    n = 4096
    src = rng.integers(0, len(blob) - 16, n)
    dst = np.arange(n) * 37 + 5
    stage = torch.full((n * 37 + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    want = np.full(n * 37 + 64, 0xA5, np.uint8)
    for s, d in zip(src.tolist(), dst.tolist()):
        want[d:d + 16] = blob[s:s + 16]
    st = stage_pieces(TE._dev(blob), TE._dev(src.astype(np.int64)), TE._dev(dst.astype(np.int64)),
                      TE._dev(np.full(n, 16, np.int32)), 262144, stage)
    torch.cuda.synchronize()
    assert not st.any() and (stage.cpu().numpy() == want).all()


def _host_inserts(ins, n):
    return [ins.hash[:n].cpu().numpy().tobytes(), ins.hashloc[:n].tolist(), ins.len[:n].tolist(), ins.pos[:n].tolist(),
            ins.offset[:n].tolist(), ins.nlen[:n].tolist(), ins.dst_buf[:n].tolist()]


@pytest.mark.gpu
def test_gpu_inserts_from_runs():
    import torch

    from sdfs_amd import HipVariableSha256HashEngine
    from sdfs_amd.device import DeviceBatch
    from sdfs_amd.extent import inserts_from_chunks
    from sdfs_amd.write import inserts_from_runs

    e = HipVariableSha256HashEngine()
    # uniform runs: the uniform entry point's list
    RL, nrun = 65536, 4
    b = DeviceBatch(e, nbuf=nrun, buf_len=RL)
    b.fill_streams(first_stream=77, bufs_per_stream=1)
    b.run()
    total = int(b.total.item())
    loc = torch.arange(total + 8, dtype=torch.int64, device="cuda:0") * 3 + PB
    dst_buf, run_pos = [3, 0, 3, 1], [100003, 5, 17, L - RL]
    a, a_first = inserts_from_chunks(b, loc, dst_buf, run_pos, 4, L)
    r, r_first = inserts_from_runs(b.out, 0, [RL] * nrun, loc, dst_buf, run_pos, 4, L, nrun * b.cap, b.data.device)
    torch.cuda.synchronize()
    assert a_first.tolist() == r_first.tolist() and r_first[-1].item() == total
    assert _host_inserts(a, total) == _host_inserts(r, total)
    # ragged runs after one whole buffer, against a model built from the host results
    lens = [8192, 1, 4095, 4096, 70001, 262144]
    offs = np.concatenate([[0], np.cumsum([(n + 63) // 64 * 64 for n in lens])])
    g = DeviceBatch(e, nbuf=len(lens), buf_len=L)  # its output arrays (cap for 262 144 bytes) and a data area
    g.fill_streams(first_stream=78, bufs_per_stream=len(lens))
    d_offs, d_lens = TE._dev(offs[:-1].astype(np.int64)), TE._dev(np.asarray(lens, np.int32))  # alive until the sync
    e.run_device_ragged(g.data.data_ptr(), int(offs[-1]), d_offs.data_ptr(), d_lens.data_ptr(), len(lens), g.out,
                        stream=torch.cuda.current_stream().cuda_stream)
    counts, st, ln, dg, total = g.host_results()
    loc = torch.arange(total, dtype=torch.int64, device="cuda:0") * 5 + PB
    dst_buf, run_pos = [2, 0, 1, 1, 0], [L - 1, 100, 5000, 150001, 0]
    cap = int(counts[1:].sum())
    r, r_first = inserts_from_runs(g.out, 1, lens[1:], loc, dst_buf, run_pos, 3, L, cap, g.data.device)
    torch.cuda.synchronize()
    want, rec = [], int(counts[0])
    for k in range(1, len(lens)):
        assert int(ln[k, :counts[k]].sum()) == lens[k]
        for i in range(int(counts[k])):
            want.append((dg[k, i].tobytes(), PB + 5 * rec, int(ln[k, i]), run_pos[k - 1] + int(st[k, i]), 0, int(ln[k, i]),
                         dst_buf[k - 1]))
            rec += 1
    assert r_first.tolist() == np.concatenate([[0], np.cumsum(counts[1:])]).tolist()
    h = _host_inserts(r, cap)
    got = [(h[0][32 * i: 32 * i + 32],) + tuple(col[i] for col in h[1:]) for i in range(cap)]
    assert got == want
    # one row short: nothing written, the total reported
    r, r_first = inserts_from_runs(g.out, 1, lens[1:], loc, dst_buf, run_pos, 3, L, cap - 1, g.data.device)
    torch.cuda.synchronize()
    assert r_first[-1].item() == cap and r.dst_buf.tolist() == [3] * (cap - 1) and not r.hash.any() and not r.nlen.any()
    # a run that leaves its buffer is refused on the host
    with pytest.raises(_lib.SdfsCdcError):
        inserts_from_runs(g.out, 1, lens[1:], loc, dst_buf, [L, 100, 5000, 150001, 0], 3, L, cap, g.data.device)
    e.destroy()


@pytest.mark.gpu
def test_gpu_md5_engine():
    from sdfs_amd import write as W

    w = _md5_base()
    fw, rd, m = _open(w)
    files = [(0, NBUF, NBUF * L)]
    reqs, blob = _blob(MIXED[:3], 17)
    res = _write(w, fw, m, NBUF, files, reqs, blob)
    assert res.row_route.tolist() == [W.ROUTE_ACCEL, W.ROUTE_ACCEL, W.ROUTE_FULL, W.ROUTE_ACCEL, W.ROUTE_FULL]
    _check(w, rd, res, m, NBUF, files, reqs, blob, [bytearray(w["data"].tobytes())])
    _done(w, rd)
