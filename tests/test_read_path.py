"""Read path (include/sdfs_read.h): write buffers rebuilt from their map slots.

CPU: hand-worked cases of the plain-Python model (tests/read_model.py, restated from
SparseDataChunk.java:159-174, HashLocPair.java:86-97, WritableCacheBuffer.java:262-278,364-396), the
C-ABI's pair capacity and argument checks.  GPU: parse, plan, the gather kernel's alignment and
placement rules, and the write -> store -> read round trip, every one bit-exact against the model.
Parity status: pinned by the reference's own deserialisation / placement code (no fixtures)."""
import ctypes
import struct

import numpy as np
import pytest

from sdfs_amd import _lib
from tests import read_model as R

H32 = bytes(range(32))
PB = 1 << 33  # pos_base of the GPU tests


def _img(pairs, **kw):
    return R.build_image([(H32,) + tuple(p) for p in pairs], **kw)


# ------------------------------------------------------------------------------------------- CPU

def test_model_hand_worked_cases():
    cl, sb = 64, 13 + 56 * 4
    A, B = bytes(range(100, 120)), bytes(range(200, 230))
    ck = {5: A, 6: B}
    rd = lambda pairs, **kw: R.read_buffer(_img(pairs, **kw), sb, 32, cl, ck)  # noqa: E731
    # one pair
    st, buf = rd([(5, 20, 3, 0, 20)])
    assert st == 0 and buf == bytes(3) + A + bytes(41)
    # a gap stays zero
    st, buf = rd([(5, 20, 0, 0, 4), (6, 30, 10, 2, 5)])
    assert st == 0 and buf == A[:4] + bytes(6) + B[2:7] + bytes(49)
    # overlap: the later pos wins where both cover
    st, buf = rd([(5, 20, 0, 0, 20), (6, 30, 10, 0, 5)])
    assert st == 0 and buf == A[:10] + B[:5] + A[15:20] + bytes(44)
    # nlen > ck.length: offset 0 copies the whole chunk, offset 1 is out of bounds
    st, buf = rd([(5, 20, 1, 0, 1000)])
    assert st == 0 and buf == bytes(1) + A + bytes(43)
    assert rd([(5, 20, 1, 1, 1000)]) == (R.BOUNDS, bytes(cl))
    # pos + c > CHUNK_LENGTH
    assert rd([(5, 20, 45, 0, 20)]) == (R.BOUNDS, bytes(cl))
    assert rd([(5, 20, 44, 0, 20)])[0] == 0
    # a terminator in the middle: the rest is ignored silently
    st, buf = rd([(5, 20, 0, 0, 2), (0, 20, 10, 0, 2), (6, 30, 20, 0, 2)])
    assert st == 0 and buf == A[:2] + bytes(62)
    # duplicate pos: the later one in the image wins; image order does not matter otherwise
    st, buf = rd([(6, 30, 30, 0, 3), (5, 20, 8, 0, 3), (6, 30, 8, 4, 3)])
    assert st == 0 and buf == bytes(8) + B[4:7] + bytes(19) + B[:3] + bytes(31)
    assert [p[3] for p in R.parse(_img([(6, 30, 30, 0, 3), (5, 20, 8, 0, 3), (6, 30, 8, 4, 3)]), sb, 32)[1]] == [8, 30]
    # zlen negative: no pairs
    assert rd([(5, 20, 0, 0, 20)], zlen=-1) == (0, bytes(cl))
    # zlen too large for the slot
    assert rd([(5, 20, 0, 0, 20)], zlen=5) == (R.CORRUPT, bytes(cl))
    # a negative field
    for neg in [(5, -1, 0, 0, 1), (5, 1, -1, 0, 1), (5, 1, 0, -1, 1), (5, 1, 0, 0, -1)]:
        assert rd([(5, 20, 0, 0, 20), neg]) == (R.CORRUPT, bytes(cl))
    # outside the directory / a failed fetch
    assert rd([(7, 20, 0, 0, 20)]) == (R.MISSING, bytes(cl))
    assert R.read_buffer(_img([(5, 20, 0, 0, 20)]), sb, 32, cl, {5: None}) == (R.FETCH, bytes(cl))
    # the free slot
    assert R.read_buffer(bytes(sb), sb, 32, cl, {}) == (0, bytes(cl))


def test_pair_cap_matches_slot_layout():
    lib = _lib.load()
    for slot in (0, 12, 13, 68, 69, 461, 7181, 13 + 56 * 20484):
        for hl in (32, 16):
            want = (slot - 13) // (hl + 24) if slot >= 13 else 0
            assert lib.sdfs_cdc_map_pair_cap(slot, hl) == want, (slot, hl)
    assert lib.sdfs_cdc_map_pair_cap(lib.sdfs_cdc_map_slot_bytes(32, 262144, 4095), 32) == 128


def _fake_pairs(cap=8):
    p = _lib.Pairs(cap=cap)
    for name, _ in _lib.Pairs._fields_[:10]:
        setattr(p, name, 0x1000)  # never dereferenced: every call below fails its argument checks
    return p


def test_new_entry_points_refuse_bad_arguments_before_the_device():
    lib = _lib.load()
    p = _fake_pairs()
    bad = _fake_pairs()
    bad.pos = None
    X = ctypes.c_void_p(0x1000)

    def einval(rc):
        assert rc == _lib.EINVAL
        assert lib.sdfs_cdc_last_error()

    # map_parse
    einval(lib.sdfs_cdc_map_parse(0, 1, X, 461, 32, None, None))
    einval(lib.sdfs_cdc_map_parse(0, 1, X, 461, 32, ctypes.byref(bad), None))
    einval(lib.sdfs_cdc_map_parse(0, 1, X, 461, 20, ctypes.byref(p), None))
    einval(lib.sdfs_cdc_map_parse(0, 1, X, 12, 32, ctypes.byref(p), None))
    einval(lib.sdfs_cdc_map_parse(0, 1, None, 461, 32, ctypes.byref(p), None))
    # read_plan
    einval(lib.sdfs_cdc_read_plan(0, 1, None, 0, 4, X, X, X, X, X, X, X, X, X, None, X, None))
    einval(lib.sdfs_cdc_read_plan(0, 1, ctypes.byref(p), 0, 4, X, X, X, X, None, X, X, X, X, None, X, None))
    einval(lib.sdfs_cdc_read_plan(0, 1, ctypes.byref(p), 0, 4, None, X, X, X, X, X, X, X, X, None, X, None))
    einval(lib.sdfs_cdc_read_plan(0, 1, ctypes.byref(p), 0, 4, X, X, X, X, X, X, X, X, X, None, None, None))
    # read_chain_lens
    einval(lib.sdfs_cdc_read_chain_lens(0, None, None, 4, X, None))
    einval(lib.sdfs_cdc_read_chain_lens(0, X, None, 4, None, None))
    # read_assemble
    einval(lib.sdfs_cdc_read_assemble(0, 1, 4096, None, X, X, X, X, X, None))
    einval(lib.sdfs_cdc_read_assemble(0, 1, 0, ctypes.byref(p), X, X, X, X, X, None))
    einval(lib.sdfs_cdc_read_assemble(0, 1, 4096, ctypes.byref(p), X, X, X, X, None, None))
    einval(lib.sdfs_cdc_read_assemble(0, 1, 4096, ctypes.byref(p), None, X, X, X, X, None))
    # read_verify
    einval(lib.sdfs_cdc_read_verify(None, 1, ctypes.byref(p), 32, X, X, X, X, X, 4, X, X, None))
    einval(lib.sdfs_cdc_read_verify(X, 1, None, 32, X, X, X, X, X, 4, X, X, None))
    einval(lib.sdfs_cdc_read_verify(X, 1, ctypes.byref(p), 20, X, X, X, X, X, 4, X, X, None))
    einval(lib.sdfs_cdc_read_verify(X, 1, ctypes.byref(p), 32, X, X, X, X, X, 4, None, X, None))
    einval(lib.sdfs_cdc_read_verify(ctypes.c_void_p(0x1234567), 1, ctypes.byref(p), 32, X, X, X, X, X, 4, X, X, None))


def test_pairs_struct_layout():
    assert ctypes.sizeof(_lib.Pairs) == 88  # 10 pointers + cap + reserved


# ------------------------------------------------------------------------------------------- GPU

def _dev(a, dt):
    import torch

    t = torch.from_numpy(np.array(a))  # a copy: the source may be a read-only buffer
    return t.to("cuda:0") if dt is None else t.to("cuda:0", dt)


def _slots(images, slot_len):
    buf = np.zeros(len(images) * slot_len, np.uint8)
    for b, img in enumerate(images):
        assert len(img) <= slot_len
        buf[b * slot_len: b * slot_len + len(img)] = np.frombuffer(img, np.uint8)
    return _dev(buf, None)


def _raw_store(chunks):
    """putChunk records of an uncompressed store, [BE32 -1][chunk], one per directory entry; an
    entry of None is a record too short to hold its header (its fetch fails)."""
    import torch

    recs = [b"\x00\x00" if c is None else struct.pack(">i", -1) + c for c in chunks]
    off = np.concatenate([[0], np.cumsum([len(r) + 3 for r in recs[:-1]])]).astype(np.int64)
    store = np.zeros(int(off[-1]) + len(recs[-1]) + 16, np.uint8)
    for o, r in zip(off, recs):
        store[int(o): int(o) + len(r)] = np.frombuffer(r, np.uint8)
    raw = [0 if c is None else len(c) for c in chunks]
    return (_dev(store, None), _dev(off, torch.int64), _dev([len(r) for r in recs], torch.int32),
            _dev(raw, torch.int32))


def _read_and_check(images, slot_len, hash_len, cl, chunks, fill=0xFF):
    """Reads hand-built images through HipBufferReader over a raw store holding `chunks` (a list:
    entry k = the chunk of hashloc PB + k, None = a record that fails) and compares every buffer and
    status with the model."""
    import torch

    from sdfs_amd.read import HipBufferReader

    store, off, ln, raw = _raw_store(chunks)
    nbuf = len(images)
    out = torch.full((nbuf, cl), fill, dtype=torch.uint8, device="cuda:0")
    rd = HipBufferReader(cl, hash_len)
    got, status, info = rd.read(_slots(images, slot_len), nbuf, slot_len, store, off, ln, raw, PB, out=out)
    torch.cuda.synchronize()
    rd.destroy()
    got, status = got.cpu().numpy(), status.cpu().numpy()
    ck = {PB + k: c for k, c in enumerate(chunks)}
    want_status = []
    for b, img in enumerate(images):
        st, buf = R.read_buffer(img, slot_len, hash_len, cl, ck)
        want_status.append(st)
        assert status[b] == st, (b, status[b], st)
        if got[b].tobytes() != buf:
            diff = np.nonzero(got[b] != np.frombuffer(buf, np.uint8))[0]
            raise AssertionError(f"buffer {b}: {len(diff)} bytes differ, first at {diff[0]}")
    return got, want_status, info


@pytest.mark.gpu
@pytest.mark.parametrize("hl", [32, 16])
def test_gpu_parse_vs_model(hl):
    import torch

    from sdfs_amd.read import parse_map_slots

    rng = np.random.default_rng(7 + hl)
    cap = 8
    slot_len = 13 + (hl + 24) * cap

    def pair(pos, **kw):
        ln = int(rng.integers(1, 5000))
        d = dict(digest=rng.bytes(hl), hashloc=int(rng.integers(1, 1 << 62)), ln=ln, pos=pos,
                 offset=int(rng.integers(0, 9)), nlen=int(rng.integers(0, ln + 1)))
        d.update(kw)
        return (d["digest"], d["hashloc"], d["ln"], d["pos"], d["offset"], d["nlen"])

    asc = [pair(1000 * i) for i in range(cap)]
    images = [
        bytes(slot_len),                                                  # a free slot
        R.build_image([pair(77)], doop=5),                                # n = 1
        R.build_image(asc, doop=123456),                                  # n = cap
        R.build_image(asc[::-1], doop=9),                                 # a descending image
        R.build_image([pair(10), pair(500), pair(10), pair(3), pair(500, hashloc=0)]),  # repeated pos
        R.build_image([pair(0), pair(9, nlen=-1)]),                       # CORRUPT
        R.build_image(asc, zlen=cap + 1),                                 # CORRUPT
        R.build_image([pair(5)], zlen=-1, doop=44),                       # no pairs
        R.build_image([pair(1), pair(2)], flags=0x81, doop=3),            # flags carried through
        R.build_image([pair(20), pair(30), pair(25)]),                    # one pair out of order
    ]
    p = parse_map_slots(_slots(images, slot_len), len(images), slot_len, hl)
    torch.cuda.synchronize()
    assert p.cap == cap
    counts, status, flags = (t.cpu().numpy() for t in (p.counts, p.status, p.flags))
    doop = p.doop.cpu().numpy().view(np.uint32)
    hashes, hashloc = p.hashes.cpu().numpy(), p.hashloc.cpu().numpy()
    f4 = [t.cpu().numpy() for t in (p.len, p.pos, p.offset, p.nlen)]
    for b, img in enumerate(images):
        st, pairs, dp, fl = R.parse(img, slot_len, hl)
        assert (status[b], counts[b], doop[b], flags[b]) == (st, len(pairs), dp, fl), b
        for i, (h, loc, ln, pos, off, nlen) in enumerate(pairs):
            assert hashes[b, i, :hl].tobytes() == h and not hashes[b, i, hl:].any(), (b, i)
            assert (int(hashloc[b, i]), f4[0][b, i], f4[1][b, i], f4[2][b, i], f4[3][b, i]) == (loc, ln, pos, off, nlen)
    assert list(status) == [0, 0, 0, 0, 0, 1, 1, 0, 0, 0] and list(counts) == [0, 1, 8, 8, 3, 0, 0, 0, 2, 3]


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["sha256", "md5"])
def test_gpu_parse_inverts_emit(algo):
    import torch

    from sdfs_amd import HipVariableMD5HashEngine, HipVariableSha256HashEngine
    from sdfs_amd.device import DeviceBatch
    from sdfs_amd.index import HipHashesMap
    from sdfs_amd.meta import emit_map_slots, slot_bytes
    from sdfs_amd.read import parse_map_slots

    e = HipVariableMD5HashEngine() if algo == "md5" else HipVariableSha256HashEngine()
    hl = 16 if algo == "md5" else 32
    nbuf, L = 4, 262144
    batch = DeviceBatch(e, nbuf=nbuf, buf_len=L)
    batch.fill_streams(first_stream=321, bufs_per_stream=2)
    batch.data.view(nbuf, L)[3].copy_(batch.data.view(nbuf, L)[0])
    batch.run(buffer_id_base=0)
    ix = HipHashesMap(1 << 12)
    dup, loc, new, nc = ix.put_records(batch.record_table(), batch.total, pos_base=PB)
    m, doop, ovf = emit_map_slots(batch, dup, loc, hash_len=hl)
    sl = slot_bytes(hl, L, 4095)
    p = parse_map_slots(m, nbuf, sl, hl)
    torch.cuda.synchronize()
    counts, st, ln, dg, total = batch.host_results()
    assert int(ovf.item()) == 0 and not p.status.any() and not p.flags.any()
    assert (p.counts.cpu().numpy() == counts).all() and torch.equal(p.doop[:nbuf], doop)
    locs = loc.cpu().numpy()[:total]
    r = 0
    pos, plen, nlen, off = (t.cpu().numpy() for t in (p.pos, p.len, p.nlen, p.offset))
    hashes, hashloc = p.hashes.cpu().numpy(), p.hashloc.cpu().numpy()
    for b in range(nbuf):
        n = int(counts[b])
        assert (pos[b, :n] == st[b, :n]).all() and (plen[b, :n] == ln[b, :n]).all()
        assert (nlen[b, :n] == ln[b, :n]).all() and not off[b, :n].any()
        assert (hashes[b, :n, :hl] == dg[b, :n, :hl]).all() and not hashes[b, :n, hl:].any()
        assert (hashloc[b, :n] == locs[r:r + n]).all()
        r += n
    assert r == total
    ix.destroy()
    e.destroy()


@pytest.mark.gpu
def test_gpu_gather_every_alignment():
    """chunk_length 1027 (no multiple of anything), 256 buffers = every (pos mod 16, source offset
    mod 16); lengths around the 16-byte vector and the 64-lane wave; the last pair ends exactly at
    chunk_length; the output starts as 0xFF."""
    rng = np.random.default_rng(1027)
    cl, cap = 1027, 8
    slot_len = 13 + 56 * cap
    lens = [1, 2, 3, 15, 16, 17, 63, 64, 65, 255]
    chunks = [rng.bytes(400) for _ in range(8)]
    images = []
    for b in range(256):
        pm, om = b % 16, b // 16
        pairs, pos = [], pm
        for i in range(4):
            n = lens[int(rng.integers(0, len(lens)))]
            if i == 3:
                pos = cl - n
            k = int(rng.integers(0, len(chunks)))
            pairs.append((rng.bytes(32), PB + k, 400, pos, om + 16 * int(rng.integers(0, 4)), n))
            pos += n + int(rng.integers(0, 21))
        images.append(R.build_image(sorted(pairs, key=lambda p: p[3])))
    _, status, _ = _read_and_check(images, slot_len, 32, cl, chunks)
    assert not any(status)


@pytest.mark.gpu
def test_gpu_placement_rules():
    rng = np.random.default_rng(4096)
    cl, cap = 4096, 8
    slot_len = 13 + 56 * cap
    chunks = [rng.bytes(1000) for _ in range(4)] + [None]
    P = lambda k, pos, off, nlen: (rng.bytes(32), PB + k if k >= 0 else 0, 1000, pos, off, nlen)  # noqa: E731
    good = lambda: R.build_image([P(0, 0, 0, 1000), P(1, 1000, 3, 997), P(2, 3096, 0, 1000)])  # noqa: E731
    cases = [
        ("gaps", [P(0, 10, 0, 100), P(1, 500, 5, 300), P(2, 4000, 900, 96)], 0),
        ("overlap", [P(0, 0, 0, 600), P(1, 300, 0, 500), P(2, 350, 7, 50), P(3, 790, 0, 20)], 0),
        ("terminator", [P(0, 0, 0, 1000), P(-1, 1000, 0, 1000), P(1, 2000, 0, 1000)], 0),
        ("nlen > ck.length, offset 0", [P(0, 100, 0, 5000)], 0),
        ("nlen > ck.length, offset 1", [P(0, 100, 1, 5000)], R.BOUNDS),
        ("good", None, 0),
        ("pos + c one past the end", [P(1, 0, 0, 10), P(0, 3097, 0, 1000)], R.BOUNDS),
        ("good", None, 0),
        ("pos > chunk_length", [P(0, 4097, 0, 0)], R.BOUNDS),
        ("nlen 0", [P(0, 50, 0, 0), P(1, 60, 1000, 0), P(2, 70, 2, 9), P(3, 4096, 0, 0)], 0),
        ("no pairs", [], 0),
        ("failed fetch", [P(0, 0, 0, 1000), P(4, 1000, 0, 10)], R.FETCH),
        ("good", None, 0),
        ("offset + c > ck.length", [P(0, 0, 991, 10)], R.BOUNDS),
        ("good", None, 0),
    ]
    images = [good() if pairs is None else R.build_image(pairs) for _, pairs, _ in cases]
    got, status, _ = _read_and_check(images, slot_len, 32, cl, chunks)
    assert status == [c[2] for c in cases]
    for b, st in enumerate(status):
        assert (not got[b].any()) == (st != 0 or cases[b][0] == "no pairs"), cases[b][0]


@pytest.mark.gpu
def test_gpu_gather_slots_too_large_for_lds():
    """Slots that hold more than 1024 pairs (the backup profile's hold 20 484) take the gather that
    searches the pair arrays in global memory: 1100-pair slots, buffers of 1050 short pieces with
    gaps and overlaps, one unsorted image, one failed buffer between them."""
    rng = np.random.default_rng(1100)
    cl, cap = 30011, 1100
    slot_len = 13 + 56 * cap
    chunks = [rng.bytes(300) for _ in range(16)]
    images = []
    for b in range(4):
        pairs, pos = [], int(rng.integers(0, 20))
        for _ in range(1050):
            n = int(rng.integers(1, 40))
            if pos + n > cl:
                break
            pairs.append((rng.bytes(32), PB + int(rng.integers(0, 16)), 300, pos, int(rng.integers(0, 200)), n))
            pos += max(1, n + int(rng.integers(-8, 9)))
        assert len(pairs) > 1024
        if b == 2:
            pairs[5], pairs[900] = pairs[900], pairs[5]
        if b == 1:
            pairs[1000] = pairs[1000][:4] + (299, 2)  # offset + c > ck.length
        images.append(R.build_image(pairs))
    _, status, _ = _read_and_check(images, slot_len, 32, cl, chunks)
    assert status == [0, R.BOUNDS, 0, 0]


@pytest.mark.gpu
def test_gpu_plan_lists_each_record_once():
    import torch

    from sdfs_amd.read import parse_map_slots, plan_reads

    rng = np.random.default_rng(3)
    cap, n_store = 8, 10
    slot_len = 13 + 56 * cap
    raw = np.array([100 + 17 * k for k in range(n_store)], np.int32)
    slen = raw + 4 + np.arange(n_store, dtype=np.int32) % 3
    soff = (np.arange(n_store, dtype=np.int64) * 1000 + 5)
    P = lambda loc, pos: (rng.bytes(32), loc, 50, pos, 0, 50)  # noqa: E731
    uses = [[5, 2, 7], [2, 9], [7, 0, 5], [1, -1], [3, n_store], [9, 9]]
    images = [R.build_image([P(PB + k, 100 * i) for i, k in enumerate(u)]) for u in uses]
    # a pair after the terminator is not used, not even when its hashloc is outside the directory
    images.append(R.build_image([P(PB + 6, 0), P(0, 100), P(PB + 4, 200), P(5, 300)]))
    nbuf = len(images)
    p = parse_map_slots(_slots(images, slot_len), nbuf, slot_len, 32)
    plan = plan_reads(p, _dev(soff, torch.int64), _dev(slen, torch.int32), _dev(raw, torch.int32), PB)
    torch.cuda.synchronize()
    want = [0, 2, 5, 6, 7, 9]
    k = int(plan["fetch_count"].item())
    assert k == len(want)
    assert plan["src_off"][:k].tolist() == [int(soff[i]) for i in want]
    assert plan["src_len"][:k].tolist() == [int(slen[i]) for i in want]
    assert plan["dst_cap"][:k].tolist() == [int(raw[i]) for i in want]
    r16 = lambda v: (int(v) + 15) // 16 * 16  # noqa: E731
    assert plan["dst_off"][:k].tolist() == [sum(r16(raw[j]) for j in want[:i]) for i in range(k)]
    assert plan["plain_off"][:k].tolist() == [sum(r16(slen[j]) for j in want[:i]) for i in range(k)]
    assert plan["total_bytes"].tolist() == [sum(r16(raw[j]) for j in want), sum(r16(slen[j]) for j in want)]
    assert p.status.tolist() == [0, 0, 0, R.MISSING, R.MISSING, 0, 0]
    pf = plan["pair_fetch"].cpu().numpy()
    rank = {idx: f for f, idx in enumerate(want)}
    for b, u in enumerate(uses):
        row = [rank[x] for x in u] if b not in (3, 4) else []
        assert pf[b].tolist() == row + [-1] * (cap - len(row)), b
    assert pf[6].tolist() == [rank[6]] + [-1] * (cap - 1)


# ---- the write path of the round-trip tests: 8 x 256 KiB buffers, the upper half copies of the
# lower half, a 100 KB zero run, through the index, LZ4 framing, AES and the map images

_KEY, _IV = bytes(range(7, 39)), bytes(range(90, 106))
_WRITTEN = {}


def _written(variant, algo="sha256"):
    """variant: raw (framed, uncompressed), lz4, aes (LZ4 + AES-256).  Computed once per variant
    and shared; the tests that damage the store work on a copy."""
    if (variant, algo) in _WRITTEN:
        return _WRITTEN[(variant, algo)]
    import torch

    from sdfs_amd import HipVariableMD5HashEngine, HipVariableSha256HashEngine
    from sdfs_amd.aes import HipEncryptUtils, cbc_bound
    from sdfs_amd.device import DeviceBatch
    from sdfs_amd.index import HipHashesMap
    from sdfs_amd.lz4 import HipLz4Compressor
    from sdfs_amd.meta import emit_map_slots, slot_bytes

    e = HipVariableMD5HashEngine() if algo == "md5" else HipVariableSha256HashEngine()
    hl = 16 if algo == "md5" else 32
    nbuf, L = 8, 262144
    batch = DeviceBatch(e, nbuf=nbuf, buf_len=L)
    batch.fill_streams(first_stream=4242, bufs_per_stream=2)
    v = batch.data.view(nbuf, L)
    v[1, 20000:120000] = 0
    for b in range(nbuf // 2, nbuf):
        v[b].copy_(v[b - nbuf // 2])
    batch.run(buffer_id_base=0)
    recs = batch.record_table()
    ix = HipHashesMap(1 << 12)
    dup, loc, new, nc = ix.put_records(recs, batch.total, pos_base=PB)
    z = HipLz4Compressor()
    cnt = nc.view(torch.int32)
    src_off, src_len, dst_off, total = z.plan_records(recs, sel=new[: recs.shape[0]], count=cnt, uniform_len=L)
    k = int(nc.item())
    src_off, src_len, dst_off = src_off[:k].contiguous(), src_len[:k].contiguous(), dst_off[:k].contiguous()
    host = batch.data.cpu().numpy()
    so, sl = src_off.cpu().numpy(), src_len.cpu().numpy()
    chunks = [host[int(o): int(o) + int(n)].tobytes() for o, n in zip(so, sl)]
    if variant == "raw":
        store, store_off, store_len, _ = _raw_store(chunks)
    else:
        store = torch.zeros(int(total.item()) + 16, dtype=torch.uint8, device="cuda:0")
        store_len = torch.zeros(k, dtype=torch.int32, device="cuda:0")
        z.compress_device(batch.data, src_off, src_len, store, dst_off, store_len, framed=True)
        store_off = dst_off
        if variant == "aes":
            room = np.array([cbc_bound(int(n)) for n in store_len.cpu().numpy()], np.int64)
            aoff = _dev(np.concatenate([[0], np.cumsum(room[:-1])]), torch.int64)
            aout = torch.zeros(int(room.sum()) + 16, dtype=torch.uint8, device="cuda:0")
            alen = torch.zeros(k, dtype=torch.int32, device="cuda:0")
            c = HipEncryptUtils(_KEY)
            c.encrypt_device(store, store_off, store_len, aout, aoff, alen, iv=_IV)
            torch.cuda.synchronize()
            c.destroy()
            store, store_off, store_len = aout, aoff, alen
    m, doop, ovf = emit_map_slots(batch, dup, loc, hash_len=hl)
    torch.cuda.synchronize()
    assert int(ovf.item()) == 0
    w = dict(engine=e, hl=hl, nbuf=nbuf, L=L, data=host.reshape(nbuf, L), m=m, slot_len=slot_bytes(hl, L, 4095),
             store=store, store_off=store_off, store_len=store_len, raw=src_len, k=k, chunks=chunks,
             loc=loc.cpu().numpy()[: int(batch.total.item())], counts=batch.counts.cpu().numpy())
    z.destroy()
    ix.destroy()
    _WRITTEN[(variant, algo)] = w
    return w


def _reader(w, variant):
    from sdfs_amd.read import HipBufferReader

    return HipBufferReader(w["L"], w["hl"], aes=_KEY if variant == "aes" else None,
                           iv=_IV if variant == "aes" else None, engine=w["engine"])


@pytest.mark.gpu
@pytest.mark.parametrize("variant,algo", [("raw", "sha256"), ("lz4", "sha256"), ("aes", "sha256"), ("lz4", "md5")])
def test_gpu_write_store_read_round_trip(variant, algo):
    import torch

    w = _written(variant, algo)
    rd = _reader(w, variant)
    out = torch.full((w["nbuf"], w["L"]), 0xFF, dtype=torch.uint8, device="cuda:0")
    got, status, info = rd.read(w["m"], w["nbuf"], w["slot_len"], w["store"], w["store_off"], w["store_len"],
                                w["raw"], PB, verify=True, out=out)
    torch.cuda.synchronize()
    rd.destroy()
    assert not status.any()
    assert (got.cpu().numpy() == w["data"]).all()
    assert info.fetch_count == w["k"]  # every inserted record, each once
    assert not info.bad_count.any() and not info.pair_bad.any()
    assert (w["data"][1, 20000:120000] == 0).all() and w["k"] < int(w["counts"].sum()) // 2 + 1


@pytest.mark.gpu
def test_gpu_partial_rewrite_images():
    """Pairs with offset != 0 and nlen < len (what a partial rewrite of a block leaves behind) into
    the chunks the write path stored; the model is fed the original chunk bytes."""
    import torch

    w = _written("lz4")
    rng = np.random.default_rng(66)
    k, cap = w["k"], (w["slot_len"] - 13) // 56
    ck = {PB + i: c for i, c in enumerate(w["chunks"])}
    images = []
    for b in range(4):
        pairs, pos = [], int(rng.integers(0, 40))
        for _ in range(int(rng.integers(3, 30))):
            i = int(rng.integers(0, k))
            n = len(w["chunks"][i])
            if n < 4:
                continue
            off = int(rng.integers(1, min(n, 300)))
            nlen = int(rng.integers(1, n - off + 1))
            if pos + nlen > w["L"]:
                break
            pairs.append((rng.bytes(32), PB + i, n, pos, off, nlen))
            pos += nlen - int(rng.integers(0, 3)) * int(rng.integers(0, 50)) + int(rng.integers(0, 100))
            pos = max(pos, pairs[-1][3] + 1)
        assert len(pairs) <= cap
        images.append(R.build_image(pairs))
    rd = _reader(w, "lz4")
    got, status, _ = rd.read(_slots(images, w["slot_len"]), len(images), w["slot_len"], w["store"], w["store_off"],
                             w["store_len"], w["raw"], PB)
    torch.cuda.synchronize()
    rd.destroy()
    got = got.cpu().numpy()
    for b, img in enumerate(images):
        st, buf = R.read_buffer(img, w["slot_len"], 32, w["L"], ck)
        assert st == 0 and int(status[b]) == 0
        assert got[b].tobytes() == buf, b


def _referencing(w, idx):
    """Buffers with a pair whose hashloc is PB + idx."""
    out, r = [], 0
    for b, n in enumerate(w["counts"]):
        if (w["loc"][r:r + int(n)] == PB + idx).any():
            out.append(b)
        r += int(n)
    return out


@pytest.mark.gpu
def test_gpu_bad_padding_does_not_travel():
    """One stored record's last ciphertext block overwritten: the decryptor reports 0xFFFFFFFF, which
    must reach the decoder as length 0 (read_chain_lens), not as a 4 GiB record."""
    import torch

    from oracle import aes_oracle as A

    w = _written("aes")
    j = w["k"] // 3
    off, n = int(w["store_off"][j].item()), int(w["store_len"][j].item())
    rec = w["store"][off: off + n].cpu().numpy().tobytes()
    for seed in range(16):  # a last block whose padding the reference cipher refuses
        blk = bytes((seed * 37 + 11 * i + 1) & 255 for i in range(16))
        try:
            A.cbc_decrypt(_KEY, _IV, rec[:-16] + blk)
        except ValueError:
            break
    else:
        raise AssertionError("no bad-padding block found")
    store = w["store"].clone()
    store[off + n - 16: off + n] = _dev(np.frombuffer(blk, np.uint8), None)
    rd = _reader(w, "aes")
    got, status, info = rd.read(w["m"], w["nbuf"], w["slot_len"], store, w["store_off"], w["store_len"], w["raw"], PB)
    torch.cuda.synchronize()
    rd.destroy()
    hit = _referencing(w, j)
    assert hit and len(hit) < w["nbuf"]
    got, status = got.cpu().numpy(), status.cpu().numpy()
    for b in range(w["nbuf"]):
        if b in hit:
            assert status[b] == R.FETCH and not got[b].any(), b
        else:
            assert status[b] == 0 and (got[b] == w["data"][b]).all(), b


@pytest.mark.gpu
def test_gpu_verify_marks_a_flipped_chunk():
    import torch

    w = _written("raw")
    j = next(i for i in range(w["k"] // 2, w["k"]) if len(w["chunks"][i]) >= 64)
    off = int(w["store_off"][j].item())
    store = w["store"].clone()
    store[off + 4 + 10] ^= 0x40  # payload byte 10 of record j
    rd = _reader(w, "raw")
    got, status, info = rd.read(w["m"], w["nbuf"], w["slot_len"], store, w["store_off"], w["store_len"], w["raw"], PB,
                                verify=True)
    torch.cuda.synchronize()
    rd.destroy()
    assert not status.any()  # the reference only logs the mismatch
    bad = info.pair_bad.cpu().numpy()
    want = np.zeros_like(bad)
    r = 0
    pos = info.pairs.pos.cpu().numpy()
    flipped = w["data"].copy()
    for b, n in enumerate(w["counts"]):
        for i in range(int(n)):
            if w["loc"][r + i] == PB + j:
                want[b, i] = 1
                flipped[b, pos[b, i] + 10] ^= 0x40
        r += int(n)
    assert want.sum() >= 2 and (bad == want).all()
    assert info.bad_count.tolist() == want.sum(axis=1).tolist()
    assert (got.cpu().numpy() == flipped).all()
