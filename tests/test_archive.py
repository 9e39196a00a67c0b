"""Chunk store layer (include/sdfs_archive.h): archive images, .map images, compaction.

CPU: the plain-Python model (tests/archive_model.py, restated from HashBlobArchive.java,
SimpleByteArrayLongMap.java and NextPrime.java) against bytes typed out by hand, the C-ABI's
map size against the model, argument checks.  GPU: plan, pack, map image, the write -> archive ->
read round trip and compaction after a sweep, every image and map byte for byte against the model.
Parity status: pinned by the reference's own serialisation code (no fixtures)."""
import ctypes
import struct

import numpy as np
import pytest

from sdfs_amd import _lib
from tests import archive_model as M

PB = 1 << 33
NONE = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------- CPU

def test_model_archive_against_hand_written_bytes():
    k = [bytes([0x10 * (i + 1) + j for j in range(32)]) for i in range(3)]
    recs = [b"\xff\xff\xff\xffAB", b"", b"\x00\x00\x00\x03xyz"]
    keyhex = [x.hex() for x in k]
    body = ("00000020" + keyhex[0] + "00000006" + "ffffffff4142"
            + "00000020" + keyhex[1] + "00000000"
            + "00000020" + keyhex[2] + "00000007" + "00000003" + "78797a")
    a0 = M.Archive(11, 1000, 0, 32)
    pos0 = [a0.put(x, r) for x, r in zip(k, recs)]
    assert bytes(a0.data).hex() == body
    assert pos0 == [40, 86, 126] and a0.np == 133
    assert [a0.map.get(x) for x in k] == [36, 82, 122]  # cp + 4 + hash.length
    iv = bytes(range(0xA0, 0xB0))
    a1 = M.Archive(11, 5000, 1, 32, iv)
    pos1 = [a1.put(x, r) for x, r in zip(k, recs)]
    assert bytes(a1.data).hex() == "00000001" + iv.hex() + "00" * 1004 + body
    assert pos1 == [1064, 1110, 1150]
    assert [a1.map.get(x) for x in k] == [(1060 << 32) | 6, (1106 << 32) | 0, (1146 << 32) | 7]
    assert [a1.get_record(x) for x in k] == recs and a1.get_record(bytes(32)) is None
    assert [(key, rec) for key, rec, _ in a1.walk()] == list(zip(k, recs))
    # the two "full" checks: np >= blocksz before the put; entries >= (int)(size * .75)
    small = M.Archive(11, 46, 0, 32)
    small.put(k[0], recs[0])  # np = 46
    with pytest.raises(M.ArchiveFull):
        small.put(k[1], recs[1])
    few = M.Archive(3, 1000, 0, 32)  # 3 slots, limit 2
    few.put(k[0], b"")
    few.put(k[1], b"")
    with pytest.raises(M.ArchiveFull):
        few.put(k[2], b"")


def _key(h, fill, n=16):
    """A key whose BE32 at bytes 8..12 is h."""
    return bytes([fill] * 8) + struct.pack(">I", h) + bytes([fill] * (n - 12))


def test_model_map_against_hand_written_bytes():
    # 7 slots: home = h % 7, step = 1 + h % 5, backwards
    a = _key(10, 0xA1)  # home 3, step 1
    b = _key(17, 0xB2)  # home 3, step 3 -> 0
    c = _key(45, 0xC3)  # home 3, step 1 (shares home and probe with a) -> 2
    d = _key(0x80000000 | 24, 0xD4)  # sign bit masked off: h = 24, home 3, step 5 -> 5
    m = M.SlotMap(7, 0, 16)
    for i, key in enumerate((a, b, c, d)):
        assert m.put(key, 100 + i)
    assert not m.put(c, 999)  # already stored
    want = [b, None, c, a, None, d, None]
    assert [s[0] if s else None for s in m.slots] == want
    hexs = {0: b.hex() + "00000065", 2: c.hex() + "00000066", 3: a.hex() + "00000064", 5: d.hex() + "00000067"}
    assert m.image().hex() == "".join(hexs.get(i, "00" * 20) for i in range(7))
    assert [m.get(x) for x in (a, b, c, d)] == [100, 101, 102, 103] and m.get(_key(3, 0xEE)) == -1
    assert [e[0] for e in m.entries()] == [b, c, a, d]  # next(): slot order, not put order
    # another order, another image
    m2 = M.SlotMap(7, 0, 16)
    for i, key in enumerate((c, a, b, d)):
        m2.put(key, i)
    assert [s[0] if s else None for s in m2.slots] == [b, None, a, c, None, d, None]
    # version 1: header, 8-byte values
    m3 = M.SlotMap(6, 1, 16)  # getNextPrimeI(6) = 7
    m3.put(a, (36 << 32) | 9)
    assert m3.size == 7
    assert m3.image().hex() == ("0000192a" + "00000001" + "00" * 8 + "00" * 24 * 3 + a.hex() + "00000024" + "00000009"
                                + "00" * 24 * 3)
    back = M.SlotMap.from_image(m3.image(), 1, 16)
    assert back.size == 7 and back.get(a) == (36 << 32) | 9


def test_map_size_equals_next_prime():
    lib = _lib.load()
    from sdfs_amd.archive import max_hm_sz

    for sz in range(0, 301):
        assert lib.sdfs_cdc_archive_map_size(sz) == M.next_prime_i(sz), sz
    assert [lib.sdfs_cdc_archive_map_size(x) for x in (0, 2, 3, 4, 5, 6, 7, 8, 9, 24, 90)] == \
        [2, 2, 3, 5, 5, 7, 7, 11, 11, 29, 97]
    d, b = _lib.default_params(), _lib.default_params(backup_volume=True)
    for hm in (max_hm_sz(d.min_len), max_hm_sz(b.min_len)):
        for sz in range(hm - 3, hm + 4):
            assert lib.sdfs_cdc_archive_map_size(sz) == M.next_prime_i(sz), sz
        live = int(M.next_prime_i(hm) * .75)
        assert lib.sdfs_cdc_archive_map_size(2 * live + 5) == M.next_prime_i(2 * live + 5)
    assert max_hm_sz(4095) == 8534  # (int)((26214400 / 4095) / .75f)
    for sz in (2 ** 31 - 2, 2 ** 31 - 1):
        assert lib.sdfs_cdc_archive_map_size(sz) == 2 ** 31 - 1 == M.next_prime_i(sz)
    assert lib.sdfs_cdc_archive_map_size(2 ** 31) == 0 == M.next_prime_i(2 ** 31)
    assert lib.sdfs_cdc_archive_map_size(2 ** 40) == 0


def test_archive_entry_points_refuse_bad_arguments_before_the_device():
    lib = _lib.load()
    X = 0x1000  # never dereferenced: every call below fails its argument checks
    lay = _lib.ArchiveLayout(arc=X, pos=X, store_off=X, arc_first=X, arc_bytes=X, arc_base=X, totals=X, status=X,
                             arc_cap=4)
    bad = _lib.ArchiveLayout.from_buffer_copy(lay)
    bad.arc_base = None
    kept = _lib.ArchiveKept(new_of_old=X, sel=X, src_off=X, rec_len=X, count=X, deleted=X, new_arc=X, map_slots=X,
                            lay=lay)
    blk = lambda *v: (ctypes.c_uint64 * len(v))(*v)  # noqa: E731
    L, B, K = ctypes.byref(lay), ctypes.byref(bad), ctypes.byref(kept)

    def einval(rc):
        assert rc == _lib.EINVAL
        assert lib.sdfs_cdc_last_error()

    einval(lib.sdfs_cdc_archive_plan(0, X, None, 4, 32, 0, blk(1 << 31), 1, 11, L, None))  # the v0 map value is an int
    einval(lib.sdfs_cdc_archive_plan(0, X, None, 4, 32, 1024, blk(5000, 1024), 2, 11, L, None))
    einval(lib.sdfs_cdc_archive_plan(0, X, None, 4, 32, 0, blk(5000), 0, 11, L, None))
    einval(lib.sdfs_cdc_archive_plan(0, X, None, 4, 24, 0, blk(5000), 1, 11, L, None))
    einval(lib.sdfs_cdc_archive_plan(0, X, None, 4, 32, 512, blk(5000), 1, 11, L, None))
    einval(lib.sdfs_cdc_archive_plan(0, X, None, 4, 32, 0, blk(5000), 1, 1, L, None))
    einval(lib.sdfs_cdc_archive_plan(0, X, None, 4, 32, 0, blk(5000), 1, 11, B, None))
    einval(lib.sdfs_cdc_archive_plan(0, None, None, 4, 32, 0, blk(5000), 1, 11, L, None))
    einval(lib.sdfs_cdc_archive_pack(0, L, None, 4, 0x1008, X, X, 0, X, None, 32, 0, 0, None, X, 64, None))  # alignment
    einval(lib.sdfs_cdc_archive_pack(0, L, None, 4, X, X, X, 0, X, None, 32, 1024, 1, None, X, 64, None))  # no IVs
    einval(lib.sdfs_cdc_archive_pack(0, L, None, 4, X, None, X, 0, X, None, 32, 0, 0, None, X, 64, None))
    einval(lib.sdfs_cdc_archive_pack(0, B, None, 4, X, X, X, 0, X, None, 32, 0, 0, None, X, 64, None))
    einval(lib.sdfs_cdc_archive_map_emit(0, L, None, 4, X, X, None, 20, 0, None, 11, X, X, X, None))  # hashLength 18
    einval(lib.sdfs_cdc_archive_map_emit(0, L, None, 4, X, X, None, 32, 0, None, 2, X, X, X, None))
    einval(lib.sdfs_cdc_archive_map_emit(0, L, None, 4, X, X, None, 32, 0, None, 11, None, X, X, None))
    einval(lib.sdfs_cdc_archive_compact_select(0, L, 4, 5, X, None, X, None, 11, X, 32, 0, K, None))  # n_arc > arc_cap
    einval(lib.sdfs_cdc_archive_compact_select(0, L, 4, 2, X, None, X, None, 11, None, 32, 0, K, None))
    einval(lib.sdfs_cdc_archive_compact(0, L, 4, 2, X, X, None, X, None, 11, X, X, 20, 0, 0, None, K, X, 64, 11, X, X, X,
                                        None))
    assert lib.sdfs_cdc_archive_pack_span() % 16 == 0
    assert lib.sdfs_cdc_archive_map_bytes(7, 16, 0) == 140 and lib.sdfs_cdc_archive_map_bytes(7, 32, 1) == 16 + 280
    assert ctypes.sizeof(_lib.ArchiveLayout) == 72 and ctypes.sizeof(_lib.ArchiveKept) == 136


# ------------------------------------------------------------------------------------------- GPU

def _dev(a, dt=None):
    import torch

    t = torch.from_numpy(np.array(a))
    return t.to("cuda:0") if dt is None else t.to("cuda:0", dt)


def _records(keys):
    """48-byte fingerprint records holding the keys (zero-padded to 32; the rest is not looked at)."""
    t = np.zeros((max(len(keys), 1), 48), np.uint8)
    for i, k in enumerate(keys):
        t[i, :len(k)] = np.frombuffer(k, np.uint8)
        t[i, 32:] = 0xEE
    return _dev(t)


def _keys(rng, n, hl):
    return [rng.bytes(hl) for _ in range(n)]


def _model_store(keys, payloads, hl, version, blocksz, map_slots, ivs=None):
    st = M.Store(map_slots, blocksz, version, hl, (lambda a: ivs[a]) if ivs else None)
    for k, p in zip(keys, payloads):
        st.put(k, p)
    return st


def _check_layout(lay, st, n, header):
    """Every output of the plan against the model store."""
    import torch

    torch.cuda.synchronize()
    na = len(st.archives)
    bs, end = M.bases(st.archives)
    assert lay.status.item() == 0
    assert lay.totals.tolist() == [na, end if na else 0]
    assert lay.arc[:n].tolist() == [w[0] for w in st.where]
    assert lay.pos[:n].tolist() == [w[1] for w in st.where]
    assert lay.store_off[:n].tolist() == [bs[w[0]] + w[1] for w in st.where]
    first = [0]
    for a in st.archives:
        first.append(first[-1] + len(a.order))
    assert lay.arc_first[: na + 1].tolist() == first
    assert lay.arc_bytes[:na].tolist() == [len(a.data) for a in st.archives]
    assert lay.arc_base[:na].tolist() == bs
    assert all(b % 4096 == 0 for b in bs)


def _edge_lens(header, blk, hl, rng):
    """Record lengths that walk the archive-full rule's edges; blk = the blocksz list."""
    unit = 8 + hl
    B = lambda a: blk[min(a, len(blk) - 1)]  # noqa: E731
    lens = [500, B(0) - header - 2 * unit - 500]      # archive 0 ends exactly at np == blocksz: the next record rolls
    lens += [B(1) - header - unit - 1, 700]           # archive 1: one byte short, the next is accepted and overshoots
    lens += [B(2) + 500]                              # archive 2: a first record larger than blocksz
    lens += [100, B(3) + 1000]                        # archive 3: such a record as a non-first one
    lens += [int(x) for x in rng.integers(0, 400, 33)]
    return lens


@pytest.mark.gpu
@pytest.mark.parametrize("header", [0, 1024])
@pytest.mark.parametrize("blk", [[3000], [3000, 3500, 2800]])
def test_gpu_plan_walks_the_archive_full_rule(header, blk):
    from sdfs_amd.archive import HipBlobArchiver

    rng = np.random.default_rng(40 + header + len(blk))
    hl = 32
    lens = _edge_lens(header, blk, hl, rng)
    n = len(lens)
    keys = _keys(rng, n, hl)
    st = _model_store(keys, [bytes(x) for x in lens], hl, 1 if header else 0, blk, 8537)
    assert 5 <= len(st.archives) <= 12
    assert len(st.archives[0].data) == blk[0] and len(st.archives[1].data) > blk[min(1, len(blk) - 1)]
    assert len(st.archives[2].order) == 1 and len(st.archives[3].order) == 2
    A = HipBlobArchiver(hl, 1 if header else 0, blk, 8537)
    import torch

    lay = A.plan(_dev(lens, torch.int32), arc_cap=16)
    _check_layout(lay, st, n, header)
    # a device count below n_max: only that many records are planned
    cnt = _dev([n - 9], torch.int32)
    lay = A.plan(_dev(lens, torch.int32), count=cnt, arc_cap=16)
    st2 = _model_store(keys[: n - 9], [bytes(x) for x in lens[: n - 9]], hl, 1 if header else 0, blk, 8537)
    _check_layout(lay, st2, n - 9, header)


@pytest.mark.gpu
def test_gpu_plan_entry_limit_empty_batch_and_arc_cap():
    import torch

    from sdfs_amd.archive import HipBlobArchiver, Layout

    rng = np.random.default_rng(7)
    hl, n = 16, 23
    lens = [int(x) for x in rng.integers(0, 40, n)]
    keys = _keys(rng, n, hl)
    # map_slots 7: limit (int)(7 * .75) = 5 entries, long before 100 000 bytes
    st = _model_store(keys, [bytes(x) for x in lens], hl, 0, 100000, 7)
    assert [len(a.order) for a in st.archives] == [5, 5, 5, 5, 3]
    A = HipBlobArchiver(hl, 0, 100000, 7)
    d_lens = _dev(lens, torch.int32)
    _check_layout(A.plan(d_lens, arc_cap=5), st, n, 0)  # arc_cap == n_arc still fits
    # n = 0
    lay = A.plan(torch.zeros(0, dtype=torch.int32, device="cuda:0"), arc_cap=3)
    torch.cuda.synchronize()
    assert lay.totals.tolist() == [0, 0] and lay.status.item() == 0 and lay.arc_first[0].item() == 0
    # arc_cap too small: the status word, and nothing else
    lay = Layout(n, 4, "cuda:0")
    for t in (lay.arc, lay.pos, lay.store_off, lay.arc_first, lay.arc_bytes, lay.arc_base, lay.totals):
        t.fill_(-7)
    A.plan(d_lens, lay=lay)
    torch.cuda.synchronize()
    assert lay.status.item() == _lib.ARCHIVE_ECAP
    for t in (lay.arc, lay.pos, lay.store_off, lay.arc_first, lay.arc_bytes, lay.arc_base, lay.totals):
        assert (t == -7).all()
    with pytest.raises(_lib.SdfsCdcError):
        lay.read_totals()


def _sparse_source(rng, payloads):
    """The records' bytes at offsets that take every residue mod 16 in turn, 0xA7 between them; the
    area is 16-byte aligned and ends on a 16-byte boundary."""
    offs, cur = [], 0
    for i, p in enumerate(payloads):
        want = (5 * i + 3) % 16
        cur += (want - cur) % 16
        offs.append(cur)
        cur += len(p) + int(rng.integers(0, 40))
    area = np.full((cur + 15) // 16 * 16 + 16, 0xA7, np.uint8)
    for o, p in zip(offs, payloads):
        area[o: o + len(p)] = np.frombuffer(p, np.uint8)
    return area, offs


def _pack_and_check(A, keys, payloads, rng, sel_perm=False, ivs=None, raw_frame=False, shift=0, arc_cap=64):
    """plan + pack of `payloads` under `keys` through HipBlobArchiver against the model: the whole
    [0, store_bytes) region, padding included, and the 64 canary bytes behind it."""
    import torch

    n = len(keys)
    area, offs = _sparse_source(rng, payloads)
    order = list(rng.permutation(n)) if sel_perm else list(range(n))  # record i's digest sits in table row order[i]
    table = [None] * n
    for i, r in enumerate(order):
        table[r] = keys[i]
    recs = _records(table)
    sel = _dev(np.array(order, np.int32)) if sel_perm else None
    src_len = _dev([len(p) for p in payloads], torch.int32)
    stored = [b"\xff\xff\xff\xff" + p for p in payloads] if raw_frame else payloads
    st = _model_store(keys, stored, A.hash_len, A.version, A.blocksz, A.map_slots, ivs)
    want = M.store_image(st.archives)
    lay = A.plan(src_len + 4 if raw_frame else src_len, arc_cap=arc_cap)
    n_arc, store_bytes, _ = lay.read_totals()
    assert (n_arc, store_bytes) == (len(st.archives), len(want))
    buf = torch.full((shift + store_bytes + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
    d_ivs = _dev(np.frombuffer(b"".join(ivs), np.uint8).reshape(-1, 16)) if ivs else None
    A.pack(lay, _dev(area), _dev(offs, torch.int64), src_len, recs, sel, ivs=d_ivs, store=buf[shift:],
           store_bytes=store_bytes, raw_frame=raw_frame)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:shift] == 0x5A).all() and (got[shift + store_bytes:] == 0x5A).all(), "wrote outside the store"
    body = got[shift: shift + store_bytes]
    if body.tobytes() != want:
        diff = np.nonzero(body != np.frombuffer(want, np.uint8))[0]
        raise AssertionError(f"{len(diff)} bytes differ, first at {diff[0]} of {store_bytes}")
    return st, lay


EDGE_LENS = [0, 1, 15, 16, 17, 63, 64, 65, 4099, 32772]


@pytest.mark.gpu
@pytest.mark.parametrize("hl", [16, 20, 32])
def test_gpu_pack_every_header_phase(hl):
    """A leading record of every length 0 .. 8 + hash_len + 16 puts the headers behind it at every
    phase of a 16-byte vector; the store itself starts at every 16-byte phase in turn."""
    from sdfs_amd.archive import HipBlobArchiver

    rng = np.random.default_rng(hl)
    A = HipBlobArchiver(hl, 0, 1 << 20, 97)
    for lead in range(0, 8 + hl + 16 + 1):
        lens = [lead, 0, 1, 15, 16, 17, 63, 64, 65, int(rng.integers(0, 300))]
        payloads = [rng.bytes(x) for x in lens]
        _pack_and_check(A, _keys(rng, len(lens), hl), payloads, rng, shift=lead % 16)


@pytest.mark.gpu
@pytest.mark.parametrize("hl,version,sel_perm", [(32, 0, False), (32, 1, True), (16, 1, False), (20, 0, True)])
def test_gpu_pack_spans_one_archive(hl, version, sel_perm):
    """One archive over more than three workgroup spans; a record header and a record's bytes each
    straddle a span boundary."""
    from sdfs_amd.archive import HipBlobArchiver, pack_span

    rng = np.random.default_rng(100 + hl + version)
    span, unit, header = pack_span(), 8 + hl, 1024 if version else 0
    lens = [span - 20 - header - unit, 70000] + EDGE_LENS + [int(x) for x in rng.integers(0, 9000, 12)]
    payloads = [rng.bytes(x) for x in lens]
    ivs = [rng.bytes(16)] if version else None
    A = HipBlobArchiver(hl, version, 1 << 24, 97)
    st, lay = _pack_and_check(A, _keys(rng, len(lens), hl), payloads, rng, sel_perm=sel_perm, ivs=ivs)
    assert len(st.archives) == 1 and len(st.archives[0].data) >= 3 * span
    p1 = st.where[1][1]  # the second record's bytes start here, its header 8 + hash_len before
    assert p1 - unit < span < p1 and p1 < 2 * span < p1 + 70000


@pytest.mark.gpu
@pytest.mark.parametrize("hl,version,raw", [(32, 0, False), (32, 1, False), (16, 0, True)])
def test_gpu_pack_several_archives(hl, version, raw):
    """Archives of about 40 000 bytes: headers, padding up to the next multiple of 4096, and a
    store that does not start at a 16-byte address."""
    from sdfs_amd.archive import HipBlobArchiver

    rng = np.random.default_rng(200 + hl + version)
    lens = EDGE_LENS + [int(x) for x in rng.integers(0, 9000, 40)]
    order = rng.permutation(len(lens))
    payloads = [rng.bytes(lens[i]) for i in order]
    ivs = [rng.bytes(16) for _ in range(64)] if version else None
    A = HipBlobArchiver(hl, version, [40000, 30000, 50000], 97)
    st, _ = _pack_and_check(A, _keys(rng, len(lens), hl), payloads, rng, sel_perm=True, ivs=ivs, raw_frame=raw, shift=5)
    assert len(st.archives) >= 4


@pytest.mark.gpu
def test_gpu_pack_more_short_records_than_a_span_stages():
    """3 000 records of 0 .. 3 bytes: a 64 KiB span holds about 2 600 of them, more than the kernel
    keeps in LDS, so it searches the record arrays in global memory."""
    from sdfs_amd.archive import HipBlobArchiver, pack_span

    rng = np.random.default_rng(3000)
    hl, n = 16, 3000
    payloads = [rng.bytes(int(x)) for x in rng.integers(0, 4, n)]
    assert pack_span() // (8 + hl + 2) > 1024
    st, _ = _pack_and_check(HipBlobArchiver(hl, 0, 1 << 24, 4099), _keys(rng, n, hl), payloads, rng, sel_perm=True)
    assert len(st.archives) == 1 and len(st.archives[0].data) > pack_span()


def _emit_and_check(A, keys, lens, version_keys_order=None, arc_cap=8):
    """plan + map_emit against the model's map images; -> (images, slot_rec rows, info)."""
    import torch

    n = len(keys)
    d_lens = _dev(np.array(lens, np.int32).reshape(-1)) if n else torch.zeros(0, dtype=torch.int32, device="cuda:0")
    lay = A.plan(d_lens, arc_cap=arc_cap)
    n_arc, _, _ = lay.read_totals()
    maps, slot_rec, info = A.map_emit(lay, d_lens, _records(keys), n_arc=n_arc)
    torch.cuda.synchronize()
    st = _model_store(keys, [bytes(x) for x in lens], A.hash_len, A.version, A.blocksz, A.map_slots)
    assert n_arc == len(st.archives)
    maps, slot_rec = maps.cpu().numpy(), slot_rec.cpu().numpy().view(np.uint32)
    first = 0
    images = []
    for a, arc in enumerate(st.archives):
        img = maps[a].tobytes()
        assert img == arc.map.image(), f"map image of archive {a} differs"
        images.append(img)
        # slot_rec is consistent with the image: the record in slot s holds the key found there
        for s, slot in enumerate(arc.map.slots):
            r = int(slot_rec[a, s])
            if slot is None:
                assert r == NONE
            else:
                assert first <= r < first + len(arc.order) and keys[r] == slot[0]
        first += len(arc.order)
    return images, slot_rec, info.tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("hl,version", [(16, 0), (32, 0), (16, 1), (32, 1)])
def test_gpu_map_image_collisions_and_order(hl, version):
    from sdfs_amd.archive import HipBlobArchiver, map_size

    rng = np.random.default_rng(300 + hl + version)
    # 7 slots (limit 5): three keys share a home slot, two of them the probe step too
    k7 = [_key(10, 1, hl), _key(17, 2, hl), _key(45, 3, hl), _key(0x80000000 | 24, 4, hl), _key(6, 5, hl)]
    A = HipBlobArchiver(hl, version, 1 << 20, 7)
    im1, _, info = _emit_and_check(A, k7, [5, 0, 9, 300, 1])
    assert info == [0, 0]
    im2, _, _ = _emit_and_check(A, [k7[i] for i in (2, 0, 4, 1, 3)], [9, 5, 1, 0, 300])
    assert im1 != im2  # the same keys in another order: another image (each equal to the model's)
    # 11 slots filled to the limit of 8, every key with home 4: h = 4 + 11 * j, steps 1 + h % 9
    A = HipBlobArchiver(hl, version, 1 << 20, 11)
    k11 = [_key(4 + 11 * j, 16 + j, hl) for j in range(8)]
    _emit_and_check(A, k11, list(range(8)))
    _emit_and_check(A, k11[::-1], list(range(8)))
    # n = 0 and n = 1
    ims, _, _ = _emit_and_check(A, [], [])
    assert ims == []
    ims, sr, _ = _emit_and_check(A, k11[:1], [77])
    assert (sr[0] != NONE).sum() == 1
    # map_size(2n + 5) slots for n random keys whose hashed bytes take few values: long probe chains
    n = 200
    size = map_size(2 * n + 5)
    keys = [rng.bytes(8) + struct.pack(">I", int(rng.integers(0, 12)) * size + int(rng.integers(0, 3)))
            + rng.bytes(hl - 12) for _ in range(n)]
    A = HipBlobArchiver(hl, version, 1 << 24, size)
    _emit_and_check(A, keys, [int(x) for x in rng.integers(0, 5000, n)])
    # several archives in one call (entry limit 8 of 11 slots)
    A = HipBlobArchiver(hl, version, 1 << 24, 11)
    _emit_and_check(A, _keys(rng, 30, hl), [int(x) for x in rng.integers(0, 50, 30)])


@pytest.mark.gpu
def test_gpu_map_counts_a_duplicated_digest_and_refuses_hash_len_20():
    import torch

    from sdfs_amd.archive import HipBlobArchiver

    rng = np.random.default_rng(5)
    keys = _keys(rng, 6, 32)
    keys[4] = keys[1]
    A = HipBlobArchiver(32, 0, 1 << 20, 11)
    d_lens = _dev(np.arange(6, dtype=np.int32))
    lay = A.plan(d_lens, arc_cap=2)
    maps, slot_rec, info = A.map_emit(lay, d_lens, _records(keys), n_arc=1)
    torch.cuda.synchronize()
    assert info.tolist() == [1, 0]
    sr = slot_rec.cpu().numpy().view(np.uint32)[0]
    assert sorted(int(r) for r in sr if r != NONE) == [0, 1, 2, 3, 5]  # the later of the two has no slot
    with pytest.raises(_lib.SdfsCdcError):
        HipBlobArchiver(20, 0, 1 << 20, 11).map_emit(lay, d_lens, _records(keys), n_arc=1)


# ---- the write path of the round-trip and compaction tests: 8 x 256 KiB buffers, the upper half
# copies of the lower half, a 100 KB zero run, through HipBufferWriter

_KEY = bytes(range(7, 39))
_WRITTEN = {}
L, NBUF = 262144, 8


def _written(variant, algo="sha256"):
    """variant: raw (framed, uncompressed), lz4, aes (LZ4 + AES-256, version 1 archives with IVs of
    their own).  Computed once per variant and shared; the archives stay as written (the compaction
    tests release claims in the variant's index, which no other test looks at)."""
    if (variant, algo) in _WRITTEN:
        return _WRITTEN[(variant, algo)]
    import torch

    from sdfs_amd import HipVariableMD5HashEngine, HipVariableSha256HashEngine
    from sdfs_amd.archive import HipBufferWriter
    from sdfs_amd.device import DeviceBatch
    from sdfs_amd.index import HipHashesMap
    from sdfs_amd.meta import slot_bytes

    e = HipVariableMD5HashEngine() if algo == "md5" else HipVariableSha256HashEngine()
    hl = 16 if algo == "md5" else 32
    batch = DeviceBatch(e, nbuf=NBUF, buf_len=L)
    batch.fill_streams(first_stream=4242, bufs_per_stream=2)
    v = batch.data.view(NBUF, L)
    v[1, 20000:120000] = 0
    for b in range(NBUF // 2, NBUF):
        v[b].copy_(v[b - NBUF // 2])
    ix = HipHashesMap(1 << 12)
    rng = np.random.default_rng(11)
    ivs = [rng.bytes(16) for _ in range(64)]
    aes = variant == "aes"
    wr = HipBufferWriter(ix, hash_len=hl, compress=variant != "raw", aes=_KEY if aes else None,
                         version=1 if aes else 0, blocksz=[200000, 260000, 150000])
    m, arcs = wr.write(batch, PB, ivs=_dev(np.frombuffer(b"".join(ivs), np.uint8).reshape(-1, 16)) if aes else None)
    torch.cuda.synchronize()
    assert int(arcs.extra["overflow"].item()) == 0
    host = batch.data.cpu().numpy().reshape(NBUF, L)
    counts, st, ln, dg, total = batch.host_results()
    loc = arcs.extra["hashloc"].cpu().numpy()[:total]
    dup = arcs.extra["dup"].cpu().numpy()[:total]
    # the new chunks in record order: (digest, chunk bytes)
    new, r = [], 0
    for b in range(NBUF):
        for i in range(int(counts[b])):
            if not dup[r]:
                assert int(loc[r]) == PB + len(new)
                new.append((dg[b, i, :hl].tobytes(), host[b, st[b, i]: st[b, i] + ln[b, i]].tobytes()))
            r += 1
    w = dict(engine=e, index=ix, writer=wr, hl=hl, m=m, arcs=arcs, data=host, new=new, ivs=ivs, variant=variant,
             slot_len=slot_bytes(hl, L, 4095), counts=counts, loc=loc, digests=dg)
    _WRITTEN[(variant, algo)] = w
    return w


def _read_back(w, arcs):
    import torch

    from sdfs_amd.read import HipBufferReader

    aes = w["variant"] == "aes"
    rd = HipBufferReader(L, w["hl"], aes=_KEY if aes else None, record_ivs=aes, engine=w["engine"])
    out = torch.full((NBUF, L), 0xFF, dtype=torch.uint8, device="cuda:0")
    got, status, info = rd.read(w["m"], NBUF, w["slot_len"], arcs.store, *arcs.directory(), PB, out=out,
                                store_ivs=arcs.record_ivs())
    torch.cuda.synchronize()
    rd.destroy()
    return got.cpu().numpy(), status.cpu().numpy(), info


def _model_of(w, arcs, walked=None):
    """The model store fed with the records the device stored (walked out of its own images when not
    given): same cuts, same bytes, same maps."""
    A = w["writer"].archiver
    st = M.Store(A.map_slots, A.blocksz, A.version, A.hash_len, lambda a: w["ivs"][a])
    for key, rec in walked:
        st.put(key, rec)
    return st


def _walk_images(arcs):
    """Every archive image parsed on the host: [len][hash][len][record] from header_bytes to arc_bytes."""
    out = []
    for a in range(arcs.n_arc):
        img = arcs.image(a)
        p, recs = arcs.header_bytes, []
        while p < len(img):
            hl = struct.unpack(">i", img[p: p + 4])[0]
            assert hl == arcs.hash_len
            n = struct.unpack(">i", img[p + 4 + hl: p + 8 + hl])[0]
            recs.append((img[p + 4: p + 4 + hl], img[p + 8 + hl: p + 8 + hl + n], p + 8 + hl))
            p += 8 + hl + n
        assert p == len(img)
        out.append(recs)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("variant,algo", [("raw", "sha256"), ("lz4", "sha256"), ("aes", "sha256"), ("lz4", "md5")])
def test_gpu_write_archive_read_round_trip(variant, algo):
    w = _written(variant, algo)
    arcs = w["arcs"]
    assert arcs.n_arc >= 3 and arcs.n_rec == len(w["new"]) < int(w["counts"].sum()) // 2 + 1
    got, status, info = _read_back(w, arcs)
    assert not status.any() and (got == w["data"]).all()
    assert info.fetch_count == arcs.n_rec
    # the images, parsed on the host, hold exactly the new records in order
    walked = _walk_images(arcs)
    flat = [x for recs in walked for x in recs]
    assert [k for k, _, _ in flat] == [k for k, _ in w["new"]]
    assert [len(r) for _, r, _ in flat] == arcs.store_len.tolist()
    if variant == "raw":
        assert [r for _, r, _ in flat] == [b"\xff\xff\xff\xff" + c for _, c in w["new"]]
    first = arcs.arc_first.tolist()
    assert [len(r) for r in walked] == [first[a + 1] - first[a] for a in range(arcs.n_arc)]
    # every record is found through its archive's map image with the model's get
    for a, recs in enumerate(walked):
        mp = M.SlotMap.from_image(arcs.map_image(a), arcs.version, arcs.hash_len)
        assert mp.size == arcs.map_stride and mp.current == len(recs)
        for key, rec, pos in recs:
            v = mp.get(key)
            assert v == (((pos - 4) << 32) | len(rec) if arcs.version else pos - 4)
    # and the whole store and every map equal the model's, fed the same records
    st = _model_of(w, arcs, [(k, r) for k, r, _ in flat])
    assert len(st.archives) == arcs.n_arc
    assert arcs.store[: arcs.store_bytes].cpu().numpy().tobytes() == M.store_image(st.archives)
    assert [arcs.map_image(a) for a in range(arcs.n_arc)] == [a.map.image() for a in st.archives]
    if variant == "aes":  # the header carries the archive's own IV
        assert [arcs.image(a)[:20] for a in range(arcs.n_arc)] == [struct.pack(">i", 1) + w["ivs"][a]
                                                                   for a in range(arcs.n_arc)]
        assert len({arcs.image(a)[4:20] for a in range(arcs.n_arc)}) == arcs.n_arc


def _model_compact(w, arcs, kept_keys, new_ivs=None, recode=None):
    """compact() of every archive of the model store that mirrors `arcs`."""
    flat = [(k, r) for recs in _walk_images(arcs) for k, r, _ in recs]
    st = _model_of(w, arcs, flat)
    out, deleted = [], []
    for a, arc in enumerate(st.archives):
        iv = new_ivs[len(out)] if new_ivs else bytes(16)
        new = M.compact(arc, lambda k: k in kept_keys, iv, (lambda r, a=a, iv=iv: recode(r, a, iv)) if recode else None)
        deleted.append(new is None)
        if new is not None:
            out.append(new)
    return out, deleted


def _check_compacted(new, model, deleted):
    assert new.n_arc == len(model) and new.deleted.tolist() == [int(d) for d in deleted]
    assert new.store[: new.store_bytes].cpu().numpy().tobytes() == M.store_image(model)
    assert new.store_bytes == len(M.store_image(model))
    for a, arc in enumerate(model):
        assert new.map_image(a) == arc.map.image(), a
        assert int(new.map_sizes[a].item()) == arc.map.size == M.next_prime_i(2 * len(arc.order) + 5)


@pytest.mark.gpu
def test_gpu_compact_keep_nothing_and_keep_everything():
    import torch

    w = _written("lz4")
    arcs, A = w["arcs"], w["writer"].archiver
    none = A.compact(arcs, torch.zeros(arcs.n_rec, dtype=torch.uint8, device="cuda:0"))
    torch.cuda.synchronize()
    assert none.n_arc == 0 and none.n_rec == 0 and none.store_bytes == 0 and none.deleted.tolist() == [1] * arcs.n_arc
    assert (none.new_of_old.cpu().numpy().view(np.uint32) == NONE).all() and not none.store_len.any()
    every = A.compact(arcs, torch.ones(arcs.n_rec, dtype=torch.uint8, device="cuda:0"))
    torch.cuda.synchronize()
    keys = {k for k, _ in w["new"]}
    model, deleted = _model_compact(w, arcs, keys)
    _check_compacted(every, model, deleted)
    # the same records, now in slot order
    walked = _walk_images(every)
    assert sorted(k for recs in walked for k, _, _ in recs) == sorted(keys)
    assert [k for recs in walked for k, _, _ in recs] != [k for k, _ in w["new"]]
    got, status, _ = _read_back(w, every)
    assert not status.any() and (got == w["data"]).all()


def _sweep_half(w, seed):
    """Release every claim of a seeded half of the new fingerprints and sweep: -> (removed_pos, the
    kept keys, the buffers whose chunks all survive)."""
    import torch

    rng = np.random.default_rng(seed)
    n = len(w["new"])
    drop = sorted(int(i) for i in rng.permutation(n)[: n // 2])
    dg = np.zeros((len(drop), 32), np.uint8)
    for j, i in enumerate(drop):
        dg[j, : w["hl"]] = np.frombuffer(w["new"][i][0], np.uint8)
    ix = w["index"]
    _, ref = ix.get_digests(_dev(dg))
    ix.claim_digests(_dev(dg), -ref)  # claim(-1) for every reference
    _, removed_pos, left = ix.sweep()
    torch.cuda.synchronize()
    assert left == 0 and sorted(removed_pos.tolist()) == [PB + i for i in drop]
    kept = {k for i, (k, _) in enumerate(w["new"]) if i not in set(drop)}
    dropped_loc = {PB + i for i in drop}
    whole, r = [], 0
    for b in range(NBUF):
        c = int(w["counts"][b])
        if not dropped_loc & set(int(x) for x in w["loc"][r: r + c]):
            whole.append(b)
        r += c
    return removed_pos, kept, drop, whole


@pytest.mark.gpu
def test_gpu_compact_after_a_sweep():
    w = _written("lz4", "md5")
    arcs = w["arcs"]
    removed_pos, kept, drop, whole = _sweep_half(w, 77)
    import torch

    new = w["writer"].compact(arcs, removed_pos, PB)
    torch.cuda.synchronize()
    model, deleted = _model_compact(w, arcs, kept)
    _check_compacted(new, model, deleted)
    assert new.n_rec == len(kept)
    # the directory keeps its index; dropped entries have length 0
    sl = new.store_len.tolist()
    assert [i for i, x in enumerate(sl) if x == 0] == drop
    got, status, _ = _read_back(w, new)
    for b in whole:  # buffers whose chunks all survive still read back bit for bit
        assert status[b] == 0 and (got[b] == w["data"][b]).all(), b
    # a second compaction of the compacted archives (maps of different sizes now): nothing more to drop
    again = w["writer"].compact(new, removed_pos, PB)
    flat = {k for recs in _walk_images(again) for k, _, _ in recs}
    assert flat == kept and again.n_rec == new.n_rec


@pytest.mark.gpu
def test_gpu_compact_encrypted_archives_get_new_ivs():
    import torch

    from oracle import aes_oracle as AO

    w = _written("aes")
    arcs = w["arcs"]
    removed_pos, kept, drop, whole = _sweep_half(w, 78)
    rng = np.random.default_rng(9)
    new_ivs = [rng.bytes(16) for _ in range(arcs.n_arc)]
    new = w["writer"].compact(arcs, removed_pos, PB,
                              new_ivs=_dev(np.frombuffer(b"".join(new_ivs), np.uint8).reshape(-1, 16)))
    torch.cuda.synchronize()

    def recode(rec, old_arc, iv):  # getChunk under the old archive's IV, putChunk under the new one
        return AO.cbc_encrypt(_KEY, iv, AO.cbc_decrypt(_KEY, w["ivs"][old_arc], rec))

    model, deleted = _model_compact(w, arcs, kept, new_ivs, recode)
    _check_compacted(new, model, deleted)
    # the new images decrypt under the new IVs to the records the old ones held
    old = {k: AO.cbc_decrypt(_KEY, w["ivs"][a], r) for a, recs in enumerate(_walk_images(arcs)) for k, r, _ in recs}
    for a, recs in enumerate(_walk_images(new)):
        assert new.image(a)[:20] == struct.pack(">i", 1) + new_ivs[a]
        for k, r, _ in recs:
            assert AO.cbc_decrypt(_KEY, new_ivs[a], r) == old[k]
    got, status, _ = _read_back(w, new)
    for b in whole:
        assert status[b] == 0 and (got[b] == w["data"][b]).all(), b
