"""A chunk store reopened from its archive and .map images, looked up and scrubbed (include/sdfs_store.h).

CPU: the plain-Python model (tests/store_model.py, restated from SimpleByteArrayLongMap.java and
HashBlobArchive.java) against bytes typed out by hand, and the argument checks of every new entry
point.  GPU: lookup against ``SlotMap.get``, the scan against the model, write -> reopen -> read,
reopen after a sweep and a compaction, the scrub.
Parity status: pinned by the reference's own serialisation code (no fixtures)."""
import ctypes
import dataclasses
import hashlib
import struct

import numpy as np
import pytest

from sdfs_amd import _lib
from tests import archive_model as M
from tests import store_model as SM
from tests import test_archive as TA

PB = TA.PB
NONE = 0xFFFFFFFF
_key = TA._key

# ---- bytes typed by hand: two records under 16-byte keys that share home slot 3 of a 7-slot map
A_HEX = "a1" * 8 + "0000000a" + "a1" * 4  # h = 10: home 3, step 1
B_HEX = "b2" * 8 + "00000011" + "b2" * 4  # h = 17: home 3, step 3 -> slot 0
BODY = ("00000010" + A_HEX + "00000006" + "ffffffff4142"             # cp 0: the record at 24, 6 bytes, raw
        + "00000010" + B_HEX + "00000007" + "00000003" + "78797a")   # cp 30: the record at 54, 7 bytes, nz = 3
FREE20, FREE24 = "00" * 20, "00" * 24
MAP0 = B_HEX + "00000032" + FREE20 * 2 + A_HEX + "00000014" + FREE20 * 3          # values 50 and 20
IV_HEX = "".join(f"{x:02x}" for x in range(0xA0, 0xB0))
ARC1 = "00000001" + IV_HEX + "00" * 1004 + BODY                                    # records at 1048 and 1078
MAP1 = ("0000192a" + "00000001" + "00" * 8 + B_HEX + "00000432" + "00000007" + FREE24 * 2
        + A_HEX + "00000414" + "00000006" + FREE24 * 3)
MAP1_NO_MAGIC = B_HEX + "00000432" + FREE20 * 2 + A_HEX + "00000414" + FREE20 * 3  # the version-0 layout
A_KEY, B_KEY = bytes.fromhex(A_HEX), bytes.fromhex(B_HEX)


def _h(x):
    return bytes.fromhex(x)


def _flat(recs, *names):
    return [tuple(r[n] for n in names) for r in recs]


# ------------------------------------------------------------------------------------------- CPU

def test_model_scan_against_hand_written_bytes():
    # the 7-slot collision map of test_archive's model test, scanned back: put order from slot order
    a, b, c, d = _key(10, 0xA1), _key(17, 0xB2), _key(45, 0xC3), _key(0x80000000 | 24, 0xD4)
    hexs = {0: b.hex() + "00000065", 2: c.hex() + "00000066", 3: a.hex() + "00000064", 5: d.hex() + "00000067"}
    img = _h("".join(hexs.get(i, "00" * 20) for i in range(7)))
    assert SM.geometry(img, 16, 0) == (0, 20, 0, 7)
    assert [(s, k) for s, k, _ in SM.slots(img, 16, 0)] == [(0, b), (2, c), (3, a), (5, d)]
    recs, ver, size, st = SM.scan_archive(b"", img, 16, 0, 0, 32768, True)
    assert _flat(recs, "slot", "key", "pos") == [(3, a, 104), (0, b, 105), (2, c, 106), (5, d, 107)]
    assert [r["flags"] for r in recs] == [SM.RANGE] * 4 and (ver, size, st) == (0, 7, 0)  # nothing unflagged, 0 bytes
    assert [SM.index(img, k, 16, 0) for k in (a, b, c, d)] == [3, 0, 2, 5]
    assert SM.index(img, _key(3, 0xEE), 16, 0) == -1 and SM.index(img, bytes(16), 16, 0) == -1
    # version 0: two records
    recs, ver, size, st = SM.scan_archive(_h(BODY), _h(MAP0), 16, 0, 0, 32768, True)
    assert _flat(recs, "slot", "pos", "len", "key", "raw_len", "flags") == [(3, 24, 6, A_KEY, 2, 0), (0, 54, 7, B_KEY, 3, 0)]
    assert (ver, size, st) == (0, 7, 0)
    # trailing bytes are ignored
    assert SM.geometry(_h(MAP0 + "ffffff"), 16, 0) == (0, 20, 0, 7)
    assert SM.scan_archive(_h(BODY), _h(MAP0 + "ffffff"), 16, 0, 0, 32768, True)[0] == recs
    # version 1 with the magic: the header, [pos][len] values, the version from the file
    assert SM.geometry(_h(MAP1), 16, 1) == (16, 24, 1, 7)
    assert SM.geometry(_h(MAP1.replace("0000192a00000001", "0000192a00000003")), 16, 1) == (16, 24, 3, 7)
    recs1, ver, size, st = SM.scan_archive(_h(ARC1), _h(MAP1), 16, 1, 1024, 32768, True)
    assert _flat(recs1, "slot", "pos", "len", "raw_len", "flags") == [(3, 1048, 6, 2, 0), (0, 1078, 7, 3, 0)]
    assert (ver, size, st) == (1, 7, 0)
    # ... and without it: the version-0 layout, the length from the archive
    assert SM.geometry(_h(MAP1_NO_MAGIC), 16, 1) == (0, 20, 0, 7)
    recs2, ver, size, st = SM.scan_archive(_h(ARC1), _h(MAP1_NO_MAGIC), 16, 1, 1024, 32768, True)
    assert recs2 == recs1 and (ver, size, st) == (0, 7, 0)
    # a 16-byte file is a new map
    assert SM.geometry(_h("0000192a00000001" + "00" * 8), 16, 1) == (0, 20, 0, 0)
    assert SM.scan_archive(_h(ARC1[:2048]), _h("0000192a00000001" + "00" * 8), 16, 1, 1024, 32768, True) == ([], 0, 0, 0)
    assert SM.scan_archive(_h(ARC1), _h("0000192a00000001" + "00" * 8), 16, 1, 1024, 32768, True)[3] == SM.GAP
    # the whole store: ordinals, slot_rec, the IV from the header
    out = SM.scan([_h(ARC1), _h(ARC1)], [_h(MAP1), _h(MAP1)], [0, 4096], 16, 1, 1024, 32768, True)
    assert out["arc_first"] == [0, 2, 4] and out["ivs"] == [_h(IV_HEX)] * 2
    assert out["slot_rec"] == [[1, NONE, NONE, 0, NONE, NONE, NONE], [3, NONE, NONE, 2, NONE, NONE, NONE]]
    assert _flat(out["records"], "arc", "store_off") == [(0, 1048), (0, 1078), (1, 5144), (1, 5174)]


def test_model_flags_against_hand_written_bytes():
    scan0 = lambda arc, mp, mc=32768: SM.scan_archive(_h(arc), _h(mp), 16, 0, 0, mc, True)  # noqa: E731
    fl = lambda out: ([r["flags"] for r in out[0]], out[3])  # noqa: E731
    # RANGE: the length word past the end (value 58 -> the record at 62 of 61 bytes) ...
    out = scan0(BODY, MAP0.replace("00000032", "0000003a"))
    assert fl(out) == ([0, SM.RANGE], SM.GAP) and out[0][1]["len"] == 0 and out[0][1]["pos"] == 62
    # ... the record past the end (value 51: the length word reads 00 00 07 00) ...
    assert fl(scan0(BODY, MAP0.replace("00000032", "00000033"))) == ([0, SM.RANGE], SM.GAP)
    # ... and a position inside the first record's header; with a 1024-byte header, one inside that
    assert fl(scan0(BODY, MAP0.replace("00000014", "00000010"))) == ([SM.RANGE, 0], SM.GAP)
    assert fl(SM.scan_archive(_h(ARC1), _h(MAP1.replace("00000414", "00000014")), 16, 1, 1024, 32768, True)) == \
        ([SM.RANGE, 0], SM.GAP)
    # KEY: one byte of the key in front of the second record
    bad = BODY[:70] + "b3" + BODY[72:]
    assert bad != BODY and fl(scan0(bad, MAP0)) == ([0, SM.KEY], SM.GAP)
    assert fl(scan0(BODY.replace("00000010" + B_HEX, "00000011" + B_HEX), MAP0)) == ([0, SM.KEY], SM.GAP)
    # LEN: version 1, the slot says 5, the image 6
    out = SM.scan_archive(_h(ARC1), _h(MAP1.replace("0000041400000006", "0000041400000005")), 16, 1, 1024, 32768, True)
    assert fl(out) == ([SM.LEN, 0], SM.GAP) and out[0][0]["len"] == 0
    # NZ: a record of 2 bytes; an nz above max_chunk
    short = "00000010" + A_HEX + "00000002" + "4142"
    assert fl(scan0(short, FREE20 * 3 + A_HEX + "00000014" + FREE20 * 3)) == ([SM.NZ], SM.GAP)
    big = "00000010" + A_HEX + "00000005" + "0001000078"
    assert fl(scan0(big, FREE20 * 3 + A_HEX + "00000014" + FREE20 * 3)) == ([SM.NZ], SM.GAP)
    assert fl(scan0(big, FREE20 * 3 + A_HEX + "00000014" + FREE20 * 3, 65536)) == ([0], 0)
    # GAP: five bytes nobody accounts for
    assert fl(scan0(BODY + "0000000000", MAP0)) == ([0, 0], SM.GAP)
    # the nz rule; the directory
    assert [SM.nz_rule(_h(x), 32768) for x in ("ffffffff4142", "0000000378", "00000000414243", "414243", "00008001")] == \
        [(2, 0), (3, 0), (3, 0), (0, SM.NZ), (0, SM.NZ)]
    recs = [dict(store_off=100 + i, len=10 + i, raw_len=20 + i, flags=f) for i, f in enumerate([0, 0, 0, 0, SM.KEY])]
    assert SM.directory(recs, [PB + 1, -1, PB + 1, PB + 9, PB + 2], PB, 3) == \
        ([0, 100, 0], [0, 10, 0], [0, 20, 0], [-1, 0, -1], [2, 1, 1])


def test_store_entry_points_refuse_bad_arguments_before_the_device():
    lib = _lib.load()
    X = 0x1000  # never dereferenced: every call below fails its argument checks
    recs = _lib.StoreRecords(arc=X, slot=X, pos=X, len=X, store_off=X, key=X, raw_len=X, flags=X, count=X, status=X,
                             n_cap=8)
    arcs = _lib.StoreArchives(map_slots=X, version=X, arc_first=X, ivs=X, slot_rec=X, status=X, slot_stride=7)
    R, A = ctypes.byref(recs), ctypes.byref(arcs)
    lens = lambda *v: (ctypes.c_uint64 * len(v))(*v)  # noqa: E731

    def einval(rc):
        assert rc == _lib.EINVAL
        assert lib.sdfs_cdc_last_error()

    scan = lib.sdfs_cdc_store_scan
    for hl in (20, 24):
        einval(scan(0, 2, X, 8192, X, X, X, 300, lens(140, 140), hl, 0, 0, 32768, 1, R, A, None))
    einval(scan(0, 2, X, 8192, X, X, X, 139, lens(100, 140), 16, 0, 0, 32768, 1, R, A, None))  # a map longer than a row
    einval(scan(0, 2, X, 8192, X, X, X, 300, lens(140, 140), 16, 1, 512, 32768, 1, R, A, None))  # header_bytes
    einval(scan(0, 2, None, 8192, X, X, X, 300, lens(140, 140), 16, 0, 0, 32768, 1, R, A, None))
    einval(scan(0, 2, X, 8192, None, X, X, 300, lens(140, 140), 16, 0, 0, 32768, 1, R, A, None))
    einval(scan(0, 2, X, 8192, X, X, None, 300, lens(140, 140), 16, 0, 0, 32768, 1, R, A, None))
    einval(scan(0, 2, X, 8192, X, X, X, 300, None, 16, 0, 0, 32768, 1, R, A, None))
    einval(scan(0, 2, X, 8192, X, X, X, 300, lens(140, 140), 16, 0, 0, 32768, 1, None, A, None))
    einval(scan(0, 2, X, 8192, X, X, X, 300, lens(140, 140), 16, 0, 0, 32768, 1, R, None, None))
    einval(scan(0, 2, X, 8192, X, X, X, 300, lens(140, 140), 16, 0, 0, 1 << 31, 1, R, A, None))
    for field in ("key", "count", "status"):
        bad = _lib.StoreRecords.from_buffer_copy(recs)
        setattr(bad, field, None)
        einval(scan(0, 2, X, 8192, X, X, X, 300, lens(140, 140), 16, 0, 0, 32768, 1, ctypes.byref(bad), A, None))
    bad = _lib.StoreArchives.from_buffer_copy(arcs)
    bad.ivs = None  # archives with a header have IVs to hand back
    einval(scan(0, 2, X, 8192, X, X, X, 400, lens(184, 184), 16, 1, 1024, 32768, 1, R, ctypes.byref(bad), None))
    bad = _lib.StoreArchives.from_buffer_copy(arcs)
    bad.slot_rec = None
    einval(scan(0, 2, X, 8192, X, X, X, 300, lens(140, 140), 16, 0, 0, 32768, 1, R, ctypes.byref(bad), None))

    raw = lib.sdfs_cdc_store_raw_lens
    einval(raw(0, None, X, X, None, 4, 32768, X, X, None))
    einval(raw(0, X, X, X, None, 4, 32768, None, X, None))
    einval(raw(0, X, X, X, None, 4, 32768, X, None, None))
    einval(raw(0, X, X, X, None, 4, 1 << 31, X, X, None))
    einval(raw(0, X, X, X, None, 1 << 32, 32768, X, X, None))

    dr = lib.sdfs_cdc_store_directory
    einval(dr(0, X, X, X, X, X, None, 4, PB, 0, X, X, X, X, X, None))     # n_store 0: nowhere to write a directory
    einval(dr(0, X, X, X, X, X, None, 4, PB, 0, None, None, None, X, X, None))
    einval(dr(0, X, X, X, X, X, None, 4, PB, 9, X, X, None, X, X, None))
    einval(dr(0, X, X, X, X, None, None, 4, PB, 9, X, X, X, X, X, None))
    einval(dr(0, X, X, X, X, X, None, 4, PB, 9, X, X, X, X, None, None))
    einval(dr(0, X, X, X, X, X, None, 4, PB, 1 << 32, X, X, X, X, X, None))

    lk = lib.sdfs_cdc_store_lookup
    for hl in (20, 24):
        einval(lk(0, 2, X, 8192, X, X, X, 300, lens(140, 140), hl, 0, 0, X, X, 4, X, X, X, X, X, None))
    einval(lk(0, 2, X, 8192, X, X, X, 139, lens(140, 100), 16, 0, 0, X, X, 4, X, X, X, X, X, None))
    einval(lk(0, 2, X, 8192, X, X, X, 300, lens(140, 140), 16, 1, 1000, X, X, 4, X, X, X, X, X, None))
    einval(lk(0, 2, X, 8192, X, X, X, 300, lens(140, 140), 16, 0, 0, None, X, 4, X, X, X, X, X, None))
    einval(lk(0, 2, X, 8192, X, X, X, 300, lens(140, 140), 16, 0, 0, X, X, 4, X, X, X, None, X, None))
    einval(lk(0, 2, X, 8192, X, X, None, 300, lens(140, 140), 16, 0, 0, X, X, 4, X, X, X, X, X, None))

    vf = lib.sdfs_cdc_store_verify
    einval(vf(None, X, X, X, X, None, 4, 32, X, None))
    for hl in (20, 24):
        einval(vf(X, X, X, X, X, None, 4, hl, X, None))
    einval(vf(X, None, X, X, X, None, 4, 32, X, None))
    einval(vf(X, X, X, X, X, None, 4, 32, None, None))
    assert ctypes.sizeof(_lib.StoreRecords) == 88 and ctypes.sizeof(_lib.StoreArchives) == 56


# ------------------------------------------------------------------------------------------- GPU

def _dev(a, dt=None):
    return TA._dev(a, dt)


def _images(archives, maps, pad=0):
    """Host images -> the device tensors the entry points take: every archive at a multiple of 4096,
    one map per row, the rows `pad` bytes longer than the longest map."""
    bases, end = [], 0
    for a in archives:
        bases.append((end + 4095) // 4096 * 4096)
        end = bases[-1] + len(a)
    store = np.full(end + 16, 0x5A, np.uint8)
    for b, a in zip(bases, archives):
        store[b: b + len(a)] = np.frombuffer(bytes(a), np.uint8)
    rows = np.full((max(len(maps), 1), max([len(m) for m in maps] + [1]) + pad), 0x77, np.uint8)
    for i, m in enumerate(maps):
        rows[i, : len(m)] = np.frombuffer(bytes(m), np.uint8)
    import torch

    return dict(store=_dev(store), arc_base=_dev(bases, torch.int64), arc_bytes=_dev([len(a) for a in archives], torch.int64),
                maps=_dev(rows), map_len=[len(m) for m in maps], bases=bases)


def _u32(t):
    return t.cpu().numpy().view(np.uint32).tolist()


def _scan_and_check(archives, maps, hl, version, pad=0, plain=True, max_chunk=32768, slot_stride=None):
    """sdfs_cdc_store_scan against the model: every output."""
    import torch

    from sdfs_amd.store import scan_store

    im = _images(archives, maps, pad)
    header = 1024 if version else 0
    want = SM.scan([bytes(a) for a in archives], [bytes(m) for m in maps], im["bases"], hl, version, header, max_chunk,
                   plain)
    sc = scan_store(im["store"], im["arc_base"], im["arc_bytes"], im["maps"], im["map_len"], hl, version, plain=plain,
                    max_chunk=max_chunk, slot_stride=slot_stride)
    torch.cuda.synchronize()
    n, na = len(want["records"]), len(archives)
    assert sc.count.item() == n and sc.status.item() == 0
    R = want["records"]
    for name, got in (("arc", sc.arc), ("slot", sc.slot), ("pos", sc.pos), ("len", sc.len), ("raw_len", sc.raw_len),
                      ("flags", sc.flags)):
        assert _u32(got[:n]) == [r[name] for r in R], name
    assert sc.store_off[:n].tolist() == [r["store_off"] for r in R]
    assert sc.key[:n].cpu().numpy().tobytes() == b"".join(r["key"] + bytes(32 - hl) for r in R)
    assert _u32(sc.map_slots[:na]) == want["sizes"] and _u32(sc.version[:na]) == want["versions"]
    assert _u32(sc.arc_first[: na + 1]) == want["arc_first"]
    assert _u32(sc.arc_status[:na]) == want["status"]
    if header:
        assert sc.ivs[:na].cpu().numpy().tobytes() == b"".join(want["ivs"])
    rows = sc.slot_rec.cpu().numpy().view(np.uint32)
    for a, row in enumerate(want["slot_rec"]):
        assert rows[a].tolist() == row + [NONE] * (sc.slot_stride - len(row)), a
    return sc, want, im


def _filled(map_sz, n, hl, version, rng, keys=None, full=False, lens=None):
    """A model archive with n records (random keys unless given) in a map of map_sz slots; full: past
    the 0.75 limit, which only a hand-built map can be."""
    arc = M.Archive(map_sz, 1 << 30, version, hl, rng.bytes(16))
    if full:
        arc.map.w_max = lambda: map_sz + 1
    keys = list(keys) if keys is not None else []
    keys += TA._keys(rng, n - len(keys), hl)
    for i, k in enumerate(keys[:n]):
        ln = int(lens[i]) if lens is not None else int(rng.integers(4, 60))
        arc.put(k, struct.pack(">i", -1) + rng.bytes(ln - 4) if ln >= 4 else bytes(ln))
    return arc


@pytest.mark.gpu
@pytest.mark.parametrize("hl,version,pad", [(16, 0, 0), (32, 0, 3), (16, 1, 1), (32, 1, 0)])
def test_gpu_lookup_against_slot_map_get(hl, version, pad):
    """One store whose archives have maps of 2, 3, 5, 7, 11, 97 and 8 537 slots, filled to the 0.75
    limit, then hand-built maps without a free slot; every stored key, as many absent ones, keys
    that share a home slot with stored ones, the all-zero key, an archive that does not exist."""
    import torch

    from sdfs_amd.archive import ArchiveSet
    from sdfs_amd.store import lookup

    rng = np.random.default_rng(500 + hl + version)
    k7 = [_key(10, 1, hl), _key(17, 2, hl), _key(45, 3, hl), _key(0x80000000 | 24, 4, hl), _key(6, 5, hl)]
    k11 = [_key(4 + 11 * j, 16 + j, hl) for j in range(8)]  # every key at home 4: the chains wrap below slot 0
    arcs = [_filled(sz, int(sz * .75), hl, version, rng, keys={7: k7, 11: k11}.get(sz)) for sz in (2, 3, 5, 7, 11, 97, 8537)]
    # no free slot: the search ends at the home slot (2 slots: one key per home, the model cannot step)
    arcs += [_filled(2, 2, hl, version, rng, keys=[_key(4, 0x31, hl), _key(7, 0x32, hl)], full=True)]
    arcs += [_filled(sz, sz, hl, version, rng, full=True) for sz in (3, 7)]
    arcs += [_filled(11, 0, hl, version, rng)]                                   # an empty map
    q_arc, q_key = [], []
    for a, arc in enumerate(arcs):
        size = arc.map.size
        stored = list(arc.order)
        absent = TA._keys(rng, max(len(stored), 4), hl)
        absent += [_key(h, 0xEE, hl) for h in (3, 10 + 7 * size, 4 + 11 * size, 0x80000000 | 24)]
        absent += [bytes(hl), bytes(8) + struct.pack(">I", 5) + bytes(hl - 12)]
        for k in stored + absent:
            q_arc.append(a)
            q_key.append(k)
    q_arc += [len(arcs), NONE]
    q_key += [arcs[0].order[0]] * 2
    map_images = [a.map.image() for a in arcs]
    im = _images([a.data for a in arcs], map_images, pad)
    keys = np.zeros((len(q_key), 32), np.uint8)
    for i, k in enumerate(q_key):
        keys[i, :hl] = np.frombuffer(k, np.uint8)
    st = ArchiveSet(store=im["store"], arc_base=im["arc_base"], arc_bytes=im["arc_bytes"], arc_first=None, store_off=None,
                    store_len=None, raw_len=None, maps=im["maps"], slot_rec=None, n_arc=len(arcs), hash_len=hl,
                    version=version, header_bytes=1024 if version else 0, extra={"open": {"map_len": im["map_len"]}})
    got = lookup(st, _dev(np.array(q_arc, np.uint32).view(np.int32)), _dev(keys))
    torch.cuda.synchronize()
    slot, pos, ln, off, flags = _u32(got.slot), _u32(got.pos), _u32(got.len), got.store_off.tolist(), _u32(got.flags)
    hits = 0
    for i, (a, k) in enumerate(zip(q_arc, q_key)):
        arc = arcs[a] if a < len(arcs) else None
        try:
            v = arc.map.get(k) if arc is not None and k != bytes(hl) else -1
        except ZeroDivisionError:  # 2 slots, the home slot holds another key: the reference's % 0 throws, get returns -1
            v = -1
        if v == -1:
            assert (slot[i], pos[i], ln[i], off[i], flags[i]) == (NONE, 0, 0, 0, 0), i
            continue
        hits += 1
        p = ((v >> 32) if version else v) + 4
        assert slot[i] == arc.map.index(k) == SM.index(map_images[a], k, hl, version), i
        assert (pos[i], off[i], flags[i]) == (p, im["bases"][a] + p, 0), i
        assert ln[i] == (v & 0xFFFFFFFF if version else SM.be32(arc.data, p - 4)), i
    assert hits == sum(len(a.order) for a in arcs) > 6400
    # the same store scanned: 6 402 records of one archive sorted in LDS, maps of every size side by side
    _, want, _ = _scan_and_check([bytes(a.data) for a in arcs], map_images, hl, version, pad)
    assert [r["key"] for r in want["records"]] == [k for a in arcs for k in a.order] and not any(want["status"])


@pytest.mark.gpu
@pytest.mark.parametrize("hl,version,pad", [(16, 0, 1), (32, 0, 0), (16, 1, 0), (32, 1, 2)])
def test_gpu_scan_against_the_model(hl, version, pad):
    """An empty map, one entry, a map at the 0.75 limit, maps of different sizes in one store, a
    version-1 file without the magic and one of 16 bytes, trailing bytes."""
    rng = np.random.default_rng(600 + hl + version)
    arcs = [_filled(11, 0, hl, version, rng), _filled(7, 1, hl, version, rng), _filled(11, 8, hl, version, rng),
            _filled(97, 30, hl, version, rng), _filled(5, 3, hl, version, rng, lens=[0, 3, 4])]
    images = [bytes(a.data) for a in arcs]
    maps = [a.map.image() for a in arcs]
    maps[3] += b"\xff" * 7  # trailing bytes
    if version:
        v0 = M.SlotMap(7, 0, hl)  # a map file from before the magic, pointing into an archive with a header
        for k in arcs[2].order[:4]:
            v0.put(k, arcs[2].map.get(k) >> 32)
        images += [images[2], images[1]]
        maps += [v0.image(), maps[1][:16]]
    sc, want, _ = _scan_and_check(images, maps, hl, version, pad)
    first = want["arc_first"]
    assert [r["flags"] for r in want["records"][first[4]: first[5]]] == [SM.NZ, SM.NZ, 0]  # records of 0, 3 and 4 bytes
    assert want["status"][:5] == [0, 0, 0, 0, SM.GAP] and want["sizes"][:5] == [11, 7, 11, 97, 5]
    if version:
        assert want["versions"] == [1] * 5 + [0, 0] and want["sizes"][5:] == [7, 0] and want["status"][5:] == [SM.GAP] * 2
    # record slots to spare, and one too few: only the count and the status word
    import torch

    from sdfs_amd.store import scan_store

    im = _images(images, maps, pad)
    n = len(want["records"])
    tight = scan_store(im["store"], im["arc_base"], im["arc_bytes"], im["maps"], im["map_len"], hl, version, n_cap=n)
    short = scan_store(im["store"], im["arc_base"], im["arc_bytes"], im["maps"], im["map_len"], hl, version, n_cap=n - 1)
    torch.cuda.synchronize()
    assert (tight.count.item(), tight.status.item()) == (n, 0) and _u32(tight.flags) == _u32(sc.flags[:n])
    assert (short.count.item(), short.status.item()) == (n, _lib.STORE_ECAP)
    assert not short.arc_first.any() and not short.flags.any() and (short.slot_rec == -1).all()
    # a map with more slots than slot_rec has columns is not scanned
    few, _, _ = _scan_and_check(images[:3], maps[:3], hl, version, pad, slot_stride=11)
    narrow = scan_store(im["store"], im["arc_base"], im["arc_bytes"], im["maps"], im["map_len"], hl, version, slot_stride=11)
    torch.cuda.synchronize()
    assert _u32(narrow.arc_status[:5])[3] == _lib.STORE_SLOTS and _u32(narrow.map_slots[:5])[3] == 97
    assert narrow.count.item() == n - 30


@pytest.mark.gpu
def test_gpu_scan_of_1025_archives():
    """arc_first is a one-block prefix over the archives' filled slots: 1 025 archives of one record
    each give its first threads two archives and its last ones none, and are no multiple of the
    block.  Every output against the model, arc_first and the record list among them."""
    rng = np.random.default_rng(1025)
    arcs = [_filled(3, 1, 16, 0, rng) for _ in range(1025)]
    sc, want, _ = _scan_and_check([bytes(a.data) for a in arcs], [a.map.image() for a in arcs], 16, 0)
    assert want["arc_first"] == list(range(1026)) and not any(want["status"])
    assert [r["key"] for r in want["records"]] == [a.order[0] for a in arcs]


@pytest.mark.gpu
def test_gpu_scan_sorts_a_large_map_in_global_memory():
    """16 500 zero-length records of 40 bytes each in one archive: more than the 16 384 (pos, slot)
    pairs the scan sorts in LDS.  (A record of 0 bytes has no nz word: every one is flagged NZ.)"""
    rng = np.random.default_rng(16500)
    n = 16500
    arc = _filled(22003, n, 32, 0, rng, lens=[0] * n)
    assert arc.map.size > _lib.STORE_SORT_LDS and len(arc.data) == 40 * n
    sc, want, _ = _scan_and_check([arc.data], [arc.map.image()], 32, 0)
    assert [r["key"] for r in want["records"]] == arc.order  # put order back from slot order
    assert {r["flags"] for r in want["records"]} == {SM.NZ} and want["status"] == [SM.GAP]


@pytest.mark.gpu
@pytest.mark.parametrize("version", [0, 1])
def test_gpu_scan_flags(version):
    """One image each for RANGE, KEY, LEN (version 1), NZ and GAP, next to a clean one: exactly the
    records the model flags, the neighbours clean."""
    rng = np.random.default_rng(700 + version)
    hl = 16
    clean = _filled(11, 5, hl, version, rng, lens=[20, 9, 33, 12, 40])
    img, mp = bytes(clean.data), clean.map.image()
    off, el = (16, hl + 8) if version else (0, hl + 4)
    slot_of = {k: clean.map.index(k) for k in clean.order}
    val = lambda j: off + slot_of[clean.order[j]] * el + hl  # noqa: E731  where record j's map value lies

    def patched(b, at, new):
        b = bytearray(b)
        b[at: at + len(new)] = new
        return bytes(b)

    header = 1024 if version else 0
    pos = [((clean.map.get(k) >> 32) if version else clean.map.get(k)) + 4 for k in clean.order]
    archives = [img, img, patched(img, pos[2] - 9, bytes([img[pos[2] - 9] ^ 1])), img,
                patched(img, pos[3] - 4, struct.pack(">I", 2)) if not version else img,
                patched(img, pos[4], struct.pack(">I", 70000)), img + bytes(5), img]
    maps = [mp, patched(mp, val(1), struct.pack(">I", len(img) + 100)), mp,
            patched(mp, val(3) + 4, struct.pack(">I", 13)) if version else mp,
            patched(mp, val(3) + 4, struct.pack(">I", 2)) if version else mp, mp, mp,
            patched(mp, val(0), struct.pack(">I", header + 3))]
    sc, want, _ = _scan_and_check(archives, maps, hl, version)
    flags = [[r["flags"] for r in want["records"][want["arc_first"][a]: want["arc_first"][a + 1]]] for a in range(8)]
    assert flags[0] == [0] * 5 and want["status"][0] == 0
    assert flags[1] == [0, 0, 0, 0, SM.RANGE]                      # past the end: it sorts last
    assert flags[2] == [0, 0, SM.KEY, 0, 0]
    assert flags[3] == ([0, 0, 0, SM.LEN, 0] if version else [0] * 5)
    # a record of 2 bytes: version 0 reads the shortened length from the image (the bytes behind it
    # are then unaccounted for), version 1 has it in the slot and the image disagrees
    assert flags[4] == [0, 0, 0, SM.LEN if version else SM.NZ, 0]
    assert flags[5] == [0, 0, 0, 0, SM.NZ]                         # nz = 70 000 > max_chunk
    assert flags[6] == [0] * 5
    assert flags[7] == [SM.RANGE, 0, 0, 0, 0]                      # inside the header: it sorts first
    assert want["status"] == [0, SM.GAP, SM.GAP, SM.GAP if version else 0, SM.GAP, SM.GAP, SM.GAP, SM.GAP]
    # an archive that does not lie inside the store: every record RANGE, nothing read through it
    import torch

    from sdfs_amd.store import scan_store

    im = _images([img], [mp])
    out = scan_store(im["store"][: len(img) - 1], im["arc_base"], im["arc_bytes"], im["maps"], im["map_len"], hl, version)
    torch.cuda.synchronize()
    assert _u32(out.flags[:5]) == [SM.RANGE] * 5 and _u32(out.arc_status[:1]) == [SM.GAP]


@pytest.mark.gpu
def test_gpu_directory_and_raw_lens_against_the_model():
    """Orphans, flagged records, hashlocs outside the directory, two and three records that claim
    one entry (the lowest ordinal wins), more than one block of records; the nz rule on its own."""
    import torch

    from sdfs_amd.store import directory, raw_lens

    rng = np.random.default_rng(900)
    n, n_store = 700, 300
    recs = [dict(store_off=int(rng.integers(0, 1 << 40)), len=int(rng.integers(4, 5000)),
                 raw_len=int(rng.integers(0, 9000)), flags=int(rng.choice([0, 0, 0, 0, SM.KEY, SM.RANGE | SM.KEY])))
            for _ in range(n)]
    hashloc = [int(PB + rng.integers(-20, n_store + 20)) if rng.random() < .8 else -1 for _ in range(n)]
    hashloc[5] = hashloc[400] = hashloc[699] = PB + 7
    recs[5]["flags"] = recs[400]["flags"] = recs[699]["flags"] = 0
    hashloc[6], hashloc[7] = PB - 1, PB + n_store
    want = SM.directory(recs, hashloc, PB, n_store)
    assert want[3][7] == 5 and want[4][2] >= 2 and min(want[4]) > 0
    col = lambda k, dt: _dev(np.array([r[k] for r in recs], np.int64), dt)  # noqa: E731
    off, ln, raw, rec, info = directory(col("store_off", torch.int64), col("len", torch.int32), col("raw_len", torch.int32),
                                        col("flags", torch.int32), _dev(np.array(hashloc, np.int64)), PB, n_store)
    torch.cuda.synchronize()
    assert (off.tolist(), ln.tolist(), raw.tolist(), rec.tolist(), info.tolist()) == want
    # no directory at all: only the counts
    *_, info = directory(col("store_off", torch.int64), col("len", torch.int32), col("raw_len", torch.int32),
                         col("flags", torch.int32), _dev(np.array(hashloc, np.int64)), PB, 0)
    torch.cuda.synchronize()
    assert info.tolist() == [want[4][0], n - want[4][0], 0]
    # raw_lens: records at odd offsets; a failed decrypt; a record flagged before
    plain = [_h("ffffffff4142"), _h("0000000378"), _h("00000000414243"), _h("414243"), _h("00008001"), b"", _h("0000000478"),
             _h("0000000578")]
    area, offs = TA._sparse_source(rng, plain)
    lens = [len(p) for p in plain]
    lens[5] = NONE
    flags = _dev(np.array([0, 0, 0, 0, 0, 0, 0, SM.KEY], np.int32))
    got = raw_lens(_dev(area), _dev(offs, torch.int64), _dev(np.array(lens, np.uint32).view(np.int32)), flags, 32768)
    torch.cuda.synchronize()
    assert got.tolist() == [2, 3, 3, 0, 0, 0, 4, 0]
    assert flags.tolist() == [0, 0, 0, SM.NZ, SM.NZ, SM.NZ, 0, SM.KEY]


_MINE = {}


def _fresh(variant, algo="sha256", tag=""):
    """A written store of this module's own (tests/test_archive.py sweeps the indexes of its shared ones)."""
    key = (variant, algo, tag)
    if key not in _MINE:
        saved = TA._WRITTEN.pop((variant, algo), None)
        try:
            _MINE[key] = TA._written(variant, algo)
        finally:
            TA._WRITTEN.pop((variant, algo), None)
            if saved is not None:
                TA._WRITTEN[(variant, algo)] = saved
    return _MINE[key]


def _map_lens(arcs):
    from sdfs_amd.archive import map_bytes

    sizes = arcs.map_sizes.tolist() if arcs.map_sizes is not None else [arcs.map_stride] * arcs.n_arc
    return [map_bytes(s, arcs.hash_len, arcs.version) for s in sizes]


def _reopen(w, arcs, **kw):
    """open_store of nothing but clones of the images, the map lengths and the index."""
    from sdfs_amd.store import open_store

    aes = w["writer"].aes if w["variant"] == "aes" else None
    return open_store(arcs.store.clone(), arcs.arc_base.clone(), arcs.arc_bytes.clone(), arcs.maps.clone(),
                      _map_lens(arcs), w["index"], PB, int(arcs.store_off.shape[0]), hash_len=w["hl"],
                      version=arcs.version, aes=aes, max_chunk=int(w["engine"]._params.max_len), **kw)


def _same(a, b):
    return a.shape == b.shape and bool((a == b).all())


@pytest.mark.gpu
@pytest.mark.parametrize("variant,algo", [("raw", "sha256"), ("lz4", "sha256"), ("aes", "sha256"), ("lz4", "md5")])
def test_gpu_reopen_round_trip(variant, algo):
    import torch

    w = _fresh(variant, algo)
    arcs, hl = w["arcs"], w["hl"]
    op = _reopen(w, arcs)
    torch.cuda.synchronize()
    n, na = arcs.n_rec, arcs.n_arc
    assert (op.n_rec, op.n_arc, op.store_bytes, op.hash_len, op.version, op.header_bytes) == \
        (n, na, arcs.store_bytes, hl, arcs.version, arcs.header_bytes)
    for name in ("arc", "pos", "store_off"):
        assert _same(getattr(op.layout, name)[:n], getattr(arcs.layout, name)[:n]), name
    assert _same(op.rec_len, arcs.rec_len) and _same(op.arc_first, arcs.arc_first)
    assert _same(op.arc_base, arcs.arc_base) and _same(op.arc_bytes, arcs.arc_bytes)
    for got, want in zip(op.directory(), arcs.directory()):
        assert got.dtype == want.dtype and _same(got, want)
    assert _same(op.rec_of_k, arcs.rec_of_k) and _same(op.slot_rec, arcs.slot_rec)
    assert op.map_stride == arcs.map_stride and op.map_sizes.tolist() == [arcs.map_stride] * na
    assert (op.ivs is None and arcs.ivs is None) or _same(op.ivs, arcs.ivs)
    assert op.sel is None and op.records.shape == (n, 48)
    assert op.records[:, :hl].cpu().numpy().tobytes() == b"".join(k for k, _ in w["new"])
    assert not op.records[:, hl:].any()
    assert op.max_entries >= int((arcs.arc_first[1:] - arcs.arc_first[:-1]).max())
    o = op.extra["open"]
    assert not o["flags"].any() and not o["arc_status"].any() and o["info"].tolist() == [0, 0, 0]
    got, status, info = TA._read_back(w, op)
    assert not status.any() and (got == w["data"]).all() and info.fetch_count == n
    if variant == "aes":
        assert _same(op.record_ivs(), arcs.record_ivs())


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["lz4", "aes"])
def test_gpu_reopen_after_a_sweep_and_a_compaction(variant):
    import torch

    w = _fresh(variant, tag="sweep")
    arcs, wr = w["arcs"], w["writer"]
    removed_pos, kept, drop, whole = TA._sweep_half(w, 81)
    rng = np.random.default_rng(82)
    iv = lambda k: _dev(np.frombuffer(rng.bytes(16 * k), np.uint8).reshape(-1, 16)) if variant == "aes" else None  # noqa: E731
    new = wr.compact(arcs, removed_pos, PB, new_ivs=iv(arcs.n_arc))
    op = _reopen(w, new)
    torch.cuda.synchronize()
    assert op.n_rec == new.n_rec == len(kept) and op.n_arc == new.n_arc
    for got, want in zip(op.directory(), new.directory()):
        assert _same(got, want)
    assert [i for i, x in enumerate(op.store_len.tolist()) if x == 0] == drop  # dropped entries have length 0
    assert _same(op.rec_of_k, new.rec_of_k) and _same(op.rec_len, new.rec_len)
    assert _same(op.map_sizes, new.map_sizes) and _same(op.layout.pos[: op.n_rec], new.layout.pos[: op.n_rec])
    assert op.extra["open"]["info"].tolist() == [0, 0, 0]  # the index no longer holds the swept keys: no orphans
    assert not op.extra["open"]["flags"].any() and not op.extra["open"]["arc_status"].any()
    # the original images, reopened against the swept index: the dropped records are orphans
    old = _reopen(w, arcs)
    torch.cuda.synchronize()
    assert old.extra["open"]["info"].tolist() == [len(drop), 0, 0]
    assert [i for i, x in enumerate(old.store_len.tolist()) if x == 0] == drop
    got, status, _ = TA._read_back(w, op)
    for b in whole:
        assert status[b] == 0 and (got[b] == w["data"][b]).all(), b
    # compacting the opened set and the set it was opened from: the same bytes
    keep = _dev((rng.random(new.n_rec) < .5).astype(np.uint8))
    ivs2 = iv(new.n_arc)
    c1 = wr.archiver.compact(op, keep, new_ivs=ivs2, aes=wr.aes)
    c2 = wr.archiver.compact(new, keep, new_ivs=ivs2, aes=wr.aes)
    torch.cuda.synchronize()
    assert (c1.n_arc, c1.n_rec, c1.store_bytes) == (c2.n_arc, c2.n_rec, c2.store_bytes) and c1.n_rec < new.n_rec
    assert _same(c1.store[: c1.store_bytes], c2.store[: c2.store_bytes])
    assert _same(c1.map_sizes, c2.map_sizes) and [c1.map_image(a) for a in range(c1.n_arc)] == \
        [c2.map_image(a) for a in range(c2.n_arc)]
    for got, want in zip(c1.directory(), c2.directory()):
        assert _same(got, want)


def _expected_scrub(w, arcs, store, maps):
    """The model's scrub of host images: the scan's flags, then every readable record through the oracles."""
    from oracle import aes_oracle as AO
    from oracle import lz4_oracle as LO

    hl, mc = w["hl"], int(w["engine"]._params.max_len)
    bases, nbytes = arcs.arc_base.tolist(), arcs.arc_bytes.tolist()
    images = [store[b: b + n].tobytes() for b, n in zip(bases, nbytes)]
    lens = _map_lens(arcs)
    want = SM.scan(images, [maps[a, : lens[a]].tobytes() for a in range(arcs.n_arc)], bases, hl, arcs.version,
                   arcs.header_bytes, mc, w["variant"] != "aes")
    digest = (lambda c: hashlib.md5(c).digest()) if hl == 16 else (lambda c: hashlib.sha256(c).digest())
    flags = []
    for r in want["records"]:
        f = r["flags"]
        if not f & (SM.RANGE | SM.LEN | SM.NZ):
            rec = images[r["arc"]][r["pos"]: r["pos"] + r["len"]]
            dec = (lambda x, a=r["arc"]: AO.cbc_decrypt(TA._KEY, want["ivs"][a], x)) if w["variant"] == "aes" else None
            f |= SM.scrub_flag(rec, r["key"], mc, digest, LO.decompress, dec)
        flags.append(f)
    return flags, want["status"]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["lz4", "aes"])
def test_gpu_scrub(variant):
    import torch

    from sdfs_amd.store import scrub

    w = _fresh(variant)
    arcs = w["arcs"]
    aes = w["writer"].aes if variant == "aes" else None
    n, na = arcs.n_rec, arcs.n_arc
    host_store, host_maps = arcs.store.cpu().numpy(), arcs.maps.cpu().numpy()

    def run(store=None, maps=None, **kw):
        st = dataclasses.replace(arcs, store=_dev(store) if store is not None else arcs.store.clone(),
                                 maps=_dev(maps) if maps is not None else arcs.maps.clone())
        flags, status = scrub(st, w["engine"], aes=aes, **kw)
        torch.cuda.synchronize()
        want = _expected_scrub(w, arcs, store if store is not None else host_store, maps if maps is not None else host_maps)
        assert (_u32(flags), _u32(status)) == want
        return want

    flags, status = run()
    assert flags == [0] * n and status == [0] * na
    # the same through the reopened set
    op = _reopen(w, arcs)
    f2, s2 = scrub(op, w["engine"], aes=aes)
    assert not f2.any() and not s2.any() and f2.shape[0] == n
    # one payload byte flipped in one record
    j = n // 2
    off, ln = int(arcs.layout.store_off[j]), int(arcs.rec_len[j])
    bad = host_store.copy()
    bad[off + 4 + (ln - 4) // 2] ^= 0x40
    flags, status = run(store=bad)
    assert flags[j] in (SM.FETCH, SM.HASH) and [i for i, f in enumerate(flags) if f] == [j] and status == [0] * na
    assert run(store=bad, batch_records=7) == (flags, status)  # slices of 7 records: the same flags
    # a byte of the key in the record's header
    bad = host_store.copy()
    bad[off - 4 - 3] ^= 1
    flags, status = run(store=bad)
    a = int(arcs.layout.arc[j])
    assert [(i, f) for i, f in enumerate(flags) if f] == [(j, SM.KEY)]
    assert status == [SM.GAP if x == a else 0 for x in range(na)]
    # the record's map slot points past the archive: RANGE (the record now sorts last in its archive), GAP
    row = arcs.slot_rec[a].tolist()
    s = row.index(j)
    el, moff = (w["hl"] + 8, 16) if arcs.version else (w["hl"] + 4, 0)
    at = moff + s * el + w["hl"]
    bad_maps = host_maps.copy()
    bad_maps[a, at: at + 4] = np.frombuffer(struct.pack(">I", int(arcs.arc_bytes[a]) + 64), np.uint8)
    flags, status = run(maps=bad_maps)
    last = int(arcs.arc_first[a + 1]) - 1
    assert [(i, f) for i, f in enumerate(flags) if f] == [(last, SM.RANGE)]
    assert status == [SM.GAP if x == a else 0 for x in range(na)]
