"""Map-file lifecycle on the index (include/sdfs_index.h: claim_slots, recount, load, export;
sdfs_amd/mapfile.py: index_map, snapshot, vanish, trim, truncate).

The reference's file delete, snapshot, trim and truncate are whole-map-file walks over
LongByteArrayMap that call DedupFileStore.removeRef / addRef per HashLocPair
(LongByteArrayMap.java:817-882, 884-940, 595-648, 656-688).  The model (tests/mapfile_model.py) is a
dict digest -> [pos, ref] plus tests/read_model.py's parse for the images.

CPU: the model against hand-worked cases and against parse + per-pair claim on 300 seeded
images; the argument checks of the four entry points (no device); the trim / truncate ranges.
GPU: every result of the HIP calls equals the model's exactly."""
import ctypes
import random

import numpy as np
import pytest

from sdfs_amd import _lib, mapfile
from tests import mapfile_model as MM
from tests import read_model as R
from tests.slot_images import digest as _digest, held as _held, seeded_image as _seeded_image

CL = 262144


def H(i, hl=32):
    return (b"h%07d" % i).ljust(hl, b"\x5a")


def _pairs(items, step=100):
    """(digest, hashloc) -> image pairs with ascending pos."""
    return [(d, loc, step, i * step, 0, step) for i, (d, loc) in enumerate(items)]


# ------------------------------------------------------------------------------------------
# CPU: the model
# ------------------------------------------------------------------------------------------
def test_model_hand_worked_walk():
    m = MM.IndexModel()
    a, b, c = H(1), H(2), H(3)
    assert m.load([(a, 10, 2), (b, 11, 1), (a, 10, 1), (c, 7, 0), (c, 5, 4)]) == [0, 0, 0, 1, 0]
    assert m.export() == sorted([(a, 10, 3), (b, 11, 1), (c, 5, 4)])
    sb = 13 + 5 * 56
    imgs = [R.build_image(_pairs([(a, 10), (b, 11), (b, 99), (H(9), 3)])),  # wrong hashloc, unknown digest
            bytes(sb),                                                      # never written
            R.build_image(_pairs([(a, 10)] * 6)),                           # zlen = cap + 1: does not fit
            R.build_image([(a, 10, 5, 0, 0, 5), (c, 5, 5, 0, 0, 5), (b, 11, 5, 9, 0, 5)]),  # repeated pos: c wins
            R.build_image([(a, 10, 5, 0, 0, 5), (b, 11, 5, 9, 0, -1)])]     # a negative field: no pair applied
    counts, status, missed, out = m.claim_slots(imgs, sb, 32, -1)
    assert counts == [4, 2, 2, 2] and status == [0, 0, 1, 0, 1] and missed == [2, 0, 0, 0, 0]
    assert m.export() == sorted([(a, 10, 2), (b, 11, -1), (c, 5, 3)])
    assert out == [i.ljust(sb, b"\0") for i in imgs]
    # selection + free: slots 0 and 2 selected; 0 becomes FREE, the corrupt one keeps its bytes
    counts, status, missed, out = m.claim_slots(imgs, sb, 32, +3, sel=[1, 0, 1, 0, 0], free=True)
    assert counts == [2, 2, 1, 1] and status == [0, 0, 1, 0, 0]
    assert out[0] == bytes(sb) and out[1:] == [i.ljust(sb, b"\0") for i in imgs[1:]]
    assert m.export() == sorted([(a, 10, 5), (b, 11, 2), (c, 5, 3)])
    assert m.sweep() == [] and m.claim(c, 5, -3) and m.sweep() == [(c, 5)]


def test_model_hand_worked_recount():
    m = MM.IndexModel()
    a, b, c, d = H(1), H(2), H(3), H(4)
    m.load([(a, 1, 2), (b, 2, 1), (c, 3, 5), (d, 4, 0)])
    sb = 13 + 3 * 56
    imgs = [R.build_image(_pairs([(a, 1), (b, 2), (c, 3)])), R.build_image(_pairs([(a, 1), (b, 2), (b, 7)]))]
    counts, status, missed, mis = m.recount(imgs, sb, 32, order=[d, c, b, a])
    # a: have 2 want 2; b: have 1 want 2 (under); c: have 5 want 1 (over); d: have 0 want 0 (unnamed, equal)
    assert counts == [5, 1, 0, 1, 1, 1, 2, 2] and missed == [0, 1]
    assert mis == [(c, 3, 5, 1), (b, 2, 1, 2)]
    assert m.recount(imgs, sb, 32, cap=1, order=[d, c, b, a], repair=True)[3] == [(c, 3, 5, 1)]
    assert m.export() == sorted([(a, 1, 2), (b, 2, 2), (c, 3, 1), (d, 4, 0)])
    assert m.recount(imgs, sb, 32)[0] == [5, 1, 0, 0, 0, 1, 4, 0]
    assert m.sweep() == [(d, 4)]


@pytest.mark.parametrize("hl", [32, 16])
def test_model_claim_slots_equals_parse_plus_claims(hl):
    rng = random.Random(400 + hl)
    cap = 7
    sb = 13 + cap * (hl + 24) + 3
    held = _held(rng, 40, hl)
    imgs = [_seeded_image(rng, held, hl, cap)[0] for _ in range(300)]
    a, b = MM.IndexModel(), MM.IndexModel()
    for mdl in (a, b):
        mdl.load([(d, p, 50) for d, p in held])
    counts, status, missed, _ = a.claim_slots(imgs, sb, hl, -1)
    applied = corrupt = 0
    for s, img in enumerate(imgs):
        st, pairs, _, _ = R.parse(img, sb, hl)
        assert st == status[s]
        corrupt += st != 0
        got = [b.claim(p[0], p[1], -1) for p in pairs]
        applied += sum(got)
        assert missed[s] == got.count(False)
    assert counts[:3] == [applied, sum(missed), corrupt] and corrupt and sum(missed) and applied
    assert a.export() == b.export()


# ------------------------------------------------------------------------------------------
# CPU: slot ranges
# ------------------------------------------------------------------------------------------
def test_trim_and_truncate_ranges():
    for f in (mapfile.trim_range, MM.trim_range):
        assert f(100000, 3 * CL, CL) == (1, 3)
        assert f(0, 3 * CL, CL) == (0, 3)            # on buffer boundaries
        assert f(CL, CL, CL) == (1, 2)
        assert f(5, CL - 6, CL)[0] == f(5, CL - 6, CL)[1]  # shorter than one buffer: empty
        assert f(CL - 1, CL, CL) == (1, 1)           # a whole buffer's length, but it straddles two
        assert f(CL + 1, 2 * CL - 2, CL) == (2, 2)
        assert f(7, 0, CL) == (1, 1)
    for f in (mapfile.truncate_keep, MM.truncate_keep):
        assert f(0, CL) == 0
        assert f(2 * CL, CL) == 2                     # on a buffer boundary
        assert f(2 * CL + CL // 2, CL) == 2           # the partial last buffer's slot goes
        assert f(CL - 1, CL) == 0
    with pytest.raises(ValueError):
        mapfile.trim_range(-1, 5, CL)
    with pytest.raises(ValueError):
        mapfile.truncate_keep(-1, CL)


# ------------------------------------------------------------------------------------------
# CPU: argument checks (before any HIP call)
# ------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_before_the_device():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    h = ctypes.addressof(ctypes.create_string_buffer(4096))  # a handle that is never looked at
    E = _lib.EINVAL

    def claim(ix=h, m=p, n=1, sb=293, hl=32, sel=None, delta=-1, free=0, st=p, ms=p, ct=p):
        return lib.sdfs_cdc_index_claim_slots(ix, m, n, sb, hl, sel, delta, free, st, ms, ct, None)

    assert claim(ix=None) == E and b"null index" in lib.sdfs_cdc_last_error()
    assert claim(hl=20) == E and b"hash_len 20" in lib.sdfs_cdc_last_error()
    assert claim(sb=12) == E and b"slot_bytes" in lib.sdfs_cdc_last_error()
    assert claim(delta=0) == E and b"delta" in lib.sdfs_cdc_last_error()
    assert claim(st=None) == E and claim(ct=None) == E and claim(m=None) == E
    assert claim(n=1 << 31) == E

    def recount(ix=h, m=p, n=1, sb=293, hl=32, st=p, ct=p, cap=0, lists=(None, None, None, None)):
        return lib.sdfs_cdc_index_recount(ix, m, n, sb, hl, None, 0, st, None, *lists, cap, ct, None)

    assert recount(ix=None) == E
    assert recount(hl=20) == E and recount(hl=0) == E
    assert recount(sb=12) == E
    assert recount(st=None) == E and recount(ct=None) == E and recount(m=None) == E
    for k in range(4):
        lists = [p] * 4
        lists[k] = None
        assert recount(cap=1, lists=lists) == E and b"mismatch list" in lib.sdfs_cdc_last_error()

    assert lib.sdfs_cdc_index_load(None, p, p, p, 1, p, None) == E
    for k in range(4):
        a = [p] * 4
        a[k] = None
        assert lib.sdfs_cdc_index_load(h, a[0], a[1], a[2], 1, a[3], None) == E
    assert lib.sdfs_cdc_index_load(h, p, p, p, 1 << 31, p, None) == E

    assert lib.sdfs_cdc_index_export(None, p, p, p, 1, p, None) == E
    assert lib.sdfs_cdc_index_export(h, p, p, p, 1, None, None) == E
    for k in range(3):
        a = [p] * 3
        a[k] = None
        assert lib.sdfs_cdc_index_export(h, *a, 1, p, None) == E and b"export list" in lib.sdfs_cdc_last_error()


# ------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------
def _dev_images(torch, images, sb, shift=0):
    """The images as one device tensor of len(images) slots, starting `shift` bytes into its
    allocation (slots of an odd length start at every alignment anyway)."""
    raw = bytes(shift) + b"".join(bytes(i).ljust(sb, b"\0") for i in images)
    t = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).cuda()
    return t[shift:]


def _load_model(torch, ix, model, items):
    """Load items [(digest, pos, ref)] into both; -> the statuses (asserted equal)."""
    want = model.load(items)
    if items:
        dg = torch.from_numpy(np.frombuffer(b"".join(MM.pad32(d) for d, _, _ in items), np.uint8).reshape(-1, 32).copy())
        got = ix.load(dg.cuda(), torch.tensor([p for _, p, _ in items], dtype=torch.int64),
                      torch.tensor([r for _, _, r in items], dtype=torch.int64)).cpu().tolist()
        assert got == want
    return want


def _export(ix, cap=None):
    dg, pos, ref, held = ix.export(cap)
    d = dg.cpu().numpy()
    return [(d[i].tobytes(), p, r) for i, (p, r) in enumerate(zip(pos.tolist(), ref.tolist()))], held


def _check_entries(torch, ix, model, extra=()):
    """Every entry's pos / ref through get_digests, absent digests included, and the held count."""
    keys = list(model.e) + [MM.pad32(k) for k in extra]
    if keys:
        pos, ref = ix.get_digests(torch.from_numpy(np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 32).copy()).cuda())
        want = [tuple(model.e[k]) if k in model.e else (-1, 0) for k in keys]
        assert list(zip(pos.tolist(), ref.tolist())) == want
    assert ix.getSize() == len(model.e)


def _claim_and_check(torch, ix, model, images, sb, hl, delta, sel=None, free=False, shift=0, extra=()):
    m = _dev_images(torch, images, sb, shift)
    sel_t = None if sel is None else torch.tensor(sel, dtype=torch.uint8, device="cuda")
    res = ix.claim_slots(m, len(images), sb, delta, sel=sel_t, free=free, hash_len=hl)
    counts, status, missed, out = model.claim_slots(images, sb, hl, delta, sel, free)
    torch.cuda.synchronize()
    assert res.counts.tolist() == counts
    assert res.slot_status.tolist() == status
    assert res.slot_missed.tolist() == missed
    assert m.cpu().numpy().tobytes() == b"".join(out)
    assert (res.applied, res.missed, res.corrupt, res.nonempty) == tuple(counts)
    _check_entries(torch, ix, model, extra)
    return counts


def _edge_images(rng, held, hl, cap, n):
    """n images that hold every edge the header names at least once (for n >= 8)."""
    want = ["zlen0", "zero", "full", "over", "negzlen", "negfield", "repeat", "plain"]
    out, seen = [], set()
    while len(out) < n:
        img, kind = _seeded_image(rng, held, hl, cap)
        if n >= len(want) and len(out) < len(want) and kind != want[len(out)]:
            continue
        seen.add(kind)
        out.append(img)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("hl", [32, 16])
@pytest.mark.parametrize("shape", ["7181", "five", "big"])
def test_gpu_walk_vs_model(hl, shape):
    torch = pytest.importorskip("torch")
    from sdfs_amd.index import HipHashesMap
    from sdfs_amd.read import pair_cap

    rng = random.Random(hl * 10 + len(shape))
    bal = hl + 24
    sb = {"7181": 7181, "five": 13 + 5 * bal, "big": 13 + bal * 1024}[shape]
    cap = pair_cap(sb, hl)
    assert cap == {"7181": (7181 - 13) // bal, "five": 5, "big": 1024}[shape]
    ix = HipHashesMap(4096)
    model = MM.IndexModel()
    held = _held(rng, 900, hl)
    _load_model(torch, ix, model, [(d, p, 1000) for d, p in held])
    absent = [_digest(rng, hl) for _ in range(3)]
    if shape == "big":  # one slot of 700 pairs: past what one wave of the apply pass takes
        def mk(n):  # ascending pos; every 50th pair names the wrong archive
            picks = [rng.choice(held) for _ in range(n)]
            return [(d[:hl], p ^ (0x100 if i % 50 == 7 else 0), 10, i * 10, 0, 10) for i, (d, p) in enumerate(picks)]

        pairs = mk(700)
        cases = [[R.build_image(pairs)], [R.build_image(mk(cap))],                  # 700 pairs; zlen == cap
                 [R.build_image(pairs[:300] + [pairs[5]] + pairs[300:])]]           # 701, one pos repeated
    else:
        cases = [_edge_images(rng, held, hl, cap, n) for n in (0, 1, 3, 67)]
    for k, images in enumerate(cases):
        for delta in (-1, +1, +3):
            counts = _claim_and_check(torch, ix, model, images, sb, hl, delta, shift=(k + delta) & 3, extra=absent)
            if len(images) == 67:
                assert counts[0] > 100 and counts[1] and counts[2] >= 2
            if shape == "big":
                assert counts[0] >= 600 and counts[1] >= 10
    ix.destroy()


def _mix64(z):
    mask = (1 << 64) - 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
    return z ^ (z >> 31)


@pytest.mark.gpu
def test_gpu_missed_pairs_and_tombstones_on_a_long_chain():
    """A table of 64 slots; 24 digests with the same first 8 bytes form one probe chain that
    wraps.  Every third one is swept: pairs naming a swept digest are missed, the live entries
    behind the tombstones are still reached; so are an unknown digest and a wrong hashloc."""
    torch = pytest.importorskip("torch")
    from sdfs_amd.index import HipHashesMap

    ix = HipHashesMap(50)
    assert ix.getMaxSize() == 56  # 64 slots
    prefix = next(p for p in range(1, 1 << 16) if _mix64(p) & 63 >= 58)
    rng = random.Random(17)
    chain = [prefix.to_bytes(8, "little") + _digest(rng, 24) for _ in range(24)]
    model = MM.IndexModel()
    _load_model(torch, ix, model, [(d, 500 + i, 2) for i, d in enumerate(chain)])
    others = _held(rng, 20, 32, pos0=900)
    _load_model(torch, ix, model, [(d, p, 2) for d, p in others])
    gone = chain[::3]
    dg = torch.from_numpy(np.frombuffer(b"".join(gone), np.uint8).reshape(-1, 32).copy()).cuda()
    ix.claim_digests(dg, -2)
    for d in gone:
        model.claim(d, model.e[d][0], -2)
    removed, rpos, left = ix.sweep()
    assert sorted((bytes(r), p) for r, p in zip(removed.cpu().numpy(), rpos.tolist())) == model.sweep() and left == 0
    assert ix.stats().tombstones == 8
    sb = 7181
    items = [(d, 500 + i) for i, d in enumerate(chain)]           # 8 swept (missed), 16 live behind them
    items += [(chain[1], 777), (_digest(rng), 501), others[3]]   # wrong hashloc, unknown digest, a hit
    images = [R.build_image(_pairs(items)), R.build_image(_pairs(items[::-1]))]
    counts = _claim_and_check(torch, ix, model, images, sb, 32, -1, extra=gone)
    assert counts == [34, 20, 0, 2]
    ix.destroy()


@pytest.mark.gpu
def test_gpu_contention_on_one_entry():
    """One digest named by all 128 pairs of 32 slots (4 096 atomics on one entry) next to 4 096
    distinct digests: the counts are exact."""
    torch = pytest.importorskip("torch")
    from sdfs_amd.index import HipHashesMap

    rng = random.Random(23)
    ix = HipHashesMap(8192)
    model = MM.IndexModel()
    hot = (_digest(rng), 5)
    cold = _held(rng, 4096, 32, pos0=100)
    _load_model(torch, ix, model, [(hot[0], hot[1], 10000)] + [(d, p, 1) for d, p in cold])
    images = [R.build_image(_pairs([hot] * 128)) for _ in range(32)]
    images += [R.build_image(_pairs(cold[128 * s: 128 * (s + 1)])) for s in range(32)]
    counts = _claim_and_check(torch, ix, model, images, 7181, 32, -1)
    assert counts == [8192, 0, 0, 64] and model.e[MM.pad32(hot[0])] == [5, 10000 - 4096]
    counts = _claim_and_check(torch, ix, model, images, 7181, 32, +2)
    assert model.e[MM.pad32(hot[0])] == [5, 10000 + 4096]
    # runs of every length of a few entries, broken by a wrong hashloc, an unknown digest and each other
    few = [hot] + cold[:3]
    items = []
    while len(items) < 5 * 128:
        d, p = rng.choice(few)
        u = rng.random()
        run = [(d, p)] * rng.choice([1, 1, 2, 3, 7, 30, 64, 65, 70])
        items += [(d, p ^ 1)] if u < 0.15 else [(_digest(rng), p)] if u < 0.25 else run
    mixed = [R.build_image(_pairs(items[128 * s: 128 * (s + 1)])) for s in range(5)]
    counts = _claim_and_check(torch, ix, model, mixed, 7181, 32, -3)
    assert counts[0] > 400 and counts[1] >= 1  # runs were applied, and something broke them
    ix.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("hl", [32, 16])
def test_gpu_selection_and_free_slots(hl):
    torch = pytest.importorskip("torch")
    from sdfs_amd.index import HipHashesMap

    rng = random.Random(31 + hl)
    sb, cap = 7181, (7181 - 13) // (hl + 24)
    ix = HipHashesMap(2048)
    model = MM.IndexModel()
    held = _held(rng, 300, hl)
    _load_model(torch, ix, model, [(d, p, 100) for d, p in held])
    images = _edge_images(rng, held, hl, cap, 21)
    sel = [s % 2 == 1 for s in range(21)]  # alternating; the forced corrupt images sit at 3 and 5
    corrupt = [s for s, i in enumerate(images) if R.parse(i, sb, hl)[0]]
    assert any(sel[s] for s in corrupt) and any(not sel[s] for s in range(21) if R.parse(images[s], sb, hl)[1])
    counts = _claim_and_check(torch, ix, model, images, sb, hl, -1, sel=sel, free=True, shift=1)
    assert counts[2] == sum(sel[s] for s in corrupt) and counts[0] > 0
    ix.destroy()


@pytest.mark.gpu
def test_gpu_claim_slots_equals_the_composed_route():
    """The same input through parse_map_slots -> mask selection -> claim_digests(-1,
    expect_pos=hashloc) leaves the index in the same state."""
    torch = pytest.importorskip("torch")
    from sdfs_amd.extent import _live
    from sdfs_amd.index import HipHashesMap
    from sdfs_amd.read import parse_map_slots

    rng = random.Random(41)
    sb, cap = 7181, 128
    held = _held(rng, 700, 32)
    images = _edge_images(rng, held, 32, cap, 40)
    a, b, model = HipHashesMap(2048), HipHashesMap(2048), MM.IndexModel()
    _load_model(torch, a, model, [(d, p, 30) for d, p in held])
    _load_model(torch, b, MM.IndexModel(), [(d, p, 30) for d, p in held])
    m = _dev_images(torch, images, sb)
    res = a.claim_slots(m, 40, sb, -1)
    p = parse_map_slots(m, 40, sb, 32)
    hashes, hashloc = _live(p, torch.ones(40, dtype=torch.bool, device="cuda"))
    out = b.claim_digests(hashes.contiguous(), -1, expect_pos=hashloc)
    torch.cuda.synchronize()
    assert res.applied == int((out != -1).sum().item()) > 0 and res.missed == int((out == -1).sum().item()) > 0
    assert res.slot_status.tolist() == p.status[:40].tolist()
    ea, eb = _export(a)[0], _export(b)[0]
    assert sorted(ea) == sorted(eb) and any(r != 30 for _, _, r in ea)
    model.claim_slots(images, sb, 32, -1)
    assert sorted(ea) == model.export()
    a.destroy()
    b.destroy()


@pytest.mark.gpu
def test_gpu_load_export_round_trip_and_conflicts():
    torch = pytest.importorskip("torch")
    from sdfs_amd.index import HipHashesMap

    rng = random.Random(53)
    ix, model = HipHashesMap(4096), MM.IndexModel()
    items = [(_digest(rng, rng.choice([16, 20, 32])), rng.randrange(1 << 40), rng.randint(-3, 9)) for _ in range(3000)]
    items += [(items[i][0], items[i][1], 4) for i in range(0, 600, 3)]       # the same digest, equal pos: counts add
    items += [(items[i][0], items[i][1] + 5 - 10 * (i % 2), 1) for i in range(1, 600, 3)]  # two positions: the smaller wins
    rng.shuffle(items)
    st = _load_model(torch, ix, model, items)
    assert st.count(1) == 200
    _check_entries(torch, ix, model)
    assert any(r <= 0 for _, r in model.e.values())
    full, held = _export(ix)
    assert held == len(model.e) == 3000 and sorted(full) == model.export()
    part, held = _export(ix, 1000)
    assert part == full[:1000] and held == 3000      # table-slot order: a prefix
    assert _export(ix, 0) == ([], 3000)
    # a digest already held at another pos: status 1, entry unchanged; at its pos: added
    k0, k1 = full[0], full[1]
    assert _load_model(torch, ix, model, [(k0[0], k0[1] + 1, 7), (k1[0], k1[1], 7), (k0[0], k0[1] + 1, 1)]) == [1, 0, 1]
    _check_entries(torch, ix, model)
    # the round trip into a fresh index
    full, _ = _export(ix)
    ix2, model2 = HipHashesMap(4096), MM.IndexModel()
    assert _load_model(torch, ix2, model2, full) == [0] * 3000
    assert sorted(_export(ix2)[0]) == sorted(full) == model.export()
    ix.destroy()
    ix2.destroy()


@pytest.mark.gpu
def test_gpu_load_rebuilds_before_ecap():
    torch = pytest.importorskip("torch")
    from sdfs_amd.index import HipHashesMap

    rng = random.Random(59)
    ix, model = HipHashesMap(100), MM.IndexModel()  # 128 slots, 112 usable
    first = [(_digest(rng), i, 1 if i < 50 else 0) for i in range(100)]
    _load_model(torch, ix, model, first)
    removed, _, left = ix.sweep()
    model.sweep()
    st = ix.stats()
    assert (st.live, st.tombstones, len(removed), left) == (50, 50, 50, 0)
    more = [(_digest(rng), 1000 + i, 2) for i in range(40)]   # 50 + 50 + 40 > 112: needs the tombstones' room
    assert _load_model(torch, ix, model, more) == [0] * 40
    st = ix.stats()
    assert (st.live, st.tombstones) == (90, 0)
    _check_entries(torch, ix, model, extra=[d for d, _, _ in first[50:]])
    before = _export(ix)[0]
    with pytest.raises(_lib.SdfsCdcError) as ei:                 # 90 + 23 > 112: no rebuild can help
        _load_model(torch, ix, MM.IndexModel(), [(_digest(rng), 5000 + i, 1) for i in range(23)])
    assert ei.value.code == _lib.ECAP
    assert _export(ix)[0] == before
    ix.destroy()


@pytest.mark.gpu
def test_gpu_recount_vs_model():
    torch = pytest.importorskip("torch")
    from sdfs_amd.index import HipHashesMap

    rng = random.Random(61)
    sb, hl, cap = 7181, 32, 128
    held = _held(rng, 1500, hl)
    images = _edge_images(rng, held, hl, cap, 50)
    # the exact counts: what the images name
    named = MM.IndexModel()
    named.load([(d, p, 0) for d, p in held])
    named.claim_slots(images, sb, hl, +1)
    exact = [(d, p, r) for d, p, r in named.export() if r > 0]
    ix, model = HipHashesMap(4096), MM.IndexModel()
    _load_model(torch, ix, model, exact)
    m = _dev_images(torch, images, sb, shift=2)

    def recount(**kw):
        order = [d for d, _, _ in _export(ix)[0]]
        res = ix.recount(m, len(images), sb, **kw)
        counts, status, missed, mis = model.recount(images, sb, hl, order=order, **kw)
        torch.cuda.synchronize()
        assert res.counts.tolist() == counts
        assert res.slot_status.tolist() == status and res.slot_missed.tolist() == missed
        assert res.mismatches() == mis
        _check_entries(torch, ix, model)
        return counts

    c = recount(cap=16)
    assert c[3:] == [0, 0, 0, len(exact), 0] and c[1] > 0 and c[2] >= 2   # clean: 0 under, 0 over
    # perturb: 20 up, 20 down, and 15 entries nobody names
    keys = [d for d, _, _ in exact]
    up, down = keys[:20], keys[20:40]
    dg = torch.from_numpy(np.frombuffer(b"".join(up + down), np.uint8).reshape(-1, 32).copy()).cuda()
    ix.claim_digests(dg, torch.tensor([2] * 20 + [-1] * 20, dtype=torch.int64))
    for d in up:
        model.e[d][1] += 2
    for d in down:
        model.e[d][1] -= 1
    unnamed = [(_digest(rng), 9000 + i, 3 if i % 3 else 0) for i in range(15)]
    _load_model(torch, ix, model, unnamed)
    c = recount(cap=1024)
    assert c[3:] == [20, 30, 15, len(exact) - 40 + 5, 50]
    assert recount(cap=7)[7] == 7      # cap smaller than the number of mismatches: the first 7 in slot order
    assert recount(cap=0)[7] == 0
    c = recount(cap=64, repair=True)   # the report describes the state before the repair
    assert c[3:] == [20, 30, 15, len(exact) - 40 + 5, 50]
    c = recount(cap=64)
    assert c[3:] == [0, 0, 15, len(exact) + 15, 0]
    removed, rpos, left = ix.sweep()
    assert sorted((bytes(r), p) for r, p in zip(removed.cpu().numpy(), rpos.tolist())) == model.sweep() and left == 0
    assert len(removed) == 15
    # a selection: only the even slots are counted
    sel = [s % 2 == 0 for s in range(len(images))]
    order = [d for d, _, _ in _export(ix)[0]]
    res = ix.recount(m, len(images), sb, sel=torch.tensor(sel, dtype=torch.uint8, device="cuda"), cap=4096)
    counts, status, missed, mis = model.recount(images, sb, hl, sel=sel, order=order, cap=4096)
    assert res.counts.tolist() == counts and res.mismatches() == mis and counts[4] > 0
    ix.destroy()


# ---- end to end: the writer's store, the lifecycle calls, the reader

PB = 1 << 33
NBUF = 8


def _written():
    """Eight buffers of 256 KiB through HipBufferWriter.write; buffers 4..7 repeat 0..3."""
    import torch

    from sdfs_amd import HipVariableSha256HashEngine
    from sdfs_amd.archive import HipBufferWriter
    from sdfs_amd.device import DeviceBatch
    from sdfs_amd.index import HipHashesMap
    from sdfs_amd.meta import slot_bytes

    e = HipVariableSha256HashEngine()
    batch = DeviceBatch(e, nbuf=NBUF, buf_len=CL)
    batch.fill_streams(first_stream=6260, bufs_per_stream=1)
    v = batch.data.view(NBUF, CL)
    v[4:].copy_(v[:4])
    ix = HipHashesMap(1 << 13)
    wr = HipBufferWriter(ix, compress=True, blocksz=[200000, 260000, 150000])
    m, arcs = wr.write(batch, PB)
    torch.cuda.synchronize()
    assert int(arcs.extra["overflow"].item()) == 0
    return dict(engine=e, ix=ix, wr=wr, m=m, arcs=arcs, data=batch.data.cpu().numpy().copy(),
                slot_len=slot_bytes(32, CL, 4095))


def _host_images(m, nbuf, sl):
    raw = m.cpu().numpy().tobytes()
    return [raw[s * sl: (s + 1) * sl] for s in range(nbuf)]


def _model_of(ix):
    model = MM.IndexModel()
    model.load(_export(ix)[0])
    return model


@pytest.mark.gpu
def test_gpu_life_cycle_snapshot_vanish_sweep_compact():
    import torch

    from sdfs_amd import snapshot, vanish

    w = _written()
    ix, m, sl = w["ix"], w["m"], w["slot_len"]
    before = sorted(_export(ix)[0])
    assert before and all(r >= 2 for _, _, r in before)  # every chunk is named by two buffers at least
    snap = snapshot(ix, m, NBUF, sl)
    assert torch.equal(snap, m) and snap.data_ptr() != m.data_ptr()
    n_pairs = sum(r for _, _, r in before)
    assert sorted(_export(ix)[0]) == [(d, p, 2 * r) for d, p, r in before]   # the snapshot doubles every count
    assert vanish(ix, m, NBUF, sl) == 0
    assert sorted(_export(ix)[0]) == before                                   # deleting the original restores them
    assert vanish(ix, snap, NBUF, sl) == 0
    after = sorted(_export(ix)[0])
    assert [(d, p) for d, p, _ in after] == [(d, p) for d, p, _ in before] and all(r <= 0 for _, _, r in after)
    assert vanish(ix, snap, 0, sl) == 0
    digests, removed_pos, left = ix.sweep()
    assert left == 0 and sorted(removed_pos.tolist()) == sorted(p for _, p, _ in before)  # every fingerprint
    assert vanish(ix, snap, NBUF, sl) == n_pairs  # nothing left to release: every pair is orphaned
    new = w["wr"].compact(w["arcs"], removed_pos, PB)
    torch.cuda.synchronize()
    assert new.n_arc == 0 and new.n_rec == 0 and new.store_bytes == 0          # the store is empty
    w["wr"].destroy()
    ix.destroy()
    w["engine"].destroy()


@pytest.mark.gpu
def test_gpu_life_cycle_truncate_trim_read_recount():
    """truncate and trim against the model; the file still reads back; and after one copy_extents
    and one rewrite_blocks a recount over every persisted slot reports no mismatch — the invariant
    'a fingerprint's count = the pairs in persisted slots that name it' checked on the device."""
    import torch

    from sdfs_amd import copy_extents, rewrite_blocks, snapshot, split_extent, trim, truncate
    from sdfs_amd.device import DeviceBatch
    from sdfs_amd.read import HipBufferReader

    w = _written()
    ix, m, sl, arcs1 = w["ix"], w["m"], w["slot_len"], w["arcs"]
    snap = snapshot(ix, m, NBUF, sl)
    model = _model_of(ix)
    # truncate the snapshot to 2.5 buffers: 2 slots stay, 6 release their pairs
    images = _host_images(snap, NBUF, sl)
    cut, k = truncate(ix, snap, NBUF, sl, 2 * CL + CL // 2, CL)
    mk, counts, kept = model.truncate(images, sl, 32, 2 * CL + CL // 2, CL)
    assert k == mk == 2 and cut.numel() == 2 * sl and cut.cpu().numpy().tobytes() == b"".join(kept)
    assert counts[1:] == [0, 0, 6] and counts[0] > 0                 # 6 slots released, nothing missed
    assert sorted(_export(ix)[0]) == model.export()
    assert truncate(ix, cut, 2, sl, 2 * CL, CL)[1] == 2              # on the boundary: nothing to cut
    assert sorted(_export(ix)[0]) == model.export()
    # trim [100 000, 100 000 + 3 CL) of the file: slots 1 and 2 are freed
    images = _host_images(m, NBUF, sl)
    rng_, res = trim(ix, m, NBUF, sl, 100000, 3 * CL, CL)
    mr, counts, out = model.trim(images, sl, 32, 100000, 3 * CL, CL)
    assert rng_ == mr == (1, 3) and res.counts.tolist() == counts and res.nonempty == 2
    assert m.cpu().numpy().tobytes() == b"".join(out) and not m[sl: 3 * sl].any() and m[3 * sl:].any()
    assert sorted(_export(ix)[0]) == model.export()
    assert trim(ix, m, NBUF, sl, 5, CL - 6, CL) == ((1, 1), None)  # shorter than a buffer: empty

    def read(store, directory):
        rd = HipBufferReader(CL, 32, engine=w["engine"])
        out = torch.full((NBUF, CL), 0xFF, dtype=torch.uint8, device="cuda:0")
        got, status, _ = rd.read(m, NBUF, sl, store, *directory, PB, out=out)
        torch.cuda.synchronize()
        rd.destroy()
        assert not status.any()
        return got.cpu().numpy().reshape(-1)

    want = w["data"].copy()
    want[CL: 3 * CL] = 0
    assert (read(arcs1.store, arcs1.directory()) == want).all()  # zeros in the freed buffers
    # one copy inside the file into a freed slot, one rewrite over a freed and a live slot
    segs = split_extent(5003, CL + 7001, 100000, CL)
    _, status, seg_status, info = copy_extents(m, m, NBUF, NBUF, sl, segs, index=ix, chunk_length=CL)
    assert info.written and not status.any() and not seg_status.any()
    want[CL + 7001: CL + 107001] = w["data"][5003: 105003]
    RL = 65536
    runs = DeviceBatch(w["engine"], nbuf=2, buf_len=RL)
    runs.fill_streams(first_stream=7370, bufs_per_stream=1)
    run_data = runs.data.cpu().numpy().copy()
    pb2 = PB + int(arcs1.store_off.shape[0])
    _, status, arcs2, info = rewrite_blocks(w["wr"], runs, pb2, m, NBUF, sl, [2, 5], [4099, 100003], chunk_length=CL)
    torch.cuda.synchronize()
    assert not status.any()
    for r, (b, at) in enumerate([(2, 4099), (5, 100003)]):
        want[b * CL + at: b * CL + at + RL] = run_data[r * RL: (r + 1) * RL]
    store = torch.cat([arcs1.store, arcs2.store])
    directory = (torch.cat([arcs1.store_off, arcs2.store_off + arcs1.store.numel()]),
                 torch.cat([arcs1.store_len, arcs2.store_len]), torch.cat([arcs1.raw_len, arcs2.raw_len]))
    assert (read(store, directory) == want).all()
    # every persisted slot of the volume: the file's eight and the truncated snapshot's two
    every = torch.cat([m[: NBUF * sl], cut])
    rc = ix.recount(every, NBUF + 2, sl, cap=64)
    torch.cuda.synchronize()
    assert rc.mismatches() == []
    assert (rc.under, rc.over, rc.missed, rc.corrupt, rc.listed) == (0, 0, 0, 0, 0)
    assert rc.counted > 0 and rc.equal == ix.getSize()
    w["wr"].destroy()
    ix.destroy()
    w["engine"].destroy()
