"""Extent copies and block rewrites (include/sdfs_extent.h): HashLocPairs merged into map slots.

CPU: hand-worked cases of the plain-Python model (tests/extent_model.py, restated from
SparseDataChunk.java:181-263,295-318 and CopyExtents.java:96-155) for every rule, the model's two
forms of line 248 against each other and against byte painting, ``split_extent`` against the
reference's loop, and the C-ABI's argument checks.  GPU: every entry point elementwise equal to the
model, both kernel paths, the capacity edges, and copy / rewrite end to end through the writer,
the reader and the index.
Parity status: pinned by the reference's own insert / serialisation code (no fixtures); the one
divergence (a split's tail is kept) is pinned by test_literal_form_loses_exactly_the_split_tail."""
import ctypes

import numpy as np
import pytest

from sdfs_amd import _lib
from sdfs_amd.extent import split_extent
from tests import extent_model as X
from tests import read_model as R

PB = 1 << 33
CL = 64            # chunk_length of the rule cases
SLOT8 = 13 + 56 * 8


def H(i):
    return bytes([i & 0xFF, i >> 8 & 0xFF]) * 16


def bp(i, pos, nlen, offset=0, ln=None):
    """Pair number i: hash H(i), hashloc PB + i."""
    return X.pair(H(i), PB + i, offset + nlen + 3 if ln is None else ln, pos, offset, nlen)


def short(ps):
    """(pair number, pos, offset, nlen, dup) of model pairs."""
    return [(p[X.HASHLOC] - PB, p[X.POS], p[X.OFFSET], p[X.NLEN], p[X.DUP]) for p in ps]


# name, base pairs, inserts in order, the list after them
CASES = [
    ("apart", [bp(0, 0, 10), bp(1, 40, 10)], [bp(9, 20, 10)],
     [(0, 0, 0, 10, False), (9, 20, 0, 10, False), (1, 40, 0, 10, False)]),
    ("touching both sides", [bp(0, 0, 10), bp(1, 20, 10)], [bp(9, 10, 10)],
     [(0, 0, 0, 10, False), (9, 10, 0, 10, False), (1, 20, 0, 10, False)]),
    ("removed, same range", [bp(0, 10, 10)], [bp(9, 10, 10)], [(9, 10, 0, 10, False)]),
    ("removed, inside", [bp(0, 10, 10), bp(1, 20, 4)], [bp(9, 5, 20)], [(9, 5, 0, 20, False)]),
    ("head trimmed", [bp(0, 10, 20, offset=2)], [bp(9, 5, 10)], [(9, 5, 0, 10, False), (0, 15, 7, 15, False)]),
    ("tail trimmed", [bp(0, 10, 20)], [bp(9, 20, 20)], [(0, 10, 0, 10, False), (9, 20, 0, 20, False)]),
    ("tail trimmed to the insert's end", [bp(0, 10, 20)], [bp(9, 20, 10)], [(0, 10, 0, 10, False), (9, 20, 0, 10, False)]),
    ("split", [bp(0, 10, 40, offset=1)], [bp(9, 20, 10)],
     [(0, 10, 1, 10, False), (9, 20, 0, 10, False), (0, 30, 21, 20, True)]),
    ("empty pairs", [bp(0, 9, 0), bp(1, 10, 0), bp(2, 12, 0), bp(3, 20, 0), bp(4, 21, 0)], [bp(9, 10, 10)],
     [(0, 9, 0, 0, False), (9, 10, 0, 10, False), (4, 21, 0, 0, False)]),
    ("ep == CHUNK_LENGTH", [bp(0, 0, CL)], [bp(9, 60, 4)], [(0, 0, 0, 60, False), (9, 60, 0, 4, False)]),
    ("never-written slot", [], [bp(9, 5, 4, offset=7)], [(9, 5, 7, 4, False)]),
    ("the second hides the first", [bp(0, 0, CL)], [bp(8, 20, 10), bp(9, 10, 30)],
     [(0, 0, 0, 10, False), (9, 10, 0, 30, False), (0, 40, 40, 24, True)]),
    ("a split tail stays dup when its head goes", [bp(0, 0, 60)], [bp(8, 20, 10), bp(9, 0, 20)],
     [(9, 0, 0, 20, False), (8, 20, 0, 10, False), (0, 30, 30, 30, True)]),
    ("an insert is split by the next", [bp(0, 0, 8)], [bp(8, 10, 40, offset=5), bp(9, 20, 5)],
     [(0, 0, 0, 8, False), (8, 10, 5, 10, False), (9, 20, 0, 5, False), (8, 25, 20, 25, True)]),
    ("neighbours cut on both sides", [bp(0, 0, 20), bp(1, 20, 10), bp(2, 30, 20)], [bp(9, 15, 20)],
     [(0, 0, 0, 15, False), (9, 15, 0, 20, False), (2, 35, 5, 15, False)]),
]


def run_model(base, inserts, cl, literal=False):
    ar = X.tree(base)
    split = False
    for p in inserts:
        split |= X.insert(ar, list(p), cl, literal=literal)
    return ar, split


# ------------------------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_model_hand_worked_cases(case):
    _, base, inserts, want = case
    ar, _ = run_model(base, inserts, CL)
    assert short(X.values(ar)) == want
    assert all(k == ar[k][X.POS] for k in ar)
    # the image: pairs in pos order, doop = the dup pairs' nlen
    st, ps, doop, flags = R.parse(X.get_bytes(ar), SLOT8, 32)
    assert st == 0 and flags == 0 and [p[3:] for p in ps] == [w[1:4] for w in want]
    assert doop == sum(w[3] for w in want if w[4])


def test_model_overflow_and_get_wl():
    with pytest.raises(X.Overflow):
        X.insert({}, bp(9, 60, 5), CL)
    ar = X.tree([bp(0, 10, 20, offset=3), bp(1, 40, 5)])
    assert short([X.get_wl(ar, 10)]) == [(0, 10, 3, 20, False)]
    assert short([X.get_wl(ar, 29)]) == [(0, 29, 22, 1, False)]
    assert short([X.get_wl(ar, 44)]) == [(1, 44, 4, 1, False)]
    for x in (0, 9, 30, 39, 45):
        with pytest.raises(X.NotFound):
            X.get_wl(ar, x)
    assert short(X.values(ar)) == [(0, 10, 3, 20, False), (1, 40, 0, 5, False)]  # clones: the map is untouched


def random_buffer(rng, cl, lo, hi, hole_p, max_ins, ins_hi, max_base=None, first=0, log_len=False):
    """Base pairs of lo..hi bytes with holes, then 0..max_ins inserts of 1..ins_hi bytes (log_len:
    their lengths log-uniform, so that short ones, which split pairs, are as common as long ones,
    which remove them)."""
    base, pos, i = [], int(rng.integers(0, lo)), first
    while pos < cl and (max_base is None or len(base) < max_base):
        n = min(int(rng.integers(lo, hi + 1)), cl - pos)
        if rng.random() >= hole_p:
            base.append(bp(i, pos, n, offset=int(rng.integers(0, 50))))
            i += 1
        pos += n
    inserts = []
    for _ in range(int(rng.integers(0, max_ins + 1))):
        n = int(ins_hi ** rng.random()) if log_len else int(rng.integers(1, ins_hi + 1))
        p = int(rng.integers(0, cl - n + 1))
        inserts.append(bp(i, p, n, offset=int(rng.integers(0, 50))))
        i += 1
    return base, inserts


def test_clone_form_equals_painting_and_literal_form_where_nothing_splits():
    rng = np.random.default_rng(20240)
    n_seq, n_split, n_runaway, n_lost = 3000, 0, 0, 0
    for _ in range(n_seq):
        base, inserts = random_buffer(rng, 256, 5, 60, 0.2, 6, 80)
        ar, split = run_model(base, inserts, 256)
        assert [p[:6] for p in X.values(ar)] == X.paint(base, inserts, 256)
        try:
            lit, _ = run_model(base, inserts, 256, literal=True)
        except X.Runaway:
            assert split
            n_runaway += 1
            n_split += 1
            continue
        if not split:
            assert X.get_bytes(lit) == X.get_bytes(ar)
        else:
            n_split += 1
            n_lost += X.covered(X.persisted(lit), 256) != X.covered(X.persisted(ar), 256)
    print(f"{n_seq} sequences: {n_split} with a split, of those {n_lost} lose data and {n_runaway} do not end "
          f"in the literal form")
    assert n_seq - n_split >= 500 and n_lost >= 500  # both sides of the comparison are exercised


def test_literal_form_loses_exactly_the_split_tail():
    base, p = [bp(0, 10, 40, offset=1)], bp(9, 20, 10)
    ar, split = run_model(base, [p], CL)
    lit, split_l = run_model(base, [p], CL, literal=True)
    assert split and split_l
    have, lost = X.covered(X.persisted(ar), CL), X.covered(X.persisted(lit), CL)
    ep, hep = 30, 50
    assert [x for x in range(CL) if have[x] != lost[x]] == list(range(ep, hep))
    assert all(lost[x] is None for x in range(ep, hep))
    assert all(have[x] == (PB, 1 + x - 10) for x in range(ep, hep))


@pytest.mark.parametrize("sstart,dstart,length", [
    (0, 0, 4 * 100), (0, 0, 4 * 100 - 30), (130, 130, 250), (130, 130, 170), (37, 255, 333), (37, 255, 345),
    (250, 12, 50), (5, 95, 5), (5, 95, 6), (99, 0, 1), (0, 299, 201)])
def test_split_extent_walks_the_reference_loop(sstart, dstart, length):
    cl = 100
    src = {b: X.tree([bp(b * 10 + i, p, n) for i, (p, n) in enumerate([(0, 33), (33, 1), (34, 40), (74, 26)])])
           for b in range(8)}
    steps = X.copy_extent_loop(src, {}, sstart, dstart, length, cl)
    segs = split_extent(sstart, dstart, length, cl)
    assert segs == X.segments_of(steps)
    assert sum(s[4] for s in segs) == length
    assert all(s[1] + s[4] <= cl and s[3] + s[4] <= cl for s in segs)


def test_extent_struct_layouts():
    assert ctypes.sizeof(_lib.Segment) == 20 and ctypes.sizeof(_lib.Run) == 8 and ctypes.sizeof(_lib.Inserts) == 56


def _fake(struct, n, **kw):
    p = struct(**kw)
    for name, _ in struct._fields_[:n]:
        setattr(p, name, 0x1000)  # never dereferenced: every call below fails its argument checks
    return p


def test_extent_entry_points_refuse_bad_arguments_before_the_device():
    lib = _lib.load()
    p, q = _fake(_lib.Pairs, 10, cap=8), _fake(_lib.Pairs, 10, cap=8)
    q.pos = q.hashes = q.counts = 0x2000
    bad = _fake(_lib.Pairs, 10, cap=8)
    bad.nlen = None
    ins, badins = _fake(_lib.Inserts, 7), _fake(_lib.Inserts, 7)
    badins.hashloc = None
    out, badout = _fake(_lib.DevOut, 4, cap=8), _fake(_lib.DevOut, 4, cap=8)
    badout.lens = None
    X_ = ctypes.c_void_p(0x1000)
    B = ctypes.byref

    def einval(rc):
        assert rc == _lib.EINVAL
        assert lib.sdfs_cdc_last_error()

    def segs(*rows):
        return ctypes.addressof(seg_keep.setdefault(rows, (_lib.Segment * len(rows))(*[_lib.Segment(*r) for r in rows])))

    seg_keep = {}
    ok = segs((0, 0, 0, 0, 64))
    # map_extents
    einval(lib.sdfs_cdc_map_extents(0, 1, None, 1, 64, 1, ok, X_, B(ins), 4, X_, X_, None))
    einval(lib.sdfs_cdc_map_extents(0, 1, B(bad), 1, 64, 1, ok, X_, B(ins), 4, X_, X_, None))
    einval(lib.sdfs_cdc_map_extents(0, 1, B(p), 1, 64, 1, ok, X_, B(badins), 4, X_, X_, None))
    einval(lib.sdfs_cdc_map_extents(0, 1, B(p), 1, 0, 1, ok, X_, B(ins), 4, X_, X_, None))
    einval(lib.sdfs_cdc_map_extents(0, 1, B(p), 1, 64, 1, None, X_, B(ins), 4, X_, X_, None))
    einval(lib.sdfs_cdc_map_extents(0, 1, B(p), 1, 64, 1, ok, None, B(ins), 4, X_, X_, None))
    einval(lib.sdfs_cdc_map_extents(0, 1, B(p), 1, 64, 1, ok, X_, B(ins), 4, None, X_, None))
    for row in [(0, 0, 0, 0, 0), (1, 0, 0, 0, 8), (0, 0, 1, 0, 8), (0, 60, 0, 0, 5), (0, 0, 0, 60, 5),
                (0, 0xFFFFFFFF, 0, 0, 2), (0, 0, 0, 0xFFFFFFFF, 2)]:
        einval(lib.sdfs_cdc_map_extents(0, 1, B(p), 1, 64, 2, segs((0, 0, 0, 0, 64), row), X_, B(ins), 4, X_, X_, None))
    # map_inserts_from_chunks
    runs = (_lib.Run * 2)(_lib.Run(0, 0), _lib.Run(0, 32))
    R_ = ctypes.addressof(runs)
    einval(lib.sdfs_cdc_map_inserts_from_chunks(0, 2, None, 32, X_, 1, 64, R_, X_, B(ins), 8, X_, None))
    einval(lib.sdfs_cdc_map_inserts_from_chunks(0, 2, B(badout), 32, X_, 1, 64, R_, X_, B(ins), 8, X_, None))
    einval(lib.sdfs_cdc_map_inserts_from_chunks(0, 2, B(out), 32, X_, 1, 64, R_, X_, B(badins), 8, X_, None))
    einval(lib.sdfs_cdc_map_inserts_from_chunks(0, 2, B(out), 32, None, 1, 64, R_, X_, B(ins), 8, X_, None))
    einval(lib.sdfs_cdc_map_inserts_from_chunks(0, 2, B(out), 32, X_, 1, 64, None, X_, B(ins), 8, X_, None))
    einval(lib.sdfs_cdc_map_inserts_from_chunks(0, 2, B(out), 32, X_, 1, 64, R_, X_, B(ins), 8, None, None))
    einval(lib.sdfs_cdc_map_inserts_from_chunks(0, 2, B(out), 0, X_, 1, 64, R_, X_, B(ins), 8, X_, None))
    einval(lib.sdfs_cdc_map_inserts_from_chunks(0, 2, B(out), 33, X_, 1, 64, R_, X_, B(ins), 8, X_, None))  # 32 + 33 > 64
    einval(lib.sdfs_cdc_map_inserts_from_chunks(0, 2, B(out), 32, X_, 0, 64, R_, X_, B(ins), 8, X_, None))  # dst_buf
    # map_insert
    einval(lib.sdfs_cdc_map_insert(0, 1, 64, 8, None, B(ins), 2, X_, B(q), X_, X_, None))
    einval(lib.sdfs_cdc_map_insert(0, 1, 64, 8, B(p), B(ins), 2, X_, B(bad), X_, X_, None))
    einval(lib.sdfs_cdc_map_insert(0, 1, 64, 8, B(p), B(badins), 2, X_, B(q), X_, X_, None))
    einval(lib.sdfs_cdc_map_insert(0, 1, 64, 8, B(p), None, 0, X_, B(q), X_, X_, None))
    einval(lib.sdfs_cdc_map_insert(0, 1, 0, 8, B(p), B(ins), 2, X_, B(q), X_, X_, None))
    einval(lib.sdfs_cdc_map_insert(0, 1, 64, 8, B(p), B(ins), 2, None, B(q), X_, X_, None))
    einval(lib.sdfs_cdc_map_insert(0, 1, 64, 8, B(p), B(ins), 2, X_, B(q), None, X_, None))
    einval(lib.sdfs_cdc_map_insert(0, 1, 64, 8, B(p), B(ins), 2, X_, B(q), X_, None, None))
    einval(lib.sdfs_cdc_map_insert(0, 1, 64, 8, B(p), B(ins), 2, X_, B(p), X_, X_, None))  # out is in
    einval(lib.sdfs_cdc_map_insert(0, 1 << 29, 64, 8, B(p), B(ins), 2, X_, B(q), X_, X_, None))  # scratch too large
    # map_emit_pairs
    einval(lib.sdfs_cdc_map_emit_pairs(0, 1, None, 32, None, None, 0, X_, 461, None, X_, None))
    einval(lib.sdfs_cdc_map_emit_pairs(0, 1, B(bad), 32, None, None, 0, X_, 461, None, X_, None))
    einval(lib.sdfs_cdc_map_emit_pairs(0, 1, B(p), 20, None, None, 0, X_, 461, None, X_, None))
    einval(lib.sdfs_cdc_map_emit_pairs(0, 1, B(p), 32, None, None, 0, X_, 12, None, X_, None))
    einval(lib.sdfs_cdc_map_emit_pairs(0, 1, B(p), 32, None, None, 0, None, 461, None, X_, None))
    einval(lib.sdfs_cdc_map_emit_pairs(0, 1, B(p), 32, None, None, 0, X_, 461, None, None, None))


# ------------------------------------------------------------------------------------------- GPU

def _dev(a, dt=None):
    import torch

    t = torch.from_numpy(np.array(a))
    return t.to("cuda:0") if dt is None else t.to("cuda:0", dt)


def _slots(images, slot_len):
    buf = np.zeros(len(images) * slot_len, np.uint8)
    for b, img in enumerate(images):
        assert len(img) <= slot_len, (b, len(img), slot_len)
        buf[b * slot_len: b * slot_len + len(img)] = np.frombuffer(img, np.uint8)
    return _dev(buf)


def _insert_list(groups, hash_len=32):
    """groups: per buffer the inserts (model pairs, any field values) -> (InsertList, ins_first)."""
    import torch

    from sdfs_amd.extent import InsertList

    rows = [(b, p) for b, g in enumerate(groups) for p in g]
    ins = InsertList.empty(len(rows), "cuda:0")
    if rows:
        hs = np.zeros((len(rows), 32), np.uint8)
        for i, (_, p) in enumerate(rows):
            hs[i, :hash_len] = np.frombuffer(p[X.HASH][:hash_len], np.uint8)
        ins.hash.copy_(_dev(hs))
        ins.hashloc.copy_(_dev(np.array([p[X.HASHLOC] for _, p in rows], np.int64)))
        for name, f in (("len", X.LEN), ("pos", X.POS), ("offset", X.OFFSET), ("nlen", X.NLEN)):
            getattr(ins, name).copy_(_dev(np.array([p[f] for _, p in rows], np.int32)))
        ins.dst_buf.copy_(_dev(np.array([b for b, _ in rows], np.int32)))
    first = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    return ins, _dev(first, torch.int32)


def _host_pairs(p, dup=None):
    """ParsedPairs -> per buffer [(hash, hashloc, len, pos, offset, nlen, dup)]."""
    c = p.counts.cpu().numpy()
    hs, hl, ln, ps, of, nl = (t.cpu().numpy() for t in (p.hashes, p.hashloc, p.len, p.pos, p.offset, p.nlen))
    d = dup.cpu().numpy() if dup is not None else None
    return [[(hs[b, i, :p.hash_len].tobytes(), int(hl[b, i]), int(ln[b, i]), int(ps[b, i]), int(of[b, i]),
              int(nl[b, i]), bool(d[b, i]) if d is not None else False) for i in range(min(int(c[b]), p.cap))]
            for b in range(p.nbuf)]


def _merge_and_check(bases, groups, cl, slot_len, hash_len=32, want_status=None, out_cap=None, images=None):
    """bases: per buffer the base pairs (or `images`: the slots' bytes as they are); groups: per
    buffer the inserts.  Runs parse -> insert -> emit_pairs and compares pairs, dup, status, counts
    and every slot's bytes with the model.  Returns (statuses, result sizes)."""
    import torch

    from sdfs_amd.extent import emit_pairs, insert_pairs
    from sdfs_amd.read import pair_cap, parse_map_slots

    nbuf = len(groups)
    images = images or [X.get_bytes(X.tree(b)) for b in bases]
    m = _slots(images, slot_len)
    before = m.clone()
    slot_pairs = pair_cap(slot_len, hash_len)
    p = parse_map_slots(m, nbuf, slot_len, hash_len)
    ins, first = _insert_list(groups, hash_len)
    cap = out_cap or max(max(len(b) + 2 * len(g) for b, g in zip(bases, groups)), 1)
    out, dup, status = insert_pairs(p, ins, first, cl, slot_pairs, cap)
    doop, skipped = emit_pairs(out, m, slot_len, dup=dup, status=status)
    torch.cuda.synchronize()
    got, st = _host_pairs(out, dup), status.cpu().numpy()
    m, before, doop = m.cpu().numpy(), before.cpu().numpy(), doop.cpu().numpy()
    sizes = []
    for b in range(nbuf):
        slot, old = m[b * slot_len: (b + 1) * slot_len], before[b * slot_len: (b + 1) * slot_len]
        if want_status is not None and want_status[b] & ~_lib.EXT_OVERFLOW:
            assert st[b] == want_status[b], (b, st[b])
            assert (slot == old).all(), b
            _, kept, _, _ = R.parse(images[b], slot_len, hash_len)
            if not st[b] & _lib.EXT_ECAP:
                assert [g[:6] for g in got[b]] == kept and not any(g[6] for g in got[b]), b
            sizes.append(len(kept))
            continue
        ar, _ = run_model(bases[b], groups[b], cl)
        want = [(p_[0][:hash_len],) + tuple(p_[1:]) for p_ in X.values(ar)]
        sizes.append(len(want))
        assert got[b] == want, (b, got[b][:4], want[:4])
        if len(want) > slot_pairs:
            assert st[b] == _lib.EXT_OVERFLOW and (slot == old).all(), b
        else:
            img = X.get_bytes({k: [v[0][:hash_len]] + v[1:] for k, v in ar.items()})
            assert st[b] == 0, (b, st[b])
            assert slot[:len(img)].tobytes() == img and (slot[len(img):] == old[len(img):]).all(), b
            assert int(doop[b]) == sum(w[5] for w in want if w[6])
    assert int(skipped.item()) == int((st != 0).sum())
    return st, sizes


@pytest.mark.gpu
def test_gpu_rules():
    bases = [c[1] for c in CASES]
    groups = [c[2] for c in CASES]
    want = [0] * len(CASES)
    ok = ([bp(0, 0, 10), bp(1, 30, 10)], [bp(9, 5, 30)])
    for badp in [bp(9, 5, 0), X.pair(H(9), PB, 9, 5, 0, -1), X.pair(H(9), PB, 9, -1, 0, 4), X.pair(H(9), PB, 9, 5, -2, 4),
                 X.pair(H(9), PB, -9, 5, 0, 4), bp(9, 60, 5), X.pair(H(9), PB, 9, 5, 0x7FFFFFFF, 4)]:
        for base, good in (ok, ([bp(0, 0, 20), bp(1, 30, 5)], [bp(8, 2, 3), badp, bp(7, 40, 3)])):
            bases.append(base)
            groups.append(good)
            want.append(0 if good is ok[1] else _lib.EXT_BAD_INSERT)
    images = [X.get_bytes(X.tree(b)) for b in bases]
    # a destination that is not disjoint, between good neighbours; one that does not parse
    for img, st in ((R.build_image([bp(0, 0, 20)[:6], bp(1, 10, 20)[:6]]), _lib.EXT_OVERLAP),
                    (R.build_image([bp(0, 0, 20)[:6]], zlen=9), _lib.EXT_CORRUPT)):
        for base, good in (([bp(0, 0, 20), bp(1, 10, 20)], [bp(9, 5, 3)]), ok):
            bases.append(base)
            groups.append(good)
            images.append(img if good is not ok[1] else X.get_bytes(X.tree(base)))
            want.append(st if good is not ok[1] else 0)
    st, _ = _merge_and_check(bases, groups, CL, SLOT8, want_status=want, images=images)
    assert st.tolist() == want


def _random_batch(seed, max_base):
    rng = np.random.default_rng(seed)
    bases, groups = [], []
    for b in range(256):
        base, ins = random_buffer(rng, 4096, 50, 600, 0.15, 6, 900, max_base=max_base, first=b * 64, log_len=True)
        bases.append(base)
        groups.append(ins)
    return bases, groups


@pytest.mark.gpu
@pytest.mark.parametrize("slot_pairs,lo,hi", [(24, 0.0, 0.05), (16, 0.10, 0.50)])
def test_gpu_random_merges(slot_pairs, lo, hi):
    bases, groups = _random_batch(777, slot_pairs)
    over = sum(len(X.values(run_model(b, g, 4096)[0])) > slot_pairs for b, g in zip(bases, groups))
    print(f"{slot_pairs}-pair slots: {over} of 256 buffers overflow in the model")
    assert lo * 256 <= over <= hi * 256
    st, sizes = _merge_and_check(bases, groups, 4096, 13 + 56 * slot_pairs)
    assert int((st == _lib.EXT_OVERFLOW).sum()) == over and not (st & ~_lib.EXT_OVERFLOW).any()


def _tiled(n, width, first=0, offset=1):
    return [bp(first + i, i * width, width, offset=offset) for i in range(n)]


@pytest.mark.gpu
def test_gpu_wave_and_path_edges():
    """Results of 63, 64 and 65 pairs; work lists of exactly 256 elements (the last buffer of the
    LDS kernel) and 257 (the first of the global-memory kernel); 1 500 pairs with 300 inserts."""
    cl = 262144
    rng = np.random.default_rng(5)
    bases, groups = [], []
    for n in (63, 64, 65):  # n - 2 pairs, one insert strictly inside one of them: + 2
        bases.append(_tiled(n - 2, 16))
        groups.append([bp(900, 16 * 40 + 3, 5)])
    for n0 in (250, 251):  # n0 + 2 * 3 = 256, 257
        bases.append(_tiled(n0, 16))
        # two splits (+ 2 each) and one insert that removes two pairs and cuts two (- 1)
        groups.append([bp(900, 16 * 100 + 3, 5), bp(901, 16 * 10 - 2, 40), bp(902, 16 * 249 + 1, 2)])
    for k in range(2):
        base = _tiled(1500, 100, offset=7)
        ins = []
        for j in range(300):
            n = int(rng.integers(1, 700))
            ins.append(bp(2000 + j, int(rng.integers(0, 150000 - n)), n, offset=j))
        bases.append(base)
        groups.append(ins)
    bases.append(_tiled(300, 16))  # copied through by the global-memory kernel
    groups.append([])
    st, sizes = _merge_and_check(bases, groups, cl, 13 + 56 * 2200)
    assert sizes[:5] == [63, 64, 65, 250 + 3, 251 + 3] and min(sizes[5:7]) > 1000 and sizes[7] == 300
    assert not st.any()


@pytest.mark.gpu
def test_gpu_slot_capacity_and_ecap():
    """128 and 129 pairs in the default 7 181-byte slots: fits / OVERFLOW; out->cap one short: ECAP
    with the needed count and nothing written."""
    import torch

    from sdfs_amd.extent import insert_pairs
    from sdfs_amd.read import parse_map_slots

    slot_len, cl = 7181, 262144
    bases = [_tiled(126, 64), _tiled(127, 64), _tiled(20, 64)]
    groups = [[bp(900, 64 * 5 + 1, 9)], [bp(900, 64 * 5 + 1, 9)], []]
    st, sizes = _merge_and_check(bases, groups, cl, slot_len)
    assert sizes == [128, 129, 20] and st.tolist() == [0, _lib.EXT_OVERFLOW, 0]
    # out->cap = 128: buffer 1 needs 129
    m = _slots([X.get_bytes(X.tree(b)) for b in bases], slot_len)
    p = parse_map_slots(m, 3, slot_len, 32)
    ins, first = _insert_list(groups)
    out, dup, status = insert_pairs(p, ins, first, cl, 128, 128)
    out.pos.fill_(-7)  # insert_pairs zero-fills; nothing may be written for the ECAP buffer
    dup.fill_(9)
    check = _lib.check(_lib.load().sdfs_cdc_map_insert(0, 3, cl, 128, ctypes.byref(p.c), ctypes.byref(ins.c), ins.cap,
                                                       first.data_ptr(), ctypes.byref(out.c), dup.data_ptr(),
                                                       status.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert check == 0 and status.tolist() == [0, _lib.EXT_ECAP, 0] and out.counts.tolist() == [128, 129, 20]
    assert (out.pos[1] == -7).all() and (dup[1] == 9).all()
    assert (out.pos[0] != -7).all() and (out.pos[2, :20] != -7).all() and (out.pos[2, 20:] == -7).all()


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["sha256", "md5"])
def test_gpu_emit_pairs_reproduces_writer_images(algo):
    import torch

    from sdfs_amd import HipVariableMD5HashEngine, HipVariableSha256HashEngine
    from sdfs_amd.device import DeviceBatch
    from sdfs_amd.extent import emit_pairs
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
    again = torch.full_like(m, 0xEE)
    d = torch.zeros((nbuf, p.cap), dtype=torch.uint8, device="cuda:0")
    d[:, 1::3] = 1
    doop2, skipped = emit_pairs(p, again, sl, dup=d)
    plain = torch.full_like(m, 0xEE)
    doop0, _ = emit_pairs(p, plain, sl)
    torch.cuda.synchronize()
    assert int(ovf.item()) == 0 and int(skipped.item()) == 0 and int(doop.sum().item()) > 0
    m, again, plain = (t.cpu().numpy().reshape(nbuf, sl) for t in (m, again, plain))
    counts, nlen = p.counts.cpu().numpy(), p.nlen.cpu().numpy()
    for b in range(nbuf):
        n = int(counts[b])
        end = 9 + n * (hl + 24)
        want = int(nlen[b, :n][1::3].sum())
        assert (again[b, :end] == m[b, :end]).all() and (plain[b, :end] == m[b, :end]).all()
        assert int.from_bytes(again[b, end:end + 4].tobytes(), "big") == want == int(doop2[b].item())
        assert int.from_bytes(plain[b, end:end + 4].tobytes(), "big") == 0 == int(doop0[b].item())
        assert (again[b, end + 4:] == 0xEE).all() and (plain[b, end + 4:] == 0xEE).all()
    ix.destroy()
    e.destroy()


@pytest.mark.gpu
def test_gpu_map_extents_vs_get_wl():
    import torch

    from sdfs_amd.extent import group_inserts, map_extents
    from sdfs_amd.read import parse_map_slots

    cl, slot_len = 4096, 13 + 56 * 24
    src = [
        [bp(1, 0, 100, offset=5), bp(2, 100, 50), bp(3, 150, 1), bp(4, 151, 849, offset=9), bp(5, 1200, 300)],
        [],                                                    # a never-written slot
        [bp(20 + i, 64 * i, 64, offset=i) for i in range(20)],  # 0 .. 1280 tiled
        [bp(50, 0, 30), bp(51, 20, 30)],                        # not disjoint
    ]
    segs = [
        (0, 10, 0, 7, 80),       # inside one pair
        (0, 0, 1, 1000, 100),    # exactly one pair
        (0, 100, 1, 0, 51),      # two pairs, boundary to boundary
        (0, 30, 2, 333, 900),    # starts and ends inside pairs, four of them
        (0, 0, 0, 500, 1000),    # up to the hole's edge
        (0, 900, 0, 0, 200),     # runs into the hole: HOLE
        (0, 1000, 0, 0, 100),    # starts in the hole: HOLE
        (0, 1100, 0, 0, 200),    # starts in the hole, ends covered: HOLE
        (0, 1499, 3, 4095, 1),   # the last byte of the last pair
        (0, 1499, 3, 0, 2),      # one past it: HOLE
        (1, 0, 0, 0, 10),        # the empty slot: HOLE
        (2, 0, 2, 2000, 1280),   # twenty pairs
        (2, 63, 1, 5, 66),       # one byte, a whole pair, one byte
        (2, 1279, 1, 0, 2),      # past the end: HOLE
        (3, 0, 0, 0, 10),        # SRC
        (2, 64, 3, 64, 128),
    ]
    m = _slots([R.build_image([p[:6] for p in b]) for b in src], slot_len)
    p = parse_map_slots(m, 4, slot_len, 32)
    ins, first, status = map_extents(p, segs, 4, cl)
    small, first_s, _ = map_extents(p, segs, 4, cl, n_ins_cap=int(1))
    torch.cuda.synchronize()
    first, status = first.cpu().numpy(), status.cpu().numpy()
    rows = list(zip(ins.hash.cpu().numpy(), ins.hashloc.tolist(), ins.len.tolist(), ins.pos.tolist(),
                    ins.offset.tolist(), ins.nlen.tolist(), ins.dst_buf.tolist()))
    n = 0
    for s, (sb, so, db, do, ln) in enumerate(segs):
        want, st = [], 0
        if s == 14:
            st = _lib.EXT_SRC
        else:
            ar, x = X.tree(src[sb]), so
            try:
                while x < so + ln:
                    w = X.get_wl(ar, x)
                    k = min(w[X.NLEN], so + ln - x)
                    want.append((w[X.HASH], w[X.HASHLOC], w[X.LEN], do + x - so, w[X.OFFSET], k, db))
                    x += k
            except X.NotFound:
                want, st = [], _lib.EXT_HOLE
        assert status[s] == st, (s, status[s], st)
        assert first[s] == n and first[s + 1] == n + len(want), s
        got = [(h.tobytes(),) + tuple(r) for h, *r in rows[n:n + len(want)]]
        assert got == want, s
        n += len(want)
    assert n > 30 and all(r[6] == 4 for r in rows[n:])  # rows past the total keep the fill
    assert first_s.tolist() == first.tolist() and small.dst_buf.tolist() == [4]  # too small: nothing written
    # grouped by destination buffer, list order kept
    g, gfirst = group_inserts(ins, 4)
    torch.cuda.synchronize()
    gfirst = gfirst.tolist()
    by_buf = [[r[1:] for r in rows[:n] if r[6] == b] for b in range(4)]
    grows = list(zip(g.hashloc.tolist(), g.len.tolist(), g.pos.tolist(), g.offset.tolist(), g.nlen.tolist(),
                     g.dst_buf.tolist()))
    assert gfirst[0] == 0 and gfirst[4] == n
    for b in range(4):
        assert grows[gfirst[b]:gfirst[b + 1]] == by_buf[b], b


@pytest.mark.gpu
@pytest.mark.parametrize("n_seg", [1023, 1025, 2049])
def test_gpu_map_extents_many_segments(n_seg):
    """seg_first is a one-block prefix over the segments' piece counts: 1 023 leaves its last
    thread without a segment, 1 025 and 2 049 give a thread more than one and are no multiple of
    the block.  Short segments over two source buffers, some of them ending in a hole (no
    pieces); seg_first (all n_seg + 1 entries), seg_status and the pieces against the model."""
    import torch

    from sdfs_amd.extent import map_extents
    from sdfs_amd.read import parse_map_slots

    cl, slot_len = 4096, 13 + 56 * 24
    src = [[bp(20 + i, 64 * i, 64, offset=i) for i in range(20)],       # 0 .. 1280 tiled
           [bp(60 + i, 55 * i, 55, offset=2 * i) for i in range(20)]]  # 0 .. 1100 tiled
    # (src_buf, src_off, dst_buf, dst_off, len): 1 .. 70 bytes, so one to three pieces each
    segs = [(s % 2, (s * 37) % 1200, s % 3, (s * 11) % 4000, 1 + s % 70) for s in range(n_seg)]
    m = _slots([R.build_image([p[:6] for p in b]) for b in src], slot_len)
    p = parse_map_slots(m, 2, slot_len, 32)
    ins, first, status = map_extents(p, segs, 3, cl, n_ins_cap=3 * n_seg)
    torch.cuda.synchronize()
    first, status = first.cpu().numpy(), status.cpu().numpy()
    rows = list(zip(ins.hash.cpu().numpy(), ins.hashloc.tolist(), ins.len.tolist(), ins.pos.tolist(),
                    ins.offset.tolist(), ins.nlen.tolist(), ins.dst_buf.tolist()))
    trees = [X.tree(b) for b in src]
    want_first, want_status, want = [0], [], []
    for sb, so, db, do, ln in segs:
        pieces, st, x = [], 0, so
        try:
            while x < so + ln:
                w = X.get_wl(trees[sb], x)
                k = min(w[X.NLEN], so + ln - x)
                pieces.append((w[X.HASH], w[X.HASHLOC], w[X.LEN], do + x - so, w[X.OFFSET], k, db))
                x += k
        except X.NotFound:
            pieces, st = [], _lib.EXT_HOLE
        want += pieces
        want_status.append(st)
        want_first.append(len(want))
    assert want_status.count(_lib.EXT_HOLE) >= 50 and len(want) > n_seg  # both kinds occur
    assert first.tolist() == want_first
    assert status.tolist() == want_status
    got = [(h.tobytes(),) + tuple(r) for h, *r in rows[:len(want)]]
    assert got == want
    assert all(r[6] == 3 for r in rows[len(want):])  # rows past the total keep the fill


# ---- end to end: the writer's store, copies and rewrites, the reader, the index

_KEY = bytes(range(7, 39))
L, NBUF = 262144, 8
_BASE = {}


def _base(variant):
    """Eight buffers of engine chunks written through HipBufferWriter (lz4, or aes = LZ4 + AES-256 in
    version 1 archives).  The device state is made afresh per test (the tests change the index and
    the slots); the host copy of the data is shared."""
    import torch

    from sdfs_amd import HipVariableSha256HashEngine
    from sdfs_amd.archive import HipBufferWriter
    from sdfs_amd.device import DeviceBatch
    from sdfs_amd.index import HipHashesMap
    from sdfs_amd.meta import slot_bytes

    e = HipVariableSha256HashEngine()
    batch = DeviceBatch(e, nbuf=NBUF, buf_len=L)
    batch.fill_streams(first_stream=5150, bufs_per_stream=2)
    v = batch.data.view(NBUF, L)
    v[1, 20000:120000] = 0
    v[6].copy_(v[2])
    ix = HipHashesMap(1 << 13)
    aes = variant == "aes"
    wr = HipBufferWriter(ix, compress=True, aes=_KEY if aes else None, version=1 if aes else 0,
                         blocksz=[200000, 260000, 150000])
    m, arcs = wr.write(batch, PB)
    torch.cuda.synchronize()
    assert int(arcs.extra["overflow"].item()) == 0
    if variant not in _BASE:
        _BASE[variant] = batch.data.cpu().numpy().copy()
    return dict(engine=e, ix=ix, wr=wr, m=m, arcs=arcs, data=_BASE[variant], slot_len=slot_bytes(32, L, 4095), aes=aes)


def _read(w, m, nbuf, store, directory, ivs=None):
    import torch

    from sdfs_amd.read import HipBufferReader

    rd = HipBufferReader(L, 32, aes=_KEY if w["aes"] else None, record_ivs=w["aes"], engine=w["engine"])
    out = torch.full((nbuf, L), 0xFF, dtype=torch.uint8, device="cuda:0")
    got, status, _ = rd.read(m, nbuf, w["slot_len"], store, *directory, PB, out=out, store_ivs=ivs)
    torch.cuda.synchronize()
    rd.destroy()
    return got.cpu().numpy().reshape(-1), status.cpu().numpy()


def _named_counts(w, maps):
    """{fingerprint: the number of pairs naming it} over the given slots (a host count)."""
    import torch

    from sdfs_amd.read import parse_map_slots

    named = {}
    for m, nbuf in maps:
        p = parse_map_slots(m, nbuf, w["slot_len"], 32)
        torch.cuda.synchronize()
        assert not p.status.any()
        for pairs in _host_pairs(p):
            for q in pairs:
                named[q[0]] = named.get(q[0], 0) + 1
    return named


def _refcounts(ix, digests):
    pos, ref = ix.get_digests(_dev(np.frombuffer(b"".join(digests), np.uint8).reshape(-1, 32).copy()))
    return pos.tolist(), ref.tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["lz4", "aes"])
def test_gpu_copy_extents_end_to_end(variant):
    import torch

    from sdfs_amd import copy_extents

    w = _base(variant)
    before = _named_counts(w, [(w["m"], NBUF)])
    dst = torch.zeros(NBUF * w["slot_len"], dtype=torch.uint8, device="cuda:0")  # a second, empty file
    want = np.zeros(NBUF * L, np.uint8)
    m_before = w["m"].clone()
    for sstart, dstart, length in [(70001, 123457, 5 * L + 31111), (1000003, 200001, 2 * L + 777)]:
        segs = split_extent(sstart, dstart, length, L)
        assert all(s[1] % 4096 or s[3] % 4096 for s in segs)
        _, status, seg_status, info = copy_extents(w["m"], dst, NBUF, NBUF, w["slot_len"], segs, index=w["ix"],
                                                   chunk_length=L)
        torch.cuda.synchronize()
        assert info.written and not status.any() and not seg_status.any() and int(info.skipped.item()) == 0
        want[dstart:dstart + length] = w["data"][sstart:sstart + length]
    assert torch.equal(w["m"], m_before)  # the source file's slots are read only
    got, status = _read(w, dst, NBUF, w["arcs"].store, w["arcs"].directory(), w["arcs"].record_ivs())
    assert not status.any()
    assert (got == want).all()
    named = _named_counts(w, [(w["m"], NBUF), (dst, NBUF)])
    assert set(named) == set(before) and any(named[k] > before[k] for k in named)
    keys = sorted(named)
    pos, ref = _refcounts(w["ix"], keys)
    assert ref == [named[k] for k in keys] and min(pos) >= PB
    w["wr"].destroy()
    w["ix"].destroy()
    w["engine"].destroy()


@pytest.mark.gpu
def test_gpu_copy_extents_stops_on_a_hole():
    import torch

    from sdfs_amd import copy_extents

    w = _base("lz4")
    src = torch.zeros(2 * w["slot_len"], dtype=torch.uint8, device="cuda:0")
    src[: w["slot_len"]].copy_(w["m"][: w["slot_len"]])  # buffer 1 of this file was never written
    dst = w["m"].clone()
    _, status, seg_status, info = copy_extents(src, dst, 2, NBUF, w["slot_len"], split_extent(1000, 5000, L, L),
                                               index=w["ix"], chunk_length=L)
    torch.cuda.synchronize()
    assert seg_status.tolist() == [0, 0, _lib.EXT_HOLE][:len(seg_status)] and len(seg_status) == 3
    assert not info.written and torch.equal(dst, w["m"]) and not status.any()
    w["wr"].destroy()
    w["ix"].destroy()
    w["engine"].destroy()


@pytest.mark.gpu
def test_gpu_rewrite_blocks_end_to_end():
    import torch

    from sdfs_amd import rewrite_blocks
    from sdfs_amd.device import DeviceBatch

    w = _base("lz4")
    ix, arcs1 = w["ix"], w["arcs"]
    before = _named_counts(w, [(w["m"], NBUF)])
    RL = 65536
    runs = DeviceBatch(w["engine"], nbuf=NBUF, buf_len=RL)
    runs.fill_streams(first_stream=9090, bufs_per_stream=1)
    base_dev = _dev(w["data"])
    rv = runs.data.view(NBUF, RL)
    for b in range(1, NBUF, 2):  # every second run repeats bytes that are stored already
        rv[b].copy_(base_dev[(b - 1) * L + 30000: (b - 1) * L + 30000 + RL])
    run_data = runs.data.cpu().numpy().copy()
    run_pos = [100003 + 17 * b for b in range(NBUF)]
    pb2 = PB + int(arcs1.store_off.shape[0])
    _, status, arcs2, info = rewrite_blocks(w["wr"], runs, pb2, w["m"], NBUF, w["slot_len"], list(range(NBUF)), run_pos,
                                            chunk_length=L)
    torch.cuda.synchronize()
    assert not status.any() and int(info.skipped.item()) == 0 and info.n_inserts == int(runs.total.item())
    assert int(arcs2.extra["dup"][: info.n_inserts].sum().item()) > 0  # the repeated runs found their chunks
    want = w["data"].copy()
    for b in range(NBUF):
        want[b * L + run_pos[b]: b * L + run_pos[b] + RL] = run_data[b * RL: (b + 1) * RL]
    store = torch.cat([arcs1.store, arcs2.store])
    directory = (torch.cat([arcs1.store_off, arcs2.store_off + arcs1.store.numel()]),
                 torch.cat([arcs1.store_len, arcs2.store_len]), torch.cat([arcs1.raw_len, arcs2.raw_len]))
    got, rstatus = _read(w, w["m"], NBUF, store, directory)
    assert not rstatus.any()
    assert (got == want).all()
    named = _named_counts(w, [(w["m"], NBUF)])
    keys = sorted(set(named) | set(before))
    pos, ref = _refcounts(ix, keys)
    assert ref == [named.get(k, 0) for k in keys]
    dead = {k for k in keys if k not in named}
    assert dead and all(p >= PB for p in pos)  # overwritten fingerprints sit at count 0 until the sweep
    digests, swept_pos, left = ix.sweep()
    assert {d.tobytes() for d in digests.cpu().numpy()} == dead and left == 0
    assert _refcounts(ix, sorted(dead))[0] == [-1] * len(dead)
    w["wr"].destroy()
    ix.destroy()
    w["engine"].destroy()


@pytest.mark.gpu
def test_gpu_rewrite_blocks_flagged_destination_moves_no_counts():
    """A destination whose pairs overlap keeps its image; its run's records, which put_records has
    counted, are released again and go with the next sweep."""
    import torch

    from sdfs_amd import rewrite_blocks
    from sdfs_amd.device import DeviceBatch

    w = _base("lz4")
    ix, sl = w["ix"], w["slot_len"]
    nlen0 = 3 * sl + 9 + 32 + 8 + 12  # buffer 3, pair 0, nlen: five bytes into pair 1
    w["m"][nlen0 + 3] += 5
    before = _named_counts(w, [(w["m"], NBUF)])
    m_before = w["m"].clone()
    RL = 65536
    runs = DeviceBatch(w["engine"], nbuf=2, buf_len=RL)
    runs.fill_streams(first_stream=9190, bufs_per_stream=1)
    _, status, arcs2, info = rewrite_blocks(w["wr"], runs, PB + int(w["arcs"].store_off.shape[0]), w["m"], NBUF, sl,
                                            [3, 5], [4099, 77], chunk_length=L)
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0, 0, _lib.EXT_OVERLAP, 0, 0, 0, 0] and int(info.skipped.item()) == 1
    assert torch.equal(w["m"][3 * sl: 4 * sl], m_before[3 * sl: 4 * sl])
    assert not torch.equal(w["m"][5 * sl: 6 * sl], m_before[5 * sl: 6 * sl])
    counts, _, _, dg, _ = runs.host_results()
    released = {dg[0, i].tobytes() for i in range(int(counts[0]))}
    named = _named_counts(w, [(w["m"], NBUF)])
    assert not released & set(named) and all(dg[1, i].tobytes() in named for i in range(int(counts[1])))
    keys = sorted(set(named) | set(before) | released)
    pos, ref = _refcounts(ix, keys)
    assert ref == [named.get(k, 0) for k in keys] and min(pos) >= PB
    digests, _, left = ix.sweep()
    assert {d.tobytes() for d in digests.cpu().numpy()} == {k for k in keys if k not in named} >= released
    w["wr"].destroy()
    ix.destroy()
    w["engine"].destroy()
