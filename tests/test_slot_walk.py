"""What the shared slot walk (csrc/store_format.h) and the shared block scan (csrc/block_scan.h)
add over the consumers' own suites.

The rule is one rule: the same seeded slot images go to ``sdfs_cdc_map_parse``, to
``sdfs_cdc_index_claim_slots`` and to ``sdfs_cdc_import_pairs``; the three must give
``read_model.parse``'s status per slot, the same pair counts and ``ingest_model.counting_pairs``'
set.  Capacity 7 is one 64-lane pass; capacity 300 is more than four passes and more than one
256-pair part, so the part boundary and the ``j > i`` tail of the TreeMap.put rule cross it.

The scan's edges, through entry points that exist: ``put_records`` around one and two tiles of
block sums, ``export`` over 2048 block sums, ``import_plan``'s three 64-bit sums over 1026 block
sums, ``ingest_chunks_plan`` around one and two tiles.  Each is compared with a cumsum."""
import ctypes
import functools
import random
import struct

import numpy as np
import pytest

from sdfs_amd import _lib
from tests import ingest_model as IM
from tests import mapfile_model as MM
from tests import read_model as R
from tests.slot_images import KINDS, held as make_held, seeded_image

N_IMAGES = 300
SEED = 2025  # chosen so that test_seeded_set_holds_every_case holds (checked with the models alone)
TILE = 1024
BIG = TILE * TILE + TILE + 1  # 1026 block sums: the second tile of block_sums_to_bases


@functools.lru_cache(maxsize=None)
def _image_set(hl, cap):
    """-> (slot_bytes, held, images, kinds, per image (status, counting pairs))."""
    rng = random.Random(SEED * 100 + hl + cap)
    sb = 13 + cap * (hl + 24) + 3
    held = make_held(rng, 200, hl)
    made = [seeded_image(rng, held, hl, cap) for _ in range(N_IMAGES)]
    images, kinds = [m[0] for m in made], [m[1] for m in made]
    return sb, held, images, kinds, [IM.counting_pairs(img, sb, hl) for img in images]


def _pos_column(img, hl):
    n = struct.unpack(">i", img[5:9])[0]
    bal = hl + 24
    return [struct.unpack(">i", img[9 + i * bal + hl + 12: 9 + i * bal + hl + 16])[0] for i in range(n)]


@pytest.mark.parametrize("hl", [32, 16])
@pytest.mark.parametrize("cap", [7, 300])
def test_seeded_set_holds_every_case(hl, cap):
    sb, held, images, kinds, model = _image_set(hl, cap)
    assert set(kinds) == set(KINDS)
    for img, (st, pairs) in zip(images, model):
        assert st == R.parse(img, sb, hl)[0] and len(pairs) == len(R.parse(img, sb, hl)[1])
    assert any(st for st, _ in model) and any(len(p) > 64 for _, p in model) == (cap == 300)
    if cap == 300:  # a repeated pos with one pair below index 256 and one at or above it
        def straddles(img):
            where = {}
            for i, ps in enumerate(_pos_column(img, hl)):
                where.setdefault(ps, []).append(i)
            return any(v[0] < 256 <= v[-1] for v in where.values() if len(v) > 1)

        assert any(k == "repeat" and straddles(img) for img, k in zip(images, kinds))


def _import_pairs(torch, req, nreq, sb, hl, stride):
    dev = req.device
    places = nreq * stride
    e = lambda k, dt: torch.zeros(k, dtype=dt, device=dev)  # noqa: E731
    wt = dict(hashes=torch.zeros((places, 32), dtype=torch.uint8, device=dev), src_hashloc=e(places, torch.int64),
              counting=e(places, torch.uint8), status=e(nreq, torch.int32), req_pairs=e(nreq, torch.int32),
              req_missed=e(nreq, torch.int32), pair_fetch=e(places, torch.int32), pair_rec=e(places, torch.int32),
              counts=e(8, torch.int64))
    work = _lib.ImportWork(**{k: v.data_ptr() for k, v in wt.items()})
    _lib.check(_lib.load().sdfs_cdc_import_pairs(0, req.data_ptr(), nreq, sb, hl, stride, ctypes.byref(work),
                                                 torch.cuda.current_stream().cuda_stream))
    return wt, work


@pytest.mark.gpu
@pytest.mark.parametrize("hl", [32, 16])
@pytest.mark.parametrize("cap", [7, 300])
def test_gpu_the_rule_is_one_rule(hl, cap):
    torch = pytest.importorskip("torch")
    from sdfs_amd.index import HipHashesMap
    from sdfs_amd.read import pair_cap, parse_map_slots

    sb, held, images, kinds, model = _image_set(hl, cap)
    assert pair_cap(sb, hl) == cap
    n = len(images)
    host = np.zeros((n, sb), np.uint8)
    for r, img in enumerate(images):
        host[r, : len(img)] = np.frombuffer(img, np.uint8)
    m = torch.from_numpy(host).cuda()
    want_status = [st for st, _ in model]
    want_count = [len(p) for _, p in model]

    # the read path's parse
    pp = parse_map_slots(m.view(-1), n, sb, hl)
    assert pp.status[:n].tolist() == want_status
    assert pp.counts[:n].tolist() == want_count

    # the import's pairs: status, image pairs, and the counting set by image place
    wt, _ = _import_pairs(torch, m, n, sb, hl, cap)
    assert wt["status"].tolist() == want_status
    counting = wt["counting"].view(n, cap).cpu().numpy()
    hashes = wt["hashes"].view(n, cap, 32).cpu().numpy()
    locs = wt["src_hashloc"].view(n, cap).cpu().numpy()
    assert counting.sum(axis=1).tolist() == want_count
    for r, (st, pairs) in enumerate(model):
        got = [(int(i), hashes[r, i, :hl].tobytes(), int(locs[r, i])) for i in np.flatnonzero(counting[r])]
        assert got == pairs
    zlens = [max(struct.unpack(">i", host[r, 5:9].tobytes())[0], 0) for r in range(n)]
    assert wt["req_pairs"].tolist() == [0 if st else z for st, z in zip(want_status, zlens)]

    # the claim: the set it applies, from the slots' misses, the total and every entry's count
    ix = HipHashesMap(4096)
    dg = torch.from_numpy(np.frombuffer(b"".join(d for d, _ in held), np.uint8).reshape(-1, 32).copy()).cuda()
    pos = torch.tensor([p for _, p in held], dtype=torch.int64)
    assert ix.load(dg, pos, torch.full((len(held),), 1 << 20, dtype=torch.int64)).cpu().tolist() == [0] * len(held)
    where = dict(held)
    hits = {d: 0 for d in where}
    want_missed = []
    for _, pairs in model:
        miss = 0
        for _, h, loc in pairs:
            if where.get(MM.pad32(h)) == loc:
                hits[MM.pad32(h)] += 1
            else:
                miss += 1
        want_missed.append(miss)
    res = ix.claim_slots(m.view(-1), n, sb, -1, hash_len=hl)
    assert res.slot_status.tolist() == want_status
    assert res.slot_missed.tolist() == want_missed
    assert (res.applied, res.missed, res.corrupt) == (sum(hits.values()), sum(want_missed), sum(map(bool, want_status)))
    assert res.applied + res.missed == sum(want_count) == int(pp.counts[:n].sum().item())
    _, ref = ix.get_digests(dg)
    assert ref.tolist() == [(1 << 20) - hits[d] for d, _ in held]
    assert res.applied > 100 and res.missed > 10 and res.corrupt > 10
    ix.destroy()


# ------------------------------------------------------------------------------------------
# the scan's edges
# ------------------------------------------------------------------------------------------
def _mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _digests_of(torch, keys):
    """int64 keys -> uint8 [n, 32] digests, equal keys alike, distinct keys distinct."""
    k = keys.to(torch.int64)
    w = torch.stack([k * 0x1E3779B97F4A7C15 - 0x61C8864680B583EB, k ^ 0x5851F42D4C957F2D, k * 31 + 7, ~k], dim=1)
    return w.contiguous().view(torch.uint8).view(-1, 32)


@pytest.fixture(scope="module")
def big_index():
    from sdfs_amd.index import HipHashesMap

    ix = HipHashesMap(1 << 20)  # 2^21 slots: 2048 block sums; the smallest that takes BIG records
    yield ix
    ix.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049, BIG])
def test_gpu_put_records_ranks_across_tiles(big_index, n):
    import torch

    ix = big_index
    ix.clear()
    g = torch.Generator().manual_seed(n)
    keys = torch.randint(0, n // 2 + 1, (n,), generator=g).cuda()  # about half repeat an earlier key
    recs = torch.zeros((n, _lib.RECORD_BYTES), dtype=torch.uint8, device="cuda")
    recs[:, :32] = _digests_of(torch, keys)
    pos_base = 5_000_000_000
    dup, loc, new, nc = ix.put_records(recs, None, pos_base=pos_base)
    idx = torch.arange(n, device="cuda")
    uniq, inv = torch.unique(keys, return_inverse=True)
    first = torch.full((uniq.numel(),), n, dtype=torch.int64, device="cuda").scatter_reduce(0, inv, idx, "amin")
    isnew = first[inv] == idx
    rank = torch.cumsum(isnew.to(torch.int64), 0) - isnew.to(torch.int64)
    assert int(nc.item()) == int(isnew.sum().item()) == uniq.numel()
    assert torch.equal(dup.to(torch.bool), ~isnew)
    assert torch.equal(loc, pos_base + rank[first[inv]])
    assert torch.equal(new[: uniq.numel()].to(torch.int64), idx[isnew])
    if n >= 1024:
        assert 0.3 * n < uniq.numel() < 0.6 * n


@pytest.mark.gpu
def test_gpu_export_in_table_order_over_2048_block_sums(big_index):
    import torch

    ix = big_index
    ix.clear()
    slots = 1 << 21
    rng = np.random.default_rng(11)
    keys = torch.from_numpy(rng.integers(1, 1 << 62, 400_000))
    dg = _digests_of(torch, keys).numpy()
    home = (_mix64(dg[:, :8].copy().view(np.uint64)[:, 0]) & np.uint64(slots - 1)).astype(np.int64)
    # no two entries in the same or in neighbouring slots: every entry lies in its home slot
    order = np.argsort(home, kind="stable")
    keep = order[np.concatenate([[True], np.diff(home[order]) > 1])]
    block = home[keep] >> 10
    must = [keep[np.flatnonzero(block == b)[0]] for b in (0, 1023, 1024, 2047)]
    pick = np.unique(np.concatenate([must, rng.choice(keep, 3000, replace=False)]))
    pick = pick[np.argsort(home[pick])]
    assert {0, 1023, 1024, 2047} <= set((home[pick] >> 10).tolist()) and (np.diff(home[pick]) > 1).all()
    shuffled = rng.permutation(pick)
    pos = torch.from_numpy(shuffled.astype(np.int64) + 77)
    ref = torch.from_numpy((shuffled % 5).astype(np.int64) - 1)
    assert ix.load(torch.from_numpy(dg[shuffled]).cuda(), pos, ref).cpu().tolist() == [0] * len(pick)
    for cap in (None, 1500):
        edg, epos, eref, held = ix.export(cap)
        k = len(pick) if cap is None else cap
        assert held == len(pick) and epos.shape[0] == k
        assert (edg.cpu().numpy() == dg[pick[:k]]).all()
        assert epos.tolist() == (pick[:k] + 77).tolist() and eref.tolist() == ((pick[:k] % 5) - 1).tolist()


@pytest.mark.gpu
def test_gpu_import_plan_three_sums_across_tiles():
    torch = pytest.importorskip("torch")
    n_src, nreq, stride = BIG, 16, 256
    places = nreq * stride
    rng = np.random.default_rng(5)
    nblk = (n_src + TILE - 1) // TILE
    ks = np.concatenate([[3, 1023 * TILE + 5, 1024 * TILE, 1024 * TILE + 1023, (nblk - 1) * TILE, n_src - 1],
                         rng.integers(0, n_src, places - 6)])
    ks[100:140] = ks[60:100]             # some entries are wanted by more than one pair
    counting = (rng.random(places) < 0.9).astype(np.uint8)
    counting[:6] = 1
    held = rng.random(places) < 0.2      # the index holds these fingerprints: not wanted
    held[:6] = False
    src_base = 1_000_000
    store_raw = rng.integers(1, 70000, n_src).astype(np.int32)
    store_len = rng.integers(1, 70000, n_src).astype(np.int32)
    store_off = np.cumsum(store_len.astype(np.int64)) * 3
    wanted = np.unique(ks[(counting == 1) & ~held])
    assert {0, 1023, 1024, nblk - 1} <= set((wanted // TILE).tolist()) and len(wanted) > 2000

    dev = "cuda"
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    z = lambda k, dt: torch.zeros(k, dtype=dt, device=dev)  # noqa: E731
    wt = dict(hashes=z((places, 32), torch.uint8), src_hashloc=up(ks.astype(np.int64) + src_base), counting=up(counting),
              status=z(nreq, torch.int32), req_pairs=z(nreq, torch.int32), req_missed=z(nreq, torch.int32),
              pair_fetch=z(places, torch.int32), pair_rec=z(places, torch.int32), counts=z(8, torch.int64))
    work = _lib.ImportWork(**{k: v.data_ptr() for k, v in wt.items()})
    pos = up(np.where(held, 9, -1).astype(np.int64))
    d_off, d_len, d_raw = up(store_off), up(store_len), up(store_raw)
    nf = len(wanted)
    out = dict(fetch_count=z(1, torch.int32), src_off=z(places, torch.int64), src_len=z(places, torch.int32),
               dst_off=z(places, torch.int64), dst_cap=z(places, torch.int32), plain_off=z(places, torch.int64),
               total_bytes=z(2, torch.int64))  # a fetch per place at the most
    _lib.check(_lib.load().sdfs_cdc_import_plan(
        0, nreq, stride, ctypes.byref(work), pos.data_ptr(), src_base, n_src, d_off.data_ptr(), d_len.data_ptr(),
        d_raw.data_ptr(), 1 << 20, out["fetch_count"].data_ptr(), out["src_off"].data_ptr(), out["src_len"].data_ptr(),
        out["dst_off"].data_ptr(), out["dst_cap"].data_ptr(), out["plain_off"].data_ptr(),
        out["total_bytes"].data_ptr(), torch.cuda.current_stream().cuda_stream))
    r16 = lambda a: (a.astype(np.int64) + 15) & ~15  # noqa: E731
    dsz, psz = r16(store_raw[wanted]), r16(store_len[wanted])
    assert out["fetch_count"].item() == nf and wt["status"].tolist() == [0] * nreq
    assert out["src_off"][:nf].tolist() == store_off[wanted].tolist()
    assert out["src_len"][:nf].tolist() == store_len[wanted].tolist()
    assert out["dst_cap"][:nf].tolist() == store_raw[wanted].tolist()
    assert out["dst_off"][:nf].tolist() == (np.cumsum(dsz) - dsz).tolist()
    assert out["plain_off"][:nf].tolist() == (np.cumsum(psz) - psz).tolist()
    assert out["total_bytes"].tolist() == [int(dsz.sum()), int(psz.sum())]
    want_fetch = np.where((counting == 1) & ~held, np.searchsorted(wanted, ks), -1)
    assert wt["pair_fetch"].tolist() == want_fetch.tolist()
    assert wt["counts"][2].item() == nf and wt["counts"][3].item() == int(store_raw[wanted].sum())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_gpu_ingest_plan_across_tiles(n):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(n)
    cl, blob_len = 4096, 1 << 20
    ents = []
    for i in range(n):
        comp = int(rng.random() < 0.4)
        raw = int(rng.integers(1, cl + 1))
        ln = int(rng.integers(1, 3000)) if comp else raw
        u = rng.random()
        if u < 0.05:
            ln = 0                       # EMPTY
        elif u < 0.10:
            raw = cl + 1 + int(rng.integers(0, 9))  # EBOUNDS
        ents.append((b"", int(rng.integers(0, blob_len - 5000)), ln, raw, comp))
    fits = IM.plan_chunks(ents, blob_len, cl)[0]
    total = sum(e[3] for e, st in zip(ents, fits) if not st)
    for stage_cap in (total, total * 2 // 3):  # everything fits; the tail does not
        want_status, want_off, want_dec = IM.plan_chunks(ents, blob_len, cl, stage_cap)
        assert (want_status == fits) == (stage_cap == total) and {0, IM.EMPTY, IM.EBOUNDS} == set(want_status)
        col = lambda k, dt: torch.tensor([e[k] for e in ents], dtype=dt, device="cuda")  # noqa: E731
        t = dict(off=col(1, torch.int64), len=col(2, torch.int32), raw_len=col(3, torch.int32),
                 compressed=col(4, torch.uint8), hash=torch.zeros((n, 32), dtype=torch.uint8, device="cuda"),
                 blob=torch.zeros(16, dtype=torch.uint8, device="cuda"))  # the plan reads no payload byte
        cb = _lib.IngestBatch(hash=t["hash"].data_ptr(), blob=t["blob"].data_ptr(), blob_bytes=blob_len,
                              off=t["off"].data_ptr(), len=t["len"].data_ptr(), raw_len=t["raw_len"].data_ptr(),
                              compressed=t["compressed"].data_ptr(), n=n)
        i32 = lambda k=n: torch.zeros(k, dtype=torch.int32, device="cuda")  # noqa: E731
        i64 = lambda k=n: torch.zeros(k, dtype=torch.int64, device="cuda")  # noqa: E731
        pt = dict(status=i32(), stage_off=i64(), rec_of=i32(), dec_src_off=i64(), dec_src_len=i32(), dec_dst_off=i64(),
                  dec_cap=i32(), dec_len=i32(), dec_entry=i32(), dec_count=i32(1), staged=i64(1))
        cp = _lib.IngestPlan(**{k: v.data_ptr() for k, v in pt.items()})
        _lib.check(_lib.load().sdfs_cdc_ingest_chunks_plan(0, ctypes.byref(cb), cl, stage_cap, ctypes.byref(cp),
                                                           torch.cuda.current_stream().cuda_stream))
        assert pt["status"].tolist() == want_status
        assert pt["stage_off"].tolist() == want_off
        k = pt["dec_count"].item()
        got = list(zip(*(pt[f][:k].tolist() for f in ("dec_src_off", "dec_src_len", "dec_dst_off", "dec_cap", "dec_entry"))))
        assert got == want_dec and k > n // 8
        assert pt["staged"].item() == min(total, stage_cap)
