"""Dedup index, the way back (include/sdfs_index.h): release claims, sweep dead fingerprints,
reuse their slots.

The reference's map is used in both directions: DedupFileStore.removeRef / addRef call
claimKey(hash, val, -ct / +ct) (DedupFileStore.java:130-141,161-172 -> RocksDBMap.claimKey,
RocksDBMap.java:388-509) and RocksDBMap.claimRecords (RocksDBMap.java:630-714) collects what stayed
unreferenced.  The index keeps an entry whose count is <= 0 in the table until a sweep removes it
(the header states the difference from the reference's rmdb side table), so the model below is a
dict of digest -> {pos, ref} with put (the oracle's write_buffers), claim and sweep.

CPU: the model itself, the argument checks of the four new entry points (no GPU needed), and
ShardedDedupIndex.claim_digests / sweep over gloo with the model standing in for the local index.
GPU: the HIP index against the model — a random life cycle, swept-means-absent, probe chains
across tombstones, churn in a small table (space comes back), the sweep cap across scan blocks,
explicit compact, and call order across streams."""
import ctypes
import os
import random
import socket

import numpy as np
import pytest

from oracle import dedup_oracle as D
from sdfs_amd import _lib


class _Model:
    """digest (32 bytes, zero-padded) -> Entry{pos, refcount}; an entry with refcount <= 0 stays,
    findable, until sweep() deletes it."""

    def __init__(self):
        self.m = D.HashesMap()
        self.ever = {}  # every key ever held (insertion-ordered)

    @property
    def entries(self):
        return self.m.entries

    def put(self, digests, bids, pos_base):
        digests = [d.ljust(32, b"\0") for d in digests]
        out = D.write_buffers(self.m, digests, bids, pos_base)
        for d in digests:
            self.ever[d] = True
        return out

    def claim(self, digests, deltas, expects=None):
        out = []
        for i, d in enumerate(digests):
            e = self.m.entries.get(d.ljust(32, b"\0"))
            want = -1 if expects is None else expects[i]
            if e is not None and (want == -1 or want == e.pos):
                e.refcount += deltas[i]
                out.append(e.pos)
            else:
                out.append(-1)
        return out

    def sweep(self):
        dead = [(k, e.pos) for k, e in self.m.entries.items() if e.refcount <= 0]
        for k, _ in dead:
            del self.m.entries[k]
        return dead

    def lookup(self, keys):
        pos = [self.m.entries[k].pos if k in self.m.entries else -1 for k in keys]
        ref = [self.m.entries[k].refcount if k in self.m.entries else 0 for k in keys]
        return pos, ref


def _digest(rng):
    return bytes(rng.getrandbits(8) for _ in range(32))


def _random_batch(rng, nbuf, per_buf, pool, dup_rate):
    """Digests for nbuf buffers (buffer ids ascending); some repeat within/between buffers."""
    digests, bids = [], []
    for b in range(nbuf):
        for _ in range(rng.randint(0, per_buf)):
            if pool and rng.random() < dup_rate:
                d = rng.choice(pool)
            else:
                d = _digest(rng)
                pool.append(d)
            digests.append(d)
            bids.append(b)
    return digests, bids


# ------------------------------------------------------------------------------------------
# CPU: the model
# ------------------------------------------------------------------------------------------
def test_model_file_life_ends_empty():
    rng = random.Random(1)
    m = _Model()
    digests, bids = _random_batch(rng, 10, 12, [], 0.4)
    dup, loc, new = m.put(digests, bids, 500)
    inserted = {digests[i]: 500 + k for k, i in enumerate(new)}
    assert set(inserted) == set(digests)
    # the file is deleted: every HashLocPair releases one claim (removeRef -> claimKey(-1))
    out = m.claim(digests, [-1] * len(digests), loc)
    assert out == loc
    assert all(e.refcount == 0 for e in m.entries.values())
    assert sorted(m.sweep()) == sorted(inserted.items())
    assert m.entries == {} and m.sweep() == []
    assert m.claim(digests[:3], [1, 1, 1]) == [-1, -1, -1]


def test_model_put_before_sweep_recovers_the_old_position():
    m = _Model()
    a, b = b"a" * 32, b"b" * 32
    m.put([a, b], [0, 0], 10)
    assert m.claim([a], [-1]) == [10] and m.entries[a].refcount == 0
    dup, loc, new = m.put([a], [1], 99)  # RocksDBMap.java:663-680 "reclaimed": the data still exists
    assert (dup, loc, new) == ([1], [10], []) and m.entries[a].refcount == 1
    assert m.sweep() == []
    # a wrong archive is not claimed; counts are not clamped
    assert m.claim([b, b], [-5, 2], [12, 11]) == [-1, 11] and m.entries[b].refcount == 3
    assert m.claim([b], [-7]) == [11] and m.entries[b].refcount == -4
    assert m.sweep() == [(b, 11)] and list(m.entries) == [a]


# ------------------------------------------------------------------------------------------
# CPU: argument checks (before any HIP call)
# ------------------------------------------------------------------------------------------
def test_new_entry_points_reject_null_arguments_without_gpu():
    lib = _lib.load()
    u = ctypes.c_uint64()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert lib.sdfs_cdc_index_claim(None, p, None, p, 1, None, None) == _lib.EINVAL
    assert lib.sdfs_cdc_index_sweep(None, p, p, 1, p, None) == _lib.EINVAL
    assert lib.sdfs_cdc_index_compact(None, None) == _lib.EINVAL
    assert lib.sdfs_cdc_index_stats(None, ctypes.byref(u), ctypes.byref(u), ctypes.byref(u)) == _lib.EINVAL
    assert b"null index" in lib.sdfs_cdc_last_error()
    # a handle that is never looked at: the pointer checks come before anything else
    handle = ctypes.addressof(ctypes.create_string_buffer(4096))
    assert lib.sdfs_cdc_index_claim(handle, None, None, p, 1, None, None) == _lib.EINVAL
    assert lib.sdfs_cdc_index_claim(handle, p, None, None, 1, None, None) == _lib.EINVAL
    assert lib.sdfs_cdc_index_sweep(handle, p, p, 1, None, None) == _lib.EINVAL
    assert lib.sdfs_cdc_index_sweep(handle, None, p, 1, p, None) == _lib.EINVAL
    assert lib.sdfs_cdc_index_sweep(handle, p, None, 1, p, None) == _lib.EINVAL


# ------------------------------------------------------------------------------------------
# CPU: the partitioned index over gloo, the model as every rank's shard
# ------------------------------------------------------------------------------------------
class _ModelIndex:
    """The model behind HipHashesMap's tensor interface (claim_digests, sweep)."""

    def __init__(self, model):
        self.model = model

    def claim_digests(self, digests, delta, expect_pos=None, stream=None):
        import torch
        keys = [bytes(r) for r in digests.tolist()]
        out = self.model.claim(keys, delta.tolist(), None if expect_pos is None else expect_pos.tolist())
        return torch.tensor(out, dtype=torch.int64)

    def sweep(self, cap=None, stream=None):
        import torch
        dead = self.model.sweep()
        dg = torch.tensor([list(k) for k, _ in dead], dtype=torch.uint8).reshape(-1, 32)
        return dg, torch.tensor([p for _, p in dead], dtype=torch.int64), 0


_NPOOL = 40


def _shard_pool():
    rng = random.Random(77)
    return [_digest(rng) for _ in range(_NPOOL)]


def _rank_items(rank):
    """This rank's claim items: pool digests (repeats), a few absent ones, deltas in -3..+2,
    expected positions right, wrong or any."""
    pool = _shard_pool()
    rng = random.Random(500 + rank)
    items = []
    for _ in range(30 + 7 * rank):
        j = rng.randrange(_NPOOL)
        d = pool[j] if rng.random() < 0.85 else _digest(rng)
        expect = rng.choice([-1, -1, 1000 + j, 1000 + j, 5000 + j])
        items.append((d, rng.randint(-3, 2), expect))
    return items


def _gc_shard_worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from sdfs_amd.dist import ShardedDedupIndex, shard_of
        pool = _shard_pool()
        pt = torch.tensor([list(d) for d in pool], dtype=torch.uint8)
        own = shard_of(pt, world).tolist()
        model = _Model()
        for j, d in enumerate(pool):
            if own[j] == rank:
                model.entries[d] = D.Entry(1000 + j, 2)
        idx = ShardedDedupIndex(_ModelIndex(model), hash_len=32)
        items = _rank_items(rank)
        dg = torch.tensor([list(d) for d, _, _ in items], dtype=torch.uint8)
        delta = torch.tensor([x for _, x, _ in items], dtype=torch.int64)
        expect = torch.tensor([e for _, _, e in items], dtype=torch.int64)
        pos = idx.claim_digests(dg, delta, expect)
        pos_any = idx.claim_digests(dg[:5], 0)  # an int delta, no expected position
        sd, sp, left = idx.sweep()
        swept = [(bytes(r), p) for r, p in zip(sd.tolist(), sp.tolist())]
        rest = {k: (e.pos, e.refcount) for k, e in model.entries.items()}
        q.put((rank, pos.tolist(), pos_any.tolist(), swept, left, rest, own))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_claim_and_sweep_gloo(world):
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gc_shard_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {r: rest for r, *rest in (q.get(timeout=120) for _ in range(world))}
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    # one unsharded model fed the ranks' items in (rank, item) order
    pool = _shard_pool()
    ref = _Model()
    for j, d in enumerate(pool):
        ref.entries[d] = D.Entry(1000 + j, 2)
    own = res[0][5]
    for r in range(world):
        items = _rank_items(r)
        want = ref.claim([d for d, _, _ in items], [x for _, x, _ in items], [e for _, _, e in items])
        assert res[r][0] == want, r
        assert any(p == -1 for p in want) and any(p != -1 for p in want)
    for r in range(world):  # the second call everywhere came after the first one everywhere
        items = _rank_items(r)[:5]
        assert res[r][1] == ref.claim([d for d, _, _ in items], [0] * 5), r
    dead = ref.sweep()
    assert dead  # the case means something
    got = [x for r in range(world) for x in res[r][2]]
    assert sorted(got) == sorted(dead)
    rest = {}
    for r in range(world):
        assert all(own[pool.index(k)] == r for k, _ in res[r][2])  # every rank swept its own shard
        assert res[r][3] == 0
        rest.update(res[r][4])
    assert rest == {k: (e.pos, e.refcount) for k, e in ref.entries.items()}


# ------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------
def _records(digests, bids):
    n = len(digests)
    rec = np.zeros((n, 48), dtype=np.uint8)
    for i, (d, b) in enumerate(zip(digests, bids)):
        rec[i, :32] = np.frombuffer(d.ljust(32, b"\0"), dtype=np.uint8)
        rec[i, 32:40] = np.frombuffer(int(b).to_bytes(8, "little"), dtype=np.uint8)
        rec[i, 40:48] = np.frombuffer((i * 4096).to_bytes(4, "little") + (4096).to_bytes(4, "little"),
                                      dtype=np.uint8)
    return rec


def _put(ix, torch, digests, bids, pos_base):
    rec = torch.from_numpy(_records(digests, bids)).cuda()
    dup, loc, new, nc = ix.put_records(rec, None, pos_base)
    torch.cuda.synchronize()
    k = int(nc.item())
    return dup.cpu().tolist(), loc.cpu().tolist(), new.cpu().tolist()[:k]


def _claim(ix, torch, digests, deltas, expects=None):
    dg = ix._digest_tensor(digests)
    delta = torch.tensor(deltas, dtype=torch.int64, device="cuda")
    expect = None if expects is None else torch.tensor(expects, dtype=torch.int64, device="cuda")
    return ix.claim_digests(dg, delta, expect).cpu().tolist()


def _sweep(ix, cap=None):
    dg, pos, left = ix.sweep(cap)
    d = dg.cpu().numpy()
    return [(d[i].tobytes(), p) for i, p in enumerate(pos.cpu().tolist())], left


def _lookup(ix, keys):
    pos, ref = ix.get_digests(ix._digest_tensor(keys))
    return pos.cpu().tolist(), ref.cpu().tolist()


@pytest.mark.gpu
def test_gc_random_life_cycle_vs_model():
    torch = pytest.importorskip("torch")
    from sdfs_amd.index import HipHashesMap
    rng = random.Random(31)
    ix = HipHashesMap(4096)
    m = _Model()
    pool = []
    base = 1 << 40

    def check(step):
        keys = list(m.ever)
        assert ix.getSize() == len(m.entries), step
        assert _lookup(ix, keys) == m.lookup(keys), step

    for rnd in range(8):
        digests, bids = _random_batch(rng, 30, 40, pool, 0.35)
        if rnd == 3:  # HASH160-sized fingerprints, zero-padded in the records
            digests = [d[:20] for d in digests]
        got = _put(ix, torch, digests, bids, base)
        dup, loc, new = m.put(digests, bids, base)
        assert got == (dup, loc, new), rnd
        base += len(new)
        check((rnd, "put"))

        keys = list(m.ever)
        cd, cdelta, cexp = [], [], []
        for _ in range(900):
            if rng.random() < 0.1:
                d = _digest(rng)  # never held
            else:
                d = rng.choice(keys)  # held, or swept in an earlier round; repeats happen
                if rnd == 3 and rng.random() < 0.5:
                    d = d.rstrip(b"\0")  # the caller's short form of a padded key
            e = m.entries.get(d.ljust(32, b"\0"))
            u = rng.random()
            cexp.append(-1 if u < 0.6 or e is None else e.pos if u < 0.85 else e.pos ^ 0x5555)
            cd.append(d)
            cdelta.append(rng.randint(-3, 2))
        if rnd % 2:
            cexp = None  # no expected positions at all
        assert _claim(ix, torch, cd, cdelta, cexp) == m.claim(cd, cdelta, cexp), rnd
        check((rnd, "claim"))
        assert any(e.refcount < 0 for e in m.entries.values())  # negative counts are compared too

        removed, left = _sweep(ix)
        want = m.sweep()
        assert want, rnd
        assert sorted(removed) == sorted(want) and left == 0, rnd
        check((rnd, "sweep"))
    ix.destroy()


@pytest.mark.gpu
def test_gc_swept_fingerprint_is_absent_and_inserts_fresh():
    torch = pytest.importorskip("torch")
    from sdfs_amd.index import HipHashesMap
    ix = HipHashesMap(1024)
    a, b, c = b"A" * 32, b"B" * 32, b"C" * 20
    assert _put(ix, torch, [a, b, c, c], [0, 0, 0, 0], 100) == ([0, 0, 0, 1], [100, 101, 102, 102], [0, 1, 2])
    assert ix.claimKey(a, 100, -1) == 100 and ix.refcount(a) == 0
    assert ix.get(a) == 100 and ix.getSize() == 3  # kept until swept
    assert ix.claimRecords() == [(a, 100)]
    assert ix.get(a) == -1 and ix.refcount(a) == 0 and ix.getSize() == 2
    assert ix.claimKey(a, -1, 1) == -1  # a claim does not bring it back
    st = ix.stats()
    assert (st.live, st.tombstones, st.capacity) == (2, 1, ix.getMaxSize())
    assert _put(ix, torch, [a], [1], 900) == ([0], [900], [0])  # fresh: not a hit on the stale key
    assert _lookup(ix, [a, b, c]) == ([900, 101, 102], [1, 1, 2])
    assert ix.getSize() == 3
    ix.clear()
    torch.cuda.synchronize()
    st = ix.stats()
    assert (st.live, st.tombstones) == (0, 0)
    ix.destroy()


def _mix64(z):
    """The table's hash of a digest's first 8 bytes (dedup_index.hip mix64), restated."""
    mask = (1 << 64) - 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
    return z ^ (z >> 31)


@pytest.mark.gpu
def test_gc_probe_chain_across_tombstones():
    """48 digests with the same first 8 bytes form one probe chain in a 128-slot table (started
    near the table's end, so it wraps).  With every third one swept, the others are still found
    by get, hit by put_records and reached by claim; no lookup matches a tombstone's stale key."""
    torch = pytest.importorskip("torch")
    from sdfs_amd.index import HipHashesMap
    ix = HipHashesMap(100)  # 128 slots
    prefix = next(p for p in range(1, 1 << 16) if _mix64(p) & 127 >= 120)
    rng = random.Random(13)
    chain = [prefix.to_bytes(8, "little") + bytes(rng.getrandbits(8) for _ in range(24)) for _ in range(48)]
    dup, loc, new = _put(ix, torch, chain, [0] * 48, 7000)
    assert dup == [0] * 48 and loc == list(range(7000, 7048))
    gone = chain[::3]
    kept = [d for i, d in enumerate(chain) if i % 3]
    kept_pos = [7000 + i for i in range(48) if i % 3]
    assert _claim(ix, torch, gone, [-1] * 16) == [7000 + i for i in range(0, 48, 3)]
    removed, left = _sweep(ix)
    assert sorted(removed) == sorted(zip(gone, range(7000, 7048, 3))) and left == 0
    zero = b"\0" * 32
    assert _lookup(ix, kept + gone + [zero]) == (kept_pos + [-1] * 17, [1] * 32 + [0] * 17)
    assert _claim(ix, torch, kept + gone + [zero], [2] * 49) == kept_pos + [-1] * 17
    dup, loc, new = _put(ix, torch, kept + gone[:4], [1] * 36, 8000)
    assert dup == [1] * 32 + [0] * 4 and loc == kept_pos + [8000, 8001, 8002, 8003] and new == [32, 33, 34, 35]
    assert _lookup(ix, kept + gone[:4] + gone[4:] + [zero]) == (kept_pos + [8000, 8001, 8002, 8003] + [-1] * 13,
                                                                [4] * 32 + [1] * 4 + [0] * 13)
    assert ix.getSize() == 36
    ix.destroy()


@pytest.mark.gpu
def test_gc_churn_in_a_small_table_gets_space_back():
    torch = pytest.importorskip("torch")
    from sdfs_amd.index import HipHashesMap
    ix = HipHashesMap(100)  # 128 slots, 112 usable
    cap = ix.getMaxSize()
    assert cap == 112
    rng = random.Random(19)
    m = _Model()
    live = [_digest(rng) for _ in range(60)]
    base = 0
    assert _put(ix, torch, live, [0] * 60, base) == m.put(live, [0] * 60, base)
    base += 60
    tombstones, rebuilds = 0, 0
    for rnd in range(20):  # 60 + 20 * 40 = 860 insertions into 128 slots
        fresh = [_digest(rng) for _ in range(40)]
        assert _put(ix, torch, fresh, [rnd + 1] * 40, base) == m.put(fresh, [rnd + 1] * 40, base), rnd
        base += 40
        st = ix.stats()
        assert st.live == 100 and st.live + st.tombstones <= cap, rnd
        assert st.tombstones in (0, tombstones), rnd  # a put removes all of them or none
        rebuilds += tombstones > 0 and st.tombstones == 0
        tombstones = st.tombstones + 40  # after the sweep below
        old, live = live[:40], live[40:] + fresh
        assert _claim(ix, torch, old, [-1] * 40) == m.claim(old, [-1] * 40), rnd
        removed, left = _sweep(ix)
        assert sorted(removed) == sorted(m.sweep()) and len(removed) == 40 and left == 0, rnd
        # the survivors keep their positions and counts through every rebuild
        assert _lookup(ix, live + old) == m.lookup(live + old), rnd
        assert ix.getSize() == 60 and ix.stats().tombstones == tombstones, rnd
    assert rebuilds >= 1  # the tombstone count fell back to 0: put_records rebuilt the table
    with pytest.raises(_lib.SdfsCdcError) as ei:  # 60 held + 53 > 112: no rebuild can help
        _put(ix, torch, [_digest(rng) for _ in range(53)], [99] * 53, base)
    assert ei.value.code == _lib.ECAP
    assert _lookup(ix, live) == m.lookup(live)
    ix.destroy()


@pytest.mark.gpu
def test_gc_sweep_cap_and_block_edges():
    torch = pytest.importorskip("torch")
    from sdfs_amd.index import HipHashesMap
    ix = HipHashesMap(8192)  # 16384 slots: sixteen 1024-slot scan blocks
    nrng = np.random.default_rng(5)
    keys = [bytes(r) for r in nrng.integers(0, 256, (4000, 32), dtype=np.uint8)]
    dup, loc, new = _put(ix, torch, keys, [0] * 4000, 0)
    assert loc == list(range(4000))
    assert _sweep(ix) == ([], 0)  # nothing dead
    dead = {k: i for i, k in enumerate(keys) if i % 4}
    assert len(dead) == 3000
    _claim(ix, torch, list(dead), [-1] * 3000)
    seen = []
    for cap, want_removed, want_left in ((0, 0, 3000), (1, 1, 2999), (1024, 1024, 1975), (None, 1975, 0)):
        removed, left = _sweep(ix, cap)
        assert (len(removed), left) == (want_removed, want_left), cap
        seen += removed
        assert ix.getSize() == 4000 - len(seen)
    assert len(set(seen)) == 3000 and dict(seen) == dead
    assert _sweep(ix) == ([], 0)
    st = ix.stats()
    assert (st.live, st.tombstones) == (1000, 3000)
    alive = keys[::4]
    assert _lookup(ix, alive) == (list(range(0, 4000, 4)), [1] * 1000)
    ix.destroy()


@pytest.mark.gpu
def test_gc_explicit_compact_keeps_live_entries():
    torch = pytest.importorskip("torch")
    from sdfs_amd.index import HipHashesMap
    ix = HipHashesMap(1000)
    rng = random.Random(23)
    keys = [_digest(rng) for _ in range(300)]
    _put(ix, torch, keys, [0] * 300, 50)
    _put(ix, torch, keys[100:200], [1] * 100, 999)  # counts of 2
    _claim(ix, torch, keys[:100] + keys[200:250], [-1] * 100 + [-3] * 50)
    removed, _ = _sweep(ix, 100)  # 100 tombstones, 50 dead entries left in the table
    assert len(removed) == 100
    before = _lookup(ix, keys)
    st = ix.stats()
    assert (st.live, st.tombstones) == (200, 100)
    ix.compact()
    st = ix.stats()
    assert (st.live, st.tombstones) == (200, 0)
    assert _lookup(ix, keys) == before
    gone = {k for k, _ in removed}
    want_pos = [-1 if k in gone else 50 + i for i, k in enumerate(keys)]
    assert before[0] == want_pos
    assert [r for k, r in zip(keys, before[1]) if k not in gone].count(-2) == 50 - len(gone & set(keys[200:250]))
    dup, loc, _ = _put(ix, torch, keys[100:200], [2] * 100, 5000)  # still hits after the rebuild
    assert dup == [1] * 100 and loc == list(range(150, 250))
    ix.destroy()


@pytest.mark.gpu
def test_gc_calls_on_two_streams_apply_in_call_order():
    """put on stream A, claim on B, sweep on A, get on B, with no host synchronisation in
    between: every call sees what the calls before it did."""
    torch = pytest.importorskip("torch")
    from sdfs_amd.index import HipHashesMap
    n = 50000
    ix = HipHashesMap(1 << 17)
    nrng = np.random.default_rng(29)
    rec_np = np.zeros((n, 48), dtype=np.uint8)
    rec_np[:, :32] = nrng.integers(0, 256, (n, 32), dtype=np.uint8)
    rec_np[:, 32:36] = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)  # one buffer each
    rec = torch.from_numpy(rec_np).cuda()
    dg = rec[:, :32].contiguous()
    half = dg[: n // 2].contiguous()
    minus = torch.full((n // 2,), -1, dtype=torch.int64, device="cuda")
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(sa):
        dup, loc, _, nc = ix.put_records(rec, None, 0, stream=sa.cuda_stream)
    with torch.cuda.stream(sb):
        cpos = ix.claim_digests(half, minus, stream=sb.cuda_stream)
    with torch.cuda.stream(sa):
        sd, sp, counts = ix.sweep_device(n, stream=sa.cuda_stream)
    with torch.cuda.stream(sb):
        pos, ref = ix.get_digests(dg, stream=sb.cuda_stream)
    torch.cuda.synchronize()
    assert int(nc.item()) == n and not dup.any() and loc.cpu().tolist() == list(range(n))
    assert cpos.cpu().tolist() == list(range(n // 2))
    assert counts.cpu().tolist() == [n // 2, 0]
    order = torch.argsort(sp[: n // 2])
    assert sp[: n // 2][order].cpu().tolist() == list(range(n // 2))
    assert torch.equal(sd[: n // 2][order], half)
    assert pos.cpu().tolist() == [-1] * (n // 2) + list(range(n // 2, n))
    assert ref.cpu().tolist() == [0] * (n // 2) + [1] * (n // 2)
    ix.destroy()
