"""Client-side dedup (include/sdfs_ingest.h, sdfs_cdc_index_addref_slots, sdfs_amd/ingest.py): the
server half of checkHashes, writeChunks and writeSparseDataChunk (StorageServiceImpl.java:175-382).

The model (tests/ingest_model.py) restates the three RPCs over tests/mapfile_model.IndexModel.
CPU: the model against hand-worked cases; the argument checks of the new entry points (no device);
the wrapper's destination checks.  GPU: every result of the HIP calls equals the model's, bit for
bit, and the client route leaves the store that HipBufferWriter.write leaves."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

from oracle import meta_oracle as MO
from sdfs_amd import _lib
from tests import ingest_model as IM
from tests import lz4_block_model as Z
from tests import mapfile_model as MM
from tests import read_model as R

PB = 1 << 33
WALK_PART = 256  # kSlotPart of store_format.h: pairs of one slot a wave of the walks takes


def H(i, hl=32):
    return (b"h%07d" % i).ljust(hl, b"\x5a")


def _sha(b):
    return hashlib.sha256(bytes(b)).digest()


def _rnd(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _pairs(items, step=100):
    """(digest, hashloc) -> image pairs with ascending pos."""
    return [(d, loc, step, i * step, 0, step) for i, (d, loc) in enumerate(items)]


# ------------------------------------------------------------------------------------------
# CPU: the model against hand-worked cases
# ------------------------------------------------------------------------------------------
def test_model_check_hashes_and_write_chunks_hand_worked():
    ix = MM.IndexModel()
    ix.load([(H(1), 77, 3), (H(2), 78, 0)])
    m = IM.IngestModel(ix, 100, digest=_sha)
    assert m.check_hashes([H(1), H(2), H(3)]) == [77, 78, -1]  # count 0, not swept: still reported
    a, b = b"A" * 40, b"B" * 30
    lit = Z.emit([], b)  # a block of literals alone
    blob = a + lit + a + b"tail"
    ents = [(H(10), 0, 40, 40, 0),                      # raw, new
            (H(11), 40, len(lit), 30, 1),               # LZ4, new
            (H(12), 0, 0, 0, 0),                        # empty
            (H(10), 40 + len(lit), 40, 40, 0),          # the same hash again
            (H(1), 0, 40, 40, 0),                       # held before the call
            (H(13), 40, len(lit), 31, 1),               # decodes to 30, not 31
            (H(14), 40, len(lit) - 1, 30, 1),           # truncated
            (H(15), 0, 40, 101, 1),                     # raw_len > chunk_length
            (H(16), len(blob) - 2, 3, 3, 0),            # past the blob
            (H(17), 0, 40, 39, 0),                      # raw, len != raw_len
            (H(18), 0, 40, 0, 0)]                       # raw_len 0
    ins, pos, stored, status = m.write_chunks(ents, blob, PB)
    E = IM
    assert status == [0, 0, E.EMPTY, 0, 0, E.EDECODE, E.EDECODE, E.EBOUNDS, E.EBOUNDS, E.EBOUNDS, E.EBOUNDS]
    assert ins == [1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert pos == [PB, PB + 1, -1, PB, 77] + [-1] * 6
    assert stored == [44, 34, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert m.chunks == {PB: a, PB + 1: b}
    assert ix.export() == sorted([(MM.pad32(H(1)), 77, 4), (MM.pad32(H(2)), 78, 0), (MM.pad32(H(10)), PB, 2),
                                  (MM.pad32(H(11)), PB + 1, 1)])
    # verify: the hash is the chunk's, or the entry is refused; without it the client's hash is trusted
    ents = [(_sha(a), 0, 40, 40, 0), (H(20), 0, 40, 40, 0)]
    assert m.write_chunks(ents, blob, PB + 2, verify=True) == ([1, 0], [PB + 2, -1], [44, 0], [0, E.EHASH])
    assert m.write_chunks(ents, blob, PB + 3)[3] == [0, 0] and MM.pad32(H(20)) in ix.e
    # a staging area that is too small: the places are the prefix over every entry that got this far
    ents = [(H(30), 0, 40, 40, 0), (H(31), 0, 40, 40, 0), (H(32), 0, 4, 4, 0)]
    assert m.write_chunks(ents, blob, PB + 9, stage_cap=50)[3] == [0, E.EBOUNDS, E.EBOUNDS]


def test_model_addref_slots_hand_worked():
    ix = MM.IndexModel()
    a, b, c = H(1), H(2), H(3)
    ix.load([(a, 10, 1), (b, 11, 1), (c, 5, 1)])
    m = IM.IngestModel(ix, 1000)
    sb = 13 + 5 * 56
    imgs = [R.build_image(_pairs([(a, 10), (b, 11), (c, 5)])),                       # all held
            R.build_image(_pairs([(a, 10), (b, 99), (c, 5)])),                       # one wrong hashloc
            R.build_image(_pairs([(a, 10), (H(9), 3)])),                             # an unknown digest
            b"",                                                                     # an empty slot
            R.build_image(_pairs([(a, 10)] * 6)),                                    # does not fit
            R.build_image([(a, 10, 5, 0, 0, 5), (b, 11, 5, 9, 0, -1)]),              # a negative field
            R.build_image([(H(9), 3, 5, 0, 0, 5), (c, 5, 5, 0, 0, 5), (b, 11, 5, 9, 0, 5)]),  # repeated pos: c wins
            R.build_image(_pairs([(a, 10), (H(8), 1)])),                             # unknown, but inserted
            R.build_image(_pairs([(a, 10), (b, 11)]))]                               # all inserted
    flags = [None] * 7 + [[0, 1], [1, 1]]
    counts, status, missed, misses = m.addref_slots(imgs, sb, 32, flags)
    assert status == [0, IM.EMISSED, IM.EMISSED, 0, IM.CORRUPT, IM.CORRUPT, 0, 0, 0]
    assert missed == [0, 1, 1, 0, 0, 0, 0, 0, 0] and misses == [(1, 1), (2, 1)]
    assert counts == [3 + 2 + 1, 2, 3, 5, 4, 2]
    # a: requests 0 and 7; b: 0 and 6; c: 0 and 6 — the rejected requests' matching pairs added nothing
    assert ix.export() == sorted([(MM.pad32(a), 10, 3), (MM.pad32(b), 11, 3), (MM.pad32(c), 5, 3)])
    # replacing a slot: the old slot's pairs are released, the file grows
    slots = [imgs[0], b""]
    res, flen = m.write_sparse_data_chunks(slots, sb, 32, [0, 1], [imgs[8], imgs[1]], [700, 1000], 5, [[0, 0], None])
    assert res[1] == [0, IM.EMISSED] and flen == 700 and slots == [imgs[8].ljust(sb, b"\0"), b""]
    assert ix.export() == sorted([(MM.pad32(a), 10, 3), (MM.pad32(b), 11, 3), (MM.pad32(c), 5, 2)])


# ------------------------------------------------------------------------------------------
# CPU: argument checks (before any HIP call), the wrapper's destination checks
# ------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_before_the_device():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    h = ctypes.addressof(ctypes.create_string_buffer(4096))  # a handle that is never looked at
    E = _lib.EINVAL

    def addref(ix=h, m=p, n=1, sb=293, hl=32, ins=None, stride=5, st=p, ms=p, lst=None, cap=0, ct=p):
        return lib.sdfs_cdc_index_addref_slots(ix, m, n, sb, hl, ins, stride, st, ms, lst, cap, ct, None)

    assert addref(ix=None) == E and b"null index" in lib.sdfs_cdc_last_error()
    assert addref(hl=20) == E and b"hash_len 20" in lib.sdfs_cdc_last_error()
    assert addref(sb=12) == E and b"slot_bytes" in lib.sdfs_cdc_last_error()
    assert addref(st=None) == E and addref(ct=None) == E and addref(m=None) == E
    assert addref(ms=None) == E and b"req_missed" in lib.sdfs_cdc_last_error()
    assert addref(cap=1) == E and b"miss list" in lib.sdfs_cdc_last_error()
    assert addref(ins=p, stride=4) == E and b"pair_stride" in lib.sdfs_cdc_last_error()
    assert addref(n=1 << 31) == E

    def batch(**kw):
        f = dict(hash=p, blob=p, blob_bytes=16, off=p, len=p, raw_len=p, compressed=p, n=1)
        f.update(kw)
        return _lib.IngestBatch(**f)

    def plan(**kw):
        f = {k: p for k, _ in _lib.IngestPlan._fields_}
        f.update(kw)
        return _lib.IngestPlan(**f)

    B, P = ctypes.byref(batch()), ctypes.byref(plan())
    calls = {
        "plan": lambda b=B, q=P, cl=4096: lib.sdfs_cdc_ingest_chunks_plan(0, b, cl, 64, q, None),
        "decode": lambda b=B, q=P, z=h, st=p: lib.sdfs_cdc_ingest_chunks_decode(z, b, q, st, None),
        "copy": lambda b=B, q=P, cl=4096, st=p: lib.sdfs_cdc_ingest_chunks_copy(0, b, q, cl, st, None),
        "verify": lambda b=B, q=P, e=h, st=p, hl=32: lib.sdfs_cdc_ingest_chunks_verify(e, b, q, st, hl, None),
        "records": lambda b=B, q=P, r=p, c=p: lib.sdfs_cdc_ingest_chunks_records(0, b, q, r, c, None),
        "results": lambda b=B, q=P, d=p, loc=p, o=p: lib.sdfs_cdc_ingest_chunks_results(
            0, b, q, d, loc, 0, None, 0, o, o, o, o, None),
    }
    for name, f in calls.items():
        assert f(b=None) == E and b"null batch" in lib.sdfs_cdc_last_error(), name
        assert f(q=None) == E and b"null plan" in lib.sdfs_cdc_last_error(), name
        assert f(b=ctypes.byref(batch(n=1 << 31))) == E and b"split the batch" in lib.sdfs_cdc_last_error(), name
        for k in ("hash", "off", "len", "raw_len", "compressed"):
            assert f(b=ctypes.byref(batch(**{k: None}))) == E and b"null entry array" in lib.sdfs_cdc_last_error()
        assert f(b=ctypes.byref(batch(blob=None))) == E and b"null blob" in lib.sdfs_cdc_last_error(), name
        for k, _ in _lib.IngestPlan._fields_:
            assert f(q=ctypes.byref(plan(**{k: None}))) == E, (name, k)
    assert calls["plan"](cl=0) == E and calls["plan"](cl=1 << 31) == E and calls["copy"](cl=0) == E
    assert b"chunk_length" in lib.sdfs_cdc_last_error()
    assert calls["decode"](z=None) == E and b"null decoder" in lib.sdfs_cdc_last_error()
    assert calls["decode"](st=None) == E and calls["copy"](st=None) == E
    assert b"staging" in lib.sdfs_cdc_last_error()
    assert calls["verify"](e=None) == E and b"null engine" in lib.sdfs_cdc_last_error()
    assert calls["verify"](hl=24) == E and b"hash_len 24" in lib.sdfs_cdc_last_error()
    assert calls["records"](r=None) == E and calls["records"](c=None) == E
    assert calls["records"](r=p + 1) == E and b"16-byte aligned" in lib.sdfs_cdc_last_error()
    assert calls["results"](d=None) == E and calls["results"](loc=None) == E and calls["results"](o=None) == E


def test_destination_checks():
    from sdfs_amd.ingest import check_destinations

    assert check_destinations([3, 0, 2], 4) == [3, 0, 2] and check_destinations([], 0) == []
    for bad in ([-1], [4], [0, 1, 0]):
        with pytest.raises(ValueError):
            check_destinations(bad, 4)


# ------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------
def _dev(a, dt=None):
    import torch

    t = torch.from_numpy(np.array(a, copy=True, order="C")).cuda()
    return t if dt is None else t.to(dt)


def _export(ix):
    dg, pos, ref, held = ix.export()
    d = dg.cpu().numpy()
    out = sorted((d[i].tobytes(), p, r) for i, (p, r) in enumerate(zip(pos.tolist(), ref.tolist())))
    assert held == len(out)
    return out


def _load(ix, model_ix, items):
    import torch

    want = model_ix.load(items)
    dg = _dev(np.frombuffer(b"".join(MM.pad32(d) for d, _, _ in items), np.uint8).reshape(-1, 32))
    got = ix.load(dg, torch.tensor([p for _, p, _ in items], dtype=torch.int64),
                  torch.tensor([r for _, _, r in items], dtype=torch.int64)).cpu().tolist()
    assert got == want


def _chunk_batch(ents, blob):
    """[(hash, off, len, raw_len, compressed)] over blob, exactly as given (the numbers may lie)."""
    import torch

    from sdfs_amd.ingest import ChunkBatch

    n = len(ents)
    hs = np.frombuffer(b"".join(MM.pad32(e[0]) for e in ents) or bytes(32), np.uint8).reshape(-1, 32)[:n]
    col = lambda k, dt: _dev(np.array([e[k] for e in ents], np.int64), dt)  # noqa: E731
    return ChunkBatch(_dev(hs), _dev(np.frombuffer(bytes(blob) or b"\0", np.uint8))[: len(blob)], col(1, torch.int64),
                      col(2, torch.int32), col(3, torch.int32), col(4, torch.uint8), sum(e[3] for e in ents))


def _ingest(cl, hl=32, cap=4096, engine=None, **kw):
    from sdfs_amd.archive import HipBufferWriter
    from sdfs_amd.index import HipHashesMap
    from sdfs_amd.ingest import HipChunkIngest

    ix = HipHashesMap(cap)
    wr = HipBufferWriter(ix, hash_len=hl, **kw)
    return ix, wr, HipChunkIngest(wr, cl, engine=engine)


def _write_and_check(ing, model, ents, blob, pos_base, verify=False):
    """write_chunks on both; results, statuses and the index equal; -> (model results, arcs)."""
    import torch

    ins, pos, stored, status, arcs = ing.write_chunks(_chunk_batch(ents, blob), pos_base, verify=verify)
    want = model.write_chunks(ents, blob, pos_base, verify=verify)
    torch.cuda.synchronize()
    assert status.tolist() == want[3]
    assert ins.tolist() == want[0] and pos.tolist() == want[1] and stored.tolist() == want[2]
    assert _export(ing.index) == model.ix.export()
    assert arcs.n_rec == sum(want[0])
    return want, arcs


def _read_back(ing, arcs, model, ents, res, pos_base, max_chunk):
    """Every chunk the call stored, through open_store + lookup + the record's decode."""
    import torch

    from sdfs_amd.store import _map_lens, lookup, open_store

    sent = [(e[0], res[1][i]) for i, e in enumerate(ents) if res[0][i]]
    if not sent:
        return 0
    op = open_store(arcs.store.clone(), arcs.arc_base.clone(), arcs.arc_bytes.clone(), arcs.maps.clone(),
                    _map_lens(arcs), ing.index, pos_base, arcs.n_rec, hash_len=ing.hash_len, version=arcs.version,
                    aes=ing.writer.aes, max_chunk=max_chunk)
    torch.cuda.synchronize()
    assert op.n_rec == len(sent) and op.extra["open"]["info"].tolist() == [0, 0, 0]
    assert not op.extra["open"]["flags"].any()
    k = torch.tensor([p - pos_base for _, p in sent], dtype=torch.int64, device="cuda")
    arc = op.layout.arc[op.rec_of_k[k]]
    keys = _dev(np.frombuffer(b"".join(MM.pad32(h) for h, _ in sent), np.uint8).reshape(-1, 32))
    lk = lookup(op, arc, keys)
    torch.cuda.synchronize()
    assert (lk.slot >= 0).all() and not lk.flags.any()
    assert lk.store_off.tolist() == op.store_off[k].tolist() and lk.len.tolist() == op.store_len[k].tolist()
    store = op.store.cpu().numpy()
    for (h, p), off, ln in zip(sent, lk.store_off.tolist(), lk.len.tolist()):
        r = Z.decode_record(store[off: off + ln].tobytes(), max_chunk)
        assert not isinstance(r, str) and r[0] == model.chunks[p], h
    return len(sent)


@pytest.mark.gpu
def test_gpu_check_hashes():
    pytest.importorskip("torch")
    ix, wr, ing = _ingest(4096, compress=False)
    model = IM.IngestModel(MM.IndexModel(), 4096)
    _load(ix, model.ix, [(H(1), 77, 3), (H(2), 78, 0), (H(3), 0, 1)])  # H(2): count 0, not swept
    asked = [H(1), H(9), H(2), H(3), H(1)]
    assert ing.check_hashes(asked).tolist() == model.check_hashes(asked) == [77, -1, 78, 0, 77]
    assert ing.check_hashes([]).tolist() == []
    ix.claimKey(H(1), 77, -3)
    assert ing.check_hashes([H(1)]).tolist() == [77]  # unreferenced, found until a sweep
    ix.sweep()
    assert ing.check_hashes([H(1), H(2), H(3)]).tolist() == [-1, -1, 0]
    wr.destroy()
    ix.destroy()


@pytest.mark.gpu
def test_gpu_write_chunks_one_batch_with_every_case():
    pytest.importorskip("torch")
    from oracle import lz4_oracle as ZO

    cl = 8192
    ix, wr, ing = _ingest(cl, compress=False)
    model = IM.IngestModel(MM.IndexModel(), cl)
    _load(ix, model.ix, [(H(1), 77, 3)])
    a, c = _rnd(1, 3001), _rnd(2, 517)
    b = (_rnd(3, 40) * 200)[:5000]
    blk, small = ZO.compress(b), ZO.compress(b[:333])
    assert len(blk) < 1000 and not isinstance(Z.decode(blk, 5000), str)
    big = _rnd(4, cl + 1)
    parts, at = {}, 0
    for name, x in (("a", a), ("blk", blk), ("a2", a), ("c", c), ("small", small), ("big", big)):
        at += 3  # odd source offsets
        parts[name] = at
        at += len(x)
    blob = bytearray(at + 5)
    for name, x in (("a", a), ("blk", blk), ("a2", a), ("c", c), ("small", small), ("big", big)):
        blob[parts[name]: parts[name] + len(x)] = x
    blob = bytes(blob)
    ents = [(_sha(a), parts["a"], len(a), len(a), 0),                # raw, new
            (_sha(b), parts["blk"], len(blk), 5000, 1),              # LZ4, new
            (H(12), 0, 0, 0, 0),                                     # empty
            (H(13), parts["blk"], len(blk), 4999, 1),                # a wrong raw_len: too short
            (H(14), parts["blk"], len(blk), 5001, 1),                # ... too long
            (_sha(a), parts["a2"], len(a), len(a), 0),               # the same hash again: count 2
            (H(1), parts["c"], len(c), len(c), 0),                   # held before the call
            (H(15), parts["blk"], len(blk) - 7, 5000, 1),            # a truncated block
            (H(16), parts["big"], cl + 1, cl + 1, 0),                # raw_len > chunk_length
            (H(17), parts["blk"], len(blk), cl + 1, 1),              # ... on a compressed entry
            (H(18), len(blob) - 10, 100, 100, 0),                    # off + len past the blob
            (H(19), 1 << 40, 5, 5, 0),                               # off past the blob
            (H(20), parts["c"], len(c), len(c) - 1, 0),              # raw, len != raw_len
            (H(21), parts["c"], len(c), 0, 0),                       # raw_len 0
            (_sha(c), parts["c"], len(c), len(c), 0),                # raw, new, behind the rejected ones
            (_sha(b[:333]), parts["small"], len(small), 333, 1)]     # LZ4, new
    res, arcs = _write_and_check(ing, model, ents, blob, PB)
    E = IM
    assert res[3] == [0, 0, E.EMPTY, E.EDECODE, E.EDECODE, 0, 0, E.EDECODE, E.EBOUNDS, E.EBOUNDS, E.EBOUNDS, E.EBOUNDS,
                      E.EBOUNDS, E.EBOUNDS, 0, 0]
    assert res[0] == [1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1] and res[1][5] == PB and res[1][6] == 77
    assert model.ix.e[MM.pad32(_sha(a))] == [PB, 2] and model.ix.e[MM.pad32(H(1))] == [77, 4]
    assert model.chunks == {PB: a, PB + 1: b, PB + 2: c, PB + 3: b[:333]}
    assert _read_back(ing, arcs, model, ents, res, PB, cl) == 4
    # the same batch again: nothing is new, every accepted entry adds a reference
    res, arcs = _write_and_check(ing, model, ents, blob, PB + 100)
    assert sum(res[0]) == 0 and arcs.n_arc == 0 and model.ix.e[MM.pad32(_sha(a))] == [PB, 4]
    wr.destroy()
    ix.destroy()


@pytest.mark.gpu
def test_gpu_copy_and_staging_edges():
    """Raw chunks of 1 .. 65 537 bytes from every source offset mod 16 (their places in the staging
    area take every alignment too); batches of 0, 1 and one more than a scan tile of entries, with
    rejected and compressed entries on both sides of the tile's edge."""
    torch = pytest.importorskip("torch")
    cl = 131072
    ix, wr, ing = _ingest(cl, cap=8192, compress=False)
    model = IM.IngestModel(MM.IndexModel(), cl)
    assert _lib.INGEST_COPY_SPAN < 65537 <= cl
    lens = [1, 15, 16, 17, 31, 4095, 65537]
    src = _rnd(7, 65537 + 64)
    blob, ents, k = bytearray(), [], 0
    for ln in lens:
        for sh in range(16):
            blob += bytes(-len(blob) % 16 + sh)
            chunk = bytes([k & 255, k >> 8]) + src[2: ln] if ln > 1 else bytes([k])
            chunk = chunk[:ln]
            ents.append((_sha(chunk + bytes([ln & 255])), len(blob), ln, ln, 0))  # the hash is the client's word
            blob += chunk
            k += 1
    assert sorted({e[1] % 16 for e in ents}) == list(range(16))
    res, arcs = _write_and_check(ing, model, ents, bytes(blob), PB)
    assert res[0] == [1] * len(ents)
    stage, offs = arcs.extra["stage"].cpu().numpy(), arcs.extra["stage_off"].tolist()
    assert offs == [int(v) for v in np.cumsum([0] + [e[3] for e in ents[:-1]])]
    assert len({o % 16 for o in offs}) == 16 and int(arcs.extra["staged"].item()) == sum(e[3] for e in ents)
    for e, o in zip(ents, offs):
        assert stage[o: o + e[2]].tobytes() == bytes(blob[e[1]: e[1] + e[2]]), e[1:]
    assert _read_back(ing, arcs, model, ents, res, PB, cl) == len(ents)
    # n = 0 and n = 1
    res, arcs = _write_and_check(ing, model, [], b"", PB + 1000)
    assert res == ([], [], [], []) and arcs.n_arc == 0
    res, arcs = _write_and_check(ing, model, [(H(1), 1, 3, 3, 0)], b"\0abc", PB + 1000)
    assert res == ([1], [PB + 1000], [7], [0]) and model.chunks[PB + 1000] == b"abc"
    # one more than a tile
    n = _lib.INGEST_TILE + 1
    blob, ents = bytearray(b"\xee"), []
    for i in range(n):
        chunk = b"%05d" % i + bytes(i % 7)
        if i % 5 == 3 or i >= n - 2:   # a block of literals alone
            pay, comp = Z.emit([], chunk), 1
        else:
            pay, comp = chunk, 0
        raw = len(chunk) + (1 if i in (500, 1022) else 0)  # EBOUNDS (raw) / EDECODE (compressed: 1022 % 5 != 3: raw)
        if i == 1018:
            raw += 1  # 1018 % 5 == 3: compressed, EDECODE
        ents.append((H(100 + i), len(blob), len(pay) if i != 7 else 0, raw, comp))
        blob += pay
    res, arcs = _write_and_check(ing, model, ents, bytes(blob), PB + 2000)
    assert [i for i, s in enumerate(res[3]) if s] == [7, 500, 1018, 1022]
    assert [res[3][i] for i in (7, 500, 1018, 1022)] == [IM.EMPTY, IM.EBOUNDS, IM.EDECODE, IM.EBOUNDS]
    assert res[0][n - 1] == 1 and res[1][n - 1] == PB + 2000 + n - 5
    assert _read_back(ing, arcs, model, ents, res, PB + 2000, cl) == n - 4
    wr.destroy()
    ix.destroy()


@pytest.mark.gpu
def test_gpu_verify_refuses_a_wrong_hash():
    pytest.importorskip("torch")
    from sdfs_amd import HipVariableSha256HashEngine

    eng = HipVariableSha256HashEngine()
    cl = 8192
    a, b, c = _rnd(1, 4097), _rnd(2, 700), _rnd(3, 64)
    blk = Z.emit([], c)
    blob = a + b + blk
    ents = [(_sha(a), 0, len(a), len(a), 0), (_sha(a), len(a), len(b), len(b), 0),  # b under a's hash
            (_sha(c), len(a) + len(b), len(blk), len(c), 1), (H(5), 0, len(a), len(a), 0)]
    for verify in (True, False):
        ix, wr, ing = _ingest(cl, engine=eng, compress=False)
        model = IM.IngestModel(MM.IndexModel(), cl, digest=_sha)
        res, arcs = _write_and_check(ing, model, ents, blob, PB, verify=verify)
        if verify:
            assert res[3] == [0, IM.EHASH, 0, IM.EHASH] and res[0] == [1, 0, 1, 0]
            assert ing.check_hashes([H(5), _sha(a)]).tolist() == [-1, PB] and ix.refcount(_sha(a)) == 1
        else:  # stored under the client's hash, as the reference does
            assert res[3] == [0, 0, 0, 0] and res[0] == [1, 0, 1, 1]
            assert ing.check_hashes([H(5)]).tolist() == [PB + 2] and ix.refcount(_sha(a)) == 2
        assert _read_back(ing, arcs, model, ents, res, PB, cl) == sum(res[0])
        wr.destroy()
        ix.destroy()
    eng.destroy()


def _addref_and_check(ing, model, images, sb, hl, flags=None, miss_cap=1024):
    import torch

    req = _dev(np.frombuffer(b"".join(bytes(i).ljust(sb, b"\0") for i in images) or b"\0", np.uint8))
    stride = (sb - 13) // (hl + 24)
    ins = None
    if flags is not None:
        f = np.zeros((len(images), stride), np.uint8)
        for r, row in enumerate(flags):
            if row is not None:
                f[r, : len(row)] = row
        ins = _dev(f)
    got = ing.addref_slots(req, len(images), sb, ins, miss_cap=miss_cap)
    counts, status, missed, misses = model.addref_slots(images, sb, hl, flags)
    torch.cuda.synchronize()
    assert got.status.tolist() == status and got.req_missed.tolist() == missed
    assert got.counts.tolist()[:5] == counts[:5] and got.listed == min(counts[5], miss_cap)
    if miss_cap >= counts[5]:
        assert got.misses() == misses
    else:
        assert set(got.misses()) <= set(misses) and len(set(got.misses())) == miss_cap
    assert (got.added, got.missed, got.skipped, got.accepted, got.rejected) == tuple(counts[:5])
    assert _export(ing.index) == model.ix.export()
    return counts, status


@pytest.mark.gpu
@pytest.mark.parametrize("hl", [32, 16])
def test_gpu_addref_slots_vs_model(hl):
    pytest.importorskip("torch")
    rng = random.Random(50 + hl)
    big = 2 * WALK_PART + 1
    sb = 13 + (hl + 24) * big + 5
    ix, wr, ing = _ingest(65536, hl=hl, compress=False)
    model = IM.IngestModel(MM.IndexModel(), 65536)
    held = [(bytes(rng.getrandbits(8) for _ in range(hl)), 1000 + i) for i in range(700)]
    _load(ix, model.ix, [(d, p, 1) for d, p in held])
    unknown = bytes(rng.getrandbits(8) for _ in range(hl))
    a, b, c, d = held[:4]
    pick = lambda n: [rng.choice(held) for _ in range(n)]  # noqa: E731
    whole = pick(big)
    last_miss = whole[:-1] + [(whole[-1][0], whole[-1][1] ^ 1)]
    images = [b"",                                                                 # 0 an empty slot
              R.build_image(_pairs(pick(9))),                                      # 1 all inserted
              R.build_image(_pairs(pick(40))),                                     # 2 all held
              R.build_image(_pairs(pick(20) + [(a[0], a[1] + 1)] + pick(20))),     # 3 one wrong hashloc
              R.build_image(_pairs([a, b, (unknown, 5), c])),                      # 4 an unknown digest
              R.build_image(_pairs(pick(3)), zlen=big + 1),                        # 5 does not fit
              R.build_image([(a[0], a[1], 5, 0, 0, 5), (b[0], b[1], 5, 9, -4, 5)]),  # 6 a negative field
              R.build_image([(unknown, 3, 5, 0, 0, 5), (c[0], c[1], 5, 0, 0, 5), (b[0], b[1], 5, 9, 0, 5),
                             (d[0], d[1] ^ 2, 5, 9, 0, 5), (d[0], d[1], 5, 9, 0, 5)]),  # 7 repeated pos: the last wins
              R.build_image(_pairs([d] * 65 + [a])),                               # 8 a run across a wave's 64 lanes
              R.build_image(_pairs(last_miss)),                                    # 9 its only miss is its last pair
              R.build_image(_pairs(whole)),                                        # 10 the same slot, nothing missed
              R.build_image(_pairs([a, b])),                                       # 11 names a: accepted
              R.build_image(_pairs([a, (b[0], 7)])),                               # 12 names a: rejected
              R.build_image(_pairs([a, (unknown, 9), b])),                         # 13 unknown, but inserted
              R.build_image([(unknown, 3, 5, 0, 0, 5), (c[0], c[1], 5, 0, 0, 5)])]  # 14 the flag is on a dead pair
    flags = [None] * len(images)
    flags[1] = [1] * 9
    flags[13] = [0, 1, 0]
    flags[14] = [1, 0]
    counts, status = _addref_and_check(ing, model, images, sb, hl, flags)
    E = IM
    assert status == [0, 0, 0, E.EMISSED, E.EMISSED, E.CORRUPT, E.CORRUPT, 0, 0, E.EMISSED, 0, 0, E.EMISSED, 0, 0]
    assert counts == [40 + 2 + 66 + big + 2 + 2 + 1, 4, 9 + 1, 9, 6, 4]
    # one request at a time, with no flags at all; then a miss list that is too short
    for r in (13, 9, 10, 0):
        _addref_and_check(ing, model, images[r: r + 1], sb, hl)
    _addref_and_check(ing, model, [], sb, hl)
    counts, _ = _addref_and_check(ing, model, [images[3], images[4], images[12], images[9]], sb, hl, miss_cap=2)
    assert counts[:2] == [0, 4] and counts[4] == 4
    wr.destroy()
    ix.destroy()


@pytest.mark.gpu
def test_gpu_replacing_a_slot_keeps_the_counts_exact():
    torch = pytest.importorskip("torch")
    cl, hl = 4096, 32
    sb = 13 + 56 * 8
    nslots = 3
    ix, wr, ing = _ingest(cl, compress=False)
    model = IM.IngestModel(MM.IndexModel(), cl)
    chunks = [_rnd(20 + i, 500 + i) for i in range(5)]
    hs = [_sha(x) for x in chunks]
    fmap = torch.zeros(nslots * sb, dtype=torch.uint8, device="cuda")
    slots = [b""] * nslots
    flen, pb = 0, PB

    def step(send, named, dest, ln, expect_status=0):
        nonlocal flen, pb
        blob = b"".join(chunks[i] for i in send)
        ents, at = [], 0
        for i in send:
            ents.append((hs[i], at, len(chunks[i]), len(chunks[i]), 0))
            at += len(chunks[i])
        res, _ = _write_and_check(ing, model, ents, blob, pb)
        pb += len(send)
        where = model.check_hashes([hs[i] for i in named])
        img = R.build_image(_pairs(list(zip([hs[i] for i in named], where))))
        ins = [[1 if i in send else 0 for i in named]]
        got = ing.write_sparse_data_chunks(fmap, sb, [dest], [img], [ln], flen, inserted=ins)
        want, flen = model.write_sparse_data_chunks(slots, sb, hl, [dest], [img], [ln], flen, ins)
        torch.cuda.synchronize()
        assert got.status.tolist() == want[1] == [expect_status] and got.counts.tolist()[:5] == want[0][:5]
        assert int(got.file_len.item()) == flen
        assert fmap.cpu().numpy().tobytes() == b"".join(s.ljust(sb, b"\0") for s in slots)
        assert _export(ix) == model.ix.export()
        rc = ix.recount(fmap, nslots, sb, hash_len=hl)
        torch.cuda.synchronize()
        c = rc.counts.tolist()
        assert c[1:5] == [0, 0, 0, 0] and c[6] == len(model.ix.e) and c[7] == 0  # every entry equal

    step([0, 1, 2], [0, 1, 2], 1, 1500)
    assert flen == cl + 1500
    step([4], [1, 2, 4], 1, 900)            # the same destination: 0's reference goes, 1 and 2 keep one
    assert flen == cl + 1500 and model.ix.e[MM.pad32(hs[0])][1] == 0
    step([], [2, 2, 4], 2, 4096)            # another slot
    assert flen == 3 * cl and model.ix.e[MM.pad32(hs[2])][1] == 3
    before = model.ix.export()
    step([], [1, 3], 1, 10, IM.EMISSED)     # 3 was never sent: refused, the slot keeps its bytes
    assert model.ix.export() == before
    with pytest.raises(ValueError):
        ing.write_sparse_data_chunks(fmap, sb, [0, 0], [b"", b""], [0, 0], flen)
    with pytest.raises(ValueError):
        ing.write_sparse_data_chunks(fmap, sb, [nslots], [b""], [0], flen)
    with pytest.raises(ValueError):
        ing.write_sparse_data_chunks(fmap, sb, [-1], [b""], [0], flen)
    wr.destroy()
    ix.destroy()


_KEY = bytes(range(7, 39))
L, NBUF = 65536, 8


@pytest.mark.gpu
@pytest.mark.parametrize("variant,algo", [("raw", "sha256"), ("lz4", "sha256"), ("aes", "sha256"), ("lz4", "md5")])
def test_gpu_the_two_routes_agree(variant, algo):
    """Eight buffers of 64 KiB, half their content repeated, chunked by the engine.  Route A:
    HipBufferWriter.write.  Route B: check_hashes, write_chunks of the first occurrence of each absent
    fingerprint, images built on the host from the answers, write_sparse_data_chunks."""
    torch = pytest.importorskip("torch")
    from oracle import lz4_oracle as ZO
    from sdfs_amd import HipVariableMD5HashEngine, HipVariableSha256HashEngine
    from sdfs_amd.archive import HipBufferWriter
    from sdfs_amd.device import DeviceBatch
    from sdfs_amd.index import HipHashesMap
    from sdfs_amd.ingest import HipChunkIngest
    from sdfs_amd.meta import slot_bytes
    from sdfs_amd.read import HipBufferReader

    e = HipVariableMD5HashEngine() if algo == "md5" else HipVariableSha256HashEngine()
    hl = 16 if algo == "md5" else 32
    aes = variant == "aes"
    batch = DeviceBatch(e, nbuf=NBUF, buf_len=L)
    batch.fill_streams(first_stream=977, bufs_per_stream=2)
    v = batch.data.view(NBUF, L)
    v[1, 20000:50000] = 0
    for b in range(NBUF // 2, NBUF):
        v[b, : L // 2 + 777 * b].copy_(v[b - NBUF // 2, : L // 2 + 777 * b])
    ivs = _dev(np.frombuffer(np.random.default_rng(12).bytes(16 * 64), np.uint8).reshape(-1, 16)) if aes else None
    mk = lambda ix: HipBufferWriter(ix, hash_len=hl, compress=variant != "raw", aes=_KEY if aes else None,  # noqa: E731
                                    version=1 if aes else 0, blocksz=[60000, 90000, 50000])
    # route A
    ixa = HipHashesMap(1 << 12)
    wa = mk(ixa)
    ma, arcs_a = wa.write(batch, PB, ivs=ivs)
    torch.cuda.synchronize()
    assert int(arcs_a.extra["overflow"].item()) == 0
    host = batch.data.cpu().numpy().reshape(NBUF, L)
    counts, st, ln, dg, total = batch.host_results()
    recs = [(b, int(st[b, i]), int(ln[b, i]), dg[b, i, :hl].tobytes())
            for b in range(NBUF) for i in range(int(counts[b]))]
    assert len(recs) == total
    # route B: the client
    ixb = HipHashesMap(1 << 12)
    wb = mk(ixb)
    ing = HipChunkIngest(wb, L, engine=e)
    held = ing.check_hashes([r[3] for r in recs]).tolist()
    assert held == [-1] * total
    first, ents = {}, []
    for r, (b, s, n, h) in enumerate(recs):
        if h not in first:
            first[h] = r
            chunk = host[b, s: s + n].tobytes()
            ents.append((h, ZO.compress(chunk), True, n) if len(ents) % 3 == 1 else (h, chunk, False, n))
    assert len(first) < total  # something repeats
    ins, pos, stored, status, arcs_b = ing.write_chunks(ents, PB, verify=True, ivs=ivs)
    torch.cuda.synchronize()
    assert not status.any() and ins.all() and pos.tolist() == list(range(PB, PB + len(ents)))
    where = dict(zip(first, pos.tolist()))
    sl = slot_bytes(hl, e.config.chunk_length, e.config.min_len)  # the slots write() emits
    assert ma.numel() == NBUF * sl
    images, flags = [], []
    for b in range(NBUF):
        mine = [(r, rec) for r, rec in enumerate(recs) if rec[0] == b]
        images.append(MO.sparse_data_chunk_bytes([(h, where[h], n, s, first[h] != r) for r, (_, s, n, h) in mine]))
        flags.append([first[h] == r for r, (_, _, _, h) in mine])
    fmap = torch.zeros(NBUF * sl, dtype=torch.uint8, device="cuda")
    out = ing.write_sparse_data_chunks(fmap, sl, list(range(NBUF)), images, [L] * NBUF, 0, inserted=flags)
    torch.cuda.synchronize()
    assert not out.status.any() and out.counts.tolist() == [total - len(first), 0, len(first), NBUF, 0, 0]
    assert int(out.file_len.item()) == NBUF * L and out.released.counts.tolist() == [0, 0, 0, 0]
    # the same store, the same maps, the same index
    assert (arcs_a.n_arc, arcs_a.n_rec, arcs_a.store_bytes) == (arcs_b.n_arc, arcs_b.n_rec, arcs_b.store_bytes)
    assert arcs_a.n_arc >= 3 and stored.tolist() == arcs_b.store_len.tolist()
    for a in range(arcs_a.n_arc):
        assert arcs_a.image(a) == arcs_b.image(a) and arcs_a.map_image(a) == arcs_b.map_image(a), a
    for x, y in zip(arcs_a.directory(), arcs_b.directory()):
        assert x.tolist() == y.tolist()
    assert ma.cpu().numpy().tobytes() == fmap.cpu().numpy().tobytes()
    assert _export(ixa) == _export(ixb)
    ra, rb = ixa.recount(ma, NBUF, sl, hash_len=hl), ixb.recount(fmap, NBUF, sl, hash_len=hl)
    torch.cuda.synchronize()
    assert ra.counts.tolist() == rb.counts.tolist() == [total, 0, 0, 0, 0, 0, len(first), 0]
    rd = HipBufferReader(L, hl, aes=_KEY if aes else None, record_ivs=aes, engine=e)
    got, rstatus, _ = rd.read(fmap, NBUF, sl, arcs_b.store, *arcs_b.directory(), PB,
                              out=torch.full((NBUF, L), 0xFF, dtype=torch.uint8, device="cuda:0"),
                              store_ivs=arcs_b.record_ivs())
    torch.cuda.synchronize()
    assert not rstatus.any() and (got.cpu().numpy() == host).all()
    rd.destroy()
    for w in (wa, wb):
        w.destroy()
    ixa.destroy()
    ixb.destroy()
    e.destroy()
