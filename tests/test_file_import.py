"""Importing a map file from another volume (include/sdfs_import.h, sdfs_amd/replicate.py): missing
chunks fetched from the source's store, every pair re-homed to the destination's hashlocs
(GetCloudFile.checkDedupFile, GetCloudFile.java:184-249; LongByteArrayMap.index(), :310-356).

The model (tests/import_model.py) restates the rule over tests/mapfile_model.IndexModel.  CPU: the
model against a hand-worked case; the argument checks of the entry points (no device).  GPU: every
result of the HIP calls equals the model's, bit for bit, and the import leaves on the destination
what HipBufferWriter.write of the same buffers leaves there."""
import ctypes
import hashlib
import struct
from types import SimpleNamespace

import numpy as np
import pytest

from sdfs_amd import _lib
from tests import import_model as XM
from tests import mapfile_model as MM
from tests import read_model as R

PB = 1 << 33
L, NBUF = 262144, 8          # chunk_length 256 KiB, a source of 8 buffers (2 MiB)
_KEY_A = bytes(range(7, 39))
_KEY_B = bytes(range(100, 132))
_ENG = {}


def H(i, hl=32):
    return (b"h%07d" % i).ljust(hl, b"\x5a")


def _sha(b):
    return hashlib.sha256(bytes(b)).digest()


def _md5(b):
    return hashlib.md5(bytes(b)).digest()


def _be64(v):
    return struct.pack(">q", v)


# ------------------------------------------------------------------------------------------
# CPU: the model, hand-worked
# ------------------------------------------------------------------------------------------
def test_model_hand_worked():
    """Three requests into a destination that already holds chunk B at position 700.  The source
    (pos_base 50) stores A, B, C, D at 50..53; D's entry was dropped by a compaction.  Request 0
    names A, B, A; request 1 names C and A (A: one fingerprint named by two requests); request 2
    names D, which nothing can fetch."""
    a, b, c, d = b"A" * 40, b"B" * 17, b"C" * 33, b"D" * 9
    ha, hb, hc, hd = H(1), H(2), H(3), H(4)
    ix = MM.IndexModel()
    ix.load([(hb, 700, 1)])
    src = XM.SourceModel(50, [(44, 40, a), (21, 17, b), (37, 33, c), (0, 9, d)])
    sb = 13 + 3 * 56
    img0 = R.build_image([(ha, 50, 40, 0, 0, 40), (hb, 51, 17, 40, 0, 17), (ha, 50, 40, 57, 0, 40)], flags=1, doop=17)
    img1 = R.build_image([(hc, 52, 33, 0, 0, 33), (ha, 50, 40, 33, 5, 20)])
    img2 = R.build_image([(hd, 53, 9, 0, 0, 9)])
    old = R.build_image([(hb, 700, 17, 0, 0, 17)])  # the slot request 0 replaces: its pair is released
    slots = [old, b"", b"\x07" * sb]
    m = XM.ImportModel(ix, 100)
    out = m.import_slots(src, [img0, img1, img2], [0, 1, 2], [97, 53, 9], slots, sb, 32, 10, 900)
    assert out.status == [0, 0, XM.EMISSING] and out.req_missed == [0, 0, 1]
    # fetches in ascending k: A (k 0) at 0, C (k 2) at 48 = 40 rounded up to 16
    assert out.fetches == [0, 2] and out.dst_off == [0, 48]
    p = MM.pad32
    assert out.records == [(p(ha), 0, 0, 40), (p(hb), 0, 0, 0), (p(ha), 0, 0, 40), (p(hc), 1, 0, 33), (p(ha), 0, 0, 40)]
    assert out.pair_rec == [{0: 0, 1: 1, 2: 2}, {0: 3, 1: 4}, {}]
    # the first record of A inserts it at 900, the first of C at 901; B stays where it was
    assert out.new_list == [0, 3] and out.hashloc == [900, 700, 900, 901, 900]
    assert out.chunks == {900: a, 901: c}
    # A: three pairs; B: its old slot's pair released, one added; C: one; D: never inserted
    assert ix.export() == sorted([(p(ha), 900, 3), (p(hb), 700, 1), (p(hc), 901, 1)])
    # records, held, fetches, raw bytes fetched, accepted, rejected, hashloc changed, missed
    assert out.counts == [5, 1, 2, 73, 2, 1, 5, 1]
    want0 = (b"\x01" + img0[1:9] + ha + _be64(900) + img0[9 + 40: 9 + 56] + hb + _be64(700) + img0[65 + 40: 65 + 56]
             + ha + _be64(900) + img0[121 + 40: 121 + 56] + struct.pack(">I", 17))
    assert len(want0) == sb and slots[0] == want0
    want1 = img1[:9] + hc + _be64(901) + img1[49:65] + ha + _be64(900) + img1[105:121] + bytes(4)
    assert slots[1] == want1.ljust(sb, b"\0") and slots[2] == b"\x07" * sb
    assert out.file_len == max(10, 0 * 100 + 97, 1 * 100 + 53) == 153


def test_model_all_or_nothing_and_verify():
    a, b = b"A" * 40, b"B" * 17
    src = XM.SourceModel(0, [(44, 40, a), (21, 17, None), (44, 40, b"x" * 39)])
    sb = 13 + 2 * 56
    imgs = [R.build_image([(_sha(a), 0, 40, 0, 0, 40), (H(2), 1, 17, 40, 0, 17)]),  # the second fetch fails
            R.build_image([(_sha(a), 0, 40, 0, 0, 40)]),                            # accepted
            R.build_image([(H(3), 2, 40, 0, 0, 40)]),                               # decodes to 39 bytes, not 40
            R.build_image([(H(4), 0, 40, 0, 0, 40)]),                               # A's chunk under another hash
            R.build_image([(H(5), 1 << 62, 1, 0, 0, 1), (H(6), -1, 1, 0, 0, 1)])]   # the first pair is shadowed
    for verify in (False, True):
        ix = MM.IndexModel()
        slots = [b""] * 5
        out = XM.ImportModel(ix, 100, digest=_sha).import_slots(src, imgs, [4, 3, 2, 1, 0], [1] * 5, slots, sb, 32, 0,
                                                                7, verify=verify)
        assert out.status == [XM.EFETCH, 0, XM.EFETCH, XM.EHASH if verify else 0, XM.EMISSING]
        assert out.req_missed == [0, 0, 0, 0, 1] and slots[4] == slots[2] == slots[0] == b""
        p = MM.pad32
        want = [(p(_sha(a)), 7, 1)] + ([] if verify else [(p(H(4)), 7 + 1, 1)])
        assert ix.export() == sorted(want)
        assert out.counts[:3] == ([1, 0, 3] if verify else [2, 0, 3])  # the fetch list was settled before the decision


# ------------------------------------------------------------------------------------------
# CPU: the entry points refuse bad arguments before the device is touched
# ------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_before_the_device():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    h = ctypes.addressof(ctypes.create_string_buffer(4096))  # a handle that is never looked at
    E = _lib.EINVAL
    sb = 13 + 5 * 56

    def work(**kw):
        f = {k: p for k, _ in _lib.ImportWork._fields_}
        f.update(kw)
        return ctypes.byref(_lib.ImportWork(**f))

    calls = {
        "pairs": lambda w=work(), n=1, hl=32, stride=5, req=p, slot=sb: lib.sdfs_cdc_import_pairs(
            0, req, n, slot, hl, stride, w, None),
        "plan": lambda w=work(), n=1, stride=5, pos=p, ns=1, d=p, o=p, cl=4096, fc=p, tb=p: lib.sdfs_cdc_import_plan(
            0, n, stride, w, pos, 0, ns, d, d, d, cl, fc, o, o, o, o, None, tb, None),
        "records": lambda w=work(), n=1, hl=32, stride=5, e=None, nf=1, f=p, rec=p, ct=p, fc=p:
            lib.sdfs_cdc_import_records(0, e, n, stride, hl, w, fc, nf, f, f, f, f, rec, ct, None),
        "install": lambda w=work(), n=1, hl=32, stride=5, req=p, slot=sb, loc=p, dd=p, cl=4096, m=p, ns=4, fl=p:
            lib.sdfs_cdc_import_install(0, req, n, slot, hl, stride, w, loc, dd, dd, cl, m, ns, fl, None),
    }
    for name, f in calls.items():
        assert f(w=None) == E and b"null work" in lib.sdfs_cdc_last_error(), name
        for k, _ in _lib.ImportWork._fields_:
            assert f(w=work(**{k: None})) == E and b"null work array" in lib.sdfs_cdc_last_error(), (name, k)
        assert f(n=1 << 31) == E and b"split the batch" in lib.sdfs_cdc_last_error(), name
        assert f(w=work(hashes=p + 4)) == E and b"16-byte aligned" in lib.sdfs_cdc_last_error(), name
        assert f(stride=0) == E, name
    for name in ("pairs", "records", "install"):
        assert calls[name](hl=20) == E and b"hash_len 20" in lib.sdfs_cdc_last_error(), name
    for name in ("pairs", "install"):
        assert calls[name](stride=4) == E and b"pair_stride 4" in lib.sdfs_cdc_last_error(), name
        assert calls[name](slot=12) == E and b"slot_bytes" in lib.sdfs_cdc_last_error(), name
        assert calls[name](req=None) == E, name
    assert calls["pairs"](hl=16, stride=6) == E  # a 293-byte slot holds 7 MD5 pairs
    assert calls["plan"](pos=None) == E and calls["plan"](d=None) == E and calls["plan"](o=None) == E
    assert calls["plan"](fc=None) == E and calls["plan"](tb=None) == E and calls["plan"](ns=1 << 31) == E
    assert calls["plan"](cl=0) == E and b"chunk_length" in lib.sdfs_cdc_last_error()
    assert calls["records"](rec=None) == E and calls["records"](ct=None) == E and calls["records"](fc=None) == E
    assert calls["records"](f=None) == E and calls["records"](rec=p + 8) == E
    assert calls["records"](e=h) == E and b"engine" in lib.sdfs_cdc_last_error()  # not a live engine handle
    assert calls["install"](loc=None) == E and calls["install"](dd=None) == E and calls["install"](m=None) == E
    assert calls["install"](fl=None) == E and b"file length" in lib.sdfs_cdc_last_error()
    assert calls["install"](cl=0) == E and calls["install"](n=5, ns=4) == E
    # destinations: distinct and inside the map
    arr = lambda *v: (ctypes.c_uint64 * len(v))(*v)  # noqa: E731
    assert lib.sdfs_cdc_import_check_dests(arr(3, 0, 2), 3, 4) == _lib.OK
    assert lib.sdfs_cdc_import_check_dests(None, 0, 0) == _lib.OK
    assert lib.sdfs_cdc_import_check_dests(arr(0, 4), 2, 4) == E and b"outside the map" in lib.sdfs_cdc_last_error()
    assert lib.sdfs_cdc_import_check_dests(arr(1, 2, 1), 3, 4) == E and b"two requests" in lib.sdfs_cdc_last_error()
    assert lib.sdfs_cdc_import_check_dests(None, 1, 4) == E


def test_wrapper_refuses_before_the_device():
    """verify without an engine, another hash length on the source, duplicate or out-of-range
    destinations: ValueError from the wrapper's own checks (no tensor is made for them)."""
    from sdfs_amd.replicate import HipFileImport, SourceVolume

    wr = SimpleNamespace(index=None, hash_len=32)
    imp = HipFileImport(wr, 4096)
    t = SimpleNamespace(dtype=None, is_contiguous=lambda: True, shape=(0,))
    with pytest.raises(ValueError, match="engine"):
        imp._check(SourceVolume(t, t, t, t, 0), True)
    with pytest.raises(ValueError, match="16 bytes"):
        imp._check(SourceVolume(t, t, t, t, 0, hash_len=16), False)
    with pytest.raises(ValueError, match="hash_len"):
        HipFileImport(SimpleNamespace(index=None, hash_len=20), 4096)
    with pytest.raises(ValueError, match="chunk_length"):
        HipFileImport(wr, 0)
    from sdfs_amd.ingest import check_destinations

    for bad in ([0, 0], [4], [-1]):
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


def _engine(algo="sha256"):
    from sdfs_amd import HipVariableMD5HashEngine, HipVariableSha256HashEngine

    if algo not in _ENG:
        _ENG[algo] = HipVariableMD5HashEngine() if algo == "md5" else HipVariableSha256HashEngine()
    return _ENG[algo]


def _ivs(seed=12):
    return _dev(np.frombuffer(np.random.default_rng(seed).bytes(16 * 64), np.uint8).reshape(-1, 16))


def _writer(ix, variant, hl=32, key=_KEY_A):
    """raw | lz4 | aes (LZ4 + AES-256, version 1 archives) | aesraw (AES over the raw frame)."""
    from sdfs_amd.archive import HipBufferWriter

    aes = variant.startswith("aes")
    return HipBufferWriter(ix, hash_len=hl, compress=variant in ("lz4", "aes"), aes=key if aes else None,
                           version=1 if aes else 0, blocksz=[300000, 500000, 400000])


def _batch(e, nbuf=NBUF, first_stream=977):
    """Buffers of engine chunks, the second half's first part a copy of the first half's."""
    from sdfs_amd.device import DeviceBatch

    batch = DeviceBatch(e, nbuf=nbuf, buf_len=L)
    batch.fill_streams(first_stream=first_stream, bufs_per_stream=2)
    v = batch.data.view(nbuf, L)
    v[1, 20000:50000] = 0
    for b in range(nbuf // 2, nbuf):
        v[b, : L // 2 + 777 * b].copy_(v[b - nbuf // 2, : L // 2 + 777 * b])
    return batch


def _volume(variant="raw", algo="sha256", pos_base=PB, key=_KEY_A, ivs=None, batch=None, cap=1 << 12):
    """A volume written by HipBufferWriter.write on an empty index: everything a test needs of it."""
    import torch

    from sdfs_amd.index import HipHashesMap
    from sdfs_amd.meta import slot_bytes

    e = _engine(algo)
    hl = 16 if algo == "md5" else 32
    batch = batch if batch is not None else _batch(e)
    ix = HipHashesMap(cap)
    wr = _writer(ix, variant, hl, key)
    aes = variant.startswith("aes")
    if aes and ivs is None:
        ivs = _ivs()
    m, arcs = wr.write(batch, pos_base, ivs=ivs)
    torch.cuda.synchronize()
    assert int(arcs.extra["overflow"].item()) == 0
    nbuf = batch.data.numel() // L
    sl = slot_bytes(hl, e.config.chunk_length, e.config.min_len)
    assert e.config.chunk_length == L and m.numel() == nbuf * sl
    return SimpleNamespace(e=e, hl=hl, batch=batch, ix=ix, wr=wr, m=m, arcs=arcs, sl=sl, nbuf=nbuf, pos_base=pos_base,
                           key=key if aes else None, ivs=ivs, variant=variant,
                           host=batch.data.cpu().numpy().reshape(nbuf, L).copy())


def _close(*vols):
    for v in vols:
        v.wr.destroy()
        v.ix.destroy()


def _source(S, **kw):
    from sdfs_amd.replicate import SourceVolume

    src = SourceVolume.from_archives(S.arcs, S.pos_base, aes=S.key)
    for k, v in kw.items():
        setattr(src, k, v)
    return src


def _source_model(S):
    """The source's directory with the chunk behind every entry: entry k is the k-th record that
    inserted, in record order."""
    counts, st, ln, dg, total = S.batch.host_results()
    recs = [(b, int(st[b, i]), int(ln[b, i])) for b in range(S.nbuf) for i in range(int(counts[b]))]
    new = S.arcs.extra["new_list"].tolist()
    slen, raw = S.arcs.store_len.tolist(), S.arcs.raw_len.tolist()
    assert len(new) == len(slen)
    ents = []
    for k, r in enumerate(new):
        b, s, n = recs[r]
        assert n == raw[k]
        ents.append((slen[k], raw[k], S.host[b, s: s + n].tobytes()))
    return XM.SourceModel(S.pos_base, ents)


def _images(m, nslots, sl):
    host = m.cpu().numpy().tobytes()
    return [host[s * sl: (s + 1) * sl] for s in range(nslots)]


def _index_model(ix):
    mi = MM.IndexModel()
    mi.e = {d: [p, r] for d, p, r in _export(ix)}
    return mi


def _importer(D, cl=L, engine=None):
    from sdfs_amd.replicate import HipFileImport

    return HipFileImport(D.wr, cl, engine=engine)


def _import_and_check(imp, src, srcm, images, dests, lens, fmap, sl, hl, flen, pos_base, verify=False, digest=_sha):
    """import_slots on the device and on the model (whose index starts as the device's is): status,
    misses, records, fetch plan, counts, pair_rec, the file's map, its length and the index equal."""
    import torch

    nslots = fmap.numel() // sl
    slots = _images(fmap, nslots, sl)
    model = XM.ImportModel(_index_model(imp.index), imp.chunk_length, digest=digest)
    want = model.import_slots(srcm, images, dests, lens, slots, sl, hl, flen, pos_base, verify=verify)
    res, arcs = imp.import_slots(src, images, dests, lens, fmap, sl, flen, pos_base, verify=verify)
    torch.cuda.synchronize()
    assert res.status.tolist() == want.status and res.req_missed.tolist() == want.req_missed
    assert res.counts.tolist() == want.counts
    nrec = len(want.records)
    assert int(arcs.extra["count"].item()) == nrec
    recs = arcs.extra["records"][:nrec].cpu().numpy()
    for n, (h, f, s0, ln) in enumerate(want.records):
        assert recs[n].tobytes() == h + struct.pack("<QII", f, s0, ln), n
    plan = arcs.extra["plan"]
    nf = len(want.fetches)
    assert int(plan["fetch_count"].item()) == nf == arcs.extra["n_fetch"]
    assert plan["dst_off"][:nf].tolist() == want.dst_off
    assert plan["dst_cap"][:nf].tolist() == [srcm.entries[k][1] for k in want.fetches]
    assert plan["src_len"][:nf].tolist() == [srcm.entries[k][0] for k in want.fetches]
    pr = res.pair_rec.cpu().numpy()
    for r, mine in enumerate(want.pair_rec):
        assert {i: int(v) for i, v in enumerate(pr[r]) if v >= 0} == mine, r
    assert arcs.extra["new_list"].tolist() == want.new_list and arcs.n_rec == len(want.new_list)
    assert arcs.extra["hashloc"][:nrec].tolist() == want.hashloc
    assert _images(fmap, nslots, sl) == [bytes(s).ljust(sl, b"\0") for s in slots]
    assert int(res.file_len.item()) == want.file_len
    assert _export(imp.index) == model.ix.export()
    return want, res, arcs


def _all_equal(ix, fmap, nslots, sl, hl):
    """recount reports every entry equal: nothing missed, nothing corrupt, no mismatch."""
    import torch

    rc = ix.recount(fmap, nslots, sl, hash_len=hl)
    torch.cuda.synchronize()
    c = rc.counts.tolist()
    assert c[1:6] == [0, 0, 0, 0, 0] and c[6] == ix.stats().live and c[7] == 0, c
    return c


def _read(D, fmap, nslots, store, directory, pos_base, ivs, sl=None):
    import torch

    from sdfs_amd.read import HipBufferReader

    rd = HipBufferReader(L, D.hl, aes=D.key, record_ivs=D.key is not None, engine=D.e)
    out = torch.full((nslots, L), 0xFF, dtype=torch.uint8, device="cuda:0")
    got, status, _ = rd.read(fmap, nslots, sl or D.sl, store, *directory, pos_base, out=out, store_ivs=ivs)
    torch.cuda.synchronize()
    rd.destroy()
    assert not status.any()
    return got.cpu().numpy()


def _pairs_of(S, slot):
    """The pairs of one slot of S's map, in image order, as build_image takes them."""
    st, pairs, _, _ = R.parse(_images(S.m, S.nbuf, S.sl)[slot], S.sl, S.hl)
    assert st == R.OK and pairs
    return pairs


@pytest.mark.gpu
def test_gpu_one_batch_with_every_case():
    torch = pytest.importorskip("torch")
    S = _volume("lz4")
    srcm = _source_model(S)
    n_src = len(srcm.entries)
    from sdfs_amd.index import HipHashesMap

    ix = HipHashesMap(1 << 12)
    D = SimpleNamespace(ix=ix, wr=_writer(ix, "raw"), hl=32, sl=S.sl, key=None, e=S.e)
    imp = _importer(D)
    nslots = 14
    fmap = torch.full((nslots * S.sl,), 0xEE, dtype=torch.uint8, device="cuda")
    src = _source(S)
    # slot 0 first, so that the big batch finds something held
    p0, p1, p2, p3 = (_pairs_of(S, s) for s in range(4))
    img = lambda s: _images(S.m, S.nbuf, S.sl)[s]  # noqa: E731
    want, res, _ = _import_and_check(imp, src, srcm, [img(0)], [5], [L], fmap, S.sl, 32, 0, PB + 7)
    assert want.status == [0] and want.counts[1] == 0 and want.counts[2] > 0
    # a directory whose last-of-slot-3 entry a compaction has dropped
    kz = p3[-1][1] - S.pos_base
    named_elsewhere = {q[1] for s in (0, 1, 2) for q in _pairs_of(S, s)} | {q[1] for q in p3[:-1]}
    assert p3[-1][1] not in named_elsewhere
    slen = S.arcs.store_len.clone()
    slen[kz] = 0
    src = _source(S, store_len=slen)
    srcm.entries[kz] = (0,) + srcm.entries[kz][1:]
    garbage = (1 << 62) + 12345
    held_far = [(p0[0][0], S.pos_base + n_src + 5) + tuple(p0[0][2:])]  # held here: its hashloc is never followed
    shadow = [(H(99), garbage, 5, p2[0][3], 0, 5)] + [tuple(q) for q in p2[:3]]  # pair 0 shares p2[0]'s pos: dead
    images = [img(0),                                                         # 0 all held: zero fetches of its own
              img(1),                                                         # 1 none held
              R.build_image([tuple(q) for q in p0[:2]] + [tuple(q) for q in p2[2:5]], flags=3, doop=9),  # 2 mixed
              b"",                                                            # 3 an all-zero image
              R.build_image([tuple(q) for q in p1[:3]], zlen=(S.sl - 13) // 56 + 1),  # 4 zlen too large
              R.build_image([tuple(p1[0]), tuple(p1[1][:5]) + (-3,)]),        # 5 a negative nlen
              R.build_image(shadow),                                          # 6 the shadowed pair's bytes are kept
              R.build_image([tuple(q) for q in p2[:2]] + [(H(50), S.pos_base + n_src, 9, 99999, 0, 9)]),  # 7 k >= n_src
              R.build_image([tuple(p3[-1])]),                                 # 8 store_len[k] == 0
              R.build_image(held_far),                                        # 9 accepted
              R.build_image([(H(51), S.pos_base - 1, 9, 0, 0, 9)])]           # 10 hashloc below the source's base
    dests = [0, 1, 2, 3, 4, 13, 6, 7, 8, 9, 10]
    lens = [L, L, 77, 0, L, L, L, L, L, 5, 5]
    want, res, arcs = _import_and_check(imp, src, srcm, images, dests, lens, fmap, S.sl, 32, 123, PB + 1000)
    C, M = XM.CORRUPT, XM.EMISSING
    assert want.status == [0, 0, 0, 0, C, C, 0, M, M, 0, M] and want.req_missed == [0] * 7 + [1, 1, 0, 1]
    assert want.counts[4:6] == [6, 5] and want.counts[7] == 3
    assert all(f == 0 and ln == 0 for _, f, _, ln in want.records[: len(p0)])  # request 0: every pair held
    got6 = _images(fmap, nslots, S.sl)[6]
    assert got6[9: 9 + 32] == H(99) and got6[9 + 32: 9 + 40] == _be64(garbage)  # dead pair: copied byte for byte
    assert _images(fmap, nslots, S.sl)[13] == b"\xee" * S.sl and want.file_len == 9 * L + 5
    # nreq = 0
    want, res, arcs = _import_and_check(imp, src, srcm, [], [], [], fmap, S.sl, 32, 55, PB + 5000)
    assert want.counts == [0] * 8 and arcs.n_arc == 0 and int(res.file_len.item()) == 55
    imp.destroy()
    _close(S, D)


@pytest.mark.gpu
@pytest.mark.parametrize("variant,algo", [("raw", "sha256"), ("lz4", "sha256"), ("aes", "sha256"), ("lz4", "md5")])
def test_gpu_the_two_routes_agree(variant, algo):
    """write() on an empty volume, then the whole file imported into an empty destination with the
    same settings, IVs and pos_base: the destination is what write() of the same buffers leaves."""
    torch = pytest.importorskip("torch")
    from sdfs_amd.index import HipHashesMap

    S = _volume(variant, algo)
    srcm = _source_model(S)
    hl = S.hl
    digest = _md5 if algo == "md5" else _sha
    for delta in (0, 4321):
        ix = HipHashesMap(1 << 12)
        D = SimpleNamespace(ix=ix, wr=_writer(ix, variant, hl), hl=hl, sl=S.sl, key=S.key, e=S.e)
        imp = _importer(D, engine=S.e)
        fmap, res, arcs = imp.import_file(_source(S), S.m, S.nbuf, S.sl, S.nbuf * L, PB + delta, verify=True, ivs=S.ivs)
        torch.cuda.synchronize()
        assert not res.status.any() and res.accepted == S.nbuf and res.rejected == 0 and res.missed == 0
        assert res.held == 0 and res.fetches == S.arcs.n_rec and int(res.file_len.item()) == S.nbuf * L
        assert res.changed == (0 if delta == 0 else res.records)
        A, B = S.arcs, arcs
        assert (A.n_arc, A.n_rec, A.store_bytes) == (B.n_arc, B.n_rec, B.store_bytes) and A.n_arc >= 3
        for a in range(A.n_arc):
            assert A.image(a) == B.image(a) and A.map_image(a) == B.map_image(a), a
        for x, y in zip(A.directory(), B.directory()):
            assert x.tolist() == y.tolist()
        ea, eb = _export(S.ix), _export(ix)
        assert [(d, p + delta, r) for d, p, r in ea] == eb
        if delta == 0:
            assert torch.equal(fmap, S.m)
        else:  # only the hashlocs differ, and by that delta
            for s, (x, y) in enumerate(zip(_images(S.m, S.nbuf, S.sl), _images(fmap, S.nbuf, S.sl))):
                px, py = R.parse(x, S.sl, hl), R.parse(y, S.sl, hl)
                assert px[0] == py[0] == R.OK and px[2:] == py[2:]
                assert [(q[0], q[1] + delta) + tuple(q[2:]) for q in px[1]] == [tuple(q) for q in py[1]], s
                bal = hl + 24
                for i in range(len(px[1])):
                    at = 9 + i * bal + hl
                    x = x[:at] + _be64(px[1][i][1] + delta) + x[at + 8:]
                assert x == y, s
        _all_equal(ix, fmap, S.nbuf, S.sl, hl)
        if delta:  # the model says the same
            ixm = HipHashesMap(1 << 12)
            Dm = SimpleNamespace(ix=ixm, wr=_writer(ixm, variant, hl), hl=hl, sl=S.sl, key=S.key, e=S.e)
            im2 = _importer(Dm, engine=S.e)
            f2 = torch.zeros_like(fmap)
            _import_and_check(im2, _source(S), srcm, _images(S.m, S.nbuf, S.sl), list(range(S.nbuf)), [L] * S.nbuf, f2,
                              S.sl, hl, 0, PB + delta, verify=True, digest=digest)
            assert torch.equal(f2, fmap)
            im2.destroy()
            _close(Dm)
        imp.destroy()
        _close(D)
    _close(S)


@pytest.mark.gpu
@pytest.mark.parametrize("sv,dv", [("aes", "raw"), ("raw", "aes")])
def test_gpu_different_settings_on_the_two_sides(sv, dv):
    """LZ4 + AES (key A, version 1) -> raw version 0, and raw -> LZ4 + AES (key B)."""
    torch = pytest.importorskip("torch")
    from sdfs_amd.index import HipHashesMap

    S = _volume(sv, key=_KEY_A)
    store_before, export_before = S.arcs.store.clone(), _export(S.ix)
    ix = HipHashesMap(1 << 12)
    key = _KEY_B if dv == "aes" else None
    D = SimpleNamespace(ix=ix, wr=_writer(ix, dv, 32, _KEY_B), hl=32, sl=S.sl, key=key, e=S.e)
    imp = _importer(D)
    pb = 31
    fmap, res, arcs = imp.import_file(_source(S), S.m, S.nbuf, S.sl, S.nbuf * L, pb, ivs=_ivs(5) if key else None)
    torch.cuda.synchronize()
    assert not res.status.any() and res.accepted == S.nbuf and res.changed == res.records
    got = _read(D, fmap, S.nbuf, arcs.store, arcs.directory(), pb, arcs.record_ivs() if key else None)
    assert (got == S.host).all()
    _all_equal(ix, fmap, S.nbuf, S.sl, 32)
    assert torch.equal(S.arcs.store, store_before) and _export(S.ix) == export_before  # the source is read only
    imp.destroy()
    _close(S, D)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["lz4", "raw"])
def test_gpu_a_damaged_source_record(variant):
    """lz4: a record whose nz word says raw_len + 1, so the decode cannot fit dst_cap (EFETCH).  raw,
    with verify: one flipped payload byte (EHASH); without verify the flipped chunk is imported under
    the source's hash, which is the reference's behaviour: it never looks at the data."""
    torch = pytest.importorskip("torch")
    from sdfs_amd.index import HipHashesMap

    S = _volume(variant)
    srcm = _source_model(S)
    p2 = _pairs_of(S, 2)
    bad_pair = p2[len(p2) // 2]
    k = bad_pair[1] - S.pos_base
    users = [s for s in range(S.nbuf) if any(q[1] == bad_pair[1] for q in _pairs_of(S, s))]
    assert users and len(users) < S.nbuf
    store = S.arcs.store.clone()
    off = int(S.arcs.store_off[k].item())
    slen, raw, chunk = srcm.entries[k]
    if variant == "lz4":
        store[off: off + 4] = _dev(np.frombuffer(struct.pack(">I", raw + 1), np.uint8))
        srcm.entries[k] = (slen, raw, None)
    else:
        store[off + 4 + raw // 2] ^= 0x40
        flipped = bytearray(chunk)
        flipped[raw // 2] ^= 0x40
        srcm.entries[k] = (slen, raw, bytes(flipped))
    src = _source(S, store=store)
    images = _images(S.m, S.nbuf, S.sl)
    for verify in ((False,) if variant == "lz4" else (True, False)):
        ix = HipHashesMap(1 << 12)
        D = SimpleNamespace(ix=ix, wr=_writer(ix, "raw"), hl=32, sl=S.sl, key=None, e=S.e)
        imp = _importer(D, engine=S.e)
        fmap = torch.full((S.nbuf * S.sl,), 0xEE, dtype=torch.uint8, device="cuda")
        want, res, arcs = _import_and_check(imp, src, srcm, images, list(range(S.nbuf)), [L] * S.nbuf, fmap, S.sl, 32, 0,
                                            PB, verify=verify)
        bit = XM.EFETCH if variant == "lz4" else XM.EHASH
        if variant == "lz4" or verify:
            assert want.status == [bit if s in users else 0 for s in range(S.nbuf)]
            assert ix.get(bad_pair[0]) == -1  # the destination does not hold that fingerprint
            for s in users:
                assert _images(fmap, S.nbuf, S.sl)[s] == b"\xee" * S.sl  # the rejected destinations keep their bytes
        else:
            assert want.status == [0] * S.nbuf and ix.get(bad_pair[0]) >= PB
            got = _read(D, fmap, S.nbuf, arcs.store, arcs.directory(), PB, None)
            b, at = next((b, q[3]) for b in users for q in _pairs_of(S, b) if q[1] == bad_pair[1])
            assert got[b, at + raw // 2] == S.host[b, at + raw // 2] ^ 0x40  # imported as it was stored
        _all_equal(ix, fmap, S.nbuf, S.sl, 32)
        imp.destroy()
        _close(D)
    _close(S)


@pytest.mark.gpu
def test_gpu_extents():
    """The source file is a copy_extents of another file shifted by 12 345 bytes: pairs with offset
    != 0 and nlen < len.  The import fetches whole stored chunks and reads back the same bytes."""
    torch = pytest.importorskip("torch")
    from sdfs_amd import copy_extents, split_extent
    from sdfs_amd.index import HipHashesMap
    from sdfs_amd.read import parse_map_slots

    S = _volume("lz4", cap=1 << 13)
    srcm = _source_model(S)
    shifted = torch.zeros_like(S.m)
    segs = split_extent(0, 12345, (S.nbuf - 1) * L, L)
    _, status, seg_status, info = copy_extents(S.m, shifted, S.nbuf, S.nbuf, S.sl, segs, index=S.ix, chunk_length=L)
    torch.cuda.synchronize()
    assert info.written and not seg_status.any()
    ok = [s for s in range(S.nbuf) if int(status[s].item()) == 0]
    assert len(ok) >= S.nbuf - 1  # a slot whose merged list overflowed would keep its old (empty) image
    pp = parse_map_slots(shifted, S.nbuf, S.sl, 32)
    torch.cuda.synchronize()
    assert (pp.offset != 0).any() and (pp.nlen < pp.len).any()
    want_bytes = _read(S, shifted, S.nbuf, S.arcs.store, S.arcs.directory(), S.pos_base, None)
    ix = HipHashesMap(1 << 13)
    D = SimpleNamespace(ix=ix, wr=_writer(ix, "lz4"), hl=32, sl=S.sl, key=None, e=S.e)
    imp = _importer(D)
    fmap = torch.zeros_like(shifted)
    want, res, arcs = _import_and_check(imp, _source(S), srcm, _images(shifted, S.nbuf, S.sl), list(range(S.nbuf)),
                                        [L] * S.nbuf, fmap, S.sl, 32, 0, 77)
    assert want.status == [0] * S.nbuf
    got = _read(D, fmap, S.nbuf, arcs.store, arcs.directory(), 77, None)
    assert (got == want_bytes).all()
    # each fetched chunk is the whole stored chunk
    chunks, plan = arcs.extra["chunks"].cpu().numpy(), arcs.extra["plan"]
    offs, flen = plan["dst_off"][: len(want.fetches)].tolist(), arcs.extra["fetch_len"].tolist()
    for f, k in enumerate(want.fetches):
        assert flen[f] == srcm.entries[k][1] and chunks[offs[f]: offs[f] + flen[f]].tobytes() == srcm.entries[k][2], f
    imp.destroy()
    _close(S, D)


@pytest.mark.gpu
def test_gpu_all_or_nothing_across_waves():
    """One slot of 2 * 256 + 1 pairs that reuse three stored chunks at ascending pos; its only
    EMISSING pair is the last, in the third wave of the layout."""
    torch = pytest.importorskip("torch")
    from sdfs_amd.index import HipHashesMap

    S = _volume("raw")
    srcm = _source_model(S)
    cl = 1 << 20
    big = 2 * 256 + 1
    sb = 13 + big * 56
    p0 = _pairs_of(S, 0)[:3]
    pairs = [(p0[i % 3][0], p0[i % 3][1], p0[i % 3][2], i * 100, 0, 50) for i in range(big)]
    broken = pairs[:-1] + [(pairs[-1][0], S.pos_base + len(srcm.entries)) + pairs[-1][2:]]
    ix = HipHashesMap(1 << 12)
    D = SimpleNamespace(ix=ix, wr=_writer(ix, "raw"), hl=32, sl=sb, key=None, e=S.e)
    imp = _importer(D, cl=cl)
    fmap = torch.zeros(2 * sb, dtype=torch.uint8, device="cuda")
    before = _export(ix)
    want, res, arcs = _import_and_check(imp, _source(S), srcm, [R.build_image(broken)], [1], [cl], fmap, sb, 32, 0, PB)
    assert want.status == [XM.EMISSING] and want.req_missed == [1] and want.counts[0] == 0 and res.records == 0
    assert _export(ix) == before == [] and not fmap.any()
    want, res, arcs = _import_and_check(imp, _source(S), srcm, [R.build_image(pairs)], [1], [cl], fmap, sb, 32, 0, PB)
    assert want.status == [0] and want.counts[0] == big and want.counts[2] == 3
    assert sum(r for _, _, r in _export(ix)) == big and len(_export(ix)) == 3
    imp.destroy()
    _close(S, D)


@pytest.mark.gpu
def test_gpu_importing_twice_onto_the_same_destinations():
    torch = pytest.importorskip("torch")
    from sdfs_amd.index import HipHashesMap

    S = _volume("lz4")
    srcm = _source_model(S)
    ix = HipHashesMap(1 << 12)
    D = SimpleNamespace(ix=ix, wr=_writer(ix, "lz4"), hl=32, sl=S.sl, key=None, e=S.e)
    imp = _importer(D)
    fmap = torch.zeros(S.nbuf * S.sl, dtype=torch.uint8, device="cuda")
    images, dests, lens = _images(S.m, S.nbuf, S.sl), list(range(S.nbuf)), [L] * (S.nbuf - 1) + [L - 999]
    w1, r1, _ = _import_and_check(imp, _source(S), srcm, images, dests, lens, fmap, S.sl, 32, 0, 500)
    after_first = _export(ix)
    flen = w1.file_len
    assert flen == S.nbuf * L - 999 and w1.counts[6] == w1.counts[0]
    # again, and then the now-native images themselves: nothing to fetch, nothing new, nothing to rewrite
    w2, r2, a2 = _import_and_check(imp, _source(S), srcm, images, dests, lens, fmap, S.sl, 32, flen, 9000)
    assert w2.counts[2] == 0 and a2.n_rec == 0 and w2.counts[1] == w2.counts[0] == w1.counts[0]
    native = _images(fmap, S.nbuf, S.sl)
    w3, r3, a3 = _import_and_check(imp, _source(S), srcm, native, dests, lens, fmap, S.sl, 32, flen, 9000)
    assert w3.counts[2] == 0 and a3.n_rec == 0 and w3.counts[6] == 0 and r3.changed == 0
    assert r3.released.counts.tolist()[:3] == [w1.counts[0], 0, 0]  # the replaced slots were released
    assert _export(ix) == after_first and int(r3.file_len.item()) == flen
    _all_equal(ix, fmap, S.nbuf, S.sl, 32)
    imp.destroy()
    _close(S, D)


@pytest.mark.gpu
def test_gpu_map_lz4_in():
    """close_map on the source, import_file_compressed on the destination: the result of the two
    routes test."""
    torch = pytest.importorskip("torch")
    from sdfs_amd import close_map
    from sdfs_amd.index import HipHashesMap
    from sdfs_amd.lz4 import HipLz4Compressor
    from sdfs_amd.lz4_stream import HipLz4BlockStream

    S = _volume("lz4")
    z = HipLz4Compressor()
    codec = HipLz4BlockStream(z)
    image = close_map(codec, S.m, S.nbuf, S.sl)
    assert image.numel() < S.m.numel()
    ix = HipHashesMap(1 << 12)
    D = SimpleNamespace(ix=ix, wr=_writer(ix, "lz4"), hl=32, sl=S.sl, key=None, e=S.e)
    imp = _importer(D)
    fmap, res, arcs = imp.import_file_compressed(codec, image, _source(S), S.sl, S.nbuf * L, PB)
    torch.cuda.synchronize()
    assert not res.status.any() and torch.equal(fmap, S.m) and _export(ix) == _export(S.ix)
    assert (S.arcs.n_arc, S.arcs.n_rec) == (arcs.n_arc, arcs.n_rec)
    for a in range(arcs.n_arc):
        assert S.arcs.image(a) == arcs.image(a) and S.arcs.map_image(a) == arcs.map_image(a), a
    imp.destroy()
    z.destroy()
    _close(S, D)


@pytest.mark.gpu
def test_gpu_a_destination_that_holds_half():
    """The destination has written the source's first four buffers itself (pos_base 0); the import
    goes in at pos_base = its record count and the file reads back through the two ArchiveSets'
    directories concatenated.  The destination's write starts with a buffer of its own, so that
    hashloc 0 — where the read path stops reading a slot (WritableCacheBuffer.java:262-278) — is
    not a chunk of the imported file."""
    torch = pytest.importorskip("torch")
    S = _volume("raw")
    srcm = _source_model(S)
    half = _batch(S.e, nbuf=NBUF // 2 + 1, first_stream=4242)
    half.data.view(NBUF // 2 + 1, L)[1:].copy_(S.batch.data.view(NBUF, L)[: NBUF // 2])
    D = _volume("raw", pos_base=0, batch=half)
    n1 = D.arcs.n_rec
    imp = _importer(D)
    fmap = torch.zeros(S.nbuf * S.sl, dtype=torch.uint8, device="cuda")
    want, res, arcs = _import_and_check(imp, _source(S), srcm, _images(S.m, S.nbuf, S.sl), list(range(S.nbuf)),
                                        [L] * S.nbuf, fmap, S.sl, 32, 0, n1)
    assert want.status == [0] * S.nbuf and 0 < want.counts[1] < want.counts[0] and 0 < want.counts[2] < S.arcs.n_rec
    first_half = {srcm.entries[q[1] - S.pos_base][2] for s in range(NBUF // 2) for q in _pairs_of(S, s)}
    assert want.counts[2] == arcs.n_rec == S.arcs.n_rec - len(first_half)
    store = torch.cat([D.arcs.store, arcs.store])
    off = torch.cat([D.arcs.store_off, arcs.store_off + D.arcs.store.numel()])
    directory = (off, torch.cat([D.arcs.store_len, arcs.store_len]), torch.cat([D.arcs.raw_len, arcs.raw_len]))
    got = _read(D, fmap, S.nbuf, store, directory, 0, None)
    assert (got == S.host).all()
    # the destination's own file and the imported one together account for every count
    both = torch.cat([D.m, fmap])
    _all_equal(D.ix, both, D.nbuf + S.nbuf, S.sl, 32)
    imp.destroy()
    _close(S, D)
