"""Both routes of sdfs_cdc_lz4_decompress_device against the plain model (tests/lz4_block_model.py).

The call runs the wave kernel alone below ``sdfs_cdc_lz4_hybrid_min_items`` items of CAPACITY and
the split decode (one lane per compressible block, waves for the rest) from there up; the device
count decides what is touched.  So one set of K records is decoded twice: with arrays of length
K (wave route) and with arrays padded to the threshold with zero-length entries and count = K
(split route).  Records: the structural edges of the block format (``M.edge_cases``), blocks of
foreign encoders (``M.foreign_blocks``) and damaged blocks (``M.mutated_set``; the CPU test
tests/test_lz4_model.py counts its reasons), bare and as putChunk records.  A decoder's contract
on damaged input is to flag it: dst_len = -1, nothing written outside the record's own extent.
"""
import numpy as np
import pytest

from oracle import lz4_oracle as Z
from tests import lz4_block_model as M
from tests.test_lz4 import comp

SENTINEL = 0x5EA5EA5
FILL = 0xA5


def _records(framed: bool):
    """[(record bytes, dst_cap, input offset mod 4 wanted or None)] of one form."""
    recs = []
    for i, (blk, cap, _, align) in enumerate(M.edge_cases()):
        recs.append((M.framed(blk, cap), cap + (0, 0, 3)[i % 3], align) if framed else (blk, cap, align))
    for i, (_, d, blk) in enumerate(M.foreign_blocks()):
        recs.append((M.framed(blk, len(d)), len(d) + (0, 3)[i % 2], None) if framed else
                    (blk, len(d) + (0, 5)[i % 2], None))
    for blk, cap in M.mutated_set():
        recs.append((M.framed(blk, cap), cap, None) if framed else (blk, cap, None))
    if framed:
        blk = M.emit([(b"0123456789", 4, 30)], b"xyz")  # decodes to 43 bytes
        raw = bytes(range(40))
        recs += [(M.framed(blk, nz), 43, None) for nz in (42, 44, 43, 1, 1000, 2**31 - 1)]  # nz -1, +1, above cap
        recs += [(M.framed(blk, 43), cap, None) for cap in (42, 0)]
        recs += [(M.framed(raw, nz), cap, None) for nz in (0, -1, -40, -2**31) for cap in (40, 41, 39, 0)]
        recs += [(M.framed(b"", nz), 8, None) for nz in (0, -1, 1)]
        recs += [(bytes(n), 16, None) for n in range(4)] + [(b"\x7f\xff\xff", 16, None)]  # 0 .. 3 bytes
    else:
        recs += [(b"", cap, None) for cap in (0, 1, 64, 65536)]  # what the stream reader feeds for RAW blocks
        recs += [(b"\x00", cap, None) for cap in (0, 1)]
    return recs


_EXPECT = {}


def _expected(framed: bool):
    """The records and the model's verdicts, computed once per form."""
    if framed not in _EXPECT:
        recs = _records(framed)
        want = [M.decode_record(r, cap) if framed else M.decode(r, cap) for r, cap, _ in recs]
        _EXPECT[framed] = (recs, want)
    return _EXPECT[framed]


def _layout(recs):
    """Inputs at unaligned offsets with gaps of 1 .. 5 bytes (or at the offset mod 4 a record
    asks for); output extents dst_cap wide with odd gaps."""
    src_off, dst_off = [], []
    p, q = 1, 3
    for i, (r, cap, align) in enumerate(recs):
        p += 1 + i % 5
        if align is not None:
            p += (align - p) % 4
        src_off.append(p)
        p += len(r)
        dst_off.append(q)
        q += cap + (1, 3, 5, 7)[i % 4]
    src = np.full(p + 32, 0x3C, np.uint8)
    for o, (r, _, _) in zip(src_off, recs):
        src[o:o + len(r)] = np.frombuffer(r, np.uint8)
    return src, np.array(src_off, np.int64), np.array(dst_off, np.int64), q + 32


def _decode_on_both_routes(framed: bool):
    import torch

    c = comp(Z.R123)
    thr = c.hybrid_min_items()
    recs, want = _expected(framed)
    K = len(recs)
    assert 2000 <= K < thr, (K, thr)
    accepted = sum(not isinstance(w, str) for w in want)
    assert accepted >= 1500 and K - accepted >= 1000, (accepted, K)
    src, src_off, dst_off, out_bytes = _layout(recs)
    src_len = np.array([len(r) for r, _, _ in recs], np.int32)
    caps = np.array([cap for _, cap, _ in recs], np.int32)
    inside = np.zeros(out_bytes, bool)
    for o, cap in zip(dst_off, caps):
        inside[o:o + cap] = True
    dev = torch.device("cuda:0")
    d_src = torch.from_numpy(src).to(dev)
    count = torch.tensor([K], dtype=torch.int32, device=dev)

    def padded(a, n):
        t = torch.zeros(n, dtype=torch.from_numpy(a).dtype, device=dev)
        t[:K] = torch.from_numpy(a).to(dev)
        return t

    for route, n_arr in (("wave", K), ("split", thr)):
        # the capacity decides the route: below the threshold the wave kernel alone, from it up
        # the split decode
        assert (n_arr < thr) == (route == "wave") and n_arr >= K
        out = torch.full((out_bytes,), FILL, dtype=torch.uint8, device=dev)
        dst_len = torch.full((n_arr + 8,), SENTINEL, dtype=torch.int32, device=dev)
        c.decompress_device(d_src, padded(src_off, n_arr), padded(src_len, n_arr), out, padded(dst_off, n_arr),
                            padded(caps, n_arr), dst_len, count=count, framed=framed)
        torch.cuda.synchronize()
        o, got = out.cpu().numpy(), dst_len.cpu().numpy()
        assert (got[K:] == SENTINEL).all(), route
        assert (o[~inside] == FILL).all(), (route, np.flatnonzero((o != FILL) & ~inside)[:8])
        assert np.array_equal(d_src.cpu().numpy(), src), route
        want_len = np.array([-1 if isinstance(w, str) else len(w[0]) for w in want], np.int32)
        bad = np.flatnonzero(got[:K] != want_len)
        assert bad.size == 0, (route, framed, [(int(i), int(got[i]), int(want_len[i]), M.reason_of(want[i]),
                                                 int(src_len[i]), int(caps[i])) for i in bad[:8]])
        for i, w in enumerate(want):
            if not isinstance(w, str):
                a = int(dst_off[i])
                assert o[a:a + len(w[0])].tobytes() == w[0], (route, framed, i, int(src_len[i]), int(caps[i]))


@pytest.mark.gpu
def test_gpu_both_routes_bare_blocks_vs_model():
    """Bare blocks (the stream reader's form): edges, foreign encoders and damage on the wave
    route and on the split route; lengths, bytes, the bytes outside every extent, the entries
    past the count and the input, against the model."""
    _decode_on_both_routes(framed=False)


@pytest.mark.gpu
def test_gpu_both_routes_putchunk_records_vs_model():
    """putChunk records [BE32 nz][block | raw chunk]: the same sets plus header damage (nz off by
    one, zero, negative with raw bytes, above the room) and records of 0 .. 3 bytes."""
    _decode_on_both_routes(framed=True)
