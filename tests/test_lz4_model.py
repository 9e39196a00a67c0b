"""The plain LZ4 block model (tests/lz4_block_model.py) against liblz4's LZ4_decompress_safe, and
the record sets the GPU decode tests use (tests/test_lz4_decode.py), counted here so that a thin
set fails without a GPU.  liblz4 is the reference for BYTES wherever both accept; it is not the
reference for verdicts (its decoder also enforces the encoder's end-of-block rules in places),
so verdict disagreements are counted and printed, not asserted."""
import collections
import ctypes

import pytest

from oracle import lz4_oracle as Z
from tests import lz4_block_model as M

needs_liblz4 = pytest.mark.skipif(Z.system_lz4() is None, reason="no system liblz4 to compare with")


def _safe(block: bytes, cap: int):
    """LZ4_decompress_safe: the decoded bytes, or None when it rejects."""
    out = ctypes.create_string_buffer(max(cap, 1))
    k = Z.system_lz4().LZ4_decompress_safe(bytes(block), out, len(block), cap)
    return None if k < 0 else out.raw[:k]


def test_emit_and_decode_known_blocks():
    assert M.emit([], b"hello") == b"\x50hello" and M.emit([]) == b"\x00"
    blk = M.emit([(b"abc", 3, 9)], b"xyz")
    assert blk == b"\x35abc\x03\x00\x30xyz"
    assert M.decode(blk, 15) == (b"abcabcabcabcxyz", M.OK)
    assert M.decode(blk, 14) == M.LIT_PAST_CAP and M.decode(blk, 11) == M.MATCH_PAST_CAP
    assert M.decode(blk[:-1], 15) == M.LIT_PAST_INPUT and M.decode(blk[:5], 15) == M.INPUT_END
    assert M.decode(b"", 5) == M.INPUT_END and M.decode(blk[:4], 15) == (b"abc", M.OK)
    assert M.decode(b"\x35abc\x00\x00\x30xyz", 15) == M.OFF_ZERO
    assert M.decode(b"\x35abc\x04\x00\x30xyz", 15) == M.OFF_BEFORE
    assert M.decode(b"\xf0" + b"\xff", 1 << 20) == M.INPUT_END
    long = M.emit([(b"q" * 300, 300, 4 + 15 + 255 + 7)], b"")
    assert M.decode(long, 1 << 20) == (b"q" * (300 + 281), M.OK)
    # a block may end on any number of literals, right after a match included
    assert M.decode(M.emit([(b"abcd", 4, 4)], b""), 8) == (b"abcdabcd", M.OK)
    assert M.decode_record(M.framed(blk, 15), 15) == (b"abcabcabcabcxyz", M.OK)
    assert M.decode_record(M.framed(blk, 16), 16) == M.SHORT and M.decode_record(M.framed(blk, 15), 14) == M.SHORT
    assert M.decode_record(M.framed(blk, 14), 15) == M.LIT_PAST_CAP
    assert M.decode_record(M.framed(b"raw", -1), 3) == (b"raw", M.OK) and M.decode_record(b"\0\0\0", 9) == M.SHORT
    assert M.decode_record(M.framed(b"raw", 0), 2) == M.LIT_PAST_CAP


@needs_liblz4
def test_model_equals_liblz4_on_unmutated_blocks():
    """Every block of the oracle's two parses, of LZ4_compress_fast (acceleration 1, 5, 9) and of
    LZ4_compress_HC (level 9): the model and LZ4_decompress_safe give the input back."""
    blocks = M.foreign_blocks()
    names = {name for name, _, _ in blocks}
    assert {"r123", "v19", "fast1", "fast5", "fast9"} <= names
    if "hc9" not in names:
        print("LZ4_compress_HC missing from the system liblz4: HC cases not run")
    for name, d, blk in blocks:
        for cap in (len(d), len(d) + 7):
            assert M.decode(blk, cap) == (d, M.OK), (name, len(d))
            assert _safe(blk, cap) == d, (name, len(d))


def test_edge_blocks_decode_and_reach_the_listed_shapes():
    cases = M.edge_cases()
    tags = {t for _, _, t, _ in cases}
    for ll in M.LIT_RUNS:
        assert f"lit{ll}" in tags and f"lastlit{ll}" in tags
    for off in M.OFFSETS:
        assert any(t.startswith(f"off{off}ml") for t in tags), off
    for ml in M.MATCH_LENS:
        assert any(t.endswith(f"ml{ml}") for t in tags), ml
    assert sum(len(b) >= 65535 for b, _, _, _ in cases) <= 16  # the large ones stay a handful
    for n in (4095, 4096, 4097):
        assert any(len(b) == n for b, _, t, _ in cases if t.startswith("stage"))
    assert sum(len(b) * 16 == cap * 15 for b, cap, t, _ in cases if t.startswith("route")) == 2
    ok = 0
    for blk, cap, tag, _ in cases:
        r = M.decode(blk, cap)
        if tag.startswith("cap-"):
            assert r in (M.MATCH_PAST_CAP, M.LIT_PAST_CAP), tag
        else:
            assert not isinstance(r, str), (tag, r)
            ok += 1
            if Z.system_lz4() is not None:
                got = _safe(blk, cap)
                assert got is None or got == r[0], tag
    assert ok >= 800


def test_mutated_set_bytes_equal_liblz4_and_reason_floors():
    """The damaged set of the GPU tests: wherever the model and liblz4 both accept, the bytes are
    equal; every reason (SHORT, the framed one, included) occurs at least 20 times and at least
    200 records are accepted, in both forms."""
    muts = M.mutated_set()
    assert len(muts) >= M.N_RANDOM_MUTATIONS
    have_lib = Z.system_lz4() is not None  # without one only the floors are checked
    both = only_model = only_lib = 0
    plain, rec = collections.Counter(), collections.Counter()
    for blk, cap in muts:
        r = M.decode(blk, cap)
        s = _safe(blk, cap) if have_lib else None
        plain[M.reason_of(r)] += 1
        rec[M.reason_of(M.decode_record(M.framed(blk, cap), cap))] += 1
        if not isinstance(r, str) and s is not None:
            assert r[0] == s
            both += 1
        elif not isinstance(r, str):
            only_model += 1
        elif s is not None:
            only_lib += 1
    print(f"mutated set: {len(muts)} records; both accept {both}, only the model {only_model}, "
          f"only liblz4 {only_lib}; unframed {dict(plain)}; framed {dict(rec)}")
    for reason in M.REASONS:
        assert rec[reason] >= 20, (reason, dict(rec))
        if reason != M.SHORT:
            assert plain[reason] >= 20, (reason, dict(plain))
    assert plain[M.OK] >= 200 and rec[M.OK] >= 200
