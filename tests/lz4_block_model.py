"""A plain model of the LZ4 block format as the device decoders accept it — TEST INFRASTRUCTURE.

``decode`` is the rule set of sdfs_amd/csrc/lz4_decode.h (the lane decoder) and of
``decompress_block`` in lz4_kernels.hip (the wave decoder), written one step at a time with no
fast path: a block is a run of sequences ``[token][literal length bytes][literals][offset LE16]
[match length bytes]``; the only accepted end is ``ip == n`` right after a literal run.  There are
no end-of-block restrictions beyond that (liblz4's decoder has some, so it is not the reference
for verdicts; where both accept, the bytes are equal: tests/test_lz4_model.py).

``decode_record`` is the framed rule of ``lz4_decompress_kernel`` (putChunk records), ``emit``
writes a block from an explicit sequence list, and the case builders at the end make the record
sets that the CPU tests count and the GPU tests (tests/test_lz4_decode.py) decode on both routes.
"""
from __future__ import annotations

import ctypes
import struct

import numpy as np

OK = "OK"
INPUT_END = "INPUT_END"            # a token, a length byte or an offset is wanted at or past n
LIT_PAST_INPUT = "LIT_PAST_INPUT"  # a literal run goes past the input
LIT_PAST_CAP = "LIT_PAST_CAP"      # a literal run goes past cap
OFF_ZERO = "OFF_ZERO"              # the offset is zero
OFF_BEFORE = "OFF_BEFORE"          # the offset is greater than op
MATCH_PAST_CAP = "MATCH_PAST_CAP"  # a match goes past cap
SHORT = "SHORT"                    # framed: bad header, or the block decodes to other than nz
REASONS = (INPUT_END, LIT_PAST_INPUT, LIT_PAST_CAP, OFF_ZERO, OFF_BEFORE, MATCH_PAST_CAP, SHORT)


def decode(block, cap: int):
    """(bytes, OK) when the block decodes within cap bytes, else the reason (a string)."""
    src = bytes(block)
    n = len(src)
    out = bytearray()
    ip = 0
    while True:
        if ip >= n:
            return INPUT_END
        token = src[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            while True:
                if ip >= n:
                    return INPUT_END
                b = src[ip]
                ip += 1
                lit += b
                if b != 255:
                    break
        if ip + lit > n:
            return LIT_PAST_INPUT
        if len(out) + lit > cap:
            return LIT_PAST_CAP
        out += src[ip:ip + lit]
        ip += lit
        if ip == n:
            return bytes(out), OK
        if ip + 2 > n:
            return INPUT_END
        off = src[ip] | src[ip + 1] << 8
        ip += 2
        if off == 0:
            return OFF_ZERO
        if off > len(out):
            return OFF_BEFORE
        ml = token & 15
        if ml == 15:
            while True:
                if ip >= n:
                    return INPUT_END
                b = src[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        ml += 4
        if len(out) + ml > cap:
            return MATCH_PAST_CAP
        start = len(out) - off
        if off >= ml:
            out += out[start:start + ml]
        else:  # overlapping: byte k of the match is byte k % off of the last off bytes
            period = bytes(out[start:])
            out += (period * (ml // off + 1))[:ml]


def decode_record(record, cap: int):
    """The framed rule: [BE32 nz][payload]; nz > 0 = a block of exactly nz <= cap bytes, else the
    payload is the raw chunk (n - 4 <= cap bytes)."""
    rec = bytes(record)
    if len(rec) < 4:
        return SHORT
    nz = struct.unpack(">i", rec[:4])[0]
    if nz > 0:
        if nz > cap:
            return SHORT
        r = decode(rec[4:], nz)
        if isinstance(r, str):
            return r
        return r if len(r[0]) == nz else SHORT
    if len(rec) - 4 > cap:
        return LIT_PAST_CAP
    return rec[4:], OK


def reason_of(result) -> str:
    return result if isinstance(result, str) else OK


def _length_bytes(v: int) -> bytes:
    return b"\xff" * (v // 255) + bytes([v % 255])


def emit(sequences, last_literals=b"") -> bytes:
    """The block of (literals, offset, match_len) sequences followed by a last literal run.
    Nothing is checked beyond the field ranges: a test may ask for any offset."""
    out = bytearray()
    for lits, off, ml in sequences:
        lits = bytes(lits)
        assert ml >= 4 and 0 <= off <= 65535
        ll, m = len(lits), ml - 4
        out.append(min(ll, 15) << 4 | min(m, 15))
        if ll >= 15:
            out += _length_bytes(ll - 15)
        out += lits
        out += struct.pack("<H", off)
        if m >= 15:
            out += _length_bytes(m - 15)
    lits = bytes(last_literals)
    out.append(min(len(lits), 15) << 4)
    if len(lits) >= 15:
        out += _length_bytes(len(lits) - 15)
    out += lits
    return bytes(out)


# ------------------------------------------------------------------------------------------
# record sets (deterministic: every generator is seeded)
# ------------------------------------------------------------------------------------------
LIT_RUNS = [0, 1, 14, 15, 16, 17, 269, 270, 271, 3087, 3088, 4095, 4096, 4097, 5000]
OFFSETS = [1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 255, 256, 4095, 65535]
MATCH_LENS = [4, 5, 7, 8, 9, 15, 18, 19, 20, 63, 64, 65, 128, 273, 274, 275, 4100, 70000]


def _rnd(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _true_len(block: bytes) -> int:
    r = decode(block, 1 << 30)
    assert not isinstance(r, str), r
    return len(r[0])


def _exact(target: int, seed: int) -> bytes:
    """A valid block of exactly `target` compressed bytes with long literal runs and matches."""
    for d in range(40):
        seqs = [(_rnd(1000 + d, seed), 7, 300), (_rnd(1800, seed + 1), 1500, 64), (b"", 3, 21)]
        room = target - len(emit(seqs, b""))
        for ll in range(max(room - 8, 0), room + 1):
            blk = emit(seqs, _rnd(ll, seed + 2))
            if len(blk) == target:
                return blk
    raise AssertionError(target)


def _routing(cap: int, n: int, seed: int) -> bytes:
    """A valid block of n compressed bytes that decodes to exactly cap bytes."""
    for b in range(0, 30):
        for a in range(max(n - 40 - b, 0), n):
            m = cap - a - b
            blk = emit([(_rnd(a, seed), 4, m)], _rnd(b, seed + 1))
            if len(blk) == n:
                return blk
    raise AssertionError((cap, n))


def edge_cases(wave_only: bool = True):
    """Section 3a: (block, cap, tag, align) with align = None or the input offset mod 4 wanted.
    wave_only=False leaves out the four items that concern the wave decoder alone."""
    cases = []

    def add(block, cap=None, tag="", align=None):
        cases.append((block, _true_len(block) if cap is None else cap, tag, align))

    s = 1000
    for ll in LIT_RUNS:  # a run before a match, and the block's last run
        s += 3
        add(emit([(_rnd(40, s), 8, 8), (_rnd(ll, s + 1), 16, 6)], _rnd(5, s + 2)), tag=f"lit{ll}")
        add(emit([], _rnd(ll, s)), tag=f"lastlit{ll}")
        add(emit([(_rnd(9, s), 9, 4)], _rnd(ll, s + 1)), tag=f"match+lastlit{ll}")
    for off in OFFSETS:
        for ml in MATCH_LENS:
            if ml == 70000 and off not in (1, 8, 65535):
                continue
            if ml == 4100 and off not in (1, 3, 7, 8, 64, 4095):
                continue
            if off == 65535 and ml not in (4, 64, 70000):
                continue
            s += 1
            for pre in (off, off + 3):  # the match starts at the oldest byte, or 3 after it
                add(emit([(_rnd(pre, s), off, ml)], _rnd(5, s + 7)), tag=f"off{off}ml{ml}")
    # a long match that does not overlap its source (the wave decoder's four-in-flight copy
    # reading bytes the wave itself wrote)
    for off, ml in ((5000, 3087), (5000, 3088), (5000, 4100), (65535, 4100)):
        s += 1
        add(emit([(_rnd(off + 1, s), off, ml)], _rnd(2, s + 1)), tag=f"disjoint{off}ml{ml}")
    # the last match ends at cap - j: j trailing literals (cap = the true length), or no literals
    # and a cap that is j larger (unframed: accepted short of cap; framed: nz != length)
    for off, ml, lit in ((12, 20, 14), (12, 9, 3), (3, 20, 14), (8, 4, 14), (5, 9, 3), (16, 24, 14), (1, 4, 0)):
        for j in range(17):
            s += 1
            pre = [(_rnd(30, s), 10, 5)]
            add(emit(pre + [(_rnd(lit, s + 1), off, ml)], _rnd(j, s + 2)), tag=f"end-j{j}")
            blk = emit(pre + [(_rnd(lit, s + 1), off, ml)], b"")
            add(blk, cap=_true_len(blk) + j, tag=f"cap+{j}")
            if j:
                add(blk, cap=_true_len(blk) - min(j, 8), tag=f"cap-{min(j, 8)}")
    # the input left at the start of the second sequence is 4 .. 35 bytes; the block ends on
    # 0 .. 16 literals
    for a in range(15):
        for b in range(17):
            s += 1
            add(emit([(_rnd(20, s), 8, 8), (_rnd(a, s + 1), 5, 6)], _rnd(b, s + 2)), tag=f"left{a}+{b}")
    for b in range(6):  # zero-literal sequences back to back
        s += 1
        add(emit([(_rnd(16, s), 3, 7), (b"", 1, 30), (b"", 7, 100), (b"", 9, 5), (b"", 64, 64)], _rnd(b, s + 1)),
            tag=f"zerolit{b}")
    if wave_only:
        for n in (4095, 4096, 4097):  # the LDS stage's edge (framed: + 4 header bytes)
            add(_exact(n, 7000 + n), tag=f"stage{n}")
        for al in (1, 2, 3):
            add(_exact(4092, 7100 + al), tag=f"align{al}", align=al)
            add(emit([], _rnd(4091 - 16, 7200 + al)), tag=f"litalign{al}", align=al)
        for cap, n in ((1600, 1500), (1600, 1499), (1600, 1501), (160, 150), (160, 149), (160, 151)):
            add(_routing(cap, n, 7300 + n), cap=cap, tag=f"route{n}/{cap}")
    return cases


def _sys_encoders():
    """name -> block encoder of the system liblz4, {} without one."""
    from oracle import lz4_oracle as Z

    L = Z.system_lz4()
    enc = {}
    if L is None:
        return enc

    def fast(acc):
        f = L.LZ4_compress_fast
        f.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        f.restype = ctypes.c_int

        def run(d):
            out = ctypes.create_string_buffer(Z.bound(len(d)))
            k = f(bytes(d), out, len(d), len(out), acc)
            return out.raw[:k]
        return run

    for acc in (1, 5, 9):
        enc[f"fast{acc}"] = fast(acc)
    hc = getattr(L, "LZ4_compress_HC", None)
    if hc is not None:
        hc.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        hc.restype = ctypes.c_int

        def run_hc(d):
            out = ctypes.create_string_buffer(Z.bound(len(d)))
            k = hc(bytes(d), out, len(d), len(out), 9)
            return out.raw[:k]
        enc["hc9"] = run_hc
    return enc


FOREIGN_LENS = [0, 1, 5, 12, 13, 17, 64, 200, 620, 1500, 4200]
_cache = {}


def _inputs():
    from oracle import cdc_oracle as C
    from oracle import lz4_oracle as Z

    out = []
    for i, n in enumerate(FOREIGN_LENS):
        out += [C.synth(3, 500 + i, 0, n).tobytes(), bytes(n), Z.text_like(3, 500 + i, n).tobytes(),
                Z.mixed(3, 500 + i, n).tobytes(), (np.arange(n) % 251).astype(np.uint8).tobytes(),
                (Z.text_like(3, 600 + i, max(n // 3, 1)).tobytes() * 4)[:n]]
    out += [Z.mixed(3, 700, 70000).tobytes(), Z.text_like(3, 701, 20000).tobytes()]
    return out


def foreign_blocks():
    """Section 3b: [(encoder name, data, block)] — the oracle's two parses and, with a system
    liblz4, LZ4_compress_fast at acceleration 1, 5, 9 and LZ4_compress_HC at level 9."""
    if "foreign" not in _cache:
        from oracle import lz4_oracle as Z

        enc = {"r123": lambda d: Z.compress(d, Z.R123), "v19": lambda d: Z.compress(d, Z.V19)}
        enc.update(_sys_encoders())
        _cache["foreign"] = [(name, d, f(d)) for d in _inputs() for name, f in enc.items()]
    return _cache["foreign"]


N_RANDOM_MUTATIONS = 3000


def mutated_set():
    """Section 3c: [(block, cap)] — bit flips, truncations and overwrites of 20 .. 620 byte
    blocks with caps below, at and above the true length, then targeted damage (an offset field
    set to zero, a cap cut by 1 .. 8) so that no reason's count depends on luck."""
    if "mutated" in _cache:
        return _cache["mutated"]
    base = [(b, len(d)) for _, d, b in foreign_blocks() if 20 <= len(b) <= 620]
    assert len(base) >= 40
    rng = np.random.default_rng(20)
    out = []
    for i in range(N_RANDOM_MUTATIONS):
        blk, n = base[i % len(base)]
        b = bytearray(blk)
        kind = int(rng.integers(0, 4))
        if kind == 0:
            for _ in range(int(rng.integers(1, 3))):
                b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
        elif kind == 1:
            b = b[:int(rng.integers(1, len(b)))]
        elif kind == 2:
            p = int(rng.integers(0, len(b)))
            k = int(rng.integers(1, 5))
            b[p:p + k] = bytes(rng.integers(0, 256, min(k, len(b) - p), dtype=np.uint8))
        # kind 3: the block as it is, under the cap below
        cap = max(n + int(rng.choice([-8, -3, -1, 0, 0, 0, 0, 1, 5, 20])), 0)
        out.append((bytes(b), cap))
    # targeted: walk the sequences of a valid block to find its offset fields
    for k, (blk, n) in enumerate(base):
        fields, ip = [], 0
        while True:
            token = blk[ip]
            ip += 1
            lit = token >> 4
            if lit == 15:
                while True:
                    lit += blk[ip]
                    ip += 1
                    if blk[ip - 1] != 255:
                        break
            ip += lit
            if ip == len(blk):
                break
            fields.append(ip)
            ip += 2
            if (token & 15) == 15:
                while True:
                    ip += 1
                    if blk[ip - 1] != 255:
                        break
        if fields:
            p = fields[k % len(fields)]
            out.append((blk[:p] + b"\0\0" + blk[p + 2:], n))
        out.append((blk, max(n - 1 - k % 8, 0)))
    _cache["mutated"] = out
    return out


def framed(block: bytes, nz: int) -> bytes:
    return struct.pack(">i", nz) + bytes(block)
