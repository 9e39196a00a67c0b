"""Pure-Python model of lz4-java 1.3.0's LZ4Block stream (LZ4BlockOutputStream / LZ4BlockInputStream,
what CompressionUtils.compressFile / decompressFile run over a map file) — TEST INFRASTRUCTURE ONLY.

Restated from the library's sources: the jar is not here, so nothing pins these bytes against the
Java classes themselves.  XXH32 is checked against the published vectors, the ``xxhash`` module and
liblz4's frame checksum (tests/test_lz4_stream.py); the LZ4 blocks come from ``oracle.lz4_oracle``.
"""
from __future__ import annotations

import struct

from oracle import lz4_oracle as Z

MAGIC = b"LZ4Block"
HEADER = 21
SEED = 0x9747B28C
RAW, LZ4 = 0x10, 0x20
MIN_BLOCK, MAX_BLOCK = 64, 1 << 25
TRUNCATED, MAGIC_BAD, HEADER_BAD, DECODE, CHECKSUM = 1, 2, 4, 8, 16
FLAG_NAMES = {TRUNCATED: "TRUNCATED", MAGIC_BAD: "MAGIC", HEADER_BAD: "HEADER", DECODE: "DECODE", CHECKSUM: "CHECKSUM"}

_M = 0xFFFFFFFF
_P1, _P2, _P3, _P4, _P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393


def _rotl(x: int, r: int) -> int:
    return ((x << r) | (x >> (32 - r))) & _M


def xxh32(data, seed: int = 0) -> int:
    data = bytes(data)
    n = len(data)
    p = 0
    if n >= 16:
        v = [(seed + _P1 + _P2) & _M, (seed + _P2) & _M, seed & _M, (seed - _P1) & _M]
        words = struct.unpack_from("<%dI" % (n // 16 * 4), data)
        for k in range(0, len(words), 4):
            for q in range(4):
                v[q] = (_rotl((v[q] + words[k + q] * _P2) & _M, 13) * _P1) & _M
        p = n // 16 * 16
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M
    else:
        h = (seed + _P5) & _M
    h = (h + n) & _M
    while p + 4 <= n:
        h = (_rotl((h + struct.unpack_from("<I", data, p)[0] * _P3) & _M, 17) * _P4) & _M
        p += 4
    while p < n:
        h = (_rotl((h + data[p] * _P5) & _M, 11) * _P1) & _M
        p += 1
    h ^= h >> 15
    h = (h * _P2) & _M
    h ^= h >> 13
    h = (h * _P3) & _M
    h ^= h >> 16
    return h


def level(block_size: int) -> int:
    """LZ4BlockOutputStream.compressionLevel - COMPRESSION_LEVEL_BASE."""
    if not MIN_BLOCK <= block_size <= MAX_BLOCK:
        raise ValueError("blockSize")
    return max(0, (block_size - 1).bit_length() - 10)


def bound(n: int, block_size: int) -> int:
    return n + HEADER * (-(-n // block_size) + 1)


def check_of(block: bytes) -> int:
    """StreamingXXHash32.asChecksum().getValue(): 28 bits."""
    return xxh32(block, SEED) & 0x0FFFFFFF


def header(token: int, clen: int, olen: int, check: int) -> bytes:
    return MAGIC + struct.pack("<BIII", token, clen & _M, olen & _M, check & _M)


def end_mark(block_size: int) -> bytes:
    return header(RAW | level(block_size), 0, 0, 0)


def write(data, block_size: int = 65536, mode: int = Z.R123) -> bytes:
    """LZ4BlockOutputStream(out, block_size, compressor): write(data); close()."""
    data = bytes(data)
    lv = level(block_size)
    out = bytearray()
    for at in range(0, len(data), block_size):
        blk = data[at: at + block_size]
        c = Z.compress(blk, mode)
        if len(c) >= len(blk):
            out += header(RAW | lv, len(blk), len(blk), check_of(blk)) + blk
        else:
            out += header(LZ4 | lv, len(c), len(blk), check_of(blk)) + c
    out += end_mark(block_size)
    return bytes(out)


def _i32(b: bytes, at: int) -> int:
    return struct.unpack_from("<i", b, at)[0]


def read(stream):
    """LZ4BlockInputStream over ``stream`` read to its end mark.  Returns a dict: status (the flag
    of the first bad block, where Java throws), n_blocks and decoded_len of the blocks located
    before it, consumed (through the end mark; else the bad block's position), data (the decoded
    bytes when status is 0, else None; a located block that fails to decode or verify comes before
    the block the header walk stopped at, so its flag is the status then) and blocks (payload offset, compressedLen, originalLen,
    method, check)."""
    s = bytes(stream)
    pos, blocks, status, done = 0, [], 0, False
    while True:
        if len(s) - pos < HEADER:
            status = TRUNCATED
            break
        h = s[pos: pos + HEADER]
        if h[:8] != MAGIC:
            status = MAGIC_BAD
            break
        token = h[8]
        method, lv = token & 0xF0, token & 0x0F
        clen, olen = _i32(h, 9), _i32(h, 13)
        check = struct.unpack_from("<I", h, 17)[0]
        if method not in (RAW, LZ4):
            status = HEADER_BAD
            break
        if (olen > 1 << (10 + lv) or olen < 0 or clen < 0 or (olen == 0) != (clen == 0)
                or (method == RAW and olen != clen)):
            status = HEADER_BAD
            break
        if olen == 0:
            if check != 0:
                status = HEADER_BAD
                break
            pos += HEADER
            done = True
            break
        if clen > len(s) - pos - HEADER:
            status = TRUNCATED
            break
        blocks.append((pos + HEADER, clen, olen, method, check))
        pos += HEADER + clen
    res = {"status": status, "n_blocks": len(blocks), "decoded_len": sum(b[2] for b in blocks), "consumed": pos,
           "blocks": blocks, "data": None}
    # Java decodes block k before it reads block k + 1's header: a located block that fails comes
    # before the block the walk stopped at
    out = bytearray()
    for at, clen, olen, method, check in blocks:
        payload = s[at: at + clen]
        if method == RAW:
            blk = payload
        else:
            try:  # the bounded rule: exactly olen bytes out of exactly clen bytes, never past either
                blk = Z.decompress(payload, olen)
            except ValueError:
                res["status"] = DECODE
                return res
        if check_of(blk) != check:  # the whole int: a stored value with a top bit set never matches
            res["status"] = CHECKSUM
            return res
        out += blk
    if done:
        res["data"] = bytes(out)
    return res


def flag_names(status: int) -> str:
    return "|".join(n for b, n in FLAG_NAMES.items() if status & b) or "OK"
