"""Plain-Python model of the read path's rules — TEST INFRASTRUCTURE ONLY.

Restated from the reference, for one write buffer:

* parse: ``SparseDataChunk(byte[], version >= 2)`` (SparseDataChunk.java:159-174) and
  ``HashLocPair(byte[])`` (HashLocPair.java:86-97): ``[u8 flags][BE32 length, ignored][BE32 zlen]
  [zlen x BAL][BE32 doop]``, pairs into a TreeMap keyed by pos (ascending pos; of two pairs with the
  same pos the later one in the image wins); zlen <= 0 = no pairs; an image that does not fit
  its slot (BufferUnderflowException) or a pair with a negative len / pos / offset / nlen
  (checkCorrupt) = corrupt;
* terminator: pairs in ascending pos up to, not including, the first whose hashloc == 0
  (WritableCacheBuffer.java:262-278);
* fetch: ``chunks`` maps hashloc -> the decoded chunk, or None when getChunk fails; a hashloc
  that is no key of it is outside the store's directory;
* placement (WritableCacheBuffer.java:364-396): c = min(nlen, len(ck)); ck[offset : offset + c] ->
  buf[pos : pos + c] in pos order; pos > CHUNK_LENGTH, pos + c > CHUNK_LENGTH or offset + c >
  len(ck) fails the buffer.
A failed buffer reads as zeros with a status bit (include/sdfs_read.h).
"""
from __future__ import annotations

import struct

from oracle import meta_oracle as M

OK, CORRUPT, MISSING, FETCH, BOUNDS = 0, 1, 2, 4, 8


def pair_bytes(digest: bytes, hashloc: int, ln: int, pos: int, offset: int = 0, nlen=None) -> bytes:
    """HashLocPair.asArray; negative fields (which asArray refuses) are packed as they are."""
    nlen = ln if nlen is None else nlen
    if min(ln, pos, offset, nlen) >= 0:
        return M.hashlocpair_as_array(digest, hashloc, ln, pos, offset, nlen)
    return bytes(digest) + struct.pack(">qiiii", hashloc, ln, pos, offset, nlen)


def build_image(pairs, flags: int = 0, doop: int = 0, zlen=None) -> bytes:
    """pairs: (digest, hashloc, len, pos, offset, nlen) in IMAGE order (not sorted)."""
    body = b"".join(pair_bytes(*p) for p in pairs)
    z = len(pairs) if zlen is None else zlen
    return struct.pack(">BIi", flags, 13 + len(body), z) + body + struct.pack(">I", doop)


def parse(img: bytes, slot_bytes: int, hash_len: int):
    """-> (status, pairs in TreeMap order as (hash, hashloc, len, pos, offset, nlen), doop, flags)."""
    img = bytes(img) + bytes(max(0, slot_bytes - len(img)))
    bal = hash_len + 24
    flags = img[0]
    zlen = struct.unpack(">i", img[5:9])[0]
    n = max(zlen, 0)
    if 13 + n * bal > slot_bytes:
        return CORRUPT, [], 0, flags
    tree = {}
    for i in range(n):
        rec = img[9 + i * bal: 9 + (i + 1) * bal]
        hashloc, ln, pos, offset, nlen = struct.unpack(">qiiii", rec[hash_len:])
        if min(ln, pos, offset, nlen) < 0:
            return CORRUPT, [], 0, flags
        tree[pos] = (rec[:hash_len], hashloc, ln, pos, offset, nlen)
    doop = struct.unpack(">I", img[9 + n * bal: 13 + n * bal])[0]
    return OK, [tree[p] for p in sorted(tree)], doop, flags


def used_pairs(pairs):
    out = []
    for p in pairs:
        if p[1] == 0:
            break
        out.append(p)
    return out


def read_buffer(img: bytes, slot_bytes: int, hash_len: int, chunk_length: int, chunks: dict):
    """-> (status, the buffer's chunk_length bytes)."""
    zeros = bytes(chunk_length)
    status, pairs, _, _ = parse(img, slot_bytes, hash_len)
    if status:
        return status, zeros
    used = used_pairs(pairs)
    if any(p[1] not in chunks for p in used):
        return MISSING, zeros
    if any(chunks[p[1]] is None for p in used):
        return FETCH, zeros
    buf = bytearray(chunk_length)
    for _, hashloc, _, pos, offset, nlen in used:
        ck = chunks[hashloc]
        c = len(ck) if nlen > len(ck) else nlen
        if pos > chunk_length or pos + c > chunk_length or offset + c > len(ck):
            return BOUNDS, zeros
        buf[pos:pos + c] = ck[offset:offset + c]
    return OK, bytes(buf)
