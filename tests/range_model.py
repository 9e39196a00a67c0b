"""Plain-Python model of the ranged read's rules — TEST INFRASTRUCTURE ONLY.

Restated from the reference: ``DedupFileChannel.read(buf, bufPos, siz, filePos)``
(DedupFileChannel.java:499-608) clips a request at the file's length (-1 at or past it) and walks
it buffer by buffer; ``WritableCacheBuffer.readChunk`` (:217-245) is ``initBuffer`` followed by an
arraycopy of ``[startPos, startPos + len)``; a buffer past the end of the map is a fresh blank one.
The buffer rules (parse, terminator, placement) are tests/read_model.py's.

One divergence from the reference, stated in include/sdfs_read.h: only the pairs that *touch* a
piece decide its status and are fetched, where the reference rebuilds (and fails) the whole buffer.
"""
from __future__ import annotations

from tests import read_model as R

OK, CORRUPT, MISSING, FETCH, BOUNDS = R.OK, R.CORRUPT, R.MISSING, R.FETCH, R.BOUNDS
NONE = -1


def split(files, requests, chunk_length):
    """files: (first_slot, n_slots, file_len); requests: (file, file_pos, siz, out_off).
    -> (n_read per request, pieces as (request, row, start, len, out_off), rows = the distinct touched
    slots ascending).  A piece past its file's map has row NONE."""
    n_read, raw = [], []
    for r, (f, file_pos, siz, out_off) in enumerate(requests):
        first, n_slots, file_len = files[f]
        if file_pos >= file_len:
            n_read.append(-1)
            continue
        n = min(siz, file_len - file_pos)
        n_read.append(n)
        pos, out = file_pos, out_off
        while pos < file_pos + n:
            b, start = divmod(pos, chunk_length)
            ln = min(chunk_length - start, file_pos + n - pos)
            raw.append((r, first + b if b < n_slots else None, start, ln, out))
            pos += ln
            out += ln
    rows = sorted({s for _, s, _, _, _ in raw if s is not None})
    index = {s: i for i, s in enumerate(rows)}
    pieces = [(r, NONE if s is None else index[s], start, ln, out) for r, s, start, ln, out in raw]
    return n_read, pieces, rows


def touching(used, start, ln):
    """Indices in U of the pairs that touch [start, start + ln): pos < start + ln, pos + nlen > start,
    nlen > 0."""
    return [i for i, p in enumerate(used) if p[5] > 0 and p[3] < start + ln and p[3] + p[5] > start]


def read_piece(img, slot_bytes, hash_len, chunk_length, chunks, start, ln):
    """One piece of the buffer whose image is img (None: no row).  chunks: hashloc -> the decoded
    chunk, or None when getChunk fails; a hashloc that is no key is outside the directory.
    -> (status, the piece's ln bytes, the indices — in the row's TreeMap order — of its touching
    pairs when the plan leaves its status 0: those pairs are needed)."""
    zeros = bytes(ln)
    if img is None:
        return OK, zeros, set()
    status, pairs, _, _ = R.parse(img, slot_bytes, hash_len)
    if status:
        return CORRUPT, zeros, set()
    used = R.used_pairs(pairs)  # a prefix of the row: U's indices are the row's
    needed = set(touching(used, start, ln))
    touch = [used[i] for i in sorted(needed)]
    if any(p[1] not in chunks for p in touch):
        return MISSING, zeros, set()
    if any(chunks[p[1]] is None for p in touch):
        return FETCH, zeros, needed
    buf = bytearray(chunk_length)
    for _, hashloc, _, pos, offset, nlen in touch:
        ck = chunks[hashloc]
        c = len(ck) if nlen > len(ck) else nlen
        if pos > chunk_length or pos + c > chunk_length or offset + c > len(ck):
            return BOUNDS, zeros, needed
    for _, hashloc, _, pos, offset, nlen in touch:  # ascending pos: the last one covering a byte wins
        ck = chunks[hashloc]
        c = min(nlen, len(ck))
        buf[pos:pos + c] = ck[offset:offset + c]
    return OK, bytes(buf[start:start + ln]), needed


def read_ranges(images, slot_bytes, hash_len, chunk_length, chunks, files, requests, out):
    """images: slot index -> image (a missing key reads as a never-written slot).  out: bytearray,
    written only inside the pieces' extents.  -> (n_read, per-request status, per-piece status,
    needed pairs as {(row, index)}, needed hashlocs, pieces, rows)."""
    n_read, pieces, rows = split(files, requests, chunk_length)
    req_status = [0] * len(requests)
    piece_status, needed, hashlocs = [], set(), set()
    for r, row, start, ln, out_off in pieces:
        img = None if row == NONE else images.get(rows[row], bytes(slot_bytes))
        st, data, need = read_piece(img, slot_bytes, hash_len, chunk_length, chunks, start, ln)
        out[out_off:out_off + ln] = data
        piece_status.append(st)
        req_status[r] |= st
        needed |= {(row, i) for i in need}
        if need:
            pairs = R.parse(img, slot_bytes, hash_len)[1]
            hashlocs |= {pairs[i][1] for i in need}
    return n_read, req_status, piece_status, needed, hashlocs, pieces, rows
