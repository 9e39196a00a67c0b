"""A plain-Python model of the ranged write (include/sdfs_write.h), restated from
DedupFileChannel.writeFile (DedupFileChannel.java:274-359) and WritableCacheBuffer.write
(WritableCacheBuffer.java:523-563): a batch is one flush, its requests applied in order.

Two parts.  The split: every byte of a buffer remembers the last request that wrote it and where
in the blob its byte lies (painting, not interval arithmetic), and the visible pieces, runs,
``row_full`` and file lengths are read off the painted buffers.  The file model: zeros-extended
bytearrays with the requests applied in order.
"""
import numpy as np


class Invalid(Exception):
    """The batch is refused (SDFS_CDC_EINVAL)."""


def split(files, requests, cl, blob_bytes):
    """files: [(first_slot, n_slots, file_len)], requests: [(file, file_pos, len, src_off)] ->
    dict(n_written, file_len, pieces [(row, start, len, src_off, req)], runs [(row, run_pos, run_len,
    first_piece, n_pieces)], rows [slot], row_full [0/1])."""
    if not 1 <= cl <= 2 ** 31 - 1:
        raise Invalid("chunk_length")
    for first, n, _ in files:
        if first + n >= 2 ** 64:
            raise Invalid("first_slot + n_slots")
    written = set()
    for f, pos, ln, src in requests:
        if f >= len(files):
            raise Invalid("file")
        if src + ln > blob_bytes or src + ln >= 2 ** 64 or pos + ln >= 2 ** 64:
            raise Invalid("blob / overflow")
        if ln and (pos + ln - 1) // cl >= files[f][1]:
            raise Invalid("past the file's slots")
        if ln:
            written.add(f)
    spans = sorted((files[f][0], files[f][0] + files[f][1]) for f in written if files[f][1])
    for a, b in zip(spans, spans[1:]):
        if b[0] < a[1]:
            raise Invalid("two written files share a slot")
    file_len = [fl for _, _, fl in files]
    painted = {}  # slot -> (req per byte, blob offset per byte)
    for r, (f, pos, ln, src) in enumerate(requests):
        if ln == 0:
            continue
        file_len[f] = max(file_len[f], pos + ln)
        done = 0
        while done < ln:
            b, start = divmod(pos + done, cl)
            n = min(cl - start, ln - done)
            who, where = painted.setdefault(files[f][0] + b, (np.full(cl, -1, np.int64), np.zeros(cl, np.int64)))
            who[start:start + n] = r
            where[start:start + n] = src + done + np.arange(n)
            done += n
    rows = sorted(painted)
    pieces, runs, full = [], [], []
    for row, slot in enumerate(rows):
        who, where = painted[slot]
        # a piece begins where the request changes or the blob bytes stop following each other
        begins = np.ones(cl, bool)
        begins[1:] = (who[1:] != who[:-1]) | ((who[1:] >= 0) & (where[1:] != where[:-1] + 1))
        edges = np.append(np.flatnonzero(begins), cl)
        prev_end = None
        for i, j in zip(edges[:-1].tolist(), edges[1:].tolist()):
            if who[i] < 0:
                continue
            if prev_end == i:
                r0 = runs[-1]
                runs[-1] = (r0[0], r0[1], r0[2] + j - i, r0[3], r0[4] + 1)
            else:
                runs.append((row, i, j - i, len(pieces), 1))
            pieces.append((row, i, j - i, int(where[i]), int(who[i])))
            prev_end = j
        full.append(int((who >= 0).all()))
    return dict(n_written=[q[2] for q in requests], file_len=file_len, pieces=pieces, runs=runs, rows=rows,
                row_full=full)


def apply(file_bytes, requests, blob):
    """file_bytes: [bytearray] (the files as they read before the batch); the requests applied in
    order, a file extended with zeros where a write starts past its end.  -> [bytearray]."""
    out = [bytearray(b) for b in file_bytes]
    for f, pos, ln, src in requests:
        if ln == 0:
            continue
        if len(out[f]) < pos + ln:
            out[f].extend(bytes(pos + ln - len(out[f])))
        out[f][pos:pos + ln] = bytes(blob[src:src + ln])
    return out


def as_lists(p):
    """``sdfs_amd.write.WritePieces`` in the shape :func:`split` returns."""
    return dict(n_written=[int(v) for v in p.n_written], file_len=[int(v) for v in p.file_len],
                pieces=[tuple(int(v) for v in t) for t in zip(p.row, p.start, p.len, p.src_off, p.req)],
                runs=[tuple(int(v) for v in t) for t in zip(p.run_row, p.run_pos, p.run_len, p.run_first_piece,
                                                             p.run_n_pieces)],
                rows=[int(v) for v in p.rows], row_full=[int(v) for v in p.row_full])
