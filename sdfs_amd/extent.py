"""Extent copies and block rewrites on the MI355X (include/sdfs_extent.h): HashLocPairs merged
into map slots that already exist, without moving a byte of chunk data.

* ``copyExtents`` (mgmt/CopyExtents.java:80-180): :func:`split_extent` cuts a file range at the
  buffer boundaries of both files, :func:`copy_extents` runs parse -> extents -> insert -> emit.
* the write accelerator (WritableCacheBuffer.java:617-781): :func:`rewrite_blocks` chunks and stores
  only the written runs and inserts one pair per finger into the existing slots.

The merge implements ``SparseDataChunk.insertHashLocPair`` (SparseDataChunk.java:208-263) with one
deliberate divergence: a split's tail is kept (the reference loses it through the alias of line 248;
see the header).  PyTorch allocates HBM, groups the inserts by destination buffer (a stable sort)
and hands over the stream; every rule runs in the library's HIP kernels.  No CPU fallback.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

from . import _lib
from ._lib import (EXT_BAD_INSERT, EXT_CORRUPT, EXT_ECAP, EXT_HOLE, EXT_OVERFLOW, EXT_OVERLAP, EXT_SRC,  # noqa: F401
                   check, ptr, stream_of)
from .read import ParsedPairs, pair_cap, parse_map_slots


def split_extent(sstart: int, dstart: int, length: int, chunk_length: int):
    """The file range [sstart, sstart + length) copied to dstart, cut at every source-buffer and
    destination-buffer boundary: [(src_buf, src_off, dst_buf, dst_off, len)], the segments
    ``CopyExtents``' loop walks (CopyExtents.java:96-155)."""
    if min(sstart, dstart) < 0 or length < 0 or chunk_length < 1:
        raise ValueError("negative range")
    out, done = [], 0
    while done < length:
        sb, so = divmod(sstart + done, chunk_length)
        db, do = divmod(dstart + done, chunk_length)
        n = min(length - done, chunk_length - so, chunk_length - do)
        out.append((sb, so, db, do, n))
        done += n
    return out


@dataclass
class InsertList:
    """``sdfs_cdc_inserts``: row i is one insert (device tensors, ``cap`` rows)."""

    cap: int
    hash: object     # uint8 [cap, 32]
    hashloc: object  # int64 [cap]
    len: object      # int32 [cap]
    pos: object
    offset: object
    nlen: object
    dst_buf: object  # int32 [cap]; rows no call has written hold ``fill``

    def __post_init__(self):
        self.c = _lib.Inserts(hash=self.hash.data_ptr(), hashloc=self.hashloc.data_ptr(), len=self.len.data_ptr(),
                              pos=self.pos.data_ptr(), offset=self.offset.data_ptr(), nlen=self.nlen.data_ptr(),
                              dst_buf=self.dst_buf.data_ptr())

    @classmethod
    def empty(cls, cap: int, device, fill: int = 0):
        import torch

        n = max(int(cap), 1)
        z = lambda *shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device=device)  # noqa: E731
        return cls(int(cap), z(n, 32, dt=torch.uint8), z(n, dt=torch.int64), z(n), z(n), z(n), z(n),
                   torch.full((n,), int(fill), dtype=torch.int32, device=device))

    def take(self, order):
        """The rows ``order`` (a device int64 tensor) as a new list."""
        return InsertList(int(order.shape[0]), self.hash[order].contiguous(), self.hashloc[order].contiguous(),
                          self.len[order].contiguous(), self.pos[order].contiguous(), self.offset[order].contiguous(),
                          self.nlen[order].contiguous(), self.dst_buf[order].contiguous())


def empty_pairs(nbuf: int, cap: int, hash_len: int, device) -> ParsedPairs:
    """A :class:`ParsedPairs` for ``insert_pairs`` to write into."""
    import torch

    nb, cap = max(int(nbuf), 1), max(int(cap), 1)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)  # noqa: E731
    return ParsedPairs(int(nbuf), cap, int(hash_len), z(nb, torch.int32), z((nb, cap, 32), torch.uint8),
                       z((nb, cap), torch.int64), z((nb, cap), torch.int32), z((nb, cap), torch.int32),
                       z((nb, cap), torch.int32), z((nb, cap), torch.int32), z(nb, torch.int32), z(nb, torch.uint8),
                       z(nb, torch.int32))


def _rows(rows, width: int):
    """Rows of uint32 values (a list of tuples or an array) as one contiguous host array [n, width]."""
    import numpy as np

    a = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, width))
    if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
        raise ValueError("segment / run fields are unsigned 32-bit values")
    return a.astype(np.uint32)


def _upload(a, device):
    import torch

    return torch.from_numpy(a.view("int32")).to(device) if a.size else torch.zeros(1, dtype=torch.int32, device=device)


def map_extents(src: ParsedPairs, segments, nbuf_dst: int, chunk_length: int, n_ins_cap: int | None = None,
                device: int = 0, stream=None):
    """``sdfs_cdc_map_extents``.  segments: [(src_buf, src_off, dst_buf, dst_off, len)], a list or an
    integer array [n_seg, 5] (the cheaper form for thousands of them).  Returns
    (:class:`InsertList` of n_ins_cap rows whose unwritten rows have dst_buf = nbuf_dst, seg_first
    int32 [n_seg + 1], seg_status int32 [n_seg]).  seg_first[-1] is the number of pieces; when it is
    larger than n_ins_cap nothing was written (call again with that capacity).  Default capacity:
    every source slot once plus one piece per segment, enough for segments that do not overlap."""
    import torch

    dev = src.counts.device
    h = _rows(segments, 5)
    n_seg = int(h.shape[0])
    if n_ins_cap is None:
        n_ins_cap = src.nbuf * src.cap + n_seg
    ins = InsertList.empty(n_ins_cap, dev, fill=nbuf_dst)
    first = torch.zeros(n_seg + 1, dtype=torch.int32, device=dev)
    status = torch.zeros(max(n_seg, 1), dtype=torch.int32, device=dev)
    d = _upload(h, dev)
    check(_lib.load().sdfs_cdc_map_extents(int(device), src.nbuf, ctypes.byref(src.c), int(nbuf_dst), int(chunk_length),
                                           n_seg, h.ctypes.data, d.data_ptr(), ctypes.byref(ins.c), int(n_ins_cap),
                                           first.data_ptr(), status.data_ptr(), stream_of(first, stream)))
    return ins, first, status[:n_seg]


def inserts_from_chunks(batch, hashloc, dst_buf, run_pos, nbuf_dst: int, chunk_length: int,
                        n_ins_cap: int | None = None, device: int = 0, stream=None):
    """``sdfs_cdc_map_inserts_from_chunks``: batch, a DeviceBatch after run() whose buffers are the
    runs; hashloc: the index's per-record output; dst_buf / run_pos: one int per run.  Returns
    (:class:`InsertList` in record order, unwritten rows with dst_buf = nbuf_dst; run_first int32
    [n_run + 1])."""
    import numpy as np
    import torch

    dev = batch.data.device
    if len(dst_buf) != batch.nbuf or len(run_pos) != batch.nbuf:
        raise ValueError("one destination buffer and one position per run")
    if n_ins_cap is None:
        n_ins_cap = batch.nbuf * batch.cap
    ins = InsertList.empty(n_ins_cap, dev, fill=nbuf_dst)
    first = torch.zeros(batch.nbuf + 1, dtype=torch.int32, device=dev)
    h = _rows(np.stack([np.asarray(dst_buf, dtype=np.int64), np.asarray(run_pos, dtype=np.int64)], axis=1), 2)
    d = _upload(h, dev)
    check(_lib.load().sdfs_cdc_map_inserts_from_chunks(
        int(device), batch.nbuf, ctypes.byref(batch.out), batch.buf_len, hashloc.data_ptr(), int(nbuf_dst),
        int(chunk_length), h.ctypes.data, d.data_ptr(), ctypes.byref(ins.c), int(n_ins_cap), first.data_ptr(),
        stream_of(first, stream)))
    return ins, first


def group_inserts(ins: InsertList, nbuf: int):
    """Inserts grouped by destination buffer, list order kept inside a group (a stable sort): the
    grouped :class:`InsertList` and ins_first int32 [nbuf + 1].  Rows whose dst_buf is not below nbuf
    (the unwritten ones) go to the end, past ins_first[nbuf]."""
    import torch

    key = ins.dst_buf[: max(ins.cap, 0)].long()
    order = torch.sort(key, stable=True).indices
    g = ins.take(order) if ins.cap else ins
    bounds = torch.arange(nbuf + 1, device=key.device, dtype=torch.int64)
    first = torch.searchsorted(key[order].contiguous(), bounds).to(torch.int32)
    return g, first


def insert_pairs(pairs: ParsedPairs, ins: InsertList, ins_first, chunk_length: int, slot_pairs: int, out_cap: int,
                 device: int = 0, stream=None):
    """``sdfs_cdc_map_insert``: (merged :class:`ParsedPairs` of out_cap columns, dup uint8 [nbuf,
    out_cap], status int32 [nbuf]).  ``ins`` grouped by destination buffer (:func:`group_inserts`)."""
    import torch

    dev = pairs.counts.device
    out = empty_pairs(pairs.nbuf, out_cap, pairs.hash_len, dev)
    dup = torch.zeros((max(pairs.nbuf, 1), out.cap), dtype=torch.uint8, device=dev)
    status = torch.zeros(max(pairs.nbuf, 1), dtype=torch.int32, device=dev)
    check(_lib.load().sdfs_cdc_map_insert(int(device), pairs.nbuf, int(chunk_length), int(slot_pairs),
                                          ctypes.byref(pairs.c), ctypes.byref(ins.c), int(ins.cap),
                                          ins_first.data_ptr(), ctypes.byref(out.c), dup.data_ptr(), status.data_ptr(),
                                          stream_of(status, stream)))
    return out, dup, status[: pairs.nbuf]


def emit_pairs(pairs: ParsedPairs, m, slot_len: int, dup=None, status=None, flags: int = 0, device: int = 0,
               stream=None):
    """``sdfs_cdc_map_emit_pairs`` into ``m`` (device uint8, nbuf slots of slot_len bytes, updated in
    place).  Returns (doop int32 [nbuf], skipped int32 [1])."""
    import torch

    dev = m.device
    if m.numel() < pairs.nbuf * slot_len:
        raise ValueError(f"map holds {m.numel()} bytes, {pairs.nbuf} slots of {slot_len} need {pairs.nbuf * slot_len}")
    doop = torch.zeros(max(pairs.nbuf, 1), dtype=torch.int32, device=dev)
    skipped = torch.zeros(1, dtype=torch.int32, device=dev)
    check(_lib.load().sdfs_cdc_map_emit_pairs(int(device), pairs.nbuf, ctypes.byref(pairs.c), pairs.hash_len,
                                              ptr(dup), ptr(status), int(flags),
                                              m.data_ptr(), int(slot_len), doop.data_ptr(), skipped.data_ptr(),
                                              stream_of(m, stream)))
    return doop[: pairs.nbuf], skipped


@dataclass
class ExtentInfo:
    n_inserts: int            # pairs inserted over all buffers
    pairs: ParsedPairs = None  # the merged pairs (valid input to plan_reads / assemble, OVERFLOW buffers included)
    dup: object = None        # uint8 [nbuf, cap]: split tails
    before: ParsedPairs = None  # the destination's pairs as parsed
    skipped: object = None    # int32 [1]: buffers emit left as they were
    written: bool = False     # False: a segment had a status, nothing was changed
    extra: dict = field(default_factory=dict)


def _live(pairs: ParsedPairs, rows):
    """(hashes [k, 32], hashloc [k]) of the pairs of the buffers ``rows`` (a bool mask [nbuf])."""
    import torch

    nb = pairs.nbuf
    col = torch.arange(pairs.cap, device=rows.device)[None, :]
    mask = (col < pairs.counts[:nb, None]) & rows[:, None]
    return pairs.hashes[:nb][mask], pairs.hashloc[:nb][mask]


def _move_claims(index, before: ParsedPairs, after: ParsedPairs, rows, minus=None):
    """One claim_digests call: +1 per pair of ``after``, -1 per pair of ``before`` in the buffers
    ``rows``, -1 per (hashes, hashloc) of ``minus``; each at its own hashloc."""
    import torch

    ah, al = _live(after, rows)
    bh, bl = _live(before, rows)
    hs, ls = [ah, bh], [al, bl]
    delta = [torch.ones_like(al), -torch.ones_like(bl)]
    if minus is not None:
        hs.append(minus[0])
        ls.append(minus[1])
        delta.append(-torch.ones_like(minus[1]))
    h = torch.cat(hs).contiguous()
    if h.shape[0]:
        index.claim_digests(h, torch.cat(delta), expect_pos=torch.cat(ls))


def copy_extents(src_map, dst_map, nbuf_src: int, nbuf_dst: int, slot_len: int, segments, index=None,
                 hash_len: int = 32, chunk_length: int = 262144, device: int = 0, stages=None):
    """``copyExtents`` for a batch of segments (:func:`split_extent`): the covering pairs of every
    source range are cut (getWL) and merged into the destination slots (insertHashLocPair), and the
    new images are written over the old ones in ``dst_map``.  No chunk data is read or written.

    All sources are parsed and cut before any destination slot is written, so ``src_map is dst_map``
    (a copy inside one file) sees the old state of the file throughout — unlike the reference's
    loop, whose later steps see what the earlier ones inserted.

    Returns (dst_map, status int32 [nbuf_dst], seg_status int32 [n_seg], :class:`ExtentInfo`).
    A segment with SDFS_CDC_EXT_HOLE or SDFS_CDC_EXT_SRC stops the whole batch before anything is
    written (the reference throws in the middle of its copy; all-or-nothing is the batch's form of
    that).  A buffer with a status keeps its old image.  SDFS_CDC_EXT_OVERFLOW — the merged list does
    not fit the slot — is reported, not handled: the caller materialises that buffer (read, overlay,
    a whole-buffer write) as the reference does (WritableCacheBuffer.java:579-595); the merged pairs
    in ``info.pairs`` are valid for such a buffer too and can go to ``plan_reads`` / ``assemble``.

    index: a :class:`sdfs_amd.index.HipHashesMap`.  Its counts are kept exact — a fingerprint's count
    is the number of pairs in persisted slots that name it — where the reference's ``reReference``
    over-counts: for every destination buffer that ended with status 0, +1 per pair after and -1 per
    pair before, in one ``claim_digests`` call.  Buffers with a status move no counts.

    One host read (piece total, segment statuses, pair and insert counts) sizes the output."""
    import torch

    mark = stages or (lambda name: None)
    src = parse_map_slots(src_map, nbuf_src, slot_len, hash_len, device)
    dst = src if (src_map is dst_map and nbuf_src == nbuf_dst) else parse_map_slots(dst_map, nbuf_dst, slot_len,
                                                                                   hash_len, device)
    mark("parse")
    ins, seg_first, seg_status = map_extents(src, segments, nbuf_dst, chunk_length, device=device)
    grouped, ins_first = group_inserts(ins, nbuf_dst)
    mark("extents")

    def read():
        per_buf = dst.counts[:nbuf_dst] + 2 * (ins_first[1:] - ins_first[:-1])
        worst = per_buf.max().view(1) if nbuf_dst else seg_first[-1:] * 0
        return torch.cat([seg_first[-1:], worst.to(torch.int32), seg_status]).tolist()

    total, out_cap, *seg_st = read()
    if total > ins.cap:  # overlapping source segments: once more with room for every piece
        ins, seg_first, seg_status = map_extents(src, segments, nbuf_dst, chunk_length, n_ins_cap=total, device=device)
        grouped, ins_first = group_inserts(ins, nbuf_dst)
        total, out_cap, *seg_st = read()
    info = ExtentInfo(total, before=dst)
    if any(seg_st):
        return dst_map, torch.zeros(nbuf_dst, dtype=torch.int32, device=dst_map.device), seg_status, info
    slot_pairs = pair_cap(slot_len, hash_len)
    out, dup, status = insert_pairs(dst, grouped, ins_first, chunk_length, slot_pairs, max(out_cap, 1), device)
    mark("insert")
    _, info.skipped = emit_pairs(out, dst_map, slot_len, dup=dup, status=status, device=device)
    mark("emit")
    if index is not None:
        _move_claims(index, dst, out, status == 0)
        mark("claims")
    info.pairs, info.dup, info.written = out, dup, True
    return dst_map, status, seg_status, info


def rewrite_blocks(writer, batch, pos_base: int, dst_map, nbuf_dst: int, slot_len: int, dst_buf, run_pos,
                   chunk_length: int = 262144, device: int = 0, stages=None, **write_args):
    """The write accelerator for a batch of partial writes: ``batch`` holds one written run per
    buffer (all of one length, a multiple of 64 — what ``DeviceBatch`` takes), run r goes to
    ``run_pos[r]`` of destination buffer ``dst_buf[r]``.  Only the runs are chunked, deduplicated and
    stored (``writer.write(batch, pos_base)``, unchanged; the map slots it makes for the runs are
    not used), then one pair per finger is merged into the existing slots of ``dst_map`` and the
    new images are written in place.  The rest of each buffer is never read, chunked or stored again.

    Returns (dst_map, status int32 [nbuf_dst], the runs' :class:`ArchiveSet`, :class:`ExtentInfo`).
    Reads go through a directory of the old and the new store concatenated (``pos_base`` of this
    call = the first write's ``pos_base`` + the length of its directory).

    Counts in ``writer.index`` stay exact: ``put_records`` has counted +1 per run record, so this
    adds +1 per pair after and -1 per pair before for the buffers that ended with status 0, and -1
    per run record.  A buffer with a status gets only the -1 per run record: its run's fingerprints
    go back to where they were, possibly at count 0 until the next sweep.  SDFS_CDC_EXT_OVERFLOW is
    reported, not handled, as in :func:`copy_extents`."""
    import torch

    mark = stages or (lambda name: None)
    _, arcs = writer.write(batch, pos_base, **write_args)
    mark("write")
    hash_len = writer.hash_len
    dst = parse_map_slots(dst_map, nbuf_dst, slot_len, hash_len, device)
    mark("parse")
    ins, run_first = inserts_from_chunks(batch, arcs.extra["hashloc"], dst_buf, run_pos, nbuf_dst, chunk_length,
                                         device=device)
    grouped, ins_first = group_inserts(ins, nbuf_dst)
    mark("extents")
    per_buf = dst.counts[:nbuf_dst] + 2 * (ins_first[1:] - ins_first[:-1])
    total, out_cap = torch.cat([run_first[-1:], per_buf.max().view(1).to(torch.int32)]).tolist()  # the one host read
    out, dup, status = insert_pairs(dst, grouped, ins_first, chunk_length, pair_cap(slot_len, hash_len),
                                    max(out_cap, 1), device)
    mark("insert")
    info = ExtentInfo(total, out, dup, dst, written=True)
    _, info.skipped = emit_pairs(out, dst_map, slot_len, dup=dup, status=status, device=device)
    mark("emit")
    _move_claims(writer.index, dst, out, status == 0, minus=(ins.hash[:total], ins.hashloc[:total]))
    mark("claims")
    return dst_map, status, arcs, info
