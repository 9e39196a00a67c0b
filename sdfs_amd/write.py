"""Ranged writes on the MI355X (include/sdfs_write.h): ``DedupFileChannel.writeFile``
(DedupFileChannel.java:274-359) for batches of byte ranges — the write twin of
``HipBufferReader.read_ranges``.

A file system hands over ``write(file, pos, len)`` calls at any alignment that cross buffer
boundaries, overlap each other, extend the file and land in buffers that were never written.
:class:`HipFileWriter` takes a batch of them as one flush:

* :func:`split_writes` — ``sdfs_cdc_write_split`` (host): requests cut at ``CHUNK_LENGTH``
  (:310-352), overlaps resolved in request order, touching pieces joined into runs.
* :func:`stage_pieces` — ``sdfs_cdc_write_stage``: the visible pieces gathered from the caller's
  blob into the staging area, any alignment on both sides.
* :func:`inserts_from_runs` — ``sdfs_cdc_map_inserts_from_runs``: the write accelerator's insert
  list (WritableCacheBuffer.java:729-753) for runs of different lengths.
* :meth:`HipFileWriter.write_ranges` — the routing of ``WritableCacheBuffer.write`` (:523-563)
  per touched buffer, one engine batch per round, the overflow fallback and exact reference counts.

PyTorch allocates HBM and hands over the stream; every step runs the library's HIP kernels.  No
CPU fallback: a failure raises :class:`SdfsCdcError`.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

from . import _lib
from ._lib import EXT_OVERFLOW, WRITE_BOUNDS, WRITE_READ, WRITE_SLOT, check, stream_of  # noqa: F401
from .extent import InsertList, _move_claims, emit_pairs, group_inserts, insert_pairs
from .read import _u64_table, pair_cap, parse_map_slots

ROUTE_FAIL, ROUTE_FULL, ROUTE_ACCEL, ROUTE_MATERIALISE, ROUTE_ACCEL_MATERIALISE = 0, 1, 2, 3, 4


@dataclass
class WritePieces:
    """``sdfs_cdc_write_split``'s outputs (host numpy arrays).  Piece p: the bytes blob[src_off[p] :
    + len[p]] of request req[p] are what row row[p] shows at [start[p], start[p] + len[p]); run u:
    pieces first_piece[u] .. + n_pieces[u] touch and cover [run_pos[u], + run_len[u]) of run_row[u];
    rows: the distinct touched slots, ascending; row_full[i]: the row's pieces cover it all."""

    n_written: object    # int64 [n_requests]
    file_len: object     # int64 [n_files]
    row: object          # int32 [n_pieces]
    start: object
    len: object
    req: object
    src_off: object      # int64 [n_pieces]
    run_row: object      # int32 [n_runs]
    run_pos: object
    run_len: object
    run_first_piece: object
    run_n_pieces: object
    rows: object         # int64 [n_rows]
    row_full: object     # uint8 [n_rows]


def split_writes(files, requests, chunk_length: int, blob_bytes: int) -> WritePieces:
    """``sdfs_cdc_write_split`` (host): ``DedupFileChannel.writeFile``'s request layer.  files: rows of
    (first_slot, n_slots, file_len); requests: rows of (file, file_pos, len, src_off)."""
    import numpy as np

    lib = _lib.load()
    f = _u64_table(files, 3, "files")
    q = _u64_table(requests, 4, "requests")
    n_written = np.zeros(max(len(q), 1), np.int64)
    file_len = np.zeros(max(len(f), 1), np.uint64)
    ip = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    # the documented bound on the cuts, clipped: a first call that runs short reports the counts
    per = np.minimum(q[:, 2] // np.uint64(max(int(chunk_length), 1)), np.uint64(1 << 20)) + np.uint64(2)
    pcap = min(int(per.sum()), 1 << 20)
    rcap = wcap = pcap
    while True:
        u32 = [np.zeros(max(pcap, 1), np.uint32) for _ in range(4)]
        src_off = np.zeros(max(pcap, 1), np.uint64)
        run = [np.zeros(max(rcap, 1), np.uint32) for _ in range(5)]
        rows = np.zeros(max(wcap, 1), np.uint64)
        full = np.zeros(max(wcap, 1), np.uint8)
        plan = _lib.WritePlan(piece_cap=pcap, run_cap=rcap, row_cap=wcap, reserved=0, piece_row=u32[0].ctypes.data,
                              piece_start=u32[1].ctypes.data, piece_len=u32[2].ctypes.data, piece_req=u32[3].ctypes.data,
                              piece_src_off=src_off.ctypes.data, run_row=run[0].ctypes.data, run_pos=run[1].ctypes.data,
                              run_len=run[2].ctypes.data, run_first_piece=run[3].ctypes.data,
                              run_n_pieces=run[4].ctypes.data, row_slot=rows.ctypes.data, row_full=full.ctypes.data)
        rc = lib.sdfs_cdc_write_split(ip(f), len(f), ip(q), len(q), int(chunk_length), int(blob_bytes), ip(n_written),
                                      ip(file_len), ctypes.byref(plan))
        if rc != _lib.ECAP:
            break
        pcap, rcap, wcap = int(plan.n_pieces), int(plan.n_runs), int(plan.n_rows)
    check(rc)
    n, r, w = int(plan.n_pieces), int(plan.n_runs), int(plan.n_rows)
    i32 = lambda a, k: a[:k].view(np.int32)  # noqa: E731
    return WritePieces(n_written[:len(q)], file_len[:len(f)].view(np.int64), i32(u32[0], n), i32(u32[1], n),
                       i32(u32[2], n), i32(u32[3], n), src_off[:n].view(np.int64), i32(run[0], r), i32(run[1], r),
                       i32(run[2], r), i32(run[3], r), i32(run[4], r), rows[:w].view(np.int64), full[:w])


def stage_pieces(blob, src_off, dst_off, length, max_len: int, stage, piece_req=None, req_status=None,
                 device: int = 0, stream=None):
    """``sdfs_cdc_write_stage``: piece p = blob[src_off[p] : + length[p]] -> stage[dst_off[p] : ...]
    (src_off / dst_off device int64, length device int32; blob / stage device uint8, flat).  Returns
    piece_status int32 [n_pieces] (``WRITE_BOUNDS`` on an entry the kernel refused); with piece_req
    (device int32) the bit is or-ed into req_status (device int32 [n_requests], not zeroed)."""
    import torch

    n = int(length.shape[0])
    status = torch.zeros(max(n, 1), dtype=torch.int32, device=stage.device)[:n]
    if n:
        nreq = int(req_status.shape[0]) if req_status is not None else 0
        check(_lib.load().sdfs_cdc_write_stage(
            int(device), n, blob.data_ptr(), int(blob.numel()), src_off.data_ptr(), dst_off.data_ptr(), length.data_ptr(),
            int(max_len), stage.data_ptr(), int(stage.numel()), status.data_ptr(),
            piece_req.data_ptr() if piece_req is not None else None, nreq,
            req_status.data_ptr() if nreq else None, stream_of(stage, stream)))
    return status


def inserts_from_runs(out, first_buf: int, run_len, hashloc, dst_buf, run_pos, nbuf_dst: int, chunk_length: int,
                      n_ins_cap: int, dev, device: int = 0, stream=None):
    """``sdfs_cdc_map_inserts_from_runs``: ``out``, the :class:`sdfs_amd._lib.DevOut` of a ragged engine
    batch whose buffers first_buf .. first_buf + n_run are the runs; run_len / dst_buf / run_pos: one
    int per run (host); hashloc: the index's per-record output for the whole batch.  Returns
    (:class:`InsertList` in record order, unwritten rows with dst_buf = nbuf_dst; run_first int32
    [n_run + 1], its last element the total)."""
    import numpy as np
    import torch

    n_run = len(run_len)
    if len(dst_buf) != n_run or len(run_pos) != n_run:
        raise ValueError("one destination buffer, one position and one length per run")
    ins = InsertList.empty(n_ins_cap, dev, fill=nbuf_dst)
    first = torch.zeros(n_run + 1, dtype=torch.int32, device=dev)
    h = np.zeros((max(n_run, 1), 3), np.int64)
    h[:n_run, 0], h[:n_run, 1], h[:n_run, 2] = dst_buf, run_pos, run_len
    if h.min() < 0 or h.max() > 0xFFFFFFFF:
        raise ValueError("run fields are unsigned 32-bit values")
    runs = np.ascontiguousarray(h[:, :2].astype(np.uint32))
    lens = np.ascontiguousarray(h[:, 2].astype(np.uint32))
    d = torch.from_numpy(np.concatenate([runs.reshape(-1), lens]).view(np.int32)).to(dev)
    d_runs, d_lens = d[: 2 * max(n_run, 1)], d[2 * max(n_run, 1):]
    check(_lib.load().sdfs_cdc_map_inserts_from_runs(
        int(device), int(first_buf), n_run, ctypes.byref(out), lens.ctypes.data, d_lens.data_ptr(), hashloc.data_ptr(),
        int(nbuf_dst), int(chunk_length), runs.ctypes.data, d_runs.data_ptr(), ctypes.byref(ins.c), int(n_ins_cap),
        first.data_ptr(), stream_of(first, stream)))
    return ins, first


@dataclass
class WriteResult:
    status: object       # int32 [n_requests] (device): the OR of the request's pieces, WRITE_* bits
    n_written: object    # int64 numpy [n_requests]: len, a write is never clipped
    file_len: object     # int64 numpy [n_files]: the files' new lengths
    row_route: object    # int8 numpy [n_rows], ROUTE_*
    rows: object         # int64 numpy [n_rows]: the touched slots
    n_runs: int
    n_pieces: int
    archives: list       # the ArchiveSets of the rounds: none (nothing stored), one or two
    pos_bases: list      # the pos_base of each
    pieces: WritePieces = None
    info: dict = field(default_factory=dict)

    def directory(self, store, store_off, store_len, store_raw_len, store_ivs=None):
        """The store the written image reads through: the old store (the arguments), then round 1,
        then round 2 — (store, store_off, store_len, store_raw_len, store_ivs) for
        ``HipBufferReader.read*`` with the old store's ``pos_base``.  Copies the stores."""
        import torch

        stores, offs, lens, raws, ivs = [store], [store_off], [store_len], [store_raw_len], [store_ivs]
        at = int(store.numel())
        for a in self.archives:
            stores.append(a.store)
            offs.append(a.store_off + at)
            lens.append(a.store_len)
            raws.append(a.raw_len)
            ivs.append(a.record_ivs())
            at += int(a.store.numel())
        joined_ivs = None
        if any(v is not None for v in ivs):
            joined_ivs = torch.cat([v if v is not None else torch.zeros((int(o.shape[0]), 16), dtype=torch.uint8,
                                                                        device=store.device)
                                    for v, o in zip(ivs, offs)])
        return torch.cat(stores), torch.cat(offs), torch.cat(lens), torch.cat(raws), joined_ivs


class HipFileWriter:
    """``DedupFileChannel.writeFile`` for batches of byte ranges on one GPU.

    writer: the store's :class:`sdfs_amd.archive.HipBufferWriter` (its index, LZ4 handle, archiver
    and cipher are the ones the written bytes go through); reader: a
    :class:`sdfs_amd.read.HipBufferReader` over the same store, used only when a buffer must be
    materialised; engine: the hash engine; chunk_length: Main.CHUNK_LENGTH, a multiple of 64."""

    def __init__(self, writer, reader, engine, chunk_length: int, device: int = 0):
        self.writer, self.reader, self.engine = writer, reader, engine
        self.index, self.hash_len = writer.index, int(writer.hash_len)
        self.chunk_length, self.device = int(chunk_length), int(device)
        if not 64 <= self.chunk_length < 1 << 31 or self.chunk_length % 64:
            raise ValueError("chunk_length: a multiple of 64 below 2^31 (what the engine's device batches take)")
        self._caps = {}

    def _slot_cap(self, n: int) -> int:
        if n not in self._caps:
            self._caps[n] = self.engine.slot_cap(n)
        return self._caps[n]

    # ---- one round: whole buffers, then runs, as one engine batch and one store tail
    def _round(self, c, w_rows, read_rows, run_idx, pos_base: int, ivs, mark):
        """w_rows: the rows staged as whole buffers, those of ``read_rows`` (a subset, listed first)
        rebuilt from their old image by the read path, the others on zeros or covered; run_idx: the
        runs chunked on their own.  Returns a dict, or None when nothing was left to store."""
        import numpy as np
        import torch

        pc, dev, CL = c["pc"], c["dev"], self.chunk_length
        nW, nread = len(w_rows), len(read_rows)
        run_len = pc.run_len[run_idx].astype(np.int64)
        run_off = nW * CL + np.concatenate([[0], np.cumsum((run_len + 63) // 64 * 64)])
        stage_bytes = int(run_off[-1])
        stage = torch.empty(stage_bytes + 64, dtype=torch.uint8, device=dev)
        w_ok = np.ones(nW, bool)
        if nread:
            imgs = c["images"][torch.from_numpy(np.asarray(read_rows, np.int64)).to(dev)].contiguous()
            _, rst, _ = self.reader.read(imgs, nread, c["slot_len"], c["store"], c["store_off"], c["store_len"],
                                         c["store_raw_len"], c["store_pos_base"], out=stage[: nread * CL].view(nread, CL),
                                         store_ivs=c["store_ivs"])
            w_ok[:nread] = np.asarray(rst.tolist()) == 0  # a host read: a buffer that does not read is left alone
            mark("materialise")
        for k in range(nread, nW):
            if not pc.row_full[w_rows[k]]:
                stage[k * CL: (k + 1) * CL].zero_()  # a new buffer is staged on zeros (SparseDedupFile.java:1327-1330)
        failed = [w_rows[k] for k in range(nW) if not w_ok[k]]
        # the pieces laid over the whole buffers and into the runs
        dst_of_row = np.full(len(pc.rows), -1, np.int64)
        dst_of_row[np.asarray(w_rows, np.int64)[w_ok]] = np.flatnonzero(w_ok) * CL
        run_of_piece = np.repeat(np.arange(len(pc.run_row)), pc.run_n_pieces)
        run_dst = np.zeros(len(pc.run_row), np.int64)
        run_dst[run_idx] = run_off[:-1] - pc.run_pos[run_idx]
        run_in = np.zeros(len(pc.run_row), bool)
        run_in[run_idx] = True
        dst = np.where(dst_of_row[pc.row] >= 0, dst_of_row[pc.row], run_dst[run_of_piece])
        act = np.flatnonzero((dst_of_row[pc.row] >= 0) | run_in[run_of_piece])
        npc = len(act)
        wk = np.flatnonzero(w_ok)
        nWb, nR = len(wk), len(run_idx)
        nbuf = nWb + nR
        if nbuf == 0:
            return dict(arcs=None, failed=failed, w_rows=[], nWb=0)
        offs = np.concatenate([wk * CL, run_off[:-1]]).astype(np.int64)
        lens = np.concatenate([np.full(nWb, CL, np.int64), run_len]).astype(np.int32)
        # one upload: the pieces' int64 columns and the buffers' starts, then the int32 columns
        n32 = 2 * npc + nbuf
        host = np.zeros(2 * npc + nbuf + (n32 + 1) // 2 + 1, np.int64)
        host[:npc] = pc.src_off[act]
        host[npc:2 * npc] = dst[act] + pc.start[act]
        host[2 * npc:2 * npc + nbuf] = offs
        h32 = host[2 * npc + nbuf:].view(np.int32)
        h32[:npc], h32[npc:2 * npc], h32[2 * npc:n32] = pc.len[act], pc.req[act], lens
        d = torch.from_numpy(host).to(dev)
        d32 = d[2 * npc + nbuf:].view(torch.int32)
        p_src, p_dst, d_offs = d[:npc], d[npc:2 * npc], d[2 * npc:2 * npc + nbuf]
        p_len, p_req, d_lens = d32[:npc], d32[npc:2 * npc], d32[2 * npc:n32]
        piece_status = stage_pieces(c["blob"], p_src, p_dst, p_len, CL, stage[:stage_bytes], piece_req=p_req,
                                    req_status=c["req_status"], device=self.device)
        mark("stage")
        # one ragged engine batch, one put_records, one store tail
        cap = self._slot_cap(CL)
        z = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device=dev)  # noqa: E731
        counts, starts, blens = z(nbuf, torch.int32), z(nbuf * cap, torch.int32), z(nbuf * cap, torch.int32)
        digests, total = z(nbuf * cap * 32, torch.uint8), z(1, torch.int32)
        recs = z(nbuf * cap * _lib.RECORD_BYTES, torch.uint8)
        out = _lib.DevOut(counts=counts.data_ptr(), starts=starts.data_ptr(), lens=blens.data_ptr(),
                          digests=digests.data_ptr(), cap=cap, reserved=0, records=recs.data_ptr(),
                          records_cap=nbuf * cap, total=total.data_ptr())
        self.engine.run_device_ragged(stage.data_ptr(), stage_bytes, d_offs.data_ptr(), d_lens.data_ptr(), nbuf, out,
                                      stream=torch.cuda.current_stream(dev).cuda_stream)
        mark("chunk")
        recs2 = recs.view(-1, _lib.RECORD_BYTES)
        dup, loc, new, nc = self.index.put_records(recs2, total, pos_base=pos_base)
        mark("index")
        arcs = self.writer.store_new(stage, int(lens.astype(np.int64).sum()), recs2, new, nc, ivs=ivs, buf_offs=d_offs)
        arcs.extra.update(dup=dup, hashloc=loc, new_list=new[: arcs.n_rec], stage=stage, piece_status=piece_status)
        mark("store")
        # the whole buffers' new slot images
        m = torch.zeros(max(nWb, 1) * c["slot_len"], dtype=torch.uint8, device=dev)
        ovf = torch.zeros(1, dtype=torch.int32, device=dev)
        if nWb:
            check(_lib.load().sdfs_cdc_map_emit(self.device, nWb, ctypes.byref(out), self.hash_len, dup.data_ptr(),
                                                loc.data_ptr(), m.data_ptr(), c["slot_len"], None, ovf.data_ptr(),
                                                stream_of(m, None)))
        mark("emit")
        return dict(arcs=arcs, failed=failed, w_rows=[w_rows[k] for k in wk], nWb=nWb, out=out, dup=dup, loc=loc,
                    images=m, ovf=ovf, counts=counts, keep=(counts, starts, blens, digests, total, recs, d))

    def _replace(self, c, rnd):
        """The whole buffers' images of a round replace the old ones, whose pairs are released first
        (one ``claim_slots(-1)`` over those rows)."""
        import numpy as np
        import torch

        if not rnd["nWb"]:
            return
        dev, sl = c["dev"], c["slot_len"]
        slots = torch.from_numpy(c["pc"].rows[np.asarray(rnd["w_rows"], np.int64)]).to(dev)
        sel = torch.zeros(c["nslots"], dtype=torch.uint8, device=dev)
        sel[slots] = 1
        self.index.claim_slots(c["map_slots"], c["nslots"], sl, -1, sel=sel, hash_len=self.hash_len)
        c["slots2d"][slots] = rnd["images"][: rnd["nWb"] * sl].view(rnd["nWb"], sl)

    def write_ranges(self, map_slots, nslots: int, slot_len: int, files, requests, blob, pos_base: int, store, store_off,
                     store_len, store_raw_len, store_pos_base: int, accel: bool = True, store_ivs=None, ivs=None,
                     stages=None) -> WriteResult:
        """``DedupFileChannel.writeFile`` for a batch of byte ranges, as one flush: what the reference
        leaves when all these calls arrive, in request order, before any touched buffer is flushed.

        map_slots: device uint8, one map image of nslots slots of slot_len bytes, updated in place;
        files: rows of (first_slot, n_slots, file_len) over that image; requests: rows of (file,
        file_pos, len, src_off): blob[src_off : src_off + len] (device uint8) goes to the file at
        file_pos.  New records get hashlocs from pos_base on.  store .. store_pos_base (and
        store_ivs): the store the existing pairs point to, ``read_ranges``' arguments, used only when
        a buffer must be materialised.  ivs: the new archives' IVs (round 1; default random).

        Route per touched row, decided after the parse of the touched slots:

        * FAIL — the slot does not parse, or (accelerator only) its pairs are not ascending and
          disjoint: the row's pieces get ``WRITE_SLOT``; image, store and counts untouched for it.
        * FULL — the row's pieces cover the buffer: staged from the blob alone, no read
          (WritableCacheBuffer.java:545-546; a buffer covered by several writes takes the same route,
          where the reference reads it first — the bytes are the same).
        * ACCEL — ``accel``, the slot has a pair, not full: each run is chunked from fresh state and
          one pair per finger is inserted (:617-781), what :func:`sdfs_amd.extent.rewrite_blocks`
          does for one run per buffer.
        * MATERIALISE — the slot has no pair (a new buffer, staged on zeros), or ``accel=False``: the
          old buffer is rebuilt by the read path into the staging area, the pieces are laid over it,
          the whole buffer is chunked as a flushed buffer is (:1007-1022) and its new image replaces
          the old one.  A buffer that does not read gets ``WRITE_READ`` and is left alone.

        The reference takes the accelerator only for buffers it calls reconstructed (:549; the flag
        travels in the slot's flags byte) and read-modify-write for every other partial write:
        ``accel=False`` is that route, ``accel=True`` what ``rewrite_blocks`` does for any buffer.
        Both leave the same file bytes.

        One round is one engine batch: the whole buffers, then the runs at 64-byte-aligned starts,
        get one ``run_device_ragged``, one ``put_records`` and one store tail.  An ACCEL row whose
        merged list does not fit the slot (``SDFS_CDC_EXT_OVERFLOW``) keeps its old image, its run
        records are released, and a second round materialises exactly those rows from the old image
        (:761-768) into a second :class:`ArchiveSet` at ``pos_base + len(first directory)``.

        Counts in ``writer.index`` stay exact (a fingerprint's count = the pairs in persisted slots
        naming it): replaced slots release their old pairs; ACCEL rows move +1 per pair after, -1
        per pair before, -1 per run record; a row that fails after its records were stored moves only
        the -1 per record.  A row is updated wholly or not at all; a request with a status has been
        applied to its other rows.

        Host reads: the parse's status and counts (the routes), the read path's own, the merge's
        statuses with the insert total, the store tail's."""
        import numpy as np
        import torch

        mark = stages or (lambda name: None)
        CL, sl = self.chunk_length, int(slot_len)
        dev = map_slots.device
        if blob.dtype != torch.uint8 or not blob.is_contiguous() or map_slots.dtype != torch.uint8:
            raise ValueError("blob and map_slots: contiguous uint8 device tensors")
        if not map_slots.is_contiguous() or map_slots.numel() < int(nslots) * sl:
            raise ValueError(f"map holds {map_slots.numel()} bytes, {nslots} slots of {sl} need more")
        pc = split_writes(files, requests, CL, int(blob.numel()))
        n_req, nrows = len(pc.n_written), len(pc.rows)
        if nrows and int(pc.rows[-1]) >= int(nslots):
            raise _lib.SdfsCdcError(_lib.EINVAL, f"a file names slot {int(pc.rows[-1])}, the image holds {nslots}")
        req_status = torch.zeros(max(n_req, 1), dtype=torch.int32, device=dev)[:n_req]
        res = WriteResult(req_status, pc.n_written, pc.file_len, np.zeros(nrows, np.int8), pc.rows, len(pc.run_row),
                          len(pc.row), [], [], pc)
        mark("split")
        if nrows == 0:
            return res
        slots2d = map_slots[: int(nslots) * sl].view(int(nslots), sl)
        rows_d = torch.from_numpy(pc.rows).to(dev)
        images = slots2d[rows_d].contiguous()
        pairs = parse_map_slots(images, nrows, sl, self.hash_len, self.device)
        both = torch.cat([pairs.status[:nrows], pairs.counts[:nrows]]).tolist()  # a host read: the routes
        pst, cnt = np.asarray(both[:nrows]), np.asarray(both[nrows:])
        mark("parse")
        route = np.where(pst != 0, ROUTE_FAIL,
                         np.where(pc.row_full != 0, ROUTE_FULL,
                                  np.where((cnt >= 1) & bool(accel), ROUTE_ACCEL, ROUTE_MATERIALISE))).astype(np.int8)
        row_code = np.where(route == ROUTE_FAIL, WRITE_SLOT, 0).astype(np.int32)
        c = dict(pc=pc, dev=dev, slot_len=sl, nslots=int(nslots), map_slots=map_slots, slots2d=slots2d, images=images,
                 blob=blob, store=store, store_off=store_off, store_len=store_len, store_raw_len=store_raw_len,
                 store_pos_base=int(store_pos_base), store_ivs=store_ivs, req_status=req_status)
        read_rows = [int(r) for r in np.flatnonzero((route == ROUTE_MATERIALISE) & (cnt >= 1))]
        rest = [int(r) for r in np.flatnonzero(((route == ROUTE_MATERIALISE) & (cnt < 1)) | (route == ROUTE_FULL))]
        run_idx = np.flatnonzero(route[pc.run_row] == ROUTE_ACCEL)
        r1 = self._round(c, read_rows + rest, read_rows, run_idx, int(pos_base), ivs, mark)
        row_code[np.asarray(r1["failed"], np.int64)] |= WRITE_READ
        over = []
        if r1["arcs"] is not None:
            arcs = r1["arcs"]
            res.archives.append(arcs)
            res.pos_bases.append(int(pos_base))
            nR, nWb = len(run_idx), r1["nWb"]
            merged = status = ins = None
            if nR:
                rl = pc.run_len[run_idx]
                per_run = np.asarray([self._slot_cap(int(v)) for v in rl]) if len(set(rl.tolist())) <= 64 else \
                    np.full(nR, self._slot_cap(int(rl.max())))
                ins, run_first = inserts_from_runs(r1["out"], nWb, rl, r1["loc"], pc.run_row[run_idx], pc.run_pos[run_idx],
                                                   nrows, CL, int(per_run.sum()), dev, device=self.device)
                grouped, ins_first = group_inserts(ins, nrows)
                per_row = cnt.astype(np.int64).copy()
                np.add.at(per_row, pc.run_row[run_idx], 2 * per_run)
                merged, dupm, status = insert_pairs(pairs, grouped, ins_first, CL, pair_cap(sl, self.hash_len),
                                                    max(int(per_row.max()), 1), self.device)
                mark("insert")
                got = torch.cat([r1["ovf"], run_first[-1:], status.to(torch.int32)]).tolist()  # a host read
            else:
                got = r1["ovf"].tolist() + [0]
            if got[0]:
                raise _lib.SdfsCdcError(_lib.ECAP, f"a whole buffer's image does not fit a slot of {sl} bytes")
            self._replace(c, r1)
            if nR:
                total, mst = int(got[1]), np.asarray(got[2:])
                if total > ins.cap:
                    raise _lib.SdfsCdcError(_lib.ECAP, f"{total} inserts, room for {ins.cap}")
                is_accel = route == ROUTE_ACCEL
                ok = is_accel & (mst == 0)
                ovr = is_accel & (mst == EXT_OVERFLOW)
                row_code[is_accel & ~ok & ~ovr] |= WRITE_SLOT
                route[ovr] = ROUTE_ACCEL_MATERIALISE
                over = [int(r) for r in np.flatnonzero(ovr)]
                ok_d = torch.from_numpy(ok).to(dev)
                emit_pairs(merged, images, sl, dup=dupm, status=(~ok_d).to(torch.int32), device=self.device)
                ok_rows = torch.from_numpy(np.flatnonzero(ok)).to(dev)
                slots2d[rows_d[ok_rows]] = images[ok_rows]
                mark("emit_pairs")
                _move_claims(self.index, pairs, merged, ok_d, minus=(ins.hash[:total], ins.hashloc[:total]))
                res.info.update(n_inserts=total, insert_status=mst, run_hash=ins.hash[:total],
                                run_hashloc=ins.hashloc[:total], run_first=run_first)
                base = r1["counts"][:nWb].sum() if nWb else 0
                res.info["run_dup"] = r1["dup"][base + torch.arange(total, device=dev)]
            mark("claims")
        if over:  # the overflow round: exactly those rows, from the old image and the old store
            pb2 = int(pos_base) + int(res.archives[0].store_off.shape[0])
            r2 = self._round(c, over, over, np.zeros(0, np.int64), pb2, None, mark)
            row_code[np.asarray(r2["failed"], np.int64)] |= WRITE_READ
            if r2["arcs"] is not None:
                if int(r2["ovf"].item()):
                    raise _lib.SdfsCdcError(_lib.ECAP, f"a whole buffer's image does not fit a slot of {sl} bytes")
                res.archives.append(r2["arcs"])
                res.pos_bases.append(pb2)
                self._replace(c, r2)
            mark("overflow_round")
        if row_code.any():
            host = np.zeros(max(n_req, 1), np.int32)
            np.bitwise_or.at(host, pc.req, row_code[pc.row])
            req_status |= torch.from_numpy(host[:n_req]).to(dev)
        res.row_route = route
        res.info["row_status"] = row_code
        return res

    def write_file(self, map_slots, nslots: int, slot_len: int, file_len: int, file_pos: int, data, pos_base: int,
                   store, store_off, store_len, store_raw_len, store_pos_base: int, accel: bool = True, store_ivs=None,
                   ivs=None) -> WriteResult:
        """One ``DedupFileChannel.writeFile(data, len(data), file_pos)`` on a file that owns the whole
        image (data: host bytes or a device uint8 tensor).  ``result.file_len[0]`` is the file's new
        length.  Raises :class:`SdfsCdcError` when the request's status is not 0, as the Java call
        throws."""
        import numpy as np
        import torch

        if not isinstance(data, torch.Tensor):
            data = torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).to(map_slots.device)
        res = self.write_ranges(map_slots, nslots, slot_len, [(0, nslots, file_len)], [(0, file_pos, int(data.numel()), 0)],
                                data, pos_base, store, store_off, store_len, store_raw_len, store_pos_base, accel=accel,
                                store_ivs=store_ivs, ivs=ivs)
        st = int(res.status[0].item())
        if st:
            raise _lib.SdfsCdcError(st, f"write of [{file_pos}, {file_pos + int(data.numel())}) failed: "
                                        f"status {st:#x} (SDFS_CDC_WRITE_* bits)")
        return res
