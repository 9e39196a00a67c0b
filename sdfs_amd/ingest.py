"""Client-side dedup on the MI355X (include/sdfs_ingest.h): the server half of
``checkHashes``, ``writeChunks`` and ``writeSparseDataChunk`` (StorageServiceImpl.java:175-382) for
batches.

A remote client runs ``getChunks`` itself, asks which fingerprints the server holds, sends only the
chunks that are missing and then each buffer's ``SparseDataChunk``.  :class:`HipChunkIngest` takes
those three requests in batches and leaves the index, the archives and the file's map exactly as
the same data written through :meth:`sdfs_amd.archive.HipBufferWriter.write` leaves them.

PyTorch allocates HBM and hands over the stream; every step runs the library's HIP kernels.  No
call of the front end reads anything back to the host (the store tail keeps the archive plan's one
host read), and there is no CPU fallback: a failure raises
:class:`SdfsCdcError`.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

from . import _lib
from ._lib import (INGEST_EBOUNDS, INGEST_EDECODE, INGEST_EHASH, INGEST_EMISSED, INGEST_EMPTY,  # noqa: F401
                   READ_CORRUPT, check, stream_of)
from .read import pair_cap


@dataclass
class ChunkBatch:
    """The entries of one ``writeChunks`` request on the device: entry i = {hash[i] (zero-padded to
    32 bytes), blob[off[i] : off[i] + len[i]], raw_len[i] (its uncompressed length; ChunkEntry's
    ``compressedLength``), compressed[i]}.  raw_total: the host-known sum of raw_len, which sizes the
    staging area."""

    hash: object        # uint8 [n, 32]
    blob: object        # uint8
    off: object         # int64 [n]
    len: object         # int32 [n]
    raw_len: object     # int32 [n]
    compressed: object  # uint8 [n]
    raw_total: int

    @property
    def n(self) -> int:
        return int(self.len.shape[0])


def pack_entries(entries, device, align: int = 1) -> ChunkBatch:
    """entries: host [(hash bytes, payload bytes, compressed, raw_len)] -> a :class:`ChunkBatch`
    whose blob holds the payloads one after another (each at a multiple of ``align``)."""
    import numpy as np
    import torch

    n = len(entries)
    hashes = np.zeros((max(n, 1), 32), np.uint8)
    off, ln, raw, comp = (np.zeros(max(n, 1), dt) for dt in (np.int64, np.int32, np.int32, np.uint8))
    parts, at = [], 0
    for i, (h, payload, c, r) in enumerate(entries):
        h, payload = bytes(h), bytes(payload)
        if len(h) > 32:
            raise ValueError("fingerprints are at most 32 bytes")
        if not 0 <= int(r) < 1 << 31 or len(payload) >= 1 << 31:
            raise ValueError("a chunk is shorter than 2 GiB")
        pad = -at % max(int(align), 1)
        parts.append(bytes(pad) + payload)
        at += pad
        hashes[i, : len(h)] = np.frombuffer(h, np.uint8)
        off[i], ln[i], raw[i], comp[i] = at, len(payload), int(r), 1 if c else 0
        at += len(payload)
    blob = np.frombuffer(b"".join(parts) + bytes(16), np.uint8)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a[:n])).to(device)  # noqa: E731
    return ChunkBatch(up(hashes), torch.from_numpy(blob.copy()).to(device), up(off), up(ln), up(raw), up(comp),
                      int(raw[:n].astype(np.int64).sum()))


def check_destinations(dests, nslots: int) -> list:
    """The destination slots of a ``write_sparse_data_chunks`` batch: distinct, non-negative and
    inside the file's map, or ``ValueError``."""
    out = [int(d) for d in dests]
    for d in out:
        if d < 0 or d >= int(nslots):
            raise ValueError(f"destination slot {d} is outside the map's {int(nslots)} slots")
    if len(set(out)) != len(out):
        raise ValueError("two requests of the batch name the same destination slot")
    return out


@dataclass
class SparseWrites:
    """What ``write_sparse_data_chunks`` did (device tensors; reading a property waits for the device)."""

    status: object      # int32 [nreq]: 0, INGEST_EMISSED or READ_CORRUPT
    req_missed: object  # int32 [nreq]
    miss_list: object   # int32 [miss_cap, 2]: {request, pair}; the first counts[5] rows, in no order
    counts: object      # int64 [6]: added, missed, skipped as inserted, accepted, rejected, misses listed
    released: object    # SlotClaims of the slots that were replaced (None when the index call stands alone)
    file_len: object    # int64 [1]: max(old, slot * chunk_length + len) over the accepted requests

    added = property(lambda self: int(self.counts[0].item()))
    missed = property(lambda self: int(self.counts[1].item()))
    skipped = property(lambda self: int(self.counts[2].item()))
    accepted = property(lambda self: int(self.counts[3].item()))
    rejected = property(lambda self: int(self.counts[4].item()))
    listed = property(lambda self: int(self.counts[5].item()))

    def misses(self):
        """Sorted [(request, pair)] of the listed misses (a host read)."""
        return sorted(tuple(r) for r in self.miss_list[: self.listed].tolist())


class HipChunkIngest:
    """writer: the store's :class:`sdfs_amd.archive.HipBufferWriter` (its index, its LZ4 handle, its
    archiver and cipher are the ones the client's chunks go through); chunk_length:
    Main.CHUNK_LENGTH, the longest chunk a client may send and the file bytes of one map slot;
    engine: the hash engine ``verify`` fingerprints with."""

    def __init__(self, writer, chunk_length: int, engine=None, device: int = 0):
        self._lib = _lib.load()
        self.writer, self.index, self.engine = writer, writer.index, engine
        self.hash_len, self.chunk_length, self.device = int(writer.hash_len), int(chunk_length), int(device)
        if not 1 <= self.chunk_length < 1 << 31:
            raise ValueError("chunk_length: 1 .. 2^31 - 1")

    # ---- checkHashes (StorageServiceImpl.java:175-211)
    def check_hashes(self, digests, stream=None):
        """digests: device uint8 [n, 32] (zero-padded) or a host list of hashes -> int64 [n]: where
        each fingerprint lives, -1 where the index does not hold it.  A fingerprint whose count is
        <= 0 but that no sweep has removed yet is held (``put_records`` would find it too)."""
        if isinstance(digests, (list, tuple)):
            import torch

            digests = (self.index._digest_tensor(list(digests)) if len(digests) else
                       torch.empty((0, 32), dtype=torch.uint8, device=f"cuda:{self.device}"))
        return self.index.get_digests(digests.contiguous(), stream)[0]

    # ---- writeChunks (StorageServiceImpl.java:214-272)
    def _plan(self, b: ChunkBatch, dev):
        import torch

        n = max(b.n, 1)
        i32 = lambda k=n: torch.empty(k, dtype=torch.int32, device=dev)  # noqa: E731
        i64 = lambda k=n: torch.empty(k, dtype=torch.int64, device=dev)  # noqa: E731
        t = dict(status=i32(), stage_off=i64(), rec_of=i32(), dec_src_off=i64(), dec_src_len=i32(), dec_dst_off=i64(),
                 dec_cap=i32(), dec_len=i32(), dec_entry=i32(), dec_count=i32(1), staged=i64(1))
        return t, _lib.IngestPlan(**{k: v.data_ptr() for k, v in t.items()})

    def write_chunks(self, entries, pos_base: int, verify: bool = False, ivs=None, stream=None):
        """entries: a :class:`ChunkBatch`, or the host list :func:`pack_entries` takes.  Returns
        (inserted uint8 [n], pos int64 [n], stored_len int32 [n], status int32 [n],
        :class:`sdfs_amd.archive.ArchiveSet`): per entry the ``InsertRecord`` of its put — pos -1 for
        an empty or rejected entry, stored_len the stored record's length where the entry inserted —
        and the archives the new chunks went into (directory indexed by ``pos - pos_base``).
        verify: refuse (``INGEST_EHASH``) an entry whose chunk does not have the client's hash."""
        import torch

        dev = torch.device(f"cuda:{self.device}")
        b = entries if isinstance(entries, ChunkBatch) else pack_entries(entries, dev)
        n = b.n
        if verify and self.engine is None:
            raise ValueError("verify needs the hash engine")
        for name, dt in (("hash", torch.uint8), ("blob", torch.uint8), ("off", torch.int64), ("len", torch.int32),
                         ("raw_len", torch.int32), ("compressed", torch.uint8)):
            t = getattr(b, name)
            if t.dtype != dt or not t.is_contiguous() or (name not in ("blob", "hash") and int(t.shape[0]) != n):
                raise ValueError(f"ChunkBatch.{name}: a contiguous {dt} tensor, one element per entry")
        s = stream_of(b.blob, stream)
        cb = _lib.IngestBatch(hash=b.hash.data_ptr(), blob=b.blob.data_ptr(), blob_bytes=int(b.blob.numel()),
                              off=b.off.data_ptr(), len=b.len.data_ptr(), raw_len=b.raw_len.data_ptr(),
                              compressed=b.compressed.data_ptr(), n=n)
        pt, cp = self._plan(b, dev)
        stage_cap = int(b.raw_total)
        stage = torch.empty(stage_cap + 16, dtype=torch.uint8, device=dev)
        recs = torch.zeros(max(n, 1), _lib.RECORD_BYTES, dtype=torch.uint8, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        L, B, P = self._lib, ctypes.byref(cb), ctypes.byref(cp)
        check(L.sdfs_cdc_ingest_chunks_plan(self.device, B, self.chunk_length, stage_cap, P, s))
        check(L.sdfs_cdc_ingest_chunks_decode(self.writer._z._h, B, P, stage.data_ptr(), s))
        check(L.sdfs_cdc_ingest_chunks_copy(self.device, B, P, self.chunk_length, stage.data_ptr(), s))
        if verify:
            check(L.sdfs_cdc_ingest_chunks_verify(self.engine._h, B, P, stage.data_ptr(), self.hash_len, s))
        check(L.sdfs_cdc_ingest_chunks_records(self.device, B, P, recs.data_ptr(), count.data_ptr(), s))
        dup, loc, new, nc = self.index.put_records(recs, count, pos_base=pos_base, stream=stream)
        arcs = self.writer.store_new(stage, stage_cap, recs, new, nc, ivs=ivs, buf_offs=pt["stage_off"])
        inserted = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        pos = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        stored = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        check(L.sdfs_cdc_ingest_chunks_results(self.device, B, P, dup.data_ptr(), loc.data_ptr(), int(pos_base),
                                               arcs.rec_len.data_ptr() if arcs.n_rec else None, arcs.n_rec,
                                               inserted.data_ptr(), pos.data_ptr(), stored.data_ptr(),
                                               status.data_ptr(), s))
        arcs.extra.update(dup=dup, hashloc=loc, new_list=new[: arcs.n_rec], rec_of=pt["rec_of"][:n], stage=stage,
                          stage_off=pt["stage_off"][:n], staged=pt["staged"], batch=b, plan=(cb, cp, pt))
        return inserted[:n], pos[:n], stored[:n], status[:n], arcs

    # ---- writeSparseDataChunk (StorageServiceImpl.java:275-382)
    def addref_slots(self, req, nreq: int, slot_len: int, inserted=None, miss_cap: int = 1024,
                     stream=None) -> SparseWrites:
        """``sdfs_cdc_index_addref_slots`` alone: req device uint8 [nreq * slot_len] images, inserted
        device uint8 [nreq, pair_cap(slot_len)] or None.  Nothing but the index's counts changes."""
        import torch

        if req.dtype != torch.uint8 or not req.is_contiguous() or req.numel() < nreq * slot_len:
            raise ValueError(f"the requests are a contiguous uint8 tensor of {nreq} images of {slot_len} bytes")
        dev = req.device
        stride = pair_cap(slot_len, self.hash_len)
        if inserted is not None:
            inserted = inserted.to(device=dev, dtype=torch.uint8).contiguous()
            if inserted.numel() != nreq * stride:
                raise ValueError(f"inserted: {nreq} rows of {stride} flags")
        miss_cap = int(miss_cap)
        status = torch.empty(max(nreq, 1), dtype=torch.int32, device=dev)
        missed = torch.empty(max(nreq, 1), dtype=torch.int32, device=dev)
        miss_list = torch.empty(max(miss_cap, 1), 2, dtype=torch.int32, device=dev)
        counts = torch.empty(6, dtype=torch.int64, device=dev)
        check(self._lib.sdfs_cdc_index_addref_slots(
            self.index._h, req.data_ptr() if nreq else None, int(nreq), int(slot_len), self.hash_len,
            _lib.ptr(inserted), stride, status.data_ptr(), missed.data_ptr(), miss_list.data_ptr(), miss_cap,
            counts.data_ptr(), stream_of(req, stream)))
        return SparseWrites(status[:nreq], missed[:nreq], miss_list, counts, None, None)

    def write_sparse_data_chunks(self, file_map, slot_len: int, dests, images, lens, file_len: int, inserted=None,
                                 miss_cap: int = 1024, stream=None) -> SparseWrites:
        """file_map: the file's map, device uint8 [nslots * slot_len], written in place.  Request r =
        {dests[r]: its slot number (``fileLocation / chunk_length``), images[r]: its
        ``SparseDataChunk.getBytes`` image (host bytes; or all of them as one device tensor), lens[r]:
        ``sp.len``, inserted[r]: the flags
        of its pairs, by the pair's place in the image (None: none)}.  Every accepted request
        releases the pairs of the slot it replaces, is written there — image bytes, the rest of the
        slot zero — and moves the file length to ``max(old, dest * chunk_length + len)``; a
        rejected one changes nothing.  Raises ``ValueError`` unless the destinations are distinct,
        non-negative and inside the map."""
        import numpy as np
        import torch

        slot_len = int(slot_len)
        if file_map.dtype != torch.uint8 or not file_map.is_contiguous() or file_map.numel() % slot_len:
            raise ValueError("the file's map is a contiguous uint8 tensor of whole slots")
        nslots = file_map.numel() // slot_len
        dests = check_destinations(dests, nslots)
        nreq = len(dests)
        if len(images) != nreq or len(lens) != nreq or (inserted is not None and len(inserted) != nreq):
            raise ValueError("one image, one length and one row of flags per request")
        dev = file_map.device
        stride = pair_cap(slot_len, self.hash_len)
        if isinstance(images, torch.Tensor):  # on the device: uint8 [nreq, slot_len], flags uint8 [nreq, stride]
            if images.dtype != torch.uint8 or images.dim() != 2 or images.shape[1] != slot_len:
                raise ValueError(f"device images: uint8 [nreq, {slot_len}]")
            req, flags = images.contiguous(), inserted
        else:
            host = np.zeros((nreq, slot_len), np.uint8)
            flags = np.zeros((nreq, stride), np.uint8)
            for r, img in enumerate(images):
                img = bytes(img)
                if len(img) > slot_len:
                    raise ValueError(f"request {r}: an image of {len(img)} bytes does not fit a slot of {slot_len}")
                host[r, : len(img)] = np.frombuffer(img, np.uint8)
                if inserted is not None and inserted[r] is not None:
                    row = np.asarray(inserted[r], np.uint8)[:stride]
                    flags[r, : len(row)] = row != 0
            req = torch.from_numpy(host).to(dev)
            flags = torch.from_numpy(flags).to(dev) if inserted is not None else None
        out = self.addref_slots(req.view(-1), nreq, slot_len, flags, miss_cap, stream)
        d = torch.tensor(dests, dtype=torch.int64, device=dev)
        ok = out.status == 0
        sel = torch.zeros(nslots, dtype=torch.uint8, device=dev)
        sel[d] = ok.to(torch.uint8)
        out.released = self.index.claim_slots(file_map, nslots, slot_len, -1, sel=sel, hash_len=self.hash_len,
                                              stream=stream)
        slots = file_map.view(nslots, slot_len)
        slots[d] = torch.where(ok[:, None], req, slots[d])
        ends = d * self.chunk_length + torch.tensor([int(v) for v in lens], dtype=torch.int64, device=dev)
        ends = torch.where(ok, ends, torch.zeros_like(ends))
        out.file_len = torch.cat([ends, torch.tensor([int(file_len)], dtype=torch.int64, device=dev)]).max().view(1)
        return out
