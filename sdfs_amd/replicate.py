"""A map file of another volume becomes a file of this one, on the MI355X (include/sdfs_import.h;
DESIGN.md §24).

What ``GetCloudFile.checkDedupFile`` (GetCloudFile.java:184-249, "Importing hashes for file") and
``LongByteArrayMap.index()`` (LongByteArrayMap.java:310-356, 884-890) do with a ``.map`` /
``.map.lz4`` that came from elsewhere: every pair's fingerprint is put with one reference and its
hashloc rewritten to where the fingerprint lives HERE.  A hashloc is a volume's own insertion rank,
so a foreign image means nothing until every pair is re-homed; a chunk the destination lacks is
fetched from the source's store (decrypt under the source's key -> decode), stored through the
destination's own codec and cipher, and counted once per pair that names it.

* :class:`SourceVolume` — the source's store and the directory the read path takes.
* :class:`HipFileImport` — ``import_slots`` for a batch of slot images, ``import_file`` for a whole
  map, ``import_file_compressed`` for a ``.map.lz4``.

A request goes in whole or not at all: any status bit and it moves no count, inserts nothing and
its destination slot keeps every byte.  PyTorch allocates HBM and hands over the stream; every
step runs the library's HIP kernels.  No call reads back to the host except the fetch's one
scratch-size read and the archive plan's.  No CPU fallback: a failure raises
:class:`SdfsCdcError`.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from types import SimpleNamespace

from . import _lib
from ._lib import IMPORT_EFETCH, IMPORT_EHASH, IMPORT_EMISSING, READ_CORRUPT, check, ptr, stream_of  # noqa: F401
from .ingest import check_destinations
from .read import pair_cap


@dataclass
class SourceVolume:
    """The volume the map file comes from: ``store`` holds its putChunk records, the record of
    hashloc ``pos_base + k`` at ``store[store_off[k] : + store_len[k]]``, its chunk
    ``store_raw_len[k]`` bytes long (a dropped entry has length 0).  aes: its cipher (a
    :class:`sdfs_amd.aes.HipEncryptUtils` or the key bytes), with ``store_ivs`` uint8 [K, 16], the IV
    of each directory entry's record, or ``iv``, one for all."""

    store: object
    store_off: object      # int64 [K]
    store_len: object      # int32 [K]
    store_raw_len: object  # int32 [K]
    pos_base: int
    aes: object = None
    store_ivs: object = None
    iv: object = None
    hash_len: int = 32

    @classmethod
    def from_archives(cls, arcs, pos_base: int, aes=None) -> "SourceVolume":
        """From the :class:`sdfs_amd.archive.ArchiveSet` of the write (or reopen) that made the store."""
        off, ln, raw = arcs.directory()
        return cls(arcs.store, off, ln, raw, int(pos_base), aes, arcs.record_ivs() if aes is not None else None,
                   None, int(arcs.hash_len))

    @property
    def n_src(self) -> int:
        return int(self.store_len.shape[0])


@dataclass
class ImportResult:
    """What an import did (device tensors; reading a property waits for the device)."""

    status: object      # int32 [nreq]: 0, or READ_CORRUPT / IMPORT_EMISSING / IMPORT_EFETCH / IMPORT_EHASH bits
    req_missed: object  # int32 [nreq]: wanted pairs that name no source directory entry
    pair_rec: object    # int32 [nreq, pair_stride]: the pair's fingerprint record, -1 without one
    counts: object      # int64 [8]: records, held, fetches, raw bytes fetched, accepted, rejected, hashloc changed, missed
    released: object    # SlotClaims of the slots that were replaced
    file_len: object    # int64 [1]: max(old, slot * chunk_length + len) over the accepted requests

    records = property(lambda self: int(self.counts[0].item()))
    held = property(lambda self: int(self.counts[1].item()))
    fetches = property(lambda self: int(self.counts[2].item()))
    fetched_bytes = property(lambda self: int(self.counts[3].item()))
    accepted = property(lambda self: int(self.counts[4].item()))
    rejected = property(lambda self: int(self.counts[5].item()))
    changed = property(lambda self: int(self.counts[6].item()))
    missed = property(lambda self: int(self.counts[7].item()))


class HipFileImport:
    """writer: the destination's :class:`sdfs_amd.archive.HipBufferWriter` (its index, codec, cipher
    and archiver are the ones the fetched chunks go through); chunk_length: Main.CHUNK_LENGTH, the
    file bytes of one map slot and the longest chunk a source record may hold; engine: the hash
    engine ``verify`` fingerprints with."""

    def __init__(self, writer, chunk_length: int, engine=None, device: int = 0):
        self._lib = _lib.load()
        self.writer, self.index, self.engine = writer, writer.index, engine
        self.hash_len, self.chunk_length, self.device = int(writer.hash_len), int(chunk_length), int(device)
        if not 1 <= self.chunk_length < 1 << 31:
            raise ValueError("chunk_length: 1 .. 2^31 - 1")
        if self.hash_len not in (16, 32):
            raise ValueError("hash_len: HashLocPair holds 32 (SHA-256) or 16 (MD5) bytes")
        self._readers = {}

    def destroy(self) -> None:
        for rd in self._readers.values():
            rd.destroy()
        self._readers = {}

    def _reader(self, src: SourceVolume):
        """The read path's fetch under the source's cipher (one per cipher, kept)."""
        from .read import HipBufferReader

        key = id(src.aes) if src.aes is not None else None
        if key not in self._readers:
            self._readers[key] = HipBufferReader(self.chunk_length, self.hash_len, self.device, aes=src.aes,
                                                 iv=src.iv, record_ivs=src.aes is not None)
        rd = self._readers[key]
        rd.iv = src.iv
        return rd

    def _check(self, src: SourceVolume, verify: bool) -> None:
        import torch

        if int(src.hash_len) != self.hash_len:
            raise ValueError(f"the source's hashes hold {src.hash_len} bytes, the destination's {self.hash_len}")
        if verify and self.engine is None:
            raise ValueError("verify needs the hash engine")
        if src.aes is not None and src.store_ivs is None and src.iv is None:
            raise ValueError("an encrypted source needs store_ivs or the archive's IV")
        for name, dt in (("store", torch.uint8), ("store_off", torch.int64), ("store_len", torch.int32),
                         ("store_raw_len", torch.int32)):
            t = getattr(src, name)
            if t.dtype != dt or not t.is_contiguous():
                raise ValueError(f"SourceVolume.{name}: a contiguous {dt} tensor")
        if src.store_off.shape[0] != src.n_src or src.store_raw_len.shape[0] != src.n_src:
            raise ValueError("the source directory's three tensors hold one entry per record")

    def import_slots(self, src: SourceVolume, images, dests, lens, file_map, slot_len: int, file_len: int,
                     pos_base: int, verify: bool = False, ivs=None, stages=None):
        """Request r = {images[r]: a slot image of the source (host bytes; or all of them as one
        device tensor uint8 [nreq, slot_len]), dests[r]: its slot number in ``file_map`` (device uint8
        [nslots * slot_len], written in place), lens[r]: ``sp.len``}.  pos_base: where the
        fingerprints the destination lacked are inserted; ivs: the new archives' IVs (an encrypted
        destination; default random).  verify: fingerprint every fetched chunk and refuse
        (``IMPORT_EHASH``) a request with a pair whose hash is not its chunk's; without it the source's
        hash is trusted, as the reference does.  ``stages``: optional callable(name) called after
        each stage is enqueued (measurements).  Returns (:class:`ImportResult`,
        :class:`sdfs_amd.archive.ArchiveSet` of the chunks that were stored, directory indexed by
        ``hashloc - pos_base``).  Raises ``ValueError`` before the device is touched unless the
        destinations are distinct and inside the map and both sides use the same hash."""
        import numpy as np
        import torch

        mark = stages or (lambda name: None)
        slot_len = int(slot_len)
        self._check(src, verify)
        if file_map.dtype != torch.uint8 or not file_map.is_contiguous() or file_map.numel() % slot_len:
            raise ValueError("the file's map is a contiguous uint8 tensor of whole slots")
        nslots = file_map.numel() // slot_len
        dests = check_destinations(dests, nslots)
        nreq = len(dests)
        if len(images) != nreq or len(lens) != nreq:
            raise ValueError("one image and one length per request")
        lens = [int(v) for v in lens]
        if any(v < 0 or v >= 1 << 32 for v in lens):
            raise ValueError("a request's len is an unsigned 32-bit value")
        dev = file_map.device
        stride = max(pair_cap(slot_len, self.hash_len), 1)
        if isinstance(images, torch.Tensor):
            if images.dtype != torch.uint8 or images.dim() != 2 or images.shape[1] != slot_len:
                raise ValueError(f"device images: uint8 [nreq, {slot_len}]")
            req = images.contiguous()
        else:
            host = np.zeros((max(nreq, 1), slot_len), np.uint8)
            for r, img in enumerate(images):
                img = bytes(img)
                if len(img) > slot_len:
                    raise ValueError(f"request {r}: an image of {len(img)} bytes does not fit a slot of {slot_len}")
                host[r, : len(img)] = np.frombuffer(img, np.uint8)
            req = torch.from_numpy(host).to(dev)
        s = stream_of(file_map, None)
        places = max(nreq * stride, 1)
        e = lambda k, dt: torch.empty(max(int(k), 1), dtype=dt, device=dev)  # noqa: E731
        wt = dict(hashes=torch.empty((places, 32), dtype=torch.uint8, device=dev), src_hashloc=e(places, torch.int64),
                  counting=e(places, torch.uint8), status=e(nreq, torch.int32), req_pairs=e(nreq, torch.int32),
                  req_missed=e(nreq, torch.int32), pair_fetch=e(places, torch.int32), pair_rec=e(places, torch.int32),
                  counts=torch.zeros(8, dtype=torch.int64, device=dev))
        work = _lib.ImportWork(**{k: v.data_ptr() for k, v in wt.items()})
        L, W = self._lib, ctypes.byref(work)
        check(L.sdfs_cdc_import_pairs(self.device, req.data_ptr() if nreq else None, nreq, slot_len, self.hash_len,
                                      stride, W, s))
        mark("pairs")
        pos = self.index.get_digests(wt["hashes"][: nreq * stride])[0] if nreq else e(1, torch.int64)
        mark("index_get")
        n_src = src.n_src
        d = lambda dt: e(n_src, dt)  # noqa: E731
        plan = dict(pair_fetch=wt["pair_fetch"], fetch_count=torch.zeros(1, dtype=torch.int32, device=dev),
                    src_off=d(torch.int64), src_len=d(torch.int32), dst_off=d(torch.int64), dst_cap=d(torch.int32),
                    plain_off=d(torch.int64), total_bytes=torch.zeros(2, dtype=torch.int64, device=dev))
        p = lambda t: t.data_ptr() if n_src else None  # noqa: E731
        check(L.sdfs_cdc_import_plan(self.device, nreq, stride, W, pos.data_ptr(), int(src.pos_base), n_src,
                                     p(src.store_off), p(src.store_len), p(src.store_raw_len), self.chunk_length,
                                     plan["fetch_count"].data_ptr(), p(plan["src_off"]), p(plan["src_len"]),
                                     p(plan["dst_off"]), p(plan["dst_cap"]), p(plan["plain_off"]),
                                     plan["total_bytes"].data_ptr(), s))
        mark("plan")
        # the read path's fetch, unchanged: decrypt under the source's key and IVs -> chain_lens -> framed decode
        k, chunks, _, fetch_len = self._reader(src)._fetch(SimpleNamespace(hashloc=wt["src_hashloc"]), plan, src.store,
                                                           int(src.pos_base), src.store_ivs, mark)
        recs = torch.zeros(places, _lib.RECORD_BYTES, dtype=torch.uint8, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        pk = lambda t: t.data_ptr() if k else None  # noqa: E731
        check(L.sdfs_cdc_import_records(self.device, self.engine._h if verify else None, nreq, stride, self.hash_len, W,
                                        plan["fetch_count"].data_ptr(), k, pk(chunks), pk(plan["dst_off"]),
                                        pk(plan["dst_cap"]), pk(fetch_len), recs.data_ptr(), count.data_ptr(), s))
        mark("records")
        dup, loc, new, nc = self.index.put_records(recs, count, pos_base=pos_base)
        mark("put_records")
        arcs = self.writer.store_new(chunks, chunks.numel() - 64, recs, new, nc, ivs=ivs, buf_offs=plan["dst_off"])
        mark("store")
        status = wt["status"][:nreq]
        dd = torch.tensor(dests, dtype=torch.int64, device=dev)
        sel = torch.zeros(max(nslots, 1), dtype=torch.uint8, device=dev)
        sel[dd] = (status == 0).to(torch.uint8)
        released = self.index.claim_slots(file_map, nslots, slot_len, -1, sel=sel[:nslots], hash_len=self.hash_len)
        mark("release")
        flen = torch.tensor([int(file_len)], dtype=torch.int64, device=dev)
        dl = torch.tensor(lens, dtype=torch.int64, device=dev).to(torch.int32) if nreq else e(1, torch.int32)
        check(L.sdfs_cdc_import_install(self.device, req.data_ptr() if nreq else None, nreq, slot_len, self.hash_len,
                                        stride, W, loc.data_ptr() if nreq else None, dd.data_ptr() if nreq else None,
                                        dl.data_ptr() if nreq else None, self.chunk_length,
                                        file_map.data_ptr() if nreq else None, nslots, flen.data_ptr(), s))
        mark("install")
        arcs.extra.update(dup=dup, hashloc=loc, new_list=new[: arcs.n_rec], records=recs, count=count, plan=plan,
                          chunks=chunks, fetch_len=fetch_len, n_fetch=k, work=wt, requests=req)
        res = ImportResult(status, wt["req_missed"][:nreq], wt["pair_rec"][: nreq * stride].view(nreq, stride),
                           wt["counts"], released, flen)
        return res, arcs

    def import_file(self, src: SourceVolume, src_map, nslots: int, slot_len: int, src_file_len: int, pos_base: int,
                    verify: bool = False, ivs=None, stages=None):
        """The whole map file ``src_map`` (device uint8, nslots slots of slot_len bytes, the file
        ``src_file_len`` bytes long) into a fresh destination map: ``dests = 0 .. nslots - 1``.
        Returns (file_map uint8 [nslots * slot_len], :class:`ImportResult`, ArchiveSet)."""
        import torch

        nslots, slot_len = int(nslots), int(slot_len)
        if src_map.numel() < nslots * slot_len:
            raise ValueError(f"map holds {src_map.numel()} bytes, {nslots} slots of {slot_len} need more")
        file_map = torch.zeros(nslots * slot_len, dtype=torch.uint8, device=src_map.device)
        cl = self.chunk_length
        lens = [max(0, min(cl, int(src_file_len) - b * cl)) for b in range(nslots)]
        images = src_map[: nslots * slot_len].view(nslots, slot_len)
        res, arcs = self.import_slots(src, images, list(range(nslots)), lens, file_map, slot_len, 0, pos_base,
                                      verify=verify, ivs=ivs, stages=stages)
        return file_map, res, arcs

    def import_file_compressed(self, codec, image, src: SourceVolume, slot_len: int, src_file_len: int, pos_base: int,
                               verify: bool = False, ivs=None, stages=None):
        """A ``.map.lz4`` image (device uint8; ``codec``: a
        :class:`sdfs_amd.lz4_stream.HipLz4BlockStream`) opened by :func:`sdfs_amd.mapfile.open_map`, then
        :meth:`import_file`."""
        from .mapfile import open_map

        m, nslots = open_map(codec, image, int(slot_len))
        return self.import_file(src, m, nslots, slot_len, src_file_len, pos_base, verify=verify, ivs=ivs,
                                stages=stages)
