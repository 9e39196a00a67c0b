"""Chunk store layer on the MI355X (include/sdfs_archive.h): archive images for new records,
their ``.map`` images, compaction after an index sweep.

What ``HashBlobArchive`` does between the write path's putChunk records and the read path's
directory: ``putChunk`` appends ``[BE32 hash.length][hash][BE32 len][record]`` to the open archive
(HashBlobArchive.java:1399-1411), closes it for a new one when it is full (:1305-1316,740-764),
keeps ``hash -> position`` in the archive's ``SimpleByteArrayLongMap``
(:1334-1350, SimpleByteArrayLongMap.java:427-539), and ``compact()`` (:2064-2186) rewrites an
archive with the records the index still holds.

* :class:`HipBlobArchiver` — a thin mirror of the C entry points: map_size, plan, pack, map_emit,
  compact.  Returns an :class:`ArchiveSet`.
* :class:`HipBufferWriter` — a batch of write buffers to archive images in one call (``write``),
  and a sweep's ``removed_pos`` to compacted images (``compact``).  ``ArchiveSet.directory()`` is
  what :meth:`sdfs_amd.read.HipBufferReader.read` takes.

PyTorch allocates HBM and hands over the stream; every step runs the library's HIP kernels.  No
CPU fallback: a failure raises :class:`SdfsCdcError`.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field

from . import _lib
from ._lib import ARCHIVE_ECAP, ARCHIVE_ESTORE, ARCHIVE_HEADER, ARCHIVE_NONE, check, ptr, stream_of  # noqa: F401

MAX_LEN = 1048576 * 20  # HashBlobArchive.MAX_LEN (HashBlobArchive.java:83)
LEN_VARIANCE = .25      # HashBlobArchive.LEN_VARIANCE (:86)


def map_size(sz: int) -> int:
    """NextPrime.getNextPrimeI (NextPrime.java:56-88); 0 where the reference throws."""
    return int(_lib.load().sdfs_cdc_archive_map_size(int(sz)))


def max_hm_sz(min_len: int, max_len: int = MAX_LEN) -> int:
    """HashBlobArchive.MAX_HM_SZ (HashBlobArchive.java:308-309)."""
    msz = int(max_len * LEN_VARIANCE) + max_len
    return int((msz // min_len) / .75)


def pack_span() -> int:
    """Bytes of the store one workgroup of the pack kernel writes."""
    return int(_lib.load().sdfs_cdc_archive_pack_span())


def map_bytes(map_slots: int, hash_len: int, version: int) -> int:
    return int(_lib.load().sdfs_cdc_archive_map_bytes(int(map_slots), int(hash_len), int(version)))


def _r16(n: int) -> int:
    return (int(n) + 15) // 16 * 16


class Layout:
    """``sdfs_cdc_archive_layout``: device tensors for n_max records and arc_cap archives."""

    def __init__(self, n_max: int, arc_cap: int, device):
        import torch

        e = lambda k, dt: torch.empty(max(int(k), 1), dtype=dt, device=device)  # noqa: E731
        self.n_max, self.arc_cap = int(n_max), max(int(arc_cap), 1)
        self.arc, self.pos, self.store_off = e(n_max, torch.int32), e(n_max, torch.int32), e(n_max, torch.int64)
        self.arc_first = e(self.arc_cap + 1, torch.int32)
        self.arc_bytes, self.arc_base = e(self.arc_cap, torch.int64), e(self.arc_cap, torch.int64)
        self.totals = torch.zeros(2, dtype=torch.int64, device=device)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self.c = _lib.ArchiveLayout(
            arc=self.arc.data_ptr(), pos=self.pos.data_ptr(), store_off=self.store_off.data_ptr(),
            arc_first=self.arc_first.data_ptr(), arc_bytes=self.arc_bytes.data_ptr(),
            arc_base=self.arc_base.data_ptr(), totals=self.totals.data_ptr(), status=self.status.data_ptr(),
            arc_cap=self.arc_cap, reserved=0)

    def read_totals(self, *more):
        """The one host read: (n_arc, store_bytes, status, *more[i][0])."""
        import torch

        vals = torch.cat([self.totals, self.status.to(torch.int64)] + [m.reshape(-1)[:1].to(torch.int64) for m in more])
        n_arc, store_bytes, status, *rest = (int(v) for v in vals.tolist())
        if status & ARCHIVE_ECAP:
            raise _lib.SdfsCdcError(_lib.ECAP, f"the batch needs more than {self.arc_cap} archives")
        return (n_arc, store_bytes, status, *rest)


@dataclass
class ArchiveSet:
    """The archives of one call.  ``store``: every image at ``arc_base[a]``, ``arc_bytes[a]`` long;
    ``store_off / store_len / raw_len``: the read path's directory, indexed by ``hashloc -
    pos_base`` of the write (a dropped entry has length 0); ``maps``: the ``.map`` images, one
    per row; ``slot_rec``: the record in each map slot (-1 = free)."""

    store: object       # uint8
    arc_base: object    # int64 [n_arc]
    arc_bytes: object   # int64 [n_arc]
    arc_first: object   # int32 [n_arc + 1]
    store_off: object   # int64 [K]
    store_len: object   # int32 [K]
    raw_len: object     # int32 [K]
    maps: object        # uint8 [n_arc, map_bytes(map_stride)]
    slot_rec: object    # int32 [n_arc, map_stride]
    n_arc: int
    store_bytes: int = 0
    n_rec: int = 0
    hash_len: int = 32
    version: int = 0
    header_bytes: int = 0
    map_stride: int = 0
    map_sizes: object = None   # int32 [n_arc] when the archives' maps differ in size (after compact)
    max_entries: int = 0       # no archive holds more records than this
    ivs: object = None         # uint8 [n_arc, 16]
    deleted: object = None     # after compact: uint8 [old n_arc]
    new_of_old: object = None  # after compact: int32 [old n_rec], -1 = dropped
    layout: Layout = None      # per-record arc / pos / store_off in record order
    rec_len: object = None     # int32 [n_rec] stored record lengths, record order
    rec_of_k: object = None    # int64 [K] directory entry -> record ordinal, -1 = dropped
    records: object = None     # the fingerprint table the digests come from
    sel: object = None         # int32 [n_rec] record -> fingerprint record (None: identity)
    extra: dict = field(default_factory=dict)  # "info": device int64[2] = duplicate keys refused, maps too full

    def directory(self):
        """The three tensors ``HipBufferReader.read`` takes after ``store``."""
        return self.store_off, self.store_len, self.raw_len

    def record_ivs(self):
        """uint8 [K, 16]: the IV each directory entry's record was encrypted under (``store_ivs`` of
        ``HipBufferReader.read``); None for a store without archive headers."""
        if self.ivs is None:
            return None
        rec = self.rec_of_k.clamp(min=0)
        return self.ivs[self.layout.arc[: max(self.n_rec, 1)].long()[rec]].contiguous()

    def image(self, a: int) -> bytes:
        """Archive a's file image (host bytes)."""
        b, n = int(self.arc_base[a].item()), int(self.arc_bytes[a].item())
        return self.store[b: b + n].cpu().numpy().tobytes()

    def map_image(self, a: int) -> bytes:
        """Archive a's ``.map`` file image (host bytes)."""
        size = int(self.map_sizes[a].item()) if self.map_sizes is not None else self.map_stride
        return self.maps[a, : map_bytes(size, self.hash_len, self.version)].cpu().numpy().tobytes()


class HipBlobArchiver:
    """plan / pack / map_emit / compact for device-resident records.

    version: HashBlobArchive.VERSION (0: no archive header, map values ``[BE32 pos]``; > 0: a
    1024-byte header with the archive's IV, map values ``[BE32 pos][BE32 len]``).  blocksz: one int or
    a list, archive a uses ``blocksz[min(a, len - 1)]`` (the reference draws nextSize() per
    archive).  map_slots: slots of every archive's map, default ``map_size(MAX_HM_SZ)``."""

    def __init__(self, hash_len: int = 32, version: int = 0, blocksz=MAX_LEN, map_slots: int | None = None,
                 min_len: int = 4095, device: int = 0):
        self._lib = _lib.load()
        self.hash_len, self.version, self.device = int(hash_len), int(version), int(device)
        self.header_bytes = ARCHIVE_HEADER if self.version > 0 else 0
        self.blocksz = [int(b) for b in (blocksz if isinstance(blocksz, (list, tuple)) else [blocksz])]
        self.map_slots = int(map_slots) if map_slots is not None else map_size(max_hm_sz(min_len))
        self.limit = int(self.map_slots * .75)

    # ---- the C entry points
    def plan(self, rec_len, count=None, arc_cap: int | None = None, header_bytes: int | None = None,
             stream=None, lay: Layout | None = None) -> Layout:
        """``sdfs_cdc_archive_plan``: rec_len int32[n] (device), count: optional device int32[1];
        lay: the layout to write into (default: a new one for arc_cap archives)."""
        n = int(rec_len.shape[0])
        if lay is None:
            lay = Layout(n, n if arc_cap is None else arc_cap, rec_len.device)
        blk = (ctypes.c_uint64 * len(self.blocksz))(*self.blocksz)
        hb = self.header_bytes if header_bytes is None else int(header_bytes)
        check(self._lib.sdfs_cdc_archive_plan(self.device, ptr(rec_len) if n else None, ptr(count), n, self.hash_len,
                                              hb, blk, len(self.blocksz), self.map_slots, ctypes.byref(lay.c),
                                              stream_of(rec_len, stream)))
        return lay

    def pack(self, lay: Layout, src, src_off, src_len, records, sel=None, count=None, ivs=None, store=None,
             store_bytes: int | None = None, raw_frame: bool = False, header_bytes: int | None = None, stream=None):
        """``sdfs_cdc_archive_pack`` into ``store`` (allocated when None: store_bytes rounded up to 16)."""
        import torch

        if store is None:
            store = torch.empty(_r16(store_bytes) + 16, dtype=torch.uint8, device=src.device)
        cap = store.numel() if store_bytes is None else int(store_bytes)
        hb = self.header_bytes if header_bytes is None else int(header_bytes)
        check(self._lib.sdfs_cdc_archive_pack(self.device, ctypes.byref(lay.c), ptr(count), int(src_len.shape[0]),
                                              src.data_ptr(), src_off.data_ptr(), src_len.data_ptr(), int(raw_frame),
                                              records.data_ptr(), ptr(sel), self.hash_len, hb, self.version,
                                              ptr(ivs), store.data_ptr(), cap, stream_of(src, stream)))
        return store

    def map_emit(self, lay: Layout, rec_len, records, sel=None, count=None, n_arc: int | None = None,
                 map_sizes=None, map_stride: int | None = None, stream=None):
        """``sdfs_cdc_archive_map_emit`` -> (maps uint8 [n_arc, map_bytes], slot_rec int32 [n_arc, stride],
        info int64[2] = duplicate keys, archives whose table was too full)."""
        import torch

        stride = int(map_stride or self.map_slots)
        rows = max(lay.arc_cap if n_arc is None else int(n_arc), 1)
        dev = rec_len.device
        maps = torch.empty((rows, map_bytes(stride, self.hash_len, self.version)), dtype=torch.uint8, device=dev)
        slot_rec = torch.empty((rows, stride), dtype=torch.int32, device=dev)
        info = torch.zeros(2, dtype=torch.int64, device=dev)
        c = _lib.ArchiveLayout.from_buffer_copy(lay.c)
        c.arc_cap = rows if n_arc is not None else lay.arc_cap
        check(self._lib.sdfs_cdc_archive_map_emit(self.device, ctypes.byref(c), ptr(count), int(rec_len.shape[0]),
                                                  rec_len.data_ptr(), records.data_ptr(), ptr(sel), self.hash_len,
                                                  self.version, ptr(map_sizes), stride, maps.data_ptr(),
                                                  slot_rec.data_ptr(), info.data_ptr(), stream_of(rec_len, stream)))
        return maps, slot_rec, info

    # ---- a batch of records to an ArchiveSet
    def archive(self, src, src_off, src_len, records, sel=None, count=None, rec_len=None, raw_len=None, ivs=None,
                arc_cap: int | None = None, raw_frame: bool = False, prepare=None) -> ArchiveSet:
        """plan -> (the one host read) -> pack -> map_emit.  rec_len: the stored lengths when they are
        known before the bytes exist (``prepare(layout)``, called after the plan, may then still
        write them: the cipher needs each record's archive for its IV); default src_len (+ 4 with
        raw_frame)."""
        import torch

        if rec_len is None:
            rec_len = src_len + 4 if raw_frame else src_len
        lay = self.plan(rec_len, count, arc_cap)
        if prepare is not None:
            prepare(lay)
        if count is not None:
            n_arc, store_bytes, _, k = lay.read_totals(count)
            k = min(k, int(rec_len.shape[0]))
        else:
            n_arc, store_bytes, _ = lay.read_totals()
            k = int(rec_len.shape[0])
        if self.header_bytes and ivs is None:
            raise ValueError("archives with a header need their IVs")
        store = self.pack(lay, src, src_off, src_len, records, sel, count, ivs, store_bytes=store_bytes,
                          raw_frame=raw_frame)
        maps, slot_rec, info = self.map_emit(lay, rec_len, records, sel, count, n_arc=n_arc)
        dev = rec_len.device
        return ArchiveSet(
            store=store, arc_base=lay.arc_base[:n_arc], arc_bytes=lay.arc_bytes[:n_arc],
            arc_first=lay.arc_first[: n_arc + 1], store_off=lay.store_off[:k], store_len=rec_len[:k],
            raw_len=raw_len[:k] if raw_len is not None else torch.zeros(k, dtype=torch.int32, device=dev),
            maps=maps, slot_rec=slot_rec, n_arc=n_arc, store_bytes=store_bytes, n_rec=k, hash_len=self.hash_len,
            version=self.version, header_bytes=self.header_bytes, map_stride=self.map_slots,
            max_entries=min(self.limit, max(k, 1)), ivs=ivs[:n_arc] if ivs is not None else None, layout=lay,
            rec_len=rec_len[:k], rec_of_k=torch.arange(k, dtype=torch.int64, device=dev), records=records,
            sel=sel[:k] if sel is not None else None, extra={"info": info})

    def compact(self, arcs: ArchiveSet, keep, new_ivs=None, aes=None) -> ArchiveSet:
        """``HashBlobArchive.compact()`` for every archive of ``arcs``: keep uint8[n_rec] (device), 1 =
        the index still holds the record's key.  With archive headers (version > 0): new_ivs uint8
        [n_arc, 16] and aes, the store's :class:`sdfs_amd.aes.HipEncryptUtils`; the records are
        decrypted under the old IVs and encrypted under the new ones before they are packed."""
        import torch

        dev = arcs.store.device
        n, n_arc = arcs.n_rec, arcs.n_arc
        i32 = lambda k: torch.empty(max(int(k), 1), dtype=torch.int32, device=dev)  # noqa: E731
        lay = Layout(n, n_arc, dev)
        new_of_old, sel, rec_len, count, new_arc, sizes = i32(n), i32(n), i32(n), i32(1), i32(n_arc), i32(n_arc)
        src_off = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        deleted = torch.empty(max(n_arc, 1), dtype=torch.uint8, device=dev)
        kept = _lib.ArchiveKept(new_of_old=new_of_old.data_ptr(), sel=sel.data_ptr(), src_off=src_off.data_ptr(),
                                rec_len=rec_len.data_ptr(), count=count.data_ptr(), deleted=deleted.data_ptr(),
                                new_arc=new_arc.data_ptr(), map_slots=sizes.data_ptr(), lay=lay.c)
        keep = keep.to(torch.uint8).contiguous()
        old = arcs.layout
        oc = _lib.ArchiveLayout.from_buffer_copy(old.c)
        s = stream_of(arcs.store, None)
        stride = map_size(2 * arcs.max_entries + 5)
        head = (self.device, ctypes.byref(oc), n, n_arc)
        old_maps = (arcs.rec_len.data_ptr(), ptr(arcs.sel), arcs.slot_rec.data_ptr(), ptr(arcs.map_sizes),
                    arcs.map_stride, keep.data_ptr())
        if not arcs.header_bytes:
            store = torch.empty(_r16(arcs.store_bytes) + 16, dtype=torch.uint8, device=dev)
            maps = torch.empty((max(n_arc, 1), map_bytes(stride, self.hash_len, self.version)), dtype=torch.uint8,
                               device=dev)
            slot_rec = torch.empty((max(n_arc, 1), stride), dtype=torch.int32, device=dev)
            info = torch.zeros(2, dtype=torch.int64, device=dev)
            check(self._lib.sdfs_cdc_archive_compact(
                *head[:4], arcs.store.data_ptr(), *old_maps, arcs.records.data_ptr(), self.hash_len, 0, self.version,
                None, ctypes.byref(kept), store.data_ptr(), arcs.store_bytes, stride, maps.data_ptr(),
                slot_rec.data_ptr(), info.data_ptr(), s))
            na, store_bytes, _, k = lay.read_totals(count)
            ivs = None
        else:
            if new_ivs is None or aes is None:
                raise ValueError("compacting encrypted archives needs the cipher and the new archives' IVs")
            check(self._lib.sdfs_cdc_archive_compact_select(*head, *old_maps, self.hash_len, arcs.header_bytes,
                                                            ctypes.byref(kept), s))
            na, store_bytes, _, k = lay.read_totals(count)
            ivs = new_ivs[:na].contiguous()
            src, off = arcs.store, src_off
            if k:
                nz = new_of_old[:n].long()
                live = nz >= 0
                old_of_new = torch.empty(k, dtype=torch.int64, device=dev)
                old_of_new[nz[live]] = torch.arange(n, device=dev)[live]
                old_ivs = arcs.ivs[old.arc[:n].long()[old_of_new]].contiguous()
                ln = rec_len[:k]
                room = ln.to(torch.int64)  # ciphertext lengths are multiples of 16
                off = (torch.cumsum(room, 0) - room).contiguous()
                total = _r16(arcs.store_bytes) + 16
                plain = torch.empty(total, dtype=torch.uint8, device=dev)
                plain_len = torch.empty(k, dtype=torch.int32, device=dev)
                aes.decrypt_device(arcs.store, src_off[:k].contiguous(), ln.contiguous(), plain, off, plain_len,
                                   ivs=old_ivs)
                src = torch.empty(total, dtype=torch.uint8, device=dev)
                out_len = torch.empty(k, dtype=torch.int32, device=dev)
                aes.encrypt_device(plain, off, plain_len, src, off, out_len, ivs=ivs[lay.arc[:k].long()].contiguous())
            store = self.pack(lay, src, off, rec_len, arcs.records, sel, count, ivs, store_bytes=store_bytes,
                              header_bytes=arcs.header_bytes)
            maps, slot_rec, info = self.map_emit(lay, rec_len, arcs.records, sel, count, n_arc=na, map_sizes=sizes,
                                                 map_stride=stride)
        nz = new_of_old[:n].long()
        rk = arcs.rec_of_k
        rec_of_k = torch.where(rk >= 0, nz[rk.clamp(min=0)] if n else rk, rk)
        on = rec_of_k >= 0
        idx = rec_of_k.clamp(min=0)
        zero64, zero32 = torch.zeros_like(arcs.store_off), torch.zeros_like(arcs.store_len)
        return ArchiveSet(
            store=store, arc_base=lay.arc_base[:na], arc_bytes=lay.arc_bytes[:na], arc_first=lay.arc_first[: na + 1],
            store_off=torch.where(on, lay.store_off[idx], zero64) if n else zero64,
            store_len=torch.where(on, rec_len[idx], zero32) if n else zero32,
            raw_len=torch.where(on, arcs.raw_len, zero32), maps=maps[: max(na, 1)], slot_rec=slot_rec[: max(na, 1)],
            n_arc=na, store_bytes=store_bytes, n_rec=k, hash_len=self.hash_len, version=self.version,
            header_bytes=arcs.header_bytes, map_stride=stride, map_sizes=sizes[:na], max_entries=arcs.max_entries,
            ivs=ivs, deleted=deleted[:n_arc], new_of_old=new_of_old[:n], layout=lay, rec_len=rec_len[:k],
            rec_of_k=rec_of_k, records=arcs.records, sel=sel[:k], extra={"info": info, "new_arc": new_arc[:n_arc]})


class HipBufferWriter:
    """A batch of write buffers to archive images: ``batch.run`` -> ``index.put_records`` ->
    ``lz4.plan_records`` -> ``compress_device(framed)`` -> (``encrypt_device``) -> archive plan -> pack ->
    map_emit -> ``emit_map_slots``.

    index: a :class:`sdfs_amd.index.HipHashesMap`.  compress: Main.compress (off: the records are
    ``[BE32 -1][chunk]``).  aes: a :class:`sdfs_amd.aes.HipEncryptUtils` or the key bytes
    (Main.chunkStoreEncryptionEnabled); it needs version > 0, whose archive headers carry the IVs."""

    def __init__(self, index, hash_len: int = 32, compress: bool = True, aes=None, version: int = 0,
                 blocksz=MAX_LEN, map_slots: int | None = None, min_len: int = 4095, device: int = 0):
        from .lz4 import HipLz4Compressor

        self.index, self.hash_len, self.compress, self.device = index, int(hash_len), bool(compress), int(device)
        self._own_aes = False
        if aes is not None and not hasattr(aes, "encrypt_device"):
            from .aes import HipEncryptUtils

            aes = HipEncryptUtils(bytes(aes), device)
            self._own_aes = True
        if aes is not None and version <= 0:
            raise ValueError("an encrypted store needs version > 0: the archive header holds the IV")
        self.aes = aes
        self.archiver = HipBlobArchiver(hash_len, version, blocksz, map_slots, min_len, device)
        self._z = HipLz4Compressor(device=device)

    def destroy(self) -> None:
        if getattr(self, "_z", None) is not None:
            self._z.destroy()
            self._z = None
        if self._own_aes and self.aes is not None:
            self.aes.destroy()
            self.aes = None

    def _new_ivs(self, n: int, dev):
        """PassPhrase.getByteIV: 16 random bytes per archive."""
        import torch

        return torch.frombuffer(bytearray(os.urandom(16 * max(n, 1))), dtype=torch.uint8).view(-1, 16).to(dev)

    def write(self, batch, pos_base: int, ivs=None, buffer_id_base: int = 0, run: bool = True):
        """-> (map_slots uint8 [nbuf * slot_len], :class:`ArchiveSet`).  ivs: uint8 [>= n_arc, 16] device
        tensor, the archives' IVs in order (default: random)."""
        from .meta import emit_map_slots

        if run:
            batch.run(buffer_id_base=buffer_id_base)
        recs = batch.recs.view(-1, _lib.RECORD_BYTES)
        dup, loc, new, nc = self.index.put_records(recs, batch.total, pos_base=pos_base)
        arcs = self.store_new(batch.data, batch.nbytes, recs, new, nc, ivs=ivs, buffer_id_base=buffer_id_base,
                              uniform_len=batch.buf_len)
        m, doop, ovf = emit_map_slots(batch, dup, loc, hash_len=self.hash_len, device=self.device)
        arcs.extra.update(dup=dup, hashloc=loc, doop=doop, overflow=ovf, new_list=new[: arcs.n_rec])
        return m, arcs

    def store_new(self, src, nbytes: int, recs, new, nc, ivs=None, buffer_id_base: int = 0, uniform_len: int = 0,
                  buf_offs=None) -> ArchiveSet:
        """What happens to the records ``put_records`` inserted: LZ4 framing or the raw frame, AES,
        archive plan, pack, ``.map`` images.  src: the bytes the records' chunks lie in (``nbytes`` of
        them at most are chunk data); recs: the 48-byte fingerprint records; new / nc: put_records'
        ``new_list`` and ``new_count``; where a record's buffer starts in src: ``buf_offs`` (device
        int64, by buffer_id - buffer_id_base) or ``uniform_len`` times that.  Shared by :meth:`write`
        and :meth:`sdfs_amd.ingest.HipChunkIngest.write_chunks`."""
        import torch

        A = self.archiver
        dev = src.device
        n = int(recs.shape[0])
        nbytes = int(nbytes)
        cnt = nc.view(torch.int32)[:1]
        src_off, src_len, dst_off, _ = self._z.plan_records(recs, sel=new, count=cnt, buffer_id_base=buffer_id_base,
                                                            uniform_len=uniform_len, buf_offs=buf_offs, framed=True)
        live = torch.arange(n, device=dev) < nc  # the entries past the count are not written by anyone
        src_len = torch.where(live, src_len, torch.zeros_like(src_len))
        # worst case of all: every byte of the batch new, every slot a chunk (no host read)
        room = _r16(nbytes + nbytes // 255 + 36 * n) + 16
        # archives: each but the last reaches blocksz or the entry limit
        arc_cap = room // min(A.blocksz) + n // max(A.limit, 1) + 2
        data, rec_off, rec_len, raw = src, src_off, src_len, False
        if self.compress:
            data = torch.empty(room, dtype=torch.uint8, device=dev)
            rec_len = torch.zeros(n, dtype=torch.int32, device=dev)
            rec_off = dst_off
            self._z.compress_device(src, src_off, src_len, data, dst_off, rec_len, count=cnt, framed=True)
        elif self.aes is None:
            raw = True
        prepare = None
        plan_len = None
        if self.aes is not None:
            if ivs is None:
                ivs = self._new_ivs(arc_cap, dev)
            plain, plain_off, plain_len = data, rec_off, rec_len
            framed = plain_len if self.compress else plain_len + 4
            plan_len = torch.where(live, (framed // 16 + 1) * 16, torch.zeros_like(framed))  # Cipher.doFinal
            r64 = plan_len.to(torch.int64)
            enc_off = (torch.cumsum(r64, 0) - r64).contiguous()  # device prefix over the padded lengths
            enc = torch.empty(room + 16 * n, dtype=torch.uint8, device=dev)
            enc_len = torch.zeros(n, dtype=torch.int32, device=dev)

            def prepare(lay):  # each record under its archive's IV
                rec_ivs = ivs[lay.arc[:n].long().clamp(0, ivs.shape[0] - 1)].contiguous()
                self.aes.encrypt_device(plain, plain_off, plain_len, enc, enc_off, enc_len, ivs=rec_ivs, count=cnt,
                                        nz_prefix=None if self.compress else -1)

            data, rec_off, rec_len = enc, enc_off, enc_len
        return A.archive(data, rec_off, rec_len, recs, sel=new, count=cnt, rec_len=plan_len, raw_len=src_len,
                         ivs=ivs, arc_cap=arc_cap, raw_frame=raw, prepare=prepare)

    def compact(self, arcs: ArchiveSet, removed_pos, pos_base: int, new_ivs=None) -> ArchiveSet:
        """A sweep's ``removed_pos`` (``HipHashesMap.sweep``) -> the compacted archives.  The
        directory stays indexed by the write's ``hashloc - pos_base``; dropped entries have
        length 0."""
        import torch

        dev = arcs.store.device
        keep = torch.ones(max(arcs.n_rec, 1), dtype=torch.uint8, device=dev)
        k = removed_pos.to(torch.int64) - int(pos_base)
        k = k[(k >= 0) & (k < arcs.rec_of_k.shape[0])]
        rec = arcs.rec_of_k[k]
        keep[rec[rec >= 0]] = 0
        if arcs.header_bytes and new_ivs is None:
            new_ivs = self._new_ivs(arcs.n_arc, dev)
        return self.archiver.compact(arcs, keep, new_ivs=new_ivs, aes=self.aes)
