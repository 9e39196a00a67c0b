"""A chunk store reopened from the bytes it persists, and scrubbed (include/sdfs_store.h).

The write path ends in archive images and ``.map`` images (:mod:`sdfs_amd.archive`); the read path
starts from a directory (:mod:`sdfs_amd.read`).  Within one process an :class:`ArchiveSet` joins
them.  This module makes one from nothing but the images and the index:

* :func:`scan_store` — ``sdfs_cdc_store_scan``: the record list of the images, in put order, with
  the map geometry decided as ``SimpleByteArrayLongMap.setUp`` decides it for an existing file.
* :func:`open_store` — scan -> (encrypted: decrypt every record under the IV in its archive's
  header -> ``chain_lens`` -> ``raw_lens``) -> ``index.get_digests`` -> directory: a complete
  :class:`ArchiveSet` that ``HipBufferReader.read`` and ``compact`` take unchanged.
* :func:`lookup` — ``HashBlobArchive.getChunk``'s lookup for a batch of ``(archive, key)``.
* :func:`scrub` — every stored record decrypted, decoded and fingerprinted against its key.

PyTorch allocates HBM and hands over the stream; every step runs the library's HIP kernels.  No
CPU fallback: a failure raises :class:`SdfsCdcError`.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

from . import _lib
from ._lib import (ARCHIVE_HEADER, STORE_ECAP, STORE_FETCH, STORE_GAP, STORE_HASH, STORE_KEY, STORE_LEN,  # noqa: F401
                   STORE_NZ, STORE_RANGE, STORE_SLOTS, STORE_UNREADABLE, check, ptr, stream_of)
from .archive import ArchiveSet, Layout, _r16, map_bytes


def _host_lens(map_len):
    """The maps' file lengths as host ints (a tensor costs a host read: hand in a list)."""
    return [int(v) for v in (map_len.tolist() if hasattr(map_len, "tolist") else map_len)]


def _i64(t):
    import torch

    return t.to(torch.int64).contiguous()


@dataclass
class StoreScan:
    """What ``sdfs_cdc_store_scan`` wrote: per record (``n_cap`` entries, ``count`` valid) and per archive."""

    n_arc: int
    n_cap: int
    arc: object        # int32 [n_cap]
    slot: object       # int32 [n_cap]
    pos: object        # int32 [n_cap]
    len: object        # int32 [n_cap]
    store_off: object  # int64 [n_cap]
    key: object        # uint8 [n_cap, 32]
    raw_len: object    # int32 [n_cap]
    flags: object      # int32 [n_cap], STORE_RANGE .. STORE_NZ
    count: object      # int32 [1]
    status: object     # int32 [1], STORE_ECAP
    map_slots: object  # int32 [n_arc]
    version: object    # int32 [n_arc]
    arc_first: object  # int32 [n_arc + 1]
    ivs: object        # uint8 [n_arc, 16], None without archive headers
    slot_rec: object   # int32 [n_arc, slot_stride], -1 = free
    arc_status: object  # int32 [n_arc], STORE_GAP | STORE_SLOTS
    slot_stride: int
    map_len: list      # host ints
    map_stride_bytes: int


def _images(store, arc_base, arc_bytes, maps, map_len):
    n_arc = int(arc_base.shape[0])
    lens = _host_lens(map_len)
    if len(lens) != n_arc or int(arc_bytes.shape[0]) != n_arc:
        raise ValueError("one base, one length and one map length per archive")
    if maps.dim() != 2 or (n_arc and (maps.shape[0] < n_arc or maps.stride(1) != 1)):
        raise ValueError("maps: uint8 [n_arc, row bytes], one .map image per row")
    stride = int(maps.stride(0)) if n_arc else 0
    c_lens = (ctypes.c_uint64 * max(n_arc, 1))(*lens)
    return n_arc, lens, stride, c_lens, _i64(arc_base), _i64(arc_bytes)


def scan_store(store, arc_base, arc_bytes, maps, map_len, hash_len: int = 32, version: int = 0, plain: bool = True,
               max_chunk: int = 32768, n_cap: int | None = None, slot_stride: int | None = None, device: int = 0,
               stream=None) -> StoreScan:
    """``sdfs_cdc_store_scan``.  store: uint8, every archive image at ``arc_base[a]``, ``arc_bytes[a]``
    long (int64 device tensors); maps: uint8 [n_arc, row bytes]; map_len: the files' true lengths (host
    ints).  n_cap: record slots (default: every slot of every map, which cannot fail); slot_stride:
    columns of ``slot_rec`` (default: the largest map in the layout ``version`` makes)."""
    import torch

    n_arc, lens, stride, c_lens, arc_base, arc_bytes = _images(store, arc_base, arc_bytes, maps, map_len)
    dev = store.device
    hl = int(hash_len)
    if n_cap is None:
        n_cap = sum(ln // (hl + 4) for ln in lens)
    if slot_stride is None:
        el, off = (hl + 8, 16) if version else (hl + 4, 0)
        slot_stride = max([max(ln - off, 0) // el for ln in lens] + [1])
    header = ARCHIVE_HEADER if version else 0
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    k, a = max(int(n_cap), 1), max(n_arc, 1)
    sc = StoreScan(n_arc, int(n_cap), z(k, torch.int32), z(k, torch.int32), z(k, torch.int32), z(k, torch.int32),
                   z(k, torch.int64), z((k, 32), torch.uint8), z(k, torch.int32), z(k, torch.int32),
                   z(1, torch.int32), z(1, torch.int32), z(a, torch.int32), z(a, torch.int32), z(a + 1, torch.int32),
                   z((a, 16), torch.uint8) if header else None,
                   torch.full((a, int(slot_stride)), -1, dtype=torch.int32, device=dev), z(a, torch.int32),
                   int(slot_stride), lens, stride)
    recs = _lib.StoreRecords(arc=sc.arc.data_ptr(), slot=sc.slot.data_ptr(), pos=sc.pos.data_ptr(),
                             len=sc.len.data_ptr(), store_off=sc.store_off.data_ptr(), key=sc.key.data_ptr(),
                             raw_len=sc.raw_len.data_ptr(), flags=sc.flags.data_ptr(), count=sc.count.data_ptr(),
                             status=sc.status.data_ptr(), n_cap=int(n_cap), reserved=0)
    arcs = _lib.StoreArchives(map_slots=sc.map_slots.data_ptr(), version=sc.version.data_ptr(),
                              arc_first=sc.arc_first.data_ptr(), ivs=sc.ivs.data_ptr() if header else None,
                              slot_rec=sc.slot_rec.data_ptr(), status=sc.arc_status.data_ptr(),
                              slot_stride=int(slot_stride), reserved=0)
    check(_lib.load().sdfs_cdc_store_scan(
        int(device), n_arc, store.data_ptr(), int(store.numel()), arc_base.data_ptr(), arc_bytes.data_ptr(),
        maps.data_ptr(), stride, c_lens, hl, int(version), header, int(max_chunk), int(bool(plain)),
        ctypes.byref(recs), ctypes.byref(arcs), stream_of(store, stream)))
    return sc


def raw_lens(plain, off, length, flags, max_chunk: int = 32768, count=None, device: int = 0, stream=None):
    """``sdfs_cdc_store_raw_lens``: the nz rule on decrypted records -> raw_len int32 [n]; STORE_NZ is
    or-ed into ``flags`` (int32 [n], in place)."""
    import torch

    n = int(length.shape[0])
    out = torch.empty(max(n, 1), dtype=torch.int32, device=plain.device)[:n]
    check(_lib.load().sdfs_cdc_store_raw_lens(int(device), plain.data_ptr(), off.data_ptr(), length.data_ptr(),
                                              ptr(count), n, int(max_chunk),
                                              out.data_ptr(), flags.data_ptr(), stream_of(plain, stream)))
    return out


def directory(store_off, length, raw_len, flags, hashloc, pos_base: int, n_store: int, count=None, device: int = 0,
              stream=None):
    """``sdfs_cdc_store_directory`` -> (store_off int64 [n_store], store_len int32, raw_len int32,
    rec_of_k int64 with -1 = no record, info int64 [3] = orphans, out of range, clashes)."""
    import torch

    n, k = int(length.shape[0]), int(n_store)
    dev = hashloc.device
    o_off = torch.empty(k, dtype=torch.int64, device=dev)
    o_len, o_raw, o_rec = (torch.empty(k, dtype=torch.int32, device=dev) for _ in range(3))
    info = torch.empty(3, dtype=torch.int64, device=dev)
    p = lambda t: t.data_ptr() if k else None  # noqa: E731
    check(_lib.load().sdfs_cdc_store_directory(
        int(device), store_off.data_ptr(), length.data_ptr(), raw_len.data_ptr(), flags.data_ptr(), hashloc.data_ptr(),
        ptr(count), n, int(pos_base), k, p(o_off), p(o_len), p(o_raw), p(o_rec),
        info.data_ptr(), stream_of(hashloc, stream)))
    return o_off, o_len, o_raw, o_rec.to(torch.int64), info


def _decrypt_records(aes, store, store_off, length, ivs, plain_bytes: int, device: int):
    """Every record under its own IV into an area of its own -> (plain, plain_off, decoder input lengths)."""
    import torch

    from .read import chain_lens

    n = int(length.shape[0])
    room = (length.to(torch.int64) + 15) // 16 * 16
    off = (torch.cumsum(room, 0) - room).contiguous()
    plain = torch.empty(_r16(plain_bytes) + 64, dtype=torch.uint8, device=store.device)
    plain_len = torch.empty(n, dtype=torch.int32, device=store.device)
    aes.decrypt_device(store, store_off.contiguous(), length.contiguous(), plain, off, plain_len, ivs=ivs.contiguous())
    return plain, off, chain_lens(plain_len, device=device)


def open_store(store, arc_base, arc_bytes, maps, map_len, index, pos_base: int, n_store: int, hash_len: int = 32,
               version: int = 0, aes=None, max_chunk: int = 32768, device: int = 0) -> ArchiveSet:
    """A store's persisted bytes -> the :class:`ArchiveSet` its writer returned.

    store / arc_base / arc_bytes / maps / map_len: as :func:`scan_store` takes them.  index: the
    :class:`sdfs_amd.index.HipHashesMap` of the volume; the directory has ``n_store`` entries, entry k
    for hashloc ``pos_base + k``.  aes: the store's :class:`sdfs_amd.aes.HipEncryptUtils` when the
    records are encrypted (version > 0: each archive's IV is read from its header).  One host read:
    the record count (with the sizes that come with it), to trim the tensors.
    ``extra["open"]``: flags int32 [n_rec], arc_status int32 [n_arc], info int64 [3] = orphans, out of
    range, clashes, and the scan itself."""
    import torch

    dev = store.device
    hl = int(hash_len)
    sc = scan_store(store, arc_base, arc_bytes, maps, map_len, hl, version, plain=aes is None, max_chunk=max_chunk,
                    device=device)
    n_arc = sc.n_arc
    ab, bb = _i64(arc_base), _i64(arc_bytes)
    per_arc = sc.arc_first[1: n_arc + 1] - sc.arc_first[:n_arc]
    one = lambda t: t.reshape(-1)[:1].to(torch.int64)  # noqa: E731
    end = (ab + bb).max().reshape(1) if n_arc else torch.zeros(1, dtype=torch.int64, device=dev)
    most = per_arc.max().reshape(1) if n_arc else torch.zeros(1, dtype=torch.int32, device=dev)
    room = ((sc.len.to(torch.int64) + 15) // 16 * 16).sum().reshape(1)  # of the decrypted records
    n, status, store_bytes, max_entries, len_total = (int(v) for v in torch.cat(
        [one(sc.count), one(sc.status), end, one(most), room]).tolist())  # the one host read
    if status & STORE_ECAP:
        raise _lib.SdfsCdcError(_lib.ECAP, f"the maps hold {n} records, more than the {sc.n_cap} slots given")
    arc, flags, rec_len = sc.arc[:n], sc.flags[:n], sc.len[:n]
    raw = sc.raw_len[:n]
    ivs = sc.ivs[:n_arc] if sc.ivs is not None else None
    if aes is not None and n:
        if ivs is None:
            raise ValueError("an encrypted store has version > 0: the archive header holds the IV")
        plain, off, dec_len = _decrypt_records(aes, store, sc.store_off[:n], rec_len, ivs[arc.long()], len_total, device)
        raw = raw_lens(plain, off, dec_len, flags, max_chunk, device=device)
    hashloc, _ = index.get_digests(sc.key[:n])
    d_off, d_len, d_raw, rec_of_k, info = directory(sc.store_off[:n], rec_len, raw, flags, hashloc, pos_base, n_store,
                                                     device=device)
    lay = Layout(n, n_arc, dev)
    lay.arc[:n].copy_(arc)
    lay.pos[:n].copy_(sc.pos[:n])
    lay.store_off[:n].copy_(sc.store_off[:n])
    lay.arc_first[: n_arc + 1].copy_(sc.arc_first[: n_arc + 1])
    lay.arc_bytes[:n_arc].copy_(bb)
    lay.arc_base[:n_arc].copy_(ab)
    lay.totals.copy_(torch.tensor([n_arc, store_bytes], dtype=torch.int64))
    records = torch.zeros((max(n, 1), _lib.RECORD_BYTES), dtype=torch.uint8, device=dev)
    records[:n, :32] = sc.key[:n]
    return ArchiveSet(
        store=store, arc_base=lay.arc_base[:n_arc], arc_bytes=lay.arc_bytes[:n_arc],
        arc_first=lay.arc_first[: n_arc + 1], store_off=d_off, store_len=d_len, raw_len=d_raw, maps=maps,
        slot_rec=sc.slot_rec, n_arc=n_arc, store_bytes=store_bytes, n_rec=n, hash_len=hl, version=int(version),
        header_bytes=ARCHIVE_HEADER if version else 0, map_stride=sc.slot_stride, map_sizes=sc.map_slots[:n_arc],
        max_entries=max(max_entries, 1), ivs=ivs, layout=lay, rec_len=rec_len, rec_of_k=rec_of_k, records=records,
        sel=None, extra={"open": dict(flags=flags, arc_status=sc.arc_status[:n_arc], info=info, scan=sc,
                                      map_len=sc.map_len, hashloc=hashloc)})


def _map_lens(arcs: ArchiveSet):
    """The ``.map`` files' lengths of a set: as opened, or what its writer made."""
    if "open" in arcs.extra:
        return arcs.extra["open"]["map_len"]
    sizes = arcs.map_sizes.tolist() if arcs.map_sizes is not None else [arcs.map_stride] * arcs.n_arc
    return [map_bytes(int(s), arcs.hash_len, arcs.version) for s in sizes[: arcs.n_arc]]


@dataclass
class Lookup:
    """``sdfs_cdc_store_lookup``'s answers, one per query (device tensors)."""

    slot: object       # int32, -1 = absent
    pos: object        # int32
    len: object        # int32
    store_off: object  # int64
    flags: object      # int32, STORE_RANGE | STORE_KEY | STORE_LEN


def lookup(arcs: ArchiveSet, arc, keys, device: int = 0, stream=None) -> Lookup:
    """``HashBlobArchive.getChunk``'s lookup: arc int32 [n] (or one int for every query), keys uint8
    [n, 32] (zero-padded digests) on the device."""
    import torch

    n = int(keys.shape[0])
    dev = arcs.store.device
    if not isinstance(arc, torch.Tensor):
        arc = torch.full((n,), int(arc), dtype=torch.int32, device=dev)
    arc = arc.to(device=dev, dtype=torch.int32).contiguous()
    keys = keys.contiguous()
    if keys.dim() != 2 or keys.shape[1] != 32 or arc.shape[0] != n:
        raise ValueError("keys: uint8 [n, 32], one archive per key")
    n_arc, _, stride, c_lens, ab, bb = _images(arcs.store, arcs.arc_base, arcs.arc_bytes, arcs.maps, _map_lens(arcs))
    e = lambda dt: torch.empty(max(n, 1), dtype=dt, device=dev)[:n]  # noqa: E731
    out = Lookup(e(torch.int32), e(torch.int32), e(torch.int32), e(torch.int64), e(torch.int32))
    check(_lib.load().sdfs_cdc_store_lookup(
        int(device), n_arc, arcs.store.data_ptr(), int(arcs.store.numel()), ab.data_ptr(), bb.data_ptr(),
        arcs.maps.data_ptr(), stride, c_lens, arcs.hash_len, arcs.version, arcs.header_bytes, arc.data_ptr(),
        keys.data_ptr(), n, out.slot.data_ptr(), out.pos.data_ptr(), out.len.data_ptr(), out.store_off.data_ptr(),
        out.flags.data_ptr(), stream_of(arcs.store, stream)))
    return out


def verify(engine, chunks, off, length, keys, flags, hash_len: int = 32, count=None, stream=None) -> None:
    """``sdfs_cdc_store_verify``: STORE_FETCH / STORE_HASH or-ed into ``flags`` (int32 [n], in place)."""
    n = int(length.shape[0])
    check(_lib.load().sdfs_cdc_store_verify(engine._h, chunks.data_ptr(), off.data_ptr(), length.data_ptr(),
                                            keys.data_ptr(), ptr(count), n,
                                            int(hash_len), flags.data_ptr(), stream_of(chunks, stream)))


def scrub(arcs: ArchiveSet, engine, aes=None, batch_records: int = 65536, device: int = 0, stages=None):
    """Every stored record against its key -> (flags int32 [n_rec], arc_status int32 [n_arc]).

    The images of ``arcs`` (from :func:`open_store` or from a writer) are scanned as they lie now,
    then decrypt -> framed decode -> verify run in slices of ``batch_records`` records, so scratch
    is bounded by the slice (one host read per slice and stage: the scratch size).  Records come in
    the scan's order: archive by archive, ascending position.  engine: the hash engine the keys
    were made with; aes: the store's cipher when it is encrypted.  ``stages``: optional
    callable(name) called after each stage is enqueued (measurements)."""
    import torch

    from .lz4 import HipLz4Compressor

    mark = stages or (lambda name: None)
    dev = arcs.store.device
    max_chunk = int(engine._params.max_len)
    sc = scan_store(arcs.store, arcs.arc_base, arcs.arc_bytes, arcs.maps, _map_lens(arcs), arcs.hash_len, arcs.version,
                    plain=aes is None, max_chunk=max_chunk, device=device)
    mark("scan")
    n = int(sc.count.item())
    flags = sc.flags[:n].clone()
    z = HipLz4Compressor(device=device)
    try:
        for i0 in range(0, n, max(int(batch_records), 1)):
            i1 = min(i0 + max(int(batch_records), 1), n)
            fl = flags[i0:i1]
            ok = (fl & STORE_UNREADABLE) == 0
            zero32 = torch.zeros(i1 - i0, dtype=torch.int32, device=dev)
            src, src_off = arcs.store, torch.where(ok, sc.store_off[i0:i1], torch.zeros_like(sc.store_off[i0:i1]))
            src_len = torch.where(ok, sc.len[i0:i1], zero32)
            raw = sc.raw_len[i0:i1]
            if aes is not None:
                if sc.ivs is None:
                    raise ValueError("an encrypted store has version > 0: the archive header holds the IV")
                total = int(((src_len.to(torch.int64) + 15) // 16 * 16).sum().item())
                src, src_off, src_len = _decrypt_records(aes, arcs.store, src_off, src_len,
                                                         sc.ivs[sc.arc[i0:i1].long()], total, device)
                mark("decrypt")
                bad = (~ok).to(torch.int32)  # not looked at; a failed decrypt gets no room and fails its fetch
                raw = raw_lens(src, src_off, src_len, bad, max_chunk, device=device)
                src_len = torch.where(bad == 0, src_len, zero32)
            room = (raw.to(torch.int64) + 15) // 16 * 16
            dst_off = (torch.cumsum(room, 0) - room).contiguous()
            chunks = torch.empty(int(room.sum().item()) + 64, dtype=torch.uint8, device=dev)
            got = torch.empty(i1 - i0, dtype=torch.int32, device=dev)
            z.decompress_device(src, src_off.contiguous(), src_len.contiguous(), chunks, dst_off, raw.contiguous(), got,
                                framed=True)
            mark("decode")
            verify(engine, chunks, dst_off, got, sc.key[i0:i1], fl, arcs.hash_len)
            mark("verify")
    finally:
        z.destroy()
    return flags, sc.arc_status[: sc.n_arc]
