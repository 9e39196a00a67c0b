"""Read path on the MI355X (include/sdfs_read.h): write buffers rebuilt from their map slots.

The way back of :mod:`sdfs_amd.meta`: ``WritableCacheBuffer.initBuffer``
(WritableCacheBuffer.java:249-410) parses the buffer's ``SparseDataChunk``
(SparseDataChunk.java:159-174), fetches the chunk of every ``HashLocPair`` before the first
``hashloc == 0`` (``HashBlobArchive.getChunk``, HashBlobArchive.java:1922-1944: decrypt, read nz,
LZ4-decode, optionally re-hash) and puts ``ck[offset : offset + min(nlen, len(ck))]`` at ``pos``
into a zeroed CHUNK_LENGTH array.

* :func:`parse_map_slots` — the slots' images as a :class:`ParsedPairs` (device tensors).
* :class:`HipBufferReader` — the whole path for a batch of buffers: parse -> plan -> (decrypt ->
  chain_lens) -> framed decode -> assemble -> (verify); ``read_ranges`` / ``read_file`` —
  ``DedupFileChannel.read`` (DedupFileChannel.java:499-608) for batches of byte ranges: split ->
  parse of the touched slots -> plan_pieces -> the same middle -> assemble_pieces -> (verify).
* :func:`split_requests`, :func:`plan_pieces`, :func:`assemble_pieces` — the ranged read's steps.

PyTorch allocates HBM and hands over the stream; every step runs the library's HIP kernels.
No CPU fallback: a failure raises :class:`SdfsCdcError`.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

from . import _lib
from ._lib import READ_BOUNDS, READ_CORRUPT, READ_FETCH, READ_MISSING, READ_NONE, check, ptr, stream_of  # noqa: F401


def pair_cap(slot_len: int, hash_len: int = 32) -> int:
    """Pairs a slot can hold: (slot_len - 13) // (hash_len + 24)."""
    return int(_lib.load().sdfs_cdc_map_pair_cap(int(slot_len), int(hash_len)))


@dataclass
class ParsedPairs:
    """``sdfs_cdc_pairs``: buffer b's pair i at row b, column i (i < counts[b]), ascending pos."""

    nbuf: int
    cap: int
    hash_len: int
    counts: object   # int32 [nbuf]
    hashes: object   # uint8 [nbuf, cap, 32]
    hashloc: object  # int64 [nbuf, cap]
    len: object      # int32 [nbuf, cap]
    pos: object
    offset: object
    nlen: object
    doop: object     # int32 [nbuf]
    flags: object    # uint8 [nbuf]
    status: object   # int32 [nbuf], SDFS_CDC_READ_* bits

    def __post_init__(self):
        self.c = _lib.Pairs(
            counts=self.counts.data_ptr(), hashes=self.hashes.data_ptr(), hashloc=self.hashloc.data_ptr(),
            len=self.len.data_ptr(), pos=self.pos.data_ptr(), offset=self.offset.data_ptr(),
            nlen=self.nlen.data_ptr(), doop=self.doop.data_ptr(), flags=self.flags.data_ptr(),
            status=self.status.data_ptr(), cap=self.cap, reserved=0)


def parse_map_slots(m, nbuf: int, slot_len: int, hash_len: int = 32, device: int = 0, stream=None) -> ParsedPairs:
    """m: device uint8 tensor holding nbuf slots of slot_len bytes (``emit_map_slots``' output)."""
    import torch

    cap = max(pair_cap(slot_len, hash_len), 1)
    dev = m.device
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    pairs = ParsedPairs(nbuf, cap, hash_len, z(max(nbuf, 1), torch.int32), z((max(nbuf, 1), cap, 32), torch.uint8),
                        z((max(nbuf, 1), cap), torch.int64), z((max(nbuf, 1), cap), torch.int32),
                        z((max(nbuf, 1), cap), torch.int32), z((max(nbuf, 1), cap), torch.int32),
                        z((max(nbuf, 1), cap), torch.int32), z(max(nbuf, 1), torch.int32),
                        z(max(nbuf, 1), torch.uint8), z(max(nbuf, 1), torch.int32))
    if m.numel() < nbuf * slot_len:
        raise ValueError(f"map holds {m.numel()} bytes, {nbuf} slots of {slot_len} need {nbuf * slot_len}")
    check(_lib.load().sdfs_cdc_map_parse(int(device), int(nbuf), m.data_ptr(), int(slot_len), int(hash_len),
                                         ctypes.byref(pairs.c), stream_of(m, stream)))
    return pairs


def plan_reads(pairs: ParsedPairs, store_off, store_len, store_raw_len, pos_base: int, device: int = 0, stream=None):
    """``sdfs_cdc_read_plan``.  Directory tensors: store_off i64[n], store_len / store_raw_len i32[n].
    Returns a dict of device tensors: pair_fetch i32[nbuf, cap] (-1 = not used), fetch_count i32[1],
    src_off, src_len, dst_off, dst_cap, plain_off (n entries each, fetch_count valid), total_bytes
    i64[2] (chunk area, decrypted-record area)."""
    import torch

    n = int(store_len.shape[0])
    dev = pairs.counts.device
    e = lambda dt: torch.empty(max(n, 1), dtype=dt, device=dev)  # noqa: E731
    out = dict(pair_fetch=torch.empty((max(pairs.nbuf, 1), pairs.cap), dtype=torch.int32, device=dev),
               fetch_count=torch.zeros(1, dtype=torch.int32, device=dev), src_off=e(torch.int64),
               src_len=e(torch.int32), dst_off=e(torch.int64), dst_cap=e(torch.int32), plain_off=e(torch.int64),
               total_bytes=torch.zeros(2, dtype=torch.int64, device=dev))
    check(_lib.load().sdfs_cdc_read_plan(
        int(device), pairs.nbuf, ctypes.byref(pairs.c), int(pos_base), n, store_off.data_ptr() if n else None,
        store_len.data_ptr() if n else None, store_raw_len.data_ptr() if n else None, out["pair_fetch"].data_ptr(),
        out["fetch_count"].data_ptr(), out["src_off"].data_ptr(), out["src_len"].data_ptr(),
        out["dst_off"].data_ptr(), out["dst_cap"].data_ptr(), out["plain_off"].data_ptr(),
        out["total_bytes"].data_ptr(), stream_of(pairs.counts, stream)))
    return out


def chain_lens(in_len, count=None, device: int = 0, stream=None):
    """``sdfs_cdc_read_chain_lens``: the decryptor's output lengths as decoder input lengths."""
    import torch

    out = torch.empty_like(in_len)
    check(_lib.load().sdfs_cdc_read_chain_lens(int(device), in_len.data_ptr(),
                                               ptr(count), int(in_len.shape[0]), out.data_ptr(),
                                               stream_of(in_len, stream)))
    return out


def assemble(pairs: ParsedPairs, chunk_length: int, pair_fetch, chunks, fetch_off, fetch_len, out=None,
             device: int = 0, stream=None):
    """``sdfs_cdc_read_assemble``: settles pairs.status and writes the buffers (uint8 [nbuf, chunk_length])."""
    import torch

    if out is None:
        out = torch.empty((pairs.nbuf, chunk_length), dtype=torch.uint8, device=chunks.device)
    check(_lib.load().sdfs_cdc_read_assemble(int(device), pairs.nbuf, int(chunk_length), ctypes.byref(pairs.c),
                                             pair_fetch.data_ptr(), chunks.data_ptr(), fetch_off.data_ptr(),
                                             fetch_len.data_ptr(), out.data_ptr(), stream_of(chunks, stream)))
    return out


def verify_reads(engine, pairs: ParsedPairs, pair_fetch, chunks, fetch_off, fetch_len, fetch_count, stream=None):
    """``sdfs_cdc_read_verify``: (pair_bad uint8 [nbuf, cap], bad_count int32 [nbuf])."""
    import torch

    dev = chunks.device
    bad = torch.empty((max(pairs.nbuf, 1), pairs.cap), dtype=torch.uint8, device=dev)
    cnt = torch.empty(max(pairs.nbuf, 1), dtype=torch.int32, device=dev)
    check(_lib.load().sdfs_cdc_read_verify(engine._h, pairs.nbuf, ctypes.byref(pairs.c), pairs.hash_len,
                                           pair_fetch.data_ptr(), chunks.data_ptr(), fetch_off.data_ptr(),
                                           fetch_len.data_ptr(), fetch_count.data_ptr(), int(fetch_len.shape[0]),
                                           bad.data_ptr(), cnt.data_ptr(), stream_of(chunks, stream)))
    return bad, cnt


@dataclass
class Pieces:
    """``sdfs_cdc_read_split``'s outputs (host numpy arrays): request r read n_read[r] bytes (-1 =
    at or past the end of the file); piece p is [start[p], start[p] + len[p]) of row row[p] (-1: past
    the map, zeros) and goes to out_off[p]; rows = the distinct touched slots, ascending."""

    n_read: object   # int64 [n_requests]
    req: object      # int32 [n_pieces]
    row: object      # int32 [n_pieces], -1 = no row
    start: object    # int32 [n_pieces]
    len: object      # int32 [n_pieces]
    out_off: object  # int64 [n_pieces]
    rows: object     # int64 [n_rows] slot indices


def _u64_table(rows, width: int, what: str):
    import numpy as np

    a = np.asarray(rows)
    if a.size == 0:
        return np.zeros((0, width), np.uint64)
    if a.ndim != 2 or a.shape[1] != width:
        raise ValueError(f"{what}: {width} integers each")
    if a.dtype.kind not in "iu":
        raise ValueError(f"{what}: integers")
    if a.dtype.kind == "i" and (a < 0).any():
        raise ValueError(f"{what}: a negative value")
    return np.ascontiguousarray(a, dtype=np.uint64)


def split_requests(files, requests, chunk_length: int) -> Pieces:
    """``sdfs_cdc_read_split`` (host): ``DedupFileChannel.read``'s request layer.  files: rows of
    (first_slot, n_slots, file_len); requests: rows of (file, file_pos, siz, out_off)."""
    import numpy as np

    lib = _lib.load()
    f = _u64_table(files, 3, "files")
    q = _u64_table(requests, 4, "requests")
    n_read = np.zeros(max(len(q), 1), np.int64)
    np_, nr = ctypes.c_uint64(0), ctypes.c_uint64(0)
    ip = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    # the documented bound, clipped: a first call that runs short reports the counts
    per = np.minimum(q[:, 2] // np.uint64(max(int(chunk_length), 1)), np.uint64(1 << 20)) + np.uint64(2)
    cap = min(int(per.sum()), 1 << 20)
    while True:
        u32 = [np.zeros(max(cap, 1), np.uint32) for _ in range(4)]
        out_off = np.zeros(max(cap, 1), np.uint64)
        rows = np.zeros(max(cap, 1), np.uint64)
        rc = lib.sdfs_cdc_read_split(ip(f), len(f), ip(q), len(q), int(chunk_length), ip(n_read), cap, ip(u32[0]),
                                     ip(u32[1]), ip(u32[2]), ip(u32[3]), ip(out_off), cap, ip(rows),
                                     ctypes.byref(np_), ctypes.byref(nr))
        if rc != _lib.ECAP:
            break
        cap = int(np_.value)  # rows <= pieces
    check(rc)
    n, r = int(np_.value), int(nr.value)
    return Pieces(n_read[:len(q)], u32[0][:n].view(np.int32), u32[1][:n].view(np.int32), u32[2][:n].view(np.int32),
                  u32[3][:n].view(np.int32), out_off[:n].view(np.int64), rows[:r].view(np.int64))


def plan_pieces(pairs: ParsedPairs, piece_row, piece_start, piece_len, store_off, store_len, store_raw_len,
                pos_base: int, device: int = 0, stream=None):
    """``sdfs_cdc_read_plan_pieces``.  piece_row / piece_start / piece_len: device int32 [n_pieces]
    (row -1 = no row).  Returns :func:`plan_reads`' dict plus piece_status int32 [n_pieces]."""
    import torch

    n = int(store_len.shape[0])
    npc = int(piece_row.shape[0])
    dev = pairs.counts.device
    e = lambda dt: torch.empty(max(n, 1), dtype=dt, device=dev)  # noqa: E731
    out = dict(pair_fetch=torch.empty((max(pairs.nbuf, 1), pairs.cap), dtype=torch.int32, device=dev),
               fetch_count=torch.zeros(1, dtype=torch.int32, device=dev), src_off=e(torch.int64),
               src_len=e(torch.int32), dst_off=e(torch.int64), dst_cap=e(torch.int32), plain_off=e(torch.int64),
               total_bytes=torch.zeros(2, dtype=torch.int64, device=dev),
               piece_status=torch.zeros(max(npc, 1), dtype=torch.int32, device=dev)[:npc])
    check(_lib.load().sdfs_cdc_read_plan_pieces(
        int(device), pairs.nbuf, ctypes.byref(pairs.c), int(pos_base), n, store_off.data_ptr() if n else None,
        store_len.data_ptr() if n else None, store_raw_len.data_ptr() if n else None, npc,
        piece_row.data_ptr() if npc else None, piece_start.data_ptr() if npc else None,
        piece_len.data_ptr() if npc else None, out["piece_status"].data_ptr() if npc else None,
        out["pair_fetch"].data_ptr(), out["fetch_count"].data_ptr(), out["src_off"].data_ptr(),
        out["src_len"].data_ptr(), out["dst_off"].data_ptr(), out["dst_cap"].data_ptr(), out["plain_off"].data_ptr(),
        out["total_bytes"].data_ptr(), stream_of(pairs.counts, stream)))
    return out


def assemble_pieces(pairs: ParsedPairs, chunk_length: int, pair_fetch, chunks, fetch_off, fetch_len, piece_row,
                    piece_start, piece_len, piece_out_off, piece_status, out, piece_req=None, n_requests: int = 0,
                    device: int = 0, stream=None):
    """``sdfs_cdc_read_assemble_pieces``: settles piece_status (in/out) and writes piece p to
    out[piece_out_off[p] : + piece_len[p]] (``out``: device uint8, flat).  With piece_req (device
    int32 [n_pieces]) and n_requests it returns the per-request status, int32 [n_requests]."""
    import torch

    npc = int(piece_row.shape[0])
    req_status = None
    if piece_req is not None:
        req_status = torch.empty(max(n_requests, 1), dtype=torch.int32, device=chunks.device)[:n_requests]
    if npc or n_requests:
        p = lambda t: t.data_ptr() if npc else None  # noqa: E731
        check(_lib.load().sdfs_cdc_read_assemble_pieces(
            int(device), pairs.nbuf, int(chunk_length), ctypes.byref(pairs.c), pair_fetch.data_ptr(),
            chunks.data_ptr(), fetch_off.data_ptr(), fetch_len.data_ptr(), npc, p(piece_row), p(piece_start),
            p(piece_len), p(piece_out_off), p(piece_status), p(piece_req) if piece_req is not None else None,
            int(n_requests) if piece_req is not None else 0, ptr(req_status) if n_requests else None,
            out.data_ptr() if npc else None, stream_of(chunks, stream)))
    return out if req_status is None else req_status


@dataclass
class RangeInfo:
    fetch_count: int        # distinct stored records the batch needed
    pieces: Pieces
    piece_status: object    # int32 [n_pieces], SDFS_CDC_READ_* bits
    rows: object            # int64 [n_rows] (device): the parsed slots, ``pairs`` row i = slot rows[i]
    pairs: ParsedPairs
    pair_fetch: object      # int32 [n_rows, cap], -1 = not needed
    bad_count: object = None  # verify: int32 [n_rows]
    pair_bad: object = None   # verify: uint8 [n_rows, cap]


@dataclass
class ReadInfo:
    fetch_count: int        # distinct stored records the batch needed
    pairs: ParsedPairs
    pair_fetch: object      # int32 [nbuf, cap], -1 = not used
    bad_count: object = None  # verify: int32 [nbuf] pairs whose hash differs from their chunk's digest
    pair_bad: object = None   # verify: uint8 [nbuf, cap]


class HipBufferReader:
    """WritableCacheBuffer.initBuffer for batches of buffers on one GPU.

    aes: a :class:`sdfs_amd.aes.HipEncryptUtils` (or the key bytes) when the store is encrypted, with
    iv the archive's 16 bytes (record_ivs: every read brings ``store_ivs`` instead).  engine: the
    hash engine, needed for ``verify=True``."""

    def __init__(self, chunk_length: int, hash_len: int = 32, device: int = 0, aes=None, iv=None, engine=None,
                 record_ivs: bool = False):
        from .lz4 import HipLz4Compressor

        self.chunk_length = int(chunk_length)
        self.hash_len = int(hash_len)
        self.device = int(device)
        self.engine = engine
        self._own_aes = False
        if aes is not None and not hasattr(aes, "decrypt_device"):
            from .aes import HipEncryptUtils

            aes = HipEncryptUtils(bytes(aes), device)
            self._own_aes = True
        if aes is not None and iv is None and not record_ivs:
            raise ValueError("an encrypted store needs the archive's IV")
        self.aes = aes
        self.iv = iv
        self._z = HipLz4Compressor(device=device)

    def destroy(self) -> None:
        if getattr(self, "_z", None) is not None:
            self._z.destroy()
            self._z = None
        if self._own_aes and self.aes is not None:
            self.aes.destroy()
            self.aes = None

    def _fetch(self, pairs, plan, store, pos_base, store_ivs, mark):
        """The middle of every read: the planned records decrypted (an encrypted store), then decoded
        into one chunk area.  Returns (fetch count, chunks, fetch_off, fetch_len) as the assemble and
        verify entry points take them."""
        import torch

        dev = store.device
        # the one host read: the scratch sizes
        chunk_bytes, plain_bytes = (int(v) for v in plan["total_bytes"].tolist())
        k = int(plan["fetch_count"].item())
        src, src_off, src_len = store, plan["src_off"][:k], plan["src_len"][:k]
        dst_off, dst_cap = plan["dst_off"][:k], plan["dst_cap"][:k]
        chunks = torch.empty(chunk_bytes + 64, dtype=torch.uint8, device=dev)
        fetch_len = torch.empty(max(k, 1), dtype=torch.int32, device=dev)[:k]
        if k and self.aes is not None:
            plain = torch.empty(plain_bytes + 64, dtype=torch.uint8, device=dev)
            plain_len = torch.empty(k, dtype=torch.int32, device=dev)
            plain_off = plan["plain_off"][:k]
            ivs = None
            if store_ivs is None and self.iv is None:
                raise ValueError("an encrypted store needs the archive's IV or store_ivs")
            if store_ivs is not None:  # fetch f's directory entry, from any pair that uses it
                pf = plan["pair_fetch"].view(-1)
                used = pf >= 0
                entry = torch.zeros(k, dtype=torch.int64, device=dev)
                entry[pf[used].long()] = pairs.hashloc.view(-1)[used] - int(pos_base)
                ivs = store_ivs[entry].contiguous()
            self.aes.decrypt_device(store, src_off, src_len, plain, plain_off, plain_len,
                                    iv=self.iv if ivs is None else None, ivs=ivs)
            mark("decrypt")
            src, src_off, src_len = plain, plain_off, chain_lens(plain_len, device=self.device)
            mark("chain_lens")
        if k:
            self._z.decompress_device(src, src_off, src_len, chunks, dst_off, dst_cap, fetch_len, framed=True)
        mark("decode")
        if k == 0:  # assemble still needs valid pointers
            dst_off = plan["dst_off"]
            fetch_len = torch.zeros(1, dtype=torch.int32, device=dev)
        return k, chunks, dst_off, fetch_len

    def read(self, map_slots, nbuf: int, slot_len: int, store, store_off, store_len, store_raw_len, pos_base: int,
             verify: bool = False, out=None, stages=None, store_ivs=None):
        """map_slots: device uint8, nbuf slots of slot_len bytes.  store: device uint8 holding the
        putChunk records ``[BE32 nz][payload]`` (AES-CBC ciphertext of them when ``aes`` is set);
        record of hashloc pos_base + k at store[store_off[k] : + store_len[k]], its chunk
        store_raw_len[k] bytes long.  Returns (buffers uint8 [nbuf, chunk_length], status int32
        [nbuf], :class:`ReadInfo`).  ``out``: optional uint8 [nbuf, chunk_length] to write into.  ``stages``: optional callable(name) called after each stage is
        enqueued (measurements).  ``store_ivs``: optional device uint8 [n_store, 16], the IV of each
        directory entry's record, for a store whose archives have IVs of their own
        (``ArchiveSet.record_ivs()``); default: ``iv`` for every record."""
        import torch

        mark = stages or (lambda name: None)
        dev = store.device
        pairs = parse_map_slots(map_slots, nbuf, slot_len, self.hash_len, self.device)
        mark("parse")
        plan = plan_reads(pairs, store_off, store_len, store_raw_len, pos_base, self.device)
        mark("plan")
        k, chunks, dst_off, fetch_len = self._fetch(pairs, plan, store, pos_base, store_ivs, mark)
        out = assemble(pairs, self.chunk_length, plan["pair_fetch"], chunks, dst_off, fetch_len, out=out,
                       device=self.device)
        mark("assemble")
        info = ReadInfo(k, pairs, plan["pair_fetch"])
        if verify:
            if self.engine is None:
                raise ValueError("verify=True needs the hash engine")
            if k:
                info.pair_bad, info.bad_count = verify_reads(self.engine, pairs, plan["pair_fetch"], chunks, dst_off,
                                                             fetch_len, plan["fetch_count"])
            else:
                info.pair_bad = torch.zeros((nbuf, pairs.cap), dtype=torch.uint8, device=dev)
                info.bad_count = torch.zeros(nbuf, dtype=torch.int32, device=dev)
            mark("verify")
        return out, pairs.status[:nbuf], info

    def read_ranges(self, map_slots, nslots: int, slot_len: int, files, requests, store, store_off, store_len,
                    store_raw_len, pos_base: int, verify: bool = False, out=None, stages=None, store_ivs=None):
        """``DedupFileChannel.read`` (DedupFileChannel.java:499-608) for a batch of byte ranges.
        map_slots: device uint8, one map image of nslots slots of slot_len bytes; files: rows of
        (first_slot, n_slots, file_len) over that image; requests: rows of (file, file_pos, siz,
        out_off).  Only the touched slots are parsed and only the records of the pairs that touch a
        range are fetched; the store arguments are :meth:`read`'s.  Returns (out uint8, flat: request
        r's bytes at out[out_off : out_off + n_read[r]]; n_read int64 numpy [n_requests], -1 = at or
        past the end of the file; status int32 [n_requests] (device), the OR of the request's pieces;
        :class:`RangeInfo`).  ``out``: optional device uint8 to write into — no byte outside the
        requests' extents is touched.  A bad record fails only the ranges that touch it, where
        :meth:`read` fails the whole buffer."""
        import numpy as np
        import torch

        mark = stages or (lambda name: None)
        dev = store.device
        pc = split_requests(files, requests, self.chunk_length)
        n_req, npc, nrows = len(pc.n_read), len(pc.req), len(pc.rows)
        if nrows and int(pc.rows[-1]) >= int(nslots):
            raise ValueError(f"a file names slot {int(pc.rows[-1])}, the image holds {nslots}")
        if map_slots.numel() < int(nslots) * int(slot_len):
            raise ValueError(f"map holds {map_slots.numel()} bytes, {nslots} slots of {slot_len} need more")
        need = int((pc.out_off + pc.len).max()) if npc else 0
        if out is None:
            out = torch.zeros(max(need, 1), dtype=torch.uint8, device=dev)[:need]
        elif out.numel() < need or not out.is_contiguous():
            raise ValueError(f"out holds {out.numel()} bytes, the requests end at {need}")
        # one upload: the pieces' int32 columns, then their out_off and the rows as int64
        n4 = (4 * npc + 1) // 2
        host = np.zeros(n4 + npc + nrows + 1, np.int64)
        host[:n4].view(np.int32)[:4 * npc] = np.concatenate([pc.req, pc.row, pc.start, pc.len])
        host[n4:n4 + npc] = pc.out_off
        host[n4 + npc:n4 + npc + nrows] = pc.rows
        d = torch.from_numpy(host).to(dev)
        d32 = d[:n4].view(torch.int32)
        p_req, p_row, p_start, p_len = (d32[i * npc:(i + 1) * npc] for i in range(4))
        p_out, rows = d[n4:n4 + npc], d[n4 + npc:n4 + npc + nrows]
        mark("split")
        images = map_slots[:int(nslots) * int(slot_len)].view(int(nslots), int(slot_len))[rows].contiguous()
        pairs = parse_map_slots(images, nrows, slot_len, self.hash_len, self.device)
        mark("parse")
        plan = plan_pieces(pairs, p_row, p_start, p_len, store_off, store_len, store_raw_len, pos_base, self.device)
        mark("plan")
        k, chunks, dst_off, fetch_len = self._fetch(pairs, plan, store, pos_base, store_ivs, mark)
        status = plan["piece_status"]
        req_status = assemble_pieces(pairs, self.chunk_length, plan["pair_fetch"], chunks, dst_off, fetch_len, p_row,
                                     p_start, p_len, p_out, status, out, piece_req=p_req, n_requests=n_req,
                                     device=self.device)
        mark("assemble")
        info = RangeInfo(k, pc, status, rows, pairs, plan["pair_fetch"])
        if verify:
            if self.engine is None:
                raise ValueError("verify=True needs the hash engine")
            if k and nrows:
                info.pair_bad, info.bad_count = verify_reads(self.engine, pairs, plan["pair_fetch"], chunks, dst_off,
                                                             fetch_len, plan["fetch_count"])
            else:
                info.pair_bad = torch.zeros((nrows, pairs.cap), dtype=torch.uint8, device=dev)
                info.bad_count = torch.zeros(nrows, dtype=torch.int32, device=dev)
            mark("verify")
        return out, pc.n_read, req_status, info

    def read_file(self, map_slots, nslots: int, slot_len: int, file_len: int, file_pos: int, siz: int, store,
                  store_off, store_len, store_raw_len, pos_base: int, verify: bool = False, store_ivs=None):
        """One ``DedupFileChannel.read(buf, 0, siz, file_pos)`` on a file that owns the whole image:
        the bytes read, ``None`` at or past the end of the file (the reference's -1).  Raises
        :class:`SdfsCdcError` when the range's status is not 0, as the Java call throws."""
        out, n_read, status, info = self.read_ranges(map_slots, nslots, slot_len, [(0, nslots, file_len)],
                                                     [(0, file_pos, siz, 0)], store, store_off, store_len,
                                                     store_raw_len, pos_base, verify=verify, store_ivs=store_ivs)
        if int(n_read[0]) < 0:
            return None
        st = int(status[0].item())
        if st:
            raise _lib.SdfsCdcError(st, f"read of [{file_pos}, {file_pos + int(n_read[0])}) failed: "
                                        f"status {st:#x} (SDFS_CDC_READ_* bits)")
        return out[:int(n_read[0])].cpu().numpy().tobytes()
