"""Map files at rest on the MI355X: lz4-java's LZ4Block stream (include/sdfs_lz4_stream.h).

With ``compress-metadata`` on, SDFS keeps a closed map file as ``GUID.map.lz4`` =
``CompressionUtils.compressFile`` (CompressionUtils.java:127-139: ``LZ4BlockOutputStream(fos, 1 << 16,
lz4Compressor)``), expands it with ``decompressFile`` (:141-151) before the first slot is read, and moves
every map file to and from a cloud store through the same two functions.

* :class:`HipLz4BlockStream` — ``compress_files`` / ``scan`` / ``decompress_files`` over many files of
  one device tensor, and ``xxh32`` of device extents.
* :func:`compressFile` / :func:`decompressFile` — the two ``CompressionUtils`` functions on host bytes.
* :func:`xxh32` — XXH32 of host bytes (through the GPU).

The LZ4 blocks are those of the :class:`sdfs_amd.lz4.HipLz4Compressor` given (mode ``R123`` = the
reference's).  No CPU fallback: every call runs the HIP kernels and raises :class:`SdfsCdcError`.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import SdfsCdcError, check, stream_of
from .lz4 import R123, HipLz4Compressor

BLOCK = _lib.LZ4S_BLOCK
SEED = _lib.LZ4S_SEED
FLAGS = {_lib.LZ4S_TRUNCATED: "TRUNCATED", _lib.LZ4S_MAGIC: "MAGIC", _lib.LZ4S_HEADER: "HEADER",
         _lib.LZ4S_DECODE: "DECODE", _lib.LZ4S_CHECKSUM: "CHECKSUM", _lib.LZ4S_ROOM: "ROOM"}
_PAD = 64  # room behind the last byte a tensor made here holds, for the block kernels' 16-byte loads


def flag_names(status: int) -> str:
    return "|".join(n for b, n in FLAGS.items() if status & b) or "OK"


def stream_level(block_size: int) -> int:
    """The token's low nibble for a block size (LZ4BlockOutputStream.compressionLevel - 10)."""
    lv = int(_lib.load().sdfs_cdc_lz4_stream_level(int(block_size)))
    if lv < 0:
        raise ValueError(f"block_size {block_size}: 64 .. 2^25")
    return lv


def stream_bound(n: int, block_size: int = BLOCK) -> int:
    """Exact room a stream of ``n`` input bytes can need."""
    stream_level(block_size)
    return int(_lib.load().sdfs_cdc_lz4_stream_bound(int(n), int(block_size)))


def _u64(a):
    return np.ascontiguousarray(a, np.uint64)


class StreamScan:
    """What ``scan`` found (device tensors): ``files`` int64[n, 3] = {status | n_blocks << 32,
    decoded_len, consumed}; ``blocks`` the block table, 32 bytes an entry; ``table_base`` the first
    entry of each file (host)."""

    def __init__(self, files, blocks, table_base):
        self.files, self.blocks, self.table_base = files, blocks, table_base

    def host(self):
        """(status, n_blocks, decoded_len, consumed) as numpy arrays: one host read."""
        f = self.files.cpu().numpy().view(np.uint64).reshape(-1, 3)
        return ((f[:, 0] & 0xFFFFFFFF).astype(np.uint32), (f[:, 0] >> 32).astype(np.uint32), f[:, 1].copy(),
                f[:, 2].copy())


class HipLz4BlockStream:
    def __init__(self, compressor: HipLz4Compressor | None = None, device: int = 0):
        self.z = compressor if compressor is not None else HipLz4Compressor(R123, device)
        self._lib = _lib.load()

    # ---- XXH32
    def xxh32(self, data, off, length, seed: int = 0, count=None, stream=None):
        """XXH32 of extents data[off[i] : off[i] + length[i]] (device tensors: data u8, off i64[n],
        length i32[n]); returns int32[n] on the device (the hash's bits)."""
        import torch

        n = int(length.shape[0])
        out = torch.empty(max(n, 1), dtype=torch.int32, device=data.device)
        check(self._lib.sdfs_cdc_xxh32_device(self.z._h, data.data_ptr(), off.data_ptr(), length.data_ptr(),
                                              _lib.ptr(count), n, int(seed) & 0xFFFFFFFF, out.data_ptr(),
                                              stream_of(data, stream)))
        return out[:n]

    # ---- compressFile
    def compress_files(self, data, offs, lens, block_size: int = BLOCK, stream=None):
        """Files data[offs[f] : offs[f] + lens[f]] of the device tensor ``data`` (u8) as LZ4Block
        streams.  Returns (out u8 tensor, out_offs numpy u64[n], out_lens device int64[n]): stream f
        is out[out_offs[f] : out_offs[f] + out_lens[f]].  Nothing waits on the host."""
        import torch

        offs, lens = _u64(offs), _u64(lens)
        n = len(lens)
        room = np.array([stream_bound(int(k), block_size) for k in lens], np.uint64)
        out_offs = np.concatenate([[0], np.cumsum(room)[:-1]]).astype(np.uint64) if n else room
        out = torch.empty(int(room.sum()) + _PAD, dtype=torch.uint8, device=data.device)
        out_lens = torch.zeros(max(n, 1), dtype=torch.int64, device=data.device)
        check(self._lib.sdfs_cdc_lz4_stream_compress_device(
            self.z._h, data.data_ptr(), offs.ctypes.data, lens.ctypes.data, n, int(block_size), out.data_ptr(),
            out_offs.ctypes.data, out_lens.data_ptr(), stream_of(data, stream)))
        return out, out_offs, out_lens[:n]

    # ---- decompressFile
    def scan(self, data, offs, lens, stream=None) -> StreamScan:
        """The header walk of streams data[offs[f] : offs[f] + lens[f]]: status, sizes and the
        block table, on the device."""
        import torch

        offs, lens = _u64(offs), _u64(lens)
        n = len(lens)
        cap = np.array([int(self._lib.sdfs_cdc_lz4_stream_max_blocks(int(k))) for k in lens], np.uint64)
        base = np.concatenate([[0], np.cumsum(cap)[:-1]]).astype(np.uint64) if n else cap
        files = torch.zeros((max(n, 1), 3), dtype=torch.int64, device=data.device)
        blocks = torch.empty((max(int(cap.sum()), 1), 4), dtype=torch.int64, device=data.device)
        check(self._lib.sdfs_cdc_lz4_stream_scan_device(
            self.z._h, data.data_ptr(), offs.ctypes.data, lens.ctypes.data, n, files.data_ptr(), blocks.data_ptr(),
            base.ctypes.data, stream_of(data, stream)))
        return StreamScan(files[:n], blocks, base)

    def decompress_files(self, data, offs, lens, stream=None):
        """Streams data[offs[f] : offs[f] + lens[f]] decoded.  Returns (out u8 tensor, out_offs numpy
        u64[n], decoded_lens numpy u64[n], status numpy u32[n], consumed numpy u64[n]): file f is
        out[out_offs[f] : out_offs[f] + decoded_lens[f]] when status[f] is 0, and not to be used
        otherwise.  One host read of the scan's sizes (to allocate), one of the final status."""
        import torch

        sc = self.scan(data, offs, lens, stream)
        _, n_blocks, decoded, consumed = sc.host()
        n = len(decoded)
        room = (decoded + np.uint64(15)) & ~np.uint64(15)
        out_offs = np.concatenate([[0], np.cumsum(room)[:-1]]).astype(np.uint64) if n else room
        out = torch.empty(int(room.sum()) + _PAD, dtype=torch.uint8, device=data.device)
        cap = _u64(decoded)
        check(self._lib.sdfs_cdc_lz4_stream_decompress_device(
            self.z._h, data.data_ptr(), n, sc.files.data_ptr(), sc.blocks.data_ptr(), sc.table_base.ctypes.data,
            int(n_blocks.astype(np.uint64).sum()), out.data_ptr(), out_offs.ctypes.data, cap.ctypes.data,
            stream_of(data, stream)))
        status = sc.host()[0]
        return out, out_offs, decoded, status, consumed

    # ---- host bytes
    def compressFile(self, data, block_size: int = BLOCK) -> bytes:
        import torch

        a = np.frombuffer(bytes(data), np.uint8)
        d = torch.zeros(len(a) + _PAD, dtype=torch.uint8, device=f"cuda:{self.z.device}")
        if len(a):
            d[: len(a)] = torch.from_numpy(a.copy())
        out, _, out_lens = self.compress_files(d, [0], [len(a)], block_size)
        return out[: int(out_lens[0])].cpu().numpy().tobytes()

    def decompressFile(self, data) -> bytes:
        import torch

        a = np.frombuffer(bytes(data), np.uint8)
        d = torch.zeros(len(a) + _PAD, dtype=torch.uint8, device=f"cuda:{self.z.device}")
        if len(a):
            d[: len(a)] = torch.from_numpy(a.copy())
        out, _, decoded, status, _ = self.decompress_files(d, [0], [len(a)])
        if status[0]:
            raise SdfsCdcError(_lib.EINVAL, f"LZ4Block stream is corrupted: {flag_names(int(status[0]))}")
        return out[: int(decoded[0])].cpu().numpy().tobytes()


_default = {}


def _codec(mode: int = R123, device: int = 0) -> HipLz4BlockStream:
    key = (mode, device)
    if key not in _default:
        _default[key] = HipLz4BlockStream(HipLz4Compressor(mode, device))
    return _default[key]


def compressFile(data, mode: int = R123, device: int = 0) -> bytes:
    """CompressionUtils.compressFile (CompressionUtils.java:127-139) on host bytes, on the GPU."""
    return _codec(mode, device).compressFile(data)


def decompressFile(data, device: int = 0) -> bytes:
    """CompressionUtils.decompressFile (CompressionUtils.java:141-151) on host bytes, on the GPU;
    raises :class:`SdfsCdcError` naming the flags where LZ4BlockInputStream throws."""
    return _codec(R123, device).decompressFile(data)


def xxh32(data, seed: int = 0, device: int = 0) -> int:
    """XXH32 of host bytes with a seed (through the GPU)."""
    import torch

    a = np.frombuffer(bytes(data), np.uint8)
    dev = f"cuda:{device}"
    d = torch.zeros(len(a) + _PAD, dtype=torch.uint8, device=dev)
    if len(a):
        d[: len(a)] = torch.from_numpy(a.copy())
    off = torch.zeros(1, dtype=torch.int64, device=dev)
    ln = torch.tensor([len(a)], dtype=torch.int32, device=dev)
    return int(_codec(R123, device).xxh32(d, off, ln, seed)[0]) & 0xFFFFFFFF
