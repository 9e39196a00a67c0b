"""sdfs_amd — MI355X-native variable-block CDC + fingerprint engine for SDFS's write path.

The drop-in boundary is the C-ABI in ``include/sdfs_cdc.h`` (``libsdfs_cdc.so``, hand-written
gfx950 HIP kernels); this package is the host-side mirror of the reference's
``org.opendedup.hashing`` plugin surface on top of it.  See DESIGN.md / INTEGRATION.md.
"""
from ._lib import MD5, MIN_GE, MIN_GT, RECORD_BYTES, SHA256, SHA256_160, SdfsCdcError  # noqa: F401
from .engine import (  # noqa: F401
    POLY,
    VARIABLE_MD5,
    VARIABLE_SHA256,
    VARIABLE_SHA256_160,
    Finger,
    HashFunctionPool,
    HipVariableMD5HashEngine,
    HipVariableSha256HashEngine,
    SdfsConfig,
)
from .archive import ArchiveSet, HipBlobArchiver, HipBufferWriter  # noqa: F401
from .read import HipBufferReader, assemble_pieces, parse_map_slots, plan_pieces, split_requests  # noqa: F401
from .store import lookup, open_store, scan_store, scrub  # noqa: F401
from .extent import copy_extents, rewrite_blocks, split_extent  # noqa: F401
from .mapfile import close_map, index_map, open_map, snapshot, snapshot_compressed, trim, truncate, vanish  # noqa: F401
from .lz4_stream import HipLz4BlockStream, compressFile, decompressFile, xxh32  # noqa: F401
from .ingest import ChunkBatch, HipChunkIngest, SparseWrites, pack_entries  # noqa: F401
from .replicate import HipFileImport, ImportResult, SourceVolume  # noqa: F401
from .write import HipFileWriter, WriteResult, split_writes  # noqa: F401

__all__ = [
    "HipFileWriter", "WriteResult", "split_writes",
    "HipFileImport", "ImportResult", "SourceVolume",
    "index_map", "snapshot", "vanish", "trim", "truncate", "close_map", "open_map", "snapshot_compressed",
    "HipChunkIngest", "ChunkBatch", "SparseWrites", "pack_entries",
    "HipLz4BlockStream", "compressFile", "decompressFile", "xxh32",
    "ArchiveSet", "HipBlobArchiver", "HipBufferWriter", "HipBufferReader", "parse_map_slots",
    "split_requests", "plan_pieces", "assemble_pieces",
    "open_store", "scan_store", "lookup", "scrub", "copy_extents", "rewrite_blocks", "split_extent",
    "Finger", "HashFunctionPool", "HipVariableMD5HashEngine", "HipVariableSha256HashEngine", "SdfsConfig",
    "SdfsCdcError", "POLY", "VARIABLE_MD5", "VARIABLE_SHA256", "VARIABLE_SHA256_160",
]
