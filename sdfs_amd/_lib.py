"""ctypes binding of ``libsdfs_cdc.so`` (the C-ABI declared in ``include/sdfs_cdc.h``).

The product path has no CPU fallback: if the HIP library is missing this module raises at import
of the engine (``load()``), and every C-ABI error surfaces as :class:`SdfsCdcError` (the Python
analogue of the ``IOException`` that ``getChunks`` throws in the reference,
SparseDedupFile.java:578-580).
"""
from __future__ import annotations

import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# SDFS_CDC_LIB selects the in-tree measurement build (libsdfs_cdc_tuning.so: kernel-variant
# sweeps and A/B switches, scripts/sweep_scan.py); the default is the product library
DEFAULT_LIB = os.path.join(HERE, "libsdfs_cdc.so")
TUNING_LIB = os.path.join(HERE, "libsdfs_cdc_tuning.so")
LIB_PATH = os.environ.get("SDFS_CDC_LIB") or DEFAULT_LIB
HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "sdfs_cdc.h")
HEADER_PATHS = [HEADER_PATH] + [os.path.join(os.path.dirname(HERE), "include", h)
                               for h in ("sdfs_index.h", "sdfs_lz4.h", "sdfs_meta.h", "sdfs_aes.h", "sdfs_read.h", "sdfs_archive.h", "sdfs_store.h",
                                         "sdfs_extent.h", "sdfs_lz4_stream.h", "sdfs_ingest.h", "sdfs_import.h", "sdfs_write.h")]

OK, EINVAL, ECAP, EHIP, ENOMEM, ENODEV = 0, -1, -2, -3, -4, -5
FLAG_DIRECT = 1  # SDFS_CDC_FLAG_DIRECT: no coalescing of concurrent getChunks/getHash calls
SHA256, SHA256_160, MD5 = 0, 1, 2
MIN_GT, MIN_GE = 0, 1
PRED_MASK, PRED_DIV = 0, 1  # sdfs_cdc_params.pred_kind: (fp & mask) == value / fp % div == rem
RECORD_BYTES = 48
NO_STREAM = (1 << 64) - 1  # SDFS_CDC_NO_STREAM
ALL_DEVICES = -1           # sdfs_cdc_params.device: every gfx950 device
FILL_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32)


class SdfsCdcError(IOError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"sdfs_cdc error {code}: {msg}")
        self.code = code


class Params(ctypes.Structure):
    """``sdfs_cdc_params`` (include/sdfs_cdc.h)."""

    _fields_ = [
        ("poly", ctypes.c_uint64),
        ("window", ctypes.c_uint32),
        ("min_len", ctypes.c_uint32),
        ("max_len", ctypes.c_uint32),
        ("chunk_length", ctypes.c_uint32),
        ("pred_mask", ctypes.c_uint64),
        ("pred_value", ctypes.c_uint64),
        ("min_cmp", ctypes.c_uint32),
        ("hash_algo", ctypes.c_uint32),
        ("device", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
        ("max_batch_bytes", ctypes.c_uint64),
        ("device_mask", ctypes.c_uint64),
        ("pred_kind", ctypes.c_uint32),  # ABI 3: boundary detector form
        ("reserved2", ctypes.c_uint32),
        ("pred_div", ctypes.c_uint64),
        ("pred_rem", ctypes.c_uint64),
    ]


class DevOut(ctypes.Structure):
    """``sdfs_cdc_dev_out``: device pointers for the device-resident path."""

    _fields_ = [
        ("counts", ctypes.c_void_p),
        ("starts", ctypes.c_void_p),
        ("lens", ctypes.c_void_p),
        ("digests", ctypes.c_void_p),
        ("cap", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("records", ctypes.c_void_p),
        ("records_cap", ctypes.c_uint64),
        ("total", ctypes.c_void_p),
    ]


class Pairs(ctypes.Structure):
    """``sdfs_cdc_pairs`` (include/sdfs_read.h): device pointers of the parsed HashLocPairs."""

    _fields_ = [
        ("counts", ctypes.c_void_p),
        ("hashes", ctypes.c_void_p),
        ("hashloc", ctypes.c_void_p),
        ("len", ctypes.c_void_p),
        ("pos", ctypes.c_void_p),
        ("offset", ctypes.c_void_p),
        ("nlen", ctypes.c_void_p),
        ("doop", ctypes.c_void_p),
        ("flags", ctypes.c_void_p),
        ("status", ctypes.c_void_p),
        ("cap", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


class ArchiveLayout(ctypes.Structure):
    """``sdfs_cdc_archive_layout`` (include/sdfs_archive.h): device pointers of where a call's records lie."""

    _fields_ = [
        ("arc", ctypes.c_void_p),
        ("pos", ctypes.c_void_p),
        ("store_off", ctypes.c_void_p),
        ("arc_first", ctypes.c_void_p),
        ("arc_bytes", ctypes.c_void_p),
        ("arc_base", ctypes.c_void_p),
        ("totals", ctypes.c_void_p),
        ("status", ctypes.c_void_p),
        ("arc_cap", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


class ArchiveKept(ctypes.Structure):
    """``sdfs_cdc_archive_kept``: what compaction lays out for the surviving records."""

    _fields_ = [
        ("new_of_old", ctypes.c_void_p),
        ("sel", ctypes.c_void_p),
        ("src_off", ctypes.c_void_p),
        ("rec_len", ctypes.c_void_p),
        ("count", ctypes.c_void_p),
        ("deleted", ctypes.c_void_p),
        ("new_arc", ctypes.c_void_p),
        ("map_slots", ctypes.c_void_p),
        ("lay", ArchiveLayout),
    ]


ARCHIVE_ALIGN, ARCHIVE_HEADER, ARCHIVE_NONE = 4096, 1024, 0xFFFFFFFF  # SDFS_CDC_ARCHIVE_*
ARCHIVE_ECAP, ARCHIVE_ESTORE = 1, 2


class StoreRecords(ctypes.Structure):
    """``sdfs_cdc_store_records`` (include/sdfs_store.h): the scan's record list."""

    _fields_ = [
        ("arc", ctypes.c_void_p),
        ("slot", ctypes.c_void_p),
        ("pos", ctypes.c_void_p),
        ("len", ctypes.c_void_p),
        ("store_off", ctypes.c_void_p),
        ("key", ctypes.c_void_p),
        ("raw_len", ctypes.c_void_p),
        ("flags", ctypes.c_void_p),
        ("count", ctypes.c_void_p),
        ("status", ctypes.c_void_p),
        ("n_cap", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


class StoreArchives(ctypes.Structure):
    """``sdfs_cdc_store_archives``: the scan's per-archive outputs."""

    _fields_ = [
        ("map_slots", ctypes.c_void_p),
        ("version", ctypes.c_void_p),
        ("arc_first", ctypes.c_void_p),
        ("ivs", ctypes.c_void_p),
        ("slot_rec", ctypes.c_void_p),
        ("status", ctypes.c_void_p),
        ("slot_stride", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


# SDFS_CDC_STORE_*: record flags, archive status, the scan's status word
STORE_RANGE, STORE_KEY, STORE_LEN, STORE_NZ, STORE_FETCH, STORE_HASH = 1, 2, 4, 8, 16, 32
STORE_UNREADABLE = STORE_RANGE | STORE_LEN | STORE_NZ
STORE_GAP, STORE_SLOTS = 1, 2
STORE_ECAP = 1
STORE_SORT_LDS = 16384

# SDFS_CDC_LZ4_STREAM_*: a stream's status word
LZ4S_TRUNCATED, LZ4S_MAGIC, LZ4S_HEADER, LZ4S_DECODE, LZ4S_CHECKSUM, LZ4S_ROOM = 1, 2, 4, 8, 16, 32
LZ4S_HEADER_BYTES, LZ4S_SEED, LZ4S_BLOCK = 21, 0x9747B28C, 65536

READ_CORRUPT, READ_MISSING, READ_FETCH, READ_BOUNDS = 1, 2, 4, 8  # SDFS_CDC_READ_*
READ_NONE = 0xFFFFFFFF


class Segment(ctypes.Structure):
    """``sdfs_cdc_segment`` (include/sdfs_extent.h)."""

    _fields_ = [("src_buf", ctypes.c_uint32), ("src_off", ctypes.c_uint32), ("dst_buf", ctypes.c_uint32),
                ("dst_off", ctypes.c_uint32), ("len", ctypes.c_uint32)]


class Run(ctypes.Structure):
    """``sdfs_cdc_run``."""

    _fields_ = [("dst_buf", ctypes.c_uint32), ("run_pos", ctypes.c_uint32)]


class Inserts(ctypes.Structure):
    """``sdfs_cdc_inserts``: device pointers of an insert list."""

    _fields_ = [("hash", ctypes.c_void_p), ("hashloc", ctypes.c_void_p), ("len", ctypes.c_void_p),
                ("pos", ctypes.c_void_p), ("offset", ctypes.c_void_p), ("nlen", ctypes.c_void_p),
                ("dst_buf", ctypes.c_void_p)]


# SDFS_CDC_EXT_*
EXT_CORRUPT, EXT_OVERLAP, EXT_BAD_INSERT, EXT_OVERFLOW, EXT_ECAP, EXT_HOLE, EXT_SRC = 1, 2, 4, 8, 16, 32, 64

class IngestBatch(ctypes.Structure):
    """``sdfs_cdc_ingest_batch`` (include/sdfs_ingest.h): the client's entries, device pointers."""

    _fields_ = [("hash", ctypes.c_void_p), ("blob", ctypes.c_void_p), ("blob_bytes", ctypes.c_uint64),
                ("off", ctypes.c_void_p), ("len", ctypes.c_void_p), ("raw_len", ctypes.c_void_p),
                ("compressed", ctypes.c_void_p), ("n", ctypes.c_uint64)]


class IngestPlan(ctypes.Structure):
    """``sdfs_cdc_ingest_plan``: what the plan lays out, device pointers."""

    _fields_ = [("status", ctypes.c_void_p), ("stage_off", ctypes.c_void_p), ("rec_of", ctypes.c_void_p),
                ("dec_src_off", ctypes.c_void_p), ("dec_src_len", ctypes.c_void_p), ("dec_dst_off", ctypes.c_void_p),
                ("dec_cap", ctypes.c_void_p), ("dec_len", ctypes.c_void_p), ("dec_entry", ctypes.c_void_p),
                ("dec_count", ctypes.c_void_p), ("staged", ctypes.c_void_p)]


# SDFS_CDC_INGEST_*
INGEST_EMPTY, INGEST_EBOUNDS, INGEST_EDECODE, INGEST_EHASH, INGEST_EMISSED = 1, 2, 4, 8, 16
INGEST_NONE, INGEST_TILE, INGEST_COPY_SPAN = 0xFFFFFFFF, 1024, 65536

class ImportWork(ctypes.Structure):
    """``sdfs_cdc_import_work`` (include/sdfs_import.h): what the calls of one import share, device pointers."""

    _fields_ = [("hashes", ctypes.c_void_p), ("src_hashloc", ctypes.c_void_p), ("counting", ctypes.c_void_p),
                ("status", ctypes.c_void_p), ("req_pairs", ctypes.c_void_p), ("req_missed", ctypes.c_void_p),
                ("pair_fetch", ctypes.c_void_p), ("pair_rec", ctypes.c_void_p), ("counts", ctypes.c_void_p)]


# SDFS_CDC_IMPORT_*
IMPORT_EMISSING, IMPORT_EFETCH, IMPORT_EHASH = 32, 64, 128
IMPORT_NONE, IMPORT_BLOCK, IMPORT_SPAN = 0xFFFFFFFF, 1024, 16384

class WritePlan(ctypes.Structure):
    """``sdfs_cdc_write_plan`` (include/sdfs_write.h): the write split's outputs, host pointers."""

    _fields_ = [("piece_cap", ctypes.c_uint32), ("run_cap", ctypes.c_uint32), ("row_cap", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("piece_row", ctypes.c_void_p), ("piece_start", ctypes.c_void_p),
                ("piece_len", ctypes.c_void_p), ("piece_req", ctypes.c_void_p), ("piece_src_off", ctypes.c_void_p),
                ("run_row", ctypes.c_void_p), ("run_pos", ctypes.c_void_p), ("run_len", ctypes.c_void_p),
                ("run_first_piece", ctypes.c_void_p), ("run_n_pieces", ctypes.c_void_p), ("row_slot", ctypes.c_void_p),
                ("row_full", ctypes.c_void_p), ("n_pieces", ctypes.c_uint64), ("n_runs", ctypes.c_uint64),
                ("n_rows", ctypes.c_uint64)]


# SDFS_CDC_WRITE_*
WRITE_SLOT, WRITE_READ, WRITE_BOUNDS = 1, 2, 4
WRITE_SPAN = 65536

# (name, restype, argtypes) for every entry point of include/sdfs_cdc.h
_P = ctypes.POINTER
_u8p, _u32p, _u64p, _vp = _P(ctypes.c_uint8), _P(ctypes.c_uint32), _P(ctypes.c_uint64), ctypes.c_void_p
SIGNATURES = {
    "sdfs_cdc_abi_version": (ctypes.c_int, []),
    "sdfs_cdc_params_default": (ctypes.c_int, [_P(Params), ctypes.c_int]),
    "sdfs_cdc_create": (ctypes.c_int, [_P(Params), _P(_vp)]),
    "sdfs_cdc_destroy": (ctypes.c_int, [_vp]),
    "sdfs_cdc_last_error": (ctypes.c_char_p, []),
    "sdfs_cdc_is_variable_length": (ctypes.c_int, [_vp]),
    "sdfs_cdc_get_max_len": (ctypes.c_int, [_vp]),
    "sdfs_cdc_get_min_len": (ctypes.c_int, [_vp]),
    "sdfs_cdc_set_seed": (ctypes.c_int, [_vp, ctypes.c_int]),
    "sdfs_cdc_digest_len": (ctypes.c_int, [_vp]),
    "sdfs_cdc_slot_cap": (ctypes.c_uint32, [_vp, ctypes.c_uint64]),
    "sdfs_cdc_get_hash": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp]),
    "sdfs_cdc_get_chunks": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_uint32, _u32p]),
    "sdfs_cdc_get_chunks_stream": (ctypes.c_int, [_vp, ctypes.c_uint64, _vp, ctypes.c_uint32, _vp, _vp, _vp,
                                                  ctypes.c_uint32, _u32p]),
    "sdfs_cdc_get_chunks_fill": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint32, FILL_FN, _vp, _vp, _vp, _vp,
                                                ctypes.c_uint32, _u32p]),
    "sdfs_cdc_device_count": (ctypes.c_int, [_vp]),
    "sdfs_cdc_device_ordinal": (ctypes.c_int, [_vp, ctypes.c_int]),
    "sdfs_cdc_share_count": (ctypes.c_int, [_vp]),
    "sdfs_cdc_kernel_times_on": (ctypes.c_int, [_vp, ctypes.c_int, _P(ctypes.c_char_p), _P(ctypes.c_float),
                                                ctypes.c_int]),
    "sdfs_cdc_allgather_records": (ctypes.c_int, [_vp, _P(_vp), _u64p, _P(_vp), _P(_vp), ctypes.c_uint64, _u32p,
                                                  _u64p, _P(_vp)]),
    "sdfs_cdc_get_chunks_batch": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, _vp,
                                                 ctypes.c_uint32]),
    "sdfs_cdc_run_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64,
                                           _P(DevOut), _vp]),
    "sdfs_cdc_run_device_ragged": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint32,
                                                  ctypes.c_uint64, _P(DevOut), _vp]),
    "sdfs_cdc_stream_sync": (ctypes.c_int, [_vp]),
    "sdfs_cdc_queue_stats": (ctypes.c_int, [_vp, _u64p, _u64p]),
    "sdfs_cdc_queue_early": (ctypes.c_int, [_vp, _u64p]),
    "sdfs_cdc_queue_timing": (ctypes.c_int, [_vp, _P(ctypes.c_double), _P(ctypes.c_double), _P(ctypes.c_double)]),
    "sdfs_cdc_set_timing": (ctypes.c_int, [_vp, ctypes.c_int]),
    "sdfs_cdc_set_timing_mask": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_uint32]),
    "sdfs_cdc_kernel_times": (ctypes.c_int, [_vp, _P(ctypes.c_char_p), _P(ctypes.c_float), ctypes.c_int]),
    "sdfs_cdc_synth_device": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                             ctypes.c_uint64, _vp]),
    "sdfs_cdc_host_register": (ctypes.c_int, [_vp, ctypes.c_uint64]),
    "sdfs_cdc_host_unregister": (ctypes.c_int, [_vp]),
    "sdfs_cdc_get_hash_batch": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint32, _vp]),
    "sdfs_cdc_hash_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_uint64, _vp, _vp]),
    # include/sdfs_index.h
    "sdfs_cdc_index_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint64, _P(_vp)]),
    "sdfs_cdc_index_destroy": (ctypes.c_int, [_vp]),
    "sdfs_cdc_index_put_records": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, ctypes.c_uint64, _vp, _vp, _vp,
                                                  _vp, _vp]),
    "sdfs_cdc_index_get": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, _vp, _vp]),
    "sdfs_cdc_index_size": (ctypes.c_int, [_vp, _u64p, _u64p]),
    "sdfs_cdc_index_clear": (ctypes.c_int, [_vp, _vp]),
    "sdfs_cdc_index_set_epoch": (ctypes.c_int, [_vp, ctypes.c_uint32]),
    "sdfs_cdc_index_claim": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint64, _vp, _vp]),
    "sdfs_cdc_index_sweep": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, _vp, _vp]),
    "sdfs_cdc_index_compact": (ctypes.c_int, [_vp, _vp]),
    "sdfs_cdc_index_stats": (ctypes.c_int, [_vp, _u64p, _u64p, _u64p]),
    "sdfs_cdc_index_claim_slots": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _vp,
                                                  ctypes.c_int64, ctypes.c_int, _vp, _vp, _vp, _vp]),
    "sdfs_cdc_index_recount": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _vp,
                                              ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint64, _vp, _vp]),
    "sdfs_cdc_index_addref_slots": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _vp,
                                                   ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_uint64, _vp, _vp]),
    "sdfs_cdc_index_load": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint64, _vp, _vp]),
    "sdfs_cdc_index_export": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint64, _vp, _vp]),
    # include/sdfs_lz4.h
    "sdfs_cdc_lz4_bound": (ctypes.c_uint64, [ctypes.c_uint64]),
    "sdfs_cdc_lz4_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _P(_vp)]),
    "sdfs_cdc_lz4_destroy": (ctypes.c_int, [_vp]),
    "sdfs_cdc_lz4_hybrid_min_items": (ctypes.c_uint64, [_vp]),
    "sdfs_cdc_lz4_compress_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_uint64, _vp, _vp, _vp,
                                                    ctypes.c_int, _vp]),
    "sdfs_cdc_lz4_plan_records": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint64, ctypes.c_uint64,
                                                 ctypes.c_uint32, _vp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp]),
    "sdfs_cdc_lz4_compress": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, _vp, ctypes.c_uint32, _u32p]),
    "sdfs_cdc_lz4_compress_batch": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp,
                                                   ctypes.c_int]),
    "sdfs_cdc_lz4_decompress_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_uint64, _vp, _vp, _vp, _vp,
                                                      ctypes.c_int, _vp]),
    "sdfs_cdc_lz4_decompress": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, _vp, ctypes.c_uint32]),
    # include/sdfs_meta.h
    "sdfs_cdc_map_slot_bytes": (ctypes.c_uint32, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]),
    "sdfs_cdc_map_emit": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint32, _P(DevOut), ctypes.c_uint32, _vp, _vp, _vp,
                                         ctypes.c_uint32, _vp, _vp, _vp]),
    # include/sdfs_aes.h
    "sdfs_cdc_aes_cbc_bound": (ctypes.c_uint64, [ctypes.c_uint64]),
    "sdfs_cdc_aes_create": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_uint32, _P(_vp)]),
    "sdfs_cdc_aes_destroy": (ctypes.c_int, [_vp]),
    "sdfs_cdc_aes_encrypt_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_uint64, ctypes.c_int,
                                                   ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sdfs_cdc_aes_decrypt_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_uint64, _vp, _vp, _vp, _vp,
                                                   _vp, _vp]),
    "sdfs_cdc_aes_encrypt": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_int, ctypes.c_int32, _vp, _vp,
                                            ctypes.c_uint64, _u64p]),
    "sdfs_cdc_aes_decrypt": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint64, _u64p]),
    "sdfs_cdc_aes_encrypt_batch": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint32, ctypes.c_int, ctypes.c_int32,
                                                  _vp, _vp, _vp, _vp]),
    # include/sdfs_read.h
    "sdfs_cdc_map_pair_cap": (ctypes.c_uint32, [ctypes.c_uint32, ctypes.c_uint32]),
    "sdfs_cdc_map_parse": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint32, _vp, ctypes.c_uint32, ctypes.c_uint32,
                                          _P(Pairs), _vp]),
    "sdfs_cdc_read_plan": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint32, _P(Pairs), ctypes.c_uint64, ctypes.c_uint64,
                                          _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sdfs_cdc_read_chain_lens": (ctypes.c_int, [ctypes.c_int, _vp, _vp, ctypes.c_uint64, _vp, _vp]),
    "sdfs_cdc_read_assemble": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, _P(Pairs), _vp, _vp,
                                              _vp, _vp, _vp, _vp]),
    "sdfs_cdc_read_verify": (ctypes.c_int, [_vp, ctypes.c_uint32, _P(Pairs), ctypes.c_uint32, _vp, _vp, _vp, _vp,
                                            _vp, ctypes.c_uint64, _vp, _vp, _vp]),
    "sdfs_cdc_read_split": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp,
                                           ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint32, _vp, _u64p,
                                           _u64p]),
    "sdfs_cdc_read_plan_pieces": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint32, _P(Pairs), ctypes.c_uint64,
                                                 ctypes.c_uint64, _vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, _vp,
                                                 _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sdfs_cdc_read_assemble_pieces": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, _P(Pairs), _vp,
                                                     _vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp,
                                                     ctypes.c_uint32, _vp, _vp, _vp]),
    # include/sdfs_archive.h
    "sdfs_cdc_archive_map_size": (ctypes.c_uint32, [ctypes.c_uint64]),
    "sdfs_cdc_archive_pack_span": (ctypes.c_uint32, []),
    "sdfs_cdc_archive_map_bytes": (ctypes.c_uint64, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]),
    "sdfs_cdc_archive_plan": (ctypes.c_int, [ctypes.c_int, _vp, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                             _u64p, ctypes.c_uint32, ctypes.c_uint32, _P(ArchiveLayout), _vp]),
    "sdfs_cdc_archive_pack": (ctypes.c_int, [ctypes.c_int, _P(ArchiveLayout), _vp, ctypes.c_uint64, _vp, _vp, _vp,
                                             ctypes.c_int, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                             _vp, _vp, ctypes.c_uint64, _vp]),
    "sdfs_cdc_archive_map_emit": (ctypes.c_int, [ctypes.c_int, _P(ArchiveLayout), _vp, ctypes.c_uint64, _vp, _vp, _vp,
                                                 ctypes.c_uint32, ctypes.c_uint32, _vp, ctypes.c_uint32, _vp, _vp, _vp,
                                                 _vp]),
    "sdfs_cdc_archive_compact_select": (ctypes.c_int, [ctypes.c_int, _P(ArchiveLayout), ctypes.c_uint64, ctypes.c_uint32,
                                                       _vp, _vp, _vp, _vp, ctypes.c_uint32, _vp, ctypes.c_uint32,
                                                       ctypes.c_uint32, _P(ArchiveKept), _vp]),
    "sdfs_cdc_archive_compact": (ctypes.c_int, [ctypes.c_int, _P(ArchiveLayout), ctypes.c_uint64, ctypes.c_uint32, _vp,
                                                _vp, _vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, ctypes.c_uint32,
                                                ctypes.c_uint32, ctypes.c_uint32, _vp, _P(ArchiveKept), _vp,
                                                ctypes.c_uint64, ctypes.c_uint32, _vp, _vp, _vp, _vp]),
    # include/sdfs_store.h
    "sdfs_cdc_store_scan": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint32, _vp, ctypes.c_uint64, _vp, _vp, _vp,
                                           ctypes.c_uint64, _u64p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                           ctypes.c_uint32, ctypes.c_int, _P(StoreRecords), _P(StoreArchives), _vp]),
    "sdfs_cdc_store_raw_lens": (ctypes.c_int, [ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_uint64, ctypes.c_uint32, _vp,
                                               _vp, _vp]),
    "sdfs_cdc_store_directory": (ctypes.c_int, [ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint64,
                                                ctypes.c_uint64, ctypes.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sdfs_cdc_store_lookup": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint32, _vp, ctypes.c_uint64, _vp, _vp, _vp,
                                             ctypes.c_uint64, _u64p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                             _vp, _vp, ctypes.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sdfs_cdc_store_verify": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint64, ctypes.c_uint32, _vp, _vp]),
    # include/sdfs_extent.h
    "sdfs_cdc_map_extents": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint32, _P(Pairs), ctypes.c_uint32, ctypes.c_uint32,
                                            ctypes.c_uint32, _vp, _vp, _P(Inserts), ctypes.c_uint64, _vp, _vp, _vp]),
    "sdfs_cdc_map_inserts_from_chunks": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint32, _P(DevOut), ctypes.c_uint32, _vp,
                                                        ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _P(Inserts),
                                                        ctypes.c_uint64, _vp, _vp]),
    "sdfs_cdc_map_insert": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _P(Pairs),
                                           _P(Inserts), ctypes.c_uint64, _vp, _P(Pairs), _vp, _vp, _vp]),
    "sdfs_cdc_map_emit_pairs": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint32, _P(Pairs), ctypes.c_uint32, _vp, _vp,
                                               ctypes.c_uint8, _vp, ctypes.c_uint32, _vp, _vp, _vp]),
    # include/sdfs_lz4_stream.h
    "sdfs_cdc_lz4_stream_level": (ctypes.c_int, [ctypes.c_uint32]),
    "sdfs_cdc_lz4_stream_bound": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint32]),
    "sdfs_cdc_lz4_stream_max_blocks": (ctypes.c_uint64, [ctypes.c_uint64]),
    "sdfs_cdc_xxh32_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_uint64, ctypes.c_uint32, _vp, _vp]),
    "sdfs_cdc_lz4_stream_compress_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp,
                                                           _vp, _vp, _vp]),
    "sdfs_cdc_lz4_stream_scan_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, _vp]),
    "sdfs_cdc_lz4_stream_decompress_device": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_uint64,
                                                             _vp, _vp, _vp, _vp]),
    # include/sdfs_ingest.h
    "sdfs_cdc_ingest_chunks_plan": (ctypes.c_int, [ctypes.c_int, _P(IngestBatch), ctypes.c_uint32, ctypes.c_uint64,
                                                   _P(IngestPlan), _vp]),
    "sdfs_cdc_ingest_chunks_decode": (ctypes.c_int, [_vp, _P(IngestBatch), _P(IngestPlan), _vp, _vp]),
    "sdfs_cdc_ingest_chunks_copy": (ctypes.c_int, [ctypes.c_int, _P(IngestBatch), _P(IngestPlan), ctypes.c_uint32, _vp,
                                                   _vp]),
    "sdfs_cdc_ingest_chunks_verify": (ctypes.c_int, [_vp, _P(IngestBatch), _P(IngestPlan), _vp, ctypes.c_uint32, _vp]),
    "sdfs_cdc_ingest_chunks_records": (ctypes.c_int, [ctypes.c_int, _P(IngestBatch), _P(IngestPlan), _vp, _vp, _vp]),
    "sdfs_cdc_ingest_chunks_results": (ctypes.c_int, [ctypes.c_int, _P(IngestBatch), _P(IngestPlan), _vp, _vp,
                                                      ctypes.c_uint64, _vp, ctypes.c_uint64, _vp, _vp, _vp, _vp, _vp]),
    # include/sdfs_import.h
    "sdfs_cdc_import_pairs": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                             ctypes.c_uint32, _P(ImportWork), _vp]),
    "sdfs_cdc_import_plan": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32, _P(ImportWork), _vp,
                                            ctypes.c_uint64, ctypes.c_uint64, _vp, _vp, _vp, ctypes.c_uint32, _vp, _vp,
                                            _vp, _vp, _vp, _vp, _vp, _vp]),
    "sdfs_cdc_import_records": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                               _P(ImportWork), _vp, ctypes.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp,
                                               _vp]),
    "sdfs_cdc_import_install": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                               ctypes.c_uint32, _P(ImportWork), _vp, _vp, _vp, ctypes.c_uint32, _vp,
                                               ctypes.c_uint64, _vp, _vp]),
    "sdfs_cdc_import_check_dests": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64]),
    # include/sdfs_write.h
    "sdfs_cdc_write_split": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64,
                                            _vp, _vp, _P(WritePlan)]),
    "sdfs_cdc_write_stage": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint32, _vp, ctypes.c_uint64, _vp, _vp, _vp,
                                            ctypes.c_uint32, _vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint32, _vp, _vp]),
    "sdfs_cdc_map_inserts_from_runs": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, _P(DevOut), _vp, _vp,
                                                      _vp, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _P(Inserts),
                                                      ctypes.c_uint64, _vp, _vp]),
}

_lib = None


def load():
    """Load the in-tree HIP library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not built: run `make` or __graft_entry__.build()")
        # PyTorch-ROCm ships its own libamdhip64 with the same soname: load it first when it is
        # installed so this library binds to the runtime torch uses (one HIP runtime per process;
        # the other order leaves torch with "No HIP GPUs are available").
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name, None)
            if fn is None:
                if LIB_PATH == DEFAULT_LIB:
                    raise ImportError(f"{LIB_PATH} does not export {name}: rebuild it")
                continue  # an older build selected for an A/B measurement
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc: int) -> int:
    if rc != OK:
        msg = load().sdfs_cdc_last_error()
        raise SdfsCdcError(rc, msg.decode() if msg else "")
    return rc


def ptr(t):
    """Device address of a tensor for a C-ABI argument; None (NULL) for an absent one."""
    return t.data_ptr() if t is not None else None


def stream_of(t, stream):
    """``stream`` if given, else the current stream of tensor ``t``'s device, as a C-ABI handle."""
    import torch

    return stream if stream is not None else torch.cuda.current_stream(t.device).cuda_stream


def default_params(backup_volume: bool = False) -> Params:
    p = Params()
    check(load().sdfs_cdc_params_default(ctypes.byref(p), 1 if backup_volume else 0))
    return p
