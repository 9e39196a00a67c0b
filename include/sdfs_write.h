/*
 * sdfs_write.h — C-ABI of the ranged write: DedupFileChannel.writeFile for a batch of byte ranges
 * (the write twin of the ranged read in sdfs_read.h).
 *
 * Reference: DedupFileChannel.writeFile (DedupFileChannel.java:274-359) cuts a write at multiples
 * of CHUNK_LENGTH (:310-352) and moves the file's length to max(length, pos + len) (:355-357);
 * WritableCacheBuffer.write (WritableCacheBuffer.java:523-563) then takes, per buffer, one of
 * three routes: a whole-buffer write wraps the caller's bytes (:545-546), the write accelerator
 * chunks only the written run (wm / writeAccelBuffer, :617-781), anything else is read-modify-write
 * (writeBlock -> initBuffer, :505-514) followed by a whole-buffer flush.  Here, for a batch:
 *
 *     sdfs_cdc_write_split            host: requests -> visible pieces, runs, rows, file lengths
 *     sdfs_cdc_write_stage            the visible pieces gathered from the caller's blob into a
 *                                     staging area (any alignment on both sides)
 *     sdfs_cdc_map_inserts_from_runs  the accelerator's insert list from ragged chunked runs
 *
 * Everything else of the route runs through entry points that exist (sdfs_cdc_map_parse,
 * sdfs_cdc_run_device_ragged, sdfs_cdc_index_put_records, sdfs_cdc_map_emit, sdfs_cdc_map_insert,
 * sdfs_cdc_map_emit_pairs, sdfs_cdc_index_claim*, the read path); sdfs_amd/write.py strings them.
 *
 * ONE BATCH IS ONE FLUSH (a stated divergence).  The result of a batch is what the reference
 * leaves when all its writeFile calls arrive, in request order, before any touched buffer is
 * flushed.  wm coalesces only a write that appends to the previous one (its end bookkeeping at
 * :626 sets accelBuffEp = accelBuffPos + b.length where += is meant), and overlapping writes reach
 * insertHashLocPair run after run.  Here overlaps are resolved and touching pieces joined on the
 * host before anything is chunked: the same bytes, fewer and longer runs, better dedup.
 *
 * Errors, threading, sdfs_cdc_last_error() and the stream conventions follow sdfs_cdc.h; arguments
 * are checked before the device is touched.
 */
#ifndef SDFS_WRITE_H
#define SDFS_WRITE_H

#include <stdint.h>

#include "sdfs_cdc.h"
#include "sdfs_extent.h"
#include "sdfs_read.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per piece, or-ed into its request: */
#define SDFS_CDC_WRITE_SLOT 1u   /* the row's slot does not parse, or (accelerator) its pairs are not ascending and disjoint */
#define SDFS_CDC_WRITE_READ 2u   /* materialising the old buffer failed (any SDFS_CDC_READ_* bit) */
#define SDFS_CDC_WRITE_BOUNDS 4u /* sdfs_cdc_write_stage: a device entry reaches past the blob or the staging area */

#define SDFS_CDC_WRITE_SPAN 65536u /* bytes of a piece one workgroup of sdfs_cdc_write_stage copies at most */

/* DedupFileChannel.writeFile(buf = blob[src_off .. src_off + len), len, pos = file_pos) on
 * files[file] (a sdfs_cdc_read_file: the file's slots are rows first_slot .. first_slot + n_slots of
 * the image). */
typedef struct sdfs_cdc_write_request {
    uint64_t file;
    uint64_t file_pos;
    uint64_t len;
    uint64_t src_off;
} sdfs_cdc_write_request;

/* sdfs_cdc_write_split's outputs, all host memory.  piece_* hold piece_cap entries, run_* run_cap,
 * row_* row_cap.  n_pieces / n_runs / n_rows: always the needed counts. */
typedef struct sdfs_cdc_write_plan {
    uint32_t piece_cap, run_cap, row_cap, reserved;
    uint32_t* piece_row;      /* index into row_slot */
    uint32_t* piece_start;    /* first byte in the buffer */
    uint32_t* piece_len;      /* >= 1 */
    uint32_t* piece_req;      /* the request whose bytes are visible here */
    uint64_t* piece_src_off;  /* into the blob */
    uint32_t* run_row;
    uint32_t* run_pos;
    uint32_t* run_len;
    uint32_t* run_first_piece;
    uint32_t* run_n_pieces;
    uint64_t* row_slot;       /* the distinct touched slots, ascending */
    uint8_t* row_full;        /* 1: the row's pieces cover [0, chunk_length) */
    uint64_t n_pieces, n_runs, n_rows;
} sdfs_cdc_write_plan;

/* The request layer, on the host.  n_written[r] = len (a write is never clipped at the end of the
 * file); new_file_len[f] = max(file_len, max over the file's requests with len > 0 of file_pos +
 * len) (DedupFileChannel.java:355-357); a request with len == 0 writes nothing and moves no length.
 * Each request is cut at multiples of chunk_length (:310-352).  Within a row the cuts are resolved
 * in request order, a later request covering an earlier one where they overlap: the row's visible
 * pieces are disjoint and ascending by start, listed row by row (a row of n cuts has at most
 * 2n - 1).  Runs are the maximal sequences of touching visible pieces of a row, in piece order.
 * SDFS_CDC_EINVAL, before anything is written: a request names a file >= n_files; src_off + len
 * passes blob_bytes; a request touches a slot at or past first_slot + n_slots (the caller grows the
 * image first, the rule of sdfs_cdc_import_check_dests); two written files (files with a request of
 * len > 0) share a slot; file_pos + len, src_off + len or first_slot + n_slots overflow 64 bits;
 * chunk_length outside 1 .. 2^31 - 1; more than UINT32_MAX - 1 cuts or pieces.
 * SDFS_CDC_ECAP when piece_cap, run_cap or row_cap is too small: the three counts are written and
 * nothing else.  Bounds: cuts <= sum over requests of (len / chunk_length + 2), pieces <= 2 * cuts,
 * runs <= pieces, rows <= cuts. */
int sdfs_cdc_write_split(const sdfs_cdc_read_file* files, uint32_t n_files, const sdfs_cdc_write_request* requests,
                         uint32_t n_requests, uint32_t chunk_length, uint64_t blob_bytes, int64_t* n_written,
                         uint64_t* new_file_len, sdfs_cdc_write_plan* plan);

/* The hot path: piece p = d_blob[d_src_off[p] .. + d_len[p]) -> d_stage[d_dst_off[p] .. + d_len[p]),
 * source and destination at any alignment, lengths 1 .. max_len (0: nothing), destinations
 * disjoint.  Every destination byte is written exactly once and no byte outside the pieces'
 * extents is written.  An entry whose src_off + len passes blob_bytes, whose dst_off + len passes
 * stage_bytes or whose len passes max_len is skipped: d_piece_status[p] = SDFS_CDC_WRITE_BOUNDS (0
 * for every other piece), and with d_piece_req (optional, with n_requests and d_req_status) the bit
 * is or-ed into d_req_status[d_piece_req[p]] (not zeroed here).
 * Work units are spans of SDFS_CDC_WRITE_SPAN bytes of a piece's destination, found by a floor
 * search over the prefix of the span counts; workgroups stride over them.  Inside a span the
 * destination takes aligned 16-byte stores, the source is read with aligned dword loads and
 * re-aligned in registers; only a piece's first and last vector go byte by byte.
 * d_blob / d_stage must not overlap. */
int sdfs_cdc_write_stage(int device, uint32_t n_pieces, const uint8_t* d_blob, uint64_t blob_bytes,
                         const uint64_t* d_src_off, const uint64_t* d_dst_off, const uint32_t* d_len, uint32_t max_len,
                         uint8_t* d_stage, uint64_t stage_bytes, uint32_t* d_piece_status,
                         const uint32_t* d_piece_req, uint32_t n_requests, uint32_t* d_req_status, void* stream);

/* sdfs_cdc_map_inserts_from_chunks for ragged runs (WritableCacheBuffer.java:729-753): run r
 * (r < n_run) is buffer first_buf + r of `out`, a batch chunked by sdfs_cdc_run_device_ragged, and
 * is run_len[r] bytes long.  One insert per chunk in record order: pos = run_pos + start, len = nlen
 * = the chunk's length, offset = 0, hash = its digest, hashloc = d_hashloc[record], where record
 * counts from the first chunk of buffer 0 of `out` (sdfs_cdc_index_put_records' order), dst_buf the
 * run's.  d_run_first[r] = run r's first insert, d_run_first[n_run] the total; when it passes
 * n_ins_cap nothing is written (the call still returns OK).  h_runs / h_run_len (host) are
 * checked, dst_buf < nbuf_dst and 1 <= run_len, run_pos + run_len <= chunk_length, else EINVAL (the
 * clip at :737-740 then never fires); d_runs / d_run_len are the same arrays on the device, and a
 * device entry that fails the check gives its inserts dst_buf = nbuf_dst (no buffer's). */
int sdfs_cdc_map_inserts_from_runs(int device, uint32_t first_buf, uint32_t n_run, const sdfs_cdc_dev_out* out,
                                   const uint32_t* h_run_len, const uint32_t* d_run_len, const uint64_t* d_hashloc,
                                   uint32_t nbuf_dst, uint32_t chunk_length, const sdfs_cdc_run* h_runs,
                                   const sdfs_cdc_run* d_runs, const sdfs_cdc_inserts* ins, uint64_t n_ins_cap,
                                   uint32_t* d_run_first, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDFS_WRITE_H */
