/*
 * sdfs_read.h — C-ABI of the device-side read path: write buffers rebuilt from their
 * LongByteArrayMap slots (the inverse of sdfs_meta.h plus the last hop).
 *
 * Every read, and every partial rewrite of an existing block, goes through
 * WritableCacheBuffer.initBuffer (WritableCacheBuffer.java:249-410): take the buffer's
 * SparseDataChunk, fetch each HashLocPair's chunk (HashBlobArchive.getChunk,
 * HashBlobArchive.java:1922-1944: decrypt, read nz, LZ4-decode when nz > 0, optionally re-hash) and
 * buf.put(ck, offset, nlen) at pos into a zeroed CHUNK_LENGTH array.  These entry points do that
 * for a whole batch of buffers in HBM:
 *
 *     sdfs_cdc_map_parse        the slots' images -> pairs in TreeMap order
 *     sdfs_cdc_read_plan        which stored records the batch needs, each once, with the argument
 *                               arrays sdfs_cdc_aes_decrypt_device / sdfs_cdc_lz4_decompress_device take
 *     (sdfs_cdc_aes_decrypt_device -> sdfs_cdc_read_chain_lens ->) sdfs_cdc_lz4_decompress_device(framed)
 *     sdfs_cdc_read_assemble    per-buffer status, then the gather of the pieces into the buffers
 *     sdfs_cdc_read_verify      Main.VERIFY_READS: re-hash the chunks, report mismatches
 *
 * Ranged reads — DedupFileChannel.read(buf, bufPos, siz, filePos) (DedupFileChannel.java:499-608)
 * for a batch of byte ranges over several files — use the same parse, decrypt, decode and verify
 * and three entry points of their own:
 *
 *     sdfs_cdc_read_split           host: requests -> n_read, pieces cut at buffer boundaries, and
 *                                   the rows (the distinct touched slots; only these are parsed)
 *     sdfs_cdc_read_plan_pieces     the records the pairs touched by some piece need, each once
 *     sdfs_cdc_read_assemble_pieces per-piece status, then the gather of the ragged pieces
 *
 * One divergence from the reference, on purpose: WritableCacheBuffer.readChunk rebuilds the whole
 * buffer, so a bad record anywhere in it fails every read of that buffer; a ranged read here is
 * decided by the pairs that touch the range alone (see sdfs_cdc_read_plan_pieces).
 *
 * hashloc is the fingerprint's pos of sdfs_cdc_index_put_records (sdfs_index.h): pos_base + the
 * rank of the insertion.  The host owns the chunk store and hands in a directory indexed by
 * hashloc - pos_base.  Errors, threading, the thread-local sdfs_cdc_last_error() message and the
 * stream conventions follow sdfs_cdc.h; arguments are checked before the device is touched.
 * Per-call scratch is allocated and released in stream order.
 */
#ifndef SDFS_READ_H
#define SDFS_READ_H

#include <stdint.h>

#include "sdfs_cdc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-buffer status word: a bitmask, 0 = OK.  A buffer with a non-zero status reads as all
 * zeros; its neighbours are unaffected. */
#define SDFS_CDC_READ_CORRUPT 1u /* the image does not parse (BufferUnderflowException, HashLocPair.checkCorrupt) */
#define SDFS_CDC_READ_MISSING 2u /* a used pair's hashloc is outside the directory */
#define SDFS_CDC_READ_FETCH 4u   /* a used pair's record failed decrypt or decode (getChunk throws) */
#define SDFS_CDC_READ_BOUNDS 8u  /* buf.put out of range (WritableCacheBuffer.java:385-394) */

/* "no fetch" in d_pair_fetch; "failed" in the decryptor's / decoder's length outputs */
#define SDFS_CDC_READ_NONE UINT32_MAX

/* Parsed pairs, a structure of arrays (all device pointers).  Buffer b's pair i lives at slot
 * b*cap + i, i < counts[b], in ascending pos (the TreeMap's order, SparseDataChunk.java:163-168). */
typedef struct sdfs_cdc_pairs {
    uint32_t* counts;  /* [nbuf] entries of the TreeMap (no terminator applied) */
    uint8_t* hashes;   /* [nbuf*cap*32] HashLocPair.hash (hash_len bytes used, zero-padded) */
    uint64_t* hashloc; /* [nbuf*cap] Longs.fromByteArray(HashLocPair.hashloc) */
    int32_t* len;      /* [nbuf*cap] */
    int32_t* pos;      /* [nbuf*cap] */
    int32_t* offset;   /* [nbuf*cap] */
    int32_t* nlen;     /* [nbuf*cap] */
    uint32_t* doop;    /* [nbuf] SparseDataChunk.doop (0 for a corrupt image) */
    uint8_t* flags;    /* [nbuf] SparseDataChunk.flags */
    uint32_t* status;  /* [nbuf] SDFS_CDC_READ_* */
    uint32_t cap;      /* slots per buffer, >= sdfs_cdc_map_pair_cap(slot_bytes, hash_len) */
    uint32_t reserved;
} sdfs_cdc_pairs;

/* Pairs a slot of slot_bytes can hold: (slot_bytes - 13) / (hash_len + 24), 0 below 13
 * (HashLocPair.BAL, HashLocPair.java:37-38; the inverse of sdfs_cdc_map_slot_bytes). */
uint32_t sdfs_cdc_map_pair_cap(uint32_t slot_bytes, uint32_t hash_len);

/* new SparseDataChunk(bytes, version >= 2) for nbuf slots (SparseDataChunk.java:159-174) with
 * HashLocPair(byte[]) per pair (HashLocPair.java:86-97).  Image:
 *     [u8 flags][BE32 length, ignored][BE32 zlen][zlen x BAL bytes][BE32 doop], BAL = hash_len + 24
 *     pair = hash | hashloc[8], big-endian | BE32 len, pos, offset, nlen (signed)
 * zlen <= 0: no pairs.  13 + zlen*BAL > slot_bytes, or any pair with len, pos, offset or nlen < 0:
 * status = SDFS_CDC_READ_CORRUPT, counts = 0.  A never-written (all-zero) slot parses as no pairs,
 * status 0.  status[b] is overwritten (0 or CORRUPT).  hash_len: 32 or 16 as in sdfs_cdc_map_emit.
 * Map versions 0 and 1 are not read.
 * An image whose pos values are strictly ascending — every image SparseDataChunk.getBytes writes —
 * is copied out in one pass.  Any other image goes through the TreeMap rule (ascending pos, of two
 * pairs with the same pos the later one in the image wins) by comparing every pair with every
 * other: 2 * zlen^2 / 64 steps of one wave per buffer — 512 steps at the default slots' 128
 * pairs, 13 million at the backup profile's 20 484 (not measured: no writer produces such an
 * image). */
int sdfs_cdc_map_parse(int device, uint32_t nbuf, const uint8_t* d_map, uint32_t slot_bytes, uint32_t hash_len,
                       const sdfs_cdc_pairs* pairs, void* stream);

/* Which stored records the batch needs (WritableCacheBuffer.java:262-278: a buffer's pairs in
 * ascending pos up to, not including, the first whose hashloc == 0 are used; the rest are ignored
 * silently).  Directory entry k (k < n_store) describes the record of hashloc pos_base + k:
 * d_store_off / d_store_len = where its putChunk record lies in the store (as stored: the
 * ciphertext when the store is encrypted), d_store_raw_len = the chunk's length.  A used pair whose
 * hashloc is outside [pos_base, pos_base + n_store) sets SDFS_CDC_READ_MISSING on its buffer; a
 * buffer whose status is not 0 uses no pair.
 * Outputs (device): d_pair_fetch[nbuf*cap] = the pair's fetch index, SDFS_CDC_READ_NONE for a
 * pair that is not used (every slot of every buffer is written); *d_fetch_count = F, the distinct
 * directory entries needed, listed once each in ascending order: for f < F, d_src_off[f] /
 * d_src_len[f] from the directory, d_dst_cap[f] = raw_len, d_dst_off[f] = the exclusive prefix of
 * raw_len rounded up to 16 (where the decoded chunk goes), d_plain_off[f] (optional, may be NULL) =
 * the exclusive prefix of src_len rounded up to 16 (where a decrypted record goes); the five
 * arrays have n_store entries.  d_total_bytes[0] = bytes of the chunk area, d_total_bytes[1] =
 * bytes of the decrypted-record area.  One pass over the directory: O(n_store). */
int sdfs_cdc_read_plan(int device, uint32_t nbuf, const sdfs_cdc_pairs* pairs, uint64_t pos_base, uint64_t n_store,
                       const uint64_t* d_store_off, const uint32_t* d_store_len, const uint32_t* d_store_raw_len,
                       uint32_t* d_pair_fetch, uint32_t* d_fetch_count, uint64_t* d_src_off, uint32_t* d_src_len,
                       uint64_t* d_dst_off, uint32_t* d_dst_cap, uint64_t* d_plain_off, uint64_t* d_total_bytes,
                       void* stream);

/* d_out_len[i] = d_in_len[i], or 0 where it is UINT32_MAX, for i < *d_count (d_count NULL: n_max).
 * Turns sdfs_cdc_aes_decrypt_device's output lengths into sdfs_cdc_lz4_decompress_device's input
 * lengths: the decoder trusts its src_len, and a record whose padding was bad
 * (BadPaddingException, EncryptUtils.java:125-140) carries 0xFFFFFFFF; with length 0 the framed
 * decoder answers "malformed", so the failure travels on as a failed fetch. */
int sdfs_cdc_read_chain_lens(int device, const uint32_t* d_in_len, const uint32_t* d_count, uint64_t n_max,
                             uint32_t* d_out_len, void* stream);

/* WritableCacheBuffer.java:364-396 for nbuf buffers: buffer b = d_out[b*chunk_length .. +
 * chunk_length), every byte written exactly once.  Fetch f's decoded chunk ck is
 * d_chunks[d_fetch_off[f] .. + d_fetch_len[f]); d_fetch_len is the decoder's d_dst_len, UINT32_MAX
 * = failed.  First each buffer's status is settled: a used pair with a failed fetch sets
 * SDFS_CDC_READ_FETCH (placement is then not looked at: getChunk threw first); else with c = nlen >
 * ck.length ? ck.length : nlen, a pair with pos > chunk_length, pos + c > chunk_length or offset +
 * c > ck.length sets SDFS_CDC_READ_BOUNDS.  Then the gather: a buffer whose status is 0 gets
 * ck[offset .. offset + c) at [pos .. pos + c) for its used pairs in ascending pos — where two
 * overlap a byte holds the value of the last pair in pos order that covers it — and zero
 * elsewhere; any other buffer is all zeros.  nlen == 0 copies nothing.  chunk_length >= 1, any
 * value (no alignment asked of it, of d_out or of the chunks).
 * The gather stages a buffer's pos / end arrays in LDS when pairs->cap is at most 1024 (the
 * default parameter set's slots hold 128); above that (the backup profile's slots hold 20 484)
 * the lanes search the same arrays in global memory. */
int sdfs_cdc_read_assemble(int device, uint32_t nbuf, uint32_t chunk_length, const sdfs_cdc_pairs* pairs,
                           const uint32_t* d_pair_fetch, const uint8_t* d_chunks, const uint64_t* d_fetch_off,
                           const uint32_t* d_fetch_len, uint8_t* d_out, void* stream);

/* Main.VERIFY_READS (HashBlobArchive.java:1934-1941): fingerprints the *d_fetch_count (at most
 * n_fetch_max) fetched chunks with sdfs_cdc_hash_device and sets d_pair_bad[b*cap + i] = 1 for every
 * used pair whose hash differs from its chunk's digest (0 for every other slot, a pair whose fetch
 * failed included); d_bad_count[b] = the buffer's marked pairs.  The engine's digest length must
 * equal the hash_len the pairs were parsed with.  status is not touched: the reference only logs
 * the mismatch and the read succeeds. */
int sdfs_cdc_read_verify(sdfs_cdc_engine* engine, uint32_t nbuf, const sdfs_cdc_pairs* pairs, uint32_t hash_len,
                         const uint32_t* d_pair_fetch, const uint8_t* d_chunks, const uint64_t* d_fetch_off,
                         const uint32_t* d_fetch_len, const uint32_t* d_fetch_count, uint64_t n_fetch_max,
                         uint8_t* d_pair_bad, uint32_t* d_bad_count, void* stream);

/* ---- ranged reads -------------------------------------------------------------------------- */

/* A file of one map image: its slots are rows first_slot .. first_slot + n_slots of the image; it
 * is file_len bytes long (a sparse file may be longer than n_slots * chunk_length). */
typedef struct sdfs_cdc_read_file {
    uint64_t first_slot;
    uint64_t n_slots;
    uint64_t file_len;
} sdfs_cdc_read_file;

/* DedupFileChannel.read(buf, bufPos = out_off, siz, filePos = file_pos) on files[file]. */
typedef struct sdfs_cdc_read_request {
    uint64_t file;
    uint64_t file_pos;
    uint64_t siz;
    uint64_t out_off;
} sdfs_cdc_read_request;

/* The request layer (DedupFileChannel.java:499-608, WritableCacheBuffer.readChunk :217-245), on the
 * host, all arrays host memory.  Request r: file_pos >= file_len -> n_read[r] = -1, no pieces;
 * else n_read[r] = min(siz, file_len - file_pos) (siz == 0 -> 0) and [file_pos, file_pos + n_read)
 * is cut at multiples of chunk_length into pieces, in request order then ascending position:
 * piece_req = r, piece_start = pos % chunk_length, piece_len, piece_out_off following each other
 * from the request's out_off, and piece_row = the index in row_slot of the slot first_slot + pos /
 * chunk_length — SDFS_CDC_READ_NONE when pos / chunk_length >= n_slots (the map is shorter than
 * the file: the reference hands out a blank buffer, the piece reads as zeros with status 0).
 * row_slot[0 .. *n_rows) = the distinct touched slots, ascending.
 * *n_pieces / *n_rows are always the needed counts; SDFS_CDC_ECAP when piece_cap or row_cap is
 * smaller (nothing else is written then).  Bounds: pieces <= sum over requests of (siz /
 * chunk_length + 2), rows <= pieces.  64-bit position arithmetic, checked: a file index >=
 * n_files, first_slot + n_slots, out_off + n_read or siz > INT64_MAX overflowing, or more than
 * UINT32_MAX - 1 pieces are SDFS_CDC_EINVAL. */
int sdfs_cdc_read_split(const sdfs_cdc_read_file* files, uint32_t n_files, const sdfs_cdc_read_request* requests,
                        uint32_t n_requests, uint32_t chunk_length, int64_t* n_read, uint32_t piece_cap,
                        uint32_t* piece_req, uint32_t* piece_row, uint32_t* piece_start, uint32_t* piece_len,
                        uint64_t* piece_out_off, uint32_t row_cap, uint64_t* row_slot, uint64_t* n_pieces,
                        uint64_t* n_rows);

/* sdfs_cdc_read_plan for pieces: pairs holds the nbuf parsed rows; piece p reads [d_piece_start[p],
 * + d_piece_len[p]) of row d_piece_row[p] (SDFS_CDC_READ_NONE or >= nbuf: no row, zeros; start +
 * len <= chunk_length is the caller's to keep).  With U = the row's pairs in ascending pos up to,
 * not including, the first hashloc == 0, a pair of U touches the piece iff nlen > 0, pos < start +
 * len and pos + nlen > start (c = min(nlen, ck.length) <= nlen: a pair that does not touch cannot
 * supply a byte of the piece).  d_piece_status[p] = SDFS_CDC_READ_CORRUPT when the row did not
 * parse, else SDFS_CDC_READ_MISSING when a touching pair's hashloc is outside the directory, else
 * 0.  A pair is needed iff it touches a piece whose status here is 0; the fetch list is the
 * distinct directory entries of the needed pairs, laid out exactly as sdfs_cdc_read_plan lays out
 * its own.  d_pair_fetch is written for every slot of every row and is SDFS_CDC_READ_NONE for a
 * pair nobody needs — the used pairs are no prefix of the row here.  pairs->status is not written.
 * Divergence from the reference (which rebuilds the whole buffer): a missing, failed or misplaced
 * pair fails only the pieces it touches; whenever the whole-buffer read of a row has status 0 the
 * ranged bytes equal the slice of that buffer. */
int sdfs_cdc_read_plan_pieces(int device, uint32_t nbuf, const sdfs_cdc_pairs* pairs, uint64_t pos_base,
                              uint64_t n_store, const uint64_t* d_store_off, const uint32_t* d_store_len,
                              const uint32_t* d_store_raw_len, uint32_t n_pieces, const uint32_t* d_piece_row,
                              const uint32_t* d_piece_start, const uint32_t* d_piece_len, uint32_t* d_piece_status,
                              uint32_t* d_pair_fetch, uint32_t* d_fetch_count, uint64_t* d_src_off, uint32_t* d_src_len,
                              uint64_t* d_dst_off, uint32_t* d_dst_cap, uint64_t* d_plain_off, uint64_t* d_total_bytes,
                              void* stream);

/* WritableCacheBuffer.readChunk (:217-245: initBuffer, then arraycopy of [startPos, startPos + len))
 * for n_pieces pieces: piece p = d_out[d_piece_out_off[p] .. + d_piece_len[p]), every byte written
 * exactly once, no byte outside the pieces' extents written, any alignment; overlapping extents are
 * the caller's error.  d_piece_status is in/out: a piece whose status is still 0 gets
 * SDFS_CDC_READ_FETCH when a touching pair's fetch failed, else SDFS_CDC_READ_BOUNDS when a
 * touching pair breaks one of sdfs_cdc_read_assemble's three placement conditions.  A piece with
 * status 0 gets, per byte, the value of the last needed pair in pos order that covers it, else
 * zero; any other piece, and a piece without a row, is all zeros.
 * d_req_status (optional, with d_piece_req: piece p belongs to request d_piece_req[p] < n_requests):
 * d_req_status[r] = the OR of the final statuses of request r's pieces, 0 for a request without
 * pieces; all n_requests entries are written.
 * The gather's work units are 64 KiB tiles of the pieces.  A tile stages in LDS only the piece's
 * window of pairs — from the first pair whose running max of end exceeds start to the last with
 * pos < start + len — so the LDS form applies whenever the window holds at most 1024 pairs,
 * whatever pairs->cap is; a larger window is searched in global memory. */
int sdfs_cdc_read_assemble_pieces(int device, uint32_t nbuf, uint32_t chunk_length, const sdfs_cdc_pairs* pairs,
                                  const uint32_t* d_pair_fetch, const uint8_t* d_chunks, const uint64_t* d_fetch_off,
                                  const uint32_t* d_fetch_len, uint32_t n_pieces, const uint32_t* d_piece_row,
                                  const uint32_t* d_piece_start, const uint32_t* d_piece_len,
                                  const uint64_t* d_piece_out_off, uint32_t* d_piece_status,
                                  const uint32_t* d_piece_req, uint32_t n_requests, uint32_t* d_req_status,
                                  uint8_t* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDFS_READ_H */
