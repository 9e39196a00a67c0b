/*
 * sdfs_extent.h — C-ABI of the device-side map edits: HashLocPairs merged into LongByteArrayMap
 * slots that already exist, without touching a byte of chunk data.
 *
 * Two features of the reference end in the same operation on a buffer's SparseDataChunk:
 *   - copyExtents (mgmt/CopyExtents.java:80-180): per source buffer SparseDataChunk.getWL
 *     (SparseDataChunk.java:181-206) cuts the covering pair, WritableCacheBuffer.copyExtent
 *     (WritableCacheBuffer.java:565-611) inserts it into the destination's list;
 *   - the write accelerator (WritableCacheBuffer.java:617-781): only the written run is chunked
 *     and one pair per finger is inserted into the existing list.
 * Both call SparseDataChunk.insertHashLocPair (SparseDataChunk.java:208-263) and persist
 * SparseDataChunk.getBytes (:295-318).  Here, for a whole batch of buffers in HBM:
 *
 *     sdfs_cdc_map_extents              getWL in bulk: segments of source buffers -> an insert list
 *     sdfs_cdc_map_inserts_from_chunks  the accelerator's insert list from a chunked run batch
 *     sdfs_cdc_map_insert               insertHashLocPair for every buffer's inserts, in order
 *     sdfs_cdc_map_emit_pairs           getBytes for arbitrary pair lists
 *
 * insertHashLocPair(ar, p), ep = p.pos + p.nlen, for a list whose pairs are ascending and disjoint,
 * an existing pair h with hep = h.pos + h.nlen:
 *     hep <= p.pos, or h.pos >= ep with h.nlen > 0      untouched (touching is not overlapping)
 *     p.pos <= h.pos and hep <= ep                      removed (a pair with nlen == 0 and
 *                                                       p.pos <= h.pos <= ep included)
 *     p.pos <= h.pos < ep < hep                         head trimmed: pos = ep, offset and nlen follow
 *     h.pos < p.pos < hep <= ep                         tail trimmed: nlen = p.pos - h.pos
 *     h.pos < p.pos and ep < hep                        split: h keeps [h.pos, p.pos), a clone takes
 *                                                       [ep, hep) with its offset moved and dup = true
 * then p is put at p.pos.  hash, hashloc and len of a fragment are its source pair's.
 *
 * ONE DELIBERATE DIVERGENCE.  In the split case the reference stores the old object under the
 * clone's key (`ar.put(_h.pos, h)`, SparseDataChunk.java:248) instead of the clone it has just
 * built.  On persist the list is keyed by each pair's own pos again, the alias collapses, and the
 * tail [ep, hep) is lost: those bytes read back as zeros (and the alias can be found again by
 * floorEntry(ep - 1), so that the loop does not end).  This library puts the clone: after an insert
 * every byte outside [p.pos, ep) reads as before.  tests/extent_model.py carries both forms and
 * tests/test_extent.py pins where they differ.
 *
 * Errors, threading, sdfs_cdc_last_error() and the stream conventions follow sdfs_cdc.h; arguments
 * are checked before the device is touched; per-call scratch is allocated and released in stream
 * order.  Arrays of 32-bit and wider elements are naturally aligned, hash arrays 4-byte aligned.
 */
#ifndef SDFS_EXTENT_H
#define SDFS_EXTENT_H

#include <stdint.h>

#include "sdfs_cdc.h"
#include "sdfs_read.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Status bits, 0 = done.  Per destination buffer: */
#define SDFS_CDC_EXT_CORRUPT 1u    /* the parse's status was not 0, or a pair's pos + nlen / offset + nlen passes 2^31 - 1 */
#define SDFS_CDC_EXT_OVERLAP 2u    /* the pairs are not ascending and disjoint (the reference's result there is an accident of tree order) */
#define SDFS_CDC_EXT_BAD_INSERT 4u /* an insert of this buffer has nlen <= 0, a negative field, pos + nlen > chunk_length or offset + nlen > 2^31 - 1 */
#define SDFS_CDC_EXT_OVERFLOW 8u   /* the result is valid and written, but holds more pairs than the slot takes */
#define SDFS_CDC_EXT_ECAP 16u      /* the result does not fit out->cap: nothing written, counts = the needed number */
/* per segment: */
#define SDFS_CDC_EXT_HOLE 32u      /* a byte of the source range is not covered (getWL: "Position not found") */
#define SDFS_CDC_EXT_SRC 64u       /* the source buffer's status is not 0, or it is not ascending and disjoint */

/* A byte range inside one source buffer copied to a range inside one destination buffer (the host
 * cuts a file range at the buffer boundaries of both files, CopyExtents.java:96-155). */
typedef struct sdfs_cdc_segment {
    uint32_t src_buf, src_off, dst_buf, dst_off, len;
} sdfs_cdc_segment;

/* Where a chunked run lands: buffer and position of its first byte. */
typedef struct sdfs_cdc_run {
    uint32_t dst_buf, run_pos;
} sdfs_cdc_run;

/* An insert list, a structure of arrays (all device pointers). */
typedef struct sdfs_cdc_inserts {
    uint8_t* hash;     /* [n*32] hash_len bytes used, zero-padded */
    uint64_t* hashloc; /* [n] */
    int32_t* len;      /* [n] */
    int32_t* pos;      /* [n] position in the destination buffer */
    int32_t* offset;   /* [n] */
    int32_t* nlen;     /* [n] */
    uint32_t* dst_buf; /* [n] */
} sdfs_cdc_inserts;

/* getWL in bulk.  src: the parsed source slots (sdfs_cdc_map_parse).  The n_seg segments are
 * handed in twice: h_segs in host memory for the argument check (len >= 1, src_buf < nbuf_src,
 * dst_buf < nbuf_dst, src_off + len and dst_off + len <= chunk_length, else EINVAL before any
 * launch) and d_segs, the same array on the device, for the kernels (a device entry that fails the
 * same check gets SDFS_CDC_EXT_SRC).
 * Per segment, one piece per source pair that covers a byte of [src_off, src_off + len), clipped to
 * it: pos = dst_off + (piece start - src_off), offset = the pair's offset + (piece start - its
 * pos), nlen = the piece's length, hash / hashloc / len the pair's, dst_buf the segment's.  Pieces
 * are listed in segment order and ascending source position inside a segment:
 * d_seg_first[s] .. d_seg_first[s + 1] are segment s's, d_seg_first[n_seg] the total.  d_seg_status[s]:
 * 0, SDFS_CDC_EXT_SRC or SDFS_CDC_EXT_HOLE; a segment with a status has no piece.
 * Count pass, prefix, emit pass.  When the total passes n_ins_cap no piece is written at all
 * (the call still returns OK: d_seg_first[n_seg] says how many are needed).
 * One wave per segment; it checks its whole source buffer (counts / 64 steps), then finds its
 * pairs by binary search. */
int sdfs_cdc_map_extents(int device, uint32_t nbuf_src, const sdfs_cdc_pairs* src, uint32_t nbuf_dst,
                         uint32_t chunk_length, uint32_t n_seg, const sdfs_cdc_segment* h_segs,
                         const sdfs_cdc_segment* d_segs, const sdfs_cdc_inserts* ins, uint64_t n_ins_cap,
                         uint32_t* d_seg_first, uint32_t* d_seg_status, void* stream);

/* The write accelerator's inserts (WritableCacheBuffer.java:729-753): one per chunk of n_run runs
 * of run_len bytes chunked by sdfs_cdc_run_device (out), in record order (run by run, chunk by
 * chunk): pos = run_pos + start, len = nlen = the chunk's length, offset = 0, hash = its digest,
 * hashloc = d_hashloc[record] (sdfs_cdc_index_put_records).  d_run_first[r] = run r's first insert,
 * d_run_first[n_run] the total; beyond n_ins_cap nothing is written, as above.  h_runs (host) /
 * d_runs (device) as for the segments: dst_buf < nbuf_dst and run_pos + run_len <= chunk_length,
 * else EINVAL (wm only sees writes inside the buffer, so the clip at :737-740 never fires). */
int sdfs_cdc_map_inserts_from_chunks(int device, uint32_t n_run, const sdfs_cdc_dev_out* out, uint32_t run_len,
                                     const uint64_t* d_hashloc, uint32_t nbuf_dst, uint32_t chunk_length,
                                     const sdfs_cdc_run* h_runs, const sdfs_cdc_run* d_runs,
                                     const sdfs_cdc_inserts* ins, uint64_t n_ins_cap, uint32_t* d_run_first,
                                     void* stream);

/* insertHashLocPair for nbuf buffers.  in: the parsed destination slots.  The n_ins inserts are
 * grouped by destination buffer: buffer b's are d_ins_first[b] .. d_ins_first[b + 1] (ascending,
 * at most n_ins), applied in list order (ins->dst_buf is not read).  out: a second sdfs_cdc_pairs (no array shared with in);
 * out->cap >= counts + 2 * (inserts of the buffer) is always enough, an insert adds itself and at
 * most one split tail.  d_out_dup[nbuf * out->cap]: 1 on split tails (and what is cut from them
 * later), 0 on every other pair.  d_status[nbuf] and out->status: SDFS_CDC_EXT_* bits.
 * slot_pairs: what the slot can take (sdfs_cdc_map_pair_cap), for SDFS_CDC_EXT_OVERFLOW.
 * A buffer with any bit but OVERFLOW keeps its pairs unchanged in out; a buffer without inserts is
 * copied through; with ECAP nothing of the buffer is written and out->counts holds the needed
 * number.  out->doop = the sum of nlen over the pairs with dup set, out->flags = in->flags.
 * Elements of out past counts are not written; every other one exactly once.
 * The inserts of a buffer are replayed one after the other on a work list of {source, pos, offset,
 * nlen}; each step finds the affected range by binary search and moves the list, all lanes at once:
 * (inserts) x (pairs / lanes) steps.  A buffer whose counts + 2 * inserts is at most 256 is one
 * wave's work with both lists in LDS; any other (the backup profile's slots hold 20 484 pairs) gets
 * a workgroup of 256 with the lists in global memory — 20 484 pairs and 300 inserts are 24 000
 * steps of 256 lanes.  Scratch: 32 bytes x (nbuf * in->cap + 2 * n_ins). */
int sdfs_cdc_map_insert(int device, uint32_t nbuf, uint32_t chunk_length, uint32_t slot_pairs,
                        const sdfs_cdc_pairs* in, const sdfs_cdc_inserts* ins, uint64_t n_ins,
                        const uint32_t* d_ins_first, const sdfs_cdc_pairs* out, uint8_t* d_out_dup,
                        uint32_t* d_status, void* stream);

/* SparseDataChunk.getBytes (version >= 2) for nbuf pair lists into their slots:
 *     [u8 flags][BE32 13 + n * BAL][BE32 n][n pairs in list order][BE32 doop], BAL = hash_len + 24
 * doop = the sum of nlen over the pairs with d_dup[b * cap + i] != 0 (d_dup NULL: 0); d_doop
 * (optional) receives it.  flags: the reference writes 0 (updateMap builds a fresh SparseDataChunk).
 * A buffer whose d_status[b] (optional) is not 0, or with more pairs than
 * sdfs_cdc_map_pair_cap(slot_bytes, hash_len) or than pairs->cap, is not written — the old image
 * stays — and is counted in *d_skipped (added to what is there).  Bytes of the slot past the image
 * are left alone, as in sdfs_cdc_map_emit.  hash_len: 32 or 16. */
int sdfs_cdc_map_emit_pairs(int device, uint32_t nbuf, const sdfs_cdc_pairs* pairs, uint32_t hash_len,
                            const uint8_t* d_dup, const uint32_t* d_status, uint8_t flags, uint8_t* d_map,
                            uint32_t slot_bytes, uint32_t* d_doop, uint32_t* d_skipped, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDFS_EXTENT_H */
