/*
 * sdfs_import.h — C-ABI of the map-file import: slot images whose hashlocs belong to ANOTHER
 * volume become slots of this one.
 *
 * The reference does it in two places.  GetCloudFile.checkDedupFile (GetCloudFile.java:184-249,
 * "Importing hashes for file") walks every SparseDataChunk of a downloaded map, puts every pair's
 * fingerprint with one reference and, where the local index answers another position, rewrites
 * the pair's hashloc (p.hashloc = ir.getHashLocs(); dirty = true) and puts the slot back;
 * LongByteArrayMap.index() / nextValue(true) (LongByteArrayMap.java:310-356, 884-890) do the same
 * rewrite through addRef.  Inside one volume there is nothing to rewrite (sdfs_index.h); between
 * two volumes the rewrite is the whole point: here a hashloc is a volume's own insertion rank, so a
 * foreign image means nothing until every pair is re-homed, and a chunk the destination lacks is
 * fetched from the source's store, because the volumes do not share a bucket.
 *
 * A batch is nreq requests: request r = {a source slot image of slot_bytes (version >= 2 layout, as
 * sdfs_cdc_map_parse reads it), a destination slot number, len (sp.len)}.  Pairs are addressed by
 * their place in the image: pair i of request r is place r * pair_stride + i, as d_inserted is in
 * sdfs_cdc_index_addref_slots.  One batch is these calls on one stream:
 *
 *   import_pairs -> sdfs_cdc_index_get -> import_plan -> (the read path's fetch: decrypt ->
 *   chain_lens -> framed decode, by the caller) -> import_records -> sdfs_cdc_index_put_records and
 *   the store tail (by the caller; d_buf_offs = the plan's d_dst_off) -> sdfs_cdc_index_claim_slots
 *   (-1) over the accepted destinations -> import_install
 *
 * The rule:
 *   1. An image is read by exactly the rule of the map-file walks (sdfs_index.h): zlen <= 0 or an
 *      all-zero image = no pairs, status 0; an image that does not fit its slot or any negative
 *      len / pos / offset / nlen = SDFS_CDC_READ_CORRUPT; a pair that shares its pos with a later
 *      pair of the image does not count; every other pair counts (no hashloc 0 / 1 or blank-hash
 *      skip).
 *   2. A counting pair whose fingerprint the destination index holds is HELD (a count <= 0 that no
 *      sweep has removed still counts as held).  Any other counting pair is WANTED: k = hashloc -
 *      src_pos_base must name a source directory entry, k < n_src, store_len[k] != 0 and 0 <
 *      store_raw_len[k] <= max_chunk; a wanted pair that names none sets
 *      SDFS_CDC_IMPORT_EMISSING on its request and is counted in req_missed[r].
 *   3. The directory entries wanted by the requests that are still clean are fetched, each once, in
 *      ascending k, in the shape sdfs_cdc_read_plan emits.  The fetched chunk is the whole stored
 *      chunk: a pair's offset / nlen are not looked at.  A fetch whose decoded length is not
 *      store_raw_len[k] sets SDFS_CDC_IMPORT_EFETCH on every clean request with a pair that uses
 *      it; with an engine, every wanted pair whose fetch succeeded and whose hash is not the
 *      fetch's digest sets SDFS_CDC_IMPORT_EHASH.
 *   4. A request with any status bit moves no count, inserts nothing and its destination slot keeps
 *      every byte; it does not stand in the way of the others.  Every status word is final when
 *      the kernel that writes it has finished, before any record is emitted.
 *   5. Every counting pair of every accepted request, in (request, image place) order, becomes one
 *      48-byte fingerprint record: a wanted pair's is {hash, buffer_id = its fetch index f, start =
 *      0, len = the fetched length}, a held pair's {hash, 0, 0, 0}.  put_records and the store tail
 *      run on them unchanged: each pair adds one reference, the first record of a fingerprint the
 *      destination lacked inserts it at pos_base + rank, its chunk is stored once.
 *   6. Every accepted request's image goes to its destination slot — image bytes first, the rest
 *      of the slot zero — with the 8 hashloc bytes of every counting pair replaced by BE64 of its
 *      record's d_hashloc; everything else is copied byte for byte.  The file length moves to
 *      max(old, dest * chunk_length + len).
 *
 * Four deliberate divergences from the reference:
 *   - put(cm, false) records the source's archive id without data, because the reference's volumes
 *     share a bucket.  Here the chunk is fetched and stored.
 *   - The reference imports blindly.  Here a request goes in whole or not at all.
 *   - Every pair counts (sdfs_index.h gives the reason).
 *   - The replaced slot's pairs are released, which keeps count = pairs in persisted slots exact.
 * Not read: map versions < 2; the reference refuses them too (GetCloudFile.java:194-195).
 *
 * Offsets and lengths read from an image or from the source directory are compared with their
 * bounds before anything is loaded through them.  Errors, threading and the last-error message
 * follow include/sdfs_cdc.h; arguments are checked before the device is touched; per-call scratch
 * is stream-ordered; no call reads anything back to the host.
 */
#ifndef SDFS_IMPORT_H
#define SDFS_IMPORT_H

#include <stdint.h>

#include "sdfs_cdc.h"
#include "sdfs_read.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a request's status word: 0 = accepted; SDFS_CDC_READ_CORRUPT (1) = the image does not parse */
#define SDFS_CDC_IMPORT_EMISSING 32u /* a wanted pair names no source directory entry */
#define SDFS_CDC_IMPORT_EFETCH 64u   /* a fetch one of its pairs uses failed or has the wrong length */
#define SDFS_CDC_IMPORT_EHASH 128u   /* verify: a wanted pair's hash is not its fetched chunk's fingerprint */

#define SDFS_CDC_IMPORT_NONE 0xFFFFFFFFu /* pair_fetch / pair_rec: the pair has none */
#define SDFS_CDC_IMPORT_BLOCK 1024u      /* entries one workgroup of the multi-block scans ranks */
#define SDFS_CDC_IMPORT_SPAN 16384u      /* bytes of one slot a workgroup of the install writes */

/* What the calls of one batch share (device).  P = nreq * pair_stride pair places. */
typedef struct sdfs_cdc_import_work {
    uint8_t* hashes;       /* [P x 32] the pair's hash, zero-padded; zero where there is no pair: the d_digests
                              of sdfs_cdc_index_get */
    uint64_t* src_hashloc; /* [P] the pair's hashloc in the source volume */
    uint8_t* counting;     /* [P] 1 = the pair counts */
    uint32_t* status;      /* [nreq] the request's status word */
    uint32_t* req_pairs;   /* [nreq] pairs of the image (0 for an empty or corrupt one) */
    uint32_t* req_missed;  /* [nreq] wanted pairs that name no source directory entry */
    uint32_t* pair_fetch;  /* [P] the wanted pair's fetch index, SDFS_CDC_IMPORT_NONE for every other place */
    uint32_t* pair_rec;    /* [P] the pair's fingerprint record, SDFS_CDC_IMPORT_NONE without one */
    uint64_t* counts;      /* [8] records emitted, pairs held (among them), distinct fetches, raw bytes fetched,
                              requests accepted, requests rejected, pairs whose hashloc changed (the reference's
                              `dirty`), pairs missed */
} sdfs_cdc_import_work;

/* Validate the nreq images of d_req (nreq x slot_bytes) and lay their pairs out by image place:
 * writes w->hashes, src_hashloc, counting, status (0 or SDFS_CDC_READ_CORRUPT) and req_pairs, and
 * zeroes req_missed and counts.  hash_len: 32 or 16; pair_stride >= the pairs a slot holds.  A
 * wave validates a request; a slot of more than 256 pairs is then spread over several waves.
 * (SparseDataChunk(byte[]) per slot, GetCloudFile.java:196-203) */
int sdfs_cdc_import_pairs(int device, const uint8_t* d_req, uint64_t nreq, uint32_t slot_bytes, uint32_t hash_len,
                          uint32_t pair_stride, const sdfs_cdc_import_work* w, void* stream);

/* d_pos: sdfs_cdc_index_get's answer for w->hashes (UINT64_MAX = absent; held otherwise).  Settles
 * EMISSING and req_missed, marks the directory entries the clean requests want and lays their
 * fetches out exactly as sdfs_cdc_read_plan does: fetch f of *d_fetch_count = the f-th wanted
 * entry in ascending k, d_src_off / d_src_len = its stored record, d_dst_off = the prefix of
 * store_raw_len rounded up to 16, d_dst_cap = store_raw_len, d_plain_off (may be NULL) = the prefix
 * of store_len rounded up to 16, d_total_bytes[2] = the two areas' sizes; w->pair_fetch = the
 * wanted pairs' fetches; w->counts[2], [3] and [7].  The fetch arrays hold n_src entries.  The
 * raw bytes count every planned fetch, whatever becomes of it.  The ranking is count / scan /
 * assign over the directory on all CUs (SDFS_CDC_IMPORT_BLOCK entries per workgroup).
 * (HashesMap.put's lookup + the chunk the reference does not have to move) */
int sdfs_cdc_import_plan(int device, uint64_t nreq, uint32_t pair_stride, const sdfs_cdc_import_work* w,
                         const uint64_t* d_pos, uint64_t src_pos_base, uint64_t n_src, const uint64_t* d_store_off,
                         const uint32_t* d_store_len, const uint32_t* d_store_raw_len, uint32_t max_chunk,
                         uint32_t* d_fetch_count, uint64_t* d_src_off, uint32_t* d_src_len, uint64_t* d_dst_off,
                         uint32_t* d_dst_cap, uint64_t* d_plain_off, uint64_t* d_total_bytes, void* stream);

/* After the fetch (d_chunks: the chunk area, fetch f at d_dst_off[f], d_fetch_len[f] bytes decoded,
 * UINT32_MAX = failed): the decision (EFETCH; with engine != NULL the fetched chunks are
 * fingerprinted once each by sdfs_cdc_hash_device and compared, EHASH), then the counting pairs of
 * the accepted requests compacted in (request, place) order into d_records (room for P), *d_count
 * (u32) = their number, w->pair_rec, w->counts[0..1].  The decision is a kernel of its own that has
 * finished before the count / scan / assign trio emits a record.  The fetch arrays hold
 * n_fetch_max >= *d_fetch_count entries (the count the fetch read back, or the plan's n_src);
 * engine's digest length must be hash_len.  (new ChunkData(hash, ...) + put per pair, GetCloudFile.java:204-222) */
int sdfs_cdc_import_records(int device, sdfs_cdc_engine* engine, uint64_t nreq, uint32_t pair_stride,
                            uint32_t hash_len, const sdfs_cdc_import_work* w, const uint32_t* d_fetch_count,
                            uint64_t n_fetch_max, const uint8_t* d_chunks, const uint64_t* d_dst_off,
                            const uint32_t* d_dst_cap, const uint32_t* d_fetch_len, uint8_t* d_records,
                            uint32_t* d_count, void* stream);

/* After put_records -> d_hashloc (per record) and the release of the replaced slots: every accepted
 * request's image to slot d_dests[r] of d_map (nslots x slot_bytes), re-homed, in one kernel;
 * *d_file_len (u64, in/out) = max(old, d_dests[r] * chunk_length + d_lens[r]); w->counts[4..6].
 * d_dests (u64[nreq]) have passed sdfs_cdc_import_check_dests; a destination outside the map is
 * skipped here all the same.  (p.hashloc = ir.getHashLocs(); mp.put(pos, ck), GetCloudFile.java:213-228) */
int sdfs_cdc_import_install(int device, const uint8_t* d_req, uint64_t nreq, uint32_t slot_bytes, uint32_t hash_len,
                            uint32_t pair_stride, const sdfs_cdc_import_work* w, const uint64_t* d_hashloc,
                            const uint64_t* d_dests, const uint32_t* d_lens, uint32_t chunk_length, uint8_t* d_map,
                            uint64_t nslots, uint64_t* d_file_len, void* stream);

/* Host only, before the first call of a batch: the destinations (a HOST array) are distinct and
 * inside the map, or SDFS_CDC_EINVAL.  Two requests on one slot would make the slot's bytes and
 * the released counts depend on the schedule. */
int sdfs_cdc_import_check_dests(const uint64_t* dests, uint64_t nreq, uint64_t nslots);

#ifdef __cplusplus
}
#endif
#endif /* SDFS_IMPORT_H */
