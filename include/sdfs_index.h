/*
 * sdfs_index.h — C-ABI of the device-resident dedup-hit index.
 *
 * After getChunks, SDFS dedups a flushed buffer's chunks by fingerprint and hands each distinct
 * one to the hash store: SparseDedupFile.writeCache groups the buffer's Fingers by hash and counts
 * `claims` (SparseDedupFile.java:435-446), calls HCServiceProxy.writeChunk(hash, chunk, claims)
 * for every distinct hash (Finger.java:50-60 -> HashChunkService.writeChunk,
 * HashChunkService.java:98-118 -> AbstractHashesMap.put), and records per chunk whether it was a
 * duplicate and where the data lives (HashLocPair dup/hashloc, SparseDedupFile.java:541-560).
 * The hash store's put (RocksDBMap.put, RocksDBMap.java:785-870) is: present -> refcount +=
 * claims, return InsertRecord(inserted=false, pos); absent -> persist the chunk, insert
 * {pos, refcount = claims}, return InsertRecord(inserted=true, pos).
 *
 * This index keeps that map (fingerprint -> {pos, refcount}) in HBM and applies a whole batch of
 * fingerprint records (the engine's 48-byte records, include/sdfs_cdc.h, in buffer order) in
 * one pass.  Results equal applying the buffers one after another in record order: the first
 * record of a fingerprint that was not yet in the index is the one "inserted"; every other
 * record is a duplicate; every record's hashloc is its fingerprint's pos.  Positions of newly
 * inserted fingerprints are pos_base + their rank among the batch's insertions (in record order):
 * the host persists exactly those chunks (new_list) and owns the pos namespace, as
 * HashBlobArchive does for the reference.
 *
 * Errors, threading and the last-error message follow include/sdfs_cdc.h (sdfs_cdc_last_error).
 * Calls apply in call order whatever streams they are enqueued on (a call on another stream than
 * the previous one waits for it on the device).
 * A full index returns SDFS_CDC_ECAP (HashtableFullException in the reference).
 */
#ifndef SDFS_INDEX_H
#define SDFS_INDEX_H

#include <stdint.h>

#include "sdfs_cdc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sdfs_cdc_index sdfs_cdc_index;

/* A device-resident map with room for `capacity` fingerprints (rounded up to a power of two,
 * filled to at most 7/8) on HIP device `device`.  64 bytes of HBM per slot.
 * (AbstractHashesMap.init, AbstractHashesMap.java: init(maxSize, fileName, fpp)) */
int sdfs_cdc_index_create(int device, uint64_t capacity, sdfs_cdc_index** out);
int sdfs_cdc_index_destroy(sdfs_cdc_index* ix);

/* Apply a batch of fingerprint records (d_records: n_max x SDFS_CDC_RECORD_BYTES on the device,
 * of which the first *d_count are valid when d_count != NULL, else all n_max).  Outputs (device,
 * n_max entries, written for the valid records): d_dup[r] = 1 if record r is a duplicate (its
 * fingerprint was indexed before or appeared earlier in the batch), d_hashloc[r] = pos of its
 * fingerprint; d_new_list[0..k) = indices of the inserted records in record order, *d_new_count
 * = k (u64).  Enqueued on `stream` (NULL = the HIP null stream).
 * (AbstractHashesMap.put(ChunkData) per distinct fingerprint, RocksDBMap.java:785-870, as driven
 * by SparseDedupFile.writeCache, SparseDedupFile.java:435-446,487-564) */
int sdfs_cdc_index_put_records(sdfs_cdc_index* ix, const uint8_t* d_records, uint64_t n_max,
                               const uint32_t* d_count, uint64_t pos_base, uint8_t* d_dup,
                               uint64_t* d_hashloc, uint32_t* d_new_list, uint64_t* d_new_count,
                               void* stream);

/* Look up n fingerprints (d_digests: n x 32 bytes, zero-padded past the digest length):
 * d_pos[i] = pos or UINT64_MAX when absent, d_refcount[i] = reference count or 0 (either output
 * may be NULL).  (AbstractHashesMap.get / containsKey, RocksDBMap.get) */
int sdfs_cdc_index_get(sdfs_cdc_index* ix, const uint8_t* d_digests, uint64_t n, uint64_t* d_pos,
                       uint64_t* d_refcount, void* stream);

/* Drop every fingerprint (AbstractHashesMap.clear / a fresh map), enqueued on `stream`. */
int sdfs_cdc_index_clear(sdfs_cdc_index* ix, void* stream);

/* Fingerprints held (synchronises the index's last stream) and slot capacity.  Fingerprints whose
 * count is <= 0 but which no sweep has removed yet are held.
 * (AbstractHashesMap.getSize / getMaxSize) */
int sdfs_cdc_index_size(sdfs_cdc_index* ix, uint64_t* used, uint64_t* capacity);

/* ---- releasing claims, collecting dead fingerprints, getting the space back ----
 *
 * The reference counts go both ways: DedupFileStore.removeRef (DedupFileStore.java:161-172) calls
 * claimKey(hash, val, -ct) for every HashLocPair of a deleted file or an overwritten block, addRef
 * (DedupFileStore.java:130-141) calls it with +ct for copies and snapshots (HCServiceProxy.claimKey
 * -> HashStore.claimKey -> RocksDBMap.claimKey, RocksDBMap.java:388-509), and the collection pass
 * RocksDBMap.claimRecords (RocksDBMap.java:630-714) removes what stayed unreferenced.
 *
 * One deliberate simplification.  RocksDBMap moves an entry whose count reaches <= 0 into a side
 * table (rmdb) with a time stamp (RocksDBMap.java:401-406,431-437); claimRecords later recovers it if it
 * was referenced again (RocksDBMap.java:663-680) or deletes it once it is older than
 * Main.HT_RM_THRESH.  Here such an entry STAYS IN THE TABLE, still found by put_records, get and
 * claim, with its count <= 0, until a sweep removes it: a put_records on it is a plain hit (dup =
 * 1, the old pos, count += claims — the reference's "reclaimed" branch; the chunk's data still
 * exists because nobody has been told to delete it).  There is no time stamp: the grace period
 * (Main.HT_RM_THRESH) is the caller's sweep schedule — whatever is unreferenced WHEN the sweep
 * runs is removed.  The count is a signed 64-bit value and is never clamped, so a batch's result
 * does not depend on the order in which its items are applied.
 *
 * A swept slot becomes a tombstone: lookups step over it and never match its stale key.
 * Fingerprints held plus tombstones count against the 7/8 fill.  When a put_records batch fits
 * the fingerprints held but not those plus the tombstones, the table is rebuilt first, on the
 * batch's stream (fingerprints held keep pos and count, tombstones go); only a batch that does
 * not fit the fingerprints held returns SDFS_CDC_ECAP.  The rebuild goes through a transient
 * second table allocated in stream order: it needs 64 x slots bytes of free device memory (as
 * much as the index itself) for its duration and returns SDFS_CDC_ENOMEM, with the index
 * unchanged, when that is not there.
 */

/* Add d_delta[i] (signed) to the count of fingerprint i (d_digests: n x 32 bytes, zero-padded) if
 * it is present and, when d_expect_pos != NULL and d_expect_pos[i] != UINT64_MAX, its pos equals
 * d_expect_pos[i]: d_out_pos[i] = its pos.  Otherwise nothing changes and d_out_pos[i] =
 * UINT64_MAX (the reference's -1: key not found or wrong archive).  Items with the same digest
 * all apply.  d_out_pos may be NULL.
 * (AbstractHashesMap.claimKey(hash, val, ct), RocksDBMap.java:388-509) */
int sdfs_cdc_index_claim(sdfs_cdc_index* ix, const uint8_t* d_digests, const uint64_t* d_expect_pos,
                         const int64_t* d_delta, uint64_t n, uint64_t* d_out_pos, void* stream);

/* Remove fingerprints whose count is <= 0: the first `cap` of them in slot order become
 * tombstones and their {digest[32], pos} are written to d_removed_digests / d_removed_pos (cap
 * entries each, order unspecified; may be NULL when cap = 0); the rest stay for the next call.
 * d_counts[0] = removed, d_counts[1] = dead fingerprints left behind (device, u64[2]).  The
 * caller tells the chunk store to drop the removed positions.
 * (AbstractHashesMap.claimRecords, RocksDBMap.java:630-714; see the note above on rmdb and
 * Main.HT_RM_THRESH) */
int sdfs_cdc_index_sweep(sdfs_cdc_index* ix, uint8_t* d_removed_digests, uint64_t* d_removed_pos,
                         uint64_t cap, uint64_t* d_counts, void* stream);

/* Rebuild the table now, on `stream`: fingerprints held keep pos and count, tombstones go.
 * Needs 64 x slots bytes of free device memory (SDFS_CDC_ENOMEM otherwise, index unchanged).
 * (the `compact` flag of RocksDBMap.claimRecords, RocksDBMap.java:697-708) */
int sdfs_cdc_index_compact(sdfs_cdc_index* ix, void* stream);

/* Fingerprints held, tombstones, and slot capacity (synchronises the index's last stream); any
 * output may be NULL.  (AbstractHashesMap.getSize / getMaxSize) */
int sdfs_cdc_index_stats(sdfs_cdc_index* ix, uint64_t* live, uint64_t* tombstones, uint64_t* capacity);

/* ---- map-file walks: claims straight from slot images, the audit, the way in and out ----
 *
 * The reference's file delete (LongByteArrayMap.vanish, LongByteArrayMap.java:817-882), snapshot
 * (copy(dest, true) -> index() -> nextValue(true), :884-890, :897-940, :310-356), trim (:595-648)
 * and truncate (:656-688) are walks over a whole map file that call DedupFileStore.removeRef /
 * addRef(p.hash, hashloc, 1) for every HashLocPair of every slot.  The calls below do that walk
 * on the device, straight from the slot images.
 *
 * An image is read by exactly the rule of sdfs_cdc_map_parse (sdfs_read.h): zlen <= 0 = no pairs;
 * 13 + zlen * BAL > slot_bytes, or any pair with a negative len / pos / offset / nlen = the slot is
 * SDFS_CDC_READ_CORRUPT and none of its pairs is applied; an all-zero slot has no pairs and status
 * 0.  The pairs that count are the TreeMap's: in an image whose pos values are not strictly
 * ascending, a pair that shares its pos with a later pair of the image does not count (each pair
 * is then compared with every later one; no writer produces such an image).  hash_len: 32 or 16.
 * d_sel (may be NULL = every slot): slot s takes part when d_sel[s] != 0; a slot that does not
 * gets status 0, 0 missed pairs, and keeps every byte.
 *
 * Two things the reference does are deliberately NOT mirrored:
 *   - addRef / removeRef skip hashloc 0 and 1 and the blank hash (DedupFileStore.java:131-136).
 *     put_records counts those pairs, and 0 / 1 are real positions when pos_base = 0, so here every
 *     pair counts.
 *   - nextValue(true) rewrites a pair's hashloc when addRef answers another value.  The claim here
 *     matches only an equal pos, so there is nothing to rewrite: the images are never edited.
 */

/* claimKey(hash, hashloc, delta) for every counting pair of the selected slots of the image
 * d_map (nslots x slot_bytes on the device): a digest that is held with pos == hashloc has delta
 * (non-zero) added to its count; any other pair changes nothing and is "missed" (the reference's
 * claimKey == -1, counted by vanish as "unable to remove orphaned reference").
 * d_slot_status[s] (required) = 0 or SDFS_CDC_READ_CORRUPT; d_slot_missed[s] (may be NULL) = the
 * slot's missed pairs; d_counts (required, device u64[4]) = {pairs applied, pairs missed, corrupt
 * slots, selected slots with at least one pair}.  With free_slots != 0 every selected slot whose
 * status is 0 is then overwritten with slot_bytes zeros (LongByteArrayMap.FREE; what trim does):
 * corrupt and unselected slots keep every byte (the reference's trim logs the exception and
 * stops at a corrupt slot; the batch flags the slot and goes on).  Validation is a kernel of its
 * own before any count moves, so the result does not depend on the schedule.  A slot with
 * thousands of pairs (the backup profile's 20 484) is spread over several waves. */
int sdfs_cdc_index_claim_slots(sdfs_cdc_index* ix, uint8_t* d_map, uint64_t nslots, uint32_t slot_bytes,
                               uint32_t hash_len, const uint8_t* d_sel, int64_t delta, int free_slots,
                               uint32_t* d_slot_status, uint32_t* d_slot_missed, uint64_t* d_counts,
                               void* stream);

/* writeSparseDataChunk for a batch of requests (StorageServiceImpl.java:275-382): the pairs of a
 * request whose `inserted` flag is not set are grouped by hash, DedupFileStore.addRef(hash, hashloc,
 * ct) must answer the same position for every group, or the request fails with its misses
 * (HashWriteException) and the slot is not written.  claim_slots applies whatever matches and
 * counts the rest; here a request goes in whole or not at all.
 *
 * d_req: nreq images (nreq x slot_bytes), read by exactly the rule stated above: corrupt images,
 * negative fields, the TreeMap rule for a repeated pos.  d_inserted (may be NULL = none):
 * d_inserted[r * pair_stride + i] != 0 = pair i of request r is `inserted` (the client has just
 * sent that chunk through writeChunks, whose put took the reference): a counting pair that is
 * inserted is skipped entirely, neither probed nor counted; pair_stride >= the pairs a slot holds.
 * A request is accepted iff it parses and EVERY counting pair that is not inserted names a
 * fingerprint held at pos == hashloc; an accepted request adds 1 per such pair (d_status[r] = 0).
 * A rejected one gets SDFS_CDC_INGEST_EMISSED (sdfs_ingest.h) or SDFS_CDC_READ_CORRUPT and moves NO
 * count, whatever its other pairs match; it does not stand in the way of the other requests.
 * d_req_missed[r] (required) = its misses; the first miss_cap misses are listed in d_miss_list as
 * {u32 request, u32 pair}, in unspecified order (may be NULL when miss_cap = 0).  d_counts
 * (required, device u64[6]) = {pairs added, pairs missed, pairs skipped as inserted, requests
 * accepted, requests rejected, misses listed}.
 * Validation, a check pass that probes and counts the misses, and an apply pass that runs only
 * where there were none are kernels of their own, so the decision holds across the several waves
 * that share a slot of thousands of pairs, and the result does not depend on the schedule.
 * The hashloc 0 / 1 and blank-hash skips of addRef are not mirrored (see above). */
int sdfs_cdc_index_addref_slots(sdfs_cdc_index* ix, const uint8_t* d_req, uint64_t nreq, uint32_t slot_bytes,
                                uint32_t hash_len, const uint8_t* d_inserted, uint32_t pair_stride,
                                uint32_t* d_status, uint32_t* d_req_missed, uint32_t* d_miss_list,
                                uint64_t miss_cap, uint64_t* d_counts, void* stream);

/* The audit: do the counts still match the files?  The same walk, but every counting pair whose
 * digest is held at pos == hashloc adds 1 to a shadow count of that fingerprint (zeroed by this
 * call; any other pair is missed); then every held entry's count (have) is compared with its
 * shadow (want).  d_counts (required, device u64[8]) = {pairs counted, pairs missed, corrupt
 * slots, entries with have < want, entries with have > want, entries with want == 0, entries
 * equal, mismatches listed}.  The first `cap` entries with have != want in table-slot order go to
 * d_mis_digests (cap x 32), d_mis_pos, d_mis_have, d_mis_want (int64; all four may be NULL when
 * cap = 0).  With repair != 0 every held entry's count is then set to its want: entries nobody
 * names go to 0 and the next sdfs_cdc_index_sweep collects them.  The counts and the list describe
 * the state BEFORE the repair.
 * The caller's duty: the image must hold every persisted slot of the volume — every file's map,
 * snapshots included — or entries named only by the slots left out read as over-counted (and a
 * repair would hand them to the sweep).
 * The shadow lives in the 8 spare bytes of the fingerprint's own 64-byte table slot: no
 * allocation (so no SDFS_CDC_ENOMEM), and the add lands in the cache line the probe fetched. */
int sdfs_cdc_index_recount(sdfs_cdc_index* ix, const uint8_t* d_map, uint64_t nslots, uint32_t slot_bytes,
                           uint32_t hash_len, const uint8_t* d_sel, int repair, uint32_t* d_slot_status,
                           uint32_t* d_slot_missed, uint8_t* d_mis_digests, uint64_t* d_mis_pos,
                           int64_t* d_mis_have, int64_t* d_mis_want, uint64_t cap, uint64_t* d_counts,
                           void* stream);

/* The way in with explicit positions (a restart from the system of record's iteration, or from
 * an export).  Item i = {d_digests[i*32 .. +32), d_pos[i], d_ref[i]}.  A digest that is not held
 * is inserted; its pos is the smallest d_pos among the items of this call that name it.  Then for
 * every item: the entry's pos == d_pos[i] -> its count += d_ref[i], d_status[i] = 0; otherwise
 * nothing is added and d_status[i] = 1 (conflict).  The outcome is a function of the arguments
 * alone.  Fill, the rebuild before SDFS_CDC_ECAP and SDFS_CDC_ENOMEM are as for put_records. */
int sdfs_cdc_index_load(sdfs_cdc_index* ix, const uint8_t* d_digests, const uint64_t* d_pos,
                        const int64_t* d_ref, uint64_t n, uint8_t* d_status, void* stream);

/* The way out: every held entry, those with count <= 0 included, in table-slot order; the first
 * `cap` are written to d_digests (cap x 32), d_pos, d_ref (may be NULL when cap = 0).
 * d_n (required, device u64[2]) = {written, held}. */
int sdfs_cdc_index_export(sdfs_cdc_index* ix, uint8_t* d_digests, uint64_t* d_pos, int64_t* d_ref,
                          uint64_t cap, uint64_t* d_n, void* stream);

/* Test hook: the batch epoch counter (31 bits; the next put_records uses epoch + 1, wrapping to 1).
 * Stamps only mark a batch's own insertions while it runs, so any value is safe. */
int sdfs_cdc_index_set_epoch(sdfs_cdc_index* ix, uint32_t epoch);

#ifdef __cplusplus
}
#endif
#endif /* SDFS_INDEX_H */
