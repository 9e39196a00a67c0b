/*
 * sdfs_ingest.h — C-ABI of the client-side dedup front end: the server half of checkHashes,
 * writeChunks and writeSparseDataChunk for batches.
 *
 * A remote client runs getChunks itself with the parameters hashingInfo publishes, asks which
 * fingerprints the server holds (StorageServiceImpl.checkHashes, StorageServiceImpl.java:175-211:
 * HashesMap.get per hash = sdfs_cdc_index_get, sdfs_index.h), sends only the chunks that are
 * missing (writeChunks, :214-272) and then each buffer's SparseDataChunk (writeSparseDataChunk,
 * :275-382 = sdfs_cdc_index_addref_slots, sdfs_index.h).  The calls below are writeChunks: chunks
 * that are already cut, hashes that are given rather than computed, a mix of raw and LZ4
 * payloads.  They turn such a batch into what the write path already takes — a dense staging area
 * of raw chunks, 48-byte fingerprint records {hash, buffer_id = entry index, start = 0, len =
 * raw_len} and a d_buf_offs table — so that sdfs_cdc_index_put_records, sdfs_cdc_lz4_plan_records,
 * the archive plan, pack and map_emit run on them unchanged, and the store that results is the one
 * the same data gives through HipBufferWriter.write.
 *
 * One batch is six calls on one stream, none of which reads anything back to the host:
 *   plan -> decode (the compressed entries) -> copy (the raw ones) -> [verify] -> records
 *        -> (put_records and the store tail, by the caller) -> results
 *
 * Two deliberate divergences from the reference:
 *   - writeChunks fails the whole request on the first bad entry, after whatever puts had already
 *     run (StorageServiceImpl.java:226-262).  Here a bad entry is flagged in its status word and left
 *     out, and the rest of the batch goes in.
 *   - HashBlobArchive only logs a chunk whose hash is not its client's (HashBlobArchive.java:
 *     1270-1276, under VERIFY_WRITES).  With the verify call such an entry is refused
 *     (SDFS_CDC_INGEST_EHASH); without it the chunk is stored under the client's hash, as the
 *     reference does.
 *
 * Offsets and lengths that come from the client are checked on the device and flagged, never
 * followed.  Errors, threading and the last-error message follow include/sdfs_cdc.h; arguments are
 * checked before the device is touched; per-call scratch is stream-ordered.
 */
#ifndef SDFS_INGEST_H
#define SDFS_INGEST_H

#include <stdint.h>

#include "sdfs_cdc.h"
#include "sdfs_lz4.h"

#ifdef __cplusplus
extern "C" {
#endif

/* an entry's (writeChunks) or a request's (writeSparseDataChunk) status word: 0 = accepted */
#define SDFS_CDC_INGEST_EMPTY 1u    /* len == 0: InsertRecord(false, -1, 0), StorageServiceImpl.java:228-231 */
#define SDFS_CDC_INGEST_EBOUNDS 2u  /* raw_len 0 or > chunk_length, payload outside the blob, raw len != raw_len,
                                       or no room left in the staging area */
#define SDFS_CDC_INGEST_EDECODE 4u  /* the LZ4 block does not decode to exactly raw_len bytes */
#define SDFS_CDC_INGEST_EHASH 8u    /* verify: the chunk's fingerprint is not the client's hash */
#define SDFS_CDC_INGEST_EMISSED 16u /* addref_slots: a pair names a fingerprint that is not held at its hashloc */

#define SDFS_CDC_INGEST_NONE 0xFFFFFFFFu /* rec_of: the entry has no record */
#define SDFS_CDC_INGEST_TILE 1024u       /* entries the plan and records kernels scan per step */
#define SDFS_CDC_INGEST_COPY_SPAN 65536u /* bytes of one entry a workgroup of the copy kernel moves */

/* The client's entries (device).  Entry i = {hash[i*32 .. +32) zero-padded past the digest,
 * blob[off[i] .. +len[i]), raw_len[i] = its uncompressed length, compressed[i] != 0: the payload is
 * an LZ4 block} — ChunkEntry {hash, data, compressed, compressedLength}, where compressedLength
 * is, despite its name, the uncompressed length (decompressLz4(data, compressedLength),
 * StorageServiceImpl.java:233-236). */
typedef struct sdfs_cdc_ingest_batch {
    const uint8_t* hash;
    const uint8_t* blob;
    uint64_t blob_bytes;
    const uint64_t* off;
    const uint32_t* len;
    const uint32_t* raw_len;
    const uint8_t* compressed;
    uint64_t n;
} sdfs_cdc_ingest_batch;

/* What the plan lays out and the later calls fill in (device; every array holds n entries). */
typedef struct sdfs_cdc_ingest_plan {
    uint32_t* status;      /* [n] the entry's status word */
    uint64_t* stage_off;   /* [n] where the entry's raw chunk lies in the staging area: the exclusive
                              prefix of raw_len over the entries the plan let through (also the
                              d_buf_offs of sdfs_cdc_lz4_plan_records); 0 for the others */
    uint32_t* rec_of;      /* [n] the entry's fingerprint record, SDFS_CDC_INGEST_NONE without one */
    /* the compressed entries alone, in entry order: the decoder's batch */
    uint64_t* dec_src_off; /* [n] */
    uint32_t* dec_src_len; /* [n] */
    uint64_t* dec_dst_off; /* [n] */
    uint32_t* dec_cap;     /* [n] raw_len */
    uint32_t* dec_len;     /* [n] written by the decoder */
    uint32_t* dec_entry;   /* [n] the item's entry */
    uint32_t* dec_count;   /* [1] items of the decoder's batch */
    uint64_t* staged;      /* [1] bytes of the staging area in use */
} sdfs_cdc_ingest_plan;

/* Classify the entries: len == 0 -> EMPTY; raw_len == 0, raw_len > chunk_length, off + len past
 * blob_bytes, a raw entry with len != raw_len, or a chunk that would end past stage_cap -> EBOUNDS;
 * every other entry is a decode item (compressed) or a copy item and gets its place in the
 * staging area.  Writes status, stage_off, the decoder's batch, *dec_count and *staged; rec_of is
 * left to the records call.
 * (the entry loop of writeChunks, StorageServiceImpl.java:226-240) */
int sdfs_cdc_ingest_chunks_plan(int device, const sdfs_cdc_ingest_batch* b, uint32_t chunk_length,
                                uint64_t stage_cap, const sdfs_cdc_ingest_plan* p, void* stream);

/* The compressed entries through sdfs_cdc_lz4_decompress_device(framed = 0) with dst_cap =
 * raw_len, into d_stage; an entry whose decoded length is not exactly raw_len gets EDECODE.
 * (CompressionUtils.decompressLz4 = LZ4FastDecompressor.decompress(src, destLen),
 * StorageServiceImpl.java:233-236, CompressionUtils.java:122-125) */
int sdfs_cdc_ingest_chunks_decode(sdfs_cdc_lz4* z, const sdfs_cdc_ingest_batch* b, const sdfs_cdc_ingest_plan* p,
                                  uint8_t* d_stage, void* stream);

/* The raw entries' bytes into d_stage.  Sources and destinations have any alignment: 16-byte
 * vector stores, edges byte by byte; a workgroup moves SDFS_CDC_INGEST_COPY_SPAN bytes of one
 * entry.  (chunk = ent.getData().toByteArray(), StorageServiceImpl.java:237-239) */
int sdfs_cdc_ingest_chunks_copy(int device, const sdfs_cdc_ingest_batch* b, const sdfs_cdc_ingest_plan* p,
                                uint32_t chunk_length, uint8_t* d_stage, void* stream);

/* Optional: fingerprint the staged chunks (sdfs_cdc_hash_device) and compare hash_len bytes with
 * the client's hash; a mismatch gets EHASH.  hash_len must be the engine's digest length.
 * (HashBlobArchive.java:1270-1276 VERIFY_WRITES; refused here, logged there) */
int sdfs_cdc_ingest_chunks_verify(sdfs_cdc_engine* engine, const sdfs_cdc_ingest_batch* b,
                                  const sdfs_cdc_ingest_plan* p, const uint8_t* d_stage, uint32_t hash_len,
                                  void* stream);

/* The accepted entries (status 0), compacted in entry order, as 48-byte fingerprint records
 * {hash, buffer_id = entry index, start = 0, len = raw_len} in d_records (room for n);
 * *d_count (u32) = their number; p->rec_of[i] = the entry's record.
 * (new ChunkData(hash, chunk), StorageServiceImpl.java:241) */
int sdfs_cdc_ingest_chunks_records(int device, const sdfs_cdc_ingest_batch* b, const sdfs_cdc_ingest_plan* p,
                                   uint8_t* d_records, uint32_t* d_count, void* stream);

/* After sdfs_cdc_index_put_records(d_records, d_count, pos_base) -> d_dup / d_hashloc and the
 * store tail -> d_rec_len (the stored length of the k-th inserted record, n_new_cap entries; may be
 * NULL = 0), per entry: d_inserted (u8), d_pos (-1 for empty and rejected entries), d_stored_len
 * (the stored record's length for an inserted entry, else 0: RocksDBMap.java:829, 862) and
 * d_status.  Every put adds one reference whether or not it inserted (RocksDBMap.java:797-809,
 * 842-862), which is what put_records does with one record per entry.
 * (InsertRecord -> ChunkEntryResponse, StorageServiceImpl.java:242-250) */
int sdfs_cdc_ingest_chunks_results(int device, const sdfs_cdc_ingest_batch* b, const sdfs_cdc_ingest_plan* p,
                                   const uint8_t* d_dup, const uint64_t* d_hashloc, uint64_t pos_base,
                                   const uint32_t* d_rec_len, uint64_t n_new_cap, uint8_t* d_inserted,
                                   int64_t* d_pos, uint32_t* d_stored_len, uint32_t* d_status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDFS_INGEST_H */
