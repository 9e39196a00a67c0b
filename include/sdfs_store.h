/*
 * sdfs_store.h — C-ABI for reopening a chunk store from the bytes it persists: the archive images
 * and their .map images (sdfs_archive.h wrote them), and for scrubbing it at rest.
 *
 * sdfs_archive.h ends in images that match HashBlobArchive and SimpleByteArrayLongMap byte for
 * byte; sdfs_read.h starts from a directory of where each record lies.  These entry points go from
 * the one to the other, with nothing but the images and the index:
 *
 *     sdfs_cdc_store_scan       the images -> the record list, in put order
 *     sdfs_cdc_store_raw_lens   the chunk length a decrypted record announces
 *     sdfs_cdc_store_directory  the record list + the index's hashloc -> the read path's directory
 *     sdfs_cdc_store_lookup     SimpleByteArrayLongMap.get for a batch of (archive, key)
 *     sdfs_cdc_store_verify     the scrub's last step: every decoded chunk against its key
 *
 * The rules, all from the reference: setUp on an existing file (SimpleByteArrayLongMap.java:198-261),
 * next (:136-175), index / indexRehashed (:340-400), get (:562-599), getChunk after the lookup
 * (HashBlobArchive.java:1712-1950), the IV read from the archive header (:1228-1249).
 *
 * Positions have the layout's meaning (sdfs_cdc_archive_layout.pos): pos = cp + 8 + hash_len, the
 * record's first byte; the map's value is pos - 4.
 *
 * Every offset or length read from an image is compared with arc_bytes or the map's length before
 * anything is loaded through it: a wrong value sets a flag and is never dereferenced.  An archive
 * that does not lie inside [0, store_bytes) is treated as 0 bytes long (every record of it: RANGE).
 *
 * Not here: walking an archive without its map (the reference never does), rebuilding the index
 * from the archives (hashloc is the insertion rank: a rebuilt index would invalidate every
 * persisted map slot), files on disk, the SMART_CACHE .cmap.
 *
 * Errors, the thread-local sdfs_cdc_last_error() message and the stream conventions follow
 * sdfs_archive.h: arguments are checked before the device is touched, per-call scratch is
 * allocated and released in stream order, no call synchronises with the host, every output element
 * is written exactly once (counters: zeroed, then added to).
 */
#ifndef SDFS_STORE_H
#define SDFS_STORE_H

#include <stdint.h>

#include "sdfs_archive.h"

#ifdef __cplusplus
extern "C" {
#endif

/* record flags, a bitmask, 0 = clean */
#define SDFS_CDC_STORE_RANGE 1u  /* the record, or for a version-0 slot its length word, lies outside [header_bytes, arc_bytes) */
#define SDFS_CDC_STORE_KEY 2u    /* the [BE32 hash_len][key] in front of the record differs from the slot's key */
#define SDFS_CDC_STORE_LEN 4u    /* version > 0 only: the slot's length differs from the image's */
#define SDFS_CDC_STORE_NZ 8u     /* len < 4, or raw_len > max_chunk */
#define SDFS_CDC_STORE_FETCH 16u /* verify: the record could not be decrypted or decoded */
#define SDFS_CDC_STORE_HASH 32u  /* verify: the chunk's digest differs from the key */
/* flags after which a record is not fetched: its extent or its chunk length cannot be trusted (raw_len is 0) */
#define SDFS_CDC_STORE_UNREADABLE (SDFS_CDC_STORE_RANGE | SDFS_CDC_STORE_LEN | SDFS_CDC_STORE_NZ)

/* archive status, a bitmask, 0 = OK */
#define SDFS_CDC_STORE_GAP 1u    /* header_bytes + sum of 8 + hash_len + len over the unflagged records != arc_bytes:
                                    bytes no map entry accounts for, or two entries that overlap */
#define SDFS_CDC_STORE_SLOTS 2u  /* the map has more slots than slot_stride: the archive was not scanned (0 records) */

/* status word of a scan */
#define SDFS_CDC_STORE_ECAP 1u   /* more records than n_cap: only count and status were written */

#define SDFS_CDC_STORE_SORT_LDS 16384u /* (pos, slot) pairs the scan sorts in LDS; above: in global scratch */

/* The scan's record list: device arrays of n_cap entries, *count of them valid. */
typedef struct sdfs_cdc_store_records {
    uint32_t* arc;        /* the record's archive */
    uint32_t* slot;       /* its slot in that archive's map */
    uint32_t* pos;        /* its first byte inside the archive image */
    uint32_t* len;        /* its stored length; 0 with RANGE or LEN */
    uint64_t* store_off;  /* arc_base[arc] + pos */
    uint8_t* key;         /* [n_cap * 32] the slot's key, zero-padded */
    uint32_t* raw_len;    /* plain != 0: the chunk's length by the nz rule; else 0 */
    uint32_t* flags;      /* SDFS_CDC_STORE_RANGE .. _NZ */
    uint32_t* count;      /* [1] records found */
    uint32_t* status;     /* [1] 0 or SDFS_CDC_STORE_ECAP */
    uint32_t n_cap;       /* >= the sum of the maps' slot counts can never fail */
    uint32_t reserved;
} sdfs_cdc_store_records;

/* The scan's per-archive outputs: device arrays of n_arc entries. */
typedef struct sdfs_cdc_store_archives {
    uint32_t* map_slots;  /* size: the map's slot count */
    uint32_t* version;    /* the map's version: the file's with the magic, else 0 */
    uint32_t* arc_first;  /* [n_arc + 1] archive a holds records arc_first[a] .. arc_first[a + 1) */
    uint8_t* ivs;         /* [n_arc * 16] bytes 4 .. 20 of the archive header; only with header_bytes != 0 (else may be NULL) */
    uint32_t* slot_rec;   /* [n_arc * slot_stride] the record ordinal in each slot, SDFS_CDC_ARCHIVE_NONE for a free one
                             and for the columns past size: the row layout sdfs_cdc_archive_map_emit writes */
    uint32_t* status;     /* SDFS_CDC_STORE_GAP | _SLOTS */
    uint32_t slot_stride;
    uint32_t reserved;
} sdfs_cdc_store_archives;

/* The images -> the record list.
 * Archive a's image is d_store[d_arc_base[a] .. + d_arc_bytes[a]) (store_bytes = the bytes d_store
 * holds), its .map image d_maps[a * map_stride_bytes .. + map_len[a]).  map_len is a HOST array of
 * the n_arc true file lengths (a directory listing has them; the geometry is decided from them
 * before anything is read): a map_len above map_stride_bytes is SDFS_CDC_EINVAL.
 * Map geometry per archive, as setUp does: version == 0: EL = hash_len + 4, no header.  version !=
 * 0: a length <= 16 is an empty map; in a longer file BE32 6442 at byte 0 means [header 16][EL =
 * hash_len + 8] with the version taken from bytes 4 .. 8, anything else the version-0 layout.  size
 * = (len - offset) / EL; trailing bytes are ignored.
 * Slots are walked as next() does; a slot whose hash_len key bytes are all zero is free.  The
 * slot's value starts with BE32 pos - 4; a slot of a map with version > 0 has BE32 len after it,
 * otherwise len is the BE32 at pos - 4 of the archive image.
 * Records come out archive by archive, in ascending pos inside an archive, ties broken by slot:
 * put order, so a never-compacted store reopens to the layout it was written with.  A flagged
 * record keeps its place.  raw_len (plain != 0: the stored records are not encrypted): with nz =
 * BE32 at pos as a signed int, nz if nz > 0, else len - 4 (HashBlobArchive.java:1922-1934).
 * max_chunk: the engine's maxLen.  hash_len: 16 or 32; 20 is SDFS_CDC_EINVAL for the reason given
 * at sdfs_cdc_archive_map_emit.  header_bytes: 0 or SDFS_CDC_ARCHIVE_HEADER.
 * Kernels: a count per archive, a one-block prefix (arc_first, count, ECAP), then one workgroup per
 * archive: (pos, slot) of every slot sorted (bitonic; in LDS up to SDFS_CDC_STORE_SORT_LDS slots,
 * else in global scratch), one thread per record for the checks and the outputs. */
int sdfs_cdc_store_scan(int device, uint32_t n_arc, const uint8_t* d_store, uint64_t store_bytes,
                        const uint64_t* d_arc_base, const uint64_t* d_arc_bytes, const uint8_t* d_maps,
                        uint64_t map_stride_bytes, const uint64_t* map_len, uint32_t hash_len, uint32_t version,
                        uint32_t header_bytes, uint32_t max_chunk, int plain, const sdfs_cdc_store_records* recs,
                        const sdfs_cdc_store_archives* arcs, void* stream);

/* The nz rule of the scan for records that had to be decrypted first: record i (i < *d_count when
 * d_count != NULL, else i < n_max) is d_plain[d_off[i] .. + d_len[i]), d_len[i] == UINT32_MAX = the
 * decrypt failed.  d_raw_len[i] = nz if nz > 0 else len - 4; with len < 4 (a failed decrypt included)
 * or raw_len > max_chunk: 0, and SDFS_CDC_STORE_NZ is or-ed into d_flags[i].  A record whose
 * d_flags[i] is not 0 on entry is not looked at: raw_len 0.  The scan runs this same code. */
int sdfs_cdc_store_raw_lens(int device, const uint8_t* d_plain, const uint64_t* d_off, const uint32_t* d_len,
                            const uint32_t* d_count, uint64_t n_max, uint32_t max_chunk, uint32_t* d_raw_len,
                            uint32_t* d_flags, void* stream);

/* The read path's directory (what sdfs_cdc_read_plan takes) from the scan's records (n = *d_count
 * when d_count != NULL, else n_max) and their hashloc from the index (sdfs_cdc_index_get on the
 * keys; < 0 = the index does not hold the key).  Entry k = hashloc - pos_base, k < n_store:
 * d_store_off[k], d_store_len[k], d_store_raw_len[k], d_rec_of_k[k] of the record that claims k; all
 * n_store entries are written: length 0, offset 0 and ordinal SDFS_CDC_ARCHIVE_NONE where no record
 * does, which is what a compaction leaves for a dropped entry.  d_info[3] = {orphans: records whose
 * key the index does not hold (compact() would drop them) or that carry a flag of the scan, records
 * whose k is outside [0, n_store), clashes: records that claim a k a record of lower ordinal has}.
 * n_store == 0: there is no directory, the four outputs must be NULL (anything else is
 * SDFS_CDC_EINVAL) and only d_info is written. */
int sdfs_cdc_store_directory(int device, const uint64_t* d_rec_store_off, const uint32_t* d_rec_len,
                             const uint32_t* d_rec_raw_len, const uint32_t* d_rec_flags, const int64_t* d_hashloc,
                             const uint32_t* d_count, uint64_t n_max, uint64_t pos_base, uint64_t n_store,
                             uint64_t* d_store_off, uint32_t* d_store_len, uint32_t* d_store_raw_len,
                             uint32_t* d_rec_of_k, uint64_t* d_info, void* stream);

/* HashBlobArchive.getChunk's lookup for n_q queries (archive d_q_arc[q], key d_q_key[q * 32 .. +
 * hash_len)) on the map images as they lie (the image arguments and the geometry of
 * sdfs_cdc_store_scan).  index() / indexRehashed(): h = BE32(key[8 .. 12)) & 0x7fffffff, home slot h %
 * size; a hit returns; a free slot ends the search with "absent"; otherwise backwards by 1 + h %
 * (size - 2) modulo size until back at the home slot.  size <= 2 with a home slot that is neither
 * a hit nor free is absent (the reference's % 0 throws and get returns -1), and so are an archive
 * >= n_arc and an all-zero key (the reference would hand back a free slot's zero value; no writer
 * stores such a key).  Found: d_slot, d_pos, d_len, d_store_off, and in d_flags the RANGE / KEY / LEN
 * checks of the scan (len 0 with RANGE or LEN).  Absent: slot SDFS_CDC_ARCHIVE_NONE, the rest 0.
 * One query per lane. */
int sdfs_cdc_store_lookup(int device, uint32_t n_arc, const uint8_t* d_store, uint64_t store_bytes,
                          const uint64_t* d_arc_base, const uint64_t* d_arc_bytes, const uint8_t* d_maps,
                          uint64_t map_stride_bytes, const uint64_t* map_len, uint32_t hash_len, uint32_t version,
                          uint32_t header_bytes, const uint32_t* d_q_arc, const uint8_t* d_q_key, uint64_t n_q,
                          uint32_t* d_slot, uint32_t* d_pos, uint32_t* d_len, uint64_t* d_store_off,
                          uint32_t* d_flags, void* stream);

/* The scrub's last step.  Chunk i (i < *d_count when d_count != NULL, else i < n_max) is
 * d_chunks[d_off[i] .. + d_len[i]), d_len[i] == UINT32_MAX = the decrypt or the decode failed; its key
 * d_keys[i * 32 .. + hash_len).  Fingerprints the chunks with sdfs_cdc_hash_device and or-s into
 * d_flags[i] SDFS_CDC_STORE_FETCH for a failed fetch, SDFS_CDC_STORE_HASH for a digest that differs
 * from the key.  A record that comes in with one of SDFS_CDC_STORE_UNREADABLE has nothing to fetch
 * and is left as it is.  The engine's digest length must equal hash_len.  Runs on the device
 * d_flags lies on. */
int sdfs_cdc_store_verify(sdfs_cdc_engine* engine, const uint8_t* d_chunks, const uint64_t* d_off,
                          const uint32_t* d_len, const uint8_t* d_keys, const uint32_t* d_count, uint64_t n_max,
                          uint32_t hash_len, uint32_t* d_flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDFS_STORE_H */
