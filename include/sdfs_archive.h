/*
 * sdfs_archive.h — C-ABI of the device-side chunk store layer: the archive images
 * HashBlobArchive writes for new records, their .map images, and compaction after an index sweep.
 *
 * The write path ends with the putChunk records of the new chunks ([BE32 nz][chunk | LZ4 block],
 * optionally AES-CBC ciphertext of it: sdfs_lz4.h, sdfs_aes.h) at worst-case-spaced offsets; the
 * read path (sdfs_read.h) starts from a directory of where each record lies.  The reference
 * joins the two with HashBlobArchive (HashBlobArchive.java): putChunk appends
 *     [BE32 hash.length][hash][BE32 record.length][record]
 * at np and advances np by 4 + hash.length + 4 + record.length (:1330-1331,1399-1411), stores
 * hash -> cp + 4 + hash.length in the archive's SimpleByteArrayLongMap (:1334-1350; with VERSION > 0
 * the value is (that << 32) | record.length), and closes the archive in favour of a new one
 * (:740-764) when np >= blocksz before the put or the map holds >= (int)(size * .75) entries
 * (:1305-1316, SimpleByteArrayLongMap.java:187-189).  With VERSION > 0 an archive starts with a
 * 1024-byte header [BE32 VERSION][16-byte IV][zeros] (:299-301,1023-1033).  These entry points
 * do that for a device-resident batch:
 *
 *     sdfs_cdc_archive_map_size   NextPrime.getNextPrimeI: slots of a map made for sz entries
 *     sdfs_cdc_archive_plan       which record goes into which archive, and where
 *     sdfs_cdc_archive_pack       the archive images: the one pass over the data
 *     sdfs_cdc_archive_map_emit   the .map file image of every archive
 *     sdfs_cdc_archive_compact    HashBlobArchive.compact() for the archives of one call
 *
 * Not here: files on disk, archive ids, cloud upload, the SMART_CACHE read-side map and
 * VERIFY_WRITES (sdfs_cdc_hash_device covers it).  Errors, threading, the thread-local
 * sdfs_cdc_last_error() message and the stream conventions follow sdfs_cdc.h; arguments are checked
 * before the device is touched.  Per-call scratch is allocated and released in stream order.  No
 * call synchronises with the host.
 */
#ifndef SDFS_ARCHIVE_H
#define SDFS_ARCHIVE_H

#include <stdint.h>

#include "sdfs_cdc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDFS_CDC_ARCHIVE_ALIGN 4096u     /* every archive image starts at a multiple of this */
#define SDFS_CDC_ARCHIVE_HEADER 1024u    /* HashBlobArchive.offset with VERSION > 0 (:299-301) */
#define SDFS_CDC_ARCHIVE_NONE UINT32_MAX /* "no record" in d_slot_rec, "dropped" in d_new_of_old */
#define SDFS_CDC_ARCHIVE_MAP_MAGIC 6442u /* SimpleByteArrayLongMap.MAGIC_NUMBER */

/* status word of a layout, a bitmask, 0 = OK */
#define SDFS_CDC_ARCHIVE_ECAP 1u   /* the batch needs more than arc_cap archives: nothing else was written */
#define SDFS_CDC_ARCHIVE_ESTORE 2u /* pack: the layout's store_bytes exceed the store handed in: nothing was written */

/* Where a call's records lie: a structure of device arrays.  n = the call's records, n_arc = the
 * archives they fill.  Archive a holds records arc_first[a] .. arc_first[a + 1); its image is
 * arc_bytes[a] long and starts at arc_base[a] in the store; arc_base is the exclusive prefix of
 * arc_bytes with every base rounded up to SDFS_CDC_ARCHIVE_ALIGN. */
typedef struct sdfs_cdc_archive_layout {
    uint32_t* arc;        /* [n] the record's archive */
    uint32_t* pos;        /* [n] the record's position inside its archive: cp + 8 + hash_len */
    uint64_t* store_off;  /* [n] arc_base[arc] + pos: what sdfs_cdc_read_plan's directory takes */
    uint32_t* arc_first;  /* [arc_cap + 1] */
    uint64_t* arc_bytes;  /* [arc_cap] np when the archive closed = its file length */
    uint64_t* arc_base;   /* [arc_cap] */
    uint64_t* totals;     /* [2] n_arc, store_bytes = arc_base[n_arc - 1] + arc_bytes[n_arc - 1] (0 for no archive) */
    uint32_t* status;     /* [1] SDFS_CDC_ARCHIVE_* */
    uint32_t arc_cap;
    uint32_t reserved;
} sdfs_cdc_archive_layout;

/* NextPrime.getNextPrimeI(sz) (NextPrime.java:56-88), the slot count SimpleByteArrayLongMap gives
 * a map made for sz entries (SimpleByteArrayLongMap.java:66-67): 2 for sz <= 2; 3, 5, 7 for sz <=
 * 3, 5, 7; else the first odd prime >= sz | 1.  0 where the reference throws (the prime would
 * exceed Integer.MAX_VALUE, i.e. sz > 2^31 - 1).  Host only. */
uint32_t sdfs_cdc_archive_map_size(uint64_t sz);

/* Bytes of the store one workgroup of the pack kernel writes (its spans are cut at absolute
 * 16-byte addresses of d_store). */
uint32_t sdfs_cdc_archive_pack_span(void);

/* Bytes of one archive's .map image for a map of map_slots slots: version 0: map_slots *
 * (hash_len + 4); version > 0: 16 + map_slots * (hash_len + 8) (SimpleByteArrayLongMap.java:224-261). */
uint64_t sdfs_cdc_archive_map_bytes(uint32_t map_slots, uint32_t hash_len, uint32_t version);

/* The putChunk "archive full" rule for records 0 .. n (n = *d_count when d_count != NULL, else
 * n_max) of lengths d_rec_len[i] (the stored records: d_dst_len of sdfs_cdc_lz4_compress_device or
 * of sdfs_cdc_aes_encrypt_device), in record order.  np starts at header_bytes (0, or
 * SDFS_CDC_ARCHIVE_HEADER for VERSION > 0); record i goes into the open archive iff np < blocksz
 * and entries < (int)(map_slots * .75) (HashBlobArchive.java:1305-1316); otherwise the archive
 * closes and i is the first record of a new one (:740-764).  So a record is never split, a
 * record larger than blocksz still goes in while np < blocksz, and the last accepted record may
 * carry np past blocksz.  Archive a uses blocksz[min(a, n_blocksz - 1)] (host array of 1 .. 256 values:
 * the reference draws nextSize() per archive, :271-280); map_slots is sdfs_cdc_archive_map_size(MAX_HM_SZ).
 * hash_len: 16, 20 or 32.
 * Writes the whole layout; when the batch needs more than out->arc_cap archives only *status =
 * SDFS_CDC_ARCHIVE_ECAP is written.  SDFS_CDC_EINVAL: a blocksz above 2^31 - 1 (the version-0 map value is
 * an int) or not above header_bytes, map_slots < 2.
 * One workgroup: an exclusive prefix of 8 + hash_len + len, then one wave walks from archive to
 * archive by a 64-way search on that prefix, then the per-record outputs in parallel. */
int sdfs_cdc_archive_plan(int device, const uint32_t* d_rec_len, const uint32_t* d_count, uint64_t n_max,
                          uint32_t hash_len, uint32_t header_bytes, const uint64_t* blocksz, uint32_t n_blocksz,
                          uint32_t map_slots, const sdfs_cdc_archive_layout* out, void* stream);

/* The archive images (HashBlobArchive.java:1399-1411 per record, :1023-1033 per header):
 * d_store[0 .. store_bytes) = for every archive, at its base, the header when header_bytes != 0
 * ([BE32 version][d_ivs[a * 16 .. + 16)][zeros]), then each of its records as
 *     [BE32 hash_len][digest[0 .. hash_len)][BE32 len][bytes]
 * and zeros from an image's end to the next base.  Every byte of [0, store_bytes) is written
 * exactly once and nothing beyond; the caller does not clear the store.  store_cap = the bytes
 * d_store holds: when the layout's store_bytes exceed it, only SDFS_CDC_ARCHIVE_ESTORE is or-ed
 * into the layout's status.  A layout whose status is not 0 packs nothing.
 * Record i's bytes are d_src[d_src_off[i] .. + d_src_len[i]) in whatever sparse layout the
 * compressor or cipher left them (len = d_src_len[i] = the plan's d_rec_len[i]); with raw_frame !=
 * 0 the source holds the raw chunks and the record is [BE32 -1][chunk] (Main.compress off,
 * :1281-1289; len = d_src_len[i] + 4 = the plan's d_rec_len[i]).  Its digest is the first hash_len
 * bytes of fingerprint record d_sel[i] (d_sel NULL: i) of d_records, exactly as
 * sdfs_cdc_lz4_plan_records takes its extents.  d_ivs (16 bytes per archive) is only read when
 * header_bytes != 0.
 * d_src must be 16-byte aligned and its allocation must end on a 16-byte boundary: the kernel
 * loads the aligned 16-byte vectors that contain a record's first and last byte, and nothing
 * further.  d_store may have any alignment.
 * Destination-driven, the mirror image of sdfs_cdc_read_assemble's gather: a workgroup owns
 * sdfs_cdc_archive_pack_span() bytes of the store cut at absolute 16-byte addresses, finds its
 * records by binary search on their start positions, stores aligned 16-byte vectors, takes a
 * vector inside a record from two aligned 16-byte loads realigned by a byte shift, and builds
 * the vectors that touch a header or a record edge byte by byte. */
int sdfs_cdc_archive_pack(int device, const sdfs_cdc_archive_layout* layout, const uint32_t* d_count,
                          uint64_t n_max, const uint8_t* d_src, const uint64_t* d_src_off,
                          const uint32_t* d_src_len, int raw_frame, const uint8_t* d_records,
                          const uint32_t* d_sel, uint32_t hash_len, uint32_t header_bytes, uint32_t version,
                          const uint8_t* d_ivs, uint8_t* d_store, uint64_t store_cap, void* stream);

/* The .map file image of every archive (SimpleByteArrayLongMap.java:224-261,509-539): archive a's
 * image at d_maps + a * sdfs_cdc_archive_map_bytes(map_slots, ..), of size[a] = d_map_slots[a]
 * (d_map_slots NULL: map_slots) slots.  version == 0: no header, slots [key][BE32 pos]; version >
 * 0: [BE32 6442][BE32 version][8 zero bytes], slots [key][BE32 pos][BE32 len].  pos = the layout's
 * pos - 4 = cp + 4 + hash_len (HashBlobArchive.java:1336,1345), len = d_rec_len[i].  Free slots and
 * the bytes between an image's end and the next image are zero; images of archives at or past
 * n_arc are not written.
 * Placement (insertionIndex / insertKeyRehash, SimpleByteArrayLongMap.java:427-498): h =
 * BE32(key[8 .. 12)) & 0x7fffffff, home slot h % size, on a collision step BACKWARDS by 1 + h %
 * (size - 2) slots modulo size until a free slot.  Records go in in record order and the image
 * depends on that order; the kernel builds it in parallel and gets the sequential result: every
 * slot keeps the lowest record ordinal that claimed it (an atomic min), an evicted record moves on
 * along its own probe sequence, a slot is never freed.  One workgroup per archive; the owner
 * table sits in LDS up to 15 360 slots (the reference's MAX_HM_SZ is about 8.5 K), above that
 * in d_slot_rec itself.
 * Also written: d_slot_rec[a * map_slots + s] = the record in slot s of archive a or
 * SDFS_CDC_ARCHIVE_NONE (compaction walks it); d_info[0] = records whose key equals that of an
 * earlier record of the same archive (the reference's HashExistsException, :1361-1363: a caller
 * bug here, the index never lists a digest as new twice; such a record gets no slot), d_info[1] =
 * archives with size[a] - 1 records or more (a table that cannot be probed: image left empty).
 * A key of hash_len zero bytes cannot be told from a free slot (the reference's FREE) and is not
 * looked at specially.
 * hash_len: 16 or 32.  20 is SDFS_CDC_EINVAL: for the *_160 engines the reference itself sets
 * HashFunctionPool.hashLength = 18 against a 20-byte hash, so its slots do not
 * hold the key; there is no image to reproduce. */
int sdfs_cdc_archive_map_emit(int device, const sdfs_cdc_archive_layout* layout, const uint32_t* d_count,
                              uint64_t n_max, const uint32_t* d_rec_len, const uint8_t* d_records,
                              const uint32_t* d_sel, uint32_t hash_len, uint32_t version,
                              const uint32_t* d_map_slots, uint32_t map_slots, uint8_t* d_maps,
                              uint32_t* d_slot_rec, uint64_t* d_info, void* stream);

/* What sdfs_cdc_archive_compact_select lays out for the surviving records (device arrays; n = the
 * old layout's records, n_arc = its archives).  lay: the new layout (arc_cap >= n_arc). */
typedef struct sdfs_cdc_archive_kept {
    uint32_t* new_of_old;  /* [n] the record's new ordinal, SDFS_CDC_ARCHIVE_NONE when dropped */
    uint32_t* sel;         /* [n] new record j's fingerprint record (for d_sel of pack / map_emit) */
    uint64_t* src_off;     /* [n] new record j's bytes in the OLD store */
    uint32_t* rec_len;     /* [n] their length */
    uint32_t* count;       /* [1] surviving records */
    uint8_t* deleted;      /* [n_arc] 1 = the old archive has no survivor and is gone */
    uint32_t* new_arc;     /* [n_arc] the old archive's new index, SDFS_CDC_ARCHIVE_NONE when deleted */
    uint32_t* map_slots;   /* [n_arc] new archive a's map size: map_size(2 * live + 5) */
    sdfs_cdc_archive_layout lay;
} sdfs_cdc_archive_kept;

/* HashBlobArchive.compact() (:2064-2186) for the n_arc archives of one call, first half: walk each
 * old map in slot order (SimpleByteArrayLongMap.next, :136-170: d_slot_rec, size d_old_map_slots[a]
 * or old_map_slots, row stride old_map_slots), keep the records whose d_keep[i] != 0 (:2105: the
 * keys the index still holds) and number them: old archive a's survivors, in ascending slot
 * order, become one new archive (the reference passes the old file length as blocksz, :2127-2128,
 * which the survivors cannot exceed before the last put); an archive without survivors is deleted
 * (:2121-2125) and absent from the output.  The new map size per archive, map_size(2 * live +
 * 5) (:2127), is computed on the device with the rule of sdfs_cdc_archive_map_size.  Then the new
 * layout with those cuts (the plan with fixed cuts).  d_old_sel: the d_sel the old images were
 * packed with (NULL: identity). */
int sdfs_cdc_archive_compact_select(int device, const sdfs_cdc_archive_layout* old_layout, uint64_t n,
                                    uint32_t n_arc, const uint32_t* d_old_rec_len, const uint32_t* d_old_sel,
                                    const uint32_t* d_slot_rec, const uint32_t* d_old_map_slots,
                                    uint32_t old_map_slots, const uint8_t* d_keep, uint32_t hash_len,
                                    uint32_t header_bytes, const sdfs_cdc_archive_kept* kept, void* stream);

/* The whole of compact(): compact_select, then sdfs_cdc_archive_pack of the survivors from the
 * old store into d_store (store_cap >= the old store_bytes always suffices) and
 * sdfs_cdc_archive_map_emit of the new maps (row stride new_map_stride slots, >= every new size:
 * map_size(2 * the largest old archive's records + 5) always suffices).
 * Without encryption this is a copy of the stored bytes: the reference's getChunk followed by
 * putChunk decodes and re-encodes each record, and both codecs are deterministic, so the bytes
 * come out as they went in.  With header_bytes != 0 the new archives have new IVs
 * (PassPhrase.getByteIV, :1028) and the records must be decrypted and encrypted again between
 * compact_select and pack: the caller runs the three steps itself (sdfs_amd.archive does). */
int sdfs_cdc_archive_compact(int device, const sdfs_cdc_archive_layout* old_layout, uint64_t n, uint32_t n_arc,
                             const uint8_t* d_old_store, const uint32_t* d_old_rec_len, const uint32_t* d_old_sel,
                             const uint32_t* d_slot_rec, const uint32_t* d_old_map_slots, uint32_t old_map_slots,
                             const uint8_t* d_keep, const uint8_t* d_records, uint32_t hash_len,
                             uint32_t header_bytes, uint32_t version, const uint8_t* d_ivs,
                             const sdfs_cdc_archive_kept* kept, uint8_t* d_store, uint64_t store_cap,
                             uint32_t new_map_stride, uint8_t* d_maps, uint32_t* d_slot_rec_new, uint64_t* d_info,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDFS_ARCHIVE_H */
