// store_format.h — the four on-disk formats of the store layer, each defined here and nowhere
// else (host + device).  Not part of the C-ABI.
//
//   slot image     SparseDataChunk.getBytes (SparseDataChunk.java:295-318, HashLocPair.asArray
//                  HashLocPair.java:49-59); written by map_emit.hip and map_merge.hip; accepted by
//                  slot_walk_check for read_path.hip, dedup_index.hip and map_import.hip
//   .map image     SimpleByteArrayLongMap's file (SimpleByteArrayLongMap.java:198-261,427-498,
//                  509-539); written by archive_pack.hip, read back by store_open.hip
//   archive record HashBlobArchive.putChunk (HashBlobArchive.java:1399-1411); laid out and packed by
//                  archive_pack.hip, checked by store_open.hip
//   LZ4Block stream a map file at rest, CompressionUtils.compressFile (CompressionUtils.java:127-139):
//                  lz4-java 1.3.0's LZ4BlockOutputStream; written and read by lz4_stream.hip
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "../../include/sdfs_archive.h"
#include "../../include/sdfs_lz4_stream.h"
#include "../../include/sdfs_read.h"

namespace sdfs {
namespace {  // internal linkage: nothing here joins the libraries' exported symbols

// ----------------------------------------------------------------------------------- byte order

__device__ __forceinline__ uint32_t get_be32(const uint8_t* p) {
    return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3];
}

__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

// byte k (0 = first in memory) of put_be32(v)
__device__ __forceinline__ uint32_t be32_byte(uint32_t v, uint32_t k) { return (v >> (8 * (3 - k))) & 255u; }

// ----------------------------------------------------------------------------------- slot image
//
// [flags][BE32 capacity][BE32 n] n x (hash | BE64 hashloc | BE32 len, pos, offset, nlen) [BE32 doop]

constexpr uint32_t kSlotHeaderBytes = 9;
constexpr uint32_t kSlotTrailerBytes = 4;
constexpr uint32_t kSlotFixedBytes = kSlotHeaderBytes + kSlotTrailerBytes;  // 13: an image with no pair
constexpr uint32_t kSlotCountAt = 5;      // BE32 n (ar.size())
// a pair's fields behind its hash
constexpr uint32_t kPairHashlocAt = 0, kPairLenAt = 8, kPairPosAt = 12, kPairOffsetAt = 16, kPairNlenAt = 20;

__host__ __device__ inline uint32_t pair_bytes(uint32_t hash_len) { return hash_len + 24; }

__host__ __device__ inline uint64_t slot_need(uint32_t n, uint32_t hash_len) {
    return (uint64_t)kSlotFixedBytes + (uint64_t)n * pair_bytes(hash_len);
}

__host__ __device__ inline uint32_t pair_cap(uint32_t slot_bytes, uint32_t hash_len) {
    return slot_bytes < kSlotFixedBytes ? 0 : (slot_bytes - kSlotFixedBytes) / pair_bytes(hash_len);
}

// pair i of the image (read or written)
template <typename B>
__device__ __forceinline__ B* slot_pair(B* img, uint32_t i, uint32_t hash_len) {
    return img + kSlotHeaderBytes + (uint64_t)i * pair_bytes(hash_len);
}

// the fields of pair i: kPair...At count from here
template <typename B>
__device__ __forceinline__ B* pair_fields(B* img, uint32_t i, uint32_t hash_len) {
    return slot_pair(img, i, hash_len) + hash_len;
}

// N 32-bit words from p, whatever its alignment: aligned loads realigned by a byte shift.  Every
// word loaded holds at least one of the bytes asked for.
template <int N>
__device__ __forceinline__ void load_words(const uint8_t* p, uint32_t (&w)[N]) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint32_t r = (uint32_t)(a & 3);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(a - r);
    uint32_t t[N + 1];
#pragma unroll
    for (int i = 0; i < N; i++) t[i] = q[i];
    t[N] = r ? q[N] : 0u;
#pragma unroll
    for (int i = 0; i < N; i++) w[i] = __builtin_amdgcn_alignbyte(t[i + 1], t[i], r);
}

// How an image is accepted (SparseDataChunk's constructor; one wave, every branch wave-uniform):
// zlen <= 0 holds no pairs; an image that needs more than slot_bytes is CORRUPT; a negative len,
// pos, offset or nlen is CORRUPT with no pairs (HashLocPair.checkCorrupt); unsorted = some pos is
// not above its predecessor's.  A lane loads a pos only for its own pairs and the ones before them.
struct SlotWalk {
    uint32_t status;  // 0 or SDFS_CDC_READ_CORRUPT
    uint32_t n;       // pairs to walk
    bool unsorted;    // only with n > 0
};

__device__ __forceinline__ SlotWalk slot_walk_check(const uint8_t* img, uint32_t slot_bytes, uint32_t hash_len,
                                                    uint32_t lane) {
    SlotWalk w{0, 0, false};
    const int32_t zlen = (int32_t)get_be32(img + kSlotCountAt);
    if (zlen > 0) {
        if (slot_need((uint32_t)zlen, hash_len) > slot_bytes) w.status = SDFS_CDC_READ_CORRUPT;  // BufferUnderflowException
        else w.n = (uint32_t)zlen;
    }
    bool neg = false, unsorted = false;
    for (uint32_t i = lane; i < w.n; i += 64) {
        const uint8_t* q = pair_fields(img, i, hash_len);
        const int32_t ps = (int32_t)get_be32(q + kPairPosAt);
        neg |= ((int32_t)get_be32(q + kPairLenAt) | ps | (int32_t)get_be32(q + kPairOffsetAt) |
                (int32_t)get_be32(q + kPairNlenAt)) < 0;
        if (i > 0) unsorted |= (int32_t)get_be32(pair_fields(img, i - 1, hash_len) + kPairPosAt) >= ps;
    }
    if (__ballot(neg) != 0) {
        w.status = SDFS_CDC_READ_CORRUPT;
        w.n = 0;
    }
    w.unsorted = w.n && __ballot(unsorted) != 0;
    return w;
}

// TreeMap.put per pair in image order: pair i of an unsorted image of n pairs does not count when
// a later pair has the same pos
__device__ __forceinline__ bool pair_superseded(const uint8_t* img, uint32_t i, uint32_t n, uint32_t hash_len) {
    const uint32_t ps = get_be32(pair_fields(img, i, hash_len) + kPairPosAt);
    bool dead = false;
    for (uint32_t j = i + 1; j < n; j++) dead |= get_be32(pair_fields(img, j, hash_len) + kPairPosAt) == ps;
    return dead;
}

// The hash of pair i as two key words (kb zero for HW = 4) and its BE64 hashloc, by aligned loads
// (pairs start at odd byte offsets).  HW: words of a pair's hash (8 = SHA-256, 4 = MD5).
template <int HW>
__device__ __forceinline__ void load_pair_key(const uint8_t* img, uint32_t i, uint4& ka, uint4& kb, uint64_t& hashloc) {
    uint32_t w[HW + 2];  // hash | BE64 hashloc
    load_words(slot_pair(img, i, HW * 4), w);
    ka = make_uint4(w[0], w[1], w[2], w[3]);
    kb = HW == 8 ? make_uint4(w[HW - 4], w[HW - 3], w[HW - 2], w[HW - 1]) : make_uint4(0, 0, 0, 0);
    hashloc = (uint64_t)__builtin_bswap32(w[HW]) << 32 | __builtin_bswap32(w[HW + 1]);
}

// What a walk keeps per image between its check and its passes over the pairs: n, and the unsorted
// flag.  A wave of such a pass takes kSlotPart pairs of one image.
constexpr uint32_t kSlotUnsorted = 0x80000000u;
constexpr uint32_t kSlotPart = 256;

__device__ __forceinline__ uint32_t slot_meta(const SlotWalk& w) { return w.n | (w.unsorted ? kSlotUnsorted : 0u); }
__device__ __forceinline__ uint32_t slot_meta_pairs(uint32_t meta) { return meta & ~kSlotUnsorted; }
__device__ __forceinline__ bool slot_meta_unsorted(uint32_t meta) { return (meta & kSlotUnsorted) != 0; }

__host__ __device__ inline uint32_t slot_parts(uint32_t pairs) { return (pairs + kSlotPart - 1) / kSlotPart; }

// pair i from its six fields (byte stores: records start at odd offsets)
__device__ __forceinline__ void put_pair_record(uint8_t* img, uint32_t i, uint32_t hash_len, const uint8_t* hash,
                                                uint64_t hashloc, uint32_t len, uint32_t pos, uint32_t offset,
                                                uint32_t nlen) {
    uint8_t* p = slot_pair(img, i, hash_len);
    for (uint32_t k = 0; k < hash_len; k++) p[k] = hash[k];
    p += hash_len;
    put_be32(p + kPairHashlocAt, (uint32_t)(hashloc >> 32));  // hashloc = Longs.toByteArray(pos)
    put_be32(p + kPairHashlocAt + 4, (uint32_t)hashloc);
    put_be32(p + kPairLenAt, len);
    put_be32(p + kPairPosAt, pos);
    put_be32(p + kPairOffsetAt, offset);
    put_be32(p + kPairNlenAt, nlen);
}

// header and trailer of an image of n pairs
__device__ __forceinline__ void put_slot_frame(uint8_t* img, uint8_t flags, uint32_t n, uint32_t hash_len,
                                               uint32_t doop) {
    img[0] = flags;
    put_be32(img + 1, (uint32_t)slot_need(n, hash_len));  // buf.capacity()
    put_be32(img + kSlotCountAt, n);                      // ar.size()
    put_be32(slot_pair(img, n, hash_len), doop);
}

// ----------------------------------------------------------------------------------- .map image
//
// VERSION > 0: a 16-byte header [BE32 magic][BE32 version][8 x 0]; then `size` entries of
// hash | BE32 pos (VERSION 0) or hash | BE32 pos | BE32 len.  An entry whose hash is all zero is
// free.  A key's home is h % size with h = map_key_hash(key); a collision walks idx - step with
// wrap, step = 1 + h % (size - 2).

constexpr uint32_t kMapHeaderBytes = 16;
constexpr uint32_t kMapVersionAt = 4;               // BE32 version in the header
constexpr uint32_t kMapPosAt = 0, kMapLenAt = 4;  // an entry's value fields behind its hash

// NextPrime.getNextPrimeI (NextPrime.java:56-88)
__host__ __device__ inline uint32_t map_size_rule(uint64_t sz) {
    if (sz <= 2) return 2;
    for (uint32_t k = 3; k < 9; k += 2)
        if (sz <= k) return k;
    if (sz > (uint64_t)INT32_MAX) return 0;  // the next prime would pass Integer.MAX_VALUE (itself prime)
    if ((sz & 1) == 0) sz += 1;
    for (uint64_t i = sz;; i += 2) {
        bool prime = true;
        for (uint64_t j = 3; j * j <= i; j += 2)
            if (i % j == 0) {
                prime = false;
                break;
            }
        if (prime) return (uint32_t)i;
    }
}

__host__ __device__ inline uint32_t map_header_bytes(uint32_t version) { return version ? kMapHeaderBytes : 0u; }

__host__ __device__ inline uint32_t map_entry_bytes(uint32_t hash_len, uint32_t version) {
    return hash_len + (version ? 8u : 4u);
}

__host__ __device__ inline uint64_t map_image_bytes(uint32_t slots, uint32_t hash_len, uint32_t version) {
    return map_header_bytes(version) + (uint64_t)slots * map_entry_bytes(hash_len, version);
}

__device__ __forceinline__ bool map_has_magic(const uint8_t* map) {
    return get_be32(map) == SDFS_CDC_ARCHIVE_MAP_MAGIC;
}

__device__ __forceinline__ uint32_t map_key_hash(const uint8_t* key) { return get_be32(key + 8) & 0x7fffffffu; }

__device__ __forceinline__ uint32_t map_probe_home(uint32_t h, uint32_t size) { return h % size; }

// size >= 3 (a map a writer fills)
__device__ __forceinline__ uint32_t map_probe_step(uint32_t h, uint32_t size) { return 1 + h % (size - 2); }

// a map of any size read back; 0 for size <= 2: such a map holds a key in its home slot only
__device__ __forceinline__ uint32_t map_probe_step_any(uint32_t h, uint32_t size) {
    return size > 2 ? map_probe_step(h, size) : 0;
}

__device__ __forceinline__ uint32_t map_probe_next(uint32_t idx, uint32_t step, uint32_t size) {
    return idx >= step ? idx - step : idx + size - step;
}

// ------------------------------------------------------------------------------- archive record
//
// [BE32 hash_len][hash][BE32 len][record]: a record's position (layout pos, store_off) is that of
// its first byte; the header lies before it, the length word last.  The .map value of a record is
// the position of its length word.

constexpr uint32_t kRecordLenBack = 4;  // the length word starts this far before the record's first byte

__host__ __device__ inline uint32_t record_header_bytes(uint32_t hash_len) { return 8 + hash_len; }

// ------------------------------------------------------------------------------ LZ4Block stream
//
// Per block "LZ4Block" | token | LE32 compressedLen | LE32 originalLen | LE32 check | payload, with
// token = method | level; after the last block an end mark: method RAW and three zero ints
// (LZ4BlockOutputStream.flushBufferedData / finish).  The flag values of a reader's status word
// are the C-ABI's SDFS_CDC_LZ4_STREAM_*.

constexpr uint32_t kStreamHeaderBytes = SDFS_CDC_LZ4_STREAM_HEADER_BYTES;
constexpr uint32_t kStreamMagicBytes = 8;
constexpr uint32_t kStreamTokenAt = 8, kStreamCompressedLenAt = 9, kStreamOriginalLenAt = 13, kStreamCheckAt = 17;
constexpr uint32_t kStreamLevelBase = 10;           // COMPRESSION_LEVEL_BASE: a block holds up to 1 << (10 + level)
constexpr uint32_t kStreamCheckMask = 0x0FFFFFFFu;  // StreamingXXHash32.asChecksum keeps 28 bits

// byte k of the magic
__host__ __device__ inline uint8_t stream_magic_byte(uint32_t k) {
    constexpr char m[kStreamMagicBytes + 1] = "LZ4Block";
    return (uint8_t)m[k];
}

__host__ __device__ inline bool stream_block_size_ok(uint32_t block_size) {
    return block_size >= SDFS_CDC_LZ4_STREAM_MIN_BLOCK && block_size <= SDFS_CDC_LZ4_STREAM_MAX_BLOCK;
}

// LZ4BlockOutputStream.compressionLevel: max(0, 32 - numberOfLeadingZeros(blockSize - 1) - 10)
__host__ __device__ inline uint32_t stream_level(uint32_t block_size) {
    uint32_t bits = 0;
    for (uint32_t v = block_size - 1; v; v >>= 1) bits++;
    return bits > kStreamLevelBase ? bits - kStreamLevelBase : 0;
}

// the writer's choice: the LZ4 block only when it is shorter than the data
__host__ __device__ inline bool stream_stores_raw(uint32_t lz4_len, uint32_t original_len) {
    return lz4_len >= original_len;
}

__host__ __device__ inline uint64_t stream_blocks_of(uint64_t n, uint32_t block_size) {
    return (n + block_size - 1) / block_size;
}

__host__ __device__ inline uint64_t stream_bound(uint64_t n, uint32_t block_size) {
    return n + (uint64_t)kStreamHeaderBytes * (stream_blocks_of(n, block_size) + 1);
}

// a data block is a header and at least one payload byte
__host__ __device__ inline uint64_t stream_max_blocks(uint64_t file_len) { return file_len / (kStreamHeaderBytes + 1) + 1; }

__device__ __forceinline__ uint32_t get_le32(const uint8_t* p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// byte k of a header (k < 21)
__device__ __forceinline__ uint8_t stream_header_byte(uint32_t k, uint32_t token, uint32_t compressed_len,
                                                      uint32_t original_len, uint32_t check) {
    if (k < kStreamMagicBytes) return stream_magic_byte(k);
    if (k == kStreamTokenAt) return (uint8_t)token;
    const uint32_t v = k < kStreamOriginalLenAt ? compressed_len : k < kStreamCheckAt ? original_len : check;
    return (uint8_t)(v >> (8 * ((k - kStreamCompressedLenAt) & 3)));
}

// What LZ4BlockInputStream.refill decides from a header it has read whole: 0 = a data block,
// MAGIC / HEADER = refused; *end_mark = the stream ends here.  Nothing of the payload is looked at.
__device__ __forceinline__ uint32_t stream_header_check(const uint8_t* h, uint32_t* token, int32_t* compressed_len,
                                                        int32_t* original_len, uint32_t* check, bool* end_mark) {
    *end_mark = false;
    for (uint32_t k = 0; k < kStreamMagicBytes; k++)
        if (h[k] != stream_magic_byte(k)) return SDFS_CDC_LZ4_STREAM_MAGIC;
    const uint32_t t = h[kStreamTokenAt], method = t & 0xF0u, level = t & 0x0Fu;
    const int32_t cl = (int32_t)get_le32(h + kStreamCompressedLenAt), ol = (int32_t)get_le32(h + kStreamOriginalLenAt);
    const uint32_t ck = get_le32(h + kStreamCheckAt);
    *token = t;
    *compressed_len = cl;
    *original_len = ol;
    *check = ck;
    if (method != SDFS_CDC_LZ4_STREAM_RAW && method != SDFS_CDC_LZ4_STREAM_LZ4) return SDFS_CDC_LZ4_STREAM_HEADER;
    if ((int64_t)ol > ((int64_t)1 << (kStreamLevelBase + level)) || ol < 0 || cl < 0 || (ol == 0) != (cl == 0) ||
        (method == SDFS_CDC_LZ4_STREAM_RAW && ol != cl))
        return SDFS_CDC_LZ4_STREAM_HEADER;
    if (ol == 0) {  // and cl == 0
        if (ck != 0) return SDFS_CDC_LZ4_STREAM_HEADER;
        *end_mark = true;
    }
    return 0;
}

}  // namespace
}  // namespace sdfs
