// lz4_stream.hip — map files at rest: the LZ4Block stream (GUID.map.lz4) written and read on the
// MI355X (include/sdfs_lz4_stream.h; the format lives in store_format.h).
//
// Reference: CompressionUtils.compressFile / decompressFile (CompressionUtils.java:127-151) =
// lz4-java 1.3.0's LZ4BlockOutputStream(fos, 1 << 16, lz4Compressor) / LZ4BlockInputStream, which
// LongByteArrayMap.close (:1003-1015), copy (:937-938), the map's open (:141-154) and the cloud
// stores' map uploads and fetches run over whole map files.
//
// Writing is five launches behind one another, no host wait: the block list of all files, the LZ4
// block kernels of lz4_kernels.hip over it (unframed, into bound-spaced scratch), XXH32 of the
// source blocks, an exclusive scan of 21 + min(compressed, original), and one pack kernel that
// writes headers and end marks and copies each payload (the LZ4 block, or the data itself when LZ4
// did not shorten it).  Reading: a header walk per file (a dependent chain: where block k + 1
// starts is written in block k's header, so one lane of one wave follows it and every step is
// bounds-checked against the file's end before it is used), then the located blocks of all files
// as one batch: LZ4 blocks through the bounded decoder of lz4_kernels.hip, RAW blocks through a
// copy, XXH32 of the decoded bytes against the stored int; a file's first bad block decides its
// status word.
//
// XXH32 is the one per-byte loop that is new here: four independent accumulators over 16-byte
// stripes, each a multiply-rotate-multiply chain.  Four lanes share an extent, one accumulator
// each (16 extents per wave, one dword load per lane and stripe), and are combined by two
// butterfly shuffles; the tail of < 16 bytes and the avalanche are one lane's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/sdfs_lz4_stream.h"
#include "block_scan.h"
#include "call_support.h"
#include "store_format.h"

namespace sdfs {
namespace {

// ------------------------------------------------------------------------------------ plumbing

// host words to device memory in stream order, as kernel arguments (no pageable-memory copy, no wait)
constexpr uint32_t kWordsPerLaunch = 64;
struct WordArgs {
    uint64_t* dst;
    uint32_t n;
    uint64_t v[kWordsPerLaunch];
};

__global__ __launch_bounds__(64) void lz4s_words_kernel(WordArgs a) {
    if (threadIdx.x < a.n) a.dst[threadIdx.x] = a.v[threadIdx.x];
}

hipError_t upload_words(const std::vector<uint64_t>& w, uint64_t* dst, hipStream_t s) {
    for (size_t i0 = 0; i0 < w.size(); i0 += kWordsPerLaunch) {
        WordArgs a;
        a.dst = dst + i0;
        a.n = (uint32_t)std::min<size_t>(kWordsPerLaunch, w.size() - i0);
        for (uint32_t i = 0; i < kWordsPerLaunch; i++) a.v[i] = i < a.n ? w[i0 + i] : 0;
        hipLaunchKernelGGL(lz4s_words_kernel, dim3(1), dim3(64), 0, s, a);
    }
    return hipGetLastError();
}

// one stream-ordered allocation cut into 16-byte aligned arrays
struct Carve {
    size_t bytes = 0;
    uint8_t* base = nullptr;
    template <typename T>
    size_t add(size_t count) {
        const size_t at = bytes;
        bytes += (std::max<size_t>(count, 1) * sizeof(T) + 15) & ~(size_t)15;
        return at;
    }
    template <typename T>
    T* at(size_t off) const {
        return reinterpret_cast<T*>(base + off);
    }
};

// the 256 threads of a workgroup copy n bytes; dst and src at any byte
__device__ __forceinline__ void block_copy_256(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint64_t n) {
    const uint32_t t = threadIdx.x;
    const uint64_t head = min<uint64_t>((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15, n);
    if (t < head) dst[t] = src[t];
    const uint64_t nv = (n - head) >> 4;
    for (uint64_t k = t; k < nv; k += 256) {
        uint4 v;
        __builtin_memcpy(&v, src + head + 16 * k, 16);
        *reinterpret_cast<uint4*>(dst + head + 16 * k) = v;
    }
    for (uint64_t b = head + (nv << 4) + t; b < n; b += 256) dst[b] = src[b];
}

// --------------------------------------------------------------------------------------- XXH32

constexpr uint32_t kP1 = 2654435761u, kP2 = 2246822519u, kP3 = 3266489917u, kP4 = 668265263u, kP5 = 374761393u;
constexpr uint32_t kXxhExtentsPerBlock = 64;  // 256 threads, four per extent

struct XxhArgs {
    const uint8_t* data;
    const uint64_t* off;
    const uint32_t* len;
    const uint32_t* count;
    uint64_t n_max;
    uint32_t seed;
    uint32_t* out;
};

__device__ __forceinline__ uint32_t ld32u(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

__device__ __forceinline__ uint32_t xxh_round(uint32_t acc, uint32_t w) {
    return __builtin_rotateleft32(acc + w * kP2, 13) * kP1;
}

__global__ __launch_bounds__(256) void xxh32_kernel(XxhArgs a) {
    const uint64_t n = live_count(a.count, a.n_max);
    const uint32_t q = threadIdx.x & 3;  // this lane's accumulator
    const uint32_t rot = q == 0 ? 1 : q == 1 ? 7 : q == 2 ? 12 : 18;
    const uint32_t init = a.seed + (q == 0 ? kP1 + kP2 : q == 1 ? kP2 : q == 2 ? 0u : 0u - kP1);
    // every lane of a workgroup makes the same number of trips, so the shuffles below see whole waves
    for (uint64_t i0 = (uint64_t)blockIdx.x * kXxhExtentsPerBlock; i0 < n; i0 += (uint64_t)gridDim.x * kXxhExtentsPerBlock) {
        const uint64_t i = i0 + (threadIdx.x >> 2);
        const bool live = i < n;
        const uint32_t len = live ? a.len[i] : 0;
        const uint8_t* p = a.data + (live ? a.off[i] : 0);
        const uint32_t stripes = len >> 4;
        uint32_t acc = init;
        const uint8_t* s = p + 4 * q;
        // an extent has a quarter of one wave to itself: its own four loads in flight are all that
        // hides memory latency here (DESIGN.md §21 has what that costs)
#pragma unroll 4
        for (uint32_t k = 0; k < stripes; k++) acc = xxh_round(acc, ld32u(s + 16ull * k));
        uint32_t h = __builtin_rotateleft32(acc, rot);
        h += __shfl_xor(h, 1);
        h += __shfl_xor(h, 2);
        if (q == 0 && live) {
            if (!stripes) h = a.seed + kP5;
            h += len;
            uint32_t b = stripes << 4;
            for (; b + 4 <= len; b += 4) h = __builtin_rotateleft32(h + ld32u(p + b) * kP3, 17) * kP4;
            for (; b < len; b++) h = __builtin_rotateleft32(h + p[b] * kP5, 11) * kP1;
            h ^= h >> 15;
            h *= kP2;
            h ^= h >> 13;
            h *= kP3;
            h ^= h >> 16;
            a.out[i] = h;
        }
    }
}

hipError_t launch_xxh32(const XxhArgs& a, hipStream_t s) {
    if (a.n_max == 0) return hipSuccess;
    const uint64_t grid = std::min<uint64_t>((a.n_max + kXxhExtentsPerBlock - 1) / kXxhExtentsPerBlock, 1u << 16);
    hipLaunchKernelGGL(xxh32_kernel, dim3((uint32_t)grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------- the writer

struct WriteArgs {
    const uint8_t* data;
    // per file (device copies of the host arrays): extent, output offset, first block ([n_files + 1])
    const uint64_t* file_off;
    const uint64_t* file_len;
    const uint64_t* out_off;
    const uint64_t* base;
    uint32_t n_files;
    uint32_t block_size;
    uint32_t level;
    uint32_t nb;       // blocks of all files
    uint64_t lz_room;  // spacing of the LZ4 blocks in tmp
    // per block
    uint64_t* src_off;
    uint32_t* src_len;
    uint64_t* tmp_off;
    uint32_t* lz_len;
    uint32_t* sum;
    uint64_t* size;  // 21 + payload
    uint64_t* pos;   // exclusive scan of size, [nb + 1]
    const uint8_t* tmp;
    uint8_t* out;
    uint64_t* out_len;
};

__device__ __forceinline__ uint32_t file_of_block(const uint64_t* base, uint32_t n_files, uint64_t g) {
    return (uint32_t)floor_index<uint64_t>(base, (int32_t)n_files, g, -2);
}

__global__ __launch_bounds__(256) void lz4s_block_list_kernel(WriteArgs a) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= a.nb) return;
    const uint32_t f = file_of_block(a.base, a.n_files, g);
    const uint64_t at = (uint64_t)(g - a.base[f]) * a.block_size;
    a.src_off[g] = a.file_off[f] + at;
    a.src_len[g] = (uint32_t)min<uint64_t>(a.block_size, a.file_len[f] - at);
    a.tmp_off[g] = (uint64_t)g * a.lz_room;
}

__global__ __launch_bounds__(256) void lz4s_size_kernel(WriteArgs a) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= a.nb) return;
    const uint32_t len = a.src_len[g], cl = a.lz_len[g];
    a.size[g] = kStreamHeaderBytes + (stream_stores_raw(cl, len) ? len : cl);
}

// workgroup b < nb: block b's header and payload; workgroup nb + f: file f's end mark and length
__global__ __launch_bounds__(256) void lz4s_pack_kernel(WriteArgs a) {
    const uint32_t b = blockIdx.x, t = threadIdx.x;
    if (b >= a.nb) {
        const uint32_t f = b - a.nb;
        const uint64_t end = a.pos[a.base[f + 1]] - a.pos[a.base[f]];
        uint8_t* dst = a.out + a.out_off[f] + end;
        if (t < kStreamHeaderBytes) dst[t] = stream_header_byte(t, SDFS_CDC_LZ4_STREAM_RAW | a.level, 0, 0, 0);
        if (t == 0) a.out_len[f] = end + kStreamHeaderBytes;
        return;
    }
    const uint32_t f = file_of_block(a.base, a.n_files, b);
    uint8_t* dst = a.out + a.out_off[f] + (a.pos[b] - a.pos[a.base[f]]);
    const uint32_t len = a.src_len[b], cl = a.lz_len[b];
    const bool raw = stream_stores_raw(cl, len);
    const uint32_t pl = raw ? len : cl;
    if (t < kStreamHeaderBytes)
        dst[t] = stream_header_byte(t, (raw ? SDFS_CDC_LZ4_STREAM_RAW : SDFS_CDC_LZ4_STREAM_LZ4) | a.level, pl, len,
                                    a.sum[b] & kStreamCheckMask);
    block_copy_256(dst + kStreamHeaderBytes, raw ? a.data + a.src_off[b] : a.tmp + a.tmp_off[b], pl);
}

// ---------------------------------------------------------------------------------- the reader

struct WalkArgs {
    const uint8_t* data;
    const uint64_t* file_off;
    const uint64_t* file_len;
    const uint64_t* table_base;
    uint32_t n_files;
    sdfs_cdc_lz4_stream_file* files;
    sdfs_cdc_lz4_stream_block* blocks;
};

// One wave per file, the chain followed by lane 0: block k + 1 is found only through block k's
// header.  `left` is what the file still holds from the current position: nothing is read or
// trusted beyond it.
__global__ __launch_bounds__(64) void lz4s_walk_kernel(WalkArgs a) {
    if (threadIdx.x != 0) return;
    const uint32_t f = blockIdx.x;
    const uint64_t flen = a.file_len[f], foff = a.file_off[f];
    const uint64_t cap = stream_max_blocks(flen);
    sdfs_cdc_lz4_stream_block* table = a.blocks + a.table_base[f];
    uint64_t pos = 0, decoded = 0;
    uint32_t nb = 0, status = 0;
    for (;;) {
        if (flen - pos < kStreamHeaderBytes) {
            status = SDFS_CDC_LZ4_STREAM_TRUNCATED;
            break;
        }
        uint8_t h[kStreamHeaderBytes];
#pragma unroll
        for (uint32_t k = 0; k < kStreamHeaderBytes; k++) h[k] = a.data[foff + pos + k];
        uint32_t token, check;
        int32_t cl, ol;
        bool end_mark;
        status = stream_header_check(h, &token, &cl, &ol, &check, &end_mark);
        if (status) break;
        if (end_mark) {
            pos += kStreamHeaderBytes;
            break;
        }
        // cap cannot be reached by blocks that lie inside the file (22 bytes each at least)
        if ((uint64_t)cl > flen - pos - kStreamHeaderBytes || nb >= cap) {
            status = SDFS_CDC_LZ4_STREAM_TRUNCATED;
            break;
        }
        table[nb] = sdfs_cdc_lz4_stream_block{foff + pos + kStreamHeaderBytes, (uint32_t)cl, (uint32_t)ol, token & 0xF0u,
                                              check, decoded};
        nb++;
        decoded += (uint32_t)ol;
        pos += kStreamHeaderBytes + (uint64_t)cl;
    }
    a.files[f] = sdfs_cdc_lz4_stream_file{status, nb, decoded, pos};
}

struct ReadArgs {
    const uint8_t* data;
    const uint64_t* table_base;
    const uint64_t* out_off;
    const uint64_t* out_cap;
    uint32_t n_files;
    uint64_t max_blocks;
    sdfs_cdc_lz4_stream_file* files;
    const sdfs_cdc_lz4_stream_block* blocks;
    uint8_t* out;
    uint32_t* cnt;    // [n_files] blocks of the files that are decoded
    uint32_t* first;  // [n_files + 1] exclusive scan of cnt
    uint32_t* count;  // [1] blocks in the list
    // per listed block
    uint64_t* src_off;
    uint32_t* lz_len;  // 0 = a RAW block: the LZ4 decoder takes nothing from it
    uint64_t* dst_off;
    uint32_t* dst_cap;
    uint32_t* got;
    uint32_t* sum;
    uint32_t* check;
    uint32_t* file;
    unsigned long long* bad;  // [n_files] (block index << 8 | flags) of a file's first bad block
};

__global__ __launch_bounds__(256) void lz4s_read_count_kernel(ReadArgs a) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f >= a.n_files) return;
    const sdfs_cdc_lz4_stream_file s = a.files[f];
    // the blocks located before a bad header are decoded too: Java reads them before it meets it
    bool take = true;
    if (s.decoded_len > a.out_cap[f]) {
        a.files[f].status = s.status | SDFS_CDC_LZ4_STREAM_ROOM;
        take = false;
    }
    a.cnt[f] = take ? s.n_blocks : 0;
}

// a file whose blocks do not all fit the list is not decoded whole: ROOM
__global__ __launch_bounds__(256) void lz4s_read_room_kernel(ReadArgs a) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f == 0) *a.count = (uint32_t)min<uint64_t>(a.first[a.n_files], a.max_blocks);
    if (f >= a.n_files) return;
    if (a.cnt[f] && a.first[f + 1] > a.max_blocks) a.files[f].status |= SDFS_CDC_LZ4_STREAM_ROOM;
}

__global__ __launch_bounds__(256) void lz4s_read_list_kernel(ReadArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= min<uint64_t>(a.first[a.n_files], a.max_blocks)) return;
    const uint32_t f = (uint32_t)floor_index<uint32_t>(a.first, (int32_t)a.n_files, (uint32_t)i, -2);
    const sdfs_cdc_lz4_stream_block e = a.blocks[a.table_base[f] + (i - a.first[f])];
    a.src_off[i] = e.payload_off;
    a.lz_len[i] = e.method == SDFS_CDC_LZ4_STREAM_LZ4 ? e.compressed_len : 0;
    a.dst_off[i] = a.out_off[f] + e.decoded_off;
    a.dst_cap[i] = e.original_len;
    a.check[i] = e.check;
    a.file[i] = f;
}

__global__ __launch_bounds__(256) void lz4s_raw_copy_kernel(ReadArgs a) {
    const uint32_t n = *a.count;
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x)
        if (a.lz_len[i] == 0) block_copy_256(a.out + a.dst_off[i], a.data + a.src_off[i], a.dst_cap[i]);
}

__global__ __launch_bounds__(256) void lz4s_verify_kernel(ReadArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= *a.count) return;
    uint32_t flag = 0;
    if (a.lz_len[i] && a.got[i] != a.dst_cap[i]) flag = SDFS_CDC_LZ4_STREAM_DECODE;
    else if ((a.sum[i] & kStreamCheckMask) != a.check[i]) flag = SDFS_CDC_LZ4_STREAM_CHECKSUM;
    const uint32_t f = a.file[i];
    if (flag) atomicMin(&a.bad[f], (unsigned long long)(i - a.first[f]) << 8 | flag);
}

__global__ __launch_bounds__(256) void lz4s_read_status_kernel(ReadArgs a) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f >= a.n_files) return;
    const unsigned long long b = a.bad[f];
    // a located block comes before the block the header walk stopped at: it is the first bad one
    if (b != ~0ull) a.files[f].status = (a.files[f].status & SDFS_CDC_LZ4_STREAM_ROOM) | (uint32_t)(b & 0xFF);
}

int device_of(const void* p) {
    hipPointerAttribute_t at;
    const hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail_status(SDFS_CDC_EINVAL, "not a device pointer: %s", hipGetErrorString(e));
    }
    return set_device(at.device);
}

uint32_t grid256(uint64_t n) { return (uint32_t)((std::max<uint64_t>(n, 1) + 255) / 256); }

}  // namespace
}  // namespace sdfs

using namespace sdfs;

extern "C" {

int sdfs_cdc_lz4_stream_level(uint32_t block_size) {
    return stream_block_size_ok(block_size) ? (int)stream_level(block_size) : -1;
}

uint64_t sdfs_cdc_lz4_stream_bound(uint64_t n, uint32_t block_size) {
    return stream_block_size_ok(block_size) ? stream_bound(n, block_size) : 0;
}

uint64_t sdfs_cdc_lz4_stream_max_blocks(uint64_t file_len) { return stream_max_blocks(file_len); }

int sdfs_cdc_xxh32_device(sdfs_cdc_lz4* z, const uint8_t* d_data, const uint64_t* d_off, const uint32_t* d_len,
                          const uint32_t* d_count, uint64_t n_max, uint32_t seed, uint32_t* d_out, void* stream) {
    if (!z) return fail_status(SDFS_CDC_EINVAL, "null compressor");
    if (n_max == 0) return SDFS_CDC_OK;
    if (!d_data || !d_off || !d_len || !d_out) return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (const int rc = device_of(d_out)) return rc;
    SDFS_TRY(launch_xxh32(XxhArgs{d_data, d_off, d_len, d_count, n_max, seed, d_out}, reinterpret_cast<hipStream_t>(stream)));
    return SDFS_CDC_OK;
}

int sdfs_cdc_lz4_stream_compress_device(sdfs_cdc_lz4* z, const uint8_t* d_data, const uint64_t* file_off,
                                        const uint64_t* file_len, uint32_t n_files, uint32_t block_size,
                                        uint8_t* d_out, const uint64_t* out_off, uint64_t* d_out_len, void* stream) {
    if (!z) return fail_status(SDFS_CDC_EINVAL, "null compressor");
    if (!stream_block_size_ok(block_size))
        return fail_status(SDFS_CDC_EINVAL, "block_size %u: %u .. %u (LZ4BlockOutputStream)", block_size,
                           SDFS_CDC_LZ4_STREAM_MIN_BLOCK, SDFS_CDC_LZ4_STREAM_MAX_BLOCK);
    if (n_files == 0) return SDFS_CDC_OK;
    if (!d_data || !file_off || !file_len || !d_out || !out_off || !d_out_len)
        return fail_status(SDFS_CDC_EINVAL, "null argument");
    // device copies of the host arrays: file_off, file_len, out_off, base[n_files + 1]
    const size_t nf = n_files;
    std::vector<uint64_t> meta(4 * nf + 1);
    uint64_t nb = 0;
    for (size_t f = 0; f < nf; f++) {
        meta[f] = file_off[f];
        meta[nf + f] = file_len[f];
        meta[2 * nf + f] = out_off[f];
        meta[3 * nf + f] = nb;
        nb += stream_blocks_of(file_len[f], block_size);
        if (nb >= (uint64_t)INT32_MAX)
            return fail_status(SDFS_CDC_EINVAL, "%llu blocks and more: block ordinals are 31-bit", (unsigned long long)nb);
    }
    meta[4 * nf] = nb;
    if (const int rc = device_of(d_out_len)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint64_t lz_room = sdfs_cdc_lz4_bound(block_size);
    Carve c;
    const size_t o_meta = c.add<uint64_t>(meta.size()), o_src = c.add<uint64_t>(nb), o_tmpo = c.add<uint64_t>(nb),
                 o_size = c.add<uint64_t>(nb), o_pos = c.add<uint64_t>(nb + 1), o_len = c.add<uint32_t>(nb),
                 o_lz = c.add<uint32_t>(nb), o_sum = c.add<uint32_t>(nb), o_tmp = c.add<uint8_t>(nb * lz_room);
    Scratch sc(s);
    SDFS_TRY(sc.get(&c.base, c.bytes));
    uint64_t* d_meta = c.at<uint64_t>(o_meta);
    SDFS_TRY(upload_words(meta, d_meta, s));
    WriteArgs a{};
    a.data = d_data;
    a.file_off = d_meta;
    a.file_len = d_meta + nf;
    a.out_off = d_meta + 2 * nf;
    a.base = d_meta + 3 * nf;
    a.n_files = n_files;
    a.block_size = block_size;
    a.level = stream_level(block_size);
    a.nb = (uint32_t)nb;
    a.lz_room = lz_room;
    a.src_off = c.at<uint64_t>(o_src);
    a.src_len = c.at<uint32_t>(o_len);
    a.tmp_off = c.at<uint64_t>(o_tmpo);
    a.lz_len = c.at<uint32_t>(o_lz);
    a.sum = c.at<uint32_t>(o_sum);
    a.size = c.at<uint64_t>(o_size);
    a.pos = c.at<uint64_t>(o_pos);
    a.tmp = c.at<uint8_t>(o_tmp);
    a.out = d_out;
    a.out_len = d_out_len;
    if (nb) {
        hipLaunchKernelGGL(lz4s_block_list_kernel, dim3(grid256(nb)), dim3(256), 0, s, a);
        SDFS_TRY(hipGetLastError());
        if (const int rc = sdfs_cdc_lz4_compress_device(z, d_data, a.src_off, a.src_len, nullptr, nb, c.at<uint8_t>(o_tmp),
                                                        a.tmp_off, a.lz_len, 0, stream))
            return rc;
        SDFS_TRY(launch_xxh32(XxhArgs{d_data, a.src_off, a.src_len, nullptr, nb, SDFS_CDC_LZ4_STREAM_SEED, a.sum}, s));
        hipLaunchKernelGGL(lz4s_size_kernel, dim3(grid256(nb)), dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(prefix_kernel<uint64_t>, dim3(1), dim3(1024), 0, s, a.size, a.nb, a.pos);
    hipLaunchKernelGGL(lz4s_pack_kernel, dim3(a.nb + n_files), dim3(256), 0, s, a);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_lz4_stream_scan_device(sdfs_cdc_lz4* z, const uint8_t* d_data, const uint64_t* file_off,
                                    const uint64_t* file_len, uint32_t n_files, sdfs_cdc_lz4_stream_file* d_files,
                                    sdfs_cdc_lz4_stream_block* d_blocks, const uint64_t* table_base, void* stream) {
    if (!z) return fail_status(SDFS_CDC_EINVAL, "null compressor");
    if (n_files == 0) return SDFS_CDC_OK;
    if (!d_data || !file_off || !file_len || !d_files || !d_blocks || !table_base)
        return fail_status(SDFS_CDC_EINVAL, "null argument");
    const size_t nf = n_files;
    std::vector<uint64_t> meta(3 * nf);
    for (size_t f = 0; f < nf; f++) {
        meta[f] = file_off[f];
        meta[nf + f] = file_len[f];
        meta[2 * nf + f] = table_base[f];
    }
    if (const int rc = device_of(d_files)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    Scratch sc(s);
    uint64_t* d_meta = nullptr;
    SDFS_TRY(sc.get(&d_meta, meta.size()));
    SDFS_TRY(upload_words(meta, d_meta, s));
    hipLaunchKernelGGL(lz4s_walk_kernel, dim3(n_files), dim3(64), 0, s,
                       WalkArgs{d_data, d_meta, d_meta + nf, d_meta + 2 * nf, n_files, d_files, d_blocks});
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_lz4_stream_decompress_device(sdfs_cdc_lz4* z, const uint8_t* d_data, uint32_t n_files,
                                          sdfs_cdc_lz4_stream_file* d_files, const sdfs_cdc_lz4_stream_block* d_blocks,
                                          const uint64_t* table_base, uint64_t max_blocks, uint8_t* d_out,
                                          const uint64_t* out_off, const uint64_t* out_cap, void* stream) {
    if (!z) return fail_status(SDFS_CDC_EINVAL, "null compressor");
    if (n_files == 0) return SDFS_CDC_OK;
    if (!d_data || !d_files || !d_blocks || !table_base || !d_out || !out_off || !out_cap)
        return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (max_blocks >= (uint64_t)INT32_MAX)
        return fail_status(SDFS_CDC_EINVAL, "max_blocks %llu: block ordinals are 31-bit", (unsigned long long)max_blocks);
    const size_t nf = n_files;
    std::vector<uint64_t> meta(3 * nf);
    for (size_t f = 0; f < nf; f++) {
        meta[f] = table_base[f];
        meta[nf + f] = out_off[f];
        meta[2 * nf + f] = out_cap[f];
    }
    if (const int rc = device_of(d_files)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint64_t mb = max_blocks;
    Carve c;
    const size_t o_meta = c.add<uint64_t>(meta.size()), o_bad = c.add<unsigned long long>(nf), o_src = c.add<uint64_t>(mb),
                 o_dst = c.add<uint64_t>(mb), o_cnt = c.add<uint32_t>(nf), o_first = c.add<uint32_t>(nf + 1),
                 o_count = c.add<uint32_t>(1), o_lz = c.add<uint32_t>(mb), o_cap = c.add<uint32_t>(mb),
                 o_got = c.add<uint32_t>(mb), o_sum = c.add<uint32_t>(mb), o_chk = c.add<uint32_t>(mb),
                 o_file = c.add<uint32_t>(mb);
    Scratch sc(s);
    SDFS_TRY(sc.get(&c.base, c.bytes));
    uint64_t* d_meta = c.at<uint64_t>(o_meta);
    SDFS_TRY(upload_words(meta, d_meta, s));
    ReadArgs a{};
    a.data = d_data;
    a.table_base = d_meta;
    a.out_off = d_meta + nf;
    a.out_cap = d_meta + 2 * nf;
    a.n_files = n_files;
    a.max_blocks = mb;
    a.files = d_files;
    a.blocks = d_blocks;
    a.out = d_out;
    a.cnt = c.at<uint32_t>(o_cnt);
    a.first = c.at<uint32_t>(o_first);
    a.count = c.at<uint32_t>(o_count);
    a.src_off = c.at<uint64_t>(o_src);
    a.lz_len = c.at<uint32_t>(o_lz);
    a.dst_off = c.at<uint64_t>(o_dst);
    a.dst_cap = c.at<uint32_t>(o_cap);
    a.got = c.at<uint32_t>(o_got);
    a.sum = c.at<uint32_t>(o_sum);
    a.check = c.at<uint32_t>(o_chk);
    a.file = c.at<uint32_t>(o_file);
    a.bad = c.at<unsigned long long>(o_bad);
    SDFS_TRY(hipMemsetAsync(a.bad, 0xFF, nf * 8, s));
    hipLaunchKernelGGL(lz4s_read_count_kernel, dim3(grid256(nf)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(prefix_kernel<uint32_t>, dim3(1), dim3(1024), 0, s, a.cnt, n_files, a.first);
    hipLaunchKernelGGL(lz4s_read_room_kernel, dim3(grid256(nf)), dim3(256), 0, s, a);
    SDFS_TRY(hipGetLastError());
    if (mb) {
        hipLaunchKernelGGL(lz4s_read_list_kernel, dim3(grid256(mb)), dim3(256), 0, s, a);
        SDFS_TRY(hipGetLastError());
        if (const int rc = sdfs_cdc_lz4_decompress_device(z, d_data, a.src_off, a.lz_len, a.count, mb, d_out, a.dst_off,
                                                          a.dst_cap, a.got, 0, stream))
            return rc;
        hipLaunchKernelGGL(lz4s_raw_copy_kernel, dim3((uint32_t)std::min<uint64_t>(mb, 1u << 16)), dim3(256), 0, s, a);
        SDFS_TRY(launch_xxh32(XxhArgs{d_out, a.dst_off, a.dst_cap, a.count, mb, SDFS_CDC_LZ4_STREAM_SEED, a.sum}, s));
        hipLaunchKernelGGL(lz4s_verify_kernel, dim3(grid256(mb)), dim3(256), 0, s, a);
        hipLaunchKernelGGL(lz4s_read_status_kernel, dim3(grid256(nf)), dim3(256), 0, s, a);
        SDFS_TRY(hipGetLastError());
    }
    return SDFS_CDC_OK;
}

}  // extern "C"
