// call_support.h — what every entry point of the store layer does around its launches: the
// device, per-call scratch, the mapping of HIP errors to C-ABI codes, the hash_len checks and the
// live count of a batch, the 64-bit add of its counters.  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "../../include/sdfs_archive.h"
#include "../../include/sdfs_read.h"
#include "cdc_internal.h"

namespace sdfs {
namespace {  // internal linkage: nothing here joins the libraries' exported symbols

// per-call scratch in stream order; released in the destructor (the frees are enqueued behind
// whatever was launched on the stream before it runs)
struct Scratch {
    hipStream_t s;
    void* ptrs[6] = {};
    int n = 0;
    explicit Scratch(hipStream_t st) : s(st) {}
    template <typename T>
    hipError_t get(T** out, size_t count) {
        void* p = nullptr;
        const hipError_t e = hipMallocAsync(&p, std::max<size_t>(count, 1) * sizeof(T), s);
        if (e == hipSuccess) ptrs[n++] = p;
        *out = static_cast<T*>(p);
        return e;
    }
    ~Scratch() {
        for (int i = 0; i < n; i++) (void)hipFreeAsync(ptrs[i], s);
    }
};

#define SDFS_TRY(expr)                                                                             \
    do {                                                                                           \
        const hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                      \
            return fail_status(e_ == hipErrorOutOfMemory ? SDFS_CDC_ENOMEM : SDFS_CDC_EHIP, "%s: %s", #expr, \
                               hipGetErrorString(e_));                                             \
    } while (0)

int set_device(int device) {
    const hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail_status(SDFS_CDC_ENODEV, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
    return SDFS_CDC_OK;
}

// what a hash_len is the length of
enum class HashOf {
    kPair,    // a HashLocPair's hash: 16 or 32
    kMapKey,  // a .map key: 16 or 32
    kRecord,  // a stored record's hash: 16, 20 or 32
};

int check_hash_len(uint32_t hash_len, HashOf of) {
    if (hash_len == 16 || hash_len == 32 || (of == HashOf::kRecord && hash_len == 20)) return SDFS_CDC_OK;
    if (of == HashOf::kPair)
        return fail_status(SDFS_CDC_EINVAL, "hash_len %u: HashLocPair holds 32 (SHA-256) or 16 (MD5) bytes", hash_len);
    if (of == HashOf::kRecord)
        return fail_status(SDFS_CDC_EINVAL, "hash_len %u: 16 (MD5), 20 (SHA-256/160) or 32 (SHA-256)", hash_len);
    if (hash_len == 20)
        return fail_status(SDFS_CDC_EINVAL,
                           "hash_len 20: the reference's map slots are made for hashLength 18 and do not hold the key");
    return fail_status(SDFS_CDC_EINVAL, "hash_len %u: 16 (MD5) or 32 (SHA-256)", hash_len);
}

// the argument checks more than one of the files makes
bool pairs_complete(const sdfs_cdc_pairs* p) {
    return p && p->counts && p->hashes && p->hashloc && p->len && p->pos && p->offset && p->nlen && p->doop &&
           p->flags && p->status && p->cap;
}

int check_chunk_length(uint32_t chunk_length) {
    if (chunk_length < 1 || chunk_length > (uint32_t)INT32_MAX)
        return fail_status(SDFS_CDC_EINVAL, "chunk_length %u: 1 .. 2^31 - 1 (HashLocPair.pos is an int)", chunk_length);
    return SDFS_CDC_OK;
}

int check_header(uint32_t header_bytes) {
    if (header_bytes == 0 || header_bytes == SDFS_CDC_ARCHIVE_HEADER) return SDFS_CDC_OK;
    return fail_status(SDFS_CDC_EINVAL, "header_bytes %u: 0 (VERSION 0) or %u", header_bytes, SDFS_CDC_ARCHIVE_HEADER);
}

// records of a batch whose count may live on the device
__device__ __forceinline__ uint64_t live_count(const uint32_t* count, uint64_t n_max) {
    return count ? min<uint64_t>(*count, n_max) : n_max;
}

// a device-scope 64-bit add, returning the word's value before it (HIP's atomicAdd takes unsigned
// long long; the counters are uint64_t words)
__device__ __forceinline__ uint64_t add64(uint64_t* p, uint64_t v) {
    return atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

}  // namespace
}  // namespace sdfs
