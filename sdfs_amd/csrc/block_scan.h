// block_scan.h — the prefix sums and the hinted floor search the store kernels share (device).
// Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sdfs {

// inclusive sum over the lanes of a wave up to and including this one
template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v, uint32_t lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        if constexpr (sizeof(T) == 8) {
            const unsigned long long y = __shfl_up((unsigned long long)v, o);
            if (lane >= (uint32_t)o) v += y;
        } else {
            const T y = __shfl_up(v, o);
            if (lane >= (uint32_t)o) v += y;
        }
    }
    return v;
}

// One block of 1024 threads, thread t holding `sum` over its run of the input: returns the sum
// over threads 0..t (Hillis–Steele in LDS), and part[1023] is the total for every thread.
template <typename T>
__device__ __forceinline__ T block_inclusive_scan_1024(T sum, T* part) {
    const uint32_t t = threadIdx.x;
    part[t] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {
        const T v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    return part[t];
}

// thread t's run [b0, b1) of n inputs split over 1024 threads
__device__ __forceinline__ void block_run_1024(uint32_t n, uint32_t& b0, uint32_t& b1) {
    const uint32_t per = (n + 1023) / 1024;
    b0 = min(threadIdx.x * per, n);
    b1 = min(b0 + per, n);
}

namespace {

// out[i] = sum of in[0..i) for i <= n (one block; 16 Ki inputs = 16 per thread).  A template, so
// that only the translation units that launch it carry it; internal linkage, so that it is no
// exported symbol.
template <typename T>
__global__ __launch_bounds__(1024) void prefix_kernel(const T* in, uint32_t n, T* out) {
    __shared__ T part[1024];
    uint32_t b0, b1;
    block_run_1024(n, b0, b1);
    T sum = 0;
    for (uint32_t b = b0; b < b1; b++) sum += in[b];
    T run = block_inclusive_scan_1024(sum, part) - sum;
    for (uint32_t b = b0; b < b1; b++) {
        out[b] = run;
        run += in[b];
    }
    if (threadIdx.x == 1023) out[n] = part[1023];
}

}  // namespace

// largest k with key[k] <= x, -1 if none (key ascending); `hint` = the answer for a nearby x
template <typename K>
__device__ __forceinline__ int32_t floor_index(const K* key, int32_t n, K x, int32_t hint) {
    // next is unsigned so that key[next] is never addressed as (key + hint) + 1: for hint = -1 and
    // key in LDS that would be a flat address below the LDS aperture plus an instruction offset,
    // and the hardware picks the aperture before it adds the offset
    const uint32_t next = (uint32_t)(hint + 1);
    if (hint >= -1 && hint < n && (hint < 0 || key[hint] <= x) && (next >= (uint32_t)n || key[next] > x))
        return hint;
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (key[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

}  // namespace sdfs
