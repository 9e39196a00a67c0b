// block_scan.h — the prefix sums and the hinted floor search the store kernels share (device).
// Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sdfs {

// a lane's value read by every lane (src is wave-uniform)
template <typename T>
__device__ __forceinline__ T wave_read(T v, uint32_t src) {
    if constexpr (sizeof(T) == 8) return (T)__shfl((unsigned long long)v, (int)src);
    else return __shfl(v, (int)src);
}

// inclusive sum over the lanes up to and including this one, in groups of W lanes (lane = the
// lane's number in its group)
template <typename T, int W = 64>
__device__ __forceinline__ T wave_inclusive_scan(T v, uint32_t lane) {
#pragma unroll
    for (int o = 1; o < W; o <<= 1) {
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

// 64-lane sum, the result in every lane
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        if constexpr (sizeof(T) == 8) v += (T)__shfl_xor((unsigned long long)v, o);
        else v += __shfl_xor(v, o);
    }
    return v;
}

// One block of 1024 threads (16 waves), K values per thread under one pair of barriers: v[k]
// becomes the sum of v[k] over the threads before this one, total[k] the block's sum.  A wave
// scan, the 16 wave sums through LDS, and every wave scans those 16 in its first lanes: one LDS
// word per lane and no third barrier to pass the result on.  lds holds K x 16 entries and may be
// used again after the call returns.
// Not used by plan_scan_kernel and archive_plan_kernel (one block walking ~130 tiles: the 16-lane scan
// and the two lane reads behind the barrier are a longer chain per tile than 16 LDS reads) nor by
// imp_rec_count_kernel (two flags: two ballots are cheaper); their rows lay above the parent's bound
// in both sessions of profiles/slot_walk_refactor/README.md (+8 %, +2 %, +3 %).
template <typename T, int K>
__device__ __forceinline__ void block_exclusive_scan_1024(T (&v)[K], T (*lds)[16], T (&total)[K]) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; k++) {
        const T inc = wave_inclusive_scan(v[k], lane);
        if (lane == 63) lds[k][wv] = inc;
        v[k] = inc - v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) {
        const T sums = wave_inclusive_scan<T, 16>(lane < 16 ? lds[k][lane] : 0, lane);
        if (wv) v[k] += wave_read(sums, wv - 1);
        total[k] = wave_read(sums, 15);
    }
    __syncthreads();
}

// the same for one value: returns the sum over the threads before this one; lds holds 16 entries
template <typename T>
__device__ __forceinline__ T block_exclusive_scan_1024(T v, T* lds, T& total) {
    T a[1] = {v}, t[1];
    block_exclusive_scan_1024<T, 1>(a, reinterpret_cast<T(*)[16]>(lds), t);
    total = t[0];
    return a[0];
}

// One block of 1024 threads: per-block sums become the sums before each block (in place, tile by
// tile with a carry); returns the sum of all, in every thread.  lds holds 16 entries.
template <typename T>
__device__ __forceinline__ uint64_t block_sums_to_bases(T* sums, uint32_t nblocks, T* lds) {
    uint64_t carry = 0;
    for (uint32_t b0 = 0; b0 < nblocks; b0 += 1024) {
        const uint32_t b = b0 + threadIdx.x;
        T total;
        const T ex = block_exclusive_scan_1024<T>(b < nblocks ? sums[b] : 0, lds, total);
        if (b < nblocks) sums[b] = (T)(carry + ex);
        carry += total;
    }
    return carry;
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
    __shared__ T lds[16];
    uint32_t b0, b1;
    block_run_1024(n, b0, b1);
    T sum = 0, total;
    for (uint32_t b = b0; b < b1; b++) sum += in[b];
    T run = block_exclusive_scan_1024(sum, lds, total);
    for (uint32_t b = b0; b < b1; b++) {
        out[b] = run;
        run += in[b];
    }
    if (threadIdx.x == 1023) out[n] = total;
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
