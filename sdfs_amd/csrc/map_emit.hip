// map_emit.hip — SparseDataChunk / HashLocPair images of flushed write buffers on the device
// (include/sdfs_meta.h).
//
// Reference: SparseDedupFile.writeCache builds one HashLocPair per chunk
// (SparseDedupFile.java:535-556) and LongByteArrayMap.put writes SparseDataChunk.getBytes()
// (SparseDataChunk.java:295-318, HashLocPair.asArray HashLocPair.java:49-59) into the buffer's
// slot of the file map (LongByteArrayMap.java:536-579).  Two kernels: a one-block prefix of the
// per-buffer chunk counts (first record of each buffer), then one wave per buffer writing its
// image — lane i the i-th record (big-endian fields, byte stores: records start at odd offsets),
// a wave reduction for doop, lane 0 the header and trailer.  Pure byte formatting: ~1/4700 of
// the data volume, HBM-write bound.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/sdfs_meta.h"
#include "block_scan.h"
#include "call_support.h"
#include "store_format.h"

namespace sdfs {
namespace {

struct MapArgs {
    uint32_t nbuf;
    const uint32_t* counts;
    const uint32_t* starts;
    const uint32_t* lens;
    const uint8_t* digests;
    uint32_t cap;
    uint32_t hash_len;
    const uint8_t* dup;
    const uint64_t* hashloc;
    const uint32_t* first;  // [nbuf] first record of each buffer
    uint8_t* map;
    uint32_t slot_bytes;
    uint32_t* doop;
    uint32_t* overflow;
};

__global__ __launch_bounds__(256) void map_emit_kernel(MapArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= a.nbuf) return;
    const uint32_t n = a.counts[b];
    if (slot_need(n, a.hash_len) > a.slot_bytes) {
        if (lane == 0) atomicOr(a.overflow, 1u);
        return;
    }
    uint8_t* img = a.map + (uint64_t)b * a.slot_bytes;
    const uint32_t r0 = a.first[b];
    uint32_t doop = 0;
    for (uint32_t i = lane; i < n; i += 64) {
        const uint64_t slot = (uint64_t)b * a.cap + i;
        const uint32_t st = a.starts[slot], ln = a.lens[slot];
        const uint64_t r = (uint64_t)r0 + i;
        // len = nlen = the chunk's length, pos = its start in the buffer, offset 0
        put_pair_record(img, i, a.hash_len, a.digests + slot * 32, a.hashloc[r], ln, st, 0, ln);
        if (a.dup[r]) doop += ln;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) doop += __shfl_xor(doop, o);
    if (lane == 0) {
        put_slot_frame(img, 0, n, a.hash_len, doop);  // flags: not RECONSTRUCTED
        if (a.doop) a.doop[b] = doop;
    }
}

}  // namespace
}  // namespace sdfs

using namespace sdfs;

extern "C" {

uint32_t sdfs_cdc_map_slot_bytes(uint32_t hash_len, uint32_t chunk_length, uint32_t min_len) {
    const uint32_t max_cluster = min_len ? chunk_length / min_len : 0;  // HashFunctionPool.java:66
    return kSlotFixedBytes + pair_bytes(hash_len) * 2 * max_cluster;
}

int sdfs_cdc_map_emit(int device, uint32_t nbuf, const sdfs_cdc_dev_out* out, uint32_t hash_len,
                      const uint8_t* d_dup, const uint64_t* d_hashloc, uint8_t* d_map, uint32_t slot_bytes,
                      uint32_t* d_doop, uint32_t* d_overflow, void* stream) {
    if (!out || !out->counts || !out->starts || !out->lens || !out->digests)
        return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_dev_out");
    if (const int rc = check_hash_len(hash_len, HashOf::kPair)) return rc;
    if (nbuf && (!d_dup || !d_hashloc || !d_map || !d_overflow)) return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (nbuf == 0) return SDFS_CDC_OK;
    if (slot_bytes < kSlotFixedBytes) return fail_status(SDFS_CDC_EINVAL, "slot_bytes %u < 13", slot_bytes);
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    Scratch sc(s);
    uint32_t* first = nullptr;  // [nbuf + 1] first record of each buffer
    SDFS_TRY(sc.get(&first, (size_t)nbuf + 1));
    hipLaunchKernelGGL(prefix_kernel<uint32_t>, dim3(1), dim3(1024), 0, s, out->counts, nbuf, first);
    MapArgs a{nbuf,     out->counts, out->starts, out->lens, out->digests, out->cap, hash_len, d_dup,
              d_hashloc, first,      d_map,       slot_bytes, d_doop,      d_overflow};
    hipLaunchKernelGGL(map_emit_kernel, dim3((nbuf + 3) / 4), dim3(256), 0, s, a);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

}  // extern "C"
