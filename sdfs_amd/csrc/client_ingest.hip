// client_ingest.hip — writeChunks for batches (include/sdfs_ingest.h).
//
// The client's entries are already cut and already fingerprinted; their payloads are raw or LZ4,
// at any offset of one blob.  Five small kernels turn them into what the write path takes:
//   plan    — one workgroup scans the entries (SDFS_CDC_INGEST_TILE per step, two running sums):
//             status, the chunk's place in a dense staging area, the decoder's batch;
//   decoded — after the LZ4 decoder: an item whose length is not raw_len flags its entry;
//   copy    — a workgroup per (entry, 64 KiB span): aligned 16-byte loads realigned by a byte
//             shift, 16-byte stores, edges byte by byte (the manner of archive_pack.hip);
//   compare — after hash_device: the client's hash against the chunk's fingerprint;
//   records — a second scan compacts the accepted entries into 48-byte fingerprint records;
//   results — per entry, from put_records' per-record outputs.
// Every phase that reads what another workgroup wrote is its own kernel on the same stream.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/sdfs_ingest.h"
#include "block_scan.h"
#include "call_support.h"
#include "cdc_internal.h"
#include "store_format.h"

namespace sdfs {
namespace {

constexpr uint32_t kTile = SDFS_CDC_INGEST_TILE;
constexpr uint32_t kCopySpan = SDFS_CDC_INGEST_COPY_SPAN;
constexpr int kCopyThreads = 256;
static_assert(kTile == 1024, "the scans are one block of 1024 threads");
static_assert(kCopySpan % 16 == 0, "a span is whole vectors");

using Batch = sdfs_cdc_ingest_batch;
using Plan = sdfs_cdc_ingest_plan;

// what the plan decides about entry i from the client's numbers alone
__device__ __forceinline__ uint32_t classify(const Batch& b, uint64_t i, uint32_t chunk_length) {
    const uint32_t len = b.len[i], raw = b.raw_len[i];
    if (len == 0) return SDFS_CDC_INGEST_EMPTY;
    if (raw == 0 || raw > chunk_length) return SDFS_CDC_INGEST_EBOUNDS;
    const uint64_t off = b.off[i];
    if (off > b.blob_bytes || len > b.blob_bytes - off) return SDFS_CDC_INGEST_EBOUNDS;
    if (!b.compressed[i] && len != raw) return SDFS_CDC_INGEST_EBOUNDS;
    return 0;
}

// One block.  Step t0 takes entries t0 .. t0 + kTile, one per thread; the carries run from step to
// step, so the prefix is over the whole batch in entry order.
__global__ __launch_bounds__(kTile) void ingest_plan_kernel(Batch b, Plan p, uint32_t chunk_length,
                                                            uint64_t stage_cap) {
    __shared__ uint64_t lds[16];
    uint64_t byte_carry = 0, dec_carry = 0, total;
    for (uint64_t t0 = 0; t0 < b.n; t0 += kTile) {
        const uint64_t i = t0 + threadIdx.x;
        uint32_t st = SDFS_CDC_INGEST_EBOUNDS, raw = 0;
        bool dec = false;
        if (i < b.n) {
            st = classify(b, i, chunk_length);
            raw = st ? 0 : b.raw_len[i];
            dec = !st && b.compressed[i];
        }
        const uint64_t at = byte_carry + block_exclusive_scan_1024<uint64_t>(raw, lds, total);
        byte_carry += total;
        // a chunk that would end past the staging area is left out; those before it keep their places
        if (!st && (at > stage_cap || raw > stage_cap - at)) {
            st = SDFS_CDC_INGEST_EBOUNDS;
            dec = false;
        }
        const uint64_t k = dec_carry + block_exclusive_scan_1024<uint64_t>(dec ? 1 : 0, lds, total);
        dec_carry += total;
        if (i < b.n) {
            p.status[i] = st;
            p.stage_off[i] = st ? 0 : at;
            if (dec) {
                p.dec_src_off[k] = b.off[i];
                p.dec_src_len[k] = b.len[i];
                p.dec_dst_off[k] = at;
                p.dec_cap[k] = raw;
                p.dec_entry[k] = (uint32_t)i;
            }
        }
    }
    if (threadIdx.x == 0) {
        *p.dec_count = (uint32_t)dec_carry;
        *p.staged = byte_carry < stage_cap ? byte_carry : stage_cap;
    }
}

__global__ __launch_bounds__(256) void ingest_decoded_kernel(Plan p, uint64_t n) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= min<uint64_t>(*p.dec_count, n)) return;
    if (p.dec_len[k] != p.dec_cap[k]) p.status[p.dec_entry[k]] |= SDFS_CDC_INGEST_EDECODE;  // entries are distinct
}

// blockIdx.x = entry, blockIdx.y = span of the entry.  The vectors lie at 16-byte addresses of the
// destination; a source vector is the aligned 16 bytes below its first byte and, when it is not
// aligned itself, the 16 above — both hold bytes of the chunk, so neither load leaves the blob.
__global__ __launch_bounds__(kCopyThreads) void ingest_copy_kernel(Batch b, Plan p, uint8_t* stage) {
    const uint64_t i = blockIdx.x;
    if (p.status[i] || b.compressed[i]) return;  // uniform over the workgroup
    const uint32_t len = b.len[i];
    const uint64_t s0 = (uint64_t)blockIdx.y * kCopySpan;
    if (s0 >= len) return;
    const uint32_t n = (uint32_t)min<uint64_t>(kCopySpan, len - s0);
    const uint8_t* src = b.blob + b.off[i] + s0;
    uint8_t* dst = stage + p.stage_off[i] + s0;
    const uint32_t head = min(n, (uint32_t)((0 - reinterpret_cast<uintptr_t>(dst)) & 15));
    const uint32_t nvec = (n - head) / 16;
    for (uint32_t k = threadIdx.x; k < head; k += kCopyThreads) dst[k] = src[k];
    const uintptr_t sa0 = reinterpret_cast<uintptr_t>(src + head);
    const uint32_t sh = (uint32_t)(sa0 & 15), q = sh >> 2, r = sh & 3;
    const uint4* ap = reinterpret_cast<const uint4*>(sa0 - sh);
    uint4* dv = reinterpret_cast<uint4*>(dst + head);
    for (uint32_t v = threadIdx.x; v < nvec; v += kCopyThreads) {
        const uint4 l = ap[v];
        uint4 w = l;
        if (sh) {
            const uint4 h = ap[v + 1];
            uint32_t t0, t1, t2, t3, t4;
            if (q == 0) { t0 = l.x; t1 = l.y; t2 = l.z; t3 = l.w; t4 = h.x; }
            else if (q == 1) { t0 = l.y; t1 = l.z; t2 = l.w; t3 = h.x; t4 = h.y; }
            else if (q == 2) { t0 = l.z; t1 = l.w; t2 = h.x; t3 = h.y; t4 = h.z; }
            else { t0 = l.w; t1 = h.x; t2 = h.y; t3 = h.z; t4 = h.w; }
            w.x = __builtin_amdgcn_alignbyte(t1, t0, r);
            w.y = __builtin_amdgcn_alignbyte(t2, t1, r);
            w.z = __builtin_amdgcn_alignbyte(t3, t2, r);
            w.w = __builtin_amdgcn_alignbyte(t4, t3, r);
        }
        dv[v] = w;
    }
    for (uint32_t k = head + nvec * 16 + threadIdx.x; k < n; k += kCopyThreads) dst[k] = src[k];
}

// the lengths hash_device takes: 0 for an entry that is not staged
__global__ __launch_bounds__(256) void ingest_hash_lens_kernel(Batch b, Plan p, uint32_t* lens) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < b.n) lens[i] = p.status[i] ? 0 : b.raw_len[i];
}

__global__ __launch_bounds__(256) void ingest_compare_kernel(Batch b, Plan p, const uint8_t* digests,
                                                             uint32_t hash_len) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= b.n || p.status[i]) return;
    uint32_t diff = 0;
    for (uint32_t k = 0; k < hash_len; k++) diff |= (uint32_t)(b.hash[i * 32 + k] ^ digests[i * 32 + k]);
    if (diff) p.status[i] = SDFS_CDC_INGEST_EHASH;
}

// One block, as the plan: the accepted entries' ranks in entry order.
__global__ __launch_bounds__(kTile) void ingest_records_kernel(Batch b, Plan p, uint8_t* records, uint32_t* count) {
    __shared__ uint32_t lds[16];
    uint32_t carry = 0, total;
    for (uint64_t t0 = 0; t0 < b.n; t0 += kTile) {
        const uint64_t i = t0 + threadIdx.x;
        const uint32_t on = i < b.n && p.status[i] == 0 ? 1u : 0u;
        const uint32_t r = carry + block_exclusive_scan_1024<uint32_t>(on, lds, total);
        carry += total;
        if (i >= b.n) continue;
        p.rec_of[i] = on ? r : SDFS_CDC_INGEST_NONE;
        if (!on) continue;
        const uint4* h = reinterpret_cast<const uint4*>(b.hash + i * 32);
        uint4* rec = reinterpret_cast<uint4*>(records + (uint64_t)r * kRecordBytes);
        rec[0] = h[0];
        rec[1] = h[1];
        rec[2] = make_uint4((uint32_t)i, (uint32_t)(i >> 32), 0u, b.raw_len[i]);  // u64 buffer_id | start | len
    }
    if (threadIdx.x == 0) *count = carry;
}

struct ResultArgs {
    const uint8_t* dup;
    const uint64_t* hashloc;
    uint64_t pos_base;
    const uint32_t* rec_len;
    uint64_t n_new_cap;
    uint8_t* inserted;
    int64_t* pos;
    uint32_t* stored_len;
    uint32_t* status;
};

__global__ __launch_bounds__(256) void ingest_results_kernel(Batch b, Plan p, ResultArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= b.n) return;
    const uint32_t r = p.rec_of[i];
    uint8_t ins = 0;
    int64_t pos = -1;
    uint32_t stored = 0;
    if (r != SDFS_CDC_INGEST_NONE) {
        ins = a.dup[r] ? 0 : 1;
        pos = (int64_t)a.hashloc[r];  // UINT64_MAX (the index overflowed) reads as -1
        const uint64_t k = a.hashloc[r] - a.pos_base;  // an inserted record's rank among the call's insertions
        if (ins && a.rec_len && k < a.n_new_cap) stored = a.rec_len[k];
    }
    a.inserted[i] = ins;
    a.pos[i] = pos;
    a.stored_len[i] = stored;
    a.status[i] = p.status[i];
}

int check_batch(const Batch* b) {
    if (!b) return fail_status(SDFS_CDC_EINVAL, "null batch");
    if (b->n >= (1ull << 31))
        return fail_status(SDFS_CDC_EINVAL, "%llu entries: split the batch", (unsigned long long)b->n);
    if (b->n && (!b->hash || !b->off || !b->len || !b->raw_len || !b->compressed))
        return fail_status(SDFS_CDC_EINVAL, "null entry array");
    if (b->blob_bytes && !b->blob) return fail_status(SDFS_CDC_EINVAL, "null blob");
    return SDFS_CDC_OK;
}

int check_plan(const Plan* p, uint64_t n) {
    if (!p) return fail_status(SDFS_CDC_EINVAL, "null plan");
    if (!p->dec_count || !p->staged) return fail_status(SDFS_CDC_EINVAL, "null dec_count or staged");
    if (n && (!p->status || !p->stage_off || !p->rec_of || !p->dec_src_off || !p->dec_src_len || !p->dec_dst_off ||
              !p->dec_cap || !p->dec_len || !p->dec_entry))
        return fail_status(SDFS_CDC_EINVAL, "null plan array");
    return SDFS_CDC_OK;
}

int check_both(const Batch* b, const Plan* p) {
    if (const int rc = check_batch(b)) return rc;
    return check_plan(p, b->n);
}

// the device the plan's arrays live on (for the calls that take a handle instead of a device)
int device_of(const void* p, int* device) {
    hipPointerAttribute_t at;
    SDFS_TRY(hipPointerGetAttributes(&at, p));
    *device = at.device;
    return SDFS_CDC_OK;
}

dim3 grid256(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

}  // namespace
}  // namespace sdfs

using namespace sdfs;

extern "C" {

int sdfs_cdc_ingest_chunks_plan(int device, const sdfs_cdc_ingest_batch* b, uint32_t chunk_length, uint64_t stage_cap,
                                const sdfs_cdc_ingest_plan* p, void* stream) {
    if (const int rc = check_both(b, p)) return rc;
    if (const int rc = check_chunk_length(chunk_length)) return rc;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ingest_plan_kernel, dim3(1), dim3(kTile), 0, s, *b, *p, chunk_length, stage_cap);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_ingest_chunks_decode(sdfs_cdc_lz4* z, const sdfs_cdc_ingest_batch* b, const sdfs_cdc_ingest_plan* p,
                                  uint8_t* d_stage, void* stream) {
    if (!z) return fail_status(SDFS_CDC_EINVAL, "null decoder");
    if (const int rc = check_both(b, p)) return rc;
    if (b->n && !d_stage) return fail_status(SDFS_CDC_EINVAL, "null staging area");
    if (b->n == 0) return SDFS_CDC_OK;
    if (const int rc = sdfs_cdc_lz4_decompress_device(z, b->blob, p->dec_src_off, p->dec_src_len, p->dec_count, b->n,
                                                      d_stage, p->dec_dst_off, p->dec_cap, p->dec_len, 0, stream))
        return rc;
    int device = 0;
    if (const int rc = device_of(p->status, &device)) return rc;
    if (const int rc = set_device(device)) return rc;
    hipLaunchKernelGGL(ingest_decoded_kernel, grid256(b->n), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *p,
                       b->n);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_ingest_chunks_copy(int device, const sdfs_cdc_ingest_batch* b, const sdfs_cdc_ingest_plan* p,
                                uint32_t chunk_length, uint8_t* d_stage, void* stream) {
    if (const int rc = check_both(b, p)) return rc;
    if (const int rc = check_chunk_length(chunk_length)) return rc;
    if (b->n && !d_stage) return fail_status(SDFS_CDC_EINVAL, "null staging area");
    if (b->n == 0) return SDFS_CDC_OK;
    if (const int rc = set_device(device)) return rc;
    const uint32_t spans = (uint32_t)(((uint64_t)chunk_length + kCopySpan - 1) / kCopySpan);  // <= 32768
    hipLaunchKernelGGL(ingest_copy_kernel, dim3((uint32_t)b->n, spans), dim3(kCopyThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), *b, *p, d_stage);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_ingest_chunks_verify(sdfs_cdc_engine* engine, const sdfs_cdc_ingest_batch* b,
                                  const sdfs_cdc_ingest_plan* p, const uint8_t* d_stage, uint32_t hash_len,
                                  void* stream) {
    if (!engine) return fail_status(SDFS_CDC_EINVAL, "null engine");
    if (const int rc = check_both(b, p)) return rc;
    if (const int rc = check_hash_len(hash_len, HashOf::kRecord)) return rc;
    const int dl = sdfs_cdc_digest_len(engine);
    if (dl < 0) return fail_status(SDFS_CDC_EINVAL, "not a live engine handle");
    if ((uint32_t)dl != hash_len)
        return fail_status(SDFS_CDC_EINVAL, "engine digests are %d bytes, the client's hashes hold %u", dl, hash_len);
    if (b->n && !d_stage) return fail_status(SDFS_CDC_EINVAL, "null staging area");
    if (b->n == 0) return SDFS_CDC_OK;
    int device = 0;
    if (const int rc = device_of(p->status, &device)) return rc;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    Scratch sc(s);
    uint32_t* lens = nullptr;
    uint8_t* digests = nullptr;
    SDFS_TRY(sc.get(&lens, (size_t)b->n));
    SDFS_TRY(sc.get(&digests, (size_t)b->n * 32));
    hipLaunchKernelGGL(ingest_hash_lens_kernel, grid256(b->n), dim3(256), 0, s, *b, *p, lens);
    SDFS_TRY(hipGetLastError());
    if (const int rc = sdfs_cdc_hash_device(engine, d_stage, p->stage_off, lens, nullptr, b->n, digests, stream))
        return rc;
    hipLaunchKernelGGL(ingest_compare_kernel, grid256(b->n), dim3(256), 0, s, *b, *p, digests, hash_len);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_ingest_chunks_records(int device, const sdfs_cdc_ingest_batch* b, const sdfs_cdc_ingest_plan* p,
                                   uint8_t* d_records, uint32_t* d_count, void* stream) {
    if (const int rc = check_both(b, p)) return rc;
    if (!d_count) return fail_status(SDFS_CDC_EINVAL, "null count");
    if (b->n && !d_records) return fail_status(SDFS_CDC_EINVAL, "null records");
    if (b->n && ((reinterpret_cast<uintptr_t>(d_records) | reinterpret_cast<uintptr_t>(b->hash)) & 15))
        return fail_status(SDFS_CDC_EINVAL, "hashes and records are 16-byte aligned");
    if (const int rc = set_device(device)) return rc;
    hipLaunchKernelGGL(ingest_records_kernel, dim3(1), dim3(kTile), 0, reinterpret_cast<hipStream_t>(stream), *b, *p,
                       d_records, d_count);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_ingest_chunks_results(int device, const sdfs_cdc_ingest_batch* b, const sdfs_cdc_ingest_plan* p,
                                   const uint8_t* d_dup, const uint64_t* d_hashloc, uint64_t pos_base,
                                   const uint32_t* d_rec_len, uint64_t n_new_cap, uint8_t* d_inserted, int64_t* d_pos,
                                   uint32_t* d_stored_len, uint32_t* d_status, void* stream) {
    if (const int rc = check_both(b, p)) return rc;
    if (b->n && (!d_dup || !d_hashloc || !d_inserted || !d_pos || !d_stored_len || !d_status))
        return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (b->n == 0) return SDFS_CDC_OK;
    if (const int rc = set_device(device)) return rc;
    const ResultArgs a{d_dup, d_hashloc, pos_base, d_rec_len, d_rec_len ? n_new_cap : 0, d_inserted, d_pos,
                       d_stored_len, d_status};
    hipLaunchKernelGGL(ingest_results_kernel, grid256(b->n), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *b,
                       *p, a);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

}  // extern "C"
