// write_path.hip — the device side of the ranged write (include/sdfs_write.h):
// DedupFileChannel.writeFile (DedupFileChannel.java:274-359) for batches of byte ranges.
//
// write_stage: the visible pieces the host split (write_split.h) leaves are copied from the
// caller's blob into the staging area the engine chunks.  The work list is the spans of all pieces
// — kSpanVecs 16-byte vectors of a piece's destination each — found by a floor search in the
// prefix of the span counts, as the ranged read tiles its pieces; workgroups stride over it, so
// thousands of short pieces and a few long ones both spread over the machine.  A lane owns whole
// destination vectors: it reads the four or five aligned source dwords that hold a vector's bytes,
// re-aligns them in registers and stores 16 aligned bytes.  Only the first and the last vector of a
// piece, where bytes of a neighbour share the vector, go byte by byte.
//
// map_inserts_from_runs: the write accelerator's insert list (WritableCacheBuffer.java:729-753)
// for runs of different lengths, the buffers of a ragged engine batch from first_buf on.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "../../include/sdfs_write.h"
#include "block_scan.h"
#include "call_support.h"
#include "write_split.h"

namespace sdfs {
namespace {

constexpr int kStageThreads = 256;
constexpr uint32_t kSpanVecs = SDFS_CDC_WRITE_SPAN / 16;  // 16-byte vectors per span
constexpr uint32_t kStageGrid = 16384;                    // workgroups at most (they stride over the spans)

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

struct StageArgs {
    uint32_t n_pieces;
    const uint8_t* blob;
    uint64_t blob_bytes;
    const uint64_t* src_off;
    const uint64_t* dst_off;
    const uint32_t* len;
    uint32_t max_len;
    uint8_t* stage;
    uint64_t stage_bytes;
    uint32_t* piece_status;
    const uint32_t* piece_req;
    uint32_t n_requests;
    uint32_t* req_status;
    uint32_t* spans;       // [n_pieces] spans of the piece's destination
    uint32_t* span_first;  // [n_pieces + 1] their exclusive prefix
};

// 16-byte vectors that hold the bytes [head, head + len) counted from a 16-byte boundary
__device__ __forceinline__ uint32_t range_vecs(uint32_t head, uint32_t len) { return (head + len + 15) >> 4; }

// per piece: the bounds check and its span count
__global__ __launch_bounds__(256) void stage_spans_kernel(StageArgs a) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.n_pieces) return;
    const uint64_t so = a.src_off[p], d = a.dst_off[p];
    const uint32_t len = a.len[p];
    const bool bad = len > a.max_len || so > a.blob_bytes || a.blob_bytes - so < len || d > a.stage_bytes ||
                     a.stage_bytes - d < len;
    uint32_t spans = 0;
    if (!bad && len) {
        const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(a.stage + d) & 15);
        spans = (range_vecs(head, len) + kSpanVecs - 1) / kSpanVecs;
    }
    a.spans[p] = spans;
    a.piece_status[p] = bad ? SDFS_CDC_WRITE_BOUNDS : 0;
    if (bad && a.req_status && a.piece_req[p] < a.n_requests) atomicOr(a.req_status + a.piece_req[p], SDFS_CDC_WRITE_BOUNDS);
}

// the 16 source bytes from s on, s at any alignment: aligned dwords, shifted together
__device__ __forceinline__ uint4 load16_unaligned(const uint8_t* s) {
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 3);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(s - sh);
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
    if (sh == 0) return make_uint4(w0, w1, w2, w3);
    const uint32_t w4 = w[4];  // holds byte s + 15: inside the piece
    return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh),
                      __builtin_amdgcn_alignbyte(w3, w2, sh), __builtin_amdgcn_alignbyte(w4, w3, sh));
}

__global__ __launch_bounds__(kStageThreads) void stage_copy_kernel(StageArgs a) {
    const uint32_t tid = threadIdx.x;
    const uint32_t total = a.span_first[a.n_pieces];
    for (uint32_t t = blockIdx.x; t < total; t += gridDim.x) {  // uniform over the workgroup
        const uint32_t p = uni((uint32_t)floor_index<uint32_t>(a.span_first, (int32_t)a.n_pieces, t, -2));
        const uint32_t len = uni(a.len[p]);
        const uint8_t* src = a.blob + a.src_off[p];
        uint8_t* dst = a.stage + a.dst_off[p];
        const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15);
        uint8_t* vbase = dst - head;  // 16-byte aligned; vector v holds the piece's bytes [16 v - head, 16 v - head + 16)
        const uint32_t nvec = range_vecs(head, len);
        const uint32_t v0 = uni(t - a.span_first[p]) * kSpanVecs;
        const uint32_t v1 = min(v0 + kSpanVecs, nvec);
#pragma unroll 4
        for (uint32_t v = v0 + tid; v < v1; v += kStageThreads) {
            const int64_t lo = (int64_t)v * 16 - head;  // of the piece's bytes
            if (lo >= 0 && lo + 16 <= (int64_t)len) {
                *reinterpret_cast<uint4*>(vbase + (uint64_t)v * 16) = load16_unaligned(src + lo);
            } else {  // the piece's first or last vector: only its own bytes
                const uint32_t b0 = lo < 0 ? (uint32_t)-lo : 0;
                const uint32_t b1 = (uint32_t)min<int64_t>(16, (int64_t)len - lo);
                for (uint32_t b = b0; b < b1; b++) vbase[(uint64_t)v * 16 + b] = src[lo + b];
            }
        }
    }
}

// ------------------------------------------------------------------------------------- from runs

struct RunsArgs {
    uint32_t first_buf, n_run, nbuf_dst, chunk_length;
    sdfs_cdc_dev_out out;
    const uint32_t* run_len;
    const uint64_t* hashloc;
    const sdfs_cdc_run* runs;
    sdfs_cdc_inserts ins;
    uint64_t n_ins_cap;
    const uint32_t* run_first;
    const uint32_t* rec_base;  // [first_buf + 1]: the last one = the records of the buffers before the runs
};

__device__ __forceinline__ void copy_hash(uint8_t* dst, const uint8_t* src) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = s[k];
}

// one wave per run, four per block
__global__ __launch_bounds__(256) void from_runs_kernel(RunsArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.n_run || a.run_first[a.n_run] > a.n_ins_cap) return;
    const uint32_t buf = a.first_buf + r;
    const uint32_t n = min(a.out.counts[buf], a.out.cap);
    const uint32_t first = a.run_first[r];
    const uint64_t rec0 = (uint64_t)a.rec_base[a.first_buf] + first;
    const sdfs_cdc_run run = a.runs[r];
    const uint32_t rl = a.run_len[r];
    const bool ok = run.dst_buf < a.nbuf_dst && rl >= 1 && (uint64_t)run.run_pos + rl <= a.chunk_length;
    for (uint32_t i = lane; i < n; i += 64) {
        const uint64_t slot = (uint64_t)buf * a.out.cap + i, o = (uint64_t)first + i;
        copy_hash(a.ins.hash + o * 32, a.out.digests + slot * 32);
        a.ins.hashloc[o] = a.hashloc[rec0 + i];
        a.ins.len[o] = (int32_t)a.out.lens[slot];
        a.ins.pos[o] = (int32_t)(run.run_pos + a.out.starts[slot]);
        a.ins.offset[o] = 0;
        a.ins.nlen[o] = (int32_t)a.out.lens[slot];
        a.ins.dst_buf[o] = ok ? run.dst_buf : a.nbuf_dst;
    }
}

}  // namespace
}  // namespace sdfs

using namespace sdfs;

extern "C" {

int sdfs_cdc_write_split(const sdfs_cdc_read_file* files, uint32_t n_files, const sdfs_cdc_write_request* requests,
                         uint32_t n_requests, uint32_t chunk_length, uint64_t blob_bytes, int64_t* n_written,
                         uint64_t* new_file_len, sdfs_cdc_write_plan* plan) {
    const char* why = "";
    const int rc = write_split(files, n_files, requests, n_requests, chunk_length, blob_bytes, n_written, new_file_len,
                               plan, &why);
    if (rc == SDFS_CDC_ECAP)
        return fail_status(rc, "%llu pieces in %llu runs of %llu rows: piece_cap %u, run_cap %u, row_cap %u",
                           (unsigned long long)plan->n_pieces, (unsigned long long)plan->n_runs,
                           (unsigned long long)plan->n_rows, plan->piece_cap, plan->run_cap, plan->row_cap);
    return rc ? fail_status(rc, "%s", why) : SDFS_CDC_OK;
}

int sdfs_cdc_write_stage(int device, uint32_t n_pieces, const uint8_t* d_blob, uint64_t blob_bytes,
                         const uint64_t* d_src_off, const uint64_t* d_dst_off, const uint32_t* d_len, uint32_t max_len,
                         uint8_t* d_stage, uint64_t stage_bytes, uint32_t* d_piece_status,
                         const uint32_t* d_piece_req, uint32_t n_requests, uint32_t* d_req_status, void* stream) {
    if (n_pieces && (!d_src_off || !d_dst_off || !d_len || !d_piece_status || !d_blob || !d_stage))
        return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (d_req_status && n_requests && n_pieces && !d_piece_req)
        return fail_status(SDFS_CDC_EINVAL, "d_req_status without d_piece_req");
    if (max_len < 1 || max_len > (uint32_t)INT32_MAX)
        return fail_status(SDFS_CDC_EINVAL, "max_len %u: 1 .. 2^31 - 1", max_len);
    const uint32_t spans = (uint32_t)(((uint64_t)max_len + 30) / 16 / kSpanVecs + 1);  // of one piece, at most
    if ((uint64_t)spans * n_pieces > (uint64_t)INT32_MAX)
        return fail_status(SDFS_CDC_EINVAL, "%u pieces of up to %u bytes: split the batch", n_pieces, max_len);
    if (n_pieces == 0) return SDFS_CDC_OK;
    {
        const uintptr_t b0 = reinterpret_cast<uintptr_t>(d_blob), s0 = reinterpret_cast<uintptr_t>(d_stage);
        if (b0 < s0 + stage_bytes && s0 < b0 + blob_bytes) return fail_status(SDFS_CDC_EINVAL, "the blob and the staging area overlap");
    }
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    Scratch sc(s);
    StageArgs a{n_pieces, d_blob,         blob_bytes,  d_src_off,  d_dst_off,
                d_len,    max_len,        d_stage,     stage_bytes, d_piece_status,
                d_piece_req, n_requests,  (d_req_status && n_requests) ? d_req_status : nullptr, nullptr, nullptr};
    uint32_t* per_piece = nullptr;  // spans, span_first
    SDFS_TRY(sc.get(&per_piece, (size_t)n_pieces * 2 + 1));
    a.spans = per_piece;
    a.span_first = per_piece + n_pieces;
    hipLaunchKernelGGL(stage_spans_kernel, dim3((n_pieces + 255) / 256), dim3(256), 0, s, a);
    hipLaunchKernelGGL(prefix_kernel<uint32_t>, dim3(1), dim3(1024), 0, s, a.spans, n_pieces, a.span_first);
    const uint64_t bound = (uint64_t)spans * n_pieces;  // of the span count, known without a host read
    hipLaunchKernelGGL(stage_copy_kernel, dim3((uint32_t)std::min<uint64_t>(bound, kStageGrid)), dim3(kStageThreads), 0, s,
                       a);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_map_inserts_from_runs(int device, uint32_t first_buf, uint32_t n_run, const sdfs_cdc_dev_out* out,
                                   const uint32_t* h_run_len, const uint32_t* d_run_len, const uint64_t* d_hashloc,
                                   uint32_t nbuf_dst, uint32_t chunk_length, const sdfs_cdc_run* h_runs,
                                   const sdfs_cdc_run* d_runs, const sdfs_cdc_inserts* ins, uint64_t n_ins_cap,
                                   uint32_t* d_run_first, void* stream) {
    if (!out || !out->counts || !out->starts || !out->lens || !out->digests || !out->cap)
        return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_dev_out");
    if (!ins || !ins->hash || !ins->hashloc || !ins->len || !ins->pos || !ins->offset || !ins->nlen || !ins->dst_buf)
        return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_inserts");
    if (const int rc = check_chunk_length(chunk_length)) return rc;
    if (!d_run_first || (n_run && (!h_runs || !d_runs || !h_run_len || !d_run_len || !d_hashloc)))
        return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_run >= (uint32_t)INT32_MAX || first_buf >= (uint32_t)INT32_MAX)
        return fail_status(SDFS_CDC_EINVAL, "%u runs after %u buffers: split the batch", n_run, first_buf);
    for (uint32_t r = 0; r < n_run; r++)
        if (h_runs[r].dst_buf >= nbuf_dst || h_run_len[r] < 1 || (uint64_t)h_runs[r].run_pos + h_run_len[r] > chunk_length)
            return fail_status(SDFS_CDC_EINVAL, "run %u {buffer %u of %u, pos %u} + %u bytes: outside the buffer (%u)", r,
                               h_runs[r].dst_buf, nbuf_dst, h_runs[r].run_pos, h_run_len[r], chunk_length);
    if (const int rc = set_device(device)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    Scratch sc(st);
    uint32_t* rec_base = nullptr;
    SDFS_TRY(sc.get(&rec_base, (size_t)first_buf + 1));
    hipLaunchKernelGGL(prefix_kernel<uint32_t>, dim3(1), dim3(1024), 0, st, out->counts, first_buf, rec_base);
    hipLaunchKernelGGL(prefix_kernel<uint32_t>, dim3(1), dim3(1024), 0, st, out->counts + first_buf, n_run, d_run_first);
    if (n_run) {
        RunsArgs a{first_buf, n_run, nbuf_dst, chunk_length, *out, d_run_len, d_hashloc, d_runs, *ins, n_ins_cap,
                   d_run_first, rec_base};
        hipLaunchKernelGGL(from_runs_kernel, dim3((n_run + 3) / 4), dim3(256), 0, st, a);
    }
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

}  // extern "C"
