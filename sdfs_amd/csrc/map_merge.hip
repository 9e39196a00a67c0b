// map_merge.hip — HashLocPairs merged into map slots that already exist (include/sdfs_extent.h):
// extent copies (CopyExtents.java:80-180, SparseDataChunk.getWL :181-206) and the write
// accelerator's block rewrites (WritableCacheBuffer.java:617-781), both through
// SparseDataChunk.insertHashLocPair (:208-263) and getBytes (:295-318).
//
// A buffer is independent work.  map_extents: one wave per segment, count pass -> prefix -> emit
// pass.  map_insert: the buffer's inserts are replayed in order on a work list of 16-byte
// elements {source | dup, pos, offset, nlen}; the list is ascending and disjoint at every step, so
// an insert [P, E) leaves a prefix (the pairs with pos < P, the last one cut at P), itself, at most
// one split tail, and a suffix (the first one cut at E): two binary searches, then every lane
// moves its elements into the second list.  Hashes move once, when the final list is written.
// One wave with both lists in LDS up to kLdsWork elements, a workgroup with the lists in global
// memory above.  map_emit_pairs: one wave per buffer, byte stores (images start at odd offsets).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "../../include/sdfs_extent.h"
#include "block_scan.h"
#include "call_support.h"
#include "store_format.h"

namespace sdfs {
namespace {

constexpr uint32_t kLdsWork = 256;  // work-list elements per buffer held in LDS (2 lists, 8 KiB)
constexpr uint32_t kDupBit = 0x80000000u;

struct Work {
    uint32_t src;  // < n0: the buffer's pair, else n0 + the buffer's insert; kDupBit = dup
    int32_t pos, offset, nlen;
};

__device__ __forceinline__ void copy_hash(uint8_t* dst, const uint8_t* src) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = s[k];
}

// a pair list the edits can work on: fields in range, ascending, disjoint
__device__ __forceinline__ uint32_t check_pair(const sdfs_cdc_pairs& p, uint64_t base, uint32_t i, uint32_t n) {
    const int64_t ps = p.pos[base + i], nl = p.nlen[base + i], of = p.offset[base + i];
    uint32_t st = 0;
    if (ps < 0 || nl < 0 || of < 0 || p.len[base + i] < 0 || ps + nl > INT32_MAX || of + nl > INT32_MAX)
        st |= SDFS_CDC_EXT_CORRUPT;
    if (i + 1 < n) {
        const int64_t q = p.pos[base + i + 1];
        if (ps >= q || ps + nl > q) st |= SDFS_CDC_EXT_OVERLAP;
    }
    return st;
}

// --------------------------------------------------------------------------------------- extents

struct ExtArgs {
    sdfs_cdc_pairs src;
    uint32_t nbuf_src, nbuf_dst, chunk_length, n_seg;
    const sdfs_cdc_segment* segs;
    sdfs_cdc_inserts ins;
    uint64_t n_ins_cap;
    uint32_t* seg_cnt;  // [n_seg] scratch
    uint32_t* seg_first;
    uint32_t* seg_status;
};

// number of pairs with pos < x (uniform over the wave)
__device__ __forceinline__ uint32_t lower_pos(const int32_t* pos, uint32_t n, int64_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pos[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// one wave per segment
template <bool EMIT>
__global__ __launch_bounds__(64) void extents_kernel(ExtArgs a) {
    __shared__ uint32_t s_st;
    const uint32_t lane = threadIdx.x;
    const uint32_t s = blockIdx.x;
    const sdfs_cdc_segment g = a.segs[s];
    const int64_t x0 = g.src_off, x1 = (int64_t)g.src_off + g.len;
    if (EMIT) {
        if (a.seg_status[s] || a.seg_first[a.n_seg] > a.n_ins_cap) return;
        const uint64_t base = (uint64_t)g.src_buf * a.src.cap;
        const uint32_t n = min(a.src.counts[g.src_buf], a.src.cap);
        const uint32_t k0 = lower_pos(a.src.pos + base, n, x0 + 1) - 1;  // the largest pos <= x0
        const uint32_t first = a.seg_first[s], cnt = a.seg_first[s + 1] - first;
        for (uint32_t i = lane; i < cnt; i += 64) {
            const uint64_t k = base + k0 + i, o = (uint64_t)first + i;
            const int64_t ps = a.src.pos[k];
            const int64_t lo = max(ps, x0), hi = min(ps + a.src.nlen[k], x1);
            copy_hash(a.ins.hash + o * 32, a.src.hashes + k * 32);
            a.ins.hashloc[o] = a.src.hashloc[k];
            a.ins.len[o] = a.src.len[k];
            a.ins.pos[o] = (int32_t)(g.dst_off + (lo - x0));
            a.ins.offset[o] = (int32_t)(a.src.offset[k] + (lo - ps));
            a.ins.nlen[o] = (int32_t)(hi - lo);
            a.ins.dst_buf[o] = g.dst_buf;
        }
        return;
    }
    if (lane == 0) s_st = 0;
    __syncthreads();
    uint32_t st = 0, cnt = 0;
    if (g.src_buf >= a.nbuf_src || g.dst_buf >= a.nbuf_dst || g.len == 0 || x1 > (int64_t)a.chunk_length ||
        (uint64_t)g.dst_off + g.len > a.chunk_length) {
        st = SDFS_CDC_EXT_SRC;  // not reached: the host refuses such a segment
    } else {
        const uint64_t base = (uint64_t)g.src_buf * a.src.cap;
        const uint32_t n = min(a.src.counts[g.src_buf], a.src.cap);
        uint32_t bad = a.src.status[g.src_buf] != 0;
        for (uint32_t i = lane; i < n; i += 64) bad |= check_pair(a.src, base, i, n);
        if (bad) atomicOr(&s_st, 1u);
        __syncthreads();
        if (s_st) {
            st = SDFS_CDC_EXT_SRC;
        } else {
            const int32_t* pos = a.src.pos + base;
            const int32_t* nlen = a.src.nlen + base;
            const uint32_t k0p = lower_pos(pos, n, x0 + 1), k1p = lower_pos(pos, n, x1);  // k0 + 1, k1 + 1
            uint32_t hole = k0p == 0;
            if (!hole) {
                const uint32_t k0 = k0p - 1, k1 = k1p - 1;
                cnt = k1 - k0 + 1;
                for (uint32_t i = lane; i < cnt; i += 64) {
                    const int64_t e = (int64_t)pos[k0 + i] + nlen[k0 + i];
                    if (i == 0 && e <= x0) hole = 1;
                    if (i + 1 < cnt ? e != pos[k0 + i + 1] : e < x1) hole = 1;
                }
            }
            if (hole) atomicOr(&s_st, 2u);
            __syncthreads();
            if (s_st & 2u) st = SDFS_CDC_EXT_HOLE;
        }
    }
    if (lane == 0) {
        a.seg_cnt[s] = st ? 0 : cnt;
        a.seg_status[s] = st;
    }
}

// ----------------------------------------------------------------------------------- from chunks

struct RunArgs {
    uint32_t n_run;
    sdfs_cdc_dev_out out;
    const uint64_t* hashloc;
    const sdfs_cdc_run* runs;
    sdfs_cdc_inserts ins;
    uint64_t n_ins_cap;
    const uint32_t* run_first;
};

__global__ __launch_bounds__(256) void from_chunks_kernel(RunArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.n_run || a.run_first[a.n_run] > a.n_ins_cap) return;
    const uint32_t n = min(a.out.counts[r], a.out.cap);
    const uint32_t first = a.run_first[r];
    const sdfs_cdc_run run = a.runs[r];
    for (uint32_t i = lane; i < n; i += 64) {
        const uint64_t slot = (uint64_t)r * a.out.cap + i, o = (uint64_t)first + i;
        copy_hash(a.ins.hash + o * 32, a.out.digests + slot * 32);
        a.ins.hashloc[o] = a.hashloc[o];
        a.ins.len[o] = (int32_t)a.out.lens[slot];
        a.ins.pos[o] = (int32_t)(run.run_pos + a.out.starts[slot]);
        a.ins.offset[o] = 0;
        a.ins.nlen[o] = (int32_t)a.out.lens[slot];
        a.ins.dst_buf[o] = run.dst_buf;
    }
}

// ---------------------------------------------------------------------------------------- insert

struct InsArgs {
    uint32_t nbuf, chunk_length, slot_pairs;
    sdfs_cdc_pairs in;
    sdfs_cdc_inserts ins;
    uint64_t n_ins;
    const uint32_t* ins_first;
    sdfs_cdc_pairs out;
    uint8_t* out_dup;
    uint32_t* status;
    uint32_t* need;       // [nbuf + 1] counts + 2 * inserts, then its prefix
    uint32_t* need_first; // [nbuf + 1]
    Work* work;           // 2 lists per buffer, at 2 * need_first[b]
    uint64_t work_total;  // elements of one list over all buffers
};

__device__ __forceinline__ void buffer_inserts(const InsArgs& a, uint32_t b, uint32_t& f0, uint32_t& m) {
    const uint64_t lo = min<uint64_t>(a.ins_first[b], a.n_ins);
    const uint64_t hi = min<uint64_t>(max<uint64_t>(a.ins_first[b + 1], lo), a.n_ins);
    f0 = (uint32_t)lo;
    m = (uint32_t)(hi - lo);
}

__global__ __launch_bounds__(256) void insert_need_kernel(InsArgs a) {
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= a.nbuf) return;
    uint32_t f0, m;
    buffer_inserts(a, b, f0, m);
    a.need[b] = min(a.in.counts[b], a.in.cap) + 2 * m;
}

template <bool LDS>
__global__ __launch_bounds__(LDS ? 64 : 256) void map_insert_kernel(InsArgs a) {
    constexpr uint32_t NT = LDS ? 64 : 256;
    __shared__ Work s_a[LDS ? kLdsWork : 1], s_b[LDS ? kLdsWork : 1];
    __shared__ uint32_t s_st, s_doop;
    const uint32_t tid = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const uint32_t n0 = min(a.in.counts[b], a.in.cap);
    uint32_t f0, m;
    buffer_inserts(a, b, f0, m);
    if ((n0 + 2 * m <= kLdsWork) != LDS) return;  // the other kernel's buffer (uniform)
    const uint64_t ib = (uint64_t)b * a.in.cap, ob = (uint64_t)b * a.out.cap;
    if (tid == 0) {
        s_st = a.in.status[b] ? SDFS_CDC_EXT_CORRUPT : 0;
        s_doop = 0;
    }
    __syncthreads();
    uint32_t bad = 0;
    for (uint32_t i = tid; i < n0; i += NT) bad |= check_pair(a.in, ib, i, n0);
    for (uint32_t j = tid; j < m; j += NT) {
        const uint64_t k = (uint64_t)f0 + j;
        const int64_t ps = a.ins.pos[k], nl = a.ins.nlen[k], of = a.ins.offset[k];
        if (nl <= 0 || ps < 0 || of < 0 || a.ins.len[k] < 0 || ps + nl > (int64_t)a.chunk_length || of + nl > INT32_MAX)
            bad |= SDFS_CDC_EXT_BAD_INSERT;
    }
    // d_ins_first that does not ascend: the buffer's lists would not lie inside the scratch
    if (!LDS && (uint64_t)a.need_first[b] + n0 + 2 * m > a.work_total) bad |= SDFS_CDC_EXT_BAD_INSERT;
    if (bad) atomicOr(&s_st, bad);
    __syncthreads();
    uint32_t st = s_st;
    if (st || m == 0) {  // copied through
        if (n0 > a.out.cap) st |= SDFS_CDC_EXT_ECAP;
        else
            for (uint32_t i = tid; i < n0; i += NT) {
                copy_hash(a.out.hashes + (ob + i) * 32, a.in.hashes + (ib + i) * 32);
                a.out.hashloc[ob + i] = a.in.hashloc[ib + i];
                a.out.len[ob + i] = a.in.len[ib + i];
                a.out.pos[ob + i] = a.in.pos[ib + i];
                a.out.offset[ob + i] = a.in.offset[ib + i];
                a.out.nlen[ob + i] = a.in.nlen[ib + i];
                a.out_dup[ob + i] = 0;
            }
        if (!st && n0 > a.slot_pairs) st = SDFS_CDC_EXT_OVERFLOW;
        if (tid == 0) {
            a.out.counts[b] = n0;
            a.out.doop[b] = 0;
            a.out.flags[b] = a.in.flags[b];
            a.out.status[b] = st;
            a.status[b] = st;
        }
        return;
    }
    Work* cur = LDS ? s_a : a.work + 2 * (uint64_t)a.need_first[b];
    Work* nxt = LDS ? s_b : cur + (n0 + 2 * m);
    for (uint32_t i = tid; i < n0; i += NT)
        cur[i] = Work{i, a.in.pos[ib + i], a.in.offset[ib + i], a.in.nlen[ib + i]};
    __syncthreads();
    uint32_t n = n0;
    for (uint32_t j = 0; j < m; j++) {
        const uint64_t k = (uint64_t)f0 + j;
        const int32_t P = a.ins.pos[k], E = P + a.ins.nlen[k];  // E <= chunk_length
        uint32_t lo = 0, hi = n;  // L = the pairs with pos < P
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (cur[mid].pos < P) lo = mid + 1;
            else hi = mid;
        }
        const uint32_t L = lo;
        hi = n;  // R = the first pair at or after L that survives: it reaches past E (an empty one: lies past E)
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            const Work w = cur[mid];
            if (w.nlen > 0 ? w.pos + w.nlen > E : w.pos > E) hi = mid;
            else lo = mid + 1;
        }
        const uint32_t R = lo;
        const uint32_t tail = L > 0 && cur[L - 1].pos + cur[L - 1].nlen > E;
        const uint32_t shift = L + 1 + tail;
        for (uint32_t i = tid; i < n; i += NT) {
            Work w = cur[i];
            if (i < L) {
                if (i == L - 1 && tail) {  // split: the clone takes [E, hep)
                    const int32_t d = E - w.pos;
                    nxt[L + 1] = Work{w.src | kDupBit, E, w.offset + d, w.nlen - d};
                }
                if (w.pos + w.nlen > P) w.nlen = P - w.pos;  // tail trimmed / the split's head
                nxt[i] = w;
            } else if (i >= R) {
                if (w.pos < E) {  // head trimmed
                    const int32_t d = E - w.pos;
                    w.pos = E;
                    w.offset += d;
                    w.nlen -= d;
                }
                nxt[shift + (i - R)] = w;
            }
        }
        if (tid == 0) nxt[L] = Work{n0 + j, P, a.ins.offset[k], a.ins.nlen[k]};
        n = shift + (n - R);
        __syncthreads();
        Work* t = cur;
        cur = nxt;
        nxt = t;
    }
    if (n > a.out.cap) {  // nothing of this buffer is written
        if (tid == 0) {
            a.out.counts[b] = n;
            a.out.status[b] = a.status[b] = SDFS_CDC_EXT_ECAP;
        }
        return;
    }
    uint32_t doop = 0;
    for (uint32_t i = tid; i < n; i += NT) {
        const Work w = cur[i];
        const uint32_t src = w.src & ~kDupBit, dup = w.src >> 31;
        if (src < n0) {
            copy_hash(a.out.hashes + (ob + i) * 32, a.in.hashes + (ib + src) * 32);
            a.out.hashloc[ob + i] = a.in.hashloc[ib + src];
            a.out.len[ob + i] = a.in.len[ib + src];
        } else {
            const uint64_t k = (uint64_t)f0 + (src - n0);
            copy_hash(a.out.hashes + (ob + i) * 32, a.ins.hash + k * 32);
            a.out.hashloc[ob + i] = a.ins.hashloc[k];
            a.out.len[ob + i] = a.ins.len[k];
        }
        a.out.pos[ob + i] = w.pos;
        a.out.offset[ob + i] = w.offset;
        a.out.nlen[ob + i] = w.nlen;
        a.out_dup[ob + i] = (uint8_t)dup;
        if (dup) doop += (uint32_t)w.nlen;
    }
    if (doop) atomicAdd(&s_doop, doop);
    __syncthreads();
    if (tid == 0) {
        st = n > a.slot_pairs ? SDFS_CDC_EXT_OVERFLOW : 0;
        a.out.counts[b] = n;
        a.out.doop[b] = s_doop;
        a.out.flags[b] = a.in.flags[b];
        a.out.status[b] = st;
        a.status[b] = st;
    }
}

// ------------------------------------------------------------------------------------ emit pairs

struct EmitArgs {
    uint32_t nbuf;
    sdfs_cdc_pairs p;
    uint32_t hash_len;
    const uint8_t* dup;
    const uint32_t* status;
    uint8_t flags;
    uint8_t* map;
    uint32_t slot_bytes;
    uint32_t* doop;
    uint32_t* skipped;
};

// one wave per buffer, four per block, as map_emit_kernel
__global__ __launch_bounds__(256) void emit_pairs_kernel(EmitArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= a.nbuf) return;
    const uint32_t n = a.p.counts[b];
    if ((a.status && a.status[b]) || slot_need(n, a.hash_len) > a.slot_bytes || n > a.p.cap) {
        if (lane == 0) atomicAdd(a.skipped, 1u);
        return;
    }
    uint8_t* img = a.map + (uint64_t)b * a.slot_bytes;
    const uint64_t base = (uint64_t)b * a.p.cap;
    uint32_t doop = 0;
    for (uint32_t i = lane; i < n; i += 64) {
        const uint64_t slot = base + i;
        const uint32_t nl = (uint32_t)a.p.nlen[slot];
        put_pair_record(img, i, a.hash_len, a.p.hashes + slot * 32, a.p.hashloc[slot], (uint32_t)a.p.len[slot],
                        (uint32_t)a.p.pos[slot], (uint32_t)a.p.offset[slot], nl);
        if (a.dup && a.dup[slot]) doop += nl;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) doop += __shfl_xor(doop, o);
    if (lane == 0) {
        put_slot_frame(img, a.flags, n, a.hash_len, doop);
        if (a.doop) a.doop[b] = doop;
    }
}

// ------------------------------------------------------------------------------------------ host

bool inserts_complete(const sdfs_cdc_inserts* i) {
    return i && i->hash && i->hashloc && i->len && i->pos && i->offset && i->nlen && i->dst_buf;
}

}  // namespace
}  // namespace sdfs

using namespace sdfs;

extern "C" {

int sdfs_cdc_map_extents(int device, uint32_t nbuf_src, const sdfs_cdc_pairs* src, uint32_t nbuf_dst,
                         uint32_t chunk_length, uint32_t n_seg, const sdfs_cdc_segment* h_segs,
                         const sdfs_cdc_segment* d_segs, const sdfs_cdc_inserts* ins, uint64_t n_ins_cap,
                         uint32_t* d_seg_first, uint32_t* d_seg_status, void* stream) {
    if (!pairs_complete(src)) return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_pairs");
    if (!inserts_complete(ins)) return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_inserts");
    if (const int rc = check_chunk_length(chunk_length)) return rc;
    if (!d_seg_first || (n_seg && (!h_segs || !d_segs || !d_seg_status))) return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_seg >= (uint32_t)INT32_MAX) return fail_status(SDFS_CDC_EINVAL, "%u segments: split the batch", n_seg);
    for (uint32_t s = 0; s < n_seg; s++) {
        const sdfs_cdc_segment& g = h_segs[s];
        if (g.len < 1 || g.src_buf >= nbuf_src || g.dst_buf >= nbuf_dst || (uint64_t)g.src_off + g.len > chunk_length ||
            (uint64_t)g.dst_off + g.len > chunk_length)
            return fail_status(SDFS_CDC_EINVAL,
                               "segment %u {src %u + %u, dst %u + %u, len %u}: not inside one buffer of %u / %u, "
                               "chunk_length %u",
                               s, g.src_buf, g.src_off, g.dst_buf, g.dst_off, g.len, nbuf_src, nbuf_dst, chunk_length);
    }
    if (const int rc = set_device(device)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (n_seg == 0) {
        SDFS_TRY(hipMemsetAsync(d_seg_first, 0, 4, st));
        return SDFS_CDC_OK;
    }
    Scratch sc(st);
    ExtArgs a{*src, nbuf_src, nbuf_dst, chunk_length, n_seg, d_segs, *ins, n_ins_cap, nullptr, d_seg_first, d_seg_status};
    SDFS_TRY(sc.get(&a.seg_cnt, n_seg));
    hipLaunchKernelGGL(extents_kernel<false>, dim3(n_seg), dim3(64), 0, st, a);
    hipLaunchKernelGGL(prefix_kernel<uint32_t>, dim3(1), dim3(1024), 0, st, a.seg_cnt, n_seg, d_seg_first);
    hipLaunchKernelGGL(extents_kernel<true>, dim3(n_seg), dim3(64), 0, st, a);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_map_inserts_from_chunks(int device, uint32_t n_run, const sdfs_cdc_dev_out* out, uint32_t run_len,
                                     const uint64_t* d_hashloc, uint32_t nbuf_dst, uint32_t chunk_length,
                                     const sdfs_cdc_run* h_runs, const sdfs_cdc_run* d_runs,
                                     const sdfs_cdc_inserts* ins, uint64_t n_ins_cap, uint32_t* d_run_first,
                                     void* stream) {
    if (!out || !out->counts || !out->starts || !out->lens || !out->digests || !out->cap)
        return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_dev_out");
    if (!inserts_complete(ins)) return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_inserts");
    if (const int rc = check_chunk_length(chunk_length)) return rc;
    if (!d_run_first || (n_run && (!h_runs || !d_runs || !d_hashloc))) return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_run >= (uint32_t)INT32_MAX) return fail_status(SDFS_CDC_EINVAL, "%u runs: split the batch", n_run);
    if (run_len < 1 || run_len > chunk_length)
        return fail_status(SDFS_CDC_EINVAL, "run_len %u: 1 .. chunk_length %u", run_len, chunk_length);
    for (uint32_t r = 0; r < n_run; r++)
        if (h_runs[r].dst_buf >= nbuf_dst || (uint64_t)h_runs[r].run_pos + run_len > chunk_length)
            return fail_status(SDFS_CDC_EINVAL, "run %u {buffer %u of %u, pos %u} + %u bytes: outside the buffer (%u)", r,
                               h_runs[r].dst_buf, nbuf_dst, h_runs[r].run_pos, run_len, chunk_length);
    if (const int rc = set_device(device)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(prefix_kernel<uint32_t>, dim3(1), dim3(1024), 0, st, out->counts, n_run, d_run_first);
    if (n_run) {
        RunArgs a{n_run, *out, d_hashloc, d_runs, *ins, n_ins_cap, d_run_first};
        hipLaunchKernelGGL(from_chunks_kernel, dim3((n_run + 3) / 4), dim3(256), 0, st, a);
    }
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_map_insert(int device, uint32_t nbuf, uint32_t chunk_length, uint32_t slot_pairs,
                        const sdfs_cdc_pairs* in, const sdfs_cdc_inserts* ins, uint64_t n_ins,
                        const uint32_t* d_ins_first, const sdfs_cdc_pairs* out, uint8_t* d_out_dup,
                        uint32_t* d_status, void* stream) {
    if (!pairs_complete(in) || !pairs_complete(out)) return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_pairs");
    if (n_ins && !inserts_complete(ins)) return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_inserts");
    if (!ins) return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (const int rc = check_chunk_length(chunk_length)) return rc;
    if (nbuf && (!d_ins_first || !d_out_dup || !d_status)) return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (in->pos == out->pos || in->hashes == out->hashes || in->counts == out->counts)
        return fail_status(SDFS_CDC_EINVAL, "out shares arrays with in");
    const uint64_t work = (uint64_t)nbuf * in->cap + 2 * n_ins;
    if (n_ins >= (1ull << 30) || work >= (1ull << 31))
        return fail_status(SDFS_CDC_EINVAL, "%u buffers of %u pairs and %llu inserts: split the batch", nbuf, in->cap,
                           (unsigned long long)n_ins);
    if (nbuf == 0) return SDFS_CDC_OK;
    if (const int rc = set_device(device)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    Scratch sc(st);
    InsArgs a{nbuf, chunk_length, slot_pairs, *in, *ins, n_ins, d_ins_first, *out, d_out_dup, d_status,
              nullptr, nullptr, nullptr, work};
    SDFS_TRY(sc.get(&a.need, (size_t)nbuf + 1));
    SDFS_TRY(sc.get(&a.need_first, (size_t)nbuf + 1));
    SDFS_TRY(sc.get(&a.work, (size_t)work * 2));
    hipLaunchKernelGGL(insert_need_kernel, dim3((nbuf + 255) / 256), dim3(256), 0, st, a);
    hipLaunchKernelGGL(prefix_kernel<uint32_t>, dim3(1), dim3(1024), 0, st, a.need, nbuf, a.need_first);
    hipLaunchKernelGGL(map_insert_kernel<true>, dim3(nbuf), dim3(64), 0, st, a);
    hipLaunchKernelGGL(map_insert_kernel<false>, dim3(nbuf), dim3(256), 0, st, a);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_map_emit_pairs(int device, uint32_t nbuf, const sdfs_cdc_pairs* pairs, uint32_t hash_len,
                            const uint8_t* d_dup, const uint32_t* d_status, uint8_t flags, uint8_t* d_map,
                            uint32_t slot_bytes, uint32_t* d_doop, uint32_t* d_skipped, void* stream) {
    if (!pairs_complete(pairs)) return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_pairs");
    if (const int rc = check_hash_len(hash_len, HashOf::kPair)) return rc;
    if (slot_bytes < kSlotFixedBytes) return fail_status(SDFS_CDC_EINVAL, "slot_bytes %u < 13", slot_bytes);
    if (nbuf && (!d_map || !d_skipped)) return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (nbuf == 0) return SDFS_CDC_OK;
    if (const int rc = set_device(device)) return rc;
    EmitArgs a{nbuf, *pairs, hash_len, d_dup, d_status, flags, d_map, slot_bytes, d_doop, d_skipped};
    hipLaunchKernelGGL(emit_pairs_kernel, dim3((nbuf + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

}  // extern "C"
