// map_import.hip — a map file of another volume becomes a file of this one (include/sdfs_import.h;
// DESIGN.md §24).
//
// Slot images whose hashlocs belong to the source volume are accepted by slot_walk_check
// (store_format.h), their pairs laid out by image place, and after the index has said which
// fingerprints it holds:
//   pairs    — validate (a wave per request), then layout (a wave per 256 pairs of a request):
//              hash, source hashloc and the counting flag of every place;
//   plan     — miss (a thread per place: EMISSING), mark (the directory entries the clean requests
//              want), then count / scan / assign over the directory on all CUs: per-block sums, one
//              small scan of the sums, a pass that writes the fetches; remap (entry -> fetch);
//   records  — [lens -> hash_device] -> decide (EFETCH / EHASH), then count / scan / assign over
//              the places: the accepted requests' counting pairs as fingerprint records;
//   install  — a workgroup per (request, 16 KiB of its slot): the image to its destination slot in
//              16-byte vectors, the hashlocs patched in registers on the way.
// Every phase that reads what another workgroup wrote is its own kernel on the same stream; a
// request's status word is final when the kernel that writes it has finished.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/sdfs_import.h"
#include "block_scan.h"
#include "call_support.h"
#include "cdc_internal.h"
#include "store_format.h"

namespace sdfs {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kBlock = SDFS_CDC_IMPORT_BLOCK;
constexpr uint32_t kSpan = SDFS_CDC_IMPORT_SPAN;
constexpr uint32_t kNone = SDFS_CDC_IMPORT_NONE;
static_assert(kBlock == 1024, "a scan block is 1024 threads, 16 waves");
static_assert(kSpan % 16 == 0, "a span is whole vectors");

using Work = sdfs_cdc_import_work;

// ---------------------------------------------------------------------------------------- pairs

struct PairsArgs {
    const uint8_t* req;
    uint64_t nreq;
    uint32_t slot_bytes;
    uint32_t hash_len;
    uint32_t pair_stride;
    uint32_t parts;  // waves per request in the layout
    Work w;
    uint32_t* meta;  // [nreq] scratch: slot_meta
};

// a wave per request (every branch is wave-uniform)
__global__ __launch_bounds__(kThreads) void imp_validate_kernel(PairsArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t r = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (r >= a.nreq) return;
    const SlotWalk w = slot_walk_check(a.req + r * a.slot_bytes, a.slot_bytes, a.hash_len, lane);
    if (lane == 0) {
        a.w.status[r] = w.status;
        a.w.req_pairs[r] = w.n;
        a.w.req_missed[r] = 0;
        a.meta[r] = slot_meta(w);
    }
}

// a wave per (request, kSlotPart places): every place of the request is written, the ones past its
// pairs with zeros.  HW: words of a pair's hash (8 = SHA-256, 4 = MD5).
template <int HW>
__global__ __launch_bounds__(kThreads) void imp_layout_kernel(PairsArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t unit = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const uint64_t r = unit / a.parts;
    if (r >= a.nreq) return;  // wave-uniform
    const uint32_t meta = a.meta[r];
    const uint32_t n = slot_meta_pairs(meta);  // <= pair_cap(slot_bytes) <= pair_stride
    const uint32_t i0 = (uint32_t)(unit % a.parts) * kSlotPart;
    const uint32_t i1 = min(a.pair_stride, i0 + kSlotPart);
    constexpr uint32_t hl = HW * 4;
    const uint8_t* img = a.req + r * a.slot_bytes;
    for (uint32_t i = i0 + lane; i < i1; i += 64) {
        const uint64_t place = r * a.pair_stride + i;
        uint4 ka = make_uint4(0, 0, 0, 0), kb = ka;
        uint64_t hashloc = 0;
        bool on = false;
        if (i < n) {
            load_pair_key<HW>(img, i, ka, kb, hashloc);
            on = !(slot_meta_unsorted(meta) && pair_superseded(img, i, n, hl));
        }
        uint4* h = reinterpret_cast<uint4*>(a.w.hashes + place * 32);
        h[0] = ka;
        h[1] = kb;
        a.w.src_hashloc[place] = hashloc;
        a.w.counting[place] = on ? 1 : 0;
    }
}

// ----------------------------------------------------------------------------------------- plan

struct PlanArgs {
    uint64_t places;
    uint32_t pair_stride;
    Work w;
    const uint64_t* pos;  // index_get's answer per place
    uint64_t src_pos_base;
    uint64_t n_src;
    const uint64_t* store_off;
    const uint32_t* store_len;
    const uint32_t* store_raw;
    uint32_t max_chunk;
    uint32_t* fetch_count;
    uint64_t* src_off;
    uint32_t* src_len;
    uint64_t* dst_off;
    uint32_t* dst_cap;
    uint64_t* plain_off;
    uint64_t* total_bytes;
    uint32_t* mark;   // [n_src] 1 = wanted, then its fetch index
    uint32_t* bcnt;   // [nblocks] wanted entries of the block, then those before it
    uint64_t* bdst;   // [nblocks] chunk-area bytes likewise
    uint64_t* bplain; // [nblocks] decrypted-area bytes likewise
    uint32_t nblocks;
};

__device__ __forceinline__ bool wanted_at(const PlanArgs& a, uint64_t place) {
    return a.w.counting[place] && a.pos[place] == UINT64_MAX;
}

// a thread per place: a wanted pair must name a live directory entry (every number is compared
// with its bound before it is used as an index)
__global__ __launch_bounds__(kThreads) void imp_miss_kernel(PlanArgs a) {
    const uint64_t place = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    uint32_t miss = 0;
    if (place < a.places && wanted_at(a, place)) {
        const uint64_t k = a.w.src_hashloc[place] - a.src_pos_base;
        bool ok = k < a.n_src;
        if (ok) {
            const uint32_t raw = a.store_raw[k];
            ok = a.store_len[k] != 0 && raw != 0 && raw <= a.max_chunk;
        }
        if (!ok) {
            const uint64_t r = place / a.pair_stride;
            atomicAdd(&a.w.req_missed[r], 1u);
            atomicOr(&a.w.status[r], SDFS_CDC_IMPORT_EMISSING);
            miss = 1;
        }
    }
    const uint32_t m = (uint32_t)__popcll(__ballot(miss));
    if (m && (threadIdx.x & 63) == 0) add64(&a.w.counts[7], m);
}

// the miss pass has finished: a request that is still clean marks what it wants
__global__ __launch_bounds__(kThreads) void imp_mark_kernel(PlanArgs a) {
    const uint64_t place = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (place >= a.places) return;
    uint32_t f = kNone;
    if (wanted_at(a, place) && a.w.status[place / a.pair_stride] == 0) {
        f = (uint32_t)(a.w.src_hashloc[place] - a.src_pos_base);  // < n_src < 2^32: the miss pass checked it
        a.mark[f] = 1;
    }
    a.w.pair_fetch[place] = f;
}

// what directory entry k adds to the three running sums
__device__ __forceinline__ void dir_terms(const PlanArgs& a, uint64_t k, uint32_t& on, uint32_t& raw, uint32_t& sl,
                                          uint64_t& d, uint64_t& p) {
    on = k < a.n_src && a.mark[k] != 0;
    raw = on ? a.store_raw[k] : 0;
    sl = on ? a.store_len[k] : 0;
    d = ((uint64_t)raw + 15) & ~15ull;
    p = ((uint64_t)sl + 15) & ~15ull;
}

// count: per block of kBlock directory entries
__global__ __launch_bounds__(kBlock) void imp_dir_count_kernel(PlanArgs a) {
    __shared__ uint64_t lds[3][16];
    const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t on, raw, sl;
    uint64_t d, p;
    dir_terms(a, k, on, raw, sl, d, p);
    const uint64_t c = wave_sum<uint64_t>(on), sd = wave_sum(d), sp = wave_sum(p);  // sums alone: no scan
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
        lds[0][wv] = c;
        lds[1][wv] = sd;
        lds[2][wv] = sp;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t tc = 0, td = 0, tp = 0;
        for (uint32_t i = 0; i < 16; i++) {
            tc += lds[0][i];
            td += lds[1][i];
            tp += lds[2][i];
        }
        a.bcnt[blockIdx.x] = (uint32_t)tc;
        a.bdst[blockIdx.x] = td;
        a.bplain[blockIdx.x] = tp;
    }
}

// scan: one block over the block sums, which become the sums before each block; the totals
__global__ __launch_bounds__(kBlock) void imp_dir_scan_kernel(PlanArgs a) {
    __shared__ uint64_t lds[16];
    const uint64_t cc = block_sums_to_bases(a.bcnt, a.nblocks, reinterpret_cast<uint32_t*>(lds));
    const uint64_t cd = block_sums_to_bases(a.bdst, a.nblocks, lds);
    const uint64_t cp = block_sums_to_bases(a.bplain, a.nblocks, lds);
    if (threadIdx.x == 0) {
        *a.fetch_count = (uint32_t)cc;
        a.total_bytes[0] = cd;
        a.total_bytes[1] = cp;
        a.w.counts[2] = cc;
    }
}

// assign: the wanted entries of a block get their fetches
__global__ __launch_bounds__(kBlock) void imp_dir_assign_kernel(PlanArgs a) {
    __shared__ uint64_t lds[3][16];
    const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t on, raw, sl;
    uint64_t d, p;
    dir_terms(a, k, on, raw, sl, d, p);
    uint64_t ex[3] = {on, d, p}, total[3];
    block_exclusive_scan_1024(ex, lds, total);
    if (on) {
        const uint32_t f = a.bcnt[blockIdx.x] + (uint32_t)ex[0];
        a.src_off[f] = a.store_off[k];
        a.src_len[f] = sl;
        a.dst_off[f] = a.bdst[blockIdx.x] + ex[1];
        a.dst_cap[f] = raw;
        if (a.plain_off) a.plain_off[f] = a.bplain[blockIdx.x] + ex[2];
        a.mark[k] = f;
    }
    const uint64_t rawsum = wave_sum<uint64_t>(raw);
    if (rawsum && (threadIdx.x & 63) == 0) add64(&a.w.counts[3], rawsum);
}

__global__ __launch_bounds__(kThreads) void imp_remap_kernel(PlanArgs a) {
    const uint64_t place = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (place >= a.places) return;
    const uint32_t k = a.w.pair_fetch[place];
    if (k != kNone) a.w.pair_fetch[place] = a.mark[k];
}

// -------------------------------------------------------------------------------------- records

struct RecArgs {
    uint64_t places;
    uint32_t pair_stride;
    uint32_t hash_len;
    Work w;
    const uint32_t* fetch_count;
    uint64_t n_fetch;
    const uint32_t* dst_cap;
    const uint32_t* fetch_len;
    const uint8_t* digests;  // [n_fetch x 32] or NULL
    uint8_t* records;
    uint32_t* count;
    uint32_t* bsum;   // [nblocks] records of the block, then those before it
    uint32_t* bheld;  // [nblocks] held pairs among them
    uint32_t nblocks;
};

// the lengths hash_device takes: 0 for a fetch that did not come out whole
__global__ __launch_bounds__(kThreads) void imp_hash_lens_kernel(RecArgs a, uint32_t* lens) {
    const uint64_t f = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= a.n_fetch) return;
    const bool live = f < *a.fetch_count && a.fetch_len[f] == a.dst_cap[f];
    lens[f] = live ? a.dst_cap[f] : 0;
}

// the decision: a thread per place; nothing is emitted before this kernel has finished
__global__ __launch_bounds__(kThreads) void imp_decide_kernel(RecArgs a) {
    const uint64_t place = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (place >= a.places) return;
    const uint32_t f = a.w.pair_fetch[place];
    if (f == kNone || f >= a.n_fetch) return;
    uint32_t bit = 0;
    if (f >= *a.fetch_count || a.fetch_len[f] != a.dst_cap[f]) {
        bit = SDFS_CDC_IMPORT_EFETCH;
    } else if (a.digests) {
        const uint32_t* h = reinterpret_cast<const uint32_t*>(a.w.hashes + place * 32);
        const uint32_t* d = reinterpret_cast<const uint32_t*>(a.digests + (uint64_t)f * 32);
        uint32_t diff = 0;
        for (uint32_t k = 0; k < a.hash_len / 4; k++) diff |= h[k] ^ d[k];
        if (diff) bit = SDFS_CDC_IMPORT_EHASH;
    }
    if (bit) atomicOr(&a.w.status[place / a.pair_stride], bit);
}

__device__ __forceinline__ bool emits(const RecArgs& a, uint64_t place) {
    return place < a.places && a.w.counting[place] && a.w.status[place / a.pair_stride] == 0;
}

// count: per block of kBlock places (two ballots, no scan: see block_exclusive_scan_1024)
__global__ __launch_bounds__(kBlock) void imp_rec_count_kernel(RecArgs a) {
    __shared__ uint32_t lds[2][16];
    const uint64_t place = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool on = emits(a, place);
    const bool held = on && a.w.pair_fetch[place] == kNone;
    const uint32_t c = (uint32_t)__popcll(__ballot(on)), h = (uint32_t)__popcll(__ballot(held));
    if ((threadIdx.x & 63) == 0) {
        lds[0][threadIdx.x >> 6] = c;
        lds[1][threadIdx.x >> 6] = h;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tc = 0, th = 0;
        for (uint32_t i = 0; i < 16; i++) {
            tc += lds[0][i];
            th += lds[1][i];
        }
        a.bsum[blockIdx.x] = tc;
        a.bheld[blockIdx.x] = th;
    }
}

// scan: one block over the block sums
__global__ __launch_bounds__(kBlock) void imp_rec_scan_kernel(RecArgs a) {
    __shared__ uint32_t lds[16];
    const uint64_t carry = block_sums_to_bases(a.bsum, a.nblocks, lds);
    uint32_t h = 0, held;  // held pairs <= places < 2^31
    for (uint32_t b = threadIdx.x; b < a.nblocks; b += kBlock) h += a.bheld[b];
    (void)block_exclusive_scan_1024(h, lds, held);
    if (threadIdx.x == 0) {
        *a.count = (uint32_t)carry;
        a.w.counts[0] = carry;
        a.w.counts[1] = held;
    }
}

// assign: the records of a block, in place order
__global__ __launch_bounds__(kBlock) void imp_rec_assign_kernel(RecArgs a) {
    __shared__ uint32_t lds[16];
    const uint64_t place = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool on = emits(a, place);
    uint32_t total;
    const uint32_t ex = block_exclusive_scan_1024<uint32_t>(on ? 1u : 0u, lds, total);
    if (place >= a.places) return;
    if (!on) {
        a.w.pair_rec[place] = kNone;
        return;
    }
    const uint32_t rec = a.bsum[blockIdx.x] + ex;
    a.w.pair_rec[place] = rec;
    const uint32_t f = a.w.pair_fetch[place];
    const uint4* h = reinterpret_cast<const uint4*>(a.w.hashes + place * 32);
    uint4* out = reinterpret_cast<uint4*>(a.records + (uint64_t)rec * kRecordBytes);
    out[0] = h[0];
    out[1] = h[1];
    // u64 buffer_id | start | len: a held pair's chunk is not in the batch
    out[2] = f == kNone ? make_uint4(0, 0, 0, 0) : make_uint4(f, 0u, 0u, a.fetch_len[f]);
}

// -------------------------------------------------------------------------------------- install

struct InstallArgs {
    const uint8_t* req;
    uint64_t nreq;
    uint32_t slot_bytes;
    uint32_t hash_len;
    uint32_t pair_stride;
    Work w;
    const uint64_t* hashloc;  // put_records' answer per record
    const uint64_t* dests;
    const uint32_t* lens;
    uint32_t chunk_length;
    uint8_t* map;
    uint64_t nslots;
    uint64_t* file_len;
};

// blockIdx.x = request, blockIdx.y = span of its slot.  The vectors lie at 16-byte addresses of
// the destination: vector j covers the slot's bytes [16 j - sh, 16 j - sh + 16) with sh = the
// slot's address & 15.  A vector inside the image is four realigned words of the source; the
// hashloc field it overlaps (BAL >= 40 > 16: at most one) is patched in registers; then one
// 16-byte store, or byte stores where the vector leaves the slot.
__global__ __launch_bounds__(kThreads) void imp_install_kernel(InstallArgs a) {
    const uint64_t r = blockIdx.x;
    const bool first = blockIdx.y == 0 && threadIdx.x == 0;
    const uint64_t dest = a.dests[r];
    if (a.w.status[r] != 0 || dest >= a.nslots) {  // uniform over the workgroup
        if (first) add64(&a.w.counts[5], 1);
        return;
    }
    const uint32_t hl = a.hash_len, bal = pair_bytes(hl);
    const uint32_t n = a.w.req_pairs[r];
    const int64_t image = (int64_t)slot_need(n, hl);  // <= slot_bytes: the image parsed
    const int64_t slot = a.slot_bytes;
    const uint8_t* src = a.req + r * a.slot_bytes;
    uint8_t* dst = a.map + dest * a.slot_bytes;
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15);
    const uint32_t nvec = (uint32_t)((sh + (uint64_t)a.slot_bytes + 15) / 16);
    const uint32_t j0 = blockIdx.y * (kSpan / 16), j1 = min(nvec, j0 + kSpan / 16);
    uint32_t changed = 0;
    for (uint32_t j = j0 + threadIdx.x; j < j1; j += kThreads) {
        const int64_t o = (int64_t)j * 16 - sh;  // the slot offset of the vector's first byte
        uint32_t w[4] = {0, 0, 0, 0};
        if (o >= 0 && o + 16 <= image) {
            load_words(src + o, w);
        } else {
            for (int t = 0; t < 16; t++) {
                const int64_t at = o + t;
                if (at >= 0 && at < image) w[t >> 2] |= (uint32_t)src[at] << (8 * (t & 3));
            }
        }
        const int64_t first_loc = (int64_t)kSlotHeaderBytes + hl;  // pair 0's hashloc field
        if (o + 15 >= first_loc) {
            const uint32_t i = (uint32_t)((o + 15 - first_loc) / bal);  // the last pair whose field starts at or before o + 15
            const int64_t hb = first_loc + (int64_t)i * bal;
            const uint64_t place = r * a.pair_stride + i;
            if (i < n && hb + 8 > o && a.w.counting[place]) {
                const uint32_t rec = a.w.pair_rec[place];
                if (rec != kNone) {
                    const uint64_t loc = a.hashloc[rec];
                    if (hb >= o) changed += loc != a.w.src_hashloc[place];  // the vector that holds the field's first byte
#pragma unroll
                    for (int t = 0; t < 16; t++) {
                        const int64_t q = o + t - hb;  // the byte's place in the BE64
                        if (q >= 0 && q < 8) {
                            const uint32_t byte = (uint32_t)(loc >> (8 * (7 - q))) & 255u;
                            w[t >> 2] = (w[t >> 2] & ~(255u << (8 * (t & 3)))) | byte << (8 * (t & 3));
                        }
                    }
                }
            }
        }
        if (o >= 0 && o + 16 <= slot) {
            *reinterpret_cast<uint4*>(dst + o) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            for (int t = 0; t < 16; t++) {
                const int64_t at = o + t;
                if (at >= 0 && at < slot) dst[at] = (uint8_t)(w[t >> 2] >> (8 * (t & 3)));
            }
        }
    }
    changed = wave_sum(changed);
    if (changed && (threadIdx.x & 63) == 0) add64(&a.w.counts[6], changed);
    if (first) {
        add64(&a.w.counts[4], 1);
        atomicMax(reinterpret_cast<unsigned long long*>(a.file_len),
                  (unsigned long long)(dest * a.chunk_length + a.lens[r]));
    }
}

// --------------------------------------------------------------------------------------- checks

bool work_complete(const Work* w) {
    return w && w->hashes && w->src_hashloc && w->counting && w->status && w->req_pairs && w->req_missed &&
           w->pair_fetch && w->pair_rec && w->counts;
}

// what every call of a batch checks: the work arrays, the batch's size, pair_stride
int check_batch(const Work* w, uint64_t nreq, uint32_t pair_stride) {
    if (!w) return fail_status(SDFS_CDC_EINVAL, "null work");
    if (!work_complete(w)) return fail_status(SDFS_CDC_EINVAL, "null work array");
    if (pair_stride == 0) return fail_status(SDFS_CDC_EINVAL, "pair_stride 0");
    if (nreq >= (1ull << 31) || nreq * pair_stride >= (1ull << 31))
        return fail_status(SDFS_CDC_EINVAL, "%llu requests of %u places: split the batch", (unsigned long long)nreq,
                           pair_stride);
    if (reinterpret_cast<uintptr_t>(w->hashes) & 15) return fail_status(SDFS_CDC_EINVAL, "hashes are 16-byte aligned");
    return SDFS_CDC_OK;
}

int check_slots(uint32_t slot_bytes, uint32_t hash_len, uint32_t pair_stride) {
    if (const int rc = check_hash_len(hash_len, HashOf::kPair)) return rc;
    if (slot_bytes < kSlotFixedBytes) return fail_status(SDFS_CDC_EINVAL, "slot_bytes %u < 13", slot_bytes);
    if (pair_stride < pair_cap(slot_bytes, hash_len))
        return fail_status(SDFS_CDC_EINVAL, "pair_stride %u < the %u pairs a slot of %u bytes holds", pair_stride,
                           pair_cap(slot_bytes, hash_len), slot_bytes);
    return SDFS_CDC_OK;
}

dim3 grid_of(uint64_t n, uint32_t per) { return dim3((uint32_t)((n + per - 1) / per)); }

}  // namespace
}  // namespace sdfs

using namespace sdfs;

extern "C" {

int sdfs_cdc_import_pairs(int device, const uint8_t* d_req, uint64_t nreq, uint32_t slot_bytes, uint32_t hash_len,
                          uint32_t pair_stride, const sdfs_cdc_import_work* w, void* stream) {
    if (const int rc = check_slots(slot_bytes, hash_len, pair_stride)) return rc;
    if (const int rc = check_batch(w, nreq, pair_stride)) return rc;
    if (nreq && !d_req) return fail_status(SDFS_CDC_EINVAL, "null requests");
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    SDFS_TRY(hipMemsetAsync(w->counts, 0, 8 * sizeof(uint64_t), s));
    if (nreq == 0) return SDFS_CDC_OK;
    Scratch sc(s);
    PairsArgs a{d_req, nreq, slot_bytes, hash_len, pair_stride, slot_parts(pair_stride), *w, nullptr};
    SDFS_TRY(sc.get(&a.meta, (size_t)nreq));
    hipLaunchKernelGGL(imp_validate_kernel, grid_of(nreq, kThreads / 64), dim3(kThreads), 0, s, a);
    const dim3 g = grid_of(nreq * a.parts, kThreads / 64);
    if (hash_len == 32) hipLaunchKernelGGL(imp_layout_kernel<8>, g, dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL(imp_layout_kernel<4>, g, dim3(kThreads), 0, s, a);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_import_plan(int device, uint64_t nreq, uint32_t pair_stride, const sdfs_cdc_import_work* w,
                         const uint64_t* d_pos, uint64_t src_pos_base, uint64_t n_src, const uint64_t* d_store_off,
                         const uint32_t* d_store_len, const uint32_t* d_store_raw_len, uint32_t max_chunk,
                         uint32_t* d_fetch_count, uint64_t* d_src_off, uint32_t* d_src_len, uint64_t* d_dst_off,
                         uint32_t* d_dst_cap, uint64_t* d_plain_off, uint64_t* d_total_bytes, void* stream) {
    if (const int rc = check_batch(w, nreq, pair_stride)) return rc;
    if (!d_fetch_count || !d_total_bytes || (nreq && !d_pos)) return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_src && (!d_store_off || !d_store_len || !d_store_raw_len || !d_src_off || !d_src_len || !d_dst_off ||
                  !d_dst_cap))
        return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_src >= (1ull << 31))
        return fail_status(SDFS_CDC_EINVAL, "n_src %llu: fetch indices are 32-bit", (unsigned long long)n_src);
    if (const int rc = check_chunk_length(max_chunk)) return rc;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    Scratch sc(s);
    PlanArgs a{};
    a.places = nreq * pair_stride;
    a.pair_stride = pair_stride;
    a.w = *w;
    a.pos = d_pos;
    a.src_pos_base = src_pos_base;
    a.n_src = n_src;
    a.store_off = d_store_off;
    a.store_len = d_store_len;
    a.store_raw = d_store_raw_len;
    a.max_chunk = max_chunk;
    a.fetch_count = d_fetch_count;
    a.src_off = d_src_off;
    a.src_len = d_src_len;
    a.dst_off = d_dst_off;
    a.dst_cap = d_dst_cap;
    a.plain_off = d_plain_off;
    a.total_bytes = d_total_bytes;
    a.nblocks = (uint32_t)((n_src + kBlock - 1) / kBlock);
    SDFS_TRY(sc.get(&a.mark, (size_t)n_src));
    SDFS_TRY(sc.get(&a.bcnt, (size_t)a.nblocks));
    SDFS_TRY(sc.get(&a.bdst, (size_t)a.nblocks));
    SDFS_TRY(sc.get(&a.bplain, (size_t)a.nblocks));
    SDFS_TRY(hipMemsetAsync(a.mark, 0, std::max<size_t>(n_src, 1) * 4, s));
    if (a.places) {
        hipLaunchKernelGGL(imp_miss_kernel, grid_of(a.places, kThreads), dim3(kThreads), 0, s, a);
        hipLaunchKernelGGL(imp_mark_kernel, grid_of(a.places, kThreads), dim3(kThreads), 0, s, a);
    }
    if (a.nblocks) hipLaunchKernelGGL(imp_dir_count_kernel, dim3(a.nblocks), dim3(kBlock), 0, s, a);
    hipLaunchKernelGGL(imp_dir_scan_kernel, dim3(1), dim3(kBlock), 0, s, a);
    if (a.nblocks) hipLaunchKernelGGL(imp_dir_assign_kernel, dim3(a.nblocks), dim3(kBlock), 0, s, a);
    if (a.places) hipLaunchKernelGGL(imp_remap_kernel, grid_of(a.places, kThreads), dim3(kThreads), 0, s, a);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_import_records(int device, sdfs_cdc_engine* engine, uint64_t nreq, uint32_t pair_stride,
                            uint32_t hash_len, const sdfs_cdc_import_work* w, const uint32_t* d_fetch_count,
                            uint64_t n_fetch_max, const uint8_t* d_chunks, const uint64_t* d_dst_off,
                            const uint32_t* d_dst_cap, const uint32_t* d_fetch_len, uint8_t* d_records,
                            uint32_t* d_count, void* stream) {
    if (const int rc = check_hash_len(hash_len, HashOf::kPair)) return rc;
    if (const int rc = check_batch(w, nreq, pair_stride)) return rc;
    if (!d_fetch_count || !d_count || (nreq && !d_records))
        return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_fetch_max && (!d_dst_off || !d_dst_cap || !d_fetch_len || !d_chunks))
        return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_fetch_max >= (1ull << 31))
        return fail_status(SDFS_CDC_EINVAL, "n_fetch_max %llu: fetch indices are 32-bit", (unsigned long long)n_fetch_max);
    if (reinterpret_cast<uintptr_t>(d_records) & 15) return fail_status(SDFS_CDC_EINVAL, "records are 16-byte aligned");
    if (engine) {
        const int dl = sdfs_cdc_digest_len(engine);
        if (dl < 0) return fail_status(SDFS_CDC_EINVAL, "not a live engine handle");
        if ((uint32_t)dl != hash_len)
            return fail_status(SDFS_CDC_EINVAL, "engine digests are %d bytes, the pairs hold %u", dl, hash_len);
    }
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    Scratch sc(s);
    RecArgs a{};
    a.places = nreq * pair_stride;
    a.pair_stride = pair_stride;
    a.hash_len = hash_len;
    a.w = *w;
    a.fetch_count = d_fetch_count;
    a.n_fetch = n_fetch_max;
    a.dst_cap = d_dst_cap;
    a.fetch_len = d_fetch_len;
    a.records = d_records;
    a.count = d_count;
    a.nblocks = (uint32_t)((a.places + kBlock - 1) / kBlock);
    SDFS_TRY(sc.get(&a.bsum, (size_t)a.nblocks));
    SDFS_TRY(sc.get(&a.bheld, (size_t)a.nblocks));
    if (engine && n_fetch_max && a.places) {
        uint32_t* lens = nullptr;
        uint8_t* digests = nullptr;
        SDFS_TRY(sc.get(&lens, (size_t)n_fetch_max));
        SDFS_TRY(sc.get(&digests, (size_t)n_fetch_max * 32));
        hipLaunchKernelGGL(imp_hash_lens_kernel, grid_of(n_fetch_max, kThreads), dim3(kThreads), 0, s, a, lens);
        SDFS_TRY(hipGetLastError());
        if (const int rc = sdfs_cdc_hash_device(engine, d_chunks, d_dst_off, lens, d_fetch_count, n_fetch_max, digests, stream))
            return rc;
        if (const int rc = set_device(device)) return rc;
        a.digests = digests;
    }
    if (a.places) {
        hipLaunchKernelGGL(imp_decide_kernel, grid_of(a.places, kThreads), dim3(kThreads), 0, s, a);
        hipLaunchKernelGGL(imp_rec_count_kernel, dim3(a.nblocks), dim3(kBlock), 0, s, a);
    }
    hipLaunchKernelGGL(imp_rec_scan_kernel, dim3(1), dim3(kBlock), 0, s, a);
    if (a.places) hipLaunchKernelGGL(imp_rec_assign_kernel, dim3(a.nblocks), dim3(kBlock), 0, s, a);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_import_install(int device, const uint8_t* d_req, uint64_t nreq, uint32_t slot_bytes, uint32_t hash_len,
                            uint32_t pair_stride, const sdfs_cdc_import_work* w, const uint64_t* d_hashloc,
                            const uint64_t* d_dests, const uint32_t* d_lens, uint32_t chunk_length, uint8_t* d_map,
                            uint64_t nslots, uint64_t* d_file_len, void* stream) {
    if (const int rc = check_slots(slot_bytes, hash_len, pair_stride)) return rc;
    if (const int rc = check_batch(w, nreq, pair_stride)) return rc;
    if (const int rc = check_chunk_length(chunk_length)) return rc;
    if (!d_file_len) return fail_status(SDFS_CDC_EINVAL, "null file length");
    if (nreq && (!d_req || !d_hashloc || !d_dests || !d_lens || !d_map))
        return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (nreq > nslots)
        return fail_status(SDFS_CDC_EINVAL, "%llu requests for a map of %llu slots: destinations are distinct",
                           (unsigned long long)nreq, (unsigned long long)nslots);
    if (nreq == 0) return SDFS_CDC_OK;
    if (const int rc = set_device(device)) return rc;
    const InstallArgs a{d_req,  nreq,    slot_bytes,   hash_len, pair_stride, *w,        d_hashloc,
                        d_dests, d_lens, chunk_length, d_map,    nslots,      d_file_len};
    const uint64_t vectors = ((uint64_t)slot_bytes + 15 + 15) / 16;  // whatever the destination's alignment
    const uint32_t spans = (uint32_t)((vectors + kSpan / 16 - 1) / (kSpan / 16));
    if (spans > 65535) return fail_status(SDFS_CDC_EINVAL, "slot_bytes %u: more than 65535 spans", slot_bytes);
    hipLaunchKernelGGL(imp_install_kernel, dim3((uint32_t)nreq, spans), dim3(kThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), a);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_import_check_dests(const uint64_t* dests, uint64_t nreq, uint64_t nslots) {
    if (nreq && !dests) return fail_status(SDFS_CDC_EINVAL, "null destinations");
    std::vector<uint64_t> d(dests, dests + nreq);
    for (uint64_t r = 0; r < nreq; r++)
        if (d[r] >= nslots)
            return fail_status(SDFS_CDC_EINVAL, "request %llu: destination slot %llu is outside the map's %llu slots",
                               (unsigned long long)r, (unsigned long long)d[r], (unsigned long long)nslots);
    std::sort(d.begin(), d.end());
    for (uint64_t r = 1; r < nreq; r++)
        if (d[r] == d[r - 1])
            return fail_status(SDFS_CDC_EINVAL, "two requests name destination slot %llu", (unsigned long long)d[r]);
    return SDFS_CDC_OK;
}

}  // extern "C"
