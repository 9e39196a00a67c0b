// archive_pack.hip — the chunk store layer on the device (include/sdfs_archive.h): which new
// record goes into which HashBlobArchive, the archive images, their .map images, compaction.
//
// Reference: HashBlobArchive.putChunk (HashBlobArchive.java:1267-1418: the "archive full" rule
// :1305-1316, the record [BE32 hash.length][hash][BE32 len][record] :1399-1411, the map value
// :1334-1350), the header of a VERSION > 0 archive (:1023-1033), SimpleByteArrayLongMap's file
// image and double-hashed insertion (SimpleByteArrayLongMap.java:224-261,427-498,509-539),
// NextPrime.getNextPrimeI (NextPrime.java:56-88) and compact() (:2064-2186).
//
// Plan: one workgroup.  Exclusive prefix P of 8 + hash_len + len over the records; the cut is
// sequential only from archive to archive, so one wave walks the archives with a 64-way search on
// P (first record whose np reaches blocksz, capped by the entry limit); then every thread lays
// out its records.
//
// Pack: destination-driven, the mirror image of read_path.hip's gather.  A workgroup owns 64 KiB
// of the store, cut at absolute 16-byte addresses; the start positions, source offsets and lengths
// of the records that touch its span sit in LDS (<= kPackLdsRecs, else they are searched in global
// memory).  A lane takes one 16-byte vector at a time: floor record by binary search (the previous
// vector's record is tried first), and
//   - the vector lies wholly inside the record's bytes: two aligned 16-byte loads of the source,
//     realigned by a byte shift, one aligned 16-byte store;
//   - else byte by byte: a record header, a record edge, an archive header, padding.
// The first and last vectors of a store whose ends are not 16-byte aligned are stored bytewise.
//
// Map: one workgroup per archive, the owner table (slot -> lowest record ordinal that claimed it)
// in LDS; see sdfs_archive.h for why the parallel build equals the sequential one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "../../include/sdfs_archive.h"
#include "block_scan.h"
#include "call_support.h"
#include "store_format.h"

namespace sdfs {
namespace {

constexpr uint32_t kNone = SDFS_CDC_ARCHIVE_NONE;
constexpr int kPlanThreads = 1024;
constexpr uint32_t kPlanBlocksz = 256;  // per-archive blocksz values a plan takes (the last one is reused)
constexpr int kPackThreads = 256;
constexpr uint32_t kPackVecs = 4096;     // 16-byte vectors per workgroup (64 KiB): 4 groups of 4 per lane
constexpr uint32_t kPackLdsRecs = 1024;  // records of a span staged in LDS (28 KiB)
constexpr int kMapThreads = 1024;
constexpr uint32_t kMapLdsSlots = 15360;  // owner table in LDS (60 KiB): map_size(2 * 0.75 * MAX_HM_SZ + 5) of a compaction fits

// ----------------------------------------------------------------------------------------- plan

struct PlanArgs {
    const uint32_t* rec_len;
    const uint32_t* count;
    uint64_t n_max;
    uint32_t hash_len;
    uint32_t header_bytes;
    uint32_t n_blocksz;
    uint32_t blocksz[kPlanBlocksz];  // by value: no copy to wait for
    uint32_t limit;           // (int)(map_slots * .75)
    sdfs_cdc_archive_layout o;
    uint64_t* prefix;         // [n_max + 1] scratch
    uint32_t* cuts;           // [arc_cap + 1] scratch of the walk
    const uint32_t* fixed_n_arc;  // not NULL: o.arc_first already holds the cuts of *fixed_n_arc archives
};

__global__ __launch_bounds__(kPlanThreads) void archive_plan_kernel(PlanArgs a) {
    __shared__ uint64_t wsum[16];
    __shared__ uint32_t s_narc, s_fail;
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint64_t n = live_count(a.count, a.n_max);
    const uint32_t unit = record_header_bytes(a.hash_len);
    // exclusive prefix of unit + len, tile by tile
    uint64_t carry = 0;
    for (uint64_t i0 = 0; i0 < n; i0 += kPlanThreads) {
        const uint64_t i = i0 + t;
        const uint64_t v = i < n ? (uint64_t)unit + a.rec_len[i] : 0;
        const uint64_t inc = wave_inclusive_scan(v, lane);  // its own scan text: see block_exclusive_scan_1024
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        uint64_t before = carry, tile = 0;
        for (uint32_t w = 0; w < 16; w++) {
            if (w < wave) before += wsum[w];
            tile += wsum[w];
        }
        if (i < n) a.prefix[i] = before + inc - v;
        carry += tile;
        __syncthreads();
    }
    if (t == 0) {
        a.prefix[n] = carry;
        s_fail = 0;
        s_narc = 0;
    }
    __syncthreads();
    const uint64_t* P = a.prefix;
    if (a.fixed_n_arc) {
        if (t == 0) {
            s_narc = *a.fixed_n_arc;
            s_fail = s_narc > a.o.arc_cap;
        }
    } else if (wave == 0) {
        // archive to archive: record i is accepted iff header + P[i] - P[f] < blocksz and i - f < limit
        uint64_t f = 0;
        uint32_t na = 0;
        bool fail = false;
        while (f < n) {
            if (na == a.o.arc_cap) {
                fail = true;
                break;
            }
            const uint64_t blk = a.blocksz[min(na, a.n_blocksz - 1)];
            const uint64_t pf = P[f];
            uint64_t lo = f, hi = min<uint64_t>(n, f + a.limit);  // full(lo) is false; the cut is in (lo, hi]
            while (hi - lo > 1) {
                const uint64_t step = (hi - lo + 63) / 64;
                const uint64_t i = lo + (uint64_t)(lane + 1) * step;
                const bool full = i < hi ? a.header_bytes + (P[i] - pf) >= blk : true;
                const uint64_t m = __ballot(full);
                const uint32_t first = (uint32_t)__ffsll((unsigned long long)m) - 1;  // lane 63 is always set
                hi = min<uint64_t>(hi, lo + (uint64_t)(first + 1) * step);
                lo = lo + (uint64_t)first * step;
            }
            if (lane == 0) a.cuts[na] = (uint32_t)f;
            na++;
            f = hi;
        }
        if (lane == 0) {
            if (!fail) a.cuts[na] = (uint32_t)n;
            s_narc = na;
            s_fail = fail;
        }
    }
    __syncthreads();
    if (s_fail) {
        if (t == 0) *a.o.status = SDFS_CDC_ARCHIVE_ECAP;
        return;
    }
    const uint32_t narc = s_narc;
    if (!a.fixed_n_arc)
        for (uint32_t k = t; k <= narc; k += kPlanThreads) a.o.arc_first[k] = a.cuts[k];
    __syncthreads();
    const uint32_t* first = a.o.arc_first;
    for (uint32_t k = t; k < narc; k += kPlanThreads) a.o.arc_bytes[k] = a.header_bytes + (P[first[k + 1]] - P[first[k]]);
    __syncthreads();
    if (t == 0) {
        uint64_t base = 0, end = 0;
        for (uint32_t k = 0; k < narc; k++) {
            base = (end + SDFS_CDC_ARCHIVE_ALIGN - 1) & ~(uint64_t)(SDFS_CDC_ARCHIVE_ALIGN - 1);
            a.o.arc_base[k] = base;
            end = base + a.o.arc_bytes[k];
        }
        a.o.totals[0] = narc;
        a.o.totals[1] = end;
        *a.o.status = 0;
    }
    __syncthreads();
    for (uint64_t i = t; i < n; i += kPlanThreads) {
        uint32_t lo = 0, hi = narc;  // the archive with first[k] <= i < first[k + 1]
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (first[mid] <= i) lo = mid;
            else hi = mid;
        }
        const uint32_t pos = (uint32_t)(a.header_bytes + (P[i] - P[first[lo]]) + unit);
        a.o.arc[i] = lo;
        a.o.pos[i] = pos;
        a.o.store_off[i] = a.o.arc_base[lo] + pos;
    }
}

// ----------------------------------------------------------------------------------------- pack

struct PackArgs {
    sdfs_cdc_archive_layout l;
    const uint32_t* count;
    uint64_t n_max;
    const uint8_t* src;
    const uint64_t* src_off;
    const uint32_t* src_len;
    uint32_t raw_frame;  // 0 or 4: bytes of the [BE32 -1] the record gets in front of the source's
    const uint8_t* records;
    const uint32_t* sel;
    uint32_t hash_len;
    uint32_t header_bytes;
    uint32_t version;
    const uint8_t* ivs;
    uint8_t* store;
    uint64_t store_cap;
};

// the records that touch a workgroup's span (LDS or global); so = store_off (the record's bytes
// start there; its header 8 + hash_len before)
struct RecView {
    const uint64_t* so;
    const uint64_t* src;
    const uint32_t* len;
    const uint32_t* arc;
    const uint32_t* sel;  // NULL: the record's own ordinal
    int64_t base;  // ordinal of entry 0
    int32_t n;
};

// byte x of the store: where it comes from (p != NULL: that byte; else the constant c); j = floor
// record of some x' <= x.  Only LDS is read on the way (arc_base for an archive header aside), so a
// vector's 16 sources are known before the first of its loads is issued.
struct ByteSrc {
    const uint8_t* p;
    uint32_t c;
};

__device__ __forceinline__ ByteSrc pack_byte(const PackArgs& a, const RecView& v, uint64_t x, int32_t& j,
                                             uint32_t n_arc) {
    const uint32_t hp = record_header_bytes(a.hash_len);
    while (j + 1 < v.n && v.so[j + 1] <= x + hp) j++;
    uint32_t next_arc = 0;
    if (j >= 0) {
        uint64_t k = x + hp - v.so[j];
        const uint32_t len = v.len[j];
        if (k < (uint64_t)hp + a.raw_frame + len) {
            if (k < 4) return {nullptr, be32_byte(a.hash_len, (uint32_t)k)};
            k -= 4;
            if (k < a.hash_len) {
                const uint64_t r = v.sel ? v.sel[j] : (uint64_t)(v.base + j);
                return {a.records + r * kRecordBytes + k, 0};
            }
            k -= a.hash_len;
            if (k < 4) return {nullptr, be32_byte(len + a.raw_frame, (uint32_t)k)};
            k -= 4;
            if (k < a.raw_frame) return {nullptr, 0xFF};  // nz = -1
            return {a.src + v.src[j] + (k - a.raw_frame), 0};
        }
        next_arc = v.arc[j] + 1;  // past the last record of its archive: padding, then the next header
    }
    if (a.header_bytes && next_arc < n_arc) {
        const uint64_t base = a.l.arc_base[next_arc];
        if (x >= base) {
            const uint64_t k = x - base;
            if (k < 4) return {nullptr, be32_byte(a.version, (uint32_t)k)};
            if (k < 20) return {a.ivs + (uint64_t)next_arc * 16 + (k - 4), 0};
        }
    }
    return {nullptr, 0};
}

__global__ __launch_bounds__(kPackThreads) void archive_pack_kernel(PackArgs a) {
    __shared__ uint64_t s_so[kPackLdsRecs], s_src[kPackLdsRecs];
    __shared__ uint32_t s_len[kPackLdsRecs], s_arc[kPackLdsRecs], s_sel[kPackLdsRecs];
    if (*a.l.status) return;
    const uint64_t sb = a.l.totals[1];
    if (sb == 0 || sb > a.store_cap) return;  // too large: archive_pack_check_kernel has flagged it
    const uint32_t n_arc = (uint32_t)a.l.totals[0];
    const int64_t n = (int64_t)live_count(a.count, a.n_max);
    const uint32_t tid = threadIdx.x;
    const uint32_t hp = record_header_bytes(a.hash_len);
    const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(a.store) & 15);
    const uint64_t nvec = ((uint64_t)head + sb + 15) / 16;  // vectors at absolute 16-byte addresses
    const uint64_t v0 = (uint64_t)blockIdx.x * kPackVecs;
    if (v0 >= nvec) return;  // uniform over the workgroup
    const uint64_t v1 = min(v0 + kPackVecs, nvec);
    const uint64_t x_lo = v0 * 16 > head ? v0 * 16 - head : 0, x_hi = min(sb, v1 * 16 - head);  // the span's bytes
    // the span's records: floor record of its first byte .. floor record of its last byte
    RecView all{a.l.store_off, a.src_off, a.src_len, a.l.arc, a.sel, 0, (int32_t)min<int64_t>(n, INT32_MAX)};
    // (floor record of byte x: the largest j with so[j] - hp <= x)
    const int32_t r0 = max(floor_index(all.so, all.n, x_lo + hp, -2), 0);
    const int32_t r1 = floor_index(all.so, all.n, x_hi - 1 + hp, -2);
    RecView rv{a.l.store_off + r0, a.src_off + r0, a.src_len + r0, a.l.arc + r0, a.sel ? a.sel + r0 : nullptr,
               r0, max(r1 - r0 + 1, 0)};
    if (rv.n <= (int32_t)kPackLdsRecs) {
        for (int32_t i = tid; i < rv.n; i += kPackThreads) {
            s_so[i] = rv.so[i];
            s_src[i] = rv.src[i];
            s_len[i] = rv.len[i];
            s_arc[i] = rv.arc[i];
            if (rv.sel) s_sel[i] = rv.sel[i];
        }
        __syncthreads();
        rv.so = s_so;
        rv.src = s_src;
        rv.len = s_len;
        rv.arc = s_arc;
        if (rv.sel) rv.sel = s_sel;
    }
    // per group of kIt vectors a lane makes three passes, so that the source loads of all of them
    // are in flight together: classify, load, realign + store
    constexpr int kIt = 4;
    enum : uint32_t { kSkip, kCopy, kBytes, kEdge };
    int32_t j = -2;
#pragma unroll 1
    for (uint64_t g0 = v0; g0 < v1; g0 += kIt * kPackThreads) {
        const uint64_t w0 = g0 + tid;  // the lane's vectors: w0 + it * kPackThreads
        uint32_t mode[kIt];
        int32_t jf[kIt];
        uintptr_t sa[kIt];
#pragma unroll
        for (int it = 0; it < kIt; it++) {
            mode[it] = kSkip;
            jf[it] = -1;
            sa[it] = 0;
            const uint64_t v = w0 + (uint64_t)it * kPackThreads;
            if (v >= v1) continue;
            const int64_t o = (int64_t)(v * 16) - head;  // store offset of the vector's first byte
            const uint64_t x0 = (uint64_t)max<int64_t>(o, 0);
            j = floor_index(rv.so, rv.n, x0 + hp, j);
            jf[it] = j;
            if (o < 0 || (uint64_t)o + 16 > sb) {  // a store end that is not 16-byte aligned
                mode[it] = kEdge;
                continue;
            }
            mode[it] = kBytes;
            if (j >= 0) {
                const uint64_t d0 = rv.so[j] + a.raw_frame;  // where the source's bytes start
                if (x0 >= d0 && x0 + 16 <= d0 + rv.len[j]) {
                    mode[it] = kCopy;
                    sa[it] = reinterpret_cast<uintptr_t>(a.src + rv.src[j] + (x0 - d0));
                }
            }
        }
        uint4 lo[kIt], hi[kIt];
#pragma unroll
        for (int it = 0; it < kIt; it++) {
            lo[it] = hi[it] = make_uint4(0, 0, 0, 0);
            if (mode[it] != kCopy) continue;
            const uint32_t sh = (uint32_t)(sa[it] & 15);
            const uint4* ap = reinterpret_cast<const uint4*>(sa[it] - sh);
            lo[it] = ap[0];
            if (sh) hi[it] = ap[1];  // holds bytes of the record the vector needs
        }
#pragma unroll
        for (int it = 0; it < kIt; it++) {
            if (mode[it] == kSkip) continue;
            const uint64_t v = w0 + (uint64_t)it * kPackThreads;
            const int64_t o = (int64_t)(v * 16) - head;
            uint8_t* dst = a.store + o;
            int32_t jj = jf[it];
            if (mode[it] == kEdge) {
                for (int b = 0; b < 16; b++) {
                    const int64_t x = o + b;
                    if (x < 0 || (uint64_t)x >= sb) continue;
                    const ByteSrc bs = pack_byte(a, rv, (uint64_t)x, jj, n_arc);
                    dst[b] = (uint8_t)(bs.p ? *bs.p : bs.c);
                }
                continue;
            }
            uint4 w;
            if (mode[it] == kCopy) {
                const uint32_t sh = (uint32_t)(sa[it] & 15), q = sh >> 2, r = sh & 3;
                const uint4 l = lo[it], h = hi[it];
                uint32_t t0, t1, t2, t3, t4;
                if (q == 0) { t0 = l.x; t1 = l.y; t2 = l.z; t3 = l.w; t4 = h.x; }
                else if (q == 1) { t0 = l.y; t1 = l.z; t2 = l.w; t3 = h.x; t4 = h.y; }
                else if (q == 2) { t0 = l.z; t1 = l.w; t2 = h.x; t3 = h.y; t4 = h.z; }
                else { t0 = l.w; t1 = h.x; t2 = h.y; t3 = h.z; t4 = h.w; }
                w.x = __builtin_amdgcn_alignbyte(t1, t0, r);
                w.y = __builtin_amdgcn_alignbyte(t2, t1, r);
                w.z = __builtin_amdgcn_alignbyte(t3, t2, r);
                w.w = __builtin_amdgcn_alignbyte(t4, t3, r);
            } else {
                ByteSrc bs[16];  // the sources first, then the 16 loads together
#pragma unroll
                for (int b = 0; b < 16; b++) bs[b] = pack_byte(a, rv, (uint64_t)o + b, jj, n_arc);
                uint32_t ws[4] = {0, 0, 0, 0};
#pragma unroll
                for (int b = 0; b < 16; b++) ws[b >> 2] |= (bs[b].p ? (uint32_t)*bs[b].p : bs[b].c) << (8 * (b & 3));
                w = make_uint4(ws[0], ws[1], ws[2], ws[3]);
            }
            *reinterpret_cast<uint4*>(dst) = w;
        }
    }
}

__global__ void archive_pack_check_kernel(sdfs_cdc_archive_layout l, uint64_t store_cap) {
    if (*l.status == 0 && l.totals[1] > store_cap) *l.status = SDFS_CDC_ARCHIVE_ESTORE;
}

// ------------------------------------------------------------------------------------------ map

struct MapArgs {
    sdfs_cdc_archive_layout l;
    const uint32_t* count;
    uint64_t n_max;
    const uint32_t* rec_len;
    const uint8_t* records;
    const uint32_t* sel;
    uint32_t hash_len;
    uint32_t version;
    const uint32_t* sizes;  // per archive, or NULL
    uint32_t stride;        // slots per row of slot_rec / per image of maps
    uint8_t* maps;
    uint32_t* slot_rec;
    unsigned long long* info;
};

__device__ __forceinline__ const uint8_t* rec_key(const MapArgs& a, uint32_t r) {
    return a.records + (uint64_t)(a.sel ? a.sel[r] : r) * kRecordBytes;
}

template <bool LDS>
__global__ __launch_bounds__(kMapThreads) void archive_map_kernel(MapArgs a) {
    __shared__ uint32_t s_owner[LDS ? kMapLdsSlots : 1];
    if (*a.l.status) return;
    const uint32_t arc = blockIdx.x, t = threadIdx.x;
    if (arc >= (uint32_t)a.l.totals[0]) return;
    const uint32_t asked = a.sizes ? a.sizes[arc] : a.stride;
    const uint32_t size = min(asked, a.stride);
    uint32_t* row = a.slot_rec + (uint64_t)arc * a.stride;
    uint32_t* owner = LDS ? s_owner : row;
    const uint64_t n = live_count(a.count, a.n_max);
    const uint32_t first = a.l.arc_first[arc], last = (uint32_t)min<uint64_t>(a.l.arc_first[arc + 1], n);
    const uint32_t cnt = last > first ? last - first : 0;
    for (uint32_t s = t; s < (LDS ? size : a.stride); s += kMapThreads) owner[s] = kNone;
    __syncthreads();
    // a probe sequence visits every slot only when the table has a free one: size prime, step < size
    const bool usable = size >= 3 && asked <= a.stride && cnt + 1 < size;
    if (!usable && t == 0 && cnt) atomicAdd(&a.info[1], 1ull);
    if (usable) {
        for (uint32_t r0 = first + t; r0 < last; r0 += kMapThreads) {
            uint32_t cur = r0;
            const uint8_t* key = rec_key(a, cur);
            uint32_t h = map_key_hash(key);
            uint32_t idx = map_probe_home(h, size);
            for (uint64_t guard = 0; guard < 2ull * size * cnt + 2; guard++) {
                const uint32_t old = atomicMin(&owner[idx], cur);
                if (old == kNone) break;
                uint32_t mover = old;  // the higher ordinal of the two moves on
                if (old < cur) mover = cur;
                const uint8_t* ko = rec_key(a, old);
                const uint8_t* kc = key;
                bool same = true;
                for (uint32_t b = 0; b < a.hash_len; b++) same &= ko[b] == kc[b];
                if (same) {  // the later of two equal keys is refused (HashExistsException)
                    atomicAdd(&a.info[0], 1ull);
                    break;
                }
                if (mover != cur) {
                    cur = mover;
                    key = ko;
                    h = map_key_hash(key);
                }
                idx = map_probe_next(idx, map_probe_step(h, size), size);
            }
        }
    }
    __syncthreads();
    for (uint32_t s = t; s < a.stride; s += kMapThreads) {
        if (LDS) row[s] = s < size ? owner[s] : kNone;
        else if (s >= size) row[s] = kNone;
    }
    // the image, one 32-bit word per thread (every field is 4-byte aligned): __builtin_bswap32(v) is
    // the word whose bytes in memory are put_be32(v)
    const uint32_t el = map_entry_bytes(a.hash_len, a.version), off = map_header_bytes(a.version);
    const uint64_t stride_bytes = map_image_bytes(a.stride, a.hash_len, a.version);
    const uint64_t image_bytes = map_image_bytes(size, a.hash_len, a.version);
    uint32_t* img = reinterpret_cast<uint32_t*>(a.maps + (uint64_t)arc * stride_bytes);
    for (uint64_t w = t; w < stride_bytes / 4; w += kMapThreads) {
        const uint64_t b = w * 4;
        uint32_t val = 0;
        if (b < off) {
            val = b == 0 ? __builtin_bswap32(SDFS_CDC_ARCHIVE_MAP_MAGIC)
                         : b == kMapVersionAt ? __builtin_bswap32(a.version) : 0;
        } else if (b < image_bytes) {
            const uint32_t s = (uint32_t)((b - off) / el), k = (uint32_t)((b - off) % el);
            const uint32_t r = owner[s];
            if (r != kNone) {
                if (k < a.hash_len) {
                    const uint8_t* key = rec_key(a, r) + k;
                    val = (uint32_t)key[0] | (uint32_t)key[1] << 8 | (uint32_t)key[2] << 16 | (uint32_t)key[3] << 24;
                } else if (k == a.hash_len + kMapPosAt) {
                    val = __builtin_bswap32(a.l.pos[r] - kRecordLenBack);  // the map value: the length word's place
                } else {  // a.hash_len + kMapLenAt
                    val = __builtin_bswap32(a.rec_len[r]);
                }
            }
        }
        img[w] = val;
    }
}

// -------------------------------------------------------------------------------------- compact

struct SelectArgs {
    sdfs_cdc_archive_layout old;
    uint64_t n;
    uint32_t n_arc;
    const uint32_t* old_len;
    const uint32_t* old_sel;
    const uint32_t* slot_rec;
    const uint32_t* old_sizes;
    uint32_t old_stride;
    const uint8_t* keep;
    sdfs_cdc_archive_kept k;
    uint32_t* live;       // [n_arc] scratch
    uint32_t* new_first;  // [n_arc] scratch: new ordinal of the archive's first survivor
};

__device__ __forceinline__ bool slot_kept(const SelectArgs& a, uint32_t arc, uint32_t s, uint32_t size, uint32_t& r) {
    r = s < size ? a.slot_rec[(uint64_t)arc * a.old_stride + s] : kNone;
    return r != kNone && r < a.n && a.keep[r] != 0;
}

__global__ __launch_bounds__(256) void compact_count_kernel(SelectArgs a) {
    __shared__ uint32_t ws[4];
    const uint32_t arc = blockIdx.x, t = threadIdx.x;
    const uint32_t size = min(a.old_sizes ? a.old_sizes[arc] : a.old_stride, a.old_stride);
    uint32_t c = 0, r;
    for (uint32_t s = t; s < size; s += 256) c += slot_kept(a, arc, s, size, r);
    c = wave_sum(c);
    if ((t & 63) == 0) ws[t >> 6] = c;
    __syncthreads();
    if (t == 0) a.live[arc] = ws[0] + ws[1] + ws[2] + ws[3];
}

// one thread: the archives are few (about 50 per GiB)
__global__ void compact_cuts_kernel(SelectArgs a) {
    uint32_t rec = 0, na = 0;
    for (uint32_t arc = 0; arc < a.n_arc; arc++) {
        const uint32_t lv = a.live[arc];
        a.new_first[arc] = rec;
        a.k.deleted[arc] = lv == 0;
        a.k.new_arc[arc] = lv ? na : kNone;
        if (lv) {
            a.k.lay.arc_first[na] = rec;
            a.k.map_slots[na] = map_size_rule(2ull * lv + 5);
            na++;
            rec += lv;
        }
    }
    a.k.lay.arc_first[na] = rec;
    *a.k.count = rec;
    a.k.lay.totals[0] = na;  // the fixed-cut plan reads it from here
}

__global__ __launch_bounds__(256) void compact_assign_kernel(SelectArgs a) {
    __shared__ uint32_t ws[4];
    __shared__ uint32_t s_carry;
    const uint32_t arc = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t size = min(a.old_sizes ? a.old_sizes[arc] : a.old_stride, a.old_stride);
    const uint32_t f = a.old.arc_first[arc], l = (uint32_t)min<uint64_t>(a.old.arc_first[arc + 1], a.n);
    for (uint32_t r = f + t; r < l; r += 256) a.k.new_of_old[r] = kNone;
    if (t == 0) s_carry = a.new_first[arc];
    __syncthreads();
    for (uint32_t s0 = 0; s0 < size; s0 += 256) {
        uint32_t r;
        const bool on = slot_kept(a, arc, s0 + t, size, r);
        const uint64_t m = __ballot(on);  // a flag's wave scan is one ballot, not a wave_inclusive_scan
        const uint32_t below = __popcll(m & ((1ull << lane) - 1));
        if (lane == 0) ws[wave] = __popcll(m);
        __syncthreads();
        uint32_t before = s_carry, tile = 0;
        for (uint32_t w = 0; w < 4; w++) {
            if (w < wave) before += ws[w];
            tile += ws[w];
        }
        if (on) {
            const uint32_t jn = before + below;
            a.k.new_of_old[r] = jn;
            a.k.sel[jn] = a.old_sel ? a.old_sel[r] : r;
            a.k.src_off[jn] = a.old.store_off[r];
            a.k.rec_len[jn] = a.old_len[r];
        }
        __syncthreads();
        if (t == 0) s_carry += tile;
        __syncthreads();
    }
}

// ----------------------------------------------------------------------------------------- host

bool layout_complete(const sdfs_cdc_archive_layout* l) {
    return l && l->arc && l->pos && l->store_off && l->arc_first && l->arc_bytes && l->arc_base && l->totals &&
           l->status && l->arc_cap;
}

bool kept_complete(const sdfs_cdc_archive_kept* k) {
    return k && k->new_of_old && k->sel && k->src_off && k->rec_len && k->count && k->deleted && k->new_arc &&
           k->map_slots && layout_complete(&k->lay);
}

// a map key that is also a stored record's hash: 16 or 32; 20 gets the map's message, any other
// length the record's
int check_map_key_len(uint32_t hash_len) {
    return check_hash_len(hash_len, hash_len == 20 ? HashOf::kMapKey : HashOf::kRecord);
}

// the plan kernel over `rec_len`; fixed_n_arc != NULL: the cuts are in out->arc_first already
int launch_plan(const uint32_t* d_rec_len, const uint32_t* d_count, uint64_t n_max, uint32_t hash_len,
                uint32_t header_bytes, const uint64_t* blocksz, uint32_t n_blocksz, uint32_t limit,
                const sdfs_cdc_archive_layout& out, const uint32_t* fixed_n_arc, hipStream_t s) {
    Scratch sc(s);
    PlanArgs a{};
    a.rec_len = d_rec_len;
    a.count = d_count;
    a.n_max = n_max;
    a.hash_len = hash_len;
    a.header_bytes = header_bytes;
    a.n_blocksz = n_blocksz;
    for (uint32_t i = 0; i < n_blocksz; i++) a.blocksz[i] = (uint32_t)blocksz[i];
    a.limit = limit;
    a.o = out;
    a.fixed_n_arc = fixed_n_arc;
    SDFS_TRY(sc.get(&a.prefix, (size_t)n_max + 1));
    SDFS_TRY(sc.get(&a.cuts, (size_t)out.arc_cap + 1));
    hipLaunchKernelGGL(archive_plan_kernel, dim3(1), dim3(kPlanThreads), 0, s, a);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

}  // namespace
}  // namespace sdfs

using namespace sdfs;

extern "C" {

uint32_t sdfs_cdc_archive_map_size(uint64_t sz) { return map_size_rule(sz); }

uint32_t sdfs_cdc_archive_pack_span(void) { return kPackVecs * 16; }

uint64_t sdfs_cdc_archive_map_bytes(uint32_t map_slots, uint32_t hash_len, uint32_t version) {
    return map_image_bytes(map_slots, hash_len, version);
}

int sdfs_cdc_archive_plan(int device, const uint32_t* d_rec_len, const uint32_t* d_count, uint64_t n_max,
                          uint32_t hash_len, uint32_t header_bytes, const uint64_t* blocksz, uint32_t n_blocksz,
                          uint32_t map_slots, const sdfs_cdc_archive_layout* out, void* stream) {
    if (!layout_complete(out)) return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_archive_layout");
    if (const int rc = check_hash_len(hash_len, HashOf::kRecord)) return rc;
    if (const int rc = check_header(header_bytes)) return rc;
    if (n_max && !d_rec_len) return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_max >= UINT32_MAX) return fail_status(SDFS_CDC_EINVAL, "n_max %llu: record ordinals are 32-bit",
                                                (unsigned long long)n_max);
    if (!blocksz || n_blocksz == 0 || n_blocksz > kPlanBlocksz)
        return fail_status(SDFS_CDC_EINVAL, "n_blocksz %u: 1 .. %u values", n_blocksz, kPlanBlocksz);
    for (uint32_t i = 0; i < n_blocksz; i++) {
        if (blocksz[i] > (uint64_t)INT32_MAX)
            return fail_status(SDFS_CDC_EINVAL, "blocksz[%u] = %llu above 2^31 - 1: the version-0 map value is an int", i,
                               (unsigned long long)blocksz[i]);
        if (blocksz[i] <= header_bytes)
            return fail_status(SDFS_CDC_EINVAL, "blocksz[%u] = %llu: an archive with a %u-byte header never takes a record",
                               i, (unsigned long long)blocksz[i], header_bytes);
    }
    const uint32_t limit = (uint32_t)(int)(map_slots * .75);
    if (map_slots < 2 || map_slots > (uint32_t)INT32_MAX)
        return fail_status(SDFS_CDC_EINVAL, "map_slots %u: a map that takes no entry", map_slots);
    if (const int rc = set_device(device)) return rc;
    return launch_plan(d_rec_len, d_count, n_max, hash_len, header_bytes, blocksz, n_blocksz, limit, *out, nullptr,
                       reinterpret_cast<hipStream_t>(stream));
}

int sdfs_cdc_archive_pack(int device, const sdfs_cdc_archive_layout* layout, const uint32_t* d_count,
                          uint64_t n_max, const uint8_t* d_src, const uint64_t* d_src_off,
                          const uint32_t* d_src_len, int raw_frame, const uint8_t* d_records,
                          const uint32_t* d_sel, uint32_t hash_len, uint32_t header_bytes, uint32_t version,
                          const uint8_t* d_ivs, uint8_t* d_store, uint64_t store_cap, void* stream) {
    if (!layout_complete(layout)) return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_archive_layout");
    if (const int rc = check_hash_len(hash_len, HashOf::kRecord)) return rc;
    if (const int rc = check_header(header_bytes)) return rc;
    if (n_max && (!d_src || !d_src_off || !d_src_len || !d_records)) return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_max >= (uint64_t)INT32_MAX) return fail_status(SDFS_CDC_EINVAL, "n_max %llu: record ordinals are 32-bit",
                                                         (unsigned long long)n_max);
    if (header_bytes && !d_ivs) return fail_status(SDFS_CDC_EINVAL, "an archive header needs the IVs");
    if (store_cap && !d_store) return fail_status(SDFS_CDC_EINVAL, "null store");
    if (reinterpret_cast<uintptr_t>(d_src) & 15) return fail_status(SDFS_CDC_EINVAL, "d_src is not 16-byte aligned");
    const uint64_t blocks = (store_cap + 15 + 16) / 16 / kPackVecs + 1;
    if (blocks > (uint64_t)INT32_MAX) return fail_status(SDFS_CDC_EINVAL, "store of %llu bytes: split the batch",
                                                         (unsigned long long)store_cap);
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PackArgs a{*layout, d_count, n_max, d_src, d_src_off, d_src_len, raw_frame ? 4u : 0u, d_records, d_sel,
               hash_len, header_bytes, version, d_ivs, d_store, store_cap};
    hipLaunchKernelGGL(archive_pack_check_kernel, dim3(1), dim3(1), 0, s, *layout, store_cap);
    if (store_cap && n_max)
        hipLaunchKernelGGL(archive_pack_kernel, dim3((uint32_t)blocks), dim3(kPackThreads), 0, s, a);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_archive_map_emit(int device, const sdfs_cdc_archive_layout* layout, const uint32_t* d_count,
                              uint64_t n_max, const uint32_t* d_rec_len, const uint8_t* d_records,
                              const uint32_t* d_sel, uint32_t hash_len, uint32_t version,
                              const uint32_t* d_map_slots, uint32_t map_slots, uint8_t* d_maps,
                              uint32_t* d_slot_rec, uint64_t* d_info, void* stream) {
    if (!layout_complete(layout)) return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_archive_layout");
    if (const int rc = check_map_key_len(hash_len)) return rc;
    if (!d_maps || !d_slot_rec || !d_info) return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_max && (!d_rec_len || !d_records)) return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_max >= UINT32_MAX) return fail_status(SDFS_CDC_EINVAL, "n_max %llu: record ordinals are 32-bit",
                                                (unsigned long long)n_max);
    if (map_slots < 3 || map_slots > (uint32_t)INT32_MAX)
        return fail_status(SDFS_CDC_EINVAL, "map_slots %u: at least 3 (the probe step is 1 + h %% (size - 2))", map_slots);
    if (reinterpret_cast<uintptr_t>(d_maps) & 3) return fail_status(SDFS_CDC_EINVAL, "d_maps is not 4-byte aligned");
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    SDFS_TRY(hipMemsetAsync(d_info, 0, 16, s));
    MapArgs a{*layout, d_count, n_max, d_rec_len, d_records, d_sel, hash_len, version, d_map_slots, map_slots,
              d_maps, d_slot_rec, reinterpret_cast<unsigned long long*>(d_info)};
    if (map_slots <= kMapLdsSlots)
        hipLaunchKernelGGL(archive_map_kernel<true>, dim3(layout->arc_cap), dim3(kMapThreads), 0, s, a);
    else
        hipLaunchKernelGGL(archive_map_kernel<false>, dim3(layout->arc_cap), dim3(kMapThreads), 0, s, a);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_archive_compact_select(int device, const sdfs_cdc_archive_layout* old_layout, uint64_t n,
                                    uint32_t n_arc, const uint32_t* d_old_rec_len, const uint32_t* d_old_sel,
                                    const uint32_t* d_slot_rec, const uint32_t* d_old_map_slots,
                                    uint32_t old_map_slots, const uint8_t* d_keep, uint32_t hash_len,
                                    uint32_t header_bytes, const sdfs_cdc_archive_kept* kept, void* stream) {
    if (!layout_complete(old_layout)) return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_archive_layout");
    if (!kept_complete(kept)) return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_archive_kept");
    if (const int rc = check_hash_len(hash_len, HashOf::kRecord)) return rc;
    if (const int rc = check_header(header_bytes)) return rc;
    if (n >= UINT32_MAX) return fail_status(SDFS_CDC_EINVAL, "n %llu: record ordinals are 32-bit", (unsigned long long)n);
    if (n_arc > old_layout->arc_cap) return fail_status(SDFS_CDC_EINVAL, "n_arc %u above the old layout's arc_cap", n_arc);
    if (kept->lay.arc_cap < n_arc)
        return fail_status(SDFS_CDC_ECAP, "new layout holds %u archives, %u may survive", kept->lay.arc_cap, n_arc);
    if (n_arc && (!d_slot_rec || !old_map_slots)) return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n && (!d_old_rec_len || !d_keep)) return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    Scratch sc(s);
    SelectArgs a{*old_layout, n, n_arc, d_old_rec_len, d_old_sel, d_slot_rec, d_old_map_slots, old_map_slots,
                 d_keep, *kept, nullptr, nullptr};
    SDFS_TRY(sc.get(&a.live, n_arc));
    SDFS_TRY(sc.get(&a.new_first, n_arc));
    if (n_arc) hipLaunchKernelGGL(compact_count_kernel, dim3(n_arc), dim3(256), 0, s, a);
    hipLaunchKernelGGL(compact_cuts_kernel, dim3(1), dim3(1), 0, s, a);
    if (n_arc) hipLaunchKernelGGL(compact_assign_kernel, dim3(n_arc), dim3(256), 0, s, a);
    SDFS_TRY(hipGetLastError());
    // the plan with fixed cuts: n_arc comes from totals[0], which the plan rewrites with the same value
    return launch_plan(kept->rec_len, kept->count, n, hash_len, header_bytes, nullptr, 0, 0, kept->lay,
                       reinterpret_cast<const uint32_t*>(kept->lay.totals), s);
}

int sdfs_cdc_archive_compact(int device, const sdfs_cdc_archive_layout* old_layout, uint64_t n, uint32_t n_arc,
                             const uint8_t* d_old_store, const uint32_t* d_old_rec_len, const uint32_t* d_old_sel,
                             const uint32_t* d_slot_rec, const uint32_t* d_old_map_slots, uint32_t old_map_slots,
                             const uint8_t* d_keep, const uint8_t* d_records, uint32_t hash_len,
                             uint32_t header_bytes, uint32_t version, const uint8_t* d_ivs,
                             const sdfs_cdc_archive_kept* kept, uint8_t* d_store, uint64_t store_cap,
                             uint32_t new_map_stride, uint8_t* d_maps, uint32_t* d_slot_rec_new, uint64_t* d_info,
                             void* stream) {
    if (!kept_complete(kept)) return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_archive_kept");
    if (const int rc = check_map_key_len(hash_len)) return rc;
    if (n && (!d_old_store || !d_records)) return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (const int rc = sdfs_cdc_archive_compact_select(device, old_layout, n, n_arc, d_old_rec_len, d_old_sel,
                                                       d_slot_rec, d_old_map_slots, old_map_slots, d_keep, hash_len,
                                                       header_bytes, kept, stream))
        return rc;
    if (const int rc = sdfs_cdc_archive_pack(device, &kept->lay, kept->count, n, d_old_store, kept->src_off,
                                             kept->rec_len, 0, d_records, kept->sel, hash_len, header_bytes, version,
                                             d_ivs, d_store, store_cap, stream))
        return rc;
    return sdfs_cdc_archive_map_emit(device, &kept->lay, kept->count, n, kept->rec_len, d_records, kept->sel, hash_len,
                                     version, kept->map_slots, new_map_stride, d_maps, d_slot_rec_new, d_info, stream);
}

}  // extern "C"
