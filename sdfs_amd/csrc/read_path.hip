// read_path.hip — write buffers rebuilt from their LongByteArrayMap slots on the device
// (include/sdfs_read.h): the inverse of map_emit.hip plus the last hop.
//
// Reference: WritableCacheBuffer.initBuffer (WritableCacheBuffer.java:249-410) takes the buffer's
// SparseDataChunk (SparseDataChunk.java:159-174, HashLocPair(byte[]) HashLocPair.java:86-97),
// fetches the chunk of every pair before the first hashloc == 0 (HashBlobArchive.getChunk,
// HashBlobArchive.java:1922-1944) and puts ck[offset .. offset + min(nlen, ck.length)) at pos into
// a zeroed CHUNK_LENGTH array.  Here: one wave per buffer parses its image (map_parse_kernel),
// one wave per buffer marks the directory entries it uses and a one-block scan ranks them
// (read_plan), the caller runs the decryptor / decoder over the ranked list, one wave per buffer
// settles its status and lays out per-pair {end, running max of end, source offset}
// (assemble_status_kernel), and the gather kernel — the only pass over the data — writes every
// output byte once.
//
// Gather: destination-driven.  A workgroup owns 64 KiB of one buffer's output, cut at absolute
// 16-byte addresses; the buffer's pos / end / max-end / source arrays sit in LDS (<= kLdsPairs used pairs,
// else they are searched in global memory).  A lane takes one 16-byte vector at a time: floor
// entry by binary search (the previous vector's entry is tried first), and
//   - the entry covers the whole vector and no later pair starts inside it: two aligned 16-byte
//     loads of the source, realigned by a byte shift, one aligned 16-byte store;
//   - nothing at or before the entry reaches the vector (max-end) and no pair starts inside: zeros;
//   - else byte by byte: per byte the floor entry, then back to the last earlier pair that reaches
//     the byte (the overlap rule; the walk ends where the running max of end stops reaching it).
// The first and last vectors of a buffer whose ends are not 16-byte aligned are stored bytewise.
//
// Ranged reads (DedupFileChannel.read, DedupFileChannel.java:499-608; the "pieces" section below):
// the host split (read_split.h) cuts requests into pieces {row, start, len, out_off}; the plan marks
// only the directory entries of the pairs that touch a piece; the same tile body gathers ragged,
// arbitrarily aligned pieces, its work list built from a prefix over the pieces' tile counts, and
// stages only the piece's window of pairs in LDS.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "../../include/sdfs_read.h"
#include "block_scan.h"
#include "call_support.h"
#include "read_split.h"
#include "store_format.h"

namespace sdfs {
namespace {

constexpr uint32_t kNone = SDFS_CDC_READ_NONE;
constexpr int kGatherThreads = 256;
constexpr uint32_t kTileVecs = 4096;  // 16-byte vectors per workgroup (64 KiB): 4 groups of 4 per lane
constexpr uint32_t kLdsPairs = 1024;  // used pairs per buffer staged in LDS (20 KiB)
// workgroups of the pieces' gather at most (they stride over the tiles): about one tile each up to
// 4 GiB of output for the LDS form; the global-memory form is the rare one
constexpr uint32_t kPieceGrid = 65536, kPieceGridBig = 4096;

__device__ __forceinline__ bool wave_any(bool v) { return __ballot(v) != 0; }
// a value every lane of the wave holds alike, moved to a scalar register
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// ---------------------------------------------------------------------------------------- parse

struct ParseArgs {
    const uint8_t* map;
    uint32_t slot_bytes;
    uint32_t hash_len;
    sdfs_cdc_pairs p;
    int32_t* tmp_pos;   // [nbuf*cap] scratch of the TreeMap path
    uint32_t* tmp_dead; // [nbuf*cap]
};

// pair i of the image -> output slot `slot`
__device__ __forceinline__ void put_pair(const ParseArgs& a, const uint8_t* rec, uint64_t slot) {
    uint8_t* h = a.p.hashes + slot * 32;
    for (uint32_t k = 0; k < a.hash_len; k++) h[k] = rec[k];
    for (uint32_t k = a.hash_len; k < 32; k++) h[k] = 0;
    const uint8_t* q = rec + a.hash_len;
    a.p.hashloc[slot] = (uint64_t)get_be32(q + kPairHashlocAt) << 32 | get_be32(q + kPairHashlocAt + 4);
    a.p.len[slot] = (int32_t)get_be32(q + kPairLenAt);
    a.p.pos[slot] = (int32_t)get_be32(q + kPairPosAt);
    a.p.offset[slot] = (int32_t)get_be32(q + kPairOffsetAt);
    a.p.nlen[slot] = (int32_t)get_be32(q + kPairNlenAt);
}

// one wave per buffer (every branch below is wave-uniform)
__global__ __launch_bounds__(64) void map_parse_kernel(ParseArgs a) {
    const uint32_t lane = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const uint8_t* img = a.map + (uint64_t)b * a.slot_bytes;
    const uint32_t hl = a.hash_len;
    const SlotWalk w = slot_walk_check(img, a.slot_bytes, hl, lane);
    const uint32_t status = w.status, n = w.n;
    const uint64_t base = (uint64_t)b * a.p.cap;
    uint32_t count = n;
    if (!w.unsorted) {
        for (uint32_t i = lane; i < n; i += 64) put_pair(a, slot_pair(img, i, hl), base + i);
    } else {
        // tmp_dead[i] = pair_superseded(img, i, n, hl), from a copy of the pos values that the rank
        // below reads again
        for (uint32_t i = lane; i < n; i += 64)
            a.tmp_pos[base + i] = (int32_t)get_be32(pair_fields(img, i, hl) + kPairPosAt);
        __syncthreads();
        uint32_t live = 0;
        for (uint32_t i = lane; i < n; i += 64) {
            const int32_t ps = a.tmp_pos[base + i];
            uint32_t dead = 0;
            for (uint32_t j = i + 1; j < n; j++) dead |= a.tmp_pos[base + j] == ps;
            a.tmp_dead[base + i] = dead;
            live += !dead;
        }
        __syncthreads();
        for (uint32_t i = lane; i < n; i += 64) {
            if (a.tmp_dead[base + i]) continue;
            const int32_t ps = a.tmp_pos[base + i];
            uint32_t rank = 0;
            for (uint32_t j = 0; j < n; j++) rank += !a.tmp_dead[base + j] && a.tmp_pos[base + j] < ps;
            put_pair(a, slot_pair(img, i, hl), base + rank);
        }
        count = wave_sum(live);
    }
    if (lane == 0) {
        a.p.counts[b] = count;
        a.p.flags[b] = img[0];
        a.p.doop[b] = status ? 0 : get_be32(slot_pair(img, n, hl));  // the trailer
        a.p.status[b] = status;
    }
}

// ----------------------------------------------------------------------------------------- plan

struct PlanArgs {
    sdfs_cdc_pairs p;
    uint64_t pos_base;
    uint64_t n_store;
    const uint64_t* store_off;
    const uint32_t* store_len;
    const uint32_t* store_raw;
    uint32_t* pair_fetch;
    uint32_t* fetch_count;
    uint64_t* src_off;
    uint32_t* src_len;
    uint64_t* dst_off;
    uint32_t* dst_cap;
    uint64_t* plain_off;
    uint64_t* total_bytes;
    uint32_t* mark;  // [n_store] 1 = needed, then its fetch index
};

// one wave per buffer: the terminator rule, MISSING, and the directory entries it needs
__global__ __launch_bounds__(64) void plan_mark_kernel(PlanArgs a) {
    const uint32_t lane = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const uint64_t base = (uint64_t)b * a.p.cap;
    const uint32_t st = a.p.status[b];
    const uint32_t n = st ? 0 : min(a.p.counts[b], a.p.cap);
    uint32_t used = n;
    for (uint32_t i = lane; i < n; i += 64)
        if (a.p.hashloc[base + i] == 0) used = min(used, i);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) used = min(used, (uint32_t)__shfl_xor(used, o));
    bool missing = false;
    for (uint32_t i = lane; i < used; i += 64) {
        const uint64_t hl = a.p.hashloc[base + i];
        missing |= hl < a.pos_base || hl - a.pos_base >= a.n_store;
    }
    if (wave_any(missing)) {
        used = 0;
        if (lane == 0) a.p.status[b] = st | SDFS_CDC_READ_MISSING;
    }
    for (uint32_t i = lane; i < a.p.cap; i += 64) {
        uint32_t f = kNone;
        if (i < used) {
            f = (uint32_t)(a.p.hashloc[base + i] - a.pos_base);
            a.mark[f] = 1;
        }
        a.pair_fetch[base + i] = f;
    }
}

// one block: rank the marked directory entries and lay out their fetches (its own scan text: see
// block_exclusive_scan_1024).  The directory is
// walked in tiles of 1024 entries (coalesced), each tile scanned wave by wave, the running totals
// carried from tile to tile.
__global__ __launch_bounds__(1024) void plan_scan_kernel(PlanArgs a) {
    __shared__ uint32_t wc[16];
    __shared__ uint64_t wd[16], wp[16];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t cf = 0;          // fetches before this tile
    uint64_t cd = 0, cp = 0;  // their chunk-area / decrypted-area bytes
    for (uint64_t k0 = 0; k0 < a.n_store; k0 += 1024) {
        const uint64_t k = k0 + t;
        const bool on = k < a.n_store && a.mark[k] != 0;
        const uint32_t raw = on ? a.store_raw[k] : 0, sl = on ? a.store_len[k] : 0;
        const uint64_t d = on ? ((uint64_t)raw + 15) & ~15ull : 0, p = on ? ((uint64_t)sl + 15) & ~15ull : 0;
        uint32_t ic = on;  // inclusive scans over the wave
        uint64_t id = d, ip = p;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t vc = __shfl_up(ic, o);
            const unsigned long long vd = __shfl_up((unsigned long long)id, o), vp = __shfl_up((unsigned long long)ip, o);
            if (lane >= (uint32_t)o) {
                ic += vc;
                id += vd;
                ip += vp;
            }
        }
        if (lane == 63) {
            wc[wave] = ic;
            wd[wave] = id;
            wp[wave] = ip;
        }
        __syncthreads();
        uint32_t bc = cf, tc = 0;
        uint64_t bd = cd, bp = cp, td = 0, tp = 0;
        for (uint32_t w = 0; w < 16; w++) {
            if (w < wave) {
                bc += wc[w];
                bd += wd[w];
                bp += wp[w];
            }
            tc += wc[w];
            td += wd[w];
            tp += wp[w];
        }
        if (on) {
            const uint32_t f = bc + ic - 1;
            a.src_off[f] = a.store_off[k];
            a.src_len[f] = sl;
            a.dst_off[f] = bd + id - d;
            a.dst_cap[f] = raw;
            if (a.plain_off) a.plain_off[f] = bp + ip - p;
            a.mark[k] = f;
        }
        cf += tc;
        cd += td;
        cp += tp;
        __syncthreads();  // the wave totals are rewritten by the next tile
    }
    if (t == 0) {
        *a.fetch_count = cf;
        a.total_bytes[0] = cd;
        a.total_bytes[1] = cp;
    }
}

__global__ __launch_bounds__(256) void plan_remap_kernel(uint32_t* pair_fetch, uint64_t n, const uint32_t* mark) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = pair_fetch[i];
    if (k != kNone) pair_fetch[i] = mark[k];
}

__global__ __launch_bounds__(256) void chain_lens_kernel(const uint32_t* in, const uint32_t* count, uint64_t n_max,
                                                         uint32_t* out) {
    const uint64_t n = live_count(count, n_max);
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = in[i] == UINT32_MAX ? 0 : in[i];
}

// ------------------------------------------------------------------------------------- assemble

struct AsmArgs {
    sdfs_cdc_pairs p;
    uint32_t nbuf;
    uint32_t chunk_length;
    const uint32_t* pair_fetch;
    const uint8_t* chunks;
    const uint64_t* fetch_off;
    const uint32_t* fetch_len;
    uint8_t* out;
    uint32_t* nused;   // [nbuf] pairs the gather places (0 for a failed buffer)
    int32_t* end;      // [nbuf*cap] pos + c
    int32_t* maxend;   // [nbuf*cap] max of end[0..i]
    uint64_t* src;     // [nbuf*cap] offset in chunks of the byte that goes to pos
    uint32_t tiles_per_buf;
};

// one wave per buffer: FETCH / BOUNDS, then the gather's per-pair arrays
__global__ __launch_bounds__(64) void assemble_status_kernel(AsmArgs a) {
    const uint32_t lane = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const uint64_t base = (uint64_t)b * a.p.cap;
    uint32_t st = a.p.status[b];
    const uint32_t n = st ? 0 : min(a.p.counts[b], a.p.cap);
    uint32_t used = n;  // used pairs are a prefix (the terminator rule)
    for (uint32_t i = lane; i < n; i += 64)
        if (a.pair_fetch[base + i] == kNone) used = min(used, i);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) used = min(used, (uint32_t)__shfl_xor(used, o));
    bool failed = false;
    for (uint32_t i = lane; i < used; i += 64) failed |= a.fetch_len[a.pair_fetch[base + i]] == UINT32_MAX;
    if (wave_any(failed)) {
        st |= SDFS_CDC_READ_FETCH;
    } else {
        bool oob = false;
        for (uint32_t i = lane; i < used; i += 64) {
            const int64_t ck = a.fetch_len[a.pair_fetch[base + i]];
            const int64_t nlen = a.p.nlen[base + i], pos = a.p.pos[base + i], off = a.p.offset[base + i];
            const int64_t c = nlen > ck ? ck : nlen;
            oob |= pos > (int64_t)a.chunk_length || pos + c > (int64_t)a.chunk_length || off + c > ck;
        }
        if (wave_any(oob)) st |= SDFS_CDC_READ_BOUNDS;
    }
    if (st) used = 0;
    if (lane == 0) {
        a.p.status[b] = st;
        a.nused[b] = used;
    }
    int32_t carry = INT_MIN;
    for (uint32_t i0 = 0; i0 < used; i0 += 64) {
        const uint32_t i = i0 + lane;
        int32_t e = INT_MIN;
        if (i < used) {
            const uint32_t f = a.pair_fetch[base + i];
            const int64_t ck = a.fetch_len[f];
            const int64_t nlen = a.p.nlen[base + i];
            const int64_t c = nlen > ck ? ck : nlen;
            e = (int32_t)(a.p.pos[base + i] + c);  // <= chunk_length <= INT32_MAX
            a.end[base + i] = e;
            a.src[base + i] = a.fetch_off[f] + (uint64_t)a.p.offset[base + i];
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int32_t v = __shfl_up(e, o);
            if (lane >= (uint32_t)o) e = max(e, v);
        }
        e = max(e, carry);
        if (i < used) a.maxend[base + i] = e;
        carry = __shfl(e, 63);
    }
}

// view of one buffer's placed pairs (LDS or global)
struct PairView {
    const int32_t* pos;
    const int32_t* end;
    const int32_t* maxend;
    const uint64_t* src;
    int32_t n;
};

// byte x of the buffer; k = floor entry of some x' <= x
__device__ __forceinline__ uint8_t gather_byte(const PairView& v, const uint8_t* chunks, int32_t x, int32_t& k) {
    while (k + 1 < v.n && v.pos[k + 1] <= x) k++;
    for (int32_t j = k; j >= 0 && v.maxend[j] > x; j--)  // the last pair in pos order that covers x
        if (v.end[j] > x) return chunks[v.src[j] + (uint64_t)(x - v.pos[j])];
    return 0;
}

// One 64 KiB tile (kTileVecs vectors from v0) of the bytes [start, start + len) of a buffer, which
// go to ob[0 .. len): the whole buffer (start 0, len chunk_length) for gather_kernel, a piece of
// one for gather_pieces_kernel.  pv holds the pairs that can supply a byte of the range; head =
// ob & 15 and nvec = the range's vectors at absolute 16-byte addresses (range_vecs), v0 < nvec.
__device__ __forceinline__ uint64_t range_vecs(uint32_t head, uint32_t len) { return ((uint64_t)head + len + 15) / 16; }

template <bool WHOLE>  // WHOLE: the range is the buffer, start = 0
__device__ __forceinline__ void gather_tile(const PairView& pv, const uint8_t* chunks, uint8_t* ob, int64_t start_,
                                            int64_t len, uint32_t head, uint64_t nvec, uint64_t v0, uint32_t tid) {
    const int64_t start = WHOLE ? 0 : start_;
    // per group of kIt vectors a lane makes three passes, so that the source loads of all of them
    // are in flight together: classify, load, realign + store
    constexpr int kIt = 4;
    enum : uint32_t { kSkip, kCopy, kZero, kBytes, kEdge };
    int32_t k = -2;
#pragma unroll 1
    for (uint64_t g0 = v0; g0 < min(v0 + kTileVecs, nvec); g0 += kIt * kGatherThreads) {
    const uint64_t w0 = g0 + tid;  // the lane's vectors: w0 + it * kGatherThreads
    uint32_t mode[kIt];
    int32_t kf[kIt];
    uintptr_t sa[kIt];
#pragma unroll
    for (int it = 0; it < kIt; it++) {
        mode[it] = kSkip;
        kf[it] = -1;
        sa[it] = 0;
        const uint64_t v = w0 + (uint64_t)it * kGatherThreads;
        if (v >= nvec) continue;
        const int64_t r = (int64_t)v * 16 - head;  // offset in the range of the vector's first byte
        const int64_t o = start + r;               // its buffer offset
        const int32_t x0 = (int32_t)max<int64_t>(o, start);
        k = floor_index(pv.pos, pv.n, x0, k);  // the largest pos <= x0
        kf[it] = k;
        if (r < 0 || r + 16 > len) {  // an end of the range that is not 16-byte aligned
            mode[it] = kEdge;
            continue;
        }
        const int64_t next = k + 1 < pv.n ? pv.pos[k + 1] : INT64_MAX;
        if (next >= o + 16 && k >= 0 && pv.end[k] >= o + 16) {
            mode[it] = kCopy;
            sa[it] = reinterpret_cast<uintptr_t>(chunks + pv.src[k] + (uint64_t)(x0 - pv.pos[k]));
        } else if (next >= o + 16 && (k < 0 || pv.maxend[k] <= o)) {
            mode[it] = kZero;
        } else {
            mode[it] = kBytes;
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
        if (sh) hi[it] = ap[1];  // holds bytes the vector needs: inside the chunk area
    }
#pragma unroll
    for (int it = 0; it < kIt; it++) {
        if (mode[it] == kSkip) continue;
        const uint64_t v = w0 + (uint64_t)it * kGatherThreads;
        const int64_t r = (int64_t)v * 16 - head;
        const int64_t o = start + r;
        uint8_t* dst = ob + r;
        int32_t kk = kf[it];
        if (mode[it] == kEdge) {
            for (int j = 0; j < 16; j++)
                if (r + j >= 0 && r + j < len) dst[j] = gather_byte(pv, chunks, (int32_t)(o + j), kk);
            continue;
        }
        uint4 w = make_uint4(0, 0, 0, 0);
        if (mode[it] == kCopy) {
            const uint32_t sh = (uint32_t)(sa[it] & 15), q = sh >> 2, rb = sh & 3;
            const uint4 l = lo[it], h = hi[it];
            uint32_t t0, t1, t2, t3, t4;
            if (q == 0) { t0 = l.x; t1 = l.y; t2 = l.z; t3 = l.w; t4 = h.x; }
            else if (q == 1) { t0 = l.y; t1 = l.z; t2 = l.w; t3 = h.x; t4 = h.y; }
            else if (q == 2) { t0 = l.z; t1 = l.w; t2 = h.x; t3 = h.y; t4 = h.z; }
            else { t0 = l.w; t1 = h.x; t2 = h.y; t3 = h.z; t4 = h.w; }
            w.x = __builtin_amdgcn_alignbyte(t1, t0, rb);
            w.y = __builtin_amdgcn_alignbyte(t2, t1, rb);
            w.z = __builtin_amdgcn_alignbyte(t3, t2, rb);
            w.w = __builtin_amdgcn_alignbyte(t4, t3, rb);
        } else if (mode[it] == kBytes) {
            uint32_t ws[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint32_t word = 0;
#pragma unroll
                for (int bb = 0; bb < 4; bb++)
                    word |= (uint32_t)gather_byte(pv, chunks, (int32_t)o + 4 * j + bb, kk) << (8 * bb);
                ws[j] = word;
            }
            w = make_uint4(ws[0], ws[1], ws[2], ws[3]);
        }
        *reinterpret_cast<uint4*>(dst) = w;
    }
    }
}

template <bool LDS>
__global__ __launch_bounds__(kGatherThreads) void gather_kernel(AsmArgs a) {
    __shared__ int32_t s_pos[LDS ? kLdsPairs : 1], s_end[LDS ? kLdsPairs : 1], s_max[LDS ? kLdsPairs : 1];
    __shared__ uint64_t s_src[LDS ? kLdsPairs : 1];
    const uint32_t b = blockIdx.x / a.tiles_per_buf;
    const uint32_t tile = blockIdx.x % a.tiles_per_buf;
    const uint32_t tid = threadIdx.x;
    uint8_t* ob = a.out + (uint64_t)b * a.chunk_length;
    const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(ob) & 15);
    const uint64_t nvec = range_vecs(head, a.chunk_length);
    const uint64_t v0 = (uint64_t)tile * kTileVecs;
    if (v0 >= nvec) return;  // uniform over the workgroup
    const uint64_t base = (uint64_t)b * a.p.cap;
    PairView pv{a.p.pos + base, a.end + base, a.maxend + base, a.src + base, (int32_t)a.nused[b]};
    if (LDS) {
        if (pv.n > (int32_t)kLdsPairs) pv.n = 0;  // not reached: the host picks the global form above kLdsPairs
        for (int32_t i = tid; i < pv.n; i += kGatherThreads) {
            s_pos[i] = pv.pos[i];
            s_end[i] = pv.end[i];
            s_max[i] = pv.maxend[i];
            s_src[i] = pv.src[i];
        }
        __syncthreads();
        pv.pos = s_pos;
        pv.end = s_end;
        pv.maxend = s_max;
        pv.src = s_src;
    }
    gather_tile<true>(pv, a.chunks, ob, 0, a.chunk_length, head, nvec, v0, tid);
}

// ---------------------------------------------------------------------------------------- pieces
// Ranged reads (sdfs_cdc_read_plan_pieces / sdfs_cdc_read_assemble_pieces): the unit is a piece
// {row, start, len, out_off}, a byte range of one buffer.  Only the pairs that touch a piece (nlen
// > 0, pos < start + len, pos + nlen > start) decide its status and are fetched.

struct PieceArgs {
    uint32_t nbuf;  // rows in the pairs
    uint32_t n_pieces;
    const uint32_t* row;  // >= nbuf (SDFS_CDC_READ_NONE): no row, the piece reads as zeros
    const uint32_t* start;
    const uint32_t* len;
    const uint64_t* out_off;  // assemble only
    uint32_t* status;
    const uint32_t* req;   // assemble only, optional: the piece's request,
    uint32_t n_requests;
    uint32_t* req_status;  // whose status is the OR of its pieces'
};

// the first i < n with key[i] >= x (key ascending), n if none
__device__ __forceinline__ uint32_t first_at_least(const int32_t* key, uint32_t n, int64_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (key[mid] >= x) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ uint32_t row_pairs(const sdfs_cdc_pairs& p, uint32_t b) {
    return (p.status[b] & SDFS_CDC_READ_CORRUPT) ? 0 : min(p.counts[b], p.cap);
}

// pairs before the first hashloc == 0 (the terminator rule), the same for every lane
__device__ __forceinline__ uint32_t row_used(const sdfs_cdc_pairs& p, uint64_t base, uint32_t n, uint32_t lane) {
    uint32_t used = n;
    for (uint32_t i = lane; i < n; i += 64)
        if (p.hashloc[base + i] == 0) used = min(used, i);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) used = min(used, (uint32_t)__shfl_xor(used, o));
    return used;
}

// one wave per row: the terminator, and "nobody needs it" for every slot
__global__ __launch_bounds__(64) void plan_rows_kernel(PlanArgs a, uint32_t* used) {
    const uint32_t lane = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const uint64_t base = (uint64_t)b * a.p.cap;
    const uint32_t u = row_used(a.p, base, row_pairs(a.p, b), lane);
    for (uint32_t i = lane; i < a.p.cap; i += 64) a.pair_fetch[base + i] = kNone;
    if (lane == 0) used[b] = u;
}

// one wave per piece: CORRUPT / MISSING, then the directory entries of its touching pairs.
// Pieces that touch the same pair, or pairs of the same entry, store the same values.
__global__ __launch_bounds__(64) void plan_mark_pieces_kernel(PlanArgs a, PieceArgs q, const uint32_t* used) {
    const uint32_t lane = threadIdx.x;
    const uint32_t p = blockIdx.x;
    const uint32_t row = q.row[p];
    uint32_t st = 0;
    if (row < q.nbuf) {  // wave-uniform
        if (a.p.status[row] & SDFS_CDC_READ_CORRUPT) {
            st = SDFS_CDC_READ_CORRUPT;
        } else {
            const uint64_t base = (uint64_t)row * a.p.cap;
            const int64_t start = q.start[p], end = start + (int64_t)q.len[p];
            const uint32_t hi = first_at_least(a.p.pos + base, used[row], end);  // pos < start + len below it
            bool missing = false;
            for (uint32_t i = lane; i < hi; i += 64) {
                const int64_t nlen = a.p.nlen[base + i];
                if (nlen == 0 || a.p.pos[base + i] + nlen <= start) continue;
                const uint64_t hl = a.p.hashloc[base + i];
                missing |= hl < a.pos_base || hl - a.pos_base >= a.n_store;
            }
            if (wave_any(missing)) {
                st = SDFS_CDC_READ_MISSING;
            } else {
                for (uint32_t i = lane; i < hi; i += 64) {
                    const int64_t nlen = a.p.nlen[base + i];
                    if (nlen == 0 || a.p.pos[base + i] + nlen <= start) continue;
                    const uint32_t f = (uint32_t)(a.p.hashloc[base + i] - a.pos_base);
                    a.pair_fetch[base + i] = f;
                    a.mark[f] = 1;
                }
            }
        }
    }
    if (lane == 0) q.status[p] = st;
}

struct PieceWork {
    uint8_t* bad;          // [nbuf*cap] 0, SDFS_CDC_READ_FETCH or SDFS_CDC_READ_BOUNDS per pair
    uint32_t* win_lo;      // [n_pieces] the piece's window of pairs: first index in its row,
    uint32_t* win_n;       // [n_pieces] and length
    uint32_t* tiles;       // [n_pieces] 64 KiB tiles of the piece's output
    uint32_t* tile_first;  // [n_pieces + 1] their exclusive prefix
    uint32_t* any_big;     // [1] set when some piece's window exceeds kLdsPairs
};

// one wave per row: each pair's {end, running max of end, source offset}.  A pair that places
// nothing — past the terminator, not needed, a failed fetch, out of bounds — gets end = pos, so it
// covers no byte and does not raise the running max above any byte at or after its pos.
__global__ __launch_bounds__(64) void pieces_rows_kernel(AsmArgs a, PieceWork w) {
    const uint32_t lane = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const uint64_t base = (uint64_t)b * a.p.cap;
    const uint32_t n = row_pairs(a.p, b);
    const uint32_t used = row_used(a.p, base, n, lane);
    int32_t carry = INT_MIN;
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        const uint32_t i = i0 + lane;
        int32_t e = INT_MIN;
        if (i < n) {
            const int64_t pos = a.p.pos[base + i];
            const uint32_t f = i < used ? a.pair_fetch[base + i] : kNone;
            uint32_t bad = 0;
            uint64_t src = 0;
            e = (int32_t)pos;
            if (f != kNone) {
                const int64_t ck = a.fetch_len[f];
                const int64_t nlen = a.p.nlen[base + i], off = a.p.offset[base + i];
                const int64_t c = nlen > ck ? ck : nlen;
                if (ck == (int64_t)UINT32_MAX) {
                    bad = SDFS_CDC_READ_FETCH;
                } else if (pos > (int64_t)a.chunk_length || pos + c > (int64_t)a.chunk_length || off + c > ck) {
                    bad = SDFS_CDC_READ_BOUNDS;
                } else {
                    e = (int32_t)(pos + c);  // <= chunk_length <= INT32_MAX
                    src = a.fetch_off[f] + (uint64_t)off;
                }
            }
            a.end[base + i] = e;
            a.src[base + i] = src;
            w.bad[base + i] = (uint8_t)bad;
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int32_t v = __shfl_up(e, o);
            if (lane >= (uint32_t)o) e = max(e, v);
        }
        e = max(e, carry);
        if (i < n) a.maxend[base + i] = e;
        carry = __shfl(e, 63);
    }
}

// one wave per piece: FETCH / BOUNDS from its touching pairs, its window, its tile count
__global__ __launch_bounds__(64) void pieces_status_kernel(AsmArgs a, PieceArgs q, PieceWork w) {
    const uint32_t lane = threadIdx.x;
    const uint32_t p = blockIdx.x;
    const uint32_t row = q.row[p];
    uint32_t st = q.status[p], lo = 0, cnt = 0;
    if (row < q.nbuf && st == 0) {  // wave-uniform
        const uint64_t base = (uint64_t)row * a.p.cap;
        const int64_t start = q.start[p], end = start + (int64_t)q.len[p];
        const uint32_t hi = first_at_least(a.p.pos + base, row_pairs(a.p, row), end);
        bool failed = false, oob = false;
        for (uint32_t i = lane; i < hi; i += 64) {
            const int64_t nlen = a.p.nlen[base + i];
            if (nlen == 0 || a.p.pos[base + i] + nlen <= start) continue;
            failed |= w.bad[base + i] == SDFS_CDC_READ_FETCH;
            oob |= w.bad[base + i] == SDFS_CDC_READ_BOUNDS;
        }
        if (wave_any(failed)) st = SDFS_CDC_READ_FETCH;
        else if (wave_any(oob)) st = SDFS_CDC_READ_BOUNDS;
        if (st == 0) {  // the window: maxend and pos are ascending
            lo = first_at_least(a.maxend + base, hi, start + 1);
            cnt = hi - lo;
        }
    }
    if (lane == 0) {
        const uint64_t head = reinterpret_cast<uintptr_t>(a.out + q.out_off[p]) & 15;
        const uint64_t nvec = (head + q.len[p] + 15) / 16;
        q.status[p] = st;
        if (st && q.req_status && q.req[p] < q.n_requests) atomicOr(&q.req_status[q.req[p]], st);
        if (cnt > kLdsPairs) *w.any_big = 1;
        w.win_lo[p] = lo;
        w.win_n[p] = cnt;
        w.tiles[p] = q.len[p] ? (uint32_t)((nvec + kTileVecs - 1) / kTileVecs) : 0;
    }
}

// The gather of the pieces: the tiles of all pieces in one list, walked with a grid stride.  A
// tile finds its piece by a floor search in the prefix of the tile counts.  Two forms share the
// list: LDS takes the tiles of the pieces whose window of pairs fits kLdsPairs and stages it (a
// piece without a row or with a status has an empty window and is zero-filled here); the other
// takes the tiles of the larger windows and searches them in global memory — it returns at once
// when the status kernel saw no such piece.
template <bool LDS>
__global__ __launch_bounds__(kGatherThreads) void gather_pieces_kernel(AsmArgs a, PieceArgs q, PieceWork w) {
    __shared__ int32_t s_pos[LDS ? kLdsPairs : 1], s_end[LDS ? kLdsPairs : 1], s_max[LDS ? kLdsPairs : 1];
    __shared__ uint64_t s_src[LDS ? kLdsPairs : 1];
    if (!LDS && *w.any_big == 0) return;
    const uint32_t tid = threadIdx.x;
    const uint32_t total = w.tile_first[q.n_pieces];
    for (uint32_t t = blockIdx.x; t < total; t += gridDim.x) {  // uniform over the workgroup
        // the tile's piece is the same for every lane: keep what describes it in scalar registers
        const uint32_t p = uni((uint32_t)floor_index<uint32_t>(w.tile_first, (int32_t)q.n_pieces, t, -2));
        const int32_t n = (int32_t)uni(w.win_n[p]);
        if ((n <= (int32_t)kLdsPairs) != LDS) continue;
        const uint64_t v0 = (uint64_t)uni(t - w.tile_first[p]) * kTileVecs;
        const uint64_t base = n ? (uint64_t)uni(q.row[p]) * a.p.cap + uni(w.win_lo[p]) : 0;
        const uint64_t oo = q.out_off[p];
        uint8_t* ob = a.out + ((uint64_t)uni((uint32_t)(oo >> 32)) << 32 | uni((uint32_t)oo));
        const uint32_t start = uni(q.start[p]), len = uni(q.len[p]);
        const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(ob) & 15);
        PairView pv{a.p.pos + base, a.end + base, a.maxend + base, a.src + base, n};
        if (LDS) {
            __syncthreads();  // the tile before this one is done with the arrays
            for (int32_t i = tid; i < n; i += kGatherThreads) {
                s_pos[i] = pv.pos[i];
                s_end[i] = pv.end[i];
                s_max[i] = pv.maxend[i];
                s_src[i] = pv.src[i];
            }
            __syncthreads();
            pv.pos = s_pos;
            pv.end = s_end;
            pv.maxend = s_max;
            pv.src = s_src;
        }
        gather_tile<false>(pv, a.chunks, ob, start, len, head, range_vecs(head, len), v0, tid);
    }
}

// --------------------------------------------------------------------------------------- verify

struct VerifyArgs {
    sdfs_cdc_pairs p;
    uint32_t hash_len;
    const uint32_t* pair_fetch;
    const uint32_t* fetch_len;
    const uint8_t* digests;  // [fetch*32]
    uint8_t* pair_bad;
    uint32_t* bad_count;
};

__global__ __launch_bounds__(64) void verify_compare_kernel(VerifyArgs a) {
    const uint32_t lane = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const uint64_t base = (uint64_t)b * a.p.cap;
    uint32_t nbad = 0;
    for (uint32_t i = lane; i < a.p.cap; i += 64) {
        const uint32_t f = a.pair_fetch[base + i];
        uint32_t bad = 0;
        if (f != kNone && a.fetch_len[f] != UINT32_MAX) {
            const uint8_t* h = a.p.hashes + (base + i) * 32;
            const uint8_t* d = a.digests + (uint64_t)f * 32;
            for (uint32_t k = 0; k < a.hash_len; k++) bad |= h[k] != d[k];
        }
        a.pair_bad[base + i] = (uint8_t)bad;
        nbad += bad;
    }
    nbad = wave_sum(nbad);
    if (lane == 0) a.bad_count[b] = nbad;
}

// ----------------------------------------------------------------------------------------- host

}  // namespace
}  // namespace sdfs

using namespace sdfs;

extern "C" {

uint32_t sdfs_cdc_map_pair_cap(uint32_t slot_bytes, uint32_t hash_len) {
    return pair_cap(slot_bytes, hash_len);
}

int sdfs_cdc_map_parse(int device, uint32_t nbuf, const uint8_t* d_map, uint32_t slot_bytes, uint32_t hash_len,
                       const sdfs_cdc_pairs* pairs, void* stream) {
    if (!pairs_complete(pairs)) return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_pairs");
    if (const int rc = check_hash_len(hash_len, HashOf::kPair)) return rc;
    if (slot_bytes < kSlotFixedBytes) return fail_status(SDFS_CDC_EINVAL, "slot_bytes %u < 13", slot_bytes);
    if (pairs->cap < sdfs_cdc_map_pair_cap(slot_bytes, hash_len))
        return fail_status(SDFS_CDC_ECAP, "pairs.cap %u < %u pairs a %u-byte slot can hold", pairs->cap,
                           sdfs_cdc_map_pair_cap(slot_bytes, hash_len), slot_bytes);
    if (nbuf && !d_map) return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (nbuf == 0) return SDFS_CDC_OK;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    Scratch sc(s);
    ParseArgs a{d_map, slot_bytes, hash_len, *pairs, nullptr, nullptr};
    SDFS_TRY(sc.get(&a.tmp_pos, (size_t)nbuf * pairs->cap));
    SDFS_TRY(sc.get(&a.tmp_dead, (size_t)nbuf * pairs->cap));
    hipLaunchKernelGGL(map_parse_kernel, dim3(nbuf), dim3(64), 0, s, a);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_read_plan(int device, uint32_t nbuf, const sdfs_cdc_pairs* pairs, uint64_t pos_base, uint64_t n_store,
                       const uint64_t* d_store_off, const uint32_t* d_store_len, const uint32_t* d_store_raw_len,
                       uint32_t* d_pair_fetch, uint32_t* d_fetch_count, uint64_t* d_src_off, uint32_t* d_src_len,
                       uint64_t* d_dst_off, uint32_t* d_dst_cap, uint64_t* d_plain_off, uint64_t* d_total_bytes,
                       void* stream) {
    if (!pairs_complete(pairs)) return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_pairs");
    if (!d_fetch_count || !d_total_bytes || (nbuf && !d_pair_fetch)) return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_store && (!d_store_off || !d_store_len || !d_store_raw_len || !d_src_off || !d_src_len || !d_dst_off ||
                    !d_dst_cap))
        return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_store >= UINT32_MAX) return fail_status(SDFS_CDC_EINVAL, "n_store %llu: fetch indices are 32-bit",
                                                  (unsigned long long)n_store);
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    Scratch sc(s);
    PlanArgs a{*pairs,    pos_base,  n_store,   d_store_off, d_store_len, d_store_raw_len, d_pair_fetch, d_fetch_count,
               d_src_off, d_src_len, d_dst_off, d_dst_cap,   d_plain_off, d_total_bytes,   nullptr};
    SDFS_TRY(sc.get(&a.mark, (size_t)n_store));
    SDFS_TRY(hipMemsetAsync(a.mark, 0, std::max<size_t>(n_store, 1) * 4, s));
    if (nbuf) hipLaunchKernelGGL(plan_mark_kernel, dim3(nbuf), dim3(64), 0, s, a);
    hipLaunchKernelGGL(plan_scan_kernel, dim3(1), dim3(1024), 0, s, a);
    const uint64_t slots = (uint64_t)nbuf * pairs->cap;
    if (slots)
        hipLaunchKernelGGL(plan_remap_kernel, dim3((uint32_t)((slots + 255) / 256)), dim3(256), 0, s, d_pair_fetch, slots,
                           a.mark);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_read_chain_lens(int device, const uint32_t* d_in_len, const uint32_t* d_count, uint64_t n_max,
                             uint32_t* d_out_len, void* stream) {
    if (n_max && (!d_in_len || !d_out_len)) return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_max >= (1ull << 39)) return fail_status(SDFS_CDC_EINVAL, "n_max %llu too large", (unsigned long long)n_max);
    if (n_max == 0) return SDFS_CDC_OK;
    if (const int rc = set_device(device)) return rc;
    hipLaunchKernelGGL(chain_lens_kernel, dim3((uint32_t)((n_max + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), d_in_len, d_count, n_max, d_out_len);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_read_assemble(int device, uint32_t nbuf, uint32_t chunk_length, const sdfs_cdc_pairs* pairs,
                           const uint32_t* d_pair_fetch, const uint8_t* d_chunks, const uint64_t* d_fetch_off,
                           const uint32_t* d_fetch_len, uint8_t* d_out, void* stream) {
    if (!pairs_complete(pairs)) return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_pairs");
    if (const int rc = check_chunk_length(chunk_length)) return rc;
    if (nbuf && (!d_pair_fetch || !d_chunks || !d_fetch_off || !d_fetch_len || !d_out))
        return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (nbuf == 0) return SDFS_CDC_OK;
    const uint32_t tiles = (uint32_t)(((uint64_t)chunk_length + 30) / 16 / kTileVecs + 1);
    if ((uint64_t)tiles * nbuf > (uint64_t)INT32_MAX)
        return fail_status(SDFS_CDC_EINVAL, "%u buffers of %u bytes: split the batch", nbuf, chunk_length);
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    Scratch sc(s);
    AsmArgs a{*pairs, nbuf, chunk_length, d_pair_fetch, d_chunks, d_fetch_off, d_fetch_len, d_out,
              nullptr, nullptr, nullptr, nullptr, tiles};
    const size_t slots = (size_t)nbuf * pairs->cap;
    SDFS_TRY(sc.get(&a.nused, nbuf));
    SDFS_TRY(sc.get(&a.end, slots));
    SDFS_TRY(sc.get(&a.maxend, slots));
    SDFS_TRY(sc.get(&a.src, slots));
    hipLaunchKernelGGL(assemble_status_kernel, dim3(nbuf), dim3(64), 0, s, a);
    const dim3 grid((uint32_t)((uint64_t)tiles * nbuf));
    if (pairs->cap <= kLdsPairs) hipLaunchKernelGGL(gather_kernel<true>, grid, dim3(kGatherThreads), 0, s, a);
    else hipLaunchKernelGGL(gather_kernel<false>, grid, dim3(kGatherThreads), 0, s, a);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_read_split(const sdfs_cdc_read_file* files, uint32_t n_files, const sdfs_cdc_read_request* requests,
                        uint32_t n_requests, uint32_t chunk_length, int64_t* n_read, uint32_t piece_cap,
                        uint32_t* piece_req, uint32_t* piece_row, uint32_t* piece_start, uint32_t* piece_len,
                        uint64_t* piece_out_off, uint32_t row_cap, uint64_t* row_slot, uint64_t* n_pieces,
                        uint64_t* n_rows) {
    const char* why = "";
    const int rc = read_split(files, n_files, requests, n_requests, chunk_length, n_read, piece_cap, piece_req, piece_row,
                              piece_start, piece_len, piece_out_off, row_cap, row_slot, n_pieces, n_rows, &why);
    if (rc == SDFS_CDC_ECAP)
        return fail_status(rc, "%llu pieces of %llu rows: piece_cap %u, row_cap %u", (unsigned long long)*n_pieces,
                           (unsigned long long)*n_rows, piece_cap, row_cap);
    return rc ? fail_status(rc, "%s", why) : SDFS_CDC_OK;
}

int sdfs_cdc_read_plan_pieces(int device, uint32_t nbuf, const sdfs_cdc_pairs* pairs, uint64_t pos_base,
                              uint64_t n_store, const uint64_t* d_store_off, const uint32_t* d_store_len,
                              const uint32_t* d_store_raw_len, uint32_t n_pieces, const uint32_t* d_piece_row,
                              const uint32_t* d_piece_start, const uint32_t* d_piece_len, uint32_t* d_piece_status,
                              uint32_t* d_pair_fetch, uint32_t* d_fetch_count, uint64_t* d_src_off, uint32_t* d_src_len,
                              uint64_t* d_dst_off, uint32_t* d_dst_cap, uint64_t* d_plain_off, uint64_t* d_total_bytes,
                              void* stream) {
    if (!pairs_complete(pairs)) return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_pairs");
    if (!d_fetch_count || !d_total_bytes || (nbuf && !d_pair_fetch)) return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_store && (!d_store_off || !d_store_len || !d_store_raw_len || !d_src_off || !d_src_len || !d_dst_off ||
                    !d_dst_cap))
        return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_pieces && (!d_piece_row || !d_piece_start || !d_piece_len || !d_piece_status))
        return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_store >= UINT32_MAX) return fail_status(SDFS_CDC_EINVAL, "n_store %llu: fetch indices are 32-bit",
                                                  (unsigned long long)n_store);
    if (n_pieces > (uint32_t)INT32_MAX) return fail_status(SDFS_CDC_EINVAL, "%u pieces: split the batch", n_pieces);
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    Scratch sc(s);
    PlanArgs a{*pairs,    pos_base,  n_store,   d_store_off, d_store_len, d_store_raw_len, d_pair_fetch, d_fetch_count,
               d_src_off, d_src_len, d_dst_off, d_dst_cap,   d_plain_off, d_total_bytes,   nullptr};
    const PieceArgs q{nbuf, n_pieces, d_piece_row, d_piece_start, d_piece_len, nullptr, d_piece_status, nullptr, 0, nullptr};
    uint32_t* used = nullptr;
    SDFS_TRY(sc.get(&a.mark, (size_t)n_store));
    SDFS_TRY(sc.get(&used, nbuf));
    SDFS_TRY(hipMemsetAsync(a.mark, 0, std::max<size_t>(n_store, 1) * 4, s));
    if (nbuf) hipLaunchKernelGGL(plan_rows_kernel, dim3(nbuf), dim3(64), 0, s, a, used);
    if (n_pieces) hipLaunchKernelGGL(plan_mark_pieces_kernel, dim3(n_pieces), dim3(64), 0, s, a, q, used);
    hipLaunchKernelGGL(plan_scan_kernel, dim3(1), dim3(1024), 0, s, a);
    const uint64_t slots = (uint64_t)nbuf * pairs->cap;
    if (slots)
        hipLaunchKernelGGL(plan_remap_kernel, dim3((uint32_t)((slots + 255) / 256)), dim3(256), 0, s, d_pair_fetch, slots,
                           a.mark);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_read_assemble_pieces(int device, uint32_t nbuf, uint32_t chunk_length, const sdfs_cdc_pairs* pairs,
                                  const uint32_t* d_pair_fetch, const uint8_t* d_chunks, const uint64_t* d_fetch_off,
                                  const uint32_t* d_fetch_len, uint32_t n_pieces, const uint32_t* d_piece_row,
                                  const uint32_t* d_piece_start, const uint32_t* d_piece_len,
                                  const uint64_t* d_piece_out_off, uint32_t* d_piece_status,
                                  const uint32_t* d_piece_req, uint32_t n_requests, uint32_t* d_req_status,
                                  uint8_t* d_out, void* stream) {
    if (!pairs_complete(pairs)) return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_pairs");
    if (const int rc = check_chunk_length(chunk_length)) return rc;
    if (nbuf && (!d_pair_fetch || !d_chunks || !d_fetch_off || !d_fetch_len))
        return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_pieces && (!d_piece_row || !d_piece_start || !d_piece_len || !d_piece_out_off || !d_piece_status || !d_out))
        return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (d_req_status && n_requests && n_pieces && !d_piece_req)
        return fail_status(SDFS_CDC_EINVAL, "d_req_status without d_piece_req");
    const uint32_t tiles = (uint32_t)(((uint64_t)chunk_length + 30) / 16 / kTileVecs + 1);  // of one piece, at most
    if ((uint64_t)tiles * n_pieces > (uint64_t)INT32_MAX)
        return fail_status(SDFS_CDC_EINVAL, "%u pieces of up to %u bytes: split the batch", n_pieces, chunk_length);
    if (n_pieces == 0 && !(d_req_status && n_requests)) return SDFS_CDC_OK;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (d_req_status && n_requests) SDFS_TRY(hipMemsetAsync(d_req_status, 0, (size_t)n_requests * 4, s));
    if (n_pieces == 0) return SDFS_CDC_OK;
    Scratch sc(s);
    AsmArgs a{*pairs, nbuf, chunk_length, d_pair_fetch, d_chunks, d_fetch_off, d_fetch_len, d_out,
              nullptr, nullptr, nullptr, nullptr, 0};
    const PieceArgs q{nbuf,           n_pieces,    d_piece_row, d_piece_start, d_piece_len, d_piece_out_off,
                      d_piece_status, d_piece_req, n_requests,  n_requests ? d_req_status : nullptr};
    PieceWork w{};
    const size_t slots = (size_t)nbuf * pairs->cap;
    uint32_t* per_piece = nullptr;  // win_lo, win_n, tiles, tile_first, any_big
    SDFS_TRY(sc.get(&a.end, slots));
    SDFS_TRY(sc.get(&a.maxend, slots));
    SDFS_TRY(sc.get(&a.src, slots));
    SDFS_TRY(sc.get(&w.bad, slots));
    SDFS_TRY(sc.get(&per_piece, (size_t)n_pieces * 4 + 2));
    w.win_lo = per_piece;
    w.win_n = per_piece + n_pieces;
    w.tiles = per_piece + (size_t)n_pieces * 2;
    w.tile_first = per_piece + (size_t)n_pieces * 3;
    w.any_big = per_piece + (size_t)n_pieces * 4 + 1;
    SDFS_TRY(hipMemsetAsync(w.any_big, 0, 4, s));
    if (nbuf) hipLaunchKernelGGL(pieces_rows_kernel, dim3(nbuf), dim3(64), 0, s, a, w);
    hipLaunchKernelGGL(pieces_status_kernel, dim3(n_pieces), dim3(64), 0, s, a, q, w);
    hipLaunchKernelGGL(prefix_kernel<uint32_t>, dim3(1), dim3(1024), 0, s, w.tiles, n_pieces, w.tile_first);
    const uint64_t bound = (uint64_t)tiles * n_pieces;  // of the tile count, known without a host read
    hipLaunchKernelGGL(gather_pieces_kernel<true>, dim3((uint32_t)std::min<uint64_t>(bound, kPieceGrid)),
                       dim3(kGatherThreads), 0, s, a, q, w);
    hipLaunchKernelGGL(gather_pieces_kernel<false>, dim3((uint32_t)std::min<uint64_t>(bound, kPieceGridBig)),
                       dim3(kGatherThreads), 0, s, a, q, w);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_read_verify(sdfs_cdc_engine* engine, uint32_t nbuf, const sdfs_cdc_pairs* pairs, uint32_t hash_len,
                         const uint32_t* d_pair_fetch, const uint8_t* d_chunks, const uint64_t* d_fetch_off,
                         const uint32_t* d_fetch_len, const uint32_t* d_fetch_count, uint64_t n_fetch_max,
                         uint8_t* d_pair_bad, uint32_t* d_bad_count, void* stream) {
    if (!engine) return fail_status(SDFS_CDC_EINVAL, "null engine");
    if (!pairs_complete(pairs)) return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_pairs");
    if (const int rc = check_hash_len(hash_len, HashOf::kPair)) return rc;
    if (nbuf && (!d_pair_fetch || !d_pair_bad || !d_bad_count)) return fail_status(SDFS_CDC_EINVAL, "null argument");
    if ((nbuf || n_fetch_max) && (!d_chunks || !d_fetch_off || !d_fetch_len))
        return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_fetch_max >= (1ull << 39))
        return fail_status(SDFS_CDC_EINVAL, "n_fetch_max %llu too large", (unsigned long long)n_fetch_max);
    const int dl = sdfs_cdc_digest_len(engine);
    if (dl < 0) return fail_status(SDFS_CDC_EINVAL, "not a live engine handle");
    if ((uint32_t)dl != hash_len)
        return fail_status(SDFS_CDC_EINVAL, "engine digests are %d bytes, the pairs hold %u", dl, hash_len);
    if (nbuf == 0) return SDFS_CDC_OK;
    hipPointerAttribute_t at;
    SDFS_TRY(hipPointerGetAttributes(&at, d_pair_bad));
    if (const int rc = set_device(at.device)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    Scratch sc(s);
    uint32_t* lens = nullptr;
    uint8_t* digests = nullptr;
    SDFS_TRY(sc.get(&lens, (size_t)n_fetch_max));
    SDFS_TRY(sc.get(&digests, (size_t)n_fetch_max * 32));
    if (n_fetch_max) {
        hipLaunchKernelGGL(chain_lens_kernel, dim3((uint32_t)((n_fetch_max + 255) / 256)), dim3(256), 0, s, d_fetch_len,
                           d_fetch_count, n_fetch_max, lens);
        SDFS_TRY(hipGetLastError());
        const int rc = sdfs_cdc_hash_device(engine, d_chunks, d_fetch_off, lens, d_fetch_count, n_fetch_max, digests, stream);
        if (rc) return rc;
    }
    VerifyArgs a{*pairs, hash_len, d_pair_fetch, d_fetch_len, digests, d_pair_bad, d_bad_count};
    hipLaunchKernelGGL(verify_compare_kernel, dim3(nbuf), dim3(64), 0, s, a);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

}  // extern "C"
