// store_open.hip — a chunk store reopened from its archive and .map images, and scrubbed
// (include/sdfs_store.h).
//
// Reference: SimpleByteArrayLongMap.setUp on an existing file (SimpleByteArrayLongMap.java:198-261)
// decides a map's geometry from the file length and the magic; next() (:136-175) walks the slots;
// index() / indexRehashed() (:340-400) and get() (:562-599) find a key; HashBlobArchive.getChunk
// (HashBlobArchive.java:1712-1950) reads [BE32 len][record] at the map's value.
//
// Everything read from an image is a claim, not a fact: map_geometry() bounds the slots by the
// file length the host handed in (itself bounded by the row stride before the launch), and
// check_record() compares a slot's position and length with the archive's bytes before it loads
// the length word, the key or the nz word through them.  The scan is three kernels: the filled
// slots per archive, their prefix over the archives, then one workgroup per archive that sorts
// (pos, slot) of the filled slots — bitonic, in LDS for maps of up to 16 Ki slots — and writes one
// record per thread.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/sdfs_store.h"
#include "block_scan.h"
#include "call_support.h"
#include "store_format.h"

namespace sdfs {
namespace {

constexpr uint32_t kNone = SDFS_CDC_ARCHIVE_NONE;
constexpr uint32_t kSortLds = SDFS_CDC_STORE_SORT_LDS;
constexpr uint32_t kEmitThreads = 1024;
constexpr uint32_t kLensPerLaunch = 256;

// 4 bytes as they lie (compared, never interpreted); p is 4-byte aligned when al4
__device__ __forceinline__ uint32_t raw32(const uint8_t* p, bool al4) {
    if (al4) return *reinterpret_cast<const uint32_t*>(p);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// the images of a store, as the scan and the lookup take them
struct Img {
    const uint8_t* store;
    uint64_t store_bytes;
    const uint64_t* arc_base;
    const uint64_t* arc_bytes;
    const uint8_t* maps;
    uint64_t map_stride;
    const uint64_t* map_len;  // device copy of the host array
    uint32_t n_arc;
    uint32_t hash_len;
    uint32_t version;
    uint32_t header_bytes;
    uint32_t al4;  // every map row starts at a 4-byte address (then every slot does)
};

struct Geo {
    uint32_t off, el, ver, size;
};

// setUp on an existing file of len bytes (len <= the row stride <= 2^31 - 1: checked on the host)
__device__ Geo map_geometry(const uint8_t* map, uint64_t len, uint32_t hash_len, uint32_t version) {
    Geo g{0, map_entry_bytes(hash_len, 0), 0, 0};
    if (version != 0) {
        if (len <= kMapHeaderBytes) return g;  // a new map: no entries
        if (map_has_magic(map)) {
            g.off = kMapHeaderBytes;
            g.el = map_entry_bytes(hash_len, 1);
            g.ver = get_be32(map + kMapVersionAt);
        }
    }
    g.size = (uint32_t)((len - g.off) / g.el);  // trailing bytes are ignored
    return g;
}

// the archive's bytes, 0 when the image does not lie inside the store
__device__ __forceinline__ uint64_t archive_bytes(const Img& im, uint32_t a) {
    const uint64_t base = im.arc_base[a], ab = im.arc_bytes[a];
    return (ab > im.store_bytes || base > im.store_bytes - ab) ? 0 : ab;
}

__device__ __forceinline__ bool slot_free(const uint8_t* slot, uint32_t hash_len, bool al4) {
    uint32_t any = 0;
    for (uint32_t i = 0; i < hash_len; i += 4) any |= raw32(slot + i, al4);
    return any == 0;
}

struct Rec {
    uint32_t pos, len, flags;
};

// A filled slot against the archive image img of ab bytes: RANGE / KEY / LEN.  Nothing is loaded
// from img before its offset is known to lie inside [header_bytes, ab).
__device__ Rec check_record(const Img& im, const Geo& g, const uint8_t* slot, const uint8_t* img, uint64_t ab) {
    const uint32_t hl = im.hash_len;
    const uint32_t v = get_be32(slot + hl + kMapPosAt);  // the map value: where the length word lies
    const uint64_t p = (uint64_t)v + kRecordLenBack;  // the record's first byte
    Rec r{v + kRecordLenBack, 0, 0};
    // the record's header [BE32 hl][key][BE32 len] starts at or after header_bytes, its length word ends by ab
    if (p < (uint64_t)im.header_bytes + record_header_bytes(hl) || p > ab || p > (uint64_t)UINT32_MAX) {
        r.flags = SDFS_CDC_STORE_RANGE;
        return r;
    }
    const uint32_t img_len = get_be32(img + p - kRecordLenBack);
    const uint32_t len = g.ver > 0 ? get_be32(slot + hl + kMapLenAt) : img_len;
    if (p + len > ab) {
        r.flags = SDFS_CDC_STORE_RANGE;
        return r;
    }
    r.len = len;
    if (g.ver > 0 && img_len != len) {
        r.flags |= SDFS_CDC_STORE_LEN;
        r.len = 0;
    }
    const uint8_t* h = img + p - record_header_bytes(hl);
    uint32_t diff = get_be32(h) ^ hl;
    for (uint32_t i = 0; i < hl; i++) diff |= (uint32_t)(h[4 + i] ^ slot[i]);
    if (diff) r.flags |= SDFS_CDC_STORE_KEY;
    return r;
}

// HashBlobArchive.getChunk's nz rule for the len bytes at rec: -> raw_len, NZ or-ed into flags
__device__ __forceinline__ uint32_t nz_rule(const uint8_t* rec, uint32_t len, uint32_t max_chunk, uint32_t& flags) {
    if (len < 4) {
        flags |= SDFS_CDC_STORE_NZ;
        return 0;
    }
    const int32_t nz = (int32_t)get_be32(rec);
    const uint32_t raw = nz > 0 ? (uint32_t)nz : len - 4;
    if (raw > max_chunk) {
        flags |= SDFS_CDC_STORE_NZ;
        return 0;
    }
    return raw;
}

// ----------------------------------------------------------------------------------------- scan

struct LenArgs {
    uint64_t* dst;
    uint32_t n;
    uint64_t v[kLensPerLaunch];  // by value: no copy to wait for
};

__global__ __launch_bounds__(256) void store_lens_kernel(LenArgs a) {
    if (threadIdx.x < a.n) a.dst[threadIdx.x] = a.v[threadIdx.x];
}

struct ScanArgs2 {
    Img im;
    sdfs_cdc_store_records r;
    sdfs_cdc_store_archives o;
    uint32_t max_chunk;
    uint32_t plain;
    uint32_t* cnt;        // [n_arc] filled slots (scratch)
    uint64_t* sort;       // global sort area, sort_stride entries per archive (maps above kSortLds slots)
    uint64_t sort_stride;
};

__global__ __launch_bounds__(256) void store_count_kernel(ScanArgs2 a) {
    __shared__ uint32_t s_cnt;
    const uint32_t arc = blockIdx.x;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const uint8_t* map = a.im.maps + (uint64_t)arc * a.im.map_stride;
    const Geo g = map_geometry(map, a.im.map_len[arc], a.im.hash_len, a.im.version);
    uint32_t n = 0;
    if (g.size <= a.o.slot_stride)
        for (uint32_t s = threadIdx.x; s < g.size; s += 256)
            n += !slot_free(map + g.off + (uint64_t)s * g.el, a.im.hash_len, a.im.al4);
    if (n) atomicAdd(&s_cnt, n);
    __syncthreads();
    if (threadIdx.x == 0) a.cnt[arc] = s_cnt;
}

// arc_first = the exclusive prefix of cnt; count, status (one block)
__global__ __launch_bounds__(1024) void store_prefix_kernel(ScanArgs2 a) {
    __shared__ uint64_t lds[16];
    const uint32_t t = threadIdx.x, n = a.im.n_arc;
    uint32_t a0, a1;
    block_run_1024(n, a0, a1);
    uint64_t sum = 0, total;
    for (uint32_t i = a0; i < a1; i++) sum += a.cnt[i];
    uint64_t run = block_exclusive_scan_1024(sum, lds, total);
    const bool fits = total <= a.r.n_cap;
    if (t == 0) {
        *a.r.count = (uint32_t)min(total, (uint64_t)UINT32_MAX);
        *a.r.status = fits ? 0 : SDFS_CDC_STORE_ECAP;
    }
    if (!fits) return;
    for (uint32_t i = a0; i < a1; i++) {
        a.o.arc_first[i] = (uint32_t)run;
        run += a.cnt[i];
    }
    if (t == 1023) a.o.arc_first[n] = (uint32_t)total;
}

template <bool LDS>
__global__ __launch_bounds__(kEmitThreads) void store_emit_kernel(ScanArgs2 a) {
    __shared__ uint64_t s_keys[LDS ? kSortLds : 1];
    __shared__ unsigned long long s_sum;
    __shared__ uint32_t s_n;
    if (*a.r.status) return;  // ECAP: only count and status
    const uint32_t t = threadIdx.x, arc = blockIdx.x, hl = a.im.hash_len;
    const uint8_t* map = a.im.maps + (uint64_t)arc * a.im.map_stride;
    const Geo g = map_geometry(map, a.im.map_len[arc], hl, a.im.version);
    const uint64_t base = a.im.arc_base[arc];
    const uint64_t ab = archive_bytes(a.im, arc);
    const uint8_t* img = a.im.store + base;  // nothing is loaded through it before check_record's bounds
    uint32_t* srow = a.o.slot_rec + (uint64_t)arc * a.o.slot_stride;
    if (t == 0) {
        s_sum = 0;
        s_n = 0;
        a.o.map_slots[arc] = g.size;
        a.o.version[arc] = g.ver;
    }
    if (a.im.header_bytes && t < 16) a.o.ivs[(uint64_t)arc * 16 + t] = ab >= 20 ? img[4 + t] : 0;
    if (g.size > a.o.slot_stride) {  // no row to write the slots' records to
        for (uint32_t s = t; s < a.o.slot_stride; s += kEmitThreads) srow[s] = kNone;
        if (t == 0) a.o.status[arc] = SDFS_CDC_STORE_SLOTS;
        return;
    }
    // cnt <= size <= slot_stride: the count kernel walked the same slots
    const uint32_t cnt = a.cnt[arc], first = a.o.arc_first[arc];
    uint32_t P = 1;
    while (P < cnt) P <<= 1;
    uint64_t* keys;
    if constexpr (LDS) keys = s_keys;
    else keys = a.sort + (uint64_t)arc * a.sort_stride;
    __syncthreads();  // s_n
    // (pos, slot) of every filled slot, in whatever order the lanes arrive: the sort settles it
    const uint32_t span = max(g.size, a.o.slot_stride);
    for (uint32_t s = t; s < span; s += kEmitThreads) {
        bool filled = false;
        if (s < g.size) {
            const uint8_t* slot = map + g.off + (uint64_t)s * g.el;
            if (!slot_free(slot, hl, a.im.al4)) {
                const uint32_t at = atomicAdd(&s_n, 1u);
                filled = at < cnt;  // always, unless the image changed under the scan
                if (filled) keys[at] = ((uint64_t)(get_be32(slot + hl + kMapPosAt) + kRecordLenBack) << 32) | s;
            }
        }
        if (s < a.o.slot_stride && !filled) srow[s] = kNone;
    }
    __syncthreads();
    for (uint32_t s = min(s_n, cnt) + t; s < P; s += kEmitThreads) keys[s] = UINT64_MAX;  // the padding sorts to the end
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t q = t; q < P / 2; q += kEmitThreads) {  // pair q of this pass: i < l = i | j
                const uint32_t i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), l = i | j;
                const uint64_t x = keys[i], y = keys[l];
                if ((x > y) == ((i & k) == 0)) {
                    keys[i] = y;
                    keys[l] = x;
                }
            }
            __syncthreads();
        }
    }
    uint64_t sum = 0;
    for (uint32_t i = t; i < cnt; i += kEmitThreads) {
        const uint32_t s = (uint32_t)keys[i];
        if (s >= g.size) continue;  // padding: only when the image changed under the scan
        const uint8_t* slot = map + g.off + (uint64_t)s * g.el;
        Rec rec = check_record(a.im, g, slot, img, ab);
        uint32_t raw = 0;
        if (!(rec.flags & (SDFS_CDC_STORE_RANGE | SDFS_CDC_STORE_LEN))) {
            if (a.plain) raw = nz_rule(img + rec.pos, rec.len, a.max_chunk, rec.flags);
            else if (rec.len < 4) rec.flags |= SDFS_CDC_STORE_NZ;
        }
        if (rec.flags == 0) sum += (uint64_t)record_header_bytes(hl) + rec.len;
        const uint64_t r = (uint64_t)first + i;  // < n_cap: the prefix kernel saw the total fit
        a.r.arc[r] = arc;
        a.r.slot[r] = s;
        a.r.pos[r] = rec.pos;
        a.r.len[r] = rec.len;
        a.r.store_off[r] = base + rec.pos;
        a.r.raw_len[r] = raw;
        a.r.flags[r] = rec.flags;
        uint8_t* key = a.r.key + r * 32;
        for (uint32_t b = 0; b < 32; b++) key[b] = b < hl ? slot[b] : 0;
        srow[s] = (uint32_t)r;
    }
    if (sum) atomicAdd(&s_sum, (unsigned long long)sum);
    __syncthreads();
    if (t == 0)
        a.o.status[arc] = (a.im.header_bytes + s_sum != a.im.arc_bytes[arc] || ab != a.im.arc_bytes[arc])
                              ? SDFS_CDC_STORE_GAP : 0;
}

// ------------------------------------------------------------------------------------- raw_lens

__global__ __launch_bounds__(256) void store_raw_lens_kernel(const uint8_t* plain, const uint64_t* off,
                                                             const uint32_t* len, const uint32_t* count,
                                                             uint64_t n_max, uint32_t max_chunk, uint32_t* raw_len,
                                                             uint32_t* flags) {
    const uint64_t n = live_count(count, n_max);
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t f = flags[i], raw = 0;
    if (f == 0) {
        const uint32_t l = len[i] == UINT32_MAX ? 0 : len[i];
        raw = nz_rule(l >= 4 ? plain + off[i] : plain, l, max_chunk, f);
        flags[i] = f;
    }
    raw_len[i] = raw;
}

// ------------------------------------------------------------------------------------ directory

struct DirArgs {
    const uint64_t* rec_off;
    const uint32_t* rec_len;
    const uint32_t* rec_raw;
    const uint32_t* rec_flags;
    const int64_t* hashloc;
    const uint32_t* count;
    uint64_t n_max, pos_base, n_store;
    uint64_t* store_off;
    uint32_t* store_len;
    uint32_t* store_raw;
    uint32_t* rec_of_k;
    uint64_t* info;
    uint32_t* owner;  // [n_store] scratch: the lowest ordinal that claims k
};

// -> the record's directory entry, or n_store when it has none
__device__ __forceinline__ uint64_t dir_entry(const DirArgs& a, uint64_t r, int& why) {
    const int64_t hl = a.hashloc[r];
    if (a.rec_flags[r] != 0 || hl < 0) {
        why = 0;  // orphan
        return a.n_store;
    }
    if ((uint64_t)hl < a.pos_base || (uint64_t)hl - a.pos_base >= a.n_store) {
        why = 1;  // out of range
        return a.n_store;
    }
    return (uint64_t)hl - a.pos_base;
}

__global__ __launch_bounds__(256) void store_dir_claim_kernel(DirArgs a) {
    const uint64_t n = live_count(a.count, a.n_max);
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    int why = 0;
    const uint64_t k = dir_entry(a, r, why);
    if (k < a.n_store) atomicMin(&a.owner[k], (uint32_t)r);
    else add64(&a.info[why], 1);
}

__global__ __launch_bounds__(256) void store_dir_write_kernel(DirArgs a) {
    const uint64_t n = live_count(a.count, a.n_max);
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.n_store) {
        const uint32_t r = a.owner[i];
        const bool on = r != kNone;
        a.store_off[i] = on ? a.rec_off[r] : 0;
        a.store_len[i] = on ? a.rec_len[r] : 0;
        a.store_raw[i] = on ? a.rec_raw[r] : 0;
        a.rec_of_k[i] = r;
    }
    if (i < n) {
        int why = 0;
        const uint64_t k = dir_entry(a, i, why);
        if (k < a.n_store && a.owner[k] != (uint32_t)i) add64(&a.info[2], 1);
    }
}

// --------------------------------------------------------------------------------------- lookup

struct LookArgs {
    Img im;
    const uint32_t* q_arc;
    const uint8_t* q_key;
    uint64_t n_q;
    uint32_t* slot;
    uint32_t* pos;
    uint32_t* len;
    uint64_t* store_off;
    uint32_t* flags;
};

__global__ __launch_bounds__(256) void store_lookup_kernel(LookArgs a) {
    const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= a.n_q) return;
    const uint32_t arc = a.q_arc[q], hl = a.im.hash_len, nw = hl / 4;
    const uint8_t* key = a.q_key + q * 32;
    uint32_t kw[8], any = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; i++) {
        kw[i] = i < nw ? raw32(key + 4 * i, false) : 0;
        any |= kw[i];
    }
    uint32_t o_slot = kNone, o_pos = 0, o_len = 0, o_flags = 0;
    uint64_t o_off = 0;
    if (arc < a.im.n_arc && any) {
        const uint8_t* map = a.im.maps + (uint64_t)arc * a.im.map_stride;
        const Geo g = map_geometry(map, a.im.map_len[arc], hl, a.im.version);
        if (g.size) {
            const uint32_t h = map_key_hash(key);
            const uint32_t home = map_probe_home(h, g.size);
            const uint32_t step = map_probe_step_any(h, g.size);  // 0 for size <= 2: the home slot only
            uint32_t idx = home;
            for (uint32_t tries = 0; tries < g.size; tries++) {  // every slot lies below map_len: size = (len - off) / el
                const uint8_t* slot = map + g.off + (uint64_t)idx * g.el;
                uint32_t diff = 0, filled = 0;
#pragma unroll
                for (uint32_t i = 0; i < 8; i++) {
                    if (i < nw) {
                        const uint32_t w = raw32(slot + 4 * i, a.im.al4);
                        diff |= w ^ kw[i];
                        filled |= w;
                    }
                }
                if (!diff) {
                    const uint64_t ab = archive_bytes(a.im, arc);
                    const Rec rec = check_record(a.im, g, slot, a.im.store + a.im.arc_base[arc], ab);
                    o_slot = idx;
                    o_pos = rec.pos;
                    o_len = rec.len;
                    o_flags = rec.flags;
                    o_off = a.im.arc_base[arc] + rec.pos;
                    break;
                }
                if (!filled || !step) break;  // FREE: absent
                idx = map_probe_next(idx, step, g.size);
                if (idx == home) break;
            }
        }
    }
    a.slot[q] = o_slot;
    a.pos[q] = o_pos;
    a.len[q] = o_len;
    a.store_off[q] = o_off;
    a.flags[q] = o_flags;
}

// --------------------------------------------------------------------------------------- verify

__global__ __launch_bounds__(256) void store_verify_lens_kernel(const uint32_t* len, const uint32_t* flags,
                                                                const uint32_t* count, uint64_t n_max, uint32_t* out) {
    const uint64_t n = live_count(count, n_max);
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (len[i] == UINT32_MAX || (flags[i] & SDFS_CDC_STORE_UNREADABLE)) ? 0 : len[i];
}

__global__ __launch_bounds__(256) void store_verify_compare_kernel(const uint32_t* len, const uint8_t* keys,
                                                                   const uint8_t* digests, const uint32_t* count,
                                                                   uint64_t n_max, uint32_t hash_len, uint32_t* flags) {
    const uint64_t n = live_count(count, n_max);
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t f = flags[i];
    if (f & SDFS_CDC_STORE_UNREADABLE) return;
    if (len[i] == UINT32_MAX) {
        flags[i] = f | SDFS_CDC_STORE_FETCH;
        return;
    }
    uint32_t diff = 0;
    for (uint32_t b = 0; b < hash_len; b++) diff |= (uint32_t)(keys[i * 32 + b] ^ digests[i * 32 + b]);
    if (diff) flags[i] = f | SDFS_CDC_STORE_HASH;
}

// ----------------------------------------------------------------------------------------- host

// the checks the scan and the lookup share; 0 = fine
int check_images(uint32_t n_arc, const uint8_t* d_store, const uint64_t* d_arc_base, const uint64_t* d_arc_bytes,
                 const uint8_t* d_maps, uint64_t map_stride_bytes, const uint64_t* map_len, uint32_t hash_len,
                 uint32_t header_bytes) {
    if (const int rc = check_hash_len(hash_len, HashOf::kMapKey)) return rc;
    if (const int rc = check_header(header_bytes)) return rc;
    if (n_arc && (!d_store || !d_arc_base || !d_arc_bytes || !d_maps || !map_len))
        return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (map_stride_bytes > (uint64_t)INT32_MAX)
        return fail_status(SDFS_CDC_EINVAL, "map_stride_bytes %llu above 2^31 - 1: the reference's map size is an int",
                           (unsigned long long)map_stride_bytes);
    for (uint32_t a = 0; a < n_arc; a++)
        if (map_len[a] > map_stride_bytes)
            return fail_status(SDFS_CDC_EINVAL, "map %u is %llu bytes long, the rows are %llu apart", a,
                               (unsigned long long)map_len[a], (unsigned long long)map_stride_bytes);
    return SDFS_CDC_OK;
}

// the host's map lengths to device scratch, 256 per launch by value
hipError_t upload_lens(const uint64_t* map_len, uint32_t n_arc, uint64_t* d_len, hipStream_t s) {
    for (uint32_t a0 = 0; a0 < n_arc; a0 += kLensPerLaunch) {
        LenArgs la;
        la.dst = d_len + a0;
        la.n = std::min(kLensPerLaunch, n_arc - a0);
        for (uint32_t i = 0; i < kLensPerLaunch; i++) la.v[i] = i < la.n ? map_len[a0 + i] : 0;
        hipLaunchKernelGGL(store_lens_kernel, dim3(1), dim3(256), 0, s, la);
    }
    return hipGetLastError();
}

Img make_img(uint32_t n_arc, const uint8_t* d_store, uint64_t store_bytes, const uint64_t* d_arc_base,
             const uint64_t* d_arc_bytes, const uint8_t* d_maps, uint64_t map_stride_bytes, const uint64_t* d_len,
             uint32_t hash_len, uint32_t version, uint32_t header_bytes) {
    const uint32_t al4 = ((reinterpret_cast<uintptr_t>(d_maps) | map_stride_bytes) & 3) == 0;
    return Img{d_store, store_bytes, d_arc_base, d_arc_bytes, d_maps, map_stride_bytes, d_len,
               n_arc,   hash_len,    version,    header_bytes, al4};
}

}  // namespace
}  // namespace sdfs

using namespace sdfs;

extern "C" {

int sdfs_cdc_store_scan(int device, uint32_t n_arc, const uint8_t* d_store, uint64_t store_bytes,
                        const uint64_t* d_arc_base, const uint64_t* d_arc_bytes, const uint8_t* d_maps,
                        uint64_t map_stride_bytes, const uint64_t* map_len, uint32_t hash_len, uint32_t version,
                        uint32_t header_bytes, uint32_t max_chunk, int plain, const sdfs_cdc_store_records* recs,
                        const sdfs_cdc_store_archives* arcs, void* stream) {
    if (const int rc = check_images(n_arc, d_store, d_arc_base, d_arc_bytes, d_maps, map_stride_bytes, map_len, hash_len,
                                    header_bytes))
        return rc;
    if (!recs || !recs->count || !recs->status)
        return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_store_records");
    if (recs->n_cap && (!recs->arc || !recs->slot || !recs->pos || !recs->len || !recs->store_off || !recs->key ||
                        !recs->raw_len || !recs->flags))
        return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_store_records");
    if (!arcs || !arcs->arc_first) return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_store_archives");
    if (n_arc && (!arcs->map_slots || !arcs->version || !arcs->status || (header_bytes && !arcs->ivs) ||
                  (arcs->slot_stride && !arcs->slot_rec)))
        return fail_status(SDFS_CDC_EINVAL, "incomplete sdfs_cdc_store_archives");
    if (max_chunk > (uint32_t)INT32_MAX) return fail_status(SDFS_CDC_EINVAL, "max_chunk %u above 2^31 - 1", max_chunk);
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    Scratch sc(s);
    ScanArgs2 a{};
    uint64_t* d_len = nullptr;
    SDFS_TRY(sc.get(&d_len, n_arc));
    SDFS_TRY(sc.get(&a.cnt, n_arc));
    a.im = make_img(n_arc, d_store, store_bytes, d_arc_base, d_arc_bytes, d_maps, map_stride_bytes, d_len, hash_len,
                    version, header_bytes);
    a.r = *recs;
    a.o = *arcs;
    a.max_chunk = max_chunk;
    a.plain = plain != 0;
    const bool lds = arcs->slot_stride <= kSortLds;
    if (!lds && n_arc) {
        a.sort_stride = 1;
        while (a.sort_stride < arcs->slot_stride) a.sort_stride <<= 1;
        SDFS_TRY(sc.get(&a.sort, (size_t)a.sort_stride * n_arc));
    }
    SDFS_TRY(upload_lens(map_len, n_arc, d_len, s));
    if (n_arc) hipLaunchKernelGGL(store_count_kernel, dim3(n_arc), dim3(256), 0, s, a);
    hipLaunchKernelGGL(store_prefix_kernel, dim3(1), dim3(1024), 0, s, a);
    if (n_arc) {
        if (lds) hipLaunchKernelGGL(store_emit_kernel<true>, dim3(n_arc), dim3(kEmitThreads), 0, s, a);
        else hipLaunchKernelGGL(store_emit_kernel<false>, dim3(n_arc), dim3(kEmitThreads), 0, s, a);
    }
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_store_raw_lens(int device, const uint8_t* d_plain, const uint64_t* d_off, const uint32_t* d_len,
                            const uint32_t* d_count, uint64_t n_max, uint32_t max_chunk, uint32_t* d_raw_len,
                            uint32_t* d_flags, void* stream) {
    if (n_max && (!d_plain || !d_off || !d_len || !d_raw_len || !d_flags))
        return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_max >= (uint64_t)UINT32_MAX)
        return fail_status(SDFS_CDC_EINVAL, "n_max %llu: record ordinals are 32-bit", (unsigned long long)n_max);
    if (max_chunk > (uint32_t)INT32_MAX) return fail_status(SDFS_CDC_EINVAL, "max_chunk %u above 2^31 - 1", max_chunk);
    if (n_max == 0) return SDFS_CDC_OK;
    if (const int rc = set_device(device)) return rc;
    hipLaunchKernelGGL(store_raw_lens_kernel, dim3((uint32_t)((n_max + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), d_plain, d_off, d_len, d_count, n_max, max_chunk, d_raw_len,
                       d_flags);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_store_directory(int device, const uint64_t* d_rec_store_off, const uint32_t* d_rec_len,
                             const uint32_t* d_rec_raw_len, const uint32_t* d_rec_flags, const int64_t* d_hashloc,
                             const uint32_t* d_count, uint64_t n_max, uint64_t pos_base, uint64_t n_store,
                             uint64_t* d_store_off, uint32_t* d_store_len, uint32_t* d_store_raw_len,
                             uint32_t* d_rec_of_k, uint64_t* d_info, void* stream) {
    if (!d_info) return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_max && (!d_rec_store_off || !d_rec_len || !d_rec_raw_len || !d_rec_flags || !d_hashloc))
        return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_store && (!d_store_off || !d_store_len || !d_store_raw_len || !d_rec_of_k))
        return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (!n_store && (d_store_off || d_store_len || d_store_raw_len || d_rec_of_k))
        return fail_status(SDFS_CDC_EINVAL, "n_store 0: there is no directory to write, the outputs must be NULL");
    if (n_max >= (uint64_t)UINT32_MAX || n_store >= (uint64_t)UINT32_MAX)
        return fail_status(SDFS_CDC_EINVAL, "n_max %llu, n_store %llu: record ordinals and fetch indices are 32-bit",
                           (unsigned long long)n_max, (unsigned long long)n_store);
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    Scratch sc(s);
    DirArgs a{d_rec_store_off, d_rec_len,   d_rec_raw_len, d_rec_flags,     d_hashloc,  d_count, n_max,  pos_base,
              n_store,         d_store_off, d_store_len,   d_store_raw_len, d_rec_of_k, d_info,  nullptr};
    SDFS_TRY(sc.get(&a.owner, (size_t)n_store));
    SDFS_TRY(hipMemsetAsync(a.owner, 0xFF, std::max<size_t>(n_store, 1) * 4, s));
    SDFS_TRY(hipMemsetAsync(d_info, 0, 24, s));
    if (n_max) hipLaunchKernelGGL(store_dir_claim_kernel, dim3((uint32_t)((n_max + 255) / 256)), dim3(256), 0, s, a);
    const uint64_t m = std::max(n_max, n_store);
    if (m) hipLaunchKernelGGL(store_dir_write_kernel, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, s, a);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_store_lookup(int device, uint32_t n_arc, const uint8_t* d_store, uint64_t store_bytes,
                          const uint64_t* d_arc_base, const uint64_t* d_arc_bytes, const uint8_t* d_maps,
                          uint64_t map_stride_bytes, const uint64_t* map_len, uint32_t hash_len, uint32_t version,
                          uint32_t header_bytes, const uint32_t* d_q_arc, const uint8_t* d_q_key, uint64_t n_q,
                          uint32_t* d_slot, uint32_t* d_pos, uint32_t* d_len, uint64_t* d_store_off,
                          uint32_t* d_flags, void* stream) {
    if (const int rc = check_images(n_arc, d_store, d_arc_base, d_arc_bytes, d_maps, map_stride_bytes, map_len, hash_len,
                                    header_bytes))
        return rc;
    if (n_q && (!d_q_arc || !d_q_key || !d_slot || !d_pos || !d_len || !d_store_off || !d_flags))
        return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_q >= (1ull << 39)) return fail_status(SDFS_CDC_EINVAL, "n_q %llu too large", (unsigned long long)n_q);
    if (n_q == 0) return SDFS_CDC_OK;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    Scratch sc(s);
    uint64_t* d_len_map = nullptr;
    SDFS_TRY(sc.get(&d_len_map, n_arc));
    SDFS_TRY(upload_lens(map_len, n_arc, d_len_map, s));
    LookArgs a{make_img(n_arc, d_store, store_bytes, d_arc_base, d_arc_bytes, d_maps, map_stride_bytes, d_len_map,
                        hash_len, version, header_bytes),
               d_q_arc, d_q_key, n_q, d_slot, d_pos, d_len, d_store_off, d_flags};
    hipLaunchKernelGGL(store_lookup_kernel, dim3((uint32_t)((n_q + 255) / 256)), dim3(256), 0, s, a);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

int sdfs_cdc_store_verify(sdfs_cdc_engine* engine, const uint8_t* d_chunks, const uint64_t* d_off,
                          const uint32_t* d_len, const uint8_t* d_keys, const uint32_t* d_count, uint64_t n_max,
                          uint32_t hash_len, uint32_t* d_flags, void* stream) {
    if (!engine) return fail_status(SDFS_CDC_EINVAL, "null engine");
    if (const int rc = check_hash_len(hash_len, HashOf::kMapKey)) return rc;
    if (n_max && (!d_chunks || !d_off || !d_len || !d_keys || !d_flags))
        return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n_max >= (uint64_t)UINT32_MAX)
        return fail_status(SDFS_CDC_EINVAL, "n_max %llu: record ordinals are 32-bit", (unsigned long long)n_max);
    const int dl = sdfs_cdc_digest_len(engine);
    if (dl < 0) return fail_status(SDFS_CDC_EINVAL, "not a live engine handle");
    if ((uint32_t)dl != hash_len)
        return fail_status(SDFS_CDC_EINVAL, "engine digests are %d bytes, the keys hold %u", dl, hash_len);
    if (n_max == 0) return SDFS_CDC_OK;
    hipPointerAttribute_t at;
    SDFS_TRY(hipPointerGetAttributes(&at, d_flags));
    if (const int rc = set_device(at.device)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    Scratch sc(s);
    uint32_t* lens = nullptr;
    uint8_t* digests = nullptr;
    SDFS_TRY(sc.get(&lens, (size_t)n_max));
    SDFS_TRY(sc.get(&digests, (size_t)n_max * 32));
    const dim3 grid((uint32_t)((n_max + 255) / 256));
    hipLaunchKernelGGL(store_verify_lens_kernel, grid, dim3(256), 0, s, d_len, d_flags, d_count, n_max, lens);
    SDFS_TRY(hipGetLastError());
    if (const int rc = sdfs_cdc_hash_device(engine, d_chunks, d_off, lens, d_count, n_max, digests, stream)) return rc;
    hipLaunchKernelGGL(store_verify_compare_kernel, grid, dim3(256), 0, s, d_len, d_keys, digests, d_count, n_max,
                       hash_len, d_flags);
    SDFS_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

}  // extern "C"
