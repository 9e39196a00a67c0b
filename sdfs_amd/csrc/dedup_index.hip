// dedup_index.hip — device-resident dedup-hit index (include/sdfs_index.h).
//
// The reference's write path, after getChunks, groups a buffer's chunks by fingerprint and counts
// `claims` (SparseDedupFile.java:435-446), then puts every distinct fingerprint into the hash
// store with that claim count (Finger.java:50-60 -> HashChunkService.writeChunk,
// HashChunkService.java:98-118 -> RocksDBMap.put, RocksDBMap.java:785-870: present -> refcount +=
// claims, not inserted; absent -> persist + insert {pos, claims}), and marks each chunk dup /
// not dup with its hashloc (SparseDedupFile.java:541-560).
//
// MI355X form: the map lives in HBM as an open-addressing table of 64-byte slots (one cache line:
// digest[32] | pos | refcount | state), and a whole batch of fingerprint records is applied with
// five small integer kernels and no sort:
//   1. group   — a batch-local table of RECORD INDICES (the keys stay in the immutable record
//                table, so a CAS on a 4-byte slot publishes a fully formed key): equal
//                fingerprints meet in one local slot, which keeps the smallest record index
//                (atomicMin) and counts the group (the claims);
//   2. probe   — one lane per group representative probes the global table: hit -> refcount +=
//                claims; miss -> claim an empty slot with a CAS on its state word, stamped with
//                this batch's epoch (lanes of the same batch skip each other's fresh slots without
//                reading their keys: representatives are distinct fingerprints); the assign step
//                turns every stamp of the batch into the committed state, so no stamp outlives
//                its batch (epochs may wrap);
//   3-4. rank  — block counts + one-block scan of the "inserted" flags in record order;
//   5. assign  — inserted record -> new_list[rank], slot pos = pos_base + rank;
//   6. output  — per record: dup = not inserted, hashloc = its fingerprint's pos.
// The outcome is what applying the batch's buffers one after another gives (the first record of
// a new fingerprint is the inserted one), independent of the GPU's schedule.
//
// The other direction (removeRef / addRef -> claimKey, RocksDBMap.java:388-509; the claimRecords
// collection pass, RocksDBMap.java:630-714): a claim adds a signed delta to a fingerprint's count;
// an entry whose count is <= 0 stays in the table, findable, until a sweep turns it into a
// tombstone (count / scan / emit over the slots, so the caller's cap is exact and the outcome
// depends on the table alone).  Probes step over tombstones and never compare their stale keys.
// Tombstones count against the fill; a rebuild copies the committed slots into a transient second
// table (one CAS on `state` per entry, no key compares: all keys are distinct) and back.  Every
// phase that reads what another workgroup wrote is its own kernel on the same stream.
//
// Whole-map-file walks (LongByteArrayMap.vanish / index / trim / truncate, LongByteArrayMap.java:
// 817-882, 897-940, 595-648, 656-688) claim straight from slot images: validate (one wave per
// slot), then apply (a wave per kSlotPart pairs).  recount is the same walk pointed at a shadow
// count in each slot's spare bytes, followed by a count / scan / emit over the table; load and
// export are the way in and out with the caller's positions.  addref_slots (writeSparseDataChunk,
// StorageServiceImpl.java:275-382) is the walk once more, all or nothing per slot: validate, a
// check pass that probes and counts each slot's misses, an apply pass that runs only where there
// were none.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <mutex>

#include "../../include/sdfs_index.h"
#include "../../include/sdfs_ingest.h"
#include "block_scan.h"
#include "call_support.h"
#include "cdc_internal.h"
#include "store_format.h"
#include "stream_order.h"

namespace sdfs {
namespace {

struct alignas(64) IndexSlot {
    uint4 key[2];     // digest, zero-padded to 32 bytes
    uint64_t pos;     // where the chunk lives (caller's namespace)
    uint64_t ref;     // reference count (signed: claims may take it to 0 or below)
    uint32_t state;   // 0 = empty, kCommitted = holds a fingerprint, kTombstone = swept (the key is
                      // stale; probes step over it), (epoch << 1) | 1 (epoch >= 1) = being inserted
                      // by the batch of that epoch
    uint32_t pad;
    uint64_t shadow;  // recount's count of the pairs that name this fingerprint (zeroed by each recount)
};
static_assert(sizeof(IndexSlot) == 64, "one cache line per slot");
static_assert(offsetof(IndexSlot, shadow) == 56, "the shadow count rides in the slot's spare bytes");

constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr uint32_t kCommitted = 1u;  // never a batch stamp: those are >= 3
constexpr uint32_t kTombstone = 2u;  // even: never a batch stamp either
constexpr int kIxThreads = 256;
constexpr int kRankBlock = 1024;

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ void load_digest(const uint8_t* records, uint32_t r, uint4& a, uint4& b) {
    const uint4* p = reinterpret_cast<const uint4*>(records + (uint64_t)r * kRecordBytes);
    a = p[0];
    b = p[1];
}

__device__ __forceinline__ bool eq4(const uint4& x, const uint4& y) {
    return ((x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w)) == 0;
}

// 1. group equal fingerprints of the batch; ltab holds the smallest record index of each group
__global__ __launch_bounds__(kIxThreads) void ix_group_kernel(const uint8_t* records, const uint32_t* d_count,
                                                              uint64_t n_max, uint32_t* ltab, uint32_t* lcount,
                                                              uint32_t lmask, uint32_t* lslot) {
    const uint32_t n = (uint32_t)live_count(d_count, n_max);
    const uint32_t r = blockIdx.x * kIxThreads + threadIdx.x;
    if (r >= n) return;
    uint4 a, b;
    load_digest(records, r, a, b);
    uint32_t h = (uint32_t)mix64(((uint64_t)a.w << 32 | a.z) ^ 0x5DF50001ull) & lmask;
    for (;;) {  // lmask + 1 >= 2n: an empty slot always exists
        uint32_t v = ltab[h];
        if (v == kEmpty) {
            const uint32_t old = atomicCAS(&ltab[h], kEmpty, r);
            if (old == kEmpty) break;
            v = old;
        }
        uint4 c, d;
        load_digest(records, v, c, d);
        if (eq4(a, c) && eq4(b, d)) {
            atomicMin(&ltab[h], r);
            break;
        }
        h = (h + 1) & lmask;
    }
    atomicAdd(&lcount[h], 1u);
    lslot[r] = h;
}

// 2. representatives probe / insert into the global table
__global__ __launch_bounds__(kIxThreads) void ix_probe_kernel(const uint8_t* records, const uint32_t* d_count,
                                                              uint64_t n_max, const uint32_t* ltab,
                                                              const uint32_t* lcount, const uint32_t* lslot,
                                                              IndexSlot* table, uint64_t cmask, uint32_t stamp,
                                                              uint32_t* gidx, uint32_t* isnew, uint32_t* overflow) {
    const uint32_t n = (uint32_t)live_count(d_count, n_max);
    const uint32_t r = blockIdx.x * kIxThreads + threadIdx.x;
    if (r >= n) return;
    const uint32_t ls = lslot[r];
    if (ltab[ls] != r) {  // not the first record of its fingerprint in this batch
        isnew[r] = 0;
        return;
    }
    const uint32_t claims = lcount[ls];
    uint4 a, b;
    load_digest(records, r, a, b);
    uint64_t h = mix64((uint64_t)a.y << 32 | a.x) & cmask;
    for (uint64_t step = 0; step <= cmask; step++, h = (h + 1) & cmask) {
        IndexSlot& s = table[h];
        uint32_t st = s.state;
        if (st == 0) {
            const uint32_t old = atomicCAS(&s.state, 0u, stamp);
            if (old == 0) {
                s.key[0] = a;
                s.key[1] = b;
                s.ref = claims;
                s.pos = ~0ull;  // assigned in rank order by ix_assign_kernel
                gidx[ls] = (uint32_t)h;
                isnew[r] = 1;
                return;
            }
            st = old;
        }
        if (st == stamp) continue;  // inserted by this batch: a different fingerprint
        if (st == kTombstone) continue;  // swept: the chain goes on, the key is stale
        if (eq4(s.key[0], a) && eq4(s.key[1], b)) {
            add64(&s.ref, claims);
            gidx[ls] = (uint32_t)h;
            isnew[r] = 0;
            return;
        }
    }
    atomicOr(overflow, 1u);
    gidx[ls] = 0xFFFFFFFFu;
    isnew[r] = 0;
}

// 3. inserted records per block of kRankBlock records
__global__ __launch_bounds__(kRankBlock) void ix_count_kernel(const uint32_t* d_count, uint64_t n_max,
                                                              const uint32_t* isnew, uint32_t* bsum) {
    __shared__ uint32_t lds[16];
    const uint32_t n = (uint32_t)live_count(d_count, n_max);
    const uint32_t r = blockIdx.x * kRankBlock + threadIdx.x;
    uint32_t total;
    (void)block_exclusive_scan_1024(r < n ? isnew[r] : 0u, lds, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// 4. exclusive scan of the block counts (one block), batch total, running index size
__global__ __launch_bounds__(kRankBlock) void ix_scan_kernel(uint32_t* bsum, uint32_t nblocks, uint64_t* new_count,
                                                             uint64_t* used) {
    __shared__ uint32_t lds[16];
    const uint64_t carry = block_sums_to_bases(bsum, nblocks, lds);
    if (threadIdx.x == 0) {
        *new_count = carry;
        *used += carry;
    }
}

// 5. inserted records: rank -> new_list, slot pos
__global__ __launch_bounds__(kRankBlock) void ix_assign_kernel(const uint32_t* d_count, uint64_t n_max,
                                                               const uint32_t* isnew, const uint32_t* bbase,
                                                               const uint32_t* lslot, const uint32_t* gidx,
                                                               IndexSlot* table, uint64_t pos_base,
                                                               uint32_t* new_list) {
    __shared__ uint32_t lds[16];
    const uint32_t n = (uint32_t)live_count(d_count, n_max);
    const uint32_t r = blockIdx.x * kRankBlock + threadIdx.x;
    const uint32_t f = r < n ? isnew[r] : 0u;
    uint32_t total;
    const uint32_t ex = block_exclusive_scan_1024(f, lds, total);
    if (f) {
        const uint32_t rank = bbase[blockIdx.x] + ex;
        if (new_list) new_list[rank] = r;
        IndexSlot& slot = table[gidx[lslot[r]]];
        slot.pos = pos_base + rank;
        slot.state = kCommitted;  // the batch stamp must not survive the batch
    }
}

// 6. per-record dup flag and hashloc
__global__ __launch_bounds__(kIxThreads) void ix_output_kernel(const uint32_t* d_count, uint64_t n_max,
                                                               const uint32_t* isnew, const uint32_t* lslot,
                                                               const uint32_t* gidx, const IndexSlot* table,
                                                               uint8_t* dup, uint64_t* hashloc) {
    const uint32_t n = (uint32_t)live_count(d_count, n_max);
    const uint32_t r = blockIdx.x * kIxThreads + threadIdx.x;
    if (r >= n) return;
    if (dup) dup[r] = isnew[r] ? 0 : 1;
    if (hashloc) {
        const uint32_t g = gidx[lslot[r]];
        hashloc[r] = g == 0xFFFFFFFFu ? ~0ull : table[g].pos;
    }
}

__global__ __launch_bounds__(kIxThreads) void ix_get_kernel(const uint8_t* digests, uint64_t n,
                                                            const IndexSlot* table, uint64_t cmask, uint64_t* pos,
                                                            uint64_t* ref) {
    const uint64_t i = (uint64_t)blockIdx.x * kIxThreads + threadIdx.x;
    if (i >= n) return;
    const uint4* p = reinterpret_cast<const uint4*>(digests + i * 32);
    const uint4 a = p[0], b = p[1];
    uint64_t h = mix64((uint64_t)a.y << 32 | a.x) & cmask;
    uint64_t rp = ~0ull, rr = 0;
    for (uint64_t step = 0; step <= cmask; step++, h = (h + 1) & cmask) {
        const IndexSlot& s = table[h];
        const uint32_t st = s.state;
        if (st == 0) break;
        if (st == kTombstone) continue;
        if (eq4(s.key[0], a) && eq4(s.key[1], b)) {
            rp = s.pos;
            rr = s.ref;
            break;
        }
    }
    if (pos) pos[i] = rp;
    if (ref) ref[i] = rr;
}

// claim: ref += delta for a fingerprint that is present (and at expect_pos, when one is given)
__global__ __launch_bounds__(kIxThreads) void ix_claim_kernel(const uint8_t* digests, const uint64_t* expect_pos,
                                                              const int64_t* delta, uint64_t n, IndexSlot* table,
                                                              uint64_t cmask, uint64_t* out_pos) {
    const uint64_t i = (uint64_t)blockIdx.x * kIxThreads + threadIdx.x;
    if (i >= n) return;
    const uint4* p = reinterpret_cast<const uint4*>(digests + i * 32);
    const uint4 a = p[0], b = p[1];
    const uint64_t want = expect_pos ? expect_pos[i] : ~0ull;
    uint64_t h = mix64((uint64_t)a.y << 32 | a.x) & cmask;
    uint64_t rp = ~0ull;
    for (uint64_t step = 0; step <= cmask; step++, h = (h + 1) & cmask) {
        IndexSlot& s = table[h];
        const uint32_t st = s.state;
        if (st == 0) break;
        if (st == kTombstone) continue;
        if (eq4(s.key[0], a) && eq4(s.key[1], b)) {
            const uint64_t pos = s.pos;
            if (want == ~0ull || want == pos) {
                add64(&s.ref, delta[i]);
                rp = pos;
            }
            break;
        }
    }
    if (out_pos) out_pos[i] = rp;
}

__device__ __forceinline__ uint32_t slot_is_dead(const IndexSlot* table, uint64_t slots, uint64_t i) {
    return i < slots && table[i].state == kCommitted && (int64_t)table[i].ref <= 0 ? 1u : 0u;
}

// sweep 1. dead entries (committed, count <= 0) per block of kRankBlock consecutive slots; one
// lane per slot, so a wave reads 64 contiguous slots; it leaves their dead flags as one 64-bit
// word, and the emit pass does not have to stream the table a second time
__global__ __launch_bounds__(kRankBlock) void ix_sweep_count_kernel(const IndexSlot* table, uint64_t slots,
                                                                    uint32_t* bsum, unsigned long long* dead) {
    __shared__ uint32_t lds[16];
    const uint64_t i = (uint64_t)blockIdx.x * kRankBlock + threadIdx.x;
    const uint32_t f = slot_is_dead(table, slots, i);
    const unsigned long long m = __ballot(f);
    if ((threadIdx.x & 63) == 0) dead[i >> 6] = m;
    uint32_t total;
    (void)block_exclusive_scan_1024(f, lds, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// sweep 2. exclusive scan of the block counts (one block); removed / left-behind counts; the
// device's live and tombstone counts follow
__global__ __launch_bounds__(kRankBlock) void ix_sweep_scan_kernel(uint32_t* bsum, uint32_t nblocks, uint64_t cap,
                                                                   uint64_t* counts, uint64_t* used) {
    __shared__ uint32_t lds[16];
    const uint64_t carry = block_sums_to_bases(bsum, nblocks, lds);  // dead entries <= slots <= 2^31
    if (threadIdx.x == 0) {
        const uint64_t removed = carry < cap ? carry : cap;
        counts[0] = removed;
        counts[1] = carry - removed;
        used[0] -= removed;
        used[1] += removed;
    }
}

// sweep 3. the first `cap` dead entries in slot order: {digest, pos} -> removed list, slot -> tombstone
__global__ __launch_bounds__(kRankBlock) void ix_sweep_emit_kernel(IndexSlot* table, uint64_t slots,
                                                                   const uint32_t* bbase,
                                                                   const unsigned long long* dead, uint64_t cap,
                                                                   uint8_t* removed_digests, uint64_t* removed_pos) {
    __shared__ uint32_t lds[16];
    const uint64_t i = (uint64_t)blockIdx.x * kRankBlock + threadIdx.x;
    const uint32_t f = (uint32_t)(dead[i >> 6] >> (threadIdx.x & 63)) & 1u;  // set only for i < slots
    uint32_t total;
    const uint32_t ex = block_exclusive_scan_1024(f, lds, total);
    if (!f) return;
    const uint64_t rank = (uint64_t)bbase[blockIdx.x] + ex;
    if (rank >= cap) return;
    IndexSlot& s = table[i];
    uint4* d = reinterpret_cast<uint4*>(removed_digests + rank * 32);
    d[0] = s.key[0];
    d[1] = s.key[1];
    removed_pos[rank] = s.pos;
    s.state = kTombstone;
}

// rebuild: every committed slot of `from` claims an empty slot of `to` (zeroed) with a CAS on its
// state and writes its fields; keys are distinct, so lanes only step over occupied slots
__global__ __launch_bounds__(kIxThreads) void ix_rebuild_kernel(const IndexSlot* from, IndexSlot* to,
                                                                uint64_t slots) {
    const uint64_t i = (uint64_t)blockIdx.x * kIxThreads + threadIdx.x;
    if (i >= slots) return;
    const IndexSlot& s = from[i];
    if (s.state != kCommitted) return;
    const uint4 a = s.key[0], b = s.key[1];
    const uint64_t cmask = slots - 1;
    uint64_t h = mix64((uint64_t)a.y << 32 | a.x) & cmask;
    for (uint64_t step = 0; step <= cmask; step++, h = (h + 1) & cmask) {
        IndexSlot& t = to[h];
        if (t.state != 0) continue;
        if (atomicCAS(&t.state, 0u, kCommitted) != 0) continue;
        t.key[0] = a;
        t.key[1] = b;
        t.pos = s.pos;
        t.ref = s.ref;
        return;
    }
}

// ---------------------------------------------------------------------------- map-file walks
//
// claim_slots and recount read HashLocPairs straight from slot images, accepted by
// slot_walk_check (store_format.h).  Validation is a kernel of its own (one wave per slot): it
// settles every slot's status and pair count before any count moves.  The apply pass gives a wave
// kSlotPart pairs of one slot, so a slot of thousands of pairs spreads over many waves; a lane
// takes its pair's key and hashloc (load_pair_key) and probes; a run of neighbouring lanes that
// found the same entry adds once, with one 64-bit device-scope atomic.  Integer adds commute: the
// outcome does not depend on the schedule.

constexpr int kWalkThreads = 256;  // four waves, each on its own slot (part)

struct WalkArgs {
    const uint8_t* map;
    uint64_t nslots;
    uint32_t slot_bytes;
    uint32_t hash_len;
    const uint8_t* sel;
    uint32_t* status;    // [nslots]
    uint32_t* missed;    // [nslots] or NULL
    uint32_t* meta;      // [nslots] scratch: slot_meta
    uint64_t* counts;    // [0] applied, [1] missed, [2] corrupt slots
    uint64_t* nonempty;  // selected slots with at least one pair, or NULL
    uint32_t parts;      // waves per slot in the apply pass
    // addref_slots alone
    const uint8_t* inserted;  // [nslots x pair_stride] or NULL: pairs that are skipped entirely
    uint32_t pair_stride;
    uint32_t* miss_list;      // [miss_cap x 2] {request, pair}
    uint64_t miss_cap;
    uint64_t* acounts;        // [0] added, [1] missed, [2] skipped, [3] accepted, [4] rejected, [5] misses listed
};

__global__ __launch_bounds__(kWalkThreads) void ix_walk_validate_kernel(WalkArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t s = (uint64_t)blockIdx.x * (kWalkThreads / 64) + (threadIdx.x >> 6);
    if (s >= a.nslots) return;  // wave-uniform, as is every branch below
    SlotWalk w{0, 0, false};
    if (!a.sel || a.sel[s]) w = slot_walk_check(a.map + s * a.slot_bytes, a.slot_bytes, a.hash_len, lane);
    if (lane == 0) {
        a.status[s] = w.status;
        if (a.missed) a.missed[s] = 0;
        a.meta[s] = slot_meta(w);
        if (w.status) add64(&a.counts[2], 1);
        if (w.n && a.nonempty) add64(a.nonempty, 1);
    }
}

// what the apply pass does with a pair whose digest is held at its hashloc
enum : int {
    kWalkClaim,        // claim_slots: delta on the entry's count
    kWalkShadow,       // recount: +1 on the entry's shadow count
    kWalkAddrefCheck,  // addref_slots, first pass: nothing moves; the slot's misses are counted and listed
    kWalkAddrefApply,  // addref_slots, second pass: +1 on the entry's count, in the slots that had no miss
};

// HW: words of a pair's hash (8 = SHA-256, 4 = MD5).
template <int HW, int MODE>
__global__ __launch_bounds__(kWalkThreads) void ix_walk_apply_kernel(WalkArgs a, IndexSlot* table, uint64_t cmask,
                                                                     int64_t delta) {
    constexpr bool SHADOW = MODE == kWalkShadow;
    constexpr bool ADDREF = MODE == kWalkAddrefCheck || MODE == kWalkAddrefApply;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t unit = (uint64_t)blockIdx.x * (kWalkThreads / 64) + (threadIdx.x >> 6);
    const uint64_t s = unit / a.parts;
    if (s >= a.nslots) return;  // wave-uniform
    const uint32_t meta = a.meta[s];
    const uint32_t n = slot_meta_pairs(meta);
    const uint32_t i0 = (uint32_t)(unit % a.parts) * kSlotPart;
    if (i0 >= n) return;
    // the check pass has finished: a slot with a miss moves no count, in any of its waves
    if (MODE == kWalkAddrefApply && a.missed[s] != 0) return;
    const uint32_t i1 = min(n, i0 + kSlotPart);
    constexpr uint32_t hl = HW * 4;
    const uint8_t* img = a.map + s * a.slot_bytes;
    uint32_t applied = 0, missed = 0, skipped = 0;
    for (uint32_t ib = i0; ib < i1; ib += 64) {  // the same trip count for every lane of the wave
        const uint32_t i = ib + lane;
        bool on = i < i1;
        if (on && slot_meta_unsorted(meta)) on = !pair_superseded(img, i, n, hl);
        if (ADDREF && on && a.inserted && a.inserted[s * a.pair_stride + i]) {  // neither probed nor counted
            on = false;
            skipped++;
        }
        bool hit = false;
        uint32_t at = 0;  // the entry's table slot (slots <= 2^31)
        if (on) {
            uint4 ka, kb;
            uint64_t hashloc;
            load_pair_key<HW>(img, i, ka, kb, hashloc);
            uint64_t h = mix64((uint64_t)ka.y << 32 | ka.x) & cmask;
            for (uint64_t step = 0; step <= cmask; step++, h = (h + 1) & cmask) {
                const IndexSlot& e = table[h];
                const uint32_t st = e.state;
                if (st == 0) break;
                if (st == kTombstone) continue;
                if (eq4(e.key[0], ka) && eq4(e.key[1], kb)) {
                    hit = e.pos == hashloc;  // claimKey: the right archive
                    at = (uint32_t)h;
                    break;
                }
            }
        }
        // A run of neighbouring pairs that name one entry — a stretch of all-zero chunks — adds
        // once, from its first lane, not lane by lane on one address.  Pairs are in pos order, so a
        // repeated chunk sits in neighbouring lanes; equal entries further apart add separately.
        const uint32_t prev_at = __shfl_up(at, 1);
        const unsigned long long hits = __ballot(hit);
        const bool head = hit && (lane == 0 || !((hits >> (lane - 1)) & 1) || prev_at != at);
        const unsigned long long stops = __ballot(head) | ~hits;  // lanes at which a run ends
        if (MODE == kWalkAddrefCheck) {
            if (on && !hit) {
                const uint64_t k = add64(&a.acounts[5], 1);
                if (k < a.miss_cap) {
                    a.miss_list[2 * k] = (uint32_t)s;
                    a.miss_list[2 * k + 1] = i;
                }
            }
        } else if (head) {
            const unsigned long long above = lane == 63 ? 0ull : stops >> (lane + 1);
            const unsigned long long k = above ? (unsigned long long)__ffsll((long long)above) : 64ull - lane;
            IndexSlot& e = table[at];
            add64(SHADOW ? &e.shadow : &e.ref, SHADOW ? k : (uint64_t)delta * k);
        }
        applied += hit;
        missed += on && !hit;
    }
    applied = wave_sum(applied);
    missed = wave_sum(missed);
    if (ADDREF) {
        skipped = wave_sum(skipped);
        if (lane != 0) return;
        if (MODE == kWalkAddrefCheck) {
            if (missed) {
                add64(&a.acounts[1], missed);
                atomicAdd(&a.missed[s], missed);
            }
            if (skipped) add64(&a.acounts[2], skipped);
        } else if (applied) {
            add64(&a.acounts[0], applied);
        }
        return;
    }
    if (lane == 0) {
        if (applied) add64(&a.counts[0], applied);
        if (missed) {
            add64(&a.counts[1], missed);
            if (a.missed) atomicAdd(&a.missed[s], missed);
        }
    }
}

// trim: every selected slot that parsed becomes LongByteArrayMap.FREE (zeros); one workgroup per slot
__global__ __launch_bounds__(kWalkThreads) void ix_walk_free_kernel(uint8_t* map, uint32_t slot_bytes,
                                                                    const uint8_t* sel, const uint32_t* status) {
    const uint64_t s = blockIdx.x;
    if ((sel && !sel[s]) || status[s]) return;
    uint8_t* p = map + s * slot_bytes;
    const uint32_t head = min(slot_bytes, (uint32_t)((0 - reinterpret_cast<uintptr_t>(p)) & 15));
    const uint32_t nvec = (slot_bytes - head) / 16;
    for (uint32_t i = threadIdx.x; i < head; i += kWalkThreads) p[i] = 0;
    uint4* v = reinterpret_cast<uint4*>(p + head);
    for (uint32_t i = threadIdx.x; i < nvec; i += kWalkThreads) v[i] = make_uint4(0, 0, 0, 0);
    for (uint32_t i = head + nvec * 16 + threadIdx.x; i < slot_bytes; i += kWalkThreads) p[i] = 0;
}

// addref_slots, last: a request's status from its parse and its misses; the batch's totals
__global__ __launch_bounds__(kIxThreads) void ix_addref_finish_kernel(WalkArgs a) {
    const uint64_t s = (uint64_t)blockIdx.x * kIxThreads + threadIdx.x;
    uint32_t ok = 0, bad = 0;
    if (s < a.nslots) {
        uint32_t st = a.status[s];
        if (!st && a.missed[s]) st = SDFS_CDC_INGEST_EMISSED;
        a.status[s] = st;
        ok = st == 0;
        bad = st != 0;
    }
    const uint32_t nok = (uint32_t)__popcll(__ballot(ok)), nbad = (uint32_t)__popcll(__ballot(bad));
    if ((threadIdx.x & 63) == 0) {
        if (nok) add64(&a.acounts[3], nok);
        if (nbad) add64(&a.acounts[4], nbad);
    }
    if (s == 0 && a.acounts[5] > a.miss_cap) a.acounts[5] = a.miss_cap;  // the check pass has finished
}

__global__ __launch_bounds__(kIxThreads) void ix_shadow_zero_kernel(IndexSlot* table, uint64_t slots) {
    const uint64_t i = (uint64_t)blockIdx.x * kIxThreads + threadIdx.x;
    if (i < slots) table[i].shadow = 0;
}

// ------------------------------------------------------------- lists in table-slot order
//
// recount's mismatch list and export use the sweep's count / scan / emit over the slots, so the
// caller's cap is exact and the order is the table's.

enum : int { kFlagHeld, kFlagMismatch };

// flags per block of kRankBlock slots; for kFlagMismatch also recount's four entry counts
// (counts[3..6] = have < want, have > want, want == 0, equal)
template <int KIND>
__global__ __launch_bounds__(kRankBlock) void ix_flag_count_kernel(const IndexSlot* table, uint64_t slots,
                                                                   uint32_t* bsum, unsigned long long* flags,
                                                                   uint64_t* counts) {
    __shared__ uint32_t lds[16];
    __shared__ uint32_t cat[4];
    const uint64_t i = (uint64_t)blockIdx.x * kRankBlock + threadIdx.x;
    if (KIND == kFlagMismatch && threadIdx.x < 4) cat[threadIdx.x] = 0;
    const bool held = i < slots && table[i].state == kCommitted;
    uint32_t f = held;
    if (KIND == kFlagMismatch) {
        __syncthreads();
        const int64_t have = held ? (int64_t)table[i].ref : 0, want = held ? (int64_t)table[i].shadow : 0;
        f = held && have != want;
        const bool c[4] = {held && have < want, held && have > want, held && want == 0, held && have == want};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t m = (uint32_t)__popcll(__ballot(c[k]));
            if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cat[k], m);
        }
    }
    const unsigned long long m = __ballot(f);
    if ((threadIdx.x & 63) == 0) flags[i >> 6] = m;
    uint32_t total;
    (void)block_exclusive_scan_1024(f, lds, total);  // its barriers also order the adds to cat[]
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
    if (KIND == kFlagMismatch && threadIdx.x < 4 && cat[threadIdx.x])
        add64(&counts[3 + threadIdx.x], cat[threadIdx.x]);
}

// exclusive scan of the block counts (one block); *listed = min(total, cap), *total_out = total
__global__ __launch_bounds__(kRankBlock) void ix_flag_scan_kernel(uint32_t* bsum, uint32_t nblocks, uint64_t cap,
                                                                  uint64_t* listed, uint64_t* total_out) {
    __shared__ uint32_t lds[16];
    const uint64_t carry = block_sums_to_bases(bsum, nblocks, lds);  // flagged entries <= slots <= 2^31
    if (threadIdx.x == 0) {
        *listed = carry < cap ? carry : cap;
        if (total_out) *total_out = carry;
    }
}

// recount: the first `cap` mismatching entries in slot order; then (repair) count = shadow for
// every held entry
__global__ __launch_bounds__(kRankBlock) void ix_recount_emit_kernel(IndexSlot* table, uint64_t slots,
                                                                     const uint32_t* bbase,
                                                                     const unsigned long long* flags, uint64_t cap,
                                                                     uint8_t* digests, uint64_t* pos, int64_t* have,
                                                                     int64_t* want, int repair) {
    __shared__ uint32_t lds[16];
    const uint64_t i = (uint64_t)blockIdx.x * kRankBlock + threadIdx.x;
    const uint32_t f = (uint32_t)(flags[i >> 6] >> (threadIdx.x & 63)) & 1u;  // set only for i < slots
    uint32_t total;
    const uint32_t ex = block_exclusive_scan_1024(f, lds, total);
    if (!f) return;  // an entry that is equal needs no repair either
    IndexSlot& s = table[i];
    const uint64_t rank = (uint64_t)bbase[blockIdx.x] + ex;
    if (rank < cap) {
        uint4* d = reinterpret_cast<uint4*>(digests + rank * 32);
        d[0] = s.key[0];
        d[1] = s.key[1];
        pos[rank] = s.pos;
        have[rank] = (int64_t)s.ref;
        want[rank] = (int64_t)s.shadow;
    }
    if (repair) s.ref = s.shadow;
}

__global__ __launch_bounds__(kRankBlock) void ix_export_emit_kernel(const IndexSlot* table, uint64_t slots,
                                                                    const uint32_t* bbase,
                                                                    const unsigned long long* flags, uint64_t cap,
                                                                    uint8_t* digests, uint64_t* pos, int64_t* ref) {
    __shared__ uint32_t lds[16];
    const uint64_t i = (uint64_t)blockIdx.x * kRankBlock + threadIdx.x;
    const uint32_t f = (uint32_t)(flags[i >> 6] >> (threadIdx.x & 63)) & 1u;
    uint32_t total;
    const uint32_t ex = block_exclusive_scan_1024(f, lds, total);
    if (!f) return;
    const uint64_t rank = (uint64_t)bbase[blockIdx.x] + ex;
    if (rank >= cap) return;
    const IndexSlot& s = table[i];
    uint4* d = reinterpret_cast<uint4*>(digests + rank * 32);
    d[0] = s.key[0];
    d[1] = s.key[1];
    pos[rank] = s.pos;
    ref[rank] = (int64_t)s.ref;
}

// ---------------------------------------------------------------------------------------- load
//
// Items {digest, pos, count} with the caller's positions.  As in put_records, equal digests of the
// call first meet in a batch-local table of ITEM INDICES (which also takes the smallest pos of the
// group), then one representative per group probes the global table and, where the digest is
// absent, claims a slot under the batch's stamp with that smallest pos; the last kernel adds every
// item's count where its pos is the entry's, and commits the stamped slots.

__device__ __forceinline__ void load_digest32(const uint8_t* digests, uint32_t i, uint4& a, uint4& b) {
    const uint4* p = reinterpret_cast<const uint4*>(digests + (uint64_t)i * 32);
    a = p[0];
    b = p[1];
}

__global__ __launch_bounds__(kIxThreads) void ix_load_group_kernel(const uint8_t* digests, const uint64_t* pos,
                                                                   uint32_t n, uint32_t* ltab,
                                                                   unsigned long long* lminpos, uint32_t lmask,
                                                                   uint32_t* lslot) {
    const uint32_t r = blockIdx.x * kIxThreads + threadIdx.x;
    if (r >= n) return;
    uint4 a, b;
    load_digest32(digests, r, a, b);
    uint32_t h = (uint32_t)mix64(((uint64_t)a.w << 32 | a.z) ^ 0x5DF50001ull) & lmask;
    for (;;) {  // lmask + 1 >= 2n: an empty slot always exists
        uint32_t v = ltab[h];
        if (v == kEmpty) {
            const uint32_t old = atomicCAS(&ltab[h], kEmpty, r);
            if (old == kEmpty) break;
            v = old;
        }
        uint4 c, d;
        load_digest32(digests, v, c, d);
        if (eq4(a, c) && eq4(b, d)) {
            atomicMin(&ltab[h], r);
            break;
        }
        h = (h + 1) & lmask;
    }
    atomicMin(&lminpos[h], (unsigned long long)pos[r]);
    lslot[r] = h;
}

__global__ __launch_bounds__(kIxThreads) void ix_load_probe_kernel(const uint8_t* digests, uint32_t n,
                                                                   const uint32_t* ltab,
                                                                   const unsigned long long* lminpos,
                                                                   const uint32_t* lslot, IndexSlot* table,
                                                                   uint64_t cmask, uint32_t stamp, uint32_t* gidx,
                                                                   uint64_t* used, uint32_t* overflow) {
    const uint32_t r = blockIdx.x * kIxThreads + threadIdx.x;
    if (r >= n) return;
    const uint32_t ls = lslot[r];
    if (ltab[ls] != r) return;  // not the representative of its digest
    uint4 a, b;
    load_digest32(digests, r, a, b);
    uint64_t h = mix64((uint64_t)a.y << 32 | a.x) & cmask;
    for (uint64_t step = 0; step <= cmask; step++, h = (h + 1) & cmask) {
        IndexSlot& s = table[h];
        uint32_t st = s.state;
        if (st == 0) {
            const uint32_t old = atomicCAS(&s.state, 0u, stamp);
            if (old == 0) {
                s.key[0] = a;
                s.key[1] = b;
                s.ref = 0;
                s.pos = lminpos[ls];
                gidx[ls] = (uint32_t)h;
                add64(used, 1);
                return;
            }
            st = old;
        }
        if (st == stamp) continue;       // inserted by this call: a different digest
        if (st == kTombstone) continue;  // swept: the chain goes on, the key is stale
        if (eq4(s.key[0], a) && eq4(s.key[1], b)) {
            gidx[ls] = (uint32_t)h;
            return;
        }
    }
    atomicOr(overflow, 1u);
    gidx[ls] = 0xFFFFFFFFu;
}

__global__ __launch_bounds__(kIxThreads) void ix_load_apply_kernel(const uint64_t* pos, const int64_t* ref, uint32_t n,
                                                                   const uint32_t* ltab, const uint32_t* lslot,
                                                                   const uint32_t* gidx, IndexSlot* table,
                                                                   uint32_t stamp, uint8_t* status) {
    const uint32_t r = blockIdx.x * kIxThreads + threadIdx.x;
    if (r >= n) return;
    const uint32_t ls = lslot[r];
    const uint32_t g = gidx[ls];
    if (g == 0xFFFFFFFFu) {
        status[r] = 1;
        return;
    }
    IndexSlot& s = table[g];
    const bool ok = s.pos == pos[r];
    if (ok) add64(&s.ref, ref[r]);
    status[r] = ok ? 0 : 1;
    if (ltab[ls] == r && s.state == stamp) s.state = kCommitted;  // the stamp must not survive the call
}

template <typename T>
struct IxBuf {
    T* p = nullptr;
    size_t n = 0;
    hipError_t ensure(size_t want) {
        if (want <= n && p) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(want, 1) * sizeof(T));
        if (e == hipSuccess) n = std::max<size_t>(want, 1);
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

uint64_t next_pow2(uint64_t x) {
    uint64_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

}  // namespace
}  // namespace sdfs

using namespace sdfs;

struct sdfs_cdc_index {
    int device = 0;
    uint64_t slots = 0;     // power of two
    uint64_t max_fill = 0;  // 7/8 of slots
    // host-side bounds: used_ub + tomb_ub is an upper bound of the occupied slots (fingerprints held
    // plus tombstones).  A sweep moves entries from the first count to the second on the device
    // only, which leaves the sum a bound; both are refreshed together from the device counts.
    uint64_t used_ub = 0;
    uint64_t tomb_ub = 0;
    uint32_t epoch = 0;
    IxBuf<IndexSlot> table;
    IxBuf<uint64_t> used;  // device counts: [0] fingerprints held, [1] tombstones
    IxBuf<uint32_t> ltab, lcount, lslot, gidx, isnew, bsum, overflow;
    IxBuf<uint32_t> sweep_bsum;  // dead entries per kRankBlock slots (allocated with the table)
    IxBuf<unsigned long long> sweep_dead;  // the slots' dead flags, one word per 64 slots (likewise)
    IxBuf<unsigned long long> lminpos;     // load: the smallest pos of each group of equal digests
    hipStream_t own = nullptr;   // the index's own non-blocking stream: set-up and readbacks
    hipStream_t last = nullptr;  // the stream of the latest batch (own until one comes)
    StreamOrder order;  // batches apply in call order whatever streams they come on
    std::mutex mu;
};

#define IX_TRY(expr)                                                                                  \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess)                                                                         \
            return fail_status(SDFS_CDC_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                               __FILE__, __LINE__);                                                   \
    } while (0)

// Both device counts (fingerprints held, tombstones) after everything enqueued so far; refreshes
// the host-side bounds.  The caller holds ix->mu.
static int read_counts(sdfs_cdc_index* ix, uint64_t* used, uint64_t* tombs, uint32_t* ovf) {
    IX_TRY(hipStreamSynchronize(ix->last));
    uint64_t c[2] = {0, 0};
    uint32_t o = 0;
    IX_TRY(hipMemcpyAsync(c, ix->used.p, sizeof(c), hipMemcpyDeviceToHost, ix->own));
    IX_TRY(hipMemcpyAsync(&o, ix->overflow.p, sizeof(o), hipMemcpyDeviceToHost, ix->own));
    IX_TRY(hipStreamSynchronize(ix->own));
    ix->used_ub = c[0];
    ix->tomb_ub = c[1];
    *used = c[0];
    *tombs = c[1];
    if (ovf) *ovf = o;
    return SDFS_CDC_OK;
}

// Enqueue a rebuild on s: committed slots -> a transient second table (stream-ordered allocation:
// no null-stream work, no device-wide synchronisation) -> back into the index's table, whose
// address stays what it was.  The caller holds ix->mu and has joined the order chain on s.
// Nothing is enqueued before the allocation has succeeded, so ENOMEM leaves the index intact.
static int rebuild_on(sdfs_cdc_index* ix, hipStream_t s) {
    const size_t bytes = ix->slots * sizeof(IndexSlot);
    IndexSlot* tmp = nullptr;
    if (hipMallocAsync(reinterpret_cast<void**>(&tmp), bytes, s) != hipSuccess || !tmp) {
        (void)hipGetLastError();
        return fail_status(SDFS_CDC_ENOMEM, "index rebuild needs %llu bytes of free device memory",
                           (unsigned long long)bytes);
    }
    hipError_t e = hipMemsetAsync(tmp, 0, bytes, s);
    if (e == hipSuccess) {
        const uint64_t g = (ix->slots + kIxThreads - 1) / kIxThreads;
        hipLaunchKernelGGL(ix_rebuild_kernel, dim3((uint32_t)g), dim3(kIxThreads), 0, s, ix->table.p, tmp,
                           ix->slots);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(ix->table.p, tmp, bytes, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(ix->used.p + 1, 0, sizeof(uint64_t), s);
    const hipError_t ef = hipFreeAsync(tmp, s);
    if (e == hipSuccess) e = ef;
    if (e != hipSuccess) return fail_status(SDFS_CDC_EHIP, "index rebuild failed: %s", hipGetErrorString(e));
    ix->tomb_ub = 0;
    return SDFS_CDC_OK;
}

// The fill rule of a batch that may insert up to n fingerprints (put_records, load), then the
// batch's place in the call order on s: ECAP when the batch does not fit the fingerprints held;
// when it fits those but not those plus the tombstones, a rebuild is enqueued first.  The caller
// holds ix->mu.
static int make_room(sdfs_cdc_index* ix, hipStream_t s, uint64_t n) {
    bool rebuild = false;
    if (ix->used_ub + ix->tomb_ub + n > ix->max_fill) {  // refresh the bounds from the device counts
        IX_TRY(hipStreamSynchronize(s));
        uint64_t used = 0, tombs = 0;
        uint32_t ovf = 0;
        const int rc = read_counts(ix, &used, &tombs, &ovf);
        if (rc != SDFS_CDC_OK) return rc;
        if (ovf) return fail_status(SDFS_CDC_ECAP, "index overflowed");
        if (used + n > ix->max_fill)
            return fail_status(SDFS_CDC_ECAP, "index full: %llu of %llu fingerprints held, batch of %llu",
                               (unsigned long long)used, (unsigned long long)ix->max_fill,
                               (unsigned long long)n);
        // the batch fits the fingerprints held but not those plus the tombstones: drop them first
        rebuild = used + tombs + n > ix->max_fill;
    }
    IX_TRY(ix->order.acquire(s));
    ix->last = s;
    if (rebuild) return rebuild_on(ix, s);
    return SDFS_CDC_OK;
}

// The argument checks the two walks share (before the device is touched).
static int check_walk(const sdfs_cdc_index* ix, const uint8_t* d_map, uint64_t nslots, uint32_t slot_bytes,
                      uint32_t hash_len, const uint32_t* d_slot_status, const uint64_t* d_counts) {
    if (!ix) return fail_status(SDFS_CDC_EINVAL, "null index");
    if (const int rc = check_hash_len(hash_len, HashOf::kPair)) return rc;
    if (slot_bytes < kSlotFixedBytes) return fail_status(SDFS_CDC_EINVAL, "slot_bytes %u < 13", slot_bytes);
    if (!d_slot_status || !d_counts) return fail_status(SDFS_CDC_EINVAL, "null slot_status or counts");
    if (nslots && !d_map) return fail_status(SDFS_CDC_EINVAL, "null map");
    const uint64_t parts = slot_parts(pair_cap(slot_bytes, hash_len));
    if (nslots >= (1ull << 31) || nslots * std::max<uint64_t>(parts, 1) >= (1ull << 32))
        return fail_status(SDFS_CDC_EINVAL, "%llu slots of %u bytes: split the image", (unsigned long long)nslots,
                           slot_bytes);
    return SDFS_CDC_OK;
}

// Validate, then apply, on s.  a.meta is filled in here; the caller has zeroed a.counts.
template <int MODE>
static void launch_apply(sdfs_cdc_index* ix, hipStream_t s, const WalkArgs& a, int64_t delta) {
    constexpr uint32_t wpb = kWalkThreads / 64;
    const dim3 grid((uint32_t)((a.nslots * a.parts + wpb - 1) / wpb));
    if (a.hash_len == 32)
        hipLaunchKernelGGL((ix_walk_apply_kernel<8, MODE>), grid, dim3(kWalkThreads), 0, s, a, ix->table.p,
                           ix->slots - 1, delta);
    else
        hipLaunchKernelGGL((ix_walk_apply_kernel<4, MODE>), grid, dim3(kWalkThreads), 0, s, a, ix->table.p,
                           ix->slots - 1, delta);
}

template <int MODE>
static int launch_walk(sdfs_cdc_index* ix, hipStream_t s, Scratch& sc, WalkArgs a, int64_t delta) {
    a.parts = std::max<uint32_t>(1, slot_parts(pair_cap(a.slot_bytes, a.hash_len)));
    SDFS_TRY(sc.get(&a.meta, (size_t)a.nslots));
    constexpr uint32_t wpb = kWalkThreads / 64;
    hipLaunchKernelGGL(ix_walk_validate_kernel, dim3((uint32_t)((a.nslots + wpb - 1) / wpb)), dim3(kWalkThreads), 0, s,
                       a);
    if (MODE == kWalkAddrefCheck) {  // check, then apply where nothing was missed, then the statuses
        launch_apply<kWalkAddrefCheck>(ix, s, a, delta);
        launch_apply<kWalkAddrefApply>(ix, s, a, delta);
        hipLaunchKernelGGL(ix_addref_finish_kernel, dim3((uint32_t)((a.nslots + kIxThreads - 1) / kIxThreads)),
                           dim3(kIxThreads), 0, s, a);
    } else {
        launch_apply<MODE>(ix, s, a, delta);
    }
    IX_TRY(hipGetLastError());
    return SDFS_CDC_OK;
}

extern "C" {

int sdfs_cdc_index_claim_slots(sdfs_cdc_index* ix, uint8_t* d_map, uint64_t nslots, uint32_t slot_bytes,
                               uint32_t hash_len, const uint8_t* d_sel, int64_t delta, int free_slots,
                               uint32_t* d_slot_status, uint32_t* d_slot_missed, uint64_t* d_counts, void* stream) {
    if (const int rc = check_walk(ix, d_map, nslots, slot_bytes, hash_len, d_slot_status, d_counts)) return rc;
    if (delta == 0) return fail_status(SDFS_CDC_EINVAL, "delta 0 claims nothing");
    std::lock_guard<std::mutex> lk(ix->mu);
    IX_TRY(hipSetDevice(ix->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    IX_TRY(ix->order.acquire(s));
    ix->last = s;
    IX_TRY(hipMemsetAsync(d_counts, 0, 4 * sizeof(uint64_t), s));
    if (nslots) {
        Scratch sc(s);
        WalkArgs a{d_map, nslots, slot_bytes, hash_len, d_sel, d_slot_status, d_slot_missed, nullptr, d_counts,
                   d_counts + 3, 1, nullptr, 0, nullptr, 0, nullptr};
        if (const int rc = launch_walk<kWalkClaim>(ix, s, sc, a, delta)) return rc;
        if (free_slots) {
            hipLaunchKernelGGL(ix_walk_free_kernel, dim3((uint32_t)nslots), dim3(kWalkThreads), 0, s, d_map, slot_bytes,
                               d_sel, d_slot_status);
            IX_TRY(hipGetLastError());
        }
    }
    IX_TRY(ix->order.release(s));
    return SDFS_CDC_OK;
}

int sdfs_cdc_index_addref_slots(sdfs_cdc_index* ix, const uint8_t* d_req, uint64_t nreq, uint32_t slot_bytes,
                                uint32_t hash_len, const uint8_t* d_inserted, uint32_t pair_stride,
                                uint32_t* d_status, uint32_t* d_req_missed, uint32_t* d_miss_list, uint64_t miss_cap,
                                uint64_t* d_counts, void* stream) {
    if (const int rc = check_walk(ix, d_req, nreq, slot_bytes, hash_len, d_status, d_counts)) return rc;
    if (!d_req_missed) return fail_status(SDFS_CDC_EINVAL, "null req_missed");
    if (miss_cap && !d_miss_list) return fail_status(SDFS_CDC_EINVAL, "null miss list");
    if (d_inserted && pair_stride < pair_cap(slot_bytes, hash_len))
        return fail_status(SDFS_CDC_EINVAL, "pair_stride %u: a slot of %u bytes holds up to %u pairs", pair_stride,
                           slot_bytes, pair_cap(slot_bytes, hash_len));
    std::lock_guard<std::mutex> lk(ix->mu);
    IX_TRY(hipSetDevice(ix->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    IX_TRY(ix->order.acquire(s));
    ix->last = s;
    IX_TRY(hipMemsetAsync(d_counts, 0, 6 * sizeof(uint64_t), s));
    if (nreq) {
        Scratch sc(s);
        uint64_t* vcounts = nullptr;  // the validation's own three counts
        SDFS_TRY(sc.get(&vcounts, 3));
        IX_TRY(hipMemsetAsync(vcounts, 0, 3 * sizeof(uint64_t), s));
        WalkArgs a{d_req, nreq, slot_bytes, hash_len, nullptr, d_status, d_req_missed, nullptr, vcounts, nullptr, 1,
                   d_inserted, pair_stride, d_miss_list, miss_cap, d_counts};
        if (const int rc = launch_walk<kWalkAddrefCheck>(ix, s, sc, a, 1)) return rc;
    }
    IX_TRY(ix->order.release(s));
    return SDFS_CDC_OK;
}

int sdfs_cdc_index_recount(sdfs_cdc_index* ix, const uint8_t* d_map, uint64_t nslots, uint32_t slot_bytes,
                           uint32_t hash_len, const uint8_t* d_sel, int repair, uint32_t* d_slot_status,
                           uint32_t* d_slot_missed, uint8_t* d_mis_digests, uint64_t* d_mis_pos, int64_t* d_mis_have,
                           int64_t* d_mis_want, uint64_t cap, uint64_t* d_counts, void* stream) {
    if (const int rc = check_walk(ix, d_map, nslots, slot_bytes, hash_len, d_slot_status, d_counts)) return rc;
    if (cap && (!d_mis_digests || !d_mis_pos || !d_mis_have || !d_mis_want))
        return fail_status(SDFS_CDC_EINVAL, "null mismatch list");
    std::lock_guard<std::mutex> lk(ix->mu);
    IX_TRY(hipSetDevice(ix->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    IX_TRY(ix->order.acquire(s));
    ix->last = s;
    IX_TRY(hipMemsetAsync(d_counts, 0, 8 * sizeof(uint64_t), s));
    hipLaunchKernelGGL(ix_shadow_zero_kernel, dim3((uint32_t)((ix->slots + kIxThreads - 1) / kIxThreads)),
                       dim3(kIxThreads), 0, s, ix->table.p, ix->slots);
    if (nslots) {
        Scratch sc(s);
        WalkArgs a{d_map, nslots, slot_bytes, hash_len, d_sel, d_slot_status, d_slot_missed, nullptr, d_counts,
                   nullptr, 1, nullptr, 0, nullptr, 0, nullptr};
        if (const int rc = launch_walk<kWalkShadow>(ix, s, sc, a, 0)) return rc;
    }
    const uint32_t nb = (uint32_t)((ix->slots + kRankBlock - 1) / kRankBlock);
    hipLaunchKernelGGL(ix_flag_count_kernel<kFlagMismatch>, dim3(nb), dim3(kRankBlock), 0, s, ix->table.p, ix->slots,
                       ix->sweep_bsum.p, ix->sweep_dead.p, d_counts);
    hipLaunchKernelGGL(ix_flag_scan_kernel, dim3(1), dim3(kRankBlock), 0, s, ix->sweep_bsum.p, nb, cap, d_counts + 7,
                       (uint64_t*)nullptr);
    if (cap || repair)
        hipLaunchKernelGGL(ix_recount_emit_kernel, dim3(nb), dim3(kRankBlock), 0, s, ix->table.p, ix->slots,
                           ix->sweep_bsum.p, ix->sweep_dead.p, cap, d_mis_digests, d_mis_pos, d_mis_have, d_mis_want,
                           repair);
    IX_TRY(hipGetLastError());
    IX_TRY(ix->order.release(s));
    return SDFS_CDC_OK;
}

int sdfs_cdc_index_load(sdfs_cdc_index* ix, const uint8_t* d_digests, const uint64_t* d_pos, const int64_t* d_ref,
                        uint64_t n, uint8_t* d_status, void* stream) {
    if (!ix) return fail_status(SDFS_CDC_EINVAL, "null index");
    if (n && (!d_digests || !d_pos || !d_ref || !d_status)) return fail_status(SDFS_CDC_EINVAL, "null argument");
    if (n >= (1ull << 31)) return fail_status(SDFS_CDC_EINVAL, "batch too large");
    if (n == 0) return SDFS_CDC_OK;
    std::lock_guard<std::mutex> lk(ix->mu);
    IX_TRY(hipSetDevice(ix->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (const int rc = make_room(ix, s, n)) return rc;
    const uint64_t lsize = std::max<uint64_t>(64, next_pow2(2 * n));
    if (ix->ltab.ensure(lsize) != hipSuccess || ix->lminpos.ensure(lsize) != hipSuccess ||
        ix->gidx.ensure(lsize) != hipSuccess || ix->lslot.ensure(n) != hipSuccess)
        return fail_status(SDFS_CDC_ENOMEM, "index scratch allocation failed");
    ix->epoch = (ix->epoch + 1) & 0x7FFFFFFFu;
    if (ix->epoch == 0) ix->epoch = 1;
    const uint32_t stamp = (ix->epoch << 1) | 1u;
    IX_TRY(hipMemsetAsync(ix->ltab.p, 0xFF, lsize * sizeof(uint32_t), s));
    IX_TRY(hipMemsetAsync(ix->lminpos.p, 0xFF, lsize * sizeof(unsigned long long), s));
    const uint32_t g = (uint32_t)((n + kIxThreads - 1) / kIxThreads);
    hipLaunchKernelGGL(ix_load_group_kernel, dim3(g), dim3(kIxThreads), 0, s, d_digests, d_pos, (uint32_t)n, ix->ltab.p,
                       ix->lminpos.p, (uint32_t)(lsize - 1), ix->lslot.p);
    hipLaunchKernelGGL(ix_load_probe_kernel, dim3(g), dim3(kIxThreads), 0, s, d_digests, (uint32_t)n, ix->ltab.p,
                       ix->lminpos.p, ix->lslot.p, ix->table.p, ix->slots - 1, stamp, ix->gidx.p, ix->used.p,
                       ix->overflow.p);
    hipLaunchKernelGGL(ix_load_apply_kernel, dim3(g), dim3(kIxThreads), 0, s, d_pos, d_ref, (uint32_t)n, ix->ltab.p,
                       ix->lslot.p, ix->gidx.p, ix->table.p, stamp, d_status);
    IX_TRY(hipGetLastError());
    IX_TRY(ix->order.release(s));
    ix->used_ub += n;
    return SDFS_CDC_OK;
}

int sdfs_cdc_index_export(sdfs_cdc_index* ix, uint8_t* d_digests, uint64_t* d_pos, int64_t* d_ref, uint64_t cap,
                          uint64_t* d_n, void* stream) {
    if (!ix) return fail_status(SDFS_CDC_EINVAL, "null index");
    if (!d_n) return fail_status(SDFS_CDC_EINVAL, "null counts");
    if (cap && (!d_digests || !d_pos || !d_ref)) return fail_status(SDFS_CDC_EINVAL, "null export list");
    std::lock_guard<std::mutex> lk(ix->mu);
    IX_TRY(hipSetDevice(ix->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    IX_TRY(ix->order.acquire(s));
    ix->last = s;
    const uint32_t nb = (uint32_t)((ix->slots + kRankBlock - 1) / kRankBlock);
    hipLaunchKernelGGL(ix_flag_count_kernel<kFlagHeld>, dim3(nb), dim3(kRankBlock), 0, s, ix->table.p, ix->slots,
                       ix->sweep_bsum.p, ix->sweep_dead.p, (uint64_t*)nullptr);
    hipLaunchKernelGGL(ix_flag_scan_kernel, dim3(1), dim3(kRankBlock), 0, s, ix->sweep_bsum.p, nb, cap, d_n, d_n + 1);
    if (cap)
        hipLaunchKernelGGL(ix_export_emit_kernel, dim3(nb), dim3(kRankBlock), 0, s, ix->table.p, ix->slots,
                           ix->sweep_bsum.p, ix->sweep_dead.p, cap, d_digests, d_pos, d_ref);
    IX_TRY(hipGetLastError());
    IX_TRY(ix->order.release(s));
    return SDFS_CDC_OK;
}

int sdfs_cdc_index_create(int device, uint64_t capacity, sdfs_cdc_index** out) {
    if (!out) return fail_status(SDFS_CDC_EINVAL, "null output");
    *out = nullptr;
    if (capacity == 0 || capacity > (1ull << 30)) return fail_status(SDFS_CDC_EINVAL, "capacity out of range");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return fail_status(SDFS_CDC_ENODEV, "no HIP device %d", device);
    IX_TRY(hipSetDevice(device));
    auto* ix = new sdfs_cdc_index();
    ix->device = device;
    if (ix->order.init() != hipSuccess || hipStreamCreateWithFlags(&ix->own, hipStreamNonBlocking) != hipSuccess) {
        ix->order.destroy();
        delete ix;
        return fail_status(SDFS_CDC_EHIP, "event or stream creation failed");
    }
    ix->last = ix->own;
    ix->slots = next_pow2(capacity + capacity / 7 + 1);
    ix->max_fill = ix->slots - ix->slots / 8;
    if (ix->table.ensure(ix->slots) != hipSuccess || ix->used.ensure(2) != hipSuccess ||
        ix->overflow.ensure(1) != hipSuccess ||
        ix->sweep_bsum.ensure((ix->slots + kRankBlock - 1) / kRankBlock) != hipSuccess ||
        ix->sweep_dead.ensure((ix->slots + kRankBlock - 1) / kRankBlock * (kRankBlock / 64)) != hipSuccess) {
        sdfs_cdc_index_destroy(ix);
        return fail_status(SDFS_CDC_ENOMEM, "index allocation (%llu slots) failed",
                           (unsigned long long)ix->slots);
    }
    // Nothing here or below runs on the legacy null stream or synchronises the device: the CDC
    // queue's lanes are blocking streams, and a null-stream operation would wait for their passes.
    if (hipMemsetAsync(ix->table.p, 0, ix->slots * sizeof(IndexSlot), ix->own) != hipSuccess ||
        hipMemsetAsync(ix->used.p, 0, 2 * sizeof(uint64_t), ix->own) != hipSuccess ||
        hipMemsetAsync(ix->overflow.p, 0, sizeof(uint32_t), ix->own) != hipSuccess ||
        hipStreamSynchronize(ix->own) != hipSuccess) {
        sdfs_cdc_index_destroy(ix);
        return fail_status(SDFS_CDC_EHIP, "index initialisation failed");
    }
    *out = ix;
    return SDFS_CDC_OK;
}

int sdfs_cdc_index_destroy(sdfs_cdc_index* ix) {
    if (!ix) return SDFS_CDC_OK;
    (void)hipSetDevice(ix->device);
    // batches are chained in call order (StreamOrder), so the latest one's stream finishing means
    // every earlier one has
    if (ix->last) (void)hipStreamSynchronize(ix->last);
    if (ix->own) (void)hipStreamSynchronize(ix->own);
    ix->table.release();
    ix->used.release();
    for (auto* b : {&ix->ltab, &ix->lcount, &ix->lslot, &ix->gidx, &ix->isnew, &ix->bsum, &ix->overflow,
                    &ix->sweep_bsum})
        b->release();
    ix->sweep_dead.release();
    ix->lminpos.release();
    ix->order.destroy();
    if (ix->own) (void)hipStreamDestroy(ix->own);
    delete ix;
    return SDFS_CDC_OK;
}

int sdfs_cdc_index_put_records(sdfs_cdc_index* ix, const uint8_t* d_records, uint64_t n_max,
                               const uint32_t* d_count, uint64_t pos_base, uint8_t* d_dup, uint64_t* d_hashloc,
                               uint32_t* d_new_list, uint64_t* d_new_count, void* stream) {
    if (!ix) return fail_status(SDFS_CDC_EINVAL, "null index");
    if (!d_new_count) return fail_status(SDFS_CDC_EINVAL, "null new_count");
    if (n_max && !d_records) return fail_status(SDFS_CDC_EINVAL, "null records");
    if (n_max >= (1ull << 31)) return fail_status(SDFS_CDC_EINVAL, "batch too large");
    std::lock_guard<std::mutex> lk(ix->mu);
    IX_TRY(hipSetDevice(ix->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (const int rc = make_room(ix, s, n_max)) return rc;
    if (n_max == 0) {
        IX_TRY(hipMemsetAsync(d_new_count, 0, sizeof(uint64_t), s));
        IX_TRY(ix->order.release(s));
        return SDFS_CDC_OK;
    }
    const uint64_t lsize = std::max<uint64_t>(64, next_pow2(2 * n_max));
    const uint32_t nrank = (uint32_t)((n_max + kRankBlock - 1) / kRankBlock);
    if (ix->ltab.ensure(lsize) != hipSuccess || ix->lcount.ensure(lsize) != hipSuccess ||
        ix->gidx.ensure(lsize) != hipSuccess || ix->lslot.ensure(n_max) != hipSuccess ||
        ix->isnew.ensure(n_max) != hipSuccess || ix->bsum.ensure(nrank) != hipSuccess)
        return fail_status(SDFS_CDC_ENOMEM, "index scratch allocation failed");
    ix->epoch = (ix->epoch + 1) & 0x7FFFFFFFu;
    if (ix->epoch == 0) ix->epoch = 1;
    const uint32_t stamp = (ix->epoch << 1) | 1u;
    IX_TRY(hipMemsetAsync(ix->ltab.p, 0xFF, lsize * sizeof(uint32_t), s));
    IX_TRY(hipMemsetAsync(ix->lcount.p, 0, lsize * sizeof(uint32_t), s));
    const uint32_t g = (uint32_t)((n_max + kIxThreads - 1) / kIxThreads);
    const uint64_t cmask = ix->slots - 1;
    hipLaunchKernelGGL(ix_group_kernel, dim3(g), dim3(kIxThreads), 0, s, d_records, d_count, n_max, ix->ltab.p,
                       ix->lcount.p, (uint32_t)(lsize - 1), ix->lslot.p);
    hipLaunchKernelGGL(ix_probe_kernel, dim3(g), dim3(kIxThreads), 0, s, d_records, d_count, n_max, ix->ltab.p,
                       ix->lcount.p, ix->lslot.p, ix->table.p, cmask, stamp, ix->gidx.p, ix->isnew.p,
                       ix->overflow.p);
    hipLaunchKernelGGL(ix_count_kernel, dim3(nrank), dim3(kRankBlock), 0, s, d_count, n_max, ix->isnew.p,
                       ix->bsum.p);
    hipLaunchKernelGGL(ix_scan_kernel, dim3(1), dim3(kRankBlock), 0, s, ix->bsum.p, nrank, d_new_count, ix->used.p);
    hipLaunchKernelGGL(ix_assign_kernel, dim3(nrank), dim3(kRankBlock), 0, s, d_count, n_max, ix->isnew.p,
                       ix->bsum.p, ix->lslot.p, ix->gidx.p, ix->table.p, pos_base, d_new_list);
    hipLaunchKernelGGL(ix_output_kernel, dim3(g), dim3(kIxThreads), 0, s, d_count, n_max, ix->isnew.p, ix->lslot.p,
                       ix->gidx.p, ix->table.p, d_dup, d_hashloc);
    IX_TRY(hipGetLastError());
    IX_TRY(ix->order.release(s));
    ix->used_ub += n_max;
    return SDFS_CDC_OK;
}

int sdfs_cdc_index_get(sdfs_cdc_index* ix, const uint8_t* d_digests, uint64_t n, uint64_t* d_pos,
                       uint64_t* d_refcount, void* stream) {
    if (!ix) return fail_status(SDFS_CDC_EINVAL, "null index");
    if (n && !d_digests) return fail_status(SDFS_CDC_EINVAL, "null digests");
    if (n == 0) return SDFS_CDC_OK;
    std::lock_guard<std::mutex> lk(ix->mu);
    IX_TRY(hipSetDevice(ix->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    IX_TRY(ix->order.acquire(s));
    ix->last = s;
    const uint64_t g = (n + kIxThreads - 1) / kIxThreads;
    hipLaunchKernelGGL(ix_get_kernel, dim3((uint32_t)g), dim3(kIxThreads), 0, s, d_digests, n, ix->table.p,
                       ix->slots - 1, d_pos, d_refcount);
    IX_TRY(hipGetLastError());
    IX_TRY(ix->order.release(s));
    return SDFS_CDC_OK;
}

int sdfs_cdc_index_clear(sdfs_cdc_index* ix, void* stream) {
    if (!ix) return fail_status(SDFS_CDC_EINVAL, "null index");
    std::lock_guard<std::mutex> lk(ix->mu);
    IX_TRY(hipSetDevice(ix->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    IX_TRY(ix->order.acquire(s));
    IX_TRY(hipMemsetAsync(ix->table.p, 0, ix->slots * sizeof(IndexSlot), s));
    IX_TRY(hipMemsetAsync(ix->used.p, 0, 2 * sizeof(uint64_t), s));
    IX_TRY(hipMemsetAsync(ix->overflow.p, 0, sizeof(uint32_t), s));
    IX_TRY(ix->order.release(s));
    ix->used_ub = 0;
    ix->tomb_ub = 0;
    ix->last = s;
    return SDFS_CDC_OK;
}

int sdfs_cdc_index_claim(sdfs_cdc_index* ix, const uint8_t* d_digests, const uint64_t* d_expect_pos,
                         const int64_t* d_delta, uint64_t n, uint64_t* d_out_pos, void* stream) {
    if (!ix) return fail_status(SDFS_CDC_EINVAL, "null index");
    if (n && !d_digests) return fail_status(SDFS_CDC_EINVAL, "null digests");
    if (n && !d_delta) return fail_status(SDFS_CDC_EINVAL, "null delta");
    if (n >= (1ull << 31) * kIxThreads) return fail_status(SDFS_CDC_EINVAL, "batch too large");
    if (n == 0) return SDFS_CDC_OK;
    std::lock_guard<std::mutex> lk(ix->mu);
    IX_TRY(hipSetDevice(ix->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    IX_TRY(ix->order.acquire(s));
    ix->last = s;
    const uint64_t g = (n + kIxThreads - 1) / kIxThreads;
    hipLaunchKernelGGL(ix_claim_kernel, dim3((uint32_t)g), dim3(kIxThreads), 0, s, d_digests, d_expect_pos, d_delta, n,
                       ix->table.p, ix->slots - 1, d_out_pos);
    IX_TRY(hipGetLastError());
    IX_TRY(ix->order.release(s));
    return SDFS_CDC_OK;
}

int sdfs_cdc_index_sweep(sdfs_cdc_index* ix, uint8_t* d_removed_digests, uint64_t* d_removed_pos, uint64_t cap,
                         uint64_t* d_counts, void* stream) {
    if (!ix) return fail_status(SDFS_CDC_EINVAL, "null index");
    if (!d_counts) return fail_status(SDFS_CDC_EINVAL, "null counts");
    if (cap && (!d_removed_digests || !d_removed_pos)) return fail_status(SDFS_CDC_EINVAL, "null removed list");
    std::lock_guard<std::mutex> lk(ix->mu);
    IX_TRY(hipSetDevice(ix->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    IX_TRY(ix->order.acquire(s));
    ix->last = s;
    const uint32_t nb = (uint32_t)((ix->slots + kRankBlock - 1) / kRankBlock);
    hipLaunchKernelGGL(ix_sweep_count_kernel, dim3(nb), dim3(kRankBlock), 0, s, ix->table.p, ix->slots,
                       ix->sweep_bsum.p, ix->sweep_dead.p);
    hipLaunchKernelGGL(ix_sweep_scan_kernel, dim3(1), dim3(kRankBlock), 0, s, ix->sweep_bsum.p, nb, cap, d_counts,
                       ix->used.p);
    hipLaunchKernelGGL(ix_sweep_emit_kernel, dim3(nb), dim3(kRankBlock), 0, s, ix->table.p, ix->slots,
                       ix->sweep_bsum.p, ix->sweep_dead.p, cap, d_removed_digests, d_removed_pos);
    IX_TRY(hipGetLastError());
    IX_TRY(ix->order.release(s));
    return SDFS_CDC_OK;
}

int sdfs_cdc_index_compact(sdfs_cdc_index* ix, void* stream) {
    if (!ix) return fail_status(SDFS_CDC_EINVAL, "null index");
    std::lock_guard<std::mutex> lk(ix->mu);
    IX_TRY(hipSetDevice(ix->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    IX_TRY(ix->order.acquire(s));
    ix->last = s;
    const int rc = rebuild_on(ix, s);
    if (rc != SDFS_CDC_OK) return rc;
    IX_TRY(ix->order.release(s));
    return SDFS_CDC_OK;
}

int sdfs_cdc_index_stats(sdfs_cdc_index* ix, uint64_t* live, uint64_t* tombstones, uint64_t* capacity) {
    if (!ix) return fail_status(SDFS_CDC_EINVAL, "null index");
    std::lock_guard<std::mutex> lk(ix->mu);
    IX_TRY(hipSetDevice(ix->device));
    uint64_t u = 0, t = 0;
    const int rc = read_counts(ix, &u, &t, nullptr);
    if (rc != SDFS_CDC_OK) return rc;
    if (live) *live = u;
    if (tombstones) *tombstones = t;
    if (capacity) *capacity = ix->max_fill;
    return SDFS_CDC_OK;
}

int sdfs_cdc_index_set_epoch(sdfs_cdc_index* ix, uint32_t epoch) {
    if (!ix) return fail_status(SDFS_CDC_EINVAL, "null index");
    std::lock_guard<std::mutex> lk(ix->mu);
    ix->epoch = epoch & 0x7FFFFFFFu;  // the next batch uses epoch + 1 (wrapping to 1)
    return SDFS_CDC_OK;
}

int sdfs_cdc_index_size(sdfs_cdc_index* ix, uint64_t* used, uint64_t* capacity) {
    if (!ix) return fail_status(SDFS_CDC_EINVAL, "null index");
    std::lock_guard<std::mutex> lk(ix->mu);
    IX_TRY(hipSetDevice(ix->device));
    uint64_t u = 0, t = 0;
    const int rc = read_counts(ix, &u, &t, nullptr);
    if (rc != SDFS_CDC_OK) return rc;
    if (used) *used = u;
    if (capacity) *capacity = ix->max_fill;
    return SDFS_CDC_OK;
}

}  // extern "C"
