// The one-lane LZ4 decoder of the split decode (sdfs_amd/csrc/lz4_decode.h: decompress_lane,
// dec_lane_class) on the host, under AddressSanitizer and UBSan, against a byte-at-a-time model.
//
// Every case runs twice: once with input and output in exactly sized heap buffers (the
// sanitizer sees a read or a write one byte outside), once with the output between two guard
// zones (a stray write that lands inside the program's own memory).  The decoder and the model
// must give the same verdict and, up to the returned length, the same bytes.
//
// Cases: (1) blocks of liblz4's encoders (dlopen'd for encoder output only: LZ4_compress_fast at
// acceleration 1, 5, 9 and LZ4_compress_HC at level 9; skipped without a liblz4) and blocks of
// this file's own emitter from random sequence lists, each unmutated, bit-flipped, truncated or
// overwritten, with caps from len - 8 to len + 20, as a bare block and as a putChunk record;
// (2) the structural edges: literal runs, offsets x match lengths, the last match ending at
// cap - j, 4 .. 35 input bytes left at a sequence start, blocks ending on 0 .. 16 literals,
// zero-literal sequences back to back.
#include <dlfcn.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../sdfs_amd/csrc/lz4_decode.h"

namespace {

typedef std::vector<uint8_t> Bytes;
constexpr long kBad = -1;

uint64_t g_state = 0x243F6A8885A308D3ull;
uint64_t rnd() {
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }

// ---- the model: one byte at a time, no fast path (the rule set in lz4_decode.h's header)
long model_decode(const Bytes& src, size_t cap, Bytes& out) {
    out.clear();
    const size_t n = src.size();
    size_t ip = 0;
    for (;;) {
        if (ip >= n) return kBad;
        const uint32_t token = src[ip++];
        size_t lit = token >> 4;
        if (lit == 15) {
            uint32_t b;
            do {
                if (ip >= n) return kBad;
                b = src[ip++];
                lit += b;
            } while (b == 255);
        }
        if (ip + lit > n) return kBad;
        if (out.size() + lit > cap) return kBad;
        for (size_t k = 0; k < lit; k++) out.push_back(src[ip + k]);
        ip += lit;
        if (ip == n) return (long)out.size();
        if (ip + 2 > n) return kBad;
        const size_t off = src[ip] | (size_t)src[ip + 1] << 8;
        ip += 2;
        if (off == 0 || off > out.size()) return kBad;
        size_t ml = token & 15;
        if (ml == 15) {
            uint32_t b;
            do {
                if (ip >= n) return kBad;
                b = src[ip++];
                ml += b;
            } while (b == 255);
        }
        ml += 4;
        if (out.size() + ml > cap) return kBad;
        for (size_t k = 0; k < ml; k++) out.push_back(out[out.size() - off]);
    }
}

// the framed rule of the decode kernels: [BE32 nz][payload]
long model_record(const Bytes& rec, size_t cap, Bytes& out) {
    out.clear();
    if (rec.size() < 4) return kBad;
    const int32_t nz = (int32_t)((uint32_t)rec[0] << 24 | (uint32_t)rec[1] << 16 | (uint32_t)rec[2] << 8 | rec[3]);
    const Bytes payload(rec.begin() + 4, rec.end());
    if (nz > 0) {
        if ((size_t)nz > cap) return kBad;
        return model_decode(payload, (size_t)nz, out) == nz ? nz : kBad;
    }
    if (payload.size() > cap) return kBad;
    out = payload;
    return (long)out.size();
}

// ---- the emitter
struct Seq {
    Bytes lits;
    uint32_t off, ml;
};

void put_len(Bytes& o, size_t v) {
    for (; v >= 255; v -= 255) o.push_back(255);
    o.push_back((uint8_t)v);
}

Bytes emit(const std::vector<Seq>& seqs, const Bytes& last) {
    Bytes o;
    for (const Seq& s : seqs) {
        const size_t ll = s.lits.size(), m = s.ml - 4;
        o.push_back((uint8_t)((ll < 15 ? ll : 15) << 4 | (m < 15 ? m : 15)));
        if (ll >= 15) put_len(o, ll - 15);
        o.insert(o.end(), s.lits.begin(), s.lits.end());
        o.push_back((uint8_t)(s.off & 255));
        o.push_back((uint8_t)(s.off >> 8));
        if (m >= 15) put_len(o, m - 15);
    }
    o.push_back((uint8_t)((last.size() < 15 ? last.size() : 15) << 4));
    if (last.size() >= 15) put_len(o, last.size() - 15);
    o.insert(o.end(), last.begin(), last.end());
    return o;
}

Bytes rbytes(size_t n) {
    Bytes b(n);
    for (auto& x : b) x = (uint8_t)rnd();
    return b;
}

// ---- one case through the decoder under test
long g_cases = 0, g_accepted = 0, g_lane_class = 0;
constexpr size_t kGuard = 64;

[[noreturn]] void fail(const char* what, const Bytes& in, size_t cap, int framed, long want, long got) {
    fprintf(stderr, "FAIL %s: n=%zu cap=%zu framed=%d model=%ld decoder=%ld\nblock:", what, in.size(), cap, framed,
            want, got);
    for (size_t i = 0; i < in.size() && i < 96; i++) fprintf(stderr, " %02x", in[i]);
    fprintf(stderr, "\n");
    exit(1);
}

// the body of lz4_decompress_lane_kernel for one record the lane kernel takes
long lane_record(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t cap, int framed) {
    uint32_t got;
    if (framed) {
        const uint32_t nz = (uint32_t)in[0] << 24 | (uint32_t)in[1] << 16 | (uint32_t)in[2] << 8 | in[3];
        got = nz <= cap ? sdfs::decompress_lane(in + 4, n - 4, out, nz) : sdfs::kLz4Corrupt;
        if (got != nz) got = sdfs::kLz4Corrupt;
    } else {
        got = sdfs::decompress_lane(in, n, out, cap);
    }
    return got == sdfs::kLz4Corrupt ? kBad : (long)got;
}

void run_case(const Bytes& in, size_t cap, int framed) {
    g_cases++;
    Bytes want;
    const long w = framed ? model_record(in, cap, want) : model_decode(in, cap, want);
    if (w >= 0) g_accepted++;
    // exactly sized heap buffers
    uint8_t* src = (uint8_t*)malloc(in.size());
    if (!in.empty()) memcpy(src, in.data(), in.size());
    const bool lane = sdfs::dec_lane_class(src, (uint32_t)in.size(), (uint32_t)cap, (uint32_t)framed);
    {   // the routing rule, restated
        bool expect;
        if (framed) {
            int32_t nz = 0;
            if (in.size() >= 4) nz = (int32_t)((uint32_t)in[0] << 24 | (uint32_t)in[1] << 16 | (uint32_t)in[2] << 8 | in[3]);
            expect = in.size() >= 4 && nz > 0 && (uint64_t)(in.size() - 4) * 16 < (uint64_t)nz * 15;
        } else {
            expect = (uint64_t)in.size() * 16 < (uint64_t)cap * 15;
        }
        if (lane != expect) fail("dec_lane_class", in, cap, framed, expect, lane);
    }
    // a framed record outside the lane class (raw, short header) is the wave kernel's: the lane
    // kernel never touches it.  A bare block is decoded whatever its class.
    if (framed && !lane) {
        free(src);
        return;
    }
    if (lane) g_lane_class++;
    size_t room = cap;  // framed: the decoder is given nz <= cap bytes, so the buffer is that small
    if (framed) {
        const uint32_t nz = (uint32_t)in[0] << 24 | (uint32_t)in[1] << 16 | (uint32_t)in[2] << 8 | in[3];
        if (nz < room) room = nz;
    }
    uint8_t* dst = (uint8_t*)malloc(room);
    const long g = lane_record(src, (uint32_t)in.size(), dst, (uint32_t)cap, framed);
    if (g != w) fail("verdict", in, cap, framed, w, g);
    if (g > 0 && memcmp(dst, want.data(), (size_t)g) != 0) fail("bytes", in, cap, framed, w, g);
    if (!in.empty() && memcmp(src, in.data(), in.size()) != 0) fail("input changed", in, cap, framed, w, g);
    free(dst);
    // between guard zones
    Bytes buf(cap + 2 * kGuard, 0xA5);
    const long g2 = lane_record(src, (uint32_t)in.size(), buf.data() + kGuard, (uint32_t)cap, framed);
    if (g2 != w) fail("verdict (guarded run)", in, cap, framed, w, g2);
    for (size_t i = 0; i < kGuard; i++)
        if (buf[i] != 0xA5 || buf[kGuard + cap + i] != 0xA5) fail("guard byte", in, cap, framed, w, g2);
    if (g2 > 0 && memcmp(buf.data() + kGuard, want.data(), (size_t)g2) != 0) fail("bytes (guarded run)", in, cap, framed, w, g2);
    free(src);
}

Bytes framed_record(const Bytes& block, int32_t nz) {
    Bytes r = {(uint8_t)((uint32_t)nz >> 24), (uint8_t)((uint32_t)nz >> 16), (uint8_t)((uint32_t)nz >> 8), (uint8_t)nz};
    r.insert(r.end(), block.begin(), block.end());
    return r;
}

// a block whose decoded length is `len`, as a bare block and as a record, under one cap
void both_forms(const Bytes& block, size_t len, size_t cap) {
    run_case(block, cap, 0);
    run_case(framed_record(block, (int32_t)cap), cap, 1);              // nz = cap: SHORT unless cap == len
    run_case(framed_record(block, (int32_t)len), cap, 1);              // nz = len, room cap
}

void all_caps(const Bytes& block) {
    Bytes tmp;
    const long len = model_decode(block, (size_t)1 << 30, tmp);
    if (len < 0) fail("edge block is not valid", block, 0, 0, len, 0);
    for (long cap = len - 8; cap <= len + 20; cap++)
        if (cap >= 0) both_forms(block, (size_t)len, (size_t)cap);
}

// ---- encoder output
typedef int (*fast_fn)(const char*, char*, int, int, int);
fast_fn g_fast = nullptr, g_hc = nullptr;

Bytes make_input(size_t n) {
    Bytes d(n);
    switch (below(5)) {
    case 0:
        for (auto& x : d) x = (uint8_t)rnd();
        break;
    case 1: {  // words
        static const char* w[] = {"the ", "chunk ", "store ", "of ", "hash ", "index ", "and\n", "volume ", "a ", "dedup "};
        size_t p = 0;
        while (p < n) {
            const char* s = w[below(10)];
            for (; *s && p < n; s++) d[p++] = (uint8_t)*s;
        }
        break;
    }
    case 2: {  // short period
        const uint32_t per = 1 + below(9);
        const Bytes pat = rbytes(per);
        for (size_t i = 0; i < n; i++) d[i] = pat[i % per];
        break;
    }
    case 3: {  // runs, repeats of earlier bytes, noise
        size_t p = 0;
        while (p < n) {
            const size_t run = 1 + below(60);
            const uint32_t kind = below(3);
            const size_t dist = p ? 1 + below((uint32_t)(p < 300 ? p : 300)) : 0;
            const uint8_t v = (uint8_t)rnd();
            for (size_t k = 0; k < run && p < n; k++, p++)
                d[p] = kind == 0 ? v : (kind == 1 && dist ? d[p - dist] : (uint8_t)rnd());
        }
        break;
    }
    default:
        break;  // zeros
    }
    return d;
}

Bytes encode(const Bytes& d, int which) {
    Bytes out(d.size() + d.size() / 255 + 16);
    const int acc[] = {1, 5, 9};
    const int k = which < 3 ? g_fast((const char*)d.data(), (char*)out.data(), (int)d.size(), (int)out.size(), acc[which])
                            : g_hc((const char*)d.data(), (char*)out.data(), (int)d.size(), (int)out.size(), 9);
    out.resize(k > 0 ? (size_t)k : 0);
    return out;
}

// a valid block from a random sequence list: offsets 1 .. 7 and long ones, zero-literal
// sequences, matches longer than their offset, any number of last literals
Bytes random_block() {
    std::vector<Seq> seqs;
    size_t op = 0;
    const uint32_t ns = below(8);
    for (uint32_t i = 0; i < ns; i++) {
        Seq s;
        s.lits = rbytes(op == 0 ? 1 + below(20) : (below(3) == 0 ? 0 : below(below(4) == 0 ? 300 : 18)));
        op += s.lits.size();
        s.off = below(2) ? 1 + below((uint32_t)(op < 8 ? op : 8)) : 1 + below((uint32_t)op);
        s.ml = 4 + (below(4) == 0 ? below(600) : below(24));
        op += s.ml;
        seqs.push_back(s);
    }
    return emit(seqs, rbytes(below(3) == 0 ? 0 : below(22)));
}

void mutate(Bytes& b) {
    if (b.empty()) return;
    switch (below(4)) {
    case 0:
        for (uint32_t k = 1 + below(2); k; k--) b[below((uint32_t)b.size())] ^= (uint8_t)(1u << below(8));
        break;
    case 1:
        b.resize(below((uint32_t)b.size()));
        break;
    case 2: {
        const size_t p = below((uint32_t)b.size());
        for (size_t k = 0; k < 1 + below(4) && p + k < b.size(); k++) b[p + k] = (uint8_t)rnd();
        break;
    }
    default:
        break;  // unmutated
    }
}

void random_cases(long count) {
    Bytes tmp;
    const long until = g_cases + count;
    while (g_cases < until) {
        Bytes blk;
        const uint32_t src = below(6);
        if (src < 4 && (src < 3 ? g_fast : g_hc)) {
            const uint32_t r = below(20);
            blk = encode(make_input(r == 0 ? below(6000) : (r < 4 ? below(24) : 20 + below(680))), (int)src);
        }
        if (blk.empty()) blk = random_block();
        long len = model_decode(blk, (size_t)1 << 30, tmp);
        if (len < 0) fail("encoder block is not valid", blk, 0, 0, len, 0);
        mutate(blk);
        const long cap = len - 8 + (long)below(29);
        if (cap < 0) continue;
        if (below(2))
            run_case(blk, (size_t)cap, 0);
        else
            run_case(framed_record(blk, (int32_t)(below(4) ? cap : len)), (size_t)cap, 1);
    }
}

void edge_cases() {
    const size_t lit_runs[] = {0, 1, 14, 15, 16, 17, 269, 270, 271, 3087, 3088, 4095, 4096, 4097, 5000};
    const uint32_t offsets[] = {1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 255, 256, 4095, 65535};
    const uint32_t match_lens[] = {4, 5, 7, 8, 9, 15, 18, 19, 20, 63, 64, 65, 128, 273, 274, 275, 4100, 70000};
    for (size_t ll : lit_runs) {
        all_caps(emit({{rbytes(40), 8, 8}, {rbytes(ll), 16, 6}}, rbytes(5)));
        all_caps(emit({}, rbytes(ll)));
        all_caps(emit({{rbytes(9), 9, 4}}, rbytes(ll)));
    }
    for (uint32_t off : offsets)
        for (uint32_t ml : match_lens) {
            if (ml == 70000 && off != 1 && off != 8 && off != 65535) continue;
            if (off == 65535 && ml != 4 && ml != 64 && ml != 70000) continue;
            all_caps(emit({{rbytes(off), off, ml}}, rbytes(5)));
            all_caps(emit({{rbytes(off + 3), off, ml}}, rbytes(below(6))));
            // the same match as a short-literal sequence in the middle of a block (the fast path)
            if (off < 200) all_caps(emit({{rbytes(200), 100, 10}, {rbytes(below(15)), off, ml}, {rbytes(3), 1, 4}}, rbytes(20)));
        }
    // long matches that do not overlap their source
    for (const auto& t : {std::pair<uint32_t, uint32_t>{5000, 3087}, {5000, 3088}, {5000, 4100}, {65535, 4100}})
        all_caps(emit({{rbytes(t.first + 1), t.first, t.second}}, rbytes(2)));
    // the last match ends at cap - j (all_caps moves cap over len - 8 .. len + 20)
    const uint32_t tail[][3] = {{12, 20, 14}, {12, 9, 3}, {3, 20, 14}, {8, 4, 14}, {5, 9, 3}, {16, 24, 14}, {1, 4, 0}, {9, 17, 7}};
    for (const auto& t : tail)
        for (size_t j = 0; j <= 16; j++) all_caps(emit({{rbytes(30), 10, 5}, {rbytes(t[2]), t[0], t[1]}}, rbytes(j)));
    // 4 .. 35 input bytes left at the start of the second sequence; blocks ending on 0 .. 16 literals
    for (size_t a = 0; a < 15; a++)
        for (size_t b = 0; b <= 16; b++) all_caps(emit({{rbytes(20), 8, 8}, {rbytes(a), 5, 6}}, rbytes(b)));
    for (size_t b = 0; b <= 5; b++)  // zero-literal sequences back to back
        all_caps(emit({{rbytes(16), 3, 7}, {{}, 1, 30}, {{}, 7, 100}, {{}, 9, 5}, {{}, 64, 64}}, rbytes(b)));
    // records of 0 .. 3 bytes, header edges, an empty block under a nonzero cap
    for (size_t n = 0; n <= 3; n++) run_case(rbytes(n), 16, 1);
    run_case({}, 64, 0);
    run_case({}, 0, 0);
    const Bytes blk = emit({{rbytes(10), 4, 30}}, rbytes(3));
    for (int32_t nz : {43, 42, 44, 0, -1, 1, 1000, 0x7fffffff, (int32_t)0x80000000}) run_case(framed_record(blk, nz), 43, 1);
}

}  // namespace

int main(int argc, char** argv) {
    const long count = argc > 1 ? atol(argv[1]) : 200000;
    if (void* h = dlopen("liblz4.so.1", RTLD_NOW)) {
        g_fast = (fast_fn)dlsym(h, "LZ4_compress_fast");
        g_hc = (fast_fn)dlsym(h, "LZ4_compress_HC");
    }
    if (!g_fast) printf("no liblz4: encoder cases skipped (emitter blocks only)\n");
    edge_cases();
    const long edges = g_cases;
    random_cases(count);
    printf("edge cases %ld, random cases %ld, accepted %ld, lane-class %ld\n", edges, g_cases - edges, g_accepted,
           g_lane_class);
    if (g_cases - edges < count || g_accepted < g_cases / 20) {
        printf("case mix too thin\n");
        return 1;
    }
    printf("OK\n");
    return 0;
}
