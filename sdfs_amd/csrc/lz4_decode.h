// lz4_decode.h — the one-lane LZ4 block decoder and the routing rule of the split decode
// (lz4_kernels.hip), in plain C++ so that a host program can run the same text under sanitizers
// (tests/cpu/lz4_decode_fuzz.cpp).  No HIP include: under hipcc the functions are
// __host__ __device__, elsewhere they are ordinary inline functions.
//
// Accept rule set (both device decoders and tests/lz4_block_model.py): a block is a run of
// sequences [token][literal length bytes][literals][offset LE16][match length bytes]; a token, a
// length byte or an offset wanted at or past n, a literal run past the input or past cap, an
// offset of zero or greater than the bytes decoded so far, and a match past cap are malformed.
// The only accepted end is ip == n right after a literal run (which may be empty); the encoder-
// side end-of-block restrictions (last five bytes literal, last match 12 bytes before the end)
// are not required of the input.
#ifndef SDFS_LZ4_DECODE_H
#define SDFS_LZ4_DECODE_H

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define SDFS_LZ4_HD __host__ __device__
#else
#define SDFS_LZ4_HD
#endif

namespace sdfs {

constexpr uint32_t kMinMatch = 4, kMlMask = 15, kRunMask = 15;
constexpr uint32_t kLz4Corrupt = 0xFFFFFFFFu;

// unaligned 8-byte word (device: one dwordx2 load)
SDFS_LZ4_HD inline __attribute__((always_inline)) uint64_t g64(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// Routing of the split decode: a block that saved under 1/16 of its bytes (or a raw record) is
// mostly literal runs, which the wave kernel copies coalesced; the others are short sequences,
// which one lane per block parses without the wave's per-sequence round trips.
SDFS_LZ4_HD inline __attribute__((always_inline)) bool dec_lane_class(const uint8_t* in, uint32_t n, uint32_t cap,
                                                                      uint32_t framed) {
    uint32_t out = cap;
    if (framed) {
        if (n < 4) return false;
        const int32_t nz = (int32_t)((uint32_t)in[0] << 24 | (uint32_t)in[1] << 16 | (uint32_t)in[2] << 8 | in[3]);
        if (nz <= 0) return false;
        out = (uint32_t)nz;
        n -= 4;
    }
    return (uint64_t)n * 16 < (uint64_t)out * 15;
}

// One LANE per block (route 1 of the split decode): the serial parse of decompress_block with
// 8-byte literal and match copies (an overlapping match with offset < 8 byte by byte, which
// reads only bytes this lane wrote before).  Same corruption checks, never writes past cap.
SDFS_LZ4_HD inline uint32_t decompress_lane(const uint8_t* __restrict__ src, uint32_t n, uint8_t* __restrict__ dst,
                                            uint32_t cap) {
    uint32_t ip = 0, op = 0;
    for (;;) {
        // fast sequence: short literal run (< 15) with its offset inside the next 17 source
        // bytes and room for 16-byte literal / 8-byte-rounded match writes before cap.  The
        // over-written bytes past op are rewritten by the following sequences before anything
        // reads them (a match only reads below its own op).
        if (ip + 17 <= n && op + 16 <= cap) {
            const uint64_t w0 = g64(src + ip), l0 = g64(src + ip + 1), l1 = g64(src + ip + 9);
            const uint32_t token = (uint32_t)w0 & 255u, lit = token >> 4;
            if (lit < kRunMask) {
                __builtin_memcpy(dst + op, &l0, 8);
                __builtin_memcpy(dst + op + 8, &l1, 8);
                // offset bytes at lit, lit + 1 of the 16 loaded after the token
                const uint32_t b0 = lit < 8 ? (uint32_t)(l0 >> (8 * lit)) : (uint32_t)(l1 >> (8 * (lit - 8)));
                const uint32_t b1 = lit + 1 < 8 ? (uint32_t)(l0 >> (8 * (lit + 1))) : (uint32_t)(l1 >> (8 * (lit - 7)));
                const uint32_t off = (b0 & 255u) | ((b1 & 255u) << 8);
                op += lit;
                ip += 3 + lit;
                if (off == 0 || off > op) return kLz4Corrupt;
                uint32_t ml = token & kMlMask;
                if (ml == kMlMask) {
                    uint32_t b;
                    do {
                        if (ip >= n) return kLz4Corrupt;
                        b = src[ip++];
                        ml += b;
                    } while (b == 255);
                }
                ml += kMinMatch;
                if (op + ml > cap) return kLz4Corrupt;
                uint32_t k = 0;
                if (off >= 8) {
                    if (op + ml + 8 <= cap) {  // 8-byte rounded (wild) copy
                        for (; k < ml; k += 8) {
                            const uint64_t v = g64(dst + op - off + k);
                            __builtin_memcpy(dst + op + k, &v, 8);
                        }
                        k = ml;
                    } else {
                        for (; k + 8 <= ml; k += 8) {
                            const uint64_t v = g64(dst + op - off + k);
                            __builtin_memcpy(dst + op + k, &v, 8);
                        }
                    }
                }
                for (; k < ml; k++) dst[op + k] = dst[op - off + k];
                op += ml;
                continue;
            }
        }
        if (ip >= n) return kLz4Corrupt;
        const uint32_t token = src[ip++];
        uint32_t lit = token >> 4;
        if (lit == kRunMask) {
            uint32_t b;
            do {
                if (ip >= n) return kLz4Corrupt;
                b = src[ip++];
                lit += b;
            } while (b == 255);
        }
        if (ip + lit > n || op + lit > cap) return kLz4Corrupt;
        {
            uint32_t k = 0;
            for (; k + 8 <= lit; k += 8) {
                const uint64_t v = g64(src + ip + k);
                __builtin_memcpy(dst + op + k, &v, 8);
            }
            for (; k < lit; k++) dst[op + k] = src[ip + k];
        }
        ip += lit;
        op += lit;
        if (ip == n) return op;
        if (ip + 2 > n) return kLz4Corrupt;
        const uint32_t off = (uint32_t)src[ip] | ((uint32_t)src[ip + 1] << 8);
        ip += 2;
        if (off == 0 || off > op) return kLz4Corrupt;
        uint32_t ml = token & kMlMask;
        if (ml == kMlMask) {
            uint32_t b;
            do {
                if (ip >= n) return kLz4Corrupt;
                b = src[ip++];
                ml += b;
            } while (b == 255);
        }
        ml += kMinMatch;
        if (op + ml > cap) return kLz4Corrupt;
        uint32_t k = 0;
        if (off >= 8) {  // each 8-byte read ends at or before the first byte this step writes
            for (; k + 8 <= ml; k += 8) {
                const uint64_t v = g64(dst + op - off + k);
                __builtin_memcpy(dst + op + k, &v, 8);
            }
        }
        for (; k < ml; k++) dst[op + k] = dst[op - off + k];
        op += ml;
    }
}

}  // namespace sdfs
#endif  // SDFS_LZ4_DECODE_H
