// read_split.h — the request layer of the ranged read (sdfs_cdc_read_split, include/sdfs_read.h)
// in plain C++ with no HIP include, so that a host program can run the same text under
// sanitizers (tests/cpu/read_split_check.cpp).
//
// Reference: DedupFileChannel.read (DedupFileChannel.java:499-608) clips a request at the file's
// length (-1 at or past it) and walks it buffer by buffer; WritableCacheBuffer.readChunk
// (:217-245) hands out [startPos, startPos + len) of each.  A buffer past the end of the map is a
// fresh blank one.
#ifndef SDFS_READ_SPLIT_H
#define SDFS_READ_SPLIT_H

#include <algorithm>
#include <climits>
#include <cstdint>
#include <new>
#include <vector>

#include "../../include/sdfs_read.h"

namespace sdfs {

// Returns SDFS_CDC_OK, SDFS_CDC_EINVAL, SDFS_CDC_ECAP or SDFS_CDC_ENOMEM; *why = a static message
// for every code but OK.  The argument rules are those of sdfs_cdc_read_split.
inline int read_split(const sdfs_cdc_read_file* files, uint32_t n_files, const sdfs_cdc_read_request* requests,
                      uint32_t n_requests, uint32_t chunk_length, int64_t* n_read, uint32_t piece_cap,
                      uint32_t* piece_req, uint32_t* piece_row, uint32_t* piece_start, uint32_t* piece_len,
                      uint64_t* piece_out_off, uint32_t row_cap, uint64_t* row_slot, uint64_t* n_pieces,
                      uint64_t* n_rows, const char** why) {
    const auto fail = [&](int code, const char* msg) {
        *why = msg;
        return code;
    };
    if (!n_pieces || !n_rows) return fail(SDFS_CDC_EINVAL, "null argument");
    *n_pieces = *n_rows = 0;
    if (chunk_length < 1 || chunk_length > (uint32_t)INT32_MAX)
        return fail(SDFS_CDC_EINVAL, "chunk_length: 1 .. 2^31 - 1 (HashLocPair.pos is an int)");
    if ((n_files && !files) || (n_requests && (!requests || !n_read))) return fail(SDFS_CDC_EINVAL, "null argument");
    if (piece_cap && (!piece_req || !piece_row || !piece_start || !piece_len || !piece_out_off))
        return fail(SDFS_CDC_EINVAL, "null argument");
    if (row_cap && !row_slot) return fail(SDFS_CDC_EINVAL, "null argument");
    const uint64_t cl = chunk_length;
    for (uint32_t f = 0; f < n_files; f++)
        if (files[f].first_slot > UINT64_MAX - files[f].n_slots)
            return fail(SDFS_CDC_EINVAL, "first_slot + n_slots overflows");

    // pass 1: the counts, and the touched slots
    uint64_t np = 0;
    std::vector<uint64_t> slots;     // touched, then distinct and ascending: the rows
    std::vector<uint32_t> row_of;    // dense case: slot - lo -> row
    uint64_t lo = UINT64_MAX, hi = 0;
    try {
        slots.reserve((size_t)n_requests * 2);
        for (uint32_t r = 0; r < n_requests; r++) {
            const sdfs_cdc_read_request& q = requests[r];
            if (q.file >= n_files) return fail(SDFS_CDC_EINVAL, "request names a file >= n_files");
            if (q.siz > (uint64_t)INT64_MAX) return fail(SDFS_CDC_EINVAL, "siz > INT64_MAX");
            const sdfs_cdc_read_file& fl = files[q.file];
            if (q.file_pos >= fl.file_len) continue;
            const uint64_t n = std::min(q.siz, fl.file_len - q.file_pos);
            if (n == 0) continue;
            if (q.out_off > UINT64_MAX - n) return fail(SDFS_CDC_EINVAL, "out_off + n_read overflows");
            const uint64_t b0 = q.file_pos / cl, b1 = (q.file_pos + n - 1) / cl;  // file_pos + n <= file_len
            np += b1 - b0 + 1;
            if (np >= UINT32_MAX) return fail(SDFS_CDC_EINVAL, "more than 2^32 - 2 pieces: split the batch");
            for (uint64_t b = b0; b <= b1 && b < fl.n_slots; b++) slots.push_back(fl.first_slot + b);
        }
        for (const uint64_t v : slots) {
            lo = std::min(lo, v);
            hi = std::max(hi, v);
        }
        if (!slots.empty() && hi - lo < 8 * (uint64_t)slots.size() + 1024) {
            // the touched slots lie close together (one image): a table over [lo, hi], no sort
            row_of.assign((size_t)(hi - lo + 1), SDFS_CDC_READ_NONE);
            for (const uint64_t v : slots) row_of[(size_t)(v - lo)] = 0;
            slots.clear();
            for (size_t i = 0; i < row_of.size(); i++)
                if (row_of[i] == 0) {
                    row_of[i] = (uint32_t)slots.size();
                    slots.push_back(lo + i);
                }
        } else {
            std::sort(slots.begin(), slots.end());
            slots.erase(std::unique(slots.begin(), slots.end()), slots.end());
        }
    } catch (const std::bad_alloc&) {
        return fail(SDFS_CDC_ENOMEM, "out of host memory");
    }
    *n_pieces = np;
    *n_rows = slots.size();
    if (np > piece_cap || slots.size() > row_cap) return fail(SDFS_CDC_ECAP, "piece_cap or row_cap too small");

    // pass 2: the outputs
    std::copy(slots.begin(), slots.end(), row_slot);
    uint32_t p = 0;
    for (uint32_t r = 0; r < n_requests; r++) {
        const sdfs_cdc_read_request& q = requests[r];
        const sdfs_cdc_read_file& fl = files[q.file];
        if (q.file_pos >= fl.file_len) {
            n_read[r] = -1;
            continue;
        }
        const uint64_t n = std::min(q.siz, fl.file_len - q.file_pos);
        n_read[r] = (int64_t)n;
        uint64_t pos = q.file_pos, out = q.out_off;
        const uint64_t end = pos + n;
        while (pos < end) {
            const uint64_t b = pos / cl, start = pos % cl;
            const uint64_t len = std::min(cl - start, end - pos);
            piece_req[p] = r;
            piece_row[p] = SDFS_CDC_READ_NONE;
            if (b < fl.n_slots)
                piece_row[p] = !row_of.empty() ? row_of[(size_t)(fl.first_slot + b - lo)]
                                               : (uint32_t)(std::lower_bound(slots.begin(), slots.end(), fl.first_slot + b) -
                                                            slots.begin());
            piece_start[p] = (uint32_t)start;
            piece_len[p] = (uint32_t)len;
            piece_out_off[p] = out;
            p++;
            pos += len;
            out += len;
        }
    }
    return SDFS_CDC_OK;
}

}  // namespace sdfs

#endif  // SDFS_READ_SPLIT_H
