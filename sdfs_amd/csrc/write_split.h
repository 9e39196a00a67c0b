// write_split.h — the request layer of the ranged write (sdfs_cdc_write_split, include/sdfs_write.h)
// in plain C++ with no HIP include, so that a host program can run the same text under
// sanitizers (tests/cpu/write_split_check.cpp).
//
// Reference: DedupFileChannel.writeFile (DedupFileChannel.java:274-359) walks a write buffer by
// buffer (:310-352) and moves the file's length (:355-357); WritableCacheBuffer.write (:523-563)
// applies each cut to its buffer in arrival order, so a later write covers an earlier one.
#ifndef SDFS_WRITE_SPLIT_H
#define SDFS_WRITE_SPLIT_H

#include <algorithm>
#include <climits>
#include <cstdint>
#include <map>
#include <new>
#include <vector>

#include "../../include/sdfs_write.h"

namespace sdfs {

struct WriteCut {
    uint64_t slot, src_off;
    uint32_t start, len, req;
};

struct WriteVisible {  // a visible piece of one row while it is resolved, keyed by its start
    uint32_t end, req;
    uint64_t src_off;
};

// the cuts [c0, c1) of one row, in request order -> its visible pieces, ascending
inline void write_resolve_row(const WriteCut* c0, const WriteCut* c1, std::map<uint32_t, WriteVisible>& vis) {
    vis.clear();
    for (const WriteCut* c = c0; c != c1; ++c) {
        const uint32_t s = c->start, e = c->start + c->len;  // e <= chunk_length < 2^31
        auto it = vis.upper_bound(s);
        if (it != vis.begin()) {
            auto pv = std::prev(it);
            if (pv->second.end > s) {  // the piece before reaches into [s, e): its head stays
                const WriteVisible old = pv->second;
                const uint32_t ps = pv->first;
                if (ps == s) it = vis.erase(pv);
                else pv->second.end = s;
                if (old.end > e) it = vis.emplace(e, WriteVisible{old.end, old.req, old.src_off + (e - ps)}).first;
            }
        }
        while (it != vis.end() && it->first < e) {
            if (it->second.end <= e) {
                it = vis.erase(it);
            } else {  // its tail stays
                const WriteVisible t{it->second.end, it->second.req, it->second.src_off + (e - it->first)};
                vis.erase(it);
                vis.emplace(e, t);
                break;
            }
        }
        vis[s] = WriteVisible{e, c->req, c->src_off};
    }
}

// Returns SDFS_CDC_OK, SDFS_CDC_EINVAL, SDFS_CDC_ECAP or SDFS_CDC_ENOMEM; *why = a static message
// for every code but OK.  The argument rules are those of sdfs_cdc_write_split.
inline int write_split(const sdfs_cdc_read_file* files, uint32_t n_files, const sdfs_cdc_write_request* requests,
                       uint32_t n_requests, uint32_t chunk_length, uint64_t blob_bytes, int64_t* n_written,
                       uint64_t* new_file_len, sdfs_cdc_write_plan* plan, const char** why) {
    const auto fail = [&](int code, const char* msg) {
        *why = msg;
        return code;
    };
    if (!plan) return fail(SDFS_CDC_EINVAL, "null argument");
    plan->n_pieces = plan->n_runs = plan->n_rows = 0;
    if (chunk_length < 1 || chunk_length > (uint32_t)INT32_MAX)
        return fail(SDFS_CDC_EINVAL, "chunk_length: 1 .. 2^31 - 1 (HashLocPair.pos is an int)");
    if ((n_files && (!files || !new_file_len)) || (n_requests && (!requests || !n_written)))
        return fail(SDFS_CDC_EINVAL, "null argument");
    if (plan->piece_cap && (!plan->piece_row || !plan->piece_start || !plan->piece_len || !plan->piece_req ||
                            !plan->piece_src_off))
        return fail(SDFS_CDC_EINVAL, "null argument");
    if (plan->run_cap && (!plan->run_row || !plan->run_pos || !plan->run_len || !plan->run_first_piece ||
                          !plan->run_n_pieces))
        return fail(SDFS_CDC_EINVAL, "null argument");
    if (plan->row_cap && (!plan->row_slot || !plan->row_full)) return fail(SDFS_CDC_EINVAL, "null argument");
    const uint64_t cl = chunk_length;
    for (uint32_t f = 0; f < n_files; f++)
        if (files[f].first_slot > UINT64_MAX - files[f].n_slots)
            return fail(SDFS_CDC_EINVAL, "first_slot + n_slots overflows");

    // pass 1: every rule about a single request, and the number of cuts
    uint64_t n_cuts = 0;
    for (uint32_t r = 0; r < n_requests; r++) {
        const sdfs_cdc_write_request& q = requests[r];
        if (q.file >= n_files) return fail(SDFS_CDC_EINVAL, "request names a file >= n_files");
        if (q.len > (uint64_t)INT64_MAX) return fail(SDFS_CDC_EINVAL, "len > INT64_MAX");
        if (q.src_off > UINT64_MAX - q.len || q.src_off + q.len > blob_bytes)
            return fail(SDFS_CDC_EINVAL, "src_off + len passes blob_bytes");
        if (q.len == 0) continue;
        if (q.file_pos > UINT64_MAX - q.len) return fail(SDFS_CDC_EINVAL, "file_pos + len overflows");
        const uint64_t b0 = q.file_pos / cl, b1 = (q.file_pos + q.len - 1) / cl;
        if (b1 >= files[q.file].n_slots)
            return fail(SDFS_CDC_EINVAL, "a request touches a slot at or past first_slot + n_slots: grow the image first");
        n_cuts += b1 - b0 + 1;
        if (n_cuts >= UINT32_MAX) return fail(SDFS_CDC_EINVAL, "more than 2^32 - 2 pieces: split the batch");
    }

    std::vector<WriteCut> cuts;
    std::vector<WriteCut> pieces;  // visible: slot = the row
    std::vector<uint64_t> slots;
    std::vector<uint8_t> full;
    std::vector<uint32_t> run_row, run_pos, run_len, run_first, run_np;
    std::vector<uint64_t> flen(n_files);
    try {
        // two written files sharing a slot
        std::vector<uint8_t> written(n_files, 0);
        for (uint32_t r = 0; r < n_requests; r++)
            if (requests[r].len) written[(size_t)requests[r].file] = 1;
        std::vector<std::pair<uint64_t, uint64_t>> spans;  // [first, end) of the written files with slots
        for (uint32_t f = 0; f < n_files; f++)
            if (written[f] && files[f].n_slots) spans.emplace_back(files[f].first_slot, files[f].first_slot + files[f].n_slots);
        std::sort(spans.begin(), spans.end());
        for (size_t i = 1; i < spans.size(); i++)
            if (spans[i].first < spans[i - 1].second) return fail(SDFS_CDC_EINVAL, "two written files share a slot");

        for (uint32_t f = 0; f < n_files; f++) flen[f] = files[f].file_len;
        cuts.reserve((size_t)n_cuts);
        for (uint32_t r = 0; r < n_requests; r++) {
            const sdfs_cdc_write_request& q = requests[r];
            if (q.len == 0) continue;
            const sdfs_cdc_read_file& fl = files[q.file];
            flen[(size_t)q.file] = std::max(flen[(size_t)q.file], q.file_pos + q.len);
            uint64_t pos = q.file_pos, src = q.src_off;
            const uint64_t end = pos + q.len;
            while (pos < end) {
                const uint64_t start = pos % cl, len = std::min(cl - start, end - pos);
                cuts.push_back(WriteCut{fl.first_slot + pos / cl, src, (uint32_t)start, (uint32_t)len, r});
                pos += len;
                src += len;
            }
        }
        // row by row, request order kept inside a row
        std::stable_sort(cuts.begin(), cuts.end(), [](const WriteCut& a, const WriteCut& b) { return a.slot < b.slot; });
        std::map<uint32_t, WriteVisible> vis;
        pieces.reserve(cuts.size());
        for (size_t i = 0; i < cuts.size();) {
            size_t j = i + 1;
            while (j < cuts.size() && cuts[j].slot == cuts[i].slot) j++;
            const uint32_t row = (uint32_t)slots.size();
            slots.push_back(cuts[i].slot);
            const size_t p0 = pieces.size();
            if (j == i + 1) {
                pieces.push_back(WriteCut{row, cuts[i].src_off, cuts[i].start, cuts[i].len, cuts[i].req});
            } else {
                write_resolve_row(&cuts[i], &cuts[j], vis);
                for (const auto& kv : vis)
                    pieces.push_back(WriteCut{row, kv.second.src_off, kv.first, kv.second.end - kv.first, kv.second.req});
            }
            if (pieces.size() >= UINT32_MAX) return fail(SDFS_CDC_EINVAL, "more than 2^32 - 2 pieces: split the batch");
            for (size_t p = p0; p < pieces.size(); p++) {
                if (p > p0 && pieces[p - 1].start + pieces[p - 1].len == pieces[p].start) {
                    run_len.back() += pieces[p].len;
                    run_np.back()++;
                } else {
                    run_row.push_back(row);
                    run_pos.push_back(pieces[p].start);
                    run_len.push_back(pieces[p].len);
                    run_first.push_back((uint32_t)p);
                    run_np.push_back(1);
                }
            }
            full.push_back(run_pos.back() == 0 && run_len.back() == chunk_length);  // then it is the row's only run
            i = j;
        }
    } catch (const std::bad_alloc&) {
        return fail(SDFS_CDC_ENOMEM, "out of host memory");
    }
    plan->n_pieces = pieces.size();
    plan->n_runs = run_row.size();
    plan->n_rows = slots.size();
    if (pieces.size() > plan->piece_cap || run_row.size() > plan->run_cap || slots.size() > plan->row_cap)
        return fail(SDFS_CDC_ECAP, "piece_cap, run_cap or row_cap too small");

    for (uint32_t r = 0; r < n_requests; r++) n_written[r] = (int64_t)requests[r].len;
    std::copy(flen.begin(), flen.end(), new_file_len);
    for (size_t p = 0; p < pieces.size(); p++) {
        plan->piece_row[p] = (uint32_t)pieces[p].slot;
        plan->piece_start[p] = pieces[p].start;
        plan->piece_len[p] = pieces[p].len;
        plan->piece_req[p] = pieces[p].req;
        plan->piece_src_off[p] = pieces[p].src_off;
    }
    std::copy(run_row.begin(), run_row.end(), plan->run_row);
    std::copy(run_pos.begin(), run_pos.end(), plan->run_pos);
    std::copy(run_len.begin(), run_len.end(), plan->run_len);
    std::copy(run_first.begin(), run_first.end(), plan->run_first_piece);
    std::copy(run_np.begin(), run_np.end(), plan->run_n_pieces);
    std::copy(slots.begin(), slots.end(), plan->row_slot);
    std::copy(full.begin(), full.end(), plan->row_full);
    return SDFS_CDC_OK;
}

}  // namespace sdfs

#endif  // SDFS_WRITE_SPLIT_H
