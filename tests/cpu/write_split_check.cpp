// write_split_check.cpp — the request layer of the ranged write (sdfs_amd/csrc/write_split.h) as a
// host program, meant to be built with -fsanitize=address,undefined (tests/test_write_ranges.py).
//
// Seeded random batches of overlapping, touching and file-extending requests over several files of
// one image, at chunk_length 67, 1027 and 4096, against byte painting: every byte of a buffer
// remembers the last request that wrote it and its place in the blob; pieces, runs and row_full are
// read off the painted buffers.  The output arrays are heap blocks of exactly the reported sizes,
// so that a write past them is a sanitizer report.  Also: too little room reports the counts and
// writes nothing, and the argument refusals.  Prints OK at the end.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "../../sdfs_amd/csrc/write_split.h"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // xorshift64*
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    return g_state * 0x2545F4914F6CDD1Dull;
}
uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            std::exit(1);                                                     \
        }                                                                     \
    } while (0)

struct Piece {
    uint64_t slot, src;
    uint32_t start, len, req;
};
struct Run {
    uint64_t slot;
    uint32_t pos, len, first, n;
};

struct Plan {  // heap arrays of exactly the given sizes
    sdfs_cdc_write_plan p{};
    Plan(uint32_t pc, uint32_t rc, uint32_t wc) {
        p.piece_cap = pc, p.run_cap = rc, p.row_cap = wc;
        p.piece_row = new uint32_t[pc], p.piece_start = new uint32_t[pc], p.piece_len = new uint32_t[pc];
        p.piece_req = new uint32_t[pc], p.piece_src_off = new uint64_t[pc];
        p.run_row = new uint32_t[rc], p.run_pos = new uint32_t[rc], p.run_len = new uint32_t[rc];
        p.run_first_piece = new uint32_t[rc], p.run_n_pieces = new uint32_t[rc];
        p.row_slot = new uint64_t[wc], p.row_full = new uint8_t[wc];
    }
    ~Plan() {
        delete[] p.piece_row, delete[] p.piece_start, delete[] p.piece_len, delete[] p.piece_req;
        delete[] p.piece_src_off, delete[] p.run_row, delete[] p.run_pos, delete[] p.run_len;
        delete[] p.run_first_piece, delete[] p.run_n_pieces, delete[] p.row_slot, delete[] p.row_full;
    }
};

void run_batch(uint32_t cl, uint32_t n_req, uint64_t max_len) {
    std::vector<sdfs_cdc_read_file> files;
    uint64_t first = below(5);
    const uint32_t n_files = 1 + (uint32_t)below(3);
    for (uint32_t f = 0; f < n_files; f++) {
        const uint64_t n_slots = 1 + below(6);
        files.push_back(sdfs_cdc_read_file{first, n_slots, below(n_slots * cl + 1)});
        first += n_slots + below(3);
        if (below(4) == 0) first += (uint64_t)1 << (12 + below(40));
    }
    const uint64_t blob = 4 * max_len + 64;
    std::vector<sdfs_cdc_write_request> reqs;
    for (uint32_t r = 0; r < n_req; r++) {
        const uint64_t f = below(n_files), room = files[f].n_slots * cl;
        uint64_t pos = below(room), len = below(4) ? below(max_len + 1) : below(40);
        if (below(6) == 0) pos = pos / cl * cl;
        if (below(8) == 0) len = (pos / cl + 1 + below(2)) * cl - pos;
        if (!reqs.empty() && below(4) == 0 && reqs.back().file == f) pos = reqs.back().file_pos + reqs.back().len;  // touching
        if (pos >= room) pos = room - 1;
        if (len > room - pos) len = room - pos;
        if (len > blob) len = blob;
        reqs.push_back(sdfs_cdc_write_request{f, pos, len, below(blob - len + 1)});
    }
    // painting
    std::map<uint64_t, std::vector<std::pair<int64_t, uint64_t>>> painted;
    std::vector<uint64_t> want_len;
    for (const auto& f : files) want_len.push_back(f.file_len);
    for (uint32_t r = 0; r < n_req; r++) {
        const sdfs_cdc_write_request& q = reqs[r];
        if (q.len && q.file_pos + q.len > want_len[q.file]) want_len[q.file] = q.file_pos + q.len;
        for (uint64_t i = 0; i < q.len; i++) {
            const uint64_t pos = q.file_pos + i;
            auto& row = painted[files[q.file].first_slot + pos / cl];
            if (row.empty()) row.assign(cl, {-1, 0});
            row[pos % cl] = {(int64_t)r, q.src_off + i};
        }
    }
    std::vector<Piece> want;
    std::vector<Run> runs;
    std::vector<uint64_t> rows;
    std::vector<uint8_t> full;
    for (const auto& kv : painted) {
        const auto& row = kv.second;
        rows.push_back(kv.first);
        bool all = true;
        int64_t prev_end = -1;
        for (uint32_t i = 0; i < cl;) {
            if (row[i].first < 0) {
                all = false;
                i++;
                continue;
            }
            uint32_t j = i + 1;
            while (j < cl && row[j].first == row[i].first && row[j].second == row[j - 1].second + 1) j++;
            if (prev_end == (int64_t)i) {
                runs.back().len += j - i;
                runs.back().n++;
            } else {
                runs.push_back(Run{kv.first, i, j - i, (uint32_t)want.size(), 1});
            }
            want.push_back(Piece{kv.first, row[i].second, i, j - i, (uint32_t)row[i].first});
            prev_end = j;
            i = j;
        }
        full.push_back(all);
    }
    const char* why = nullptr;
    const uint32_t pc = (uint32_t)want.size(), rc = (uint32_t)runs.size(), wc = (uint32_t)rows.size();
    int64_t* nw = new int64_t[n_req];
    uint64_t* fl = new uint64_t[n_files];
    {  // too little room: the counts, nothing written
        sdfs_cdc_write_plan none{};
        const int rcode = sdfs::write_split(files.data(), n_files, reqs.data(), n_req, cl, blob, nw, fl, &none, &why);
        CHECK(rcode == (want.empty() ? SDFS_CDC_OK : SDFS_CDC_ECAP));
        CHECK(none.n_pieces == pc && none.n_runs == rc && none.n_rows == wc);
    }
    Plan P(pc, rc, wc);
    CHECK(sdfs::write_split(files.data(), n_files, reqs.data(), n_req, cl, blob, nw, fl, &P.p, &why) == SDFS_CDC_OK);
    const sdfs_cdc_write_plan& p = P.p;
    CHECK(p.n_pieces == pc && p.n_runs == rc && p.n_rows == wc);
    for (uint32_t r = 0; r < n_req; r++) CHECK(nw[r] == (int64_t)reqs[r].len);
    for (uint32_t f = 0; f < n_files; f++) CHECK(fl[f] == want_len[f]);
    for (uint32_t i = 0; i < wc; i++) CHECK(p.row_slot[i] == rows[i] && p.row_full[i] == full[i]);
    for (uint32_t i = 0; i < pc; i++) {
        const Piece& w = want[i];
        CHECK(p.piece_row[i] < wc && p.row_slot[p.piece_row[i]] == w.slot);
        CHECK(p.piece_start[i] == w.start && p.piece_len[i] == w.len && p.piece_req[i] == w.req && p.piece_src_off[i] == w.src);
    }
    for (uint32_t i = 0; i < rc; i++) {
        const Run& w = runs[i];
        CHECK(p.row_slot[p.run_row[i]] == w.slot && p.run_pos[i] == w.pos && p.run_len[i] == w.len);
        CHECK(p.run_first_piece[i] == w.first && p.run_n_pieces[i] == w.n);
    }
    if (pc > 1) {  // one entry short
        Plan S(pc - 1, rc, wc);
        CHECK(sdfs::write_split(files.data(), n_files, reqs.data(), n_req, cl, blob, nw, fl, &S.p, &why) == SDFS_CDC_ECAP);
        CHECK(S.p.n_pieces == pc && S.p.n_runs == rc && S.p.n_rows == wc);
    }
    if (rc > 1) {
        Plan S(pc, rc - 1, wc);
        CHECK(sdfs::write_split(files.data(), n_files, reqs.data(), n_req, cl, blob, nw, fl, &S.p, &why) == SDFS_CDC_ECAP);
    }
    if (wc > 1) {
        Plan S(pc, rc, wc - 1);
        CHECK(sdfs::write_split(files.data(), n_files, reqs.data(), n_req, cl, blob, nw, fl, &S.p, &why) == SDFS_CDC_ECAP);
    }
    delete[] nw;
    delete[] fl;
}

void refusals() {
    const char* why = nullptr;
    int64_t nw[2];
    uint64_t fl[2];
    Plan P(8, 8, 8);
    sdfs_cdc_read_file f[2] = {{0, 4, 100}, {4, 4, 0}};
    sdfs_cdc_write_request q[2] = {{0, 0, 10, 0}, {1, 0, 0, 0}};
    const auto call = [&](uint32_t cl, uint64_t blob) { return sdfs::write_split(f, 2, q, 2, cl, blob, nw, fl, &P.p, &why); };
    CHECK(call(1000, 64) == SDFS_CDC_OK && P.p.n_pieces == 1 && P.p.n_rows == 1 && nw[0] == 10 && nw[1] == 0 && fl[0] == 100);
    CHECK(call(0, 64) == SDFS_CDC_EINVAL && why);
    CHECK(call(0x80000000u, 64) == SDFS_CDC_EINVAL);
    CHECK(call(1000, 9) == SDFS_CDC_EINVAL);  // src_off + len passes the blob
    q[0].file = 2;
    CHECK(call(1000, 64) == SDFS_CDC_EINVAL);
    q[0] = sdfs_cdc_write_request{0, 3999, 2, 0};  // the second byte needs slot 4 of a file of 4
    CHECK(call(1000, 64) == SDFS_CDC_EINVAL);
    q[0] = sdfs_cdc_write_request{0, 3999, 1, 0};
    CHECK(call(1000, 64) == SDFS_CDC_OK && fl[0] == 4000);
    q[0] = sdfs_cdc_write_request{0, UINT64_MAX - 3, 10, 0};
    CHECK(call(1000, 64) == SDFS_CDC_EINVAL);
    q[0] = sdfs_cdc_write_request{0, 0, 10, UINT64_MAX - 3};
    CHECK(call(1000, UINT64_MAX) == SDFS_CDC_EINVAL);
    q[0] = sdfs_cdc_write_request{0, 0, 10, 0};
    q[1] = sdfs_cdc_write_request{1, 5, 1, 20};
    CHECK(call(1000, 64) == SDFS_CDC_OK && P.p.n_rows == 2 && fl[1] == 6);
    f[1].first_slot = 3;  // both files written, slot 3 shared
    CHECK(call(1000, 64) == SDFS_CDC_EINVAL);
    q[1].len = 0;  // the second file is no longer written
    CHECK(call(1000, 64) == SDFS_CDC_OK);
    f[1] = sdfs_cdc_read_file{UINT64_MAX - 2, 4, 0};
    CHECK(call(1000, 64) == SDFS_CDC_EINVAL);
    f[1] = sdfs_cdc_read_file{4, 4, 0};
    // more pieces than a 32-bit index holds
    sdfs_cdc_read_file big{0, UINT64_MAX / 2, 0};
    sdfs_cdc_write_request huge{0, 0, (uint64_t)1 << 33, 0};
    CHECK(sdfs::write_split(&big, 1, &huge, 1, 1, UINT64_MAX, nw, fl, &P.p, &why) == SDFS_CDC_EINVAL);
    CHECK(sdfs::write_split(f, 2, q, 2, 1000, 64, nw, fl, nullptr, &why) == SDFS_CDC_EINVAL);
    CHECK(sdfs::write_split(nullptr, 2, q, 2, 1000, 64, nw, fl, &P.p, &why) == SDFS_CDC_EINVAL);
    CHECK(sdfs::write_split(nullptr, 0, nullptr, 0, 1000, 0, nullptr, nullptr, &P.p, &why) == SDFS_CDC_OK && P.p.n_pieces == 0);
}

}  // namespace

int main() {
    refusals();
    for (int i = 0; i < 200; i++) run_batch(67, 1 + (uint32_t)below(40), 3 * 67);
    for (int i = 0; i < 100; i++) run_batch(1027, 1 + (uint32_t)below(40), 2 * 1027);
    for (int i = 0; i < 50; i++) run_batch(4096, 1 + (uint32_t)below(20), 3 * 4096);
    for (int i = 0; i < 20; i++) run_batch(1, 5, 4);
    run_batch(1027, 0, 0);
    std::printf("OK\n");
    return 0;
}
