// read_split_check.cpp — the request layer of the ranged read (sdfs_amd/csrc/read_split.h) as a
// host program, meant to be built with -fsanitize=address,undefined (tests/test_read_ranges.py).
//
// Seeded random batches of requests over several files of one image, at chunk_length 1027 and
// 262144, against a byte-at-a-time restatement of DedupFileChannel.read's walk: every byte of a
// request is visited, a piece begins at the request's first byte and at every byte whose position
// is a multiple of chunk_length.  The output arrays are heap blocks of exactly the reported sizes,
// so that a write past them is a sanitizer report.  Also: too little room reports the counts and
// writes nothing, and the argument refusals.  Prints OK at the end.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../../sdfs_amd/csrc/read_split.h"

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
    uint32_t req;
    uint64_t slot;  // UINT64_MAX: past the map
    uint32_t start, len;
    uint64_t out_off;
};

void naive(const std::vector<sdfs_cdc_read_file>& files, const std::vector<sdfs_cdc_read_request>& reqs, uint64_t cl,
           std::vector<int64_t>& n_read, std::vector<Piece>& pieces, std::set<uint64_t>& slots) {
    for (uint32_t r = 0; r < reqs.size(); r++) {
        const sdfs_cdc_read_request& q = reqs[r];
        const sdfs_cdc_read_file& f = files[q.file];
        if (q.file_pos >= f.file_len) {
            n_read.push_back(-1);
            continue;
        }
        uint64_t n = 0;
        for (uint64_t i = 0; i < q.siz && q.file_pos + i < f.file_len; i++) {  // byte by byte
            const uint64_t pos = q.file_pos + i;
            if (i == 0 || pos % cl == 0) {
                const uint64_t b = pos / cl;
                pieces.push_back(Piece{r, b < f.n_slots ? f.first_slot + b : UINT64_MAX, (uint32_t)(pos % cl), 0,
                                       q.out_off + i});
                if (b < f.n_slots) slots.insert(f.first_slot + b);
            }
            pieces.back().len++;
            n++;
        }
        n_read.push_back((int64_t)n);
    }
}

void run_batch(uint32_t cl, uint32_t n_req, uint64_t max_siz) {
    std::vector<sdfs_cdc_read_file> files;
    uint64_t first = below(5);
    const uint32_t n_files = 1 + (uint32_t)below(4);
    for (uint32_t f = 0; f < n_files; f++) {
        const uint64_t n_slots = below(7);
        uint64_t len = n_slots * cl;
        switch (below(4)) {
        case 0: break;                                   // ends on a buffer boundary
        case 1: len = len ? len - 1 - below(cl) : 0; break;  // ends in mid-buffer
        case 2: len += 1 + below(3 * (uint64_t)cl); break;   // longer than its map
        default: len = below(len + 2); break;
        }
        files.push_back(sdfs_cdc_read_file{first, n_slots, len});
        first += below(3) ? n_slots : below(n_slots + 1);  // some files share slots
        if (below(3) == 0) first += (uint64_t)1 << (12 + below(40));  // and some lie far apart in the image
    }
    std::vector<sdfs_cdc_read_request> reqs;
    uint64_t out = below(16);
    for (uint32_t r = 0; r < n_req; r++) {
        const uint64_t f = below(n_files);
        const uint64_t len = files[f].file_len;
        uint64_t pos = below(len + cl);
        if (below(8) == 0) pos = len;
        if (below(8) == 0 && len) pos = len - 1;
        if (below(6) == 0) pos = pos / cl * cl;
        uint64_t siz = below(4) ? below(max_siz + 1) : below(40);
        if (below(8) == 0) siz = (pos / cl + 1 + below(3)) * cl - pos;  // ends exactly on a boundary
        reqs.push_back(sdfs_cdc_read_request{f, pos, siz, out});
        out += siz + below(3);
    }
    std::vector<int64_t> want_n;
    std::vector<Piece> want;
    std::set<uint64_t> want_slots;
    naive(files, reqs, cl, want_n, want, want_slots);
    const std::vector<uint64_t> rows(want_slots.begin(), want_slots.end());

    const char* why = nullptr;
    uint64_t np = 99, nr = 99;
    // too little room: the counts, nothing written
    int rc;
    if (n_req) {
        int64_t* nrd = new int64_t[n_req];
        rc = sdfs::read_split(files.data(), n_files, reqs.data(), n_req, cl, nrd, 0, nullptr, nullptr, nullptr, nullptr,
                              nullptr, 0, nullptr, &np, &nr, &why);
        CHECK(rc == (want.empty() ? SDFS_CDC_OK : SDFS_CDC_ECAP));
        CHECK(np == want.size() && nr == rows.size());
        delete[] nrd;
    }
    // exact room
    const uint32_t pc = (uint32_t)want.size(), rcap = (uint32_t)rows.size();
    int64_t* nrd = new int64_t[n_req];
    uint32_t *p_req = new uint32_t[pc], *p_row = new uint32_t[pc], *p_start = new uint32_t[pc], *p_len = new uint32_t[pc];
    uint64_t *p_out = new uint64_t[pc], *row_slot = new uint64_t[rcap];
    rc = sdfs::read_split(files.data(), n_files, reqs.data(), n_req, cl, nrd, pc, p_req, p_row, p_start, p_len, p_out,
                          rcap, row_slot, &np, &nr, &why);
    CHECK(rc == SDFS_CDC_OK);
    CHECK(np == want.size() && nr == rows.size());
    for (uint32_t r = 0; r < n_req; r++) CHECK(nrd[r] == want_n[r]);
    for (uint32_t i = 0; i < rcap; i++) CHECK(row_slot[i] == rows[i]);
    uint64_t sum = 0;
    for (uint32_t p = 0; p < pc; p++) {
        const Piece& w = want[p];
        CHECK(p_req[p] == w.req && p_start[p] == w.start && p_len[p] == w.len && p_out[p] == w.out_off);
        CHECK((uint64_t)p_start[p] + p_len[p] <= cl && p_len[p] >= 1);
        if (w.slot == UINT64_MAX) CHECK(p_row[p] == SDFS_CDC_READ_NONE);
        else CHECK(p_row[p] < rcap && row_slot[p_row[p]] == w.slot);
        sum += p_len[p];
    }
    uint64_t total = 0, bound = 0;
    for (uint32_t r = 0; r < n_req; r++) {
        total += nrd[r] > 0 ? (uint64_t)nrd[r] : 0;
        bound += reqs[r].siz / cl + 2;
    }
    CHECK(sum == total && pc <= bound && rcap <= pc);
    if (pc > 1) {  // one entry short on either side
        rc = sdfs::read_split(files.data(), n_files, reqs.data(), n_req, cl, nrd, pc - 1, p_req, p_row, p_start, p_len,
                              p_out, rcap, row_slot, &np, &nr, &why);
        CHECK(rc == SDFS_CDC_ECAP && np == pc && nr == rcap);
    }
    if (rcap > 0) {
        rc = sdfs::read_split(files.data(), n_files, reqs.data(), n_req, cl, nrd, pc, p_req, p_row, p_start, p_len, p_out,
                              rcap - 1, row_slot, &np, &nr, &why);
        CHECK(rc == SDFS_CDC_ECAP && np == pc && nr == rcap);
    }
    delete[] nrd;
    delete[] p_req;
    delete[] p_row;
    delete[] p_start;
    delete[] p_len;
    delete[] p_out;
    delete[] row_slot;
}

void refusals() {
    const char* why = nullptr;
    uint64_t np = 0, nr = 0;
    int64_t nrd[1];
    uint32_t u[4][4];
    uint64_t o[4], rows[4];
    sdfs_cdc_read_file f{0, 4, 4000};
    sdfs_cdc_read_request q{0, 0, 10, 0};
    const auto call = [&](uint32_t cl) {
        return sdfs::read_split(&f, 1, &q, 1, cl, nrd, 4, u[0], u[1], u[2], u[3], o, 4, rows, &np, &nr, &why);
    };
    CHECK(call(1000) == SDFS_CDC_OK && np == 1 && nr == 1 && nrd[0] == 10);
    CHECK(call(0) == SDFS_CDC_EINVAL && why);
    CHECK(call(0x80000000u) == SDFS_CDC_EINVAL);
    q.file = 1;
    CHECK(call(1000) == SDFS_CDC_EINVAL);
    q = sdfs_cdc_read_request{0, 0, UINT64_MAX, 0};
    CHECK(call(1000) == SDFS_CDC_EINVAL);
    q = sdfs_cdc_read_request{0, 0, 10, UINT64_MAX - 3};
    CHECK(call(1000) == SDFS_CDC_EINVAL);
    q = sdfs_cdc_read_request{0, 0, 10, UINT64_MAX - 10};  // the last byte lands on UINT64_MAX - 1
    CHECK(call(1000) == SDFS_CDC_OK);
    q = sdfs_cdc_read_request{0, 0, 10, 0};
    f = sdfs_cdc_read_file{UINT64_MAX - 2, 4, 4000};
    CHECK(call(1000) == SDFS_CDC_EINVAL);
    // positions near 2^64: a file of the largest length, read at its very end
    f = sdfs_cdc_read_file{0, 0, UINT64_MAX};
    q = sdfs_cdc_read_request{0, UINT64_MAX - 5, 100, 0};
    CHECK(call(1000) == SDFS_CDC_OK && nrd[0] == 5 && np <= 2 && nr == 0);
    q = sdfs_cdc_read_request{0, UINT64_MAX, 100, 0};
    CHECK(call(1000) == SDFS_CDC_OK && nrd[0] == -1 && np == 0);
    // more pieces than a 32-bit index holds
    q = sdfs_cdc_read_request{0, 0, (uint64_t)INT64_MAX, 0};
    CHECK(call(1) == SDFS_CDC_EINVAL);
    CHECK(sdfs::read_split(&f, 1, &q, 1, 1000, nrd, 4, u[0], u[1], u[2], u[3], o, 4, rows, nullptr, &nr, &why) ==
          SDFS_CDC_EINVAL);
    CHECK(sdfs::read_split(nullptr, 1, &q, 1, 1000, nrd, 4, u[0], u[1], u[2], u[3], o, 4, rows, &np, &nr, &why) ==
          SDFS_CDC_EINVAL);
    CHECK(sdfs::read_split(&f, 1, &q, 1, 1000, nrd, 4, u[0], nullptr, u[2], u[3], o, 4, rows, &np, &nr, &why) ==
          SDFS_CDC_EINVAL);
    CHECK(sdfs::read_split(nullptr, 0, nullptr, 0, 1000, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                           nullptr, &np, &nr, &why) == SDFS_CDC_OK && np == 0 && nr == 0);
}

}  // namespace

int main() {
    refusals();
    for (int i = 0; i < 100; i++) run_batch(1027, 20, 4 * 1027);      // 2 000 requests
    for (int i = 0; i < 100; i++) run_batch(262144, 20, 131072);      // FUSE-sized pieces
    for (int i = 0; i < 10; i++) run_batch(262144, 10, 3 * 262144);   // several buffers each
    for (int i = 0; i < 20; i++) run_batch(1, 5, 40);                 // the smallest chunk_length
    run_batch(1027, 0, 0);
    std::printf("OK\n");
    return 0;
}
