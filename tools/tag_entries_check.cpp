// tag_entries_check.cpp -- tag_entries_host (csrc/tag_entries.cpp: the host statement of the tag kernels' contract and the second
// route of gft_group_tag_records) under the address and undefined-behaviour sanitizers: a stand-alone program, CPU only.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I. tools/tag_entries_check.cpp \
//       gofindthem_amd/csrc/tag_entries.cpp -o build/tag_entries_check
//   build/tag_entries_check 2000 1
//
// N seeded batches; every array -- hit rows, fields, offsets, the validity mask, the expressions' tags and the outputs -- lies in
// a heap block of exactly its size, so that a read or a store past an end is an error of the sanitizer.  Every batch runs with
// caps 0, 1, total - 1, total and total + 7 (the arrays then have exactly `cap` elements) and is compared with a restatement
// that builds the lists with vectors.  Exit code 0: all agree.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "gofindthem_amd/csrc/tag_entries.hpp"

using namespace gft;

namespace {

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size()]);
    if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
    return p;
}

struct Batch {
    uint32_t n_exprs = 0, n_fields = 0;
    std::vector<uint32_t> valid, expr_tag, hit, field;
    std::vector<uint64_t> rec_off;
};

Batch make(std::mt19937_64& rng) {
    static const uint32_t kE[] = {0, 1, 31, 32, 33, 64, 65, 200, 2049}, kF[] = {1, 31, 32, 33, 65};
    Batch b;
    b.n_exprs = kE[rng() % 9];
    b.n_fields = kF[rng() % 5];
    const uint32_t EW = (b.n_exprs + 31) / 32, FW = (b.n_fields + 31) / 32;
    const unsigned valid_mode = rng() % 4;                // all, none, about half, all but the word borders
    b.valid.assign(FW, 0);
    for (uint32_t f = 0; f < b.n_fields; f++) {
        const bool ok = valid_mode == 0 || (valid_mode == 2 && (rng() & 1)) || (valid_mode == 3 && f != 31 && f != 32);
        if (ok) b.valid[f >> 5] |= 1u << (f & 31);
    }
    for (uint32_t e = 0; e < b.n_exprs; e++) b.expr_tag.push_back((uint32_t)(rng() % 7));
    const uint64_t n_records = rng() % 9;
    b.rec_off.push_back(0);
    for (uint64_t r = 0; r < n_records; r++) b.rec_off.push_back(b.rec_off.back() + (rng() % 3 ? rng() % 5 : 0));
    const uint64_t n_leaves = b.rec_off.back();
    const unsigned density = rng() % 4;                   // empty, sparse, half, every bit (garbage above n_exprs included)
    for (uint64_t l = 0; l < n_leaves; l++) {
        b.field.push_back((uint32_t)(rng() % b.n_fields));
        for (uint32_t w = 0; w < EW; w++) {
            const uint32_t x = (uint32_t)rng(), y = (uint32_t)rng();
            b.hit.push_back(density == 0 ? 0u : density == 1 ? (x & y & (uint32_t)rng()) : density == 2 ? x : 0xFFFFFFFFu);
        }
    }
    return b;
}

bool check(const Batch& b, uint64_t& entries) {
    const uint64_t n_records = b.rec_off.size() - 1, n_leaves = b.field.size();
    const uint32_t EW = (b.n_exprs + 31) / 32;
    // the restatement
    std::vector<uint64_t> want_off;
    std::vector<uint32_t> want_field, want_expr, want_tag;
    for (uint64_t r = 0; r < n_records; r++) {
        want_off.push_back(want_expr.size());
        for (uint64_t l = b.rec_off[r]; l < b.rec_off[r + 1]; l++) {
            const uint32_t f = b.field[l];
            if (!((b.valid[f / 32] >> (f % 32)) & 1)) continue;
            for (uint32_t e = 0; e < b.n_exprs; e++)
                if ((b.hit[l * EW + e / 32] >> (e % 32)) & 1) { want_field.push_back(f); want_expr.push_back(e); want_tag.push_back(b.expr_tag[e]); }
        }
    }
    want_off.push_back(want_expr.size());
    const uint64_t total = want_expr.size();
    entries += total;
    RuleSet rs;
    rs.n_fields = b.n_fields; rs.n_exprs = b.n_exprs; rs.field_words = (b.n_fields + 31) / 32;
    rs.valid = b.valid; rs.expr_tag = b.expr_tag;
    rs.valid.shrink_to_fit(); rs.expr_tag.shrink_to_fit();
    auto hit = exact(b.hit);
    auto field = exact(b.field);
    auto rec_off = exact(b.rec_off);
    const uint64_t caps[5] = {0, 1, total ? total - 1 : 0, total, total + 7};
    for (uint64_t cap : caps)
        for (int with_tag = 0; with_tag < 2; with_tag++) {
            std::unique_ptr<uint64_t[]> row_off(new uint64_t[n_records + 1]);
            std::unique_ptr<uint32_t[]> ef(new uint32_t[cap]), ee(new uint32_t[cap]), et(new uint32_t[cap]);
            for (uint64_t k = 0; k < cap; k++) ef[k] = ee[k] = et[k] = 0xA5A5A5A5u;
            uint64_t got_total = ~0ull;
            tag_entries_host(rs, hit.get(), b.n_exprs, field.get(), rec_off.get(), n_records, n_leaves, row_off.get(), cap ? ef.get() : nullptr,
                             cap ? ee.get() : nullptr, with_tag && cap ? et.get() : nullptr, cap, &got_total);
            if (got_total != total || memcmp(row_off.get(), want_off.data(), (n_records + 1) * 8)) return false;
            for (uint64_t k = 0; k < cap; k++) {
                const bool stored = k < total;
                if (ef[k] != (stored ? want_field[k] : 0xA5A5A5A5u) || ee[k] != (stored ? want_expr[k] : 0xA5A5A5A5u)) return false;
                if (et[k] != (stored && with_tag ? want_tag[k] : 0xA5A5A5A5u)) return false;
            }
        }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 2000;
    std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
    uint64_t entries = 0, empty = 0;
    for (uint64_t i = 0; i < n; i++) {
        const Batch b = make(rng);
        const uint64_t before = entries;
        if (!check(b, entries)) { fprintf(stderr, "batch %llu: tag_entries_host disagrees with the restatement\n", (unsigned long long)i); return 1; }
        empty += entries == before;
    }
    printf("tag_entries_check: %llu batches, %llu entries, %llu batches without an entry: ok\n", (unsigned long long)n, (unsigned long long)entries,
           (unsigned long long)empty);
    return entries && empty && empty < n ? 0 : 2;          // (a run that never produced an entry, or always did, checked too little)
}
