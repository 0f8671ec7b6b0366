// stats_host.cpp -- gft_term_stats_device's and gft_count_columns_device's walks on the host (gft_stats.hpp): the check, then the
// count pass workgroup by workgroup, step by step and lane by lane through gft_stats_piece.hpp, with the step's set, the large
// path's bitset and the workgroup's cache as arrays and the phases of a step one after the other.  No HIP.
#include <algorithm>
#include <vector>

#include "../../include/gft.h"
#include "gft_stats.hpp"

namespace gft {

namespace {

constexpr uint64_t kNoDoc = ~0ull;
constexpr uint64_t kHostResident = 768;     // workgroups the host walk cuts a list into at most

struct Out {
    uint64_t* occ;
    uint64_t* docs;
    uint64_t* first;
    void add(uint32_t t, uint64_t o, uint64_t dc, uint64_t f) const {
        if (occ) occ[t] += o;
        if (docs) docs[t] += dc;
        if (first && f < first[t]) first[t] = f;
    }
};

struct Entry { uint32_t t; bool fst; uint64_t doc; };

struct Cache {
    std::vector<uint32_t> term, occ, docs, flag;
    std::vector<uint64_t> first;
    Cache() : term(kStatsCacheSlots, kStatsNoTerm), occ(kStatsCacheSlots), docs(kStatsCacheSlots), flag(kStatsCacheSlots), first(kStatsCacheSlots, kNoDoc) {}
    void add(uint32_t s, const Entry& e) {
        occ[s]++;
        if (e.fst) { docs[s]++; first[s] = std::min(first[s], e.doc); }
    }
    void reset(uint32_t s, uint32_t t) { term[s] = t; occ[s] = 0; docs[s] = 0; first[s] = kNoDoc; }
    void flush(const Out& G) {
        for (uint32_t s = 0; s < kStatsCacheSlots; s++) {
            if (term[s] == kStatsNoTerm) continue;
            G.add(term[s], occ[s], docs[s], first[s]);
            reset(s, kStatsNoTerm);
        }
    }
    // cache_step of gft_stats.hip: the three phases, every lane's entries in each
    void step(const Out& G, const std::vector<Entry>& E) {
        std::vector<uint8_t> conf(E.size()), won(E.size());
        for (size_t i = 0; i < E.size(); i++) {
            const uint32_t s = stats_cache_slot(E[i].t);
            if (term[s] == kStatsNoTerm) term[s] = E[i].t;
            if (term[s] == E[i].t) add(s, E[i]); else conf[i] = 1;
        }
        for (size_t i = 0; i < E.size(); i++) {
            if (!conf[i]) continue;
            const uint32_t s = stats_cache_slot(E[i].t);
            if (flag[s]) continue;
            flag[s] = 1; won[i] = 1;
            G.add(term[s], occ[s], docs[s], first[s]);
            reset(s, E[i].t);
        }
        for (size_t i = 0; i < E.size(); i++) {
            if (!conf[i]) continue;
            const uint32_t s = stats_cache_slot(E[i].t);
            if (term[s] == E[i].t) add(s, E[i]);
            else G.add(E[i].t, 1, E[i].fst, E[i].fst ? E[i].doc : kNoDoc);
        }
        for (size_t i = 0; i < E.size(); i++)
            if (won[i]) flag[stats_cache_slot(E[i].t)] = 0;
    }
};

// k_stats_count for workgroup w of G
void count_group(const uint64_t* off, const uint32_t* term, uint64_t n_docs, uint32_t n_terms, uint64_t doc_base, uint64_t w, uint64_t G,
                 const Out& out, std::vector<uint64_t>& set, std::vector<uint32_t>& bits) {
    Cache C;
    const uint64_t dlo = stats_cut(off, n_docs, w, G), dhi = stats_cut(off, n_docs, w + 1, G);
    uint64_t since = 0;
    std::vector<uint32_t> rel(kStatsStepDocs + 1);
    std::vector<Entry> E;
    for (uint64_t d = dlo; d < dhi;) {
        const uint64_t e0 = off[d];
        const uint32_t tries = (uint32_t)std::min<uint64_t>(kStatsStepDocs, dhi - d);
        for (uint32_t k = 0; k <= tries; k++) rel[k] = stats_rel(off[d + k], e0);
        const uint32_t nd = stats_step_docs(rel, tries);
        if (nd) {
            const uint32_t ne = rel[nd];
            if (ne) {
                if (since + ne > kStatsFlushEntries) { C.flush(out); since = 0; }
                since += ne;
                E.clear();
                std::vector<uint32_t> mine;
                for (uint32_t i = 0; i < ne; i++) {
                    const uint32_t t = term[e0 + i], dl = stats_find_doc(rel, nd, i);
                    const uint64_t key = stats_set_key(dl, t);
                    bool fst = false;
                    for (uint32_t s = stats_set_slot(dl, t);; s = stats_set_next(s)) {
                        if (set[s] == 0) { set[s] = key; fst = true; mine.push_back(s); break; }
                        if (set[s] == key) break;
                    }
                    E.push_back(Entry{t, fst, doc_base + d + dl});
                }
                for (uint32_t s : mine) set[s] = 0;
                C.step(out, E);
            }
            d += nd;
        } else {
            const uint64_t cnt = off[d + 1] - e0;
            uint32_t* const b = stats_bitset_in_lds(n_terms) ? reinterpret_cast<uint32_t*>(set.data()) : bits.data();
            for (uint64_t c0 = 0; c0 < cnt; c0 += kStatsStep) {
                const uint32_t ne = (uint32_t)std::min<uint64_t>(kStatsStep, cnt - c0);
                if (since + ne > kStatsFlushEntries) { C.flush(out); since = 0; }
                since += ne;
                E.clear();
                for (uint32_t i = 0; i < ne; i++) {
                    const uint32_t t = term[e0 + c0 + i], bit = 1u << (t & 31u);
                    const bool fst = !(b[t >> 5] & bit);
                    b[t >> 5] |= bit;
                    E.push_back(Entry{t, fst, doc_base + d});
                }
                C.step(out, E);
            }
            for (uint64_t i = 0; i < cnt; i++) b[term[e0 + i] >> 5] = 0;
            d += 1;
        }
    }
    C.flush(out);
}

}  // namespace

int term_stats_host(const uint64_t* off, const uint32_t* term, uint64_t n_docs, uint32_t n_terms, uint32_t flags, uint64_t doc_base,
                    uint64_t* occ, uint64_t* docs, uint64_t* first) {
    if (flags & ~GFT_STATS_ACCUMULATE) return GFT_E_INVALID;
    if (n_docs && !off) return GFT_E_INVALID;
    if (n_docs > (~0ull >> 4)) return GFT_E_INVALID;
    const uint64_t e0 = n_docs ? off[0] : 0, e1 = n_docs ? off[n_docs] : 0;
    if (e1 < e0 || e1 - e0 > (~0ull >> 4)) return GFT_E_INVALID;
    const uint64_t n = e1 - e0;
    if (n && (!term || !n_terms)) return GFT_E_INVALID;
    if (stats_buffers_overlap(off, n_docs, term, e0, n, n_terms, occ, docs, first)) return GFT_E_INVALID;
    // k_stats_check
    for (uint64_t d = 0; d < n_docs; d++)
        if (off[d + 1] < off[d]) return GFT_E_INVALID;
    for (uint64_t i = 0; i < n; i++)
        if (term[e0 + i] >= n_terms) return GFT_E_INVALID;
    if (!occ && !docs && !first) return GFT_OK;
    // k_stats_init
    if (!(flags & GFT_STATS_ACCUMULATE))
        for (uint32_t t = 0; t < n_terms; t++) {
            if (occ) occ[t] = 0;
            if (docs) docs[t] = 0;
            if (first) first[t] = kNoDoc;
        }
    if (!n) return GFT_OK;
    const uint64_t G = stats_grid(n, n_docs, kHostResident);
    std::vector<uint64_t> set(kStatsSetSlots);
    std::vector<uint32_t> bits(stats_bitset_in_lds(n_terms) ? 0 : stats_bitset_words(n_terms));
    const Out out{occ, docs, first};
    for (uint64_t w = 0; w < G; w++) count_group(off, term, n_docs, n_terms, doc_base, w, G, out, set, bits);
    return GFT_OK;
}

int count_columns_host(const uint32_t* bitmap, uint64_t n_rows, uint32_t n_cols, const uint64_t* row_idx, uint32_t flags, uint64_t* count) {
    if (flags & ~GFT_STATS_ACCUMULATE) return GFT_E_INVALID;
    if (n_cols && !count) return GFT_E_INVALID;
    if (n_rows && n_cols && !bitmap) return GFT_E_INVALID;
    if (n_rows > (~0ull >> 4)) return GFT_E_INVALID;
    if (columns_buffers_overlap(bitmap, n_rows, n_cols, row_idx, count)) return GFT_E_INVALID;
    const uint32_t W = stats_col_words(n_cols);
    if (!(flags & GFT_STATS_ACCUMULATE))
        for (uint32_t c = 0; c < n_cols; c++) count[c] = 0;
    // k_count_columns: a workgroup a (row chunk, word column)
    for (uint64_t r0 = 0; r0 < n_rows; r0 += kStatsColRows)
        for (uint32_t w = 0; w < W; w++) {
            uint32_t cnt[32] = {0};
            const uint32_t mask = stats_col_mask(n_cols, w);
            for (uint64_t r = r0; r < std::min<uint64_t>(n_rows, r0 + kStatsColRows); r++) {
                const uint32_t word = bitmap[(row_idx ? row_idx[r] : r) * W + w] & mask;
                for (uint32_t b = 0; b < 32; b++) cnt[b] += word >> b & 1u;
            }
            for (uint32_t b = 0; b < 32; b++)
                if (cnt[b]) count[(uint64_t)w * 32 + b] += cnt[b];
        }
    return GFT_OK;
}

}  // namespace gft
