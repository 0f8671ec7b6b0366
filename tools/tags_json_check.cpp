// tags_json_check.cpp -- make_tag_fragments and tags_json_host (csrc/tags_json.cpp: the slot and field tables and the host
// statement of the tag document kernels' contract) under the address and undefined-behaviour sanitizers: a stand-alone program,
// CPU only.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I. tools/tags_json_check.cpp \
//       gofindthem_amd/csrc/tags_json.cpp gofindthem_amd/csrc/dsl_compile.cpp -o build/tags_json_check
//   build/tags_json_check 2000 1
//
// N seeded finders, schemas and batches.  Tags, expression strings and paths are arbitrary byte strings (make_tag_fragments
// takes what the DSL would refuse), repeated pairs and repeated strings under other tags included; tags have 1 .. 70 slots.
// Every array -- the columns of both tables, the blobs with their slack, hit rows, leaf fields, record offsets, hole lengths,
// offsets, the text -- lies in a heap block of exactly its size, so that a read or a store past an end is an error of the
// sanitizer.  Every batch runs with caps 0, 1, 10, 11, total - 1, total, total + 7 and one in the middle, without holes, with
// some and with every record a hole, and is compared with a restatement that builds the documents from a std::map of strings.
// Exit code 0: all agree.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "gofindthem_amd/csrc/tags_json.hpp"

using namespace gft;

namespace {

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size()]);
    if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
    return p;
}

template <class T>
void tight(std::vector<T>& v) { std::vector<T>(v.begin(), v.end()).swap(v); }

// the escaper, restated: json_str's cases one by one
std::string quoted(const std::string& s) {
    static const char* hex = "0123456789abcdef";
    std::string o = "\"";
    for (unsigned char c : s) {
        switch (c) {
            case '"': o += "\\\""; break;
            case '\\': o += "\\\\"; break;
            case '\n': o += "\\n"; break;
            case '\r': o += "\\r"; break;
            case '\t': o += "\\t"; break;
            default:
                if (c < 0x20) { o += "\\u00"; o += hex[c >> 4]; o += hex[c & 15]; }
                else o += (char)c;
        }
    }
    return o + "\"";
}

std::string random_bytes(std::mt19937_64& rng, size_t n) {
    static const unsigned char kPool[] = {'a', 'z', '"', '\\', '\n', '\r', '\t', 0x01, 0x1f, 0x7f, 0xc3, 0xa9, 0xff, ' ', ':', 0};
    std::string s;
    for (size_t k = 0; k < n; k++) s += (char)kPool[rng() % sizeof kPool];
    return s;
}

struct Setup {
    std::vector<std::string> tags, exprs;         // [E]
    std::vector<std::string> schema;              // [F], unique
    std::vector<uint32_t> valid;                  // [ceil(F / 32)]
};

Setup make_setup(std::mt19937_64& rng) {
    static const uint32_t kE[] = {0, 1, 31, 32, 33, 64, 65, 200, 1000};
    static const uint32_t kF[] = {1, 2, 5, 33, 65};
    static const size_t kLen[] = {0, 1, 2, 3, 57, 58, 59, 249, 250, 251, 4994};
    Setup s;
    const uint32_t E = kE[rng() % 9], F = kF[rng() % 5];
    std::vector<std::string> tag_pool;
    const uint32_t T = 1 + (uint32_t)(rng() % (E > 100 ? 40 : 4));
    for (uint32_t t = 0; t < T; t++) tag_pool.push_back(t ? random_bytes(rng, rng() % 4 ? 1 + rng() % 5 : kLen[rng() % 11]) : std::string());
    for (uint32_t e = 0; e < E; e++) {
        if (e && rng() % 6 == 0) {                // a pair once more, or its string under another tag
            const uint32_t k = (uint32_t)(rng() % e);
            s.exprs.push_back(s.exprs[k]);
            s.tags.push_back(rng() % 2 ? s.tags[k] : tag_pool[rng() % T]);
        } else {
            s.exprs.push_back(random_bytes(rng, rng() % 32 ? rng() % 12 : kLen[rng() % 11]));
            s.tags.push_back(rng() % 3 ? tag_pool[0] : tag_pool[rng() % T]);      // (one large tag: more than 32 slots)
        }
    }
    std::set<std::string> seen;
    while (s.schema.size() < F) {
        const std::string p = random_bytes(rng, rng() % 8 ? rng() % 7 : kLen[rng() % 11]);
        if (seen.insert(p).second) s.schema.push_back(p);
    }
    s.valid.assign((F + 31) / 32, 0);
    for (uint32_t f = 0; f < F; f++)
        if (rng() % 5) s.valid[f >> 5] |= 1u << (f & 31);
    return s;
}

bool check(const Setup& s, std::mt19937_64& rng, uint64_t& bytes, uint64_t& hole_docs, uint64_t& shared_slots) {
    const uint32_t E = (uint32_t)s.exprs.size(), F = (uint32_t)s.schema.size();
    const uint64_t EW = (E + 31) / 32;
    std::vector<TagExpr> exprs;
    for (uint32_t e = 0; e < E; e++) exprs.push_back(TagExpr{&s.tags[e], &s.exprs[e]});
    TagFragments fr;
    std::string why;
    if (!make_tag_fragments(exprs, s.schema, s.valid, fr, why)) return false;
    TagSlots& ts = fr.slots;
    TagFields& tf = fr.fields;
    // the tables in blocks of exactly their size
    for (auto* v : {&ts.expr_slot, &ts.src_off, &ts.src_expr, &ts.slot_off, &ts.slot_len, &ts.word_tag, &ts.tag_word, &ts.tag_words, &ts.tag_off,
                    &ts.tag_len, &tf.field_rank, &tf.field_off, &tf.field_len, &tf.valid})
        tight(*v);
    tight(ts.blob);
    tight(tf.blob);
    if (ts.blob.size() < kTagFragSlack || tf.blob.size() < kTagFragSlack) return false;
    // the tables against their description
    std::set<std::pair<std::string, std::string>> pairs;
    for (uint32_t e = 0; e < E; e++) pairs.insert({s.tags[e], s.exprs[e]});
    shared_slots += E - pairs.size();
    if (ts.expr_slot.size() != E || ts.word_tag.size() != ts.SW || ts.src_off.size() != (size_t)ts.SW * 32 + 1 || ts.src_expr.size() != E) return false;
    {
        int64_t prev_slot = -1;
        std::string prev_tag;
        bool first = true;
        uint32_t real = 0;
        for (const auto& p : pairs) {             // (the set's order: unsigned bytes, tag then string)
            // the pair's slot: that of any of its expressions
            uint32_t slot = ~0u;
            for (uint32_t e = 0; e < E; e++)
                if (s.tags[e] == p.first && s.exprs[e] == p.second) {
                    if (slot != ~0u && ts.expr_slot[e] != slot) return false;
                    slot = ts.expr_slot[e];
                }
            if ((int64_t)slot <= prev_slot || slot >= ts.SW * 32) return false;
            const bool new_tag = first || p.first != prev_tag;
            if (new_tag && (slot & 31)) return false;                          // a tag begins at a word border
            if (!new_tag && ts.word_tag[slot >> 5] != ts.word_tag[(uint32_t)prev_slot >> 5]) return false;
            const std::string frag = quoted(p.second), tfrag = quoted(p.first) + ":{";
            if (ts.slot_len[slot] != frag.size() || memcmp(ts.blob.data() + ts.slot_off[slot], frag.data(), frag.size())) return false;
            const uint32_t t = ts.word_tag[slot >> 5];
            if (t >= ts.n_tags || ts.tag_len[t] != tfrag.size() || memcmp(ts.blob.data() + ts.tag_off[t], tfrag.data(), tfrag.size())) return false;
            if (slot >> 5 < ts.tag_word[t] || slot >> 5 >= ts.tag_word[t] + ts.tag_words[t]) return false;
            prev_slot = slot; prev_tag = p.first; first = false;
            real++;
        }
        uint32_t with_source = 0;
        for (uint32_t k = 0; k < ts.SW * 32; k++) {
            with_source += ts.src_off[k + 1] > ts.src_off[k];
            for (uint32_t j = ts.src_off[k]; j < ts.src_off[k + 1]; j++)
                if (ts.src_expr[j] >= E || ts.expr_slot[ts.src_expr[j]] != k) return false;
        }
        if (with_source != real) return false;
    }
    for (uint32_t f = 0; f < F; f++) {
        uint32_t below = 0;
        for (uint32_t h = 0; h < F; h++) below += s.schema[h] < s.schema[f];
        const std::string frag = quoted(s.schema[f]) + ":[";
        if (tf.field_rank[f] != below || tf.field_len[f] != frag.size() || memcmp(tf.blob.data() + tf.field_off[f], frag.data(), frag.size())) return false;
    }
    // a batch: records that name a field at most once, in any order
    static const uint64_t kRecs[] = {0, 1, 2, 5, 63, 64, 65, 129};
    const uint64_t n_records = kRecs[rng() % (E > 100 ? 4 : 8)];
    std::vector<uint32_t> hits, leaf_field;
    std::vector<uint64_t> rec_off{0};
    for (uint64_t d = 0; d < n_records; d++) {
        std::vector<uint32_t> order(F);
        for (uint32_t f = 0; f < F; f++) order[f] = f;
        for (uint32_t f = F; f > 1; f--) std::swap(order[f - 1], order[rng() % f]);
        const uint32_t L = (uint32_t)(rng() % (F + 1));
        const unsigned density = rng() % 5;       // empty, sparse, one bit a word, half, every bit (garbage at and above E included)
        for (uint32_t l = 0; l < L; l++) {
            leaf_field.push_back(order[l]);
            for (uint64_t w = 0; w < EW; w++) {
                const uint32_t x = (uint32_t)rng(), y = (uint32_t)rng();
                hits.push_back(density == 0 ? 0u : density == 1 ? (x & y & (uint32_t)rng()) : density == 2 ? 1u << (x & 31) : density == 3 ? x : 0xFFFFFFFFu);
            }
        }
        rec_off.push_back(leaf_field.size());
    }
    auto d_hits = exact(hits);
    auto d_field = exact(leaf_field);
    auto d_rec = exact(rec_off);
    for (int hole_mode = 0; hole_mode < 3; hole_mode++) {  // none, some (first, last, adjacent), every record
        std::vector<uint64_t> holes(n_records, 0);
        for (uint64_t d = 0; d < n_records; d++)
            if (hole_mode == 2 || (hole_mode == 1 && (d == 0 || d + 1 == n_records || d == n_records / 2 || d == n_records / 2 + 1 || rng() % 7 == 0))) holes[d] = 11 + rng() % 90;
        // the restatement: a map of sets of strings
        std::string want = "[";
        std::vector<uint64_t> want_off{1};
        for (uint64_t d = 0; d < n_records; d++) {
            std::string doc;
            if (holes[d]) {
                doc.assign((size_t)holes[d], (char)0xA5);
                hole_docs++;
            } else {
                TagDocMap m;
                for (uint64_t l = rec_off[d]; l < rec_off[d + 1]; l++) {
                    const uint32_t f = leaf_field[l];
                    if (!(s.valid[f >> 5] >> (f & 31) & 1u)) continue;
                    for (uint32_t e = 0; e < E; e++)
                        if (hits[l * EW + e / 32] >> (e % 32) & 1u) m[s.tags[e]][s.schema[f]].insert(s.exprs[e]);
                }
                doc = "{\"tags\":{";
                bool f1 = true;
                for (const auto& t : m) {
                    if (!f1) doc += ",";
                    f1 = false;
                    doc += quoted(t.first) + ":{";
                    bool f2 = true;
                    for (const auto& fp : t.second) {
                        if (!f2) doc += ",";
                        f2 = false;
                        doc += quoted(fp.first) + ":[";
                        bool f3 = true;
                        for (const auto& x : fp.second) { if (!f3) doc += ","; f3 = false; doc += quoted(x); }
                        doc += "]";
                    }
                    doc += "}";
                }
                doc += "}}";
                std::string same;
                tag_doc_text("", m, same);         // the host serialisation's own writer says the same
                if (same != doc) return false;
            }
            if (d) want += ",";
            want += doc;
            want_off.push_back(want.size() + 1);
        }
        want += "]";
        const uint64_t total = want.size();
        bytes += total;
        auto d_holes = exact(holes);
        const uint64_t caps[8] = {0, 1, 10, 11, total - 1, total, total + 7, total / 2};
        for (uint64_t cap : caps) {
            std::unique_ptr<uint64_t[]> out_off(new uint64_t[n_records + 1]);
            std::unique_ptr<uint8_t[]> out(new uint8_t[cap]);
            memset(out.get(), 0xA5, cap);
            uint64_t got_total = ~0ull;
            if (tags_json_host(ts, tf, d_hits.get(), d_field.get(), d_rec.get(), n_records, hole_mode ? d_holes.get() : nullptr, cap ? out.get() : nullptr, cap,
                               out_off.get(), &got_total) != kTagsJsonOk)
                return false;
            if (got_total != total || memcmp(out_off.get(), want_off.data(), (n_records + 1) * 8)) return false;
            for (uint64_t k = 0; k < cap; k++)
                if (out[k] != (k < total ? (uint8_t)want[k] : 0xA5)) return false;
        }
    }
    return true;
}

// the refusals: a hole of 4 GiB, a field twice, a record wider than the cap (and the same as a hole)
bool refusals() {
    const std::string tag = "t", expr = "x";
    TagFragments fr;
    std::string why;
    if (!make_tag_fragments({TagExpr{&tag, &expr}}, {"a", "b"}, {3u}, fr, why)) return false;
    uint64_t total = 0;
    {
        const uint64_t hole = 1ull << 32, rec_off[2] = {0, 0};
        uint64_t off[2];
        if (tags_json_host(fr.slots, fr.fields, nullptr, nullptr, rec_off, 1, &hole, nullptr, 0, off, &total) != kTagsJsonHole) return false;
    }
    {
        const uint32_t hits[2] = {1, 1}, field[2] = {1, 1};
        const uint64_t rec_off[2] = {0, 2};
        uint64_t off[2];
        if (tags_json_host(fr.slots, fr.fields, hits, field, rec_off, 1, nullptr, nullptr, 0, off, &total) != kTagsJsonTwice) return false;
    }
    {
        std::vector<uint32_t> hits(GFT_TAGS_JSON_MAX_LEAVES + 1, 0), field(GFT_TAGS_JSON_MAX_LEAVES + 1, 0);
        const uint64_t rec_off[2] = {0, GFT_TAGS_JSON_MAX_LEAVES + 1}, hole = 40;
        uint64_t off[2];
        auto d_hits = exact(hits);
        auto d_field = exact(field);
        if (tags_json_host(fr.slots, fr.fields, d_hits.get(), d_field.get(), rec_off, 1, nullptr, nullptr, 0, off, &total) != kTagsJsonLeaves) return false;
        if (tags_json_host(fr.slots, fr.fields, d_hits.get(), d_field.get(), rec_off, 1, &hole, nullptr, 0, off, &total) != kTagsJsonOk || total != 42) return false;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 2000;
    std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
    uint64_t bytes = 0, hole_docs = 0, shared_slots = 0;
    for (uint64_t i = 0; i < n; i++) {
        const Setup s = make_setup(rng);
        if (!check(s, rng, bytes, hole_docs, shared_slots)) { fprintf(stderr, "batch %llu: tags_json_host disagrees with the restatement\n", (unsigned long long)i); return 1; }
    }
    if (!refusals()) { fprintf(stderr, "a refusal was not answered as the contract says\n"); return 1; }
    printf("tags_json_check: %llu batches, %llu bytes of text, %llu holes, %llu expressions that share a slot: ok\n", (unsigned long long)n,
           (unsigned long long)bytes, (unsigned long long)hole_docs, (unsigned long long)shared_slots);
    return bytes && hole_docs && shared_slots ? 0 : 2;   // (a run without text, holes or shared slots checked too little)
}
