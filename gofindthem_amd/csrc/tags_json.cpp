// tags_json.cpp -- make_tag_slots / make_tag_fields, tags_json_host, tag_doc_text (tags_json.hpp): a bit at a time, a byte at a
// time.
#include "tags_json.hpp"

#include <algorithm>
#include <numeric>

#include "dsl_compile.hpp"

namespace gft {

namespace {

constexpr uint64_t kBlobLimit = 0xFFFFFFFFull - kTagFragSlack;

// (std::string compares as unsigned bytes: the order of the std::map and the std::set of the host serialisation)
bool blob_add(std::string& blob, const std::string& frag, std::vector<uint32_t>& off, std::vector<uint32_t>& len) {
    if (blob.size() + frag.size() > kBlobLimit) return false;
    off.push_back((uint32_t)blob.size());
    len.push_back((uint32_t)frag.size());
    blob += frag;
    return true;
}

void blob_close(const std::string& blob, std::vector<uint8_t>& out) {
    out.assign(blob.begin(), blob.end());
    out.resize(blob.size() + kTagFragSlack, 0);
}

}  // namespace

bool make_tag_slots(const std::vector<TagExpr>& exprs, TagSlots& out, std::string& why) {
    out = TagSlots();
    const uint32_t E = (uint32_t)exprs.size();
    // the distinct (tag, expression string) pairs in output order
    std::vector<uint32_t> order(E);
    std::iota(order.begin(), order.end(), 0u);
    auto less = [&](uint32_t a, uint32_t b) {
        const int c = exprs[a].tag->compare(*exprs[b].tag);
        return c ? c < 0 : *exprs[a].expr < *exprs[b].expr;
    };
    auto same = [&](uint32_t a, uint32_t b) { return *exprs[a].tag == *exprs[b].tag && *exprs[a].expr == *exprs[b].expr; };
    std::stable_sort(order.begin(), order.end(), less);
    out.n_exprs = E;
    out.expr_slot.assign(E, 0);
    std::string blob, frag;
    std::vector<std::vector<uint32_t>> sources;            // per slot, padding slots included
    auto pad_to_word = [&]() {
        while (sources.size() & 31u) { sources.emplace_back(); out.slot_off.push_back(0); out.slot_len.push_back(0); }
    };
    bool fits = true;
    for (uint32_t k = 0; k < E && fits; k++) {
        const uint32_t e = order[k];
        const bool new_tag = k == 0 || *exprs[e].tag != *exprs[order[k - 1]].tag;
        if (new_tag) {
            pad_to_word();
            if (k) out.tag_words.push_back((uint32_t)(sources.size() / 32) - out.tag_word.back());
            out.tag_word.push_back((uint32_t)(sources.size() / 32));
            frag.clear();
            dsl::json_str(*exprs[e].tag, frag);
            frag += ":{";
            fits = blob_add(blob, frag, out.tag_off, out.tag_len);
        }
        if (new_tag || !same(e, order[k - 1])) {
            sources.emplace_back();
            frag.clear();
            dsl::json_str(*exprs[e].expr, frag);
            fits = fits && blob_add(blob, frag, out.slot_off, out.slot_len);
        }
        sources.back().push_back(e);
        out.expr_slot[e] = (uint32_t)sources.size() - 1;
    }
    if (!fits) {
        out = TagSlots();
        why = "the tags and expression strings, escaped, do not fit 32-bit offsets";
        return false;
    }
    pad_to_word();
    out.SW = (uint32_t)(sources.size() / 32);
    if (E) out.tag_words.push_back(out.SW - out.tag_word.back());
    out.n_tags = (uint32_t)out.tag_word.size();
    out.word_tag.assign(out.SW, 0);
    for (uint32_t t = 0; t < out.n_tags; t++)
        for (uint32_t w = 0; w < out.tag_words[t]; w++) out.word_tag[out.tag_word[t] + w] = t;
    out.src_off.push_back(0);
    for (auto& s : sources) {
        std::sort(s.begin(), s.end());
        out.src_expr.insert(out.src_expr.end(), s.begin(), s.end());
        out.src_off.push_back((uint32_t)out.src_expr.size());
    }
    blob_close(blob, out.blob);
    return true;
}

bool make_tag_fields(const std::vector<std::string>& schema, const std::vector<uint32_t>& valid, TagFields& out, std::string& why) {
    out = TagFields();
    const uint32_t F = (uint32_t)schema.size();
    out.n_fields = F;
    std::vector<uint32_t> order(F);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return schema[a] < schema[b]; });
    out.field_rank.assign(F, 0);
    // (paths listed twice -- SetSchema refuses them -- would share a rank, and a record that names both is "a field twice")
    for (uint32_t k = 0; k < F; k++) out.field_rank[order[k]] = k && schema[order[k]] == schema[order[k - 1]] ? out.field_rank[order[k - 1]] : k;
    std::string blob, frag;
    for (uint32_t f = 0; f < F; f++) {
        frag.clear();
        dsl::json_str(schema[f], frag);
        frag += ":[";
        if (!blob_add(blob, frag, out.field_off, out.field_len)) {
            out = TagFields();
            why = "the field paths, escaped, do not fit 32-bit offsets";
            return false;
        }
    }
    out.valid.assign((F + 31) / 32, 0);
    for (uint32_t w = 0; w < out.valid.size() && w < valid.size(); w++) out.valid[w] = valid[w];
    blob_close(blob, out.blob);
    return true;
}

bool make_tag_fragments(const std::vector<TagExpr>& exprs, const std::vector<std::string>& schema, const std::vector<uint32_t>& valid,
                        TagFragments& out, std::string& why) {
    return make_tag_slots(exprs, out.slots, why) && make_tag_fields(schema, valid, out.fields, why);
}

const char* tags_json_refusal_text(int refusal) {
    switch (refusal) {
        case kTagsJsonOk: return "";
        case kTagsJsonHole: return "a hole of 4 GiB or more";
        case kTagsJsonTwice: return "a record names a field twice";
        case kTagsJsonLeaves: return "a record of more leaves than GFT_TAGS_JSON_MAX_LEAVES that is not a hole";
        default: return "a document of 4 GiB or more";
    }
}

namespace {

// the stores of one batch: a byte at a position at or past the cap is dropped
struct CappedText {
    uint8_t* out; uint64_t cap;
    void put(uint64_t at, uint8_t c) const { if (at < cap) out[at] = c; }
    void put(uint64_t at, const uint8_t* p, uint64_t n) const { for (uint64_t k = 0; k < n; k++) put(at + k, p[k]); }
    void put(uint64_t at, const char* s) const { for (; *s; s++, at++) put(at, (uint8_t)*s); }
};

}  // namespace

int tags_json_host(const TagSlots& ts, const TagFields& tf, const uint32_t* hit_bitmap, const uint32_t* leaf_field, const uint64_t* rec_off,
                   uint64_t n_records, const uint64_t* hole_len, uint8_t* out, uint64_t cap, uint64_t* out_off, uint64_t* total) {
    const uint32_t E = ts.n_exprs, SW = ts.SW;
    const uint64_t EW = (E + 31) / 32;
    const CappedText T{out, out ? cap : 0};
    if (hole_len)
        for (uint64_t d = 0; d < n_records; d++)
            if (hole_len[d] >= 0xFFFFFFFFull) return kTagsJsonHole;
    uint64_t at = 1;
    T.put(0, '[');
    out_off[0] = 1;
    std::vector<uint64_t> leaves;                          // the record's contributing leaves, by field rank
    std::vector<uint32_t> rows;                            // their slot rows [leaves][SW]
    for (uint64_t d = 0; d < n_records; d++) {
        if (hole_len && hole_len[d]) {
            at += hole_len[d];
        } else {
            const uint64_t begin = rec_off[d], end = rec_off[d + 1];
            if (end - begin > GFT_TAGS_JSON_MAX_LEAVES) return kTagsJsonLeaves;
            leaves.clear();
            for (uint64_t l = begin; l < end; l++) {
                const uint32_t f = leaf_field[l];
                if (f < tf.n_fields && (tf.valid[f >> 5] >> (f & 31) & 1u)) leaves.push_back(l);
            }
            std::sort(leaves.begin(), leaves.end(), [&](uint64_t a, uint64_t b) { return tf.field_rank[leaf_field[a]] < tf.field_rank[leaf_field[b]]; });
            for (size_t i = 1; i < leaves.size(); i++)
                if (tf.field_rank[leaf_field[leaves[i]]] == tf.field_rank[leaf_field[leaves[i - 1]]]) return kTagsJsonTwice;
            rows.assign(leaves.size() * (size_t)SW, 0);
            for (size_t i = 0; i < leaves.size(); i++) {
                const uint32_t* hit = hit_bitmap + leaves[i] * EW;
                for (uint32_t e = 0; e < E; e++)
                    if (hit[e >> 5] >> (e & 31) & 1u) rows[i * SW + (ts.expr_slot[e] >> 5)] |= 1u << (ts.expr_slot[e] & 31);
            }
            const uint64_t doc = at;
            T.put(at, "{\"tags\":{");
            at += 9;
            int64_t prev_tag = -1, prev_leaf = -1;         // of the set bit before this one
            for (uint32_t t = 0; t < ts.n_tags; t++)
                for (size_t i = 0; i < leaves.size(); i++)
                    for (uint32_t s = ts.tag_word[t] * 32; s < (ts.tag_word[t] + ts.tag_words[t]) * 32; s++) {
                        if (!(rows[i * SW + (s >> 5)] >> (s & 31) & 1u)) continue;
                        const uint32_t f = leaf_field[leaves[i]];
                        if (prev_tag == (int64_t)t && prev_leaf == (int64_t)i) {
                            T.put(at++, ',');
                        } else {
                            if (prev_tag == (int64_t)t) { T.put(at, "],"); at += 2; }
                            else {
                                if (prev_tag >= 0) { T.put(at, "]},"); at += 3; }
                                T.put(at, ts.blob.data() + ts.tag_off[t], ts.tag_len[t]);
                                at += ts.tag_len[t];
                            }
                            T.put(at, tf.blob.data() + tf.field_off[f], tf.field_len[f]);
                            at += tf.field_len[f];
                        }
                        T.put(at, ts.blob.data() + ts.slot_off[s], ts.slot_len[s]);
                        at += ts.slot_len[s];
                        prev_tag = t; prev_leaf = (int64_t)i;
                    }
            if (prev_tag >= 0) { T.put(at, "]}"); at += 2; }
            T.put(at, "}}");
            at += 2;
            if (at - doc + 1 > 0xFFFFFFFFull) return kTagsJsonLong;
        }
        T.put(at++, d + 1 == n_records ? ']' : ',');
        out_off[d + 1] = at;
    }
    if (!n_records) T.put(at++, ']');
    if (total) *total = at;
    return kTagsJsonOk;
}

void tag_doc_text(const std::string& err, const TagDocMap& tags, std::string& o) {
    if (!err.empty()) { o += "{\"error\":"; dsl::json_str(err, o); o += "}"; return; }
    o += "{\"tags\":{";
    bool f1 = true;
    for (const auto& t : tags) {
        if (!f1) o += ",";
        f1 = false;
        dsl::json_str(t.first, o);
        o += ":{";
        bool f2 = true;
        for (const auto& fp : t.second) {
            if (!f2) o += ",";
            f2 = false;
            dsl::json_str(fp.first, o);
            o += ":[";
            bool f3 = true;
            for (const auto& x : fp.second) { if (!f3) o += ","; f3 = false; dsl::json_str(x, o); }
            o += "]";
        }
        o += "}";
    }
    o += "}}";
}

}  // namespace gft
