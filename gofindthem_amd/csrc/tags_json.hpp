// tags_json.hpp -- the tag result document of a record batch as text: the tables the device copies from, and the contract of
// gft_tagdoc.hip stated in plain loops.  Pure: no device, no handle.  It is gft_debug_tags_json and what the device kernels are
// compared with.
//
//   text = '[' D0 ',' D1 ',' ... ']',   Dd = {"tags":{ members }}
//   a member per tag that was matched in a valid field of record d, tags ascending bytewise: json_str(tag) ":{" then a member per
//   field in which it was matched, paths ascending bytewise: json_str(path) ":[" the distinct expression strings of that tag true
//   in that field, ascending bytewise, each json_str(expr), joined by ',' then ']'; fields joined by ',' then '}'; tags joined
//   by ','.  A record without a contributing hit: {"tags":{}}.
//
// That is byte for byte what gft_group_process_jsons(..., what = 1) writes for a document with those hits: the iteration order of
// std::map<tag, std::map<path, std::set<expression>>>.  The order is compiled into tables once instead of being sorted per entry:
//   slots   a slot is a distinct (tag, expression string) pair, numbered in output order; two expressions with the same pair
//           share one.  Every tag begins at a 32-bit word border of the slot row, so a word of a slot row belongs to one tag.
//   fields  a rank per schema field: the position of its path among the schema's paths in byte order.
// A leaf's hit row [ceil(E / 32)] is permuted into a slot row [SW] (bit s = the OR of the slot's expressions); the text is then a
// function of the slot rows of a record's leaves taken in rank order:  for tag, for leaf by rank, for the tag's words, for bit.
#pragma once
#include <cstdint>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/gft.h"

namespace gft {

constexpr uint32_t kTagDocFixed = 11;      // {"tags":{ and }}: every document is at least this long, so 0 can mean "no hole"
constexpr uint32_t kTagFragSlack = 16;     // readable bytes behind a blob

// The slot part: depends on the finder's expressions only.  The group's.
struct TagSlots {
    uint32_t n_exprs = 0, n_tags = 0, SW = 0;          // SW: words of a slot row
    std::vector<uint32_t> expr_slot;                   // [E] the slot of every expression
    std::vector<uint32_t> src_off, src_expr;           // CSR [SW * 32 + 1], [E]: the expressions of every slot (a padding slot: none)
    std::vector<uint32_t> slot_off, slot_len;          // [SW * 32] json_str(exprString) in the blob (a padding slot: 0, 0)
    std::vector<uint32_t> word_tag;                    // [SW] the tag of every word
    std::vector<uint32_t> tag_word, tag_words;         // [T] a tag's first word and its number of words
    std::vector<uint32_t> tag_off, tag_len;            // [T] json_str(tag) + ":{" in the blob
    std::vector<uint8_t> blob;                         // the fragments, then kTagFragSlack zero bytes
};

// The field part: depends on a schema and its include / exclude lists.  A Records'.
struct TagFields {
    uint32_t n_fields = 0;
    std::vector<uint32_t> field_rank;                  // [F] rank of the path among the schema's paths, bytewise
    std::vector<uint32_t> field_off, field_len;        // [F] json_str(path) + ":[" in the blob
    std::vector<uint32_t> valid;                       // [ceil(F / 32)] RuleSet::valid
    std::vector<uint8_t> blob;
};

struct TagFragments { TagSlots slots; TagFields fields; };

// an expression of the finder, in the order of the hit rows' bits
struct TagExpr { const std::string* tag; const std::string* expr; };

// false: a table the format cannot hold -- a blob that does not fit 32-bit offsets -- and `why` says so.  Never the caller's
// error: such a group serialises on the host.
bool make_tag_slots(const std::vector<TagExpr>& exprs, TagSlots& out, std::string& why);
bool make_tag_fields(const std::vector<std::string>& schema, const std::vector<uint32_t>& valid, TagFields& out, std::string& why);
bool make_tag_fragments(const std::vector<TagExpr>& exprs, const std::vector<std::string>& schema, const std::vector<uint32_t>& valid,
                        TagFragments& out, std::string& why);

// what tags_json_host and the device call answer besides "done"
enum TagsJsonRefusal {
    kTagsJsonOk = 0,
    kTagsJsonHole,         // a hole of 4 GiB or more (GFT_E_INVALID)
    kTagsJsonTwice,        // a record names a valid field twice          } GFT_E_UNSUPPORTED: "serialise on the host"
    kTagsJsonLeaves,       // more than GFT_TAGS_JSON_MAX_LEAVES, no hole  }
    kTagsJsonLong,         // a document whose length + 1 is not 32 bits   }
};
const char* tags_json_refusal_text(int refusal);

// hit rows [n_leaves][ceil(n_exprs / 32)] (bits at and above n_exprs ignored), leaf_field, rec_off: a validated batch
// (validate_records) -> the text and out_off [n_records + 1]: out_off[0] = 1, out_off[d + 1] = out_off[d] + len(d) + 1, the
// separator behind document d (',' or the closing ']') at out_off[d + 1] - 1.  hole_len (nullable) [n_records]: a value != 0
// reserves exactly that many bytes for document d, none of them is written and its leaves are not read.  A leaf whose field is
// invalid contributes nothing.  A byte at a position >= cap is not stored; *total (nullable) = the text's size (2 for
// n_records == 0: "[]").  out == nullptr with cap == 0 counts only.  Anything but kTagsJsonOk: nothing is complete.
int tags_json_host(const TagSlots& ts, const TagFields& tf, const uint32_t* hit_bitmap, const uint32_t* leaf_field, const uint64_t* rec_off,
                   uint64_t n_records, const uint64_t* hole_len, uint8_t* out, uint64_t cap, uint64_t* out_off, uint64_t* total);

// One document of the host serialisation: {"error": json_str(err)} or {"tags":{..}} -- what a hole's text is
using TagDocMap = std::map<std::string, std::map<std::string, std::set<std::string>>>;
void tag_doc_text(const std::string& err, const TagDocMap& tags, std::string& o);

}  // namespace gft
