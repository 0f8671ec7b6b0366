// json_walk_check.cpp -- the device JSON walker's logic (csrc/gft_json_walk.hpp, run on the host by json_leaves_emulate) against
// its reference (json_leaves_ref) under the address and undefined-behaviour sanitizers: a stand-alone program, CPU only.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I. tools/json_walk_check.cpp \
//       gofindthem_amd/csrc/json_schema.cpp gofindthem_amd/csrc/json_mini.cpp gofindthem_amd/csrc/dsl_compile.cpp -o build/json_walk_check
//   python tests/json_docs.py build/json_table.bin          # the edge table of the test suite, as a data file
//   build/json_walk_check build/json_table.bin 1000000 1
//
// Every document is its own batch in a heap block of exactly its size, so that a read past its end -- the walker promises
// none -- is an error of the sanitizer; the output arrays have exactly the sizes the count pass asked for.  Documents: the
// table (with the status each must get), then N seeded ones: generated from the schema, mutated by a few byte edits, random
// bytes.  Exit code 0: the walker and the reference agree on every array of every document.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "gofindthem_amd/csrc/json_schema.hpp"

using namespace gft;

namespace {

struct Result {
    uint8_t status = 0;
    uint64_t rec_off[2] = {0, 0}, totals[2] = {0, 0};
    std::vector<uint32_t> field;
    std::vector<uint64_t> off;
    std::vector<uint8_t> text;
    bool operator==(const Result& o) const {
        return status == o.status && rec_off[1] == o.rec_off[1] && totals[0] == o.totals[0] && totals[1] == o.totals[1] && field == o.field &&
               off == o.off && text == o.text;
    }
};

template <class F>
bool run(F&& call, const std::string& doc, Result& r) {
    // exactly-sized blocks: the document without slack, the arrays as the count pass sized them
    std::unique_ptr<uint8_t[]> blob(new uint8_t[doc.size() ? doc.size() : 1]);
    memcpy(blob.get(), doc.data(), doc.size());
    const uint64_t doc_off[2] = {0, doc.size()};
    std::string err;
    JsonLeavesOut count{&r.status, r.rec_off, nullptr, nullptr, 0, nullptr, 0, r.totals};
    if (call(blob.get(), doc_off, count, err)) { fprintf(stderr, "count pass: %s\n", err.c_str()); return false; }
    r.field.assign(r.totals[0], 0);
    r.off.assign(r.totals[0] + 1, 0);
    r.text.assign(r.totals[1], 0);
    uint64_t again[2] = {0, 0};
    JsonLeavesOut write{&r.status, r.rec_off, r.field.data(), r.off.data(), r.totals[0], r.text.data(), r.totals[1], again};
    if (call(blob.get(), doc_off, write, err)) { fprintf(stderr, "write pass: %s\n", err.c_str()); return false; }
    return again[0] == r.totals[0] && again[1] == r.totals[1];
}

struct Checker {
    std::vector<std::string> paths;
    JsonSchema trie;
    uint64_t by_status[8] = {0, 0, 0, 0, 0, 0, 0, 0}, leaves = 0;
    bool set_schema(const std::vector<std::string>& p) {
        std::string err;
        paths = p;
        if (compile_json_schema(p, trie, err)) { fprintf(stderr, "schema: %s\n", err.c_str()); return false; }
        return true;
    }
    bool check(const std::string& doc, int want_status) {
        Result ref, emu;
        const bool ok = run([&](const uint8_t* b, const uint64_t* o, const JsonLeavesOut& out, std::string& err) {
                            return json_leaves_ref(paths, b, o, 1, out, err); }, doc, ref) &&
                        run([&](const uint8_t* b, const uint64_t* o, const JsonLeavesOut& out, std::string& err) {
                            return json_leaves_emulate(trie, b, o, 1, out, err); }, doc, emu);
        if (!ok || !(ref == emu) || (want_status >= 0 && ref.status != want_status)) {
            fprintf(stderr, "MISMATCH: reference status %u (%llu leaves), walker status %u (%llu leaves), expected %d; document (%zu bytes):\n",
                    ref.status, (unsigned long long)ref.totals[0], emu.status, (unsigned long long)emu.totals[0], want_status, doc.size());
            fwrite(doc.data(), 1, doc.size() < 400 ? doc.size() : 400, stderr);
            fputc('\n', stderr);
            return false;
        }
        by_status[ref.status & 7]++;
        leaves += ref.totals[0];
        return true;
    }
};

// ---- seeded documents against the schema of the test suite's table ------------------------------------------------------
const std::vector<std::string> kSchema = {"", "a", "a.b", "k", "items.index(0)", "items.index(2)", "m.n.o"};

struct Gen {
    std::mt19937_64 rng;
    explicit Gen(uint64_t seed) : rng(seed) {}
    uint32_t below(uint32_t n) { return (uint32_t)(rng() % n); }
    bool chance(uint32_t percent) { return below(100) < percent; }
    void ws(std::string& o) { while (chance(25)) o += " \n\t\r"[below(4)]; }
    void text(std::string& o) {
        static const char* const parts[] = {"a", "b", "Z", "0", " ", ".", "{", "}", "[", "]", ":", ",", "\\\"", "\\\\", "\\/", "/", "\\b", "\\f", "\\n", "\\r",
                                            "\\t", "\\u0000", "\\u001f", "\\u00e9", "\\u00E9", "\\u20ac", "\\uffff", "\\ud7ff", "\\ue000", "\xc3\xa9",
                                            "\xe2\x82\xac", "\xf0\x9f\x98\x80", "\xef\xbf\xbd", "lorem ipsum ", "u", "\\u0075"};
        static const char* const rare[] = {"\\ud83d\\ude00", "\\ud800", "\\udc00", "\xff", "\xc3", "\x80", "\xed\xa0\x80", "\xc0\x80", "\x01", "\\q", "\\u12G4"};
        o += '"';
        for (uint32_t n = below(chance(5) ? 200 : 24); n; n--) {
            if (chance(1) && chance(30)) o += rare[below(sizeof rare / sizeof *rare)];
            else o += parts[below(sizeof parts / sizeof *parts)];
        }
        o += '"';
    }
    void scalar(std::string& o, int depth) {
        static const char* const s[] = {"0", "-1", "3.25", "1e9", "-0.5E-3", "true", "false", "null", "12345678901234567890", "[]", "{}"};
        if (depth < 3 && chance(20)) {
            const bool obj = chance(50);
            o += obj ? '{' : '[';
            for (uint32_t n = below(4), i = 0; i < n; i++) {
                if (i) o += ',';
                ws(o);
                if (obj) { o += "\"u" + std::to_string(chance(10) ? 0 : i) + "\":"; }
                scalar(o, depth + 1);
                ws(o);
            }
            o += obj ? '}' : ']';
        } else {
            o += s[below(sizeof s / sizeof *s)];
        }
    }
    std::string doc() {
        std::string o;
        ws(o);
        if (chance(4)) { text(o); ws(o); return o; }
        o += '{';
        bool first = true;
        auto member = [&](const char* key) { if (!first) o += ','; first = false; ws(o); o += '"'; o += key; o += '"'; ws(o); o += ':'; ws(o); };
        uint32_t order[6] = {0, 1, 2, 3, 4, 5};
        for (uint32_t i = 5; i; i--) std::swap(order[i], order[below(i + 1)]);
        for (uint32_t k : order) {
            if (chance(40)) continue;
            switch (k) {
            case 0: member("a"); if (chance(50)) text(o); else { o += "{"; ws(o); o += "\"b\":"; text(o); ws(o); o += "}"; } break;
            case 1: member("k"); text(o); break;
            case 2:
                member("items");
                o += '[';
                for (uint32_t n = below(5), i = 0; i < n; i++) {
                    if (i) o += ',';
                    ws(o);
                    if ((i == 0 || i == 2) && chance(80)) text(o); else scalar(o, 1);
                    ws(o);
                }
                o += ']';
                break;
            case 3: member("m"); o += "{\"n\":"; ws(o); o += "{"; ws(o); o += "\"o\""; ws(o); o += ":"; text(o); o += "}}"; break;
            case 4: member(chance(50) ? "x1" : "extra"); scalar(o, 0); break;
            default: member(chance(90) ? "y" : chance(50) ? "a.b" : ""); if (chance(90)) scalar(o, 0); else text(o); break;
            }
            ws(o);
        }
        if (chance(4)) { member(chance(50) ? "k" : chance(50) ? "a" : "m"); if (chance(50)) text(o); else scalar(o, 0); }     // perhaps a duplicate
        o += '}';
        ws(o);
        return o;
    }
    void mutate(std::string& d) {
        static const char special[] = "\"\\{}[]:,u \n0-.e\x01\xff\x80\xc3t";
        for (uint32_t n = 1 + below(2); n; n--) {
            const char b = chance(70) ? special[below(sizeof special - 1)] : (char)below(256);
            const size_t at = d.empty() ? 0 : below((uint32_t)d.size());
            const uint32_t kind = below(3);
            if (kind == 0 && !d.empty()) d[at] = b;
            else if (kind == 1 || d.empty()) d.insert(d.begin() + at, b);
            else d.erase(d.begin() + at);
        }
    }
    std::string bytes() {
        static const char pool[] = "{}[]\":,\\ abtrue0123.e-nfls\n";
        std::string o;
        const bool any = chance(50);
        for (uint32_t n = below(200); n; n--) o += any ? (char)below(256) : pool[below(sizeof pool - 1)];
        return o;
    }
};

bool read_u32(FILE* f, uint32_t& v) { return fread(&v, 4, 1, f) == 1; }
bool read_str(FILE* f, std::string& s) {
    uint32_t n;
    if (!read_u32(f, n)) return false;
    s.resize(n);
    return !n || fread(&s[0], 1, n, f) == n;
}

}  // namespace

int main(int argc, char** argv) {
    const char* table = argc > 1 ? argv[1] : "";
    const uint64_t n_random = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1000000;
    const uint64_t seed = argc > 3 ? strtoull(argv[3], nullptr, 10) : 1;
    Checker c;
    uint64_t n_table = 0;
    if (*table) {
        // records of tests/json_docs.py write_table: u32 paths, (u32 length, bytes) each, u32 status, u32 length, the document
        FILE* f = fopen(table, "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", table); return 2; }
        uint32_t n_paths;
        while (read_u32(f, n_paths)) {
            std::vector<std::string> paths(n_paths);
            uint32_t status;
            std::string doc;
            for (auto& p : paths) if (!read_str(f, p)) { fprintf(stderr, "%s: cut record\n", table); return 2; }
            if (!read_u32(f, status) || !read_str(f, doc)) { fprintf(stderr, "%s: cut record\n", table); return 2; }
            if (paths != c.paths && !c.set_schema(paths)) return 1;
            if (!c.check(doc, (int)status)) return 1;
            n_table++;
        }
        fclose(f);
    }
    if (!c.set_schema(kSchema)) return 1;
    Gen g(seed);
    for (uint64_t i = 0; i < n_random; i++) {
        std::string doc = g.chance(8) ? g.bytes() : g.doc();
        const bool clean = !g.chance(45);
        if (!clean) g.mutate(doc);
        if (!c.check(doc, -1)) { fprintf(stderr, "(document %llu of seed %llu)\n", (unsigned long long)i, (unsigned long long)seed); return 1; }
    }
    printf("%llu table documents, %llu seeded documents, %llu leaves; by status:", (unsigned long long)n_table, (unsigned long long)n_random,
           (unsigned long long)c.leaves);
    for (int s = 0; s < 7; s++) printf(" %d: %llu", s, (unsigned long long)c.by_status[s]);
    printf("\nthe walker and the reference agree\n");
    return 0;
}
