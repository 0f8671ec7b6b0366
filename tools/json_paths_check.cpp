// json_paths_check.cpp -- the discovery mode of the device JSON walker (csrc/gft_json_walk.hpp, run on the host by
// json_paths_emulate) against its reference (json_paths_ref) under the address and undefined-behaviour sanitizers: a
// stand-alone program, CPU only.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I. tools/json_paths_check.cpp \
//       gofindthem_amd/csrc/json_paths.cpp gofindthem_amd/csrc/json_schema.cpp gofindthem_amd/csrc/json_mini.cpp \
//       gofindthem_amd/csrc/dsl_compile.cpp -o build/json_paths_check
//   python tests/json_docs.py build/json_table.bin          # the edge table of the test suite, as a data file
//   build/json_paths_check build/json_table.bin 200000 1
//
// Discovery rebuilds a path from key offsets that the wave remembered while it walked the document.  Every document here is
// its own batch in a heap block of exactly its size, so that a read outside it -- in front of it or behind it -- is an error
// of the sanitizer; the set, the offsets and the pool are blocks of exactly their sizes too.  Documents: the table, then N
// seeded ones: generated with keys of 1 to 200 bytes nested up to 40 deep, mutated by a few byte edits, random bytes.  Per
// document: the reference's paths are among the walker's; they are equal when the reader accepts the document.  Exit code 0:
// that held for every document.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "gofindthem_amd/csrc/json_mini.hpp"
#include "gofindthem_amd/csrc/json_paths.hpp"

using namespace gft;

namespace {

constexpr uint32_t kPool = 256u << 10;       // (a pool of the full 8 MiB per document is most of the run time under the sanitizer)

struct Checker {
    uint64_t n_paths = 0, n_accepted = 0, n_extra = 0;
    bool check(const std::string& doc) {
        std::unique_ptr<uint8_t[]> blob(new uint8_t[doc.size() ? doc.size() : 1]);
        memcpy(blob.get(), doc.data(), doc.size());
        const uint64_t doc_off[2] = {0, doc.size()};
        std::vector<std::string> emu, ref;
        std::string err;
        uint64_t dropped = 0;
        if (json_paths_emulate(blob.get(), doc_off, 1, emu, nullptr, &dropped, err, kPool) || json_paths_ref(blob.get(), doc_off, 1, ref, err)) {
            fprintf(stderr, "call failed: %s\n", err.c_str());
            return false;
        }
        json::Value v;
        const bool accepted = json::Parse((const char*)blob.get(), doc.size(), v).empty();
        const bool inside = std::includes(emu.begin(), emu.end(), ref.begin(), ref.end());
        if (dropped || !inside || (accepted && emu != ref) || (!accepted && !ref.empty())) {
            fprintf(stderr, "MISMATCH: walker %zu paths (%llu dropped), reference %zu paths, reader %s; document (%zu bytes):\n", emu.size(),
                    (unsigned long long)dropped, ref.size(), accepted ? "accepts" : "refuses", doc.size());
            fwrite(doc.data(), 1, doc.size() < 400 ? doc.size() : 400, stderr);
            fputc('\n', stderr);
            return false;
        }
        n_paths += emu.size(); n_accepted += accepted; n_extra += emu.size() - ref.size();
        return true;
    }
};

struct Gen {
    std::mt19937_64 rng;
    explicit Gen(uint64_t seed) : rng(seed) {}
    uint32_t below(uint32_t n) { return (uint32_t)(rng() % n); }
    bool chance(uint32_t percent) { return below(100) < percent; }
    void ws(std::string& o) { while (chance(20)) o += " \n\t\r"[below(4)]; }
    void key(std::string& o) {
        static const char* const odd[] = {"", "a.b", "q\\u0041", "\\\\", "\xff", "\xc3\xa9", "index(1)", "\xe6\x97\xa5"};
        o += '"';
        if (chance(8)) o += odd[below(sizeof odd / sizeof *odd)];
        else for (uint32_t n = 1 + below(chance(10) ? 200 : 12); n; n--) o += (char)('a' + below(26));
        o += '"';
    }
    void text(std::string& o) {
        static const char* const parts[] = {"a", " ", "\\\"", "\\\\", "\\n", "\\u00e9", "\\ud83d", "\xe2\x82\xac", "{", "}", "\":", "lorem ipsum "};
        o += '"';
        for (uint32_t n = below(chance(5) ? 150 : 10); n; n--) o += parts[below(sizeof parts / sizeof *parts)];
        o += '"';
    }
    void value(std::string& o, uint32_t depth, uint32_t max_depth) {
        const uint32_t r = below(100);
        if (depth >= max_depth || r < 40) { if (chance(75)) text(o); else o += chance(50) ? "12.5e3" : chance(50) ? "null" : "true"; return; }
        const bool obj = r < 80;
        o += obj ? '{' : '[';
        const uint32_t n = depth > 6 ? 1 + below(2) : below(4);
        for (uint32_t i = 0; i < n; i++) {
            if (i) o += ',';
            ws(o);
            if (obj) { key(o); ws(o); o += ':'; ws(o); }
            value(o, depth + 1, max_depth);
            ws(o);
        }
        o += obj ? '}' : ']';
    }
    std::string doc() {
        std::string o;
        ws(o);
        value(o, 0, chance(10) ? 40 : 5);
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
    const uint64_t n_random = argc > 2 ? strtoull(argv[2], nullptr, 10) : 200000;
    const uint64_t seed = argc > 3 ? strtoull(argv[3], nullptr, 10) : 1;
    Checker c;
    uint64_t n_table = 0;
    if (*table) {
        // records of tests/json_docs.py write_table: u32 paths, (u32 length, bytes) each, u32 status, u32 length, the document
        FILE* f = fopen(table, "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", table); return 2; }
        uint32_t n_paths;
        while (read_u32(f, n_paths)) {
            std::string skip, doc;
            uint32_t status;
            for (uint32_t i = 0; i < n_paths; i++) if (!read_str(f, skip)) { fprintf(stderr, "%s: cut record\n", table); return 2; }
            if (!read_u32(f, status) || !read_str(f, doc)) { fprintf(stderr, "%s: cut record\n", table); return 2; }
            if (!c.check(doc)) return 1;
            n_table++;
        }
        fclose(f);
    }
    Gen g(seed);
    for (uint64_t i = 0; i < n_random; i++) {
        std::string doc = g.chance(8) ? g.bytes() : g.doc();
        if (g.chance(40)) g.mutate(doc);
        if (!c.check(doc)) { fprintf(stderr, "(document %llu of seed %llu)\n", (unsigned long long)i, (unsigned long long)seed); return 1; }
    }
    printf("%llu table documents, %llu seeded documents: %llu accepted by the reader, %llu paths, %llu of them from documents it refuses\n",
           (unsigned long long)n_table, (unsigned long long)n_random, (unsigned long long)c.n_accepted, (unsigned long long)c.n_paths,
           (unsigned long long)c.n_extra);
    printf("the walker's paths and the reference's agree\n");
    return 0;
}
