// group_dsl_check.cpp -- the tag-rule DSL (csrc/group_dsl.cpp: Scanner, Parse, ToJson, Solve) under the address and
// undefined-behaviour sanitizers: a stand-alone program, CPU only.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I. tools/group_dsl_check.cpp \
//       gofindthem_amd/csrc/group_dsl.cpp gofindthem_amd/csrc/dsl_compile.cpp gofindthem_amd/csrc/json_mini.cpp \
//       -o build/group_dsl_check
//   build/group_dsl_check tests/golden/group_scanner.json tests/golden/group_parser.json tests/golden/group_solver.json 5000 1
//
// The golden files are the data: every "expStr" of the three tables is an input, a solver case brings its tag map.  Each input
// goes through the scanner to the end, then Parse, ToJson of the tree and Solve (against the case's map, else an empty one).
// Then N seeded byte mutations of those inputs do the same.  Checked here for the unmutated inputs: the parser's error text
// and the solver's verdict.  Tokens and tree shapes are compared with the golden files by tests/test_group_host.py, through
// the C ABI.  Exit code 0: no sanitizer report and no difference.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "gofindthem_amd/csrc/group_dsl.hpp"
#include "gofindthem_amd/csrc/json_mini.hpp"

using namespace gft;

namespace {

struct Case {
    std::string src;
    bool has_map = false; gdsl::TagMap map;                // solver cases
    bool want_verdict = false;
    bool parser_case = false; std::string want_err;        // parser cases ("" = parses)
};

const json::Value* member(const json::Value& o, const char* key) {
    for (const auto& kv : o.obj) if (kv.first == key) return &kv.second;
    return nullptr;
}

bool load(const char* path, std::vector<Case>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return false; }
    std::string text;
    char buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, n);
    fclose(f);
    json::Value doc;
    const std::string err = json::Parse(text.data(), text.size(), doc);
    const json::Value* cases = err.empty() ? member(doc, "cases") : nullptr;
    if (!cases) { fprintf(stderr, "%s: %s\n", path, err.empty() ? "no \"cases\"" : err.c_str()); return false; }
    for (const auto& c : cases->arr) {
        const json::Value* src = member(c, "expStr");
        if (!src) { fprintf(stderr, "%s: a case without expStr\n", path); return false; }
        Case k;
        k.src = src->str;
        if (const json::Value* m = member(c, "map")) {     // {tag: {field: [expressions]} | null}
            k.has_map = true;
            for (const auto& t : m->obj) {
                auto& fields = k.map[t.first];
                for (const auto& fp : t.second.obj) {
                    auto& set = fields[fp.first];
                    for (const auto& x : fp.second.arr) set.insert(x.str);
                }
            }
            k.want_verdict = member(c, "expected") && member(c, "expected")->b;
        }
        if (const json::Value* e = member(c, "error")) { k.parser_case = true; k.want_err = e->str; }
        out.push_back(std::move(k));
    }
    return true;
}

uint64_t n_tokens = 0, n_trees = 0, n_true = 0;

// everything the DSL does with one input; fills what the caller may compare
void run(const std::string& src, const gdsl::TagMap& map, std::string& parse_err, bool& verdict) {
    gdsl::Scanner sc(src);
    for (;;) {
        const gdsl::ScanResult r = sc.Scan();
        n_tokens++;
        if (!r.err.empty() || r.tok == gdsl::END_OF_INPUT) break;
    }
    gdsl::ParseResult pr = gdsl::Parse(src);
    parse_err = pr.err;
    verdict = false;
    if (!pr.expr) return;
    n_trees++;
    if (gdsl::ToJson(*pr.expr).empty()) abort();
    std::string err;
    verdict = gdsl::Solve(*pr.expr, map, err) && err.empty();
    n_true += verdict;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s scanner.json parser.json solver.json [mutations] [seed]\n", argv[0]); return 2; }
    const uint64_t n_mut = argc > 4 ? strtoull(argv[4], nullptr, 10) : 5000;
    const uint64_t seed = argc > 5 ? strtoull(argv[5], nullptr, 10) : 1;
    std::vector<Case> cases;
    for (int i = 1; i <= 3; i++) if (!load(argv[i], cases)) return 2;
    if (cases.empty()) { fprintf(stderr, "no cases\n"); return 2; }
    const gdsl::TagMap none;
    std::string err;
    bool verdict;
    int bad = 0;
    for (const Case& c : cases) {
        run(c.src, c.has_map ? c.map : none, err, verdict);
        if (c.parser_case && err != c.want_err) { fprintf(stderr, "PARSE: %s\n  got  '%s'\n  want '%s'\n", c.src.c_str(), err.c_str(), c.want_err.c_str()); bad++; }
        if (c.has_map && verdict != c.want_verdict) { fprintf(stderr, "SOLVE: %s: got %d, want %d\n", c.src.c_str(), verdict, c.want_verdict); bad++; }
    }
    std::mt19937_64 rng(seed);
    static const char special[] = "\"\\:() \t\nandortANDORNOT\x00\xff\x80\xc3\xa9";
    for (uint64_t i = 0; i < n_mut; i++) {
        const Case& c = cases[rng() % cases.size()];
        std::string s = c.src;
        for (uint32_t n = 1 + rng() % 3; n; n--) {
            const char b = rng() % 10 < 7 ? special[rng() % (sizeof special - 1)] : (char)(rng() % 256);
            const size_t at = s.empty() ? 0 : rng() % s.size();
            const uint32_t kind = rng() % 3;
            if (kind == 0 && !s.empty()) s[at] = b;
            else if (kind == 1 || s.empty()) s.insert(s.begin() + at, b);
            else s.erase(s.begin() + at);
        }
        run(s, c.has_map ? c.map : none, err, verdict);
    }
    printf("%zu golden inputs, %llu mutations of seed %llu: %llu tokens, %llu trees, %llu true verdicts; %d differences\n", cases.size(),
           (unsigned long long)n_mut, (unsigned long long)seed, (unsigned long long)n_tokens, (unsigned long long)n_trees,
           (unsigned long long)n_true, bad);
    return bad ? 1 : 0;
}
