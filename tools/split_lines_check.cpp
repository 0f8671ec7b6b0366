// split_lines_check.cpp -- the split kernels' logic (csrc/gft_split_piece.hpp, run on the host by split_lines_host) against a
// byte-by-byte reference under the address and undefined-behaviour sanitizers: a stand-alone program, CPU only.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I. tools/split_lines_check.cpp \
//       gofindthem_amd/csrc/split_host.cpp -o build/split_lines_check
//   build/split_lines_check 200
//
// Every blob lies in a heap block of exactly its size and the offsets in one of exactly cap entries, so that a read past the
// blob -- the host walk promises none -- or a store past cap is an error of the sanitizer.  Blobs: the fixed cases of
// tests/split_lines.py (built from the walk's own tile and carry-trip sizes), then N seeded random ones.  Both modes; full cap,
// count only, and one entry short.  Exit code 0: walk and reference agree everywhere.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "gofindthem_amd/csrc/gft_split.hpp"

using namespace gft;

namespace {

bool is_ws(uint8_t b) { return b == 0x20 || b == 0x09 || b == 0x0A || b == 0x0D; }

// the contract of include/gft.h, one byte at a time
std::vector<uint64_t> reference(const std::string& s, uint32_t mode) {
    std::vector<uint64_t> off;
    const uint64_t len = s.size();
    if (mode == GFT_SPLIT_AFTER_NL) {
        if (!len) return {0};
        off.push_back(0);
        for (uint64_t p = 0; p + 1 < len; p++)
            if (s[p] == '\n') off.push_back(p + 1);
        off.push_back(len);
        return off;
    }
    uint64_t line = 0;
    bool blank = true;
    for (uint64_t p = 0; p < len; p++) {
        if (blank && !is_ws((uint8_t)s[p])) { off.push_back(off.empty() ? 0 : line); blank = false; }
        if (s[p] == '\n') { line = p + 1; blank = true; }
    }
    if (off.empty()) return {0};
    off.push_back(len);
    return off;
}

int failures = 0;

void check(const std::string& name, const std::string& s) {
    for (uint32_t mode = 0; mode < 2; mode++) {
        const std::vector<uint64_t> want = reference(s, mode);
        const uint64_t n_want = want.size() - 1;
        std::unique_ptr<uint8_t[]> blob(new uint8_t[s.size() ? s.size() : 1]);
        memcpy(blob.get(), s.data(), s.size());
        const uint64_t caps[3] = {n_want + 1, 0, n_want};
        for (uint64_t cap : caps) {
            std::unique_ptr<uint64_t[]> out(new uint64_t[cap ? cap : 1]);
            for (uint64_t i = 0; i < cap; i++) out[i] = ~0ull;
            uint64_t n = ~0ull;
            const int rc = split_lines_host(blob.get(), s.size(), mode, cap ? out.get() : nullptr, cap, &n);
            bool ok = rc == GFT_OK && n == n_want;
            for (uint64_t i = 0; ok && i < cap; i++) ok = out[i] == want[i];
            if (!ok) {
                fprintf(stderr, "MISMATCH %s mode %u cap %llu: rc %d n %llu (want %llu)\n", name.c_str(), mode, (unsigned long long)cap, rc,
                        (unsigned long long)n, (unsigned long long)n_want);
                failures++;
            }
        }
    }
}

std::string short_lines(uint64_t len, uint64_t seed) {
    std::string s;
    std::mt19937_64 rng(seed);
    while (s.size() < len) {
        s += "{\"k\":" + std::to_string(rng() % 1000) + "}";
        s += (rng() % 4 == 0) ? "\r\n" : "\n";
        if (rng() % 8 == 0) s += " \n";
    }
    s.resize(len);
    return s;
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t n_random = argc > 1 ? strtoull(argv[1], nullptr, 10) : 200;
    const uint64_t T = kSplitTile, K = kSplitCarryTrip;
    check("empty", "");
    for (const char* one : {"\n", "x", " "}) check("one byte", one);
    for (uint64_t len : {15ull, 16ull, 17ull, (unsigned long long)T - 1, (unsigned long long)T, (unsigned long long)T + 1}) {
        std::string body;
        while (body.size() < len) body += "{\"a\":1}\n";
        body.resize(len);
        check("final newline or not", body);
        if (len) { body[len - 1] = '\n'; check("final newline", body); body[len - 1] = 'x'; check("no final newline", body); }
        check("only newlines", std::string(len, '\n'));
        check("only whitespace", std::string(len, ' '));
        std::string crlf, ind;
        while (crlf.size() < len) crlf += "{\"a\":1}\r\n";
        while (ind.size() < len) ind += "  \t{\"a\":1}\n";
        crlf.resize(len); ind.resize(len);
        check("crlf", crlf);
        check("indented", ind);
    }
    for (uint64_t at : {T - 1, T, T + 1}) {
        std::string s(2 * T, 'a');
        s[at] = '\n';
        check("newline at a border", s);
        s[at + 1] = ' ';
        check("newline at a border, space behind", s);
    }
    {
        std::string s(2 * T, 'a');
        s[T - 1] = '\n';                              // a line starts exactly on the border: not blank ...
        check("line start on the border", s);
        for (uint64_t i = T; i < T + 40; i++) s[i] = ' ';
        s[T + 40] = '\n';                             // ... and blank
        check("blank line on the border", s);
    }
    check("long line", std::string(3 * T + 5, 'a') + "\n{}\n");
    check("long line, no final newline", "{}\n" + std::string(3 * T + 5, 'a'));
    check("not blank across tiles", "ab\nx" + std::string(2 * T + 3, ' ') + "\n{}\n");
    check("blank across tiles", "ab\n" + std::string(2 * T + 3, ' ') + "{\"a\":1}\n{}\n");
    check("blank from the start", std::string(2 * T + 3, '\t') + "{}\n");
    check("second carry trip", short_lines((K + 1) * T + 7, 1));
    {
        std::string s = short_lines((K + 1) * T + 7, 2);
        for (uint64_t i = K * T - 3 * T / 2; i < K * T + 3 * T / 2; i++) s[i] = (i & 7) ? 'a' : ' ';
        check("a line over the trip border", s);
        for (uint64_t i = K * T - 3 * T / 2; i < K * T + 3 * T / 2; i++) s[i] = ' ';
        check("a blank stretch over the trip border", s);
    }
    std::mt19937_64 rng(12345);
    const char alphabet[] = {'\n', '\r', ' ', '\t', 'a', '{'};
    for (uint64_t r = 0; r < n_random; r++) {
        const uint64_t len = rng() % (r % 10 == 0 ? 1000000 : 20000);
        const uint64_t inv = 2 + rng() % (r % 3 == 0 ? 5000 : 20);
        std::string s(len, ' ');
        for (auto& c : s) c = rng() % inv == 0 ? '\n' : alphabet[1 + rng() % 5];
        check("random " + std::to_string(r), s);
    }
    if (failures) { fprintf(stderr, "%d mismatches\n", failures); return 1; }
    printf("split_lines_check: all cases agree\n");
    return 0;
}
