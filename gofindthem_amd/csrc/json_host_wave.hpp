// json_host_wave.hpp -- the lanes of a wave as loops: the policy class with which the host runs gft_json_walk.hpp
// (json_schema.cpp: the walk against a trie; json_paths.cpp: discovery).  One thread: the atomics are plain accesses.
#pragma once
#include "gft_json_walk.hpp"

namespace gft {

struct HostWave {
    uint8_t bytes[64];
    uint32_t fl[64];
    JsonLaneOut lo[64];
    JsonWaveMem* m;
    void load(const uint8_t* doc, uint32_t base, uint32_t len) {
        for (uint32_t l = 0; l < 64; l++) bytes[l] = (uint64_t)base + l < len ? doc[base + l] : 0;
    }
    uint32_t lane_byte(uint32_t l) const { return bytes[l]; }
    uint32_t byte_at(uint32_t k) const { return bytes[k]; }
    template <class F> uint64_t ballot(F&& f) { uint64_t r = 0; for (uint32_t l = 0; l < 64; l++) if (f(l)) r |= 1ull << l; return r; }
    template <class F> uint32_t sum(F&& f) { uint32_t r = 0; for (uint32_t l = 0; l < 64; l++) r += f(l); return r; }
    template <class F> void each(F&& f) { for (uint32_t l = 0; l < 64; l++) f(l); }
    template <class F> void once(F&& f) { f(); }
    JsonLaneOut& out(uint32_t l) { return lo[l]; }
    uint32_t& flags(uint32_t l) { return fl[l]; }
    template <class T> T uni(T x) const { return x; }
    JsonWaveMem& mem() { return *m; }
    // discovery
    uint64_t uni64(uint64_t x) const { return x; }
    template <class F> uint64_t sum64(F&& f) { uint64_t r = 0; for (uint32_t l = 0; l < 64; l++) r += f(l); return r; }
    uint64_t load64(const uint64_t* p) const { return *p; }
    uint64_t cas64(uint64_t* p, uint64_t v) const { const uint64_t old = *p; if (!old) *p = v; return old; }   // expects 0
    uint32_t add32(uint32_t* p, uint32_t v) const { const uint32_t old = *p; *p = old + v; return old; }
};

}  // namespace gft
