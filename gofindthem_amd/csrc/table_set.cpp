// table_set.cpp -- a dictionary's tables, their blob and the choice of the scan kernel (table_set.hpp): host arithmetic
// only, no device and no handle.
#include "table_set.hpp"

#include <algorithm>
#include <cstring>

#include "../../include/gft.h"

namespace gft {

void compile_tables(std::vector<std::string> terms, TableSet& out) {
    build_ac_tables(std::move(terms), out.tab);
    build_scan2_tables(out.tab, out.s2);     // suffix-window tables (scan2, kept as a cross-check)
    build_scan3_tables(out.tab, out.s3);     // stride-2 suffix-window tables (the fast path)
}

// ---- compiled tables as one blob --------------------------------------------------------------------------------------
namespace {
constexpr uint32_t kTablesMagic = 0x54544647u;   // "GFTT"

struct Writer {
    std::vector<uint8_t> b;
    void raw(const void* p, size_t n) { const uint8_t* q = (const uint8_t*)p; b.insert(b.end(), q, q + n); }
    void u32(uint32_t v) { raw(&v, 4); }
    void u64(uint64_t v) { raw(&v, 8); }
    template <class T> void vec(const std::vector<T>& v) { u64(v.size()); if (!v.empty()) raw(v.data(), v.size() * sizeof(T)); }
};
struct Reader {
    const uint8_t* p; uint64_t n, i = 0; bool ok = true;
    bool raw(void* d, size_t k) { if (!ok || k > n - i) { ok = false; return false; } memcpy(d, p + i, k); i += k; return true; }
    uint32_t u32() { uint32_t v = 0; raw(&v, 4); return v; }
    uint64_t u64() { uint64_t v = 0; raw(&v, 8); return v; }
    template <class T> void vec(std::vector<T>& v) {
        const uint64_t k = u64();
        if (!ok || k > (n - i) / sizeof(T)) { ok = false; return; }
        v.resize((size_t)k);
        if (k) raw(v.data(), (size_t)k * sizeof(T));
    }
};
// Every index a kernel follows must stay inside the table it indexes: a blob that passes the checksum may still be stale
// (another library build) or crafted.  Returns what is wrong, or nullptr.
const char* validate_tables(const AcTables& a, const Scan2Tables& t, const Scan3Tables& u) {
    const size_t n_terms = a.terms.size();
    if (a.n_classes == 0 || a.n_classes > 256) return "class count";
    for (int b = 0; b < 256; b++) if (a.byte_class[b] >= a.n_classes) return "byte class";
    for (uint32_t d : a.delta) if ((d & ~kOutFlag) >= a.n_states) return "DFA target";
    for (uint32_t x : a.out_term) if (x != kNoTerm && x >= n_terms) return "DFA output term";
    for (uint32_t x : a.out_link) if (x >= a.n_states) return "DFA output link";
    for (size_t i = 0; i < n_terms; i++) if (a.term_len[i] != a.terms[i].size()) return "term length";
    auto slots_ok = [&](const std::vector<Scan2Slot>& slots, const std::vector<Scan2Slot>& more, uint32_t shift, const std::vector<uint8_t>& blob,
                        const std::vector<uint32_t>& off) -> const char* {
        if (shift < 1 || shift > 31 || slots.size() != ((size_t)1 << (32 - shift))) return "bucket table size";
        if (off.size() != n_terms + 1) return "term offsets";
        for (size_t i = 0; i < n_terms; i++)
            if (off[i] < 4 || (uint64_t)off[i] + a.terms[i].size() + 8 > blob.size()) return "term offset";
        auto entry_ok = [&](const Scan2Slot& s) {
            const uint32_t len1 = s.len & kScan2LenMask;
            const int off8 = (int)(int8_t)(s.len >> 24);
            return s.info < n_terms && off8 >= -1 && off8 <= (int)kScan2MaxOff && (int64_t)len1 + off8 == (int64_t)a.terms[s.info].size() && len1 >= 4;
        };
        for (const Scan2Slot& s : slots) {
            if (s.key == kScan2EmptyKey) continue;
            if (s.info & kScan2Multi) {
                const uint64_t at = s.info & ~kScan2Multi;
                if (at + s.len > more.size() || s.len == 0) return "bucket list";
            } else if (!entry_ok(s)) return "bucket entry";
        }
        for (const Scan2Slot& s : more) if (s.key != kScan2EmptyKey && !entry_ok(s)) return "bucket list entry";
        return nullptr;
    };
    if (t.supported) {
        if (t.kp == 0 || t.kp > 256 || t.pad_class >= t.kp) return "scan2 classes";
        for (int b = 0; b < 256; b++) if (t.cls[b] >= t.kp || t.cls_fold[b] >= t.kp) return "scan2 byte class";
        // build_scan5_tables (run on imported tables too) indexes its class counters by the automaton's byte classes and splits
        // every bucket key into four classes: the two class maps must be one, and a key must be four classes
        if (t.kp != a.n_classes) return "scan2 class count differs from the automaton's";
        for (int b = 0; b < 256; b++) if (t.cls[b] != a.byte_class[b]) return "scan2 byte class differs from the automaton's";
        // (a key lives in ITS pair of the bucket table and nowhere else: the kernels look nowhere else)
        if (t.slot_shift < 1 || t.slot_shift > 31) return "bucket table size";
        for (size_t i = 0; i < t.slots.size(); i++)
            if (t.slots[i].key != kScan2EmptyKey && (scan2_pair_slot(t.slots[i].key, 0, t.slot_shift, t.slot_seed) | 1u) != ((uint32_t)i | 1u)) return "bucket placement";
        {
            const uint64_t kp4 = (uint64_t)t.kp * t.kp * t.kp * t.kp;
            for (const Scan2Slot& s : t.slots) if (s.key != kScan2EmptyKey && s.key >= kp4) return "bucket key";
            for (const Scan2Slot& s : t.more) if (s.key != kScan2EmptyKey && s.key >= kp4) return "bucket list key";
        }
        if (t.hashed ? (t.hash_shift < 1 || t.hash_shift > 31 || t.filter_bits != (1u << (32 - t.hash_shift)))
                     : (uint64_t)t.kp * t.kp * t.kp * t.kp > t.filter_bits) return "scan2 filter size";
        if (!t.short3.empty() && t.short3.size() < (uint64_t)t.kp * t.kp * t.kp) return "scan2 short3 size";
        if (!t.short3_big.empty() && t.short3_big.size() != t.short3.size()) return "scan2 short3_big size";
        if (t.shorts_packed.size() != t.shorts.size() * 3) return "scan2 short records";
        for (uint8_t id : t.short3) if (id != 255 && id >= t.shorts.size()) return "scan2 short record id";
        for (uint32_t id : t.short3_big) if (id >= t.shorts.size()) return "scan2 short record id";
        for (uint32_t w : t.shorts_packed) if (w && ((w & 0x0FFFFFFFu) >= n_terms || (w >> 28) > 3)) return "scan2 short record";
        if (const char* why = slots_ok(t.slots, t.more, t.slot_shift, t.term_blob, t.term_off)) return why;
    }
    if (u.supported) {
        if (u.G == 0 || u.G > kScan3Groups) return "scan3 groups";
        const uint64_t G3 = (uint64_t)u.G * u.G * u.G;
        for (int b = 0; b < 256; b++) if (u.cls[b] >= u.G || u.cls_fold[b] >= u.G) return "scan3 byte group";
        if (u.filter.size() != (size_t)((G3 * u.G + 31) / 32)) return "scan3 filter size";
        if (!u.short3.empty() && (u.short3.size() < G3 || u.short3.size() % 16)) return "scan3 short3 size";
        if (!u.short3_big.empty() && u.short3_big.size() != u.short3.size()) return "scan3 short3_big size";
        if (u.srec.size() % kScan3RecWords || u.srec.empty() || u.srec.size() / kScan3RecWords > kScan3RecLds + 1) return "scan3 records";
        for (uint8_t id : u.short3) if (id != 255 && id >= u.srec.size() / kScan3RecWords) return "scan3 record id";
        for (size_t i = 0; i < u.short3.size(); i++) if (u.short3[i] == 255 && (u.short3_big.empty() || u.short3_big[i] >= u.srec_big.size())) return "scan3 big record";
        for (size_t i = 0; i < u.srec.size(); i += 2) if (u.srec[i] && ((u.srec[i] & 0x0FFFFFFFu) >= n_terms || (u.srec[i] >> 28) > 3)) return "scan3 record entry";
        for (size_t at = 0; at < u.srec_big.size();) {
            const uint64_t n = u.srec_big[at];
            if (at + 1 + 2 * n > u.srec_big.size()) return "scan3 big record length";
            for (uint64_t j = 0; j < n; j++) { const uint32_t w = u.srec_big[at + 1 + 2 * j]; if (w && ((w & 0x0FFFFFFFu) >= n_terms || (w >> 28) > 3)) return "scan3 big record entry"; }
            at += 1 + 2 * n;
        }
        if (u.bloom_lg < 1 || u.bloom_lg > 28 || u.bloom.size() != ((size_t)1 << u.bloom_lg)) return "scan3 bloom size";
        if (const char* why = slots_ok(u.slots, u.more, u.slot_shift, u.term_blob, u.term_off)) return why;
    }
    return nullptr;
}
}  // namespace

void write_tables(const TableSet& ts, uint32_t flags, std::vector<uint8_t>& out) {
    Writer w;
    w.u32(kTablesMagic); w.u32(kTablesVersion); w.u32((uint32_t)sizeof(Scan2Slot)); w.u32(kScan2FptSize); w.u32(flags);
    const AcTables& a = ts.tab;
    w.u64(a.terms.size());
    for (const auto& t : a.terms) { w.u64(t.size()); w.raw(t.data(), t.size()); }
    w.u32(a.n_classes); w.raw(a.byte_class, 256); w.u32(a.n_states); w.u32(a.max_term_len);
    w.vec(a.delta); w.vec(a.out_term); w.vec(a.out_link); w.vec(a.term_len); w.vec(a.depth); w.vec(a.fail);
    w.vec(a.child_begin); w.vec(a.in_class);
    const Scan2Tables& t = ts.s2;
    w.u32(t.supported ? 1 : 0); w.u32(t.kp); w.u32(t.pad_class); w.u32(t.hashed ? 1 : 0); w.u32(t.filter_bits); w.u32(t.hash_shift);
    w.vec(t.filter); w.vec(t.short3); w.vec(t.shorts); w.vec(t.short3_big); w.vec(t.shorts_packed); w.u32(t.fpt_lg); w.vec(t.fpt);
    w.u32(t.slot_shift); w.u32(t.slot_seed); w.vec(t.slots); w.vec(t.more);
    w.raw(t.cls, 256); w.raw(t.cls_fold, 256); w.vec(t.term_blob); w.vec(t.term_off); w.u64(t.n_keys);
    const Scan3Tables& u = ts.s3;
    w.u32(u.supported ? 1 : 0); w.u32(u.G); w.u32(u.grouped ? 1 : 0); w.raw(u.cls, 256); w.raw(u.cls_fold, 256);
    w.vec(u.filter); w.vec(u.short3); w.vec(u.srec); w.vec(u.short3_big); w.vec(u.srec_big); w.u32(u.bloom_lg); w.vec(u.bloom);
    w.u32(u.slot_shift); w.u32(u.slot_seed); w.vec(u.slots); w.vec(u.more); w.vec(u.term_blob); w.vec(u.term_off);
    w.u64(u.n_keys); w.u64(u.n_anchors);
    uint64_t sum = 1469598103934665603ull;          // FNV-1a over everything before it
    for (uint8_t c : w.b) { sum ^= c; sum *= 1099511628211ull; }
    w.u64(sum);
    out = std::move(w.b);
}

int read_tables(const uint8_t* blob, uint64_t len, TableSet& out, uint32_t& out_flags, std::string& err) {
    auto fail = [&](int code, const std::string& msg) { err = msg; return code; };
    if (len < 28) return fail(GFT_E_INVALID, "table blob too short");
    uint64_t sum = 1469598103934665603ull, stored;
    for (uint64_t i = 0; i + 8 < len; i++) { sum ^= blob[i]; sum *= 1099511628211ull; }
    memcpy(&stored, blob + len - 8, 8);
    if (sum != stored) return fail(GFT_E_INVALID, "table blob is corrupt (checksum)");
    Reader r{blob, len - 8};
    if (r.u32() != kTablesMagic) return fail(GFT_E_INVALID, "not a gft table blob");
    if (r.u32() != kTablesVersion || r.u32() != sizeof(Scan2Slot) || r.u32() != kScan2FptSize)
        return fail(GFT_E_UNSUPPORTED, "table blob was written by another library version");
    const uint32_t flags = r.u32();
    TableSet ts;
    AcTables& a = ts.tab;
    const uint64_t nt = r.u64();
    if (!r.ok || nt > len) return fail(GFT_E_INVALID, "table blob is truncated");
    a.terms.resize((size_t)nt);
    for (auto& t : a.terms) {
        const uint64_t k = r.u64();
        if (!r.ok || k > r.n - r.i) return fail(GFT_E_INVALID, "table blob is truncated");
        t.assign((const char*)r.p + r.i, (size_t)k);
        r.i += k;
    }
    a.n_classes = r.u32(); r.raw(a.byte_class, 256); a.n_states = r.u32(); a.max_term_len = r.u32();
    r.vec(a.delta); r.vec(a.out_term); r.vec(a.out_link); r.vec(a.term_len); r.vec(a.depth); r.vec(a.fail);
    r.vec(a.child_begin); r.vec(a.in_class);
    Scan2Tables& t = ts.s2;
    t.supported = r.u32() != 0; t.kp = r.u32(); t.pad_class = r.u32(); t.hashed = r.u32() != 0; t.filter_bits = r.u32(); t.hash_shift = r.u32();
    r.vec(t.filter); r.vec(t.short3); r.vec(t.shorts); r.vec(t.short3_big); r.vec(t.shorts_packed); t.fpt_lg = r.u32(); r.vec(t.fpt);
    t.slot_shift = r.u32(); t.slot_seed = r.u32(); r.vec(t.slots); r.vec(t.more);
    r.raw(t.cls, 256); r.raw(t.cls_fold, 256); r.vec(t.term_blob); r.vec(t.term_off); t.n_keys = r.u64();
    Scan3Tables& u = ts.s3;
    u.supported = r.u32() != 0; u.G = r.u32(); u.grouped = r.u32() != 0; r.raw(u.cls, 256); r.raw(u.cls_fold, 256);
    r.vec(u.filter); r.vec(u.short3); r.vec(u.srec); r.vec(u.short3_big); r.vec(u.srec_big); u.bloom_lg = r.u32(); r.vec(u.bloom);
    u.slot_shift = r.u32(); u.slot_seed = r.u32(); r.vec(u.slots); r.vec(u.more); r.vec(u.term_blob); r.vec(u.term_off);
    u.n_keys = r.u64(); u.n_anchors = r.u64();
    if (!r.ok || r.i != r.n) return fail(GFT_E_INVALID, "table blob is truncated");
    // shape checks first: validate_tables indexes the tables by each other's sizes
    if (a.n_classes == 0 || a.n_classes > 256 || a.delta.size() != (size_t)a.n_states * a.n_classes || a.out_term.size() != a.n_states ||
        a.out_link.size() != a.n_states || a.term_len.size() != a.terms.size() ||
        (t.supported && (t.fpt_lg > 28 || t.fpt.size() != (t.fpt_lg ? (size_t)1 << t.fpt_lg : (size_t)kScan2FptSize) || t.slots.size() != ((size_t)1 << (32 - t.slot_shift)) || t.term_off.size() != a.terms.size() + 1 ||
                         t.filter.size() * 32 != t.filter_bits)))
        return fail(GFT_E_INVALID, "table blob is inconsistent");
    if (const char* why = validate_tables(a, t, u)) return fail(GFT_E_INVALID, std::string("table blob is inconsistent: ") + why);
    if (!t.supported) t.why_not = "not supported by the suffix-window kernel (imported tables)";
    // (a dictionary whose suffix-window set is not serialised as complete -- more than 32 byte classes -- gets its long-term
    // tables from the compiler again: a blob only ever holds what validate_tables checks)
    if (!t.supported) build_scan2_tables(a, t);
    else t.long_ok = true;
    out = std::move(ts);
    out_flags = flags;
    return GFT_OK;
}

// ---- the scan kernel ---------------------------------------------------------------------------------------------------
Forced parse_forced(const char* v) {
    if (!v || !*v || !std::strcmp(v, "auto")) return Forced::none;
    for (int k = 0; k < 5; k++)
        if (!std::strcmp(v, kScanKernelName[k])) return (Forced)(k + 1);     // (ScanKernel's order)
    return Forced::unknown;
}

namespace {
// Does scan5 apply to the compiled tables?  It runs on scan2's long-term tables; a fifo entry of 32 bits holds term id and
// relative position.  With more than 32 byte classes there is no direct short-term table
// (Scan2Tables::short_direct): the group-indexed one of scan3's tables serves then (GFT_SCAN5_LARGE=0 leaves such
// dictionaries to scan3).  true: its LDS plan and the shape of its fifo entries and Bloom level are in `p`; false: `p` is
// untouched.
bool plan_scan5(const TableSet& ts, const ScanOptions& opt, size_t lds_max, ScanPlan& p) {
    const AcTables& tab = ts.tab;
    const Scan2Tables& s2 = ts.s2;
    const Scan3Tables& s3 = ts.s3;
    ScanPlan q = p;
    const bool large = !s2.short_direct && s3.supported && opt.scan5_large;
    if (!s2.long_ok || !(s2.supported || large)) return false;
    uint32_t tb = 1;
    while ((1ull << tb) < tab.terms.size()) tb++;
    q.s5_term_bits = tb;
    q.s5_pos_bias = tab.max_term_len + kScan2MaxOff;
    const bool packs = (uint64_t)kScan2UnitMax + q.s5_pos_bias + 8 < (1ull << (32 - tb));
    const uint32_t short_bytes = large ? (uint32_t)s3.short3.size() : (uint32_t)s2.short3.size();
    const uint32_t rec_words = large ? (uint32_t)s3.srec.size() : (uint32_t)std::min<size_t>(s2.shorts_packed.size(), 255 * 3);
    // a fingerprint table too large for LDS (fpt_lg != 0) gets a Bloom level there instead: 2^lg bits, as large as
    // GFT_SCAN5_BLOOM_KB allows but not more than eight bits per item would take
    q.s5_bloom_lg = 0;
    if (s2.fpt_lg && opt.scan5_bloom_kb) {
        uint32_t lg = 13;
        while ((2u << lg) / 8 <= opt.scan5_bloom_kb * 1024u && (1ull << lg) < 8 * s2.n_keys) lg++;
        q.s5_bloom_lg = lg;
    }
    bool fits = false;
    for (int attempt = 0; attempt < 2 && packs && !fits; attempt++) {
        const uint32_t in_lds = s2.fpt_lg ? (q.s5_bloom_lg ? (1u << q.s5_bloom_lg) / 8 : 0u) : kScan2FptSize;
        fits = scan5_plan(s2.kp, short_bytes, rec_words, in_lds, lds_max - 512, opt.scan5_fifo ? opt.scan5_fifo : kScan2FifoCap, &q.s5plan);
        if (!fits) q.s5_bloom_lg = 0;                      // (no room: without the Bloom level)
    }
    if (!fits) return false;
    if (opt.scan5_groups && opt.scan5_groups < q.s5plan.G) {      // (tests: more merging than LDS asks for)
        q.s5plan.G = std::max<uint32_t>(opt.scan5_groups, 2);
        q.s5plan.dual_entries = q.s5plan.G * q.s5plan.G * q.s5plan.G;
    }
    q.s5_short_groups = large;
    p = q;
    return true;
}
}  // namespace

int plan_scan(const TableSet& ts, const ScanOptions& opt, size_t lds_max, bool extra_kernels, ScanPlan& out, std::string& err) {
    const AcTables& tab = ts.tab;
    const Scan2Tables& s2 = ts.s2;
    const Scan3Tables& s3 = ts.s3;
    auto fail = [&](int code, const std::string& msg) { err = msg; return code; };
    if (tab.max_term_len + 1024 > kTextBuf)
        return fail(GFT_E_UNSUPPORTED, "keyword longer than " + std::to_string(kTextBuf - 1024) + " bytes");
    if (tab.n_states >= 0x7FFFFFFFu) return fail(GFT_E_UNSUPPORTED, "automaton too large");
    const size_t fixed = 256 + (size_t)(kScanBlockThreads / 64) * kTextBuf + 1024;
    if (lds_max < fixed + (size_t)tab.n_classes * 4)
        return fail(GFT_E_UNSUPPORTED, "device LDS too small for the scan kernel");
    ScanPlan p;
    size_t rows = (lds_max - fixed) / ((size_t)tab.n_classes * 4);
    p.n_lds_states = (uint32_t)std::min<size_t>(rows, tab.n_states);
    const Forced f = opt.forced;
    if (!extra_kernels && (f == Forced::scan2 || f == Forced::scan4))
        return fail(GFT_E_UNSUPPORTED, std::string("GFT_SCAN_KERNEL=") + kScanKernelName[(int)f - 1] + ": this library was built without the cross-check kernels (GFT_EXTRA_KERNELS=1 python -m gofindthem_amd.build --force)");
    const size_t lds = lds_max - 512;
    const uint32_t s2_filter = (uint32_t)s2.filter.size(), s2_short3 = (uint32_t)s2.short3.size(),
                   s2_recs = (uint32_t)std::min<size_t>(s2.shorts_packed.size(), 255 * 3), s2_fpt = s2.fpt_lg ? 0u : kScan2FptSize;
    uint32_t w2 = 0, w3 = 0, w4[2] = {0, 0};
    const bool k2_fits = s2.supported && scan2_plan(s2_filter, s2_short3, s2_recs, s2_fpt, lds, &w2, &p.scan2_cand_cap);
    // (scan4's fifo capacities belong to the smaller of the two wave counts; with fewer waves there is only more room)
    const bool k4_fits = s2.supported && scan4_plan(s2_filter, s2_short3, s2_recs, s2_fpt, lds, false, &w4[0], &p.scan4_fifo[0]) &&
                         scan4_plan(s2_filter, s2_short3, s2_recs, s2_fpt, lds, true, &w4[1], &p.scan4_fifo[1]);
    const bool k5_fits = (f == Forced::none || f == Forced::scan5) && plan_scan5(ts, opt, lds_max, p);
    const uint32_t bloom_lds_bytes = s3.supported && s3.bloom_lg <= kScan3BloomLdsLg ? 4u << s3.bloom_lg : 0u;
    const bool k3_fits = s3.supported && scan3_plan((uint32_t)s3.filter.size(), (uint32_t)s3.short3.size(), (uint32_t)s3.srec.size(),
                                                        bloom_lds_bytes, lds, &w3, &p.scan3_cand_cap);
    // (scan5 asked for but not applicable: as by default)
    auto chosen = [&](ScanKernel k, uint32_t waves) { p.kernel = k; p.scan_waves = waves; out = p; return (int)GFT_OK; };
    if (k3_fits && f != Forced::dfa && f != Forced::scan2 && f != Forced::scan4 && (f == Forced::scan3 || !(k5_fits || k2_fits)))
        return chosen(ScanKernel::scan3, w3);
    if (f == Forced::scan4 && k2_fits && k4_fits) return chosen(ScanKernel::scan4, std::min(w4[0], w4[1]));
    if (k5_fits) return chosen(ScanKernel::scan5, kScan5Waves);
    if (k2_fits && f != Forced::dfa) return chosen(ScanKernel::scan2, w2);
    return chosen(ScanKernel::dfa, 0);
}

void derive_scan5(const TableSet& ts, const ScanPlan& plan, Scan5Tables& s5, std::vector<uint32_t>& bloom) {
    const Scan2Tables& s2 = ts.s2;
    build_scan5_tables(ts.tab, s2, plan.s5plan.G, s5);
    bloom.clear();
    if (plan.s5_bloom_lg) {
        // one bit per owner of a fingerprint cell, read off the bucket table: (window key, byte in front of the
        // window with its case bit cleared), or the window key alone where the window is the term's first four bytes
        bloom.assign((size_t)1 << (plan.s5_bloom_lg - 5), 0u);
        auto set = [&](uint32_t h) { bloom[h >> 5] |= 1u << (h & 31); };
        auto add = [&](const Scan2Slot& t) {
            if ((t.len & kScan2LenMask) == 4) set(scan5_bloom_x(t.key, plan.s5_bloom_lg));
            else set(scan5_bloom_g(t.key, (t.front[0] >> 24) & 0xDFu, plan.s5_bloom_lg));
        };
        for (const Scan2Slot& sl : s2.slots) {
            if (sl.key == kScan2EmptyKey) continue;
            if (!(sl.info & kScan2Multi)) { add(sl); continue; }
            for (uint32_t j = 0; j < sl.len; j++) add(s2.more[(sl.info & ~kScan2Multi) + j]);
        }
    }
}

}  // namespace gft

