// program_set.cpp -- the solver's program compiler (program_set.hpp): host arithmetic only, no device and no handle.
#include "program_set.hpp"

#include <algorithm>
#include <cstdio>

#include "../../include/gft.h"
#include "gft_kernels.hpp"

namespace gft {

// validates one postfix program and measures its stack needs.  A program beyond the device solver's limits is not refused
// but marked (it is solved on the host), and the slots of its multi-leaf INORD groups are listed
int check_program(const uint32_t* w, uint64_t len, uint32_t n_slots, uint32_t idx, ProgramTraits& traits, std::string& err) {
    uint32_t sp = 0, psp = 0, g_tot = 0, g_psp = 0, max_sp = 0;   // g_*: the most pairs / the deepest pair stack of the group being read
    std::vector<uint32_t> group_slots;
    std::vector<uint32_t> pcnt;   // pair counts of the INORD operand stack
    bool in_group = false;
    auto bad = [&](const char* m) {
        err = "program " + std::to_string(idx) + ": " + m;
        return (int)GFT_E_INVALID;
    };
    for (uint64_t pc = 0; pc < len; pc++) {
        const uint32_t op = w[pc] >> 28;
        const bool fl = (w[pc] & GFT_INORD_FLAG) != 0;
        switch (op) {
        case GFT_OP_UNIT:
            if ((w[pc] & GFT_SLOT_MASK) >= n_slots) return bad("slot out of range");
            sp++;
            if (fl) { pcnt.push_back(1); in_group = true; group_slots.push_back(w[pc] & GFT_SLOT_MASK); }
            break;
        case GFT_OP_AND:
        case GFT_OP_OR:
            if (sp < 2) return bad("operand stack underflow");
            sp--;
            if (fl) {
                if (pcnt.size() < 2) return bad("INORD operand stack underflow");
                uint32_t r = pcnt.back(); pcnt.pop_back();
                if (op == GFT_OP_AND) pcnt.back() = r; else pcnt.back() += r;
            }
            break;
        case GFT_OP_NOT:
            if (sp < 1) return bad("operand stack underflow");
            if (in_group) return bad("NOT inside INORD");
            break;
        case GFT_OP_INORD:
            if (sp < 1 || pcnt.size() != 1) return bad("malformed INORD group");
            pcnt.clear(); in_group = false;
            if ((g_tot > kMaxPairs || g_psp > kMaxPairDepth) && g_tot <= kMaxPairsWide && g_psp <= kMaxPairDepthWide)
                traits.wide_pairs = std::max(traits.wide_pairs, g_tot);
            g_tot = g_psp = 0;
            // (a group of ONE leaf is true exactly when the leaf is present: no position is ever compared)
            if (group_slots.size() > 1) traits.inord_slots.insert(traits.inord_slots.end(), group_slots.begin(), group_slots.end());
            group_slots.clear();
            break;
        default:
            return bad("unknown opcode");
        }
        // (the depth of the PUBLIC postfix form binds nobody; compile_programs judges the depth of the fused form, which is
        // what the device interprets: operands are reordered there, a chain nested to one side is flat)
        max_sp = std::max(max_sp, sp);
        uint32_t tot = 0;
        for (uint32_t c : pcnt) tot += c;
        psp = (uint32_t)pcnt.size();
        g_tot = std::max(g_tot, tot); g_psp = std::max(g_psp, psp);
        // (more than a pair per lane: the device's scratch path up to kMaxPairsWide, the host beyond)
        if (tot > kMaxPairsWide || psp > kMaxPairDepthWide) traits.over_limit = true;
    }
    if (sp != 1 || !pcnt.empty()) return bad("program does not reduce to one value");
    if (traits.wide_pairs && max_sp > kMaxPairDepthWide) traits.over_limit = true;   // (the wide evaluator's boolean stack: a bit per entry)
    std::sort(traits.inord_slots.begin(), traits.inord_slots.end());
    traits.inord_slots.erase(std::unique(traits.inord_slots.begin(), traits.inord_slots.end()), traits.inord_slots.end());
    return GFT_OK;
}

// public postfix words -> fused words (gft_kernels.hpp FusedOp) + INORD group table; returns the deepest the accumulator
// stack gets.  `gbase` = offset of this program inside the uploaded public word array.
uint32_t fuse_program(const uint32_t* w, uint64_t len, uint64_t gbase, std::vector<uint32_t>& out,
                      std::vector<uint32_t>& groups) {
    // postfix -> tree (node = operator or leaf, with the range of public words it covers)
    struct Node { uint32_t op, slot; int64_t l, r; uint64_t s, e; };
    std::vector<Node> nodes;
    std::vector<int64_t> st;
    for (uint64_t i = 0; i < len; i++) {
        const uint32_t op = w[i] >> 28;
        switch (op) {
        case GFT_OP_UNIT:
            nodes.push_back(Node{op, w[i] & GFT_SLOT_MASK, -1, -1, i, i});
            st.push_back((int64_t)nodes.size() - 1);
            break;
        case GFT_OP_AND:
        case GFT_OP_OR: {
            const int64_t r = st.back(); st.pop_back();
            const int64_t l = st.back(); st.pop_back();
            nodes.push_back(Node{op, 0, l, r, nodes[l].s, i});
            st.push_back((int64_t)nodes.size() - 1);
            break;
        }
        case GFT_OP_NOT:
        case GFT_OP_INORD: {
            const int64_t c = st.back(); st.pop_back();
            nodes.push_back(Node{op, 0, c, -1, nodes[c].s, i});
            st.push_back((int64_t)nodes.size() - 1);
            break;
        }
        default:
            break;
        }
    }
    if (st.empty()) return 0;
    const size_t out0 = out.size();
    // Code generation with an explicit job stack (left-deep chains of 10 000 leaves must not recurse).
    //  * NOT is pushed down to the leaves (De Morgan; every node is evaluated anyway, the reference does not
    //    short-circuit), so it only survives on top of an INORD group;
    //  * AND / OR commute: the operand that is a leaf goes second and folds into the operator word;
    //  * the accumulator is pushed only between two operands that are both subtrees -- and of those the one that needs
    //    the deeper stack goes FIRST (Sethi-Ullman), so a chain of parentheses nested to the right stays one entry deep
    //    and only a balanced tree of 2^k subtrees gets k deep: real rule sets fit the interpreter's register stack.
    auto strip = [&](int64_t n, bool& neg) {        // skip NOT chains
        while (nodes[n].op == GFT_OP_NOT) { neg = !neg; n = nodes[n].l; }
        return n;
    };
    std::vector<uint32_t> need(nodes.size(), 0);    // stack entries the subtree's code needs (children come before parents)
    for (size_t n = 0; n < nodes.size(); n++) {
        const Node& nd = nodes[n];
        bool dummy = false;
        if (nd.op == GFT_OP_NOT || nd.op == GFT_OP_INORD) need[n] = need[nd.l];
        else if (nd.op == GFT_OP_AND || nd.op == GFT_OP_OR) {
            const int64_t l = strip(nd.l, dummy), r = strip(nd.r, dummy);
            if (nodes[r].op == GFT_OP_UNIT) need[n] = need[nd.l];
            else if (nodes[l].op == GFT_OP_UNIT) need[n] = need[nd.r];
            else need[n] = need[nd.l] == need[nd.r] ? need[nd.l] + 1 : std::max(need[nd.l], need[nd.r]);
        }
    }
    struct Job { int64_t n; int phase; bool neg; };
    std::vector<Job> jobs{{st.back(), 0, false}};
    uint32_t depth = 0, max_depth = 0;
    while (!jobs.empty()) {
        Job j = jobs.back(); jobs.pop_back();
        bool neg = j.neg;
        const int64_t n = j.phase == 0 ? strip(j.n, neg) : j.n;
        const Node& nd = nodes[n];
        switch (nd.op) {
        case GFT_OP_UNIT:
            out.push_back((neg ? kFopSetN : kFopSet) << 28 | nd.slot);
            break;
        case GFT_OP_INORD:
            if (j.phase == 0) { jobs.push_back({n, 1, neg}); jobs.push_back({nd.l, 0, false}); }
            else {
                // (a group with a single leaf has a non-empty position list exactly when the leaf is present: every
                // reported key carries >= 1 position, so no position check is needed)
                if (nodes[nd.l].op != GFT_OP_UNIT) {
                    out.push_back(kFopInord << 28 | (uint32_t)(groups.size() / 2));
                    groups.push_back((uint32_t)(gbase + nodes[nd.l].s));
                    groups.push_back((uint32_t)(nodes[nd.l].e - nodes[nd.l].s + 1));
                }
                if (neg) out.push_back(kFopNot << 28);
            }
            break;
        case GFT_OP_AND:
        case GFT_OP_OR: {
            const bool is_and = (nd.op == GFT_OP_AND) != neg;        // not (a and b) == not a or not b
            if (j.phase == 0) {
                bool ln = neg, rn = neg;
                const int64_t l = strip(nd.l, ln), r = strip(nd.r, rn);
                if (nodes[r].op == GFT_OP_UNIT) { jobs.push_back({n, 1, neg}); jobs.push_back({nd.l, 0, neg}); }
                else if (nodes[l].op == GFT_OP_UNIT) { jobs.push_back({n, 2, neg}); jobs.push_back({nd.r, 0, neg}); }
                else {
                    const bool left_first = need[nd.l] >= need[nd.r];
                    jobs.push_back({n, 4, neg}); jobs.push_back({left_first ? nd.r : nd.l, 0, neg});
                    jobs.push_back({n, 3, neg}); jobs.push_back({left_first ? nd.l : nd.r, 0, neg});
                }
            } else if (j.phase == 1 || j.phase == 2) {
                bool ln = neg;
                const int64_t leaf = strip(j.phase == 1 ? nd.r : nd.l, ln);
                out.push_back((is_and ? (ln ? kFopAndNS : kFopAndS) : (ln ? kFopOrNS : kFopOrS)) << 28 | nodes[leaf].slot);
            } else if (j.phase == 3) {
                out.push_back(kFopPush << 28);
                max_depth = std::max(max_depth, ++depth);
            } else {
                out.push_back((is_and ? kFopAndPop : kFopOrPop) << 28);
                depth--;
            }
            break;
        }
        default:
            break;
        }
    }
    // a push is always followed by the first leaf of the next subtree: one word does both
    size_t k = out0;
    for (size_t i = out0; i < out.size(); i++) {
        const uint32_t op = out[i] >> 28, nx = i + 1 < out.size() ? out[i + 1] >> 28 : 0u;
        if (op == kFopPush && (nx == kFopSet || nx == kFopSetN)) {
            out[k++] = (nx == kFopSet ? kFopPushSet : kFopPushSetN) << 28 | (out[i + 1] & 0x0FFFFFFFu);
            i++;
        } else out[k++] = out[i];
    }
    out.resize(k);
    return max_depth;
}

int compile_programs(const uint32_t* prog_words, const uint64_t* prog_off, uint32_t n_exprs, uint32_t n_slots, ProgramSet& out,
                     std::string& err) {
    auto fail = [&](int code, const char* msg) { err = msg; return code; };
    // (slot n_slots itself is the solver's never-present slot: it must fit a program word's field too)
    if (n_slots > GFT_SLOT_MASK || n_slots >= (1u << kDwFieldBits)) return fail(GFT_E_UNSUPPORTED, "too many slots");
    std::vector<ProgramTraits> traits(n_exprs);
    for (uint32_t i = 0; i < n_exprs; i++) {
        if (prog_off[i + 1] < prog_off[i]) return fail(GFT_E_INVALID, "prog_off is not ascending");
        int rc = check_program(prog_words + prog_off[i], prog_off[i + 1] - prog_off[i], n_slots, i, traits[i], err);
        if (rc) return rc;
    }
    std::vector<uint32_t> w(prog_words, prog_words + (n_exprs ? prog_off[n_exprs] : 0));
    std::vector<uint64_t> o(prog_off, prog_off + (n_exprs ? n_exprs + 1 : 0));
    if (o.empty()) o.push_back(0);
    std::vector<uint32_t> fw, groups, fdepth;
    std::vector<uint64_t> fo(1, 0);
    for (uint32_t i = 0; i < n_exprs; i++) {
        if (traits[i].over_limit || traits[i].wide_pairs) {
            // beyond a limit of the device solver: the device evaluates a stand-in (one leaf on the never-present slot), the
            // expression itself is solved on the host from the scan's matches (host_solve.hpp) and its bit patched in.
            // An expression with a WIDE INORD group gets the same stand-in in the fused form: the solver's second phase
            // (gft_solve.hip wide_expr_doc) answers it from its public words, a document per wave
            const uint32_t stub = GFT_OP_UNIT << 28 | n_slots;
            fdepth.push_back(fuse_program(&stub, 1, 0, fw, groups));
        } else {
            const size_t fw0 = fw.size(), g0 = groups.size();
            uint32_t depth = fuse_program(prog_words + prog_off[i], prog_off[i + 1] - prog_off[i], prog_off[i], fw, groups);
            if (depth > kMaxBoolDepth) {
                // the fused form still nests deeper than the interpreter's stack (a balanced tree of 2^128 sub-trees would):
                // the host's
                fw.resize(fw0); groups.resize(g0);
                traits[i].over_limit = true;
                const uint32_t stub = GFT_OP_UNIT << 28 | n_slots;
                depth = fuse_program(&stub, 1, 0, fw, groups);
            }
            fdepth.push_back(depth);
        }
        while (fw.size() % 4) fw.push_back((uint32_t)kFopNop << 28);       // the interpreter reads 4-word chunks
        fo.push_back(fw.size());
    }
    // Evaluation order: inside every output tile (kSolveTileWords * 32 expressions) the programs are sorted by the
    // interpreter they need -- 2: nest deeper than its register stack, 1: use the stack, 0: flat (no push / pop at all,
    // half the work per word) -- and by length, and handed to the waves 64 at a time, so that the lanes of a wave run
    // loops of similar length on the cheapest interpreter that serves them all (longest first inside classes 2 and 1,
    // shortest first inside class 0: the block on the border mixes short programs of both).
    // order[i] = expression evaluated at sorted position i; blk_class[b] = the interpreter of block b.
    std::vector<uint32_t> order(n_exprs), blk_class, fprog_t, fblk_off, wave_blk;
    for (uint32_t i = 0; i < n_exprs; i++) order[i] = i;
    auto klass = [&](uint32_t x) { return fdepth[x] > kSolveRegStack ? 2u : fdepth[x] > 0 ? 1u : 0u; };
    auto plen = [&](uint32_t x) { return fo[x + 1] - fo[x]; };
    const uint32_t tile_exprs = kSolveTileWords * 32;
    constexpr uint32_t kWaves = kSolveBlockThreads / 64;
    for (uint32_t t0 = 0; t0 < n_exprs; t0 += tile_exprs) {
        const uint32_t t1 = std::min(n_exprs, t0 + tile_exprs);
        std::stable_sort(order.begin() + t0, order.begin() + t1, [&](uint32_t a, uint32_t b) {
            if (klass(a) != klass(b)) return klass(a) > klass(b);
            return klass(a) ? plen(a) > plen(b) : plen(a) < plen(b);
        });
        std::vector<uint64_t> cost;              // VALU work of a block, for the deal below
        for (uint32_t b0 = t0; b0 < t1; b0 += 64) {
            uint32_t cls = 0;
            uint64_t maxlen = 0;
            for (uint32_t i = b0; i < std::min(t1, b0 + 64); i++) {
                cls = std::max(cls, klass(order[i]));
                maxlen = std::max(maxlen, plen(order[i]));
            }
            blk_class.push_back(cls);
            cost.push_back(maxlen * (cls == 2 ? 40 : cls == 1 ? 26 : 14) + 160);
            // the block's chunks transposed: words 4c..4c+3 of lane l at off + (c * 64 + l) * 4
            if (fprog_t.size() + maxlen * 64 > 0xFFFFFFFFull) return fail(GFT_E_UNSUPPORTED, "program set too large");
            fblk_off.push_back((uint32_t)fprog_t.size());
            fprog_t.resize(fprog_t.size() + maxlen * 64, kDwNop);
            for (uint32_t i = b0; i < std::min(t1, b0 + 64); i++) {
                const uint64_t p0 = fo[order[i]], len = fo[order[i] + 1] - p0;
                for (uint64_t pc = 0; pc < len; pc++)
                    fprog_t[fblk_off.back() + ((pc / 4) * 64 + (i - b0)) * 4 + pc % 4] = fused_to_device(fw[p0 + pc]);
            }
        }
        // The deal: the tile's blocks go to the workgroup's waves sixteen at a time.  Wave w runs on SIMD w % 4 and the
        // four waves of a SIMD share its issue slots, so every round's blocks are dealt by cost, the most expensive
        // first, to the SIMD with the least work so far that still has a wave free (its lowest wave: the oldest wave of
        // a SIMD is served first, which suits the block everybody else ends up waiting for).
        // wave_blk[tile's first block + round * 16 + wave] = block (relative to the tile) or ~0.
        // (a full tile is 32 blocks = two rounds, so a tile's entries start at its first block's index)
        const uint32_t nblk = (uint32_t)cost.size();
        std::vector<uint32_t> by_cost(nblk);
        for (uint32_t b = 0; b < nblk; b++) by_cost[b] = b;
        for (uint32_t r0 = 0; r0 < nblk; r0 += kWaves) {
            const uint32_t r1 = std::min(nblk, r0 + kWaves);
            std::stable_sort(by_cost.begin() + r0, by_cost.begin() + r1, [&](uint32_t a, uint32_t b) { return cost[a] > cost[b]; });
            uint64_t load[4] = {0, 0, 0, 0};
            uint32_t used[4] = {0, 0, 0, 0};
            uint32_t deal[kWaves];
            for (uint32_t w = 0; w < kWaves; w++) deal[w] = 0xFFFFFFFFu;
            for (uint32_t k = r0; k < r1; k++) {
                int best = -1;
                for (int q = 0; q < 4; q++)
                    if (used[q] < kWaves / 4 && (best < 0 || load[q] < load[best])) best = q;
                deal[used[best] * 4 + best] = by_cost[k];
                used[best]++;
                load[best] += cost[by_cost[k]];
            }
            for (uint32_t w = 0; w < kWaves; w++) wave_blk.push_back(deal[w]);
        }
    }
    if (order.empty()) order.push_back(0);
    if (blk_class.empty()) blk_class.push_back(0);
    if (wave_blk.empty()) wave_blk.push_back(0xFFFFFFFFu);
    if (fblk_off.empty()) fblk_off.push_back(0);
    if (fprog_t.empty()) fprog_t.push_back(0);
    if (groups.size() / 2 > (1u << kDwFieldBits)) return fail(GFT_E_UNSUPPORTED, "too many INORD groups");
    // the kernel reads control bits, not opcodes (gft_kernels.hpp fused_to_device)
    std::vector<uint32_t> dw(fw.size());
    for (size_t i = 0; i < fw.size(); i++) dw[i] = fused_to_device(fw[i]);
    if (dw.empty()) dw.push_back(kDwNop);
    if (groups.empty()) groups.assign(2, 0);
    // what the host may have to solve (host_solve.hpp)
    ProgramSet ps;
    ps.inord_slot.assign((size_t)n_slots + 1, 0);
    for (uint32_t i = 0; i < n_exprs; i++) {
        if (traits[i].over_limit) ps.host_only.push_back(i);
        else if (!traits[i].inord_slots.empty()) {
            ps.inord_exprs.push_back(i);
            for (uint32_t sl : traits[i].inord_slots) ps.inord_slot[sl] = 1;
        }
    }
    std::vector<uint32_t> wide_list;                     // per wide expression: index, offset and length of its public words
    for (uint32_t i = 0; i < n_exprs; i++)
        if (!traits[i].over_limit && traits[i].wide_pairs) {
            ps.wide_pairs = std::max(ps.wide_pairs, traits[i].wide_pairs);
            if (prog_off[i + 1] > 0xFFFFFFFFull) return fail(GFT_E_UNSUPPORTED, "program set too large");
            wide_list.push_back(i); wide_list.push_back((uint32_t)prog_off[i]); wide_list.push_back((uint32_t)(prog_off[i + 1] - prog_off[i]));
        }
    ps.n_wide = (uint32_t)(wide_list.size() / 3);
    ps.fprog_words = (uint32_t)fw.size();
    for (uint32_t w : fw) {
        ps.n_inord_groups += (w >> 28) == kFopInord;
        ps.n_rare_words += (w >> 28) == kFopInord || (w >> 28) == kFopNot;
    }
    ps.n_inord_groups += ps.n_wide;                      // (their groups read positions too: the scan must write them)
    ps.n_exprs = n_exprs; ps.n_slots = n_slots;
    ps.prog = std::move(w); ps.prog_off = std::move(o);
    ps.fprog = std::move(dw); ps.fprog_off = std::move(fo); ps.groups = std::move(groups);
    ps.order = std::move(order); ps.blk_class = std::move(blk_class); ps.wave_blk = std::move(wave_blk);
    ps.fprog_t = std::move(fprog_t); ps.fblk_off = std::move(fblk_off); ps.wide_list = std::move(wide_list);
    ps.fdepth = std::move(fdepth);
    out = std::move(ps);                                 // (a refusal above has left `out` as it was)
    return GFT_OK;
}

// the GFT_SOLVE_DEBUG line of gft_set_programs: what the fused programs are made of
void print_program_stats(const ProgramSet& ps) {
    // (the fused opcode of a device word: fused_to_device keeps every opcode's control bits apart; 4 is no opcode)
    auto fused_op = [](uint32_t dw) {
        for (uint32_t op = 1; op <= 15; op++)
            if (op != 4 && fused_to_device(op << 28) == (dw & ~kDwFieldMask)) return op;
        return 0u;
    };
    const std::vector<uint64_t>& fo = ps.fprog_off;
    uint64_t hist[16] = {0}, with_rare = 0, maxlen = 0;
    for (uint32_t i = 0; i < ps.n_exprs; i++) {
        bool rare = false;
        for (uint64_t k = fo[i]; k < fo[i + 1]; k++) { const uint32_t op = fused_op(ps.fprog[k]); hist[op]++; rare |= op >= kFopAndPop; }
        with_rare += rare;
        maxlen = std::max<uint64_t>(maxlen, fo[i + 1] - fo[i]);
    }
    fprintf(stderr, "[gft solve debug] %u programs, %zu fused words (max %llu); programs with stack/not/inord ops: %llu; ops:",
            ps.n_exprs, (size_t)ps.fprog_words, (unsigned long long)maxlen, (unsigned long long)with_rare);
    for (int k = 1; k <= 15; k++) fprintf(stderr, " %d:%llu", k, (unsigned long long)hist[k]);
    fprintf(stderr, "\n");
}

}  // namespace gft
