// gft_multi.cpp -- multi-device handles: one process, one host thread + stream per device, tables
// replicated, contiguous document ranges of near-equal text bytes, and -- for device-resident shards -- one RCCL gather of
// the bitmaps to the first device.  The Go side keeps calling finder.NewFinder(&GpuEngine{...}): the
// fan-out lives behind the same gft_engine handle.
#include "gft_engine.hpp"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <cstdlib>
#include <thread>

using namespace gft;
using namespace gft::api;

namespace {

// RCCL is bound at run time (dlopen): libgft.so itself does not depend on it, and a process that already carries a
// copy (PyTorch does) shares that one
struct RcclApi {
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    void* lib = nullptr;
    bool ok() const { return CommInitAll && CommDestroy && GroupStart && GroupEnd && Send && Recv && GetErrorString; }
};
RcclApi& rccl_api() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char* name : {"librccl.so.1", "librccl.so"}) {
            api.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (api.lib) break;
        }
        if (!api.lib) return;
        api.CommInitAll = (decltype(api.CommInitAll))dlsym(api.lib, "ncclCommInitAll");
        api.CommDestroy = (decltype(api.CommDestroy))dlsym(api.lib, "ncclCommDestroy");
        api.GroupStart = (decltype(api.GroupStart))dlsym(api.lib, "ncclGroupStart");
        api.GroupEnd = (decltype(api.GroupEnd))dlsym(api.lib, "ncclGroupEnd");
        api.Send = (decltype(api.Send))dlsym(api.lib, "ncclSend");
        api.Recv = (decltype(api.Recv))dlsym(api.lib, "ncclRecv");
        api.GetErrorString = (decltype(api.GetErrorString))dlsym(api.lib, "ncclGetErrorString");
    });
    return api;
}

std::vector<gft_engine*> all_engines(gft_engine* e) {
    std::vector<gft_engine*> v{e};
    v.insert(v.end(), e->peers.begin(), e->peers.end());
    return v;
}

// behind a call that every device ran its share of: device 0's own verdict is this handle's, the peers' are OR-ed in
void or_peer_verdicts(gft_engine* e) {
    for (gft_engine* g : e->peers) e->reported.nonascii = e->reported.nonascii || g->reported.nonascii;
}

// contiguous document ranges of near-equal text bytes: device i owns documents [cut[i], cut[i+1])
void split_by_bytes(const uint64_t* doc_off, uint64_t n_docs, size_t n, std::vector<uint64_t>& cut) {
    cut.assign(n + 1, n_docs);
    cut[0] = 0;
    const uint64_t base = n_docs ? doc_off[0] : 0, total = n_docs ? doc_off[n_docs] - base : 0;
    for (size_t i = 1; i < n; i++) {
        const uint64_t target = base + (uint64_t)((unsigned __int128)total * i / n);
        uint64_t c = (uint64_t)(std::lower_bound(doc_off, doc_off + n_docs + 1, target) - doc_off);
        cut[i] = std::min(std::max(c, cut[i - 1]), n_docs);
    }
}

// run f(i, engine_i) for every device, each on its own host thread (the caller's thread takes device 0); the first
// failure's code and message become the handle's
template <class F>
int fan_out(gft_engine* e, F f) {
    const std::vector<gft_engine*> eng = all_engines(e);
    std::vector<int> rc(eng.size(), GFT_OK);
    std::vector<std::thread> th;
    th.reserve(eng.size());
    {
        JoinAll joined(th);                  // (also when a thread could not be started, or device 0's share threw)
        // a thread's body never lets an exception out (that would be std::terminate): it becomes the device's status
        auto guarded = [&](size_t i) noexcept {
            try { rc[i] = f(i, eng[i]); } catch (...) { rc[i] = translate_exception(&eng[i]->err); }
        };
        struct InMulti { gft_engine* e; explicit InMulti(gft_engine* e_) : e(e_) { e->in_multi = true; } ~InMulti() { e->in_multi = false; } };
        for (size_t i = 1; i < eng.size(); i++) th.emplace_back(guarded, i);
        InMulti im(e);
        guarded(0);
    }
    for (size_t i = 0; i < eng.size(); i++)
        if (rc[i]) {
            if (i) e->err = "device " + std::to_string(eng[i]->device) + ": " + eng[i]->err;
            return rc[i];
        }
    return GFT_OK;
}

}  // namespace

namespace gft::api {

void destroy_multi(gft_engine* e) {
    if (!e->comms.empty() && rccl_api().ok())
        for (void* c : e->comms) (void)rccl_api().CommDestroy((ncclComm_t)c);
    e->comms.clear();
    for (gft_engine* p : e->peers) gft_engine_destroy(p);
    e->peers.clear();
}

static int replicate_tables(gft_engine* e, uint32_t flags) {
    // the compiled tables are copied, not compiled again; every device uploads its own copy
    std::vector<std::thread> th;
    std::vector<int> rc(e->peers.size(), GFT_OK);
    th.reserve(e->peers.size());
    {
        JoinAll joined(th);
        for (size_t i = 0; i < e->peers.size(); i++)
            th.emplace_back([&, i]() noexcept {
                gft_engine* p = e->peers[i];
                try {
                    GFT_LOCK(p);
                    TableSet copy = e->tables;
                    rc[i] = install_tables(p, std::move(copy), flags);
                } catch (...) { rc[i] = translate_exception(&p->err); }
            });
    }
    for (size_t i = 0; i < rc.size(); i++)
        if (rc[i]) { e->err = "device " + std::to_string(e->peers[i]->device) + ": " + e->peers[i]->err; return rc[i]; }
    return GFT_OK;
}

int multi_build(gft_engine* e, const uint8_t* terms_blob, const uint64_t* term_off, uint32_t n_terms, uint32_t flags) {
    e->in_multi = true;
    const int rc = gft_build(e, terms_blob, term_off, n_terms, flags);
    e->in_multi = false;
    return rc ? rc : replicate_tables(e, flags);
}

int multi_import_tables(gft_engine* e, const uint8_t* blob, uint64_t len) {
    e->in_multi = true;
    const int rc = gft_import_tables(e, blob, len);
    e->in_multi = false;
    return rc ? rc : replicate_tables(e, e->build_flags);
}

int multi_set_programs(gft_engine* e, const uint32_t* prog_words, const uint64_t* prog_off, uint32_t n_exprs, uint32_t n_extra) {
    return fan_out(e, [&](size_t, gft_engine* g) { return gft_set_programs(g, prog_words, prog_off, n_exprs, n_extra); });
}

// caller-supplied matches of the documents [a, b): the same arrays, offsets rebased
struct ExtraSlice {
    std::vector<uint64_t> off;
    gft_extra_matches x{nullptr, nullptr, nullptr};
    const gft_extra_matches* ptr = nullptr;
    void set(const gft_extra_matches* extra, uint64_t a, uint64_t b) {
        if (!(extra && extra->off)) return;
        off.assign(extra->off + a, extra->off + b + 1);
        const uint64_t base = off[0];
        for (auto& o : off) o -= base;
        x.off = off.data(); x.slot = extra->slot + base; x.pos = extra->pos + base;
        ptr = &x;
    }
};

int multi_process(gft_engine* e, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags,
                  const gft_extra_matches* extra, uint32_t* hit_bitmap) {
    const size_t n = e->peers.size() + 1;
    // (an empty batch may come without offsets, as on a single device: every shard then is [0, 0) of this one entry)
    static const uint64_t kNoDocs[1] = {0};
    if (n_docs == 0) doc_off = kNoDocs;
    split_by_bytes(doc_off, n_docs, n, e->shard_cut);
    const uint64_t words = (e->n_exprs + 31) / 32;
    e->reported.nonascii = false;
    const int rc = fan_out(e, [&](size_t i, gft_engine* g) {
        const uint64_t a = e->shard_cut[i], b = e->shard_cut[i + 1];
        std::vector<uint64_t> off(doc_off + a, doc_off + b + 1);        // this shard's documents, offsets from its first byte
        const uint64_t base = off[0];
        for (auto& o : off) o -= base;
        ExtraSlice xs;
        xs.set(extra, a, b);
        return gft_process(g, text_blob + base, off.data(), b - a, flags, xs.ptr, hit_bitmap ? hit_bitmap + a * words : nullptr);
    });
    or_peer_verdicts(e);
    return rc;
}

int multi_process_again(gft_engine* e, uint64_t n_docs, const gft_extra_matches* extra, uint32_t* hit_bitmap) {
    const size_t n = e->peers.size() + 1;
    if (e->shard_cut.size() != n + 1 || e->shard_cut.back() != n_docs || !n_docs)
        return fail(e, GFT_E_INVALID, "gft_process_again: no scan of these documents to reuse");
    const uint64_t words = (e->n_exprs + 31) / 32;
    return fan_out(e, [&](size_t i, gft_engine* g) {
        const uint64_t a = e->shard_cut[i], b = e->shard_cut[i + 1];
        if (a == b) return (int)GFT_OK;
        ExtraSlice xs;
        xs.set(extra, a, b);
        return gft_process_again(g, b - a, xs.ptr, hit_bitmap ? hit_bitmap + a * words : nullptr);
    });
}

int multi_scan(gft_engine* e, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags, gft_matches* out) {
    const size_t n = e->peers.size() + 1;
    static const uint64_t kNoDocs[1] = {0};
    if (n_docs == 0) doc_off = kNoDocs;                  // (see multi_process)
    std::vector<uint64_t> cut;
    split_by_bytes(doc_off, n_docs, n, cut);
    std::vector<gft_matches> part(n);
    int rc = fan_out(e, [&](size_t i, gft_engine* g) {
        const uint64_t a = cut[i], b = cut[i + 1];
        std::vector<uint64_t> off(doc_off + a, doc_off + b + 1);
        const uint64_t base = off[0];
        for (auto& o : off) o -= base;
        return gft_scan(g, text_blob + base, off.data(), b - a, flags, &part[i]);
    });
    if (rc) return rc;
    // the shards' CSRs one behind the other (device 0's own result lives in this handle's vectors: copied out first)
    uint64_t total = 0;
    for (const auto& p : part) total += p.n_matches;
    std::vector<uint64_t> mo(n_docs + 1, 0);
    std::vector<uint32_t> ti((size_t)total), po((size_t)total);
    uint64_t at = 0;
    for (size_t i = 0; i < n; i++) {
        const uint64_t a = cut[i], nd = cut[i + 1] - a;
        for (uint64_t d = 0; d <= nd; d++) mo[a + d] = at + part[i].match_off[d];
        if (part[i].n_matches) {
            memcpy(ti.data() + at, part[i].term_id, part[i].n_matches * 4);
            memcpy(po.data() + at, part[i].pos, part[i].n_matches * 4);
        }
        at += part[i].n_matches;
    }
    e->h_match_off.swap(mo); e->h_term.swap(ti); e->h_pos.swap(po);
    or_peer_verdicts(e);
    out->n_docs = n_docs; out->n_matches = total;
    out->match_off = e->h_match_off.data(); out->term_id = e->h_term.data(); out->pos = e->h_pos.data();
    return GFT_OK;
}

}  // namespace gft::api

extern "C" {

int gft_engine_create_multi(gft_engine** out, const int* devices, int n_devices) try {
    if (!out || n_devices < 0 || (n_devices && !devices)) return GFT_E_INVALID;
    *out = nullptr;
    std::vector<int> devs(devices, devices + n_devices);
    if (devs.empty()) {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess) count = 0;
        for (int d = 0; d < count; d++) devs.push_back(d);
        if (devs.empty()) devs.push_back(0);       // (gft_engine_create reports the missing device)
    }
    gft_engine* e = nullptr;
    int rc = gft_engine_create(&e, devs[0]);
    *out = e;
    if (rc) return rc;
    for (size_t i = 1; i < devs.size(); i++) {
        gft_engine* p = nullptr;
        rc = gft_engine_create(&p, devs[i]);
        if (rc) {
            e->err = "device " + std::to_string(devs[i]) + ": " + (p ? p->err : std::string("cannot create an engine"));
            if (p) gft_engine_destroy(p);
            return rc;
        }
        e->peers.push_back(p);
    }
    // RCCL communicators over xGMI for the device-resident entry point -- only when the devices are distinct (a list
    // that names one device twice is a test configuration: the gather is then plain device-to-device copies)
    std::vector<int> uniq(devs);
    std::sort(uniq.begin(), uniq.end());
    const bool distinct = std::adjacent_find(uniq.begin(), uniq.end()) == uniq.end();
    // GFT_RCCL_SELF=1: a list that names ONE device several times gets a communicator of one rank, and the gather moves every
    // further shard's bitmap with a grouped ncclSend / ncclRecv of that rank to itself -- the same dlopen, the same bound
    // entry points, the same group and stream ordering as the N-device gather, on the one GPU a test box has
    const char* self_env = getenv("GFT_RCCL_SELF");
    e->rccl_self = devs.size() > 1 && uniq.front() == uniq.back() && self_env && self_env[0] == '1';
    if (devs.size() > 1 && (distinct || e->rccl_self)) {
        RcclApi& api = rccl_api();
        if (!api.ok()) {
            e->rccl_self = false;
            e->err = "RCCL (librccl.so) could not be loaded: bitmaps will be gathered by device-to-device copies";
            return GFT_W_NO_RCCL;
        }
        std::vector<ncclComm_t> comms(e->rccl_self ? 1 : devs.size());
        DeviceGuard dg(devs[0]);
        const ncclResult_t r = api.CommInitAll(comms.data(), (int)comms.size(), devs.data());
        if (r != ncclSuccess) {
            // the handle is complete without communicators, but the caller is TOLD that its gathers are not RCCL's
            e->rccl_self = false;
            e->err = std::string("ncclCommInitAll: ") + api.GetErrorString(r) + " (bitmaps will be gathered by device-to-device copies)";
            return GFT_W_NO_RCCL;
        }
        for (ncclComm_t c : comms) e->comms.push_back((void*)c);
    }
    return GFT_OK;
} GFT_CATCH(nullptr)

int gft_n_devices(const gft_engine* e) { return e ? (int)e->peers.size() + 1 : 0; }
const char* gft_gather_mode(const gft_engine* e) { return !e || e->peers.empty() ? "" : e->comms.empty() ? "copy" : "rccl"; }

gft_engine* gft_device_engine(gft_engine* e, int i) {
    if (!e || i < 0 || i > (int)e->peers.size()) return nullptr;
    return i == 0 ? e : e->peers[(size_t)i - 1];
}

int gft_split_docs(const gft_engine* e, const uint64_t* doc_off, uint64_t n_docs, uint64_t* cut) try {
    if (!e || !cut || (n_docs && !doc_off)) return GFT_E_INVALID;
    std::vector<uint64_t> c;
    split_by_bytes(doc_off, n_docs, e->peers.size() + 1, c);
    memcpy(cut, c.data(), c.size() * 8);
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int gft_process_device_multi(gft_engine* e, const uint8_t* const* d_text, const uint64_t* const* d_doc_off, const uint64_t* n_docs,
                             uint32_t flags, uint32_t* d_bitmap_root) try {
    if (!e || !d_text || !d_doc_off || !n_docs) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    if (int rc = check_ready(e, kNeedBuilt | kNeedPrograms)) return rc;
    const std::vector<gft_engine*> eng = all_engines(e);
    const size_t n = eng.size();
    const uint64_t words = (e->n_exprs + 31) / 32;
    std::vector<uint64_t> first(n + 1, 0);
    for (size_t i = 0; i < n; i++) first[i + 1] = first[i] + n_docs[i];
    if (first[n] * words && !d_bitmap_root) return fail(e, GFT_E_INVALID, "null bitmap");
    // every device solves its shard into its own bitmap (device 0 straight into its slice of the result) ...
    int rc = fan_out(e, [&](size_t i, gft_engine* g) {
        uint32_t* dst = d_bitmap_root;
        if (i) {
            GFT_LOCK(g);
            DeviceGuard dg(g->device);
            if (g->d_bitmap.ensure(std::max<uint64_t>(n_docs[i] * words, 1) * 4) != hipSuccess) return fail(g, GFT_E_HIP, "bitmap alloc");
            dst = g->d_bitmap.as<uint32_t>();
        }
        return gft_process_device(g, d_text[i], d_doc_off[i], n_docs[i], flags, nullptr, dst);
    });
    if (rc) return rc;
    // ... then ONE exchange step: the shards' bitmaps to the first device, ncclSend / ncclRecv in one group over xGMI
    // (plain device-to-device copies when there is no communicator)
    if (n > 1 && words) {
        RcclApi& api = rccl_api();
        if (!e->comms.empty() && api.ok()) {
            DeviceGuard dgr(e->device);
            ncclResult_t r = api.GroupStart();
            for (size_t i = 1; i < n && r == ncclSuccess; i++) {
                if (!n_docs[i]) continue;
                // (one rank for all shards under GFT_RCCL_SELF: peer 0 on communicator 0, both halves on the root's stream --
                // the shard's stream was drained when its gft_process_device returned)
                const int from = e->rccl_self ? 0 : (int)i;
                ncclComm_t send_comm = (ncclComm_t)e->comms[e->rccl_self ? 0 : i];
                hipStream_t send_stream = e->rccl_self ? e->stream : eng[i]->stream;
                r = api.Recv(d_bitmap_root + first[i] * words, n_docs[i] * words, ncclUint32, from, (ncclComm_t)e->comms[0], e->stream);
                if (r == ncclSuccess)
                    r = api.Send(eng[i]->d_bitmap.p, n_docs[i] * words, ncclUint32, 0, send_comm, send_stream);
            }
            const ncclResult_t r2 = api.GroupEnd();
            if (r != ncclSuccess || r2 != ncclSuccess)
                return fail(e, GFT_E_HIP, std::string("RCCL gather: ") + api.GetErrorString(r != ncclSuccess ? r : r2));
            for (gft_engine* g : eng) {
                DeviceGuard dg(g->device);
                HIP_TRY(hipStreamSynchronize(g->stream), "RCCL gather");
            }
        } else {
            DeviceGuard dg(e->device);
            for (size_t i = 1; i < n; i++)
                if (n_docs[i]) HIP_TRY(hipMemcpyAsync(d_bitmap_root + first[i] * words, eng[i]->d_bitmap.p, n_docs[i] * words * 4, hipMemcpyDeviceToDevice, e->stream), "bitmap gather");
            HIP_TRY(hipStreamSynchronize(e->stream), "bitmap gather");
        }
    }
    or_peer_verdicts(e);
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

}  // extern "C"
