// gft_json_api.cpp -- JSON documents decoded on the device into the record form (gft_json.hpp): the engine's side, which
// group_json.cpp drives.
#include "gft_engine.hpp"

#include <atomic>

#include "gft_json.hpp"
#include "json_paths.hpp"
#include "json_schema.hpp"

using namespace gft;
using namespace gft::api;

namespace {
int json_entry_checks(gft_engine* e) {
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, "JSON batches: single-device handles only");
    return check_ready(e, kNeedDevice | kNeedSettled, "JSON batches");
}
constexpr RoomTexts kJsonRoom{"no device memory for the JSON batch's work buffers", "JSON batch alloc"};
bool overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
    if (!a || !b || !a_bytes || !b_bytes) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + b_bytes && y < x + a_bytes;
}
}  // namespace

namespace gft {

int json_install(gft_engine* e, const JsonSchema& s, uint64_t* serial) try {
    if (!e || !serial) return GFT_E_INVALID;
    GFT_LOCK(e);
    int rc = json_entry_checks(e);
    if (rc) return rc;
    DeviceGuard g(e->device);
    auto& J = e->d_json;
    J.serial = 0;                          // (a failed upload leaves no trie)
    if ((rc = upload(e, J.nodes, s.nodes, "JSON schema upload"))) return rc;
    if ((rc = upload(e, J.keys, s.keys, "JSON schema upload"))) return rc;
    if ((rc = upload(e, J.table, s.table, "JSON schema upload"))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream), "JSON schema upload");
    J.n_nodes = (uint32_t)s.nodes.size(); J.table_mask = (uint32_t)s.table.size() - 1; J.max_key_len = s.max_key_len;
    static std::atomic<uint64_t> next_serial{1};
    *serial = J.serial = next_serial.fetch_add(1);
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

uint64_t json_serial(gft_engine* e) {
    if (!e) return 0;
    GFT_LOCK(e);
    return e->d_json.serial;
}

int json_leaves_device(gft_engine* e, const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_status, uint64_t* d_rec_off,
                       uint32_t* d_leaf_field, uint64_t* d_leaf_off, uint64_t leaf_cap, uint8_t* d_text, uint64_t text_cap, uint64_t* totals) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    int rc = json_entry_checks(e);
    if (rc) return rc;
    auto& J = e->d_json;
    if (!J.serial) return fail(e, GFT_E_INVALID, "JSON batch: no schema installed");
    if (!d_rec_off || (n_docs && (!d_blob || !d_doc_off || !d_status))) return fail(e, GFT_E_INVALID, "JSON batch: null argument");
    if ((leaf_cap && (!d_leaf_field || !d_leaf_off)) || (text_cap && !d_text)) return fail(e, GFT_E_INVALID, "JSON batch: a cap but no array");
    DeviceGuard g(e->device);
    hipStream_t st = e->stream;
    if (totals) totals[0] = totals[1] = 0;
    if (!n_docs) {
        HIP_TRY(hipMemsetAsync(d_rec_off, 0, 8, st), "JSON offsets");
        if (d_leaf_off) HIP_TRY(hipMemsetAsync(d_leaf_off, 0, 8, st), "JSON offsets");
        HIP_TRY(hipStreamSynchronize(st), "JSON offsets");
        return GFT_OK;
    }
    uint64_t ends[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&ends[0], d_doc_off, 8, hipMemcpyDeviceToHost, st), "JSON offsets");
    HIP_TRY(hipMemcpyAsync(&ends[1], d_doc_off + n_docs, 8, hipMemcpyDeviceToHost, st), "JSON offsets");
    HIP_TRY(hipStreamSynchronize(st), "JSON offsets");
    if (ends[1] < ends[0]) return fail(e, GFT_E_INVALID, "gft_group_json_leaves_device: document offsets descend");
    const struct { const void* p; uint64_t bytes; } in[2] = {{d_blob + ends[0], ends[1] - ends[0] + 64}, {d_doc_off, (n_docs + 1) * 8}},
        outs[5] = {{d_status, n_docs}, {d_rec_off, (n_docs + 1) * 8}, {d_leaf_field, leaf_cap * 4}, {d_leaf_off, d_leaf_off ? (leaf_cap + 1) * 8 : 0},
                   {d_text, text_cap}};
    for (const auto& i : in)
        for (const auto& o : outs)
            if (overlap(i.p, i.bytes, o.p, o.bytes)) return fail(e, GFT_E_INVALID, "gft_group_json_leaves_device: the output overlaps the input");
    if ((rc = room(e, J.cnt_leaves, n_docs * 4, kJsonRoom)) || (rc = room(e, J.cnt_text, n_docs * 4, kJsonRoom)) || (rc = room(e, J.text_off, (n_docs + 1) * 8, kJsonRoom)) ||
        (rc = room(e, J.partial, scan_partials_needed(n_docs) * 8, kJsonRoom)) || (rc = room(e, J.flags, 16, kJsonRoom)))
        return rc;
    JsonParams P{};
    P.blob = d_blob; P.doc_off = d_doc_off; P.n_docs = n_docs;
    P.T = JsonTrie{J.nodes.as<JsonTrieNode>(), J.keys.as<uint8_t>(), J.table.as<uint32_t>(), J.table_mask, J.n_nodes, J.max_key_len};
    P.status = d_status; P.cnt_leaves = J.cnt_leaves.as<uint32_t>(); P.cnt_text = J.cnt_text.as<uint32_t>(); P.flags = J.flags.as<uint32_t>();
    P.rec_off = d_rec_off; P.text_off = J.text_off.as<uint64_t>();
    P.leaf_field = d_leaf_field; P.leaf_off = d_leaf_off; P.text = d_text; P.leaf_cap = leaf_cap; P.text_cap = text_cap;
    HIP_TRY(hipMemsetAsync(P.flags, 0, 8, st), "JSON count");
    {
        ProfScope ps(e, "json_count");
        HIP_TRY(launch_json_count(P, e->n_cus, st), "JSON count kernel launch");
    }
    {
        ProfScope ps(e, "json_scan");
        HIP_TRY(launch_exclusive_scan(P.cnt_leaves, n_docs, d_rec_off, J.partial.as<uint64_t>(), st), "JSON scan");
        HIP_TRY(launch_exclusive_scan(P.cnt_text, n_docs, J.text_off.as<uint64_t>(), J.partial.as<uint64_t>(), st), "JSON scan");
    }
    uint64_t h_tot[2] = {0, 0};
    uint32_t h_flags[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&h_tot[0], d_rec_off + n_docs, 8, hipMemcpyDeviceToHost, st), "JSON totals");
    HIP_TRY(hipMemcpyAsync(&h_tot[1], J.text_off.as<uint64_t>() + n_docs, 8, hipMemcpyDeviceToHost, st), "JSON totals");
    HIP_TRY(hipMemcpyAsync(h_flags, P.flags, 8, hipMemcpyDeviceToHost, st), "JSON totals");
    HIP_TRY(hipStreamSynchronize(st), "JSON count");
    if (h_flags[0]) return fail(e, GFT_E_INVALID, "gft_group_json_leaves_device: document offsets descend, or a document of 4 GiB or more");
    if (totals) { totals[0] = h_tot[0]; totals[1] = h_tot[1]; }
    if (d_leaf_off || d_text) {
        ProfScope ps(e, "json_write");
        HIP_TRY(launch_json_write(P, e->n_cus, st), "JSON write kernel launch");
    }
    HIP_TRY(hipStreamSynchronize(st), "JSON write");
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int json_leaves_owned(gft_engine* e, const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_status,
                      const uint64_t** d_rec_off, const uint32_t** d_leaf_field, const uint64_t** d_leaf_off, const uint8_t** d_text,
                      uint64_t* totals) try {
    if (!e || !d_rec_off || !d_leaf_field || !d_leaf_off || !d_text || !totals) return GFT_E_INVALID;
    GFT_LOCK(e);
    int rc = json_entry_checks(e);
    if (rc) return rc;
    DeviceGuard g(e->device);
    auto& J = e->d_json;
    if ((rc = room(e, J.rec_off, (n_docs + 1) * 8, kJsonRoom)) || (rc = room(e, J.leaf_field, 16, kJsonRoom)) || (rc = room(e, J.leaf_off, 16, kJsonRoom)) ||
        (rc = room(e, J.text, 64, kJsonRoom)))
        return rc;
    for (int round = 0;; round++) {
        const uint64_t leaf_cap = std::min<uint64_t>(J.leaf_field.cap / 4, J.leaf_off.cap / 8 - 1), text_cap = J.text.cap - 64;
        if ((rc = json_leaves_device(e, d_blob, d_doc_off, n_docs, d_status, J.rec_off.as<uint64_t>(), J.leaf_field.as<uint32_t>(),
                                     J.leaf_off.as<uint64_t>(), leaf_cap, J.text.as<uint8_t>(), text_cap, totals)))
            return rc;
        if (totals[0] <= leaf_cap && totals[1] <= text_cap) break;
        if (round) return fail(e, GFT_E_INTERNAL, "JSON batch: the record arrays do not fit the buffers grown for them");
        if ((rc = room(e, J.leaf_field, totals[0] * 4, kJsonRoom)) || (rc = room(e, J.leaf_off, (totals[0] + 1) * 8, kJsonRoom)) ||
            (rc = room(e, J.text, totals[1] + 64, kJsonRoom)))
            return rc;
    }
    HIP_TRY(hipMemsetAsync(J.text.as<uint8_t>() + totals[1], 0, 64, e->stream), "JSON text slack");
    HIP_TRY(hipStreamSynchronize(e->stream), "JSON text slack");
    *d_rec_off = J.rec_off.as<uint64_t>(); *d_leaf_field = J.leaf_field.as<uint32_t>();
    *d_leaf_off = J.leaf_off.as<uint64_t>(); *d_text = J.text.as<uint8_t>();
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int json_paths_device(gft_engine* e, const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, std::vector<std::string>& paths,
                      uint64_t* dropped) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    int rc = json_entry_checks(e);
    if (rc) return rc;
    paths.clear();
    if (dropped) *dropped = 0;
    if (n_docs && (!d_blob || !d_doc_off)) return fail(e, GFT_E_INVALID, "JSON batch: null argument");
    if (!n_docs) return GFT_OK;
    DeviceGuard g(e->device);
    SyncOnExit drain(e);                   // (the copies below land in vectors of this call)
    hipStream_t st = e->stream;
    uint64_t ends[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&ends[0], d_doc_off, 8, hipMemcpyDeviceToHost, st), "JSON offsets");
    HIP_TRY(hipMemcpyAsync(&ends[1], d_doc_off + n_docs, 8, hipMemcpyDeviceToHost, st), "JSON offsets");
    HIP_TRY(hipStreamSynchronize(st), "JSON offsets");
    if (ends[1] < ends[0]) return fail(e, GFT_E_INVALID, "gft_group_json_paths_device: document offsets descend");
    // counters (count, dropped, cursor, -) | slots | path_off | pool: one allocation of a fixed size
    constexpr uint64_t kHead = 16, kSlots = (uint64_t)kJsonPathSlots * 8, kOffs = (uint64_t)kJsonPathCap * 4;
    auto& J = e->d_json;
    if ((rc = room(e, J.paths, kHead + kSlots + kOffs + kJsonPathPool, kJsonRoom)) || (rc = room(e, J.flags, 16, kJsonRoom))) return rc;
    uint8_t* base = J.paths.as<uint8_t>();
    JsonPathParams P{};
    P.blob = d_blob; P.doc_off = d_doc_off; P.n_docs = n_docs; P.flags = J.flags.as<uint32_t>();
    uint32_t* head = reinterpret_cast<uint32_t*>(base);
    P.set = JsonPathSet{reinterpret_cast<uint64_t*>(base + kHead), head, head + 1, head + 2, reinterpret_cast<uint32_t*>(base + kHead + kSlots),
                        base + kHead + kSlots + kOffs, kJsonPathPool};
    HIP_TRY(hipMemsetAsync(base, 0, kHead + kSlots, st), "JSON paths");
    HIP_TRY(hipMemsetAsync(P.set.path_off, 0xFF, kOffs, st), "JSON paths");
    HIP_TRY(hipMemsetAsync(P.flags, 0, 8, st), "JSON paths");
    {
        ProfScope ps(e, "json_paths");
        HIP_TRY(launch_json_paths(P, e->n_cus, st), "JSON paths kernel launch");
    }
    uint32_t h_head[4] = {0, 0, 0, 0}, h_flags[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(h_head, head, 16, hipMemcpyDeviceToHost, st), "JSON paths");
    HIP_TRY(hipMemcpyAsync(h_flags, P.flags, 8, hipMemcpyDeviceToHost, st), "JSON paths");
    HIP_TRY(hipStreamSynchronize(st), "JSON paths");
    if (h_flags[0]) return fail(e, GFT_E_INVALID, "gft_group_json_paths_device: document offsets descend, or a document of 4 GiB or more");
    const uint32_t n = std::min(h_head[0], kJsonPathCap);
    const uint64_t pool_valid = std::min<uint64_t>(h_head[2], kJsonPathPool);
    std::vector<uint32_t> offs(n);
    std::vector<uint8_t> pool(pool_valid);
    if (n) HIP_TRY(hipMemcpyAsync(offs.data(), P.set.path_off, (size_t)n * 4, hipMemcpyDeviceToHost, st), "JSON paths");
    if (pool_valid) HIP_TRY(hipMemcpyAsync(pool.data(), P.set.pool, pool_valid, hipMemcpyDeviceToHost, st), "JSON paths");
    HIP_TRY(hipStreamSynchronize(st), "JSON paths");
    json_paths_collect(h_head[0], offs.data(), pool.data(), pool_valid, paths);
    if (dropped) *dropped = h_head[1];
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int json_stage(gft_engine* e, const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, uint64_t row_bytes, const uint8_t** d_blob,
               const uint64_t** d_doc_off, uint8_t** d_status, uint32_t** d_rows) try {
    if (!e || !doc_off || !d_blob || !d_doc_off || !d_status || !d_rows) return GFT_E_INVALID;
    GFT_LOCK(e);
    int rc = json_entry_checks(e);
    if (rc) return rc;
    DeviceGuard g(e->device);
    SyncOnExit drain(e);
    auto& J = e->d_json;
    const uint64_t lo = doc_off[0], bytes = doc_off[n_docs] - lo;
    if ((rc = room(e, J.blob, lo + bytes + 64, kJsonRoom)) || (rc = room(e, J.doc_off, (n_docs + 1) * 8, kJsonRoom)) || (rc = room(e, J.status, n_docs, kJsonRoom)) ||
        (rc = room(e, J.rows, n_docs * row_bytes, kJsonRoom)))
        return rc;
    // (the offsets stay as the caller gave them: the blob keeps its place in the buffer)
    if (bytes) HIP_TRY(hipMemcpyAsync(J.blob.as<uint8_t>() + lo, blob + lo, bytes, hipMemcpyHostToDevice, e->stream), "JSON batch upload");
    HIP_TRY(hipMemsetAsync(J.blob.as<uint8_t>() + lo + bytes, 0, 64, e->stream), "JSON batch upload");
    HIP_TRY(hipMemcpyAsync(J.doc_off.p, doc_off, (n_docs + 1) * 8, hipMemcpyHostToDevice, e->stream), "JSON batch upload");
    HIP_TRY(hipStreamSynchronize(e->stream), "JSON batch upload");
    *d_blob = J.blob.as<uint8_t>(); *d_doc_off = J.doc_off.as<uint64_t>(); *d_status = J.status.as<uint8_t>(); *d_rows = J.rows.as<uint32_t>();
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int json_stage_lines(gft_engine* e, const uint8_t* blob, uint64_t len, uint64_t row_bytes, const uint8_t** d_blob, const uint64_t** d_doc_off,
                     uint8_t** d_status, uint32_t** d_rows, std::vector<uint64_t>& h_doc_off) try {
    if (!e || (len && !blob) || !d_blob || !d_doc_off || !d_status || !d_rows) return GFT_E_INVALID;
    GFT_LOCK(e);
    int rc = json_entry_checks(e);
    if (rc) return rc;
    DeviceGuard g(e->device);
    SyncOnExit drain(e);
    auto& J = e->d_json;
    if ((rc = room(e, J.blob, len + 64, kJsonRoom)) || (rc = room(e, J.doc_off, 16, kJsonRoom))) return rc;
    if (len) HIP_TRY(hipMemcpyAsync(J.blob.p, blob, len, hipMemcpyHostToDevice, e->stream), "JSON batch upload");
    HIP_TRY(hipMemsetAsync(J.blob.as<uint8_t>() + len, 0, 64, e->stream), "JSON batch upload");
    uint64_t n = 0;
    for (int round = 0;; round++) {
        const uint64_t cap = J.doc_off.cap / 8;
        if ((rc = gft_split_lines_device(e, J.blob.as<uint8_t>(), len, GFT_SPLIT_JSON_LINES, J.doc_off.as<uint64_t>(), cap, &n))) return rc;
        if (n + 1 <= cap) break;
        if (round) return fail(e, GFT_E_INTERNAL, "JSON Lines: the offsets do not fit the buffer grown for them");
        if ((rc = room(e, J.doc_off, (n + 1) * 8, kJsonRoom))) return rc;
    }
    if ((rc = room(e, J.status, n, kJsonRoom)) || (rc = room(e, J.rows, n * row_bytes, kJsonRoom))) return rc;
    h_doc_off.assign(n + 1, 0);
    if ((rc = d2h_staged(e, h_doc_off.data(), J.doc_off.p, (n + 1) * 8))) return rc;
    *d_blob = J.blob.as<uint8_t>(); *d_doc_off = J.doc_off.as<uint64_t>(); *d_status = J.status.as<uint8_t>(); *d_rows = J.rows.as<uint32_t>();
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

}  // namespace gft
