// gft_staging.cpp -- pageable host memory <-> device through two pinned bounce buffers and a few copy threads.
#include "gft_engine.hpp"

#include <cstdlib>
#include <thread>

namespace gft::api {

constexpr size_t kPinBuf = 128u << 20;       // bytes per bounce buffer
// what goes through a buffer at once (GFT_HOST_CHUNK_MB, 4 .. 128; timing study)
static size_t pin_chunk() {
    static const size_t n = [] {
        size_t mb = 128;
        if (const char* e = getenv("GFT_HOST_CHUNK_MB")) { const long v = atol(e); if (v >= 4 && v <= 128) mb = (size_t)v; }
        return mb << 20;
    }();
    return n;
}
// copy threads that fill a bounce buffer: the link (PCIe Gen5 x16, 57 GB/s from pinned memory) is only kept busy when the
// host side copies faster than that -- four threads reach ~58 GB/s, eight 120 (tools/probe_pcie.py); more than eight only add
// wake-ups (12: 11.4-12.0 M documents/s on the 250 000-document batch, 8: 12.2-12.3).  GFT_HOST_THREADS overrides
static unsigned pin_threads() {
    static const unsigned n = [] {
        if (const char* e = getenv("GFT_HOST_THREADS")) { const int v = atoi(e); if (v > 0) return (unsigned)std::min(v, 32); }
        const unsigned hc = std::thread::hardware_concurrency();
        return hc ? std::min(std::max(hc, 2u), 8u) : 4u;
    }();
    return n;
}

// the two pinned bounce buffers with their events, and the threads that fill / empty them
static int ensure_bounce(gft_engine* e) {
    for (int k = 0; k < 2; k++) {
        if (!e->staging.pin[k]) HIP_TRY(hipHostMalloc(&e->staging.pin[k], kPinBuf, hipHostMallocDefault), "pinned alloc");
        if (!e->staging.pin_ev[k]) HIP_TRY(hipEventCreateWithFlags(&e->staging.pin_ev[k], hipEventDisableTiming), "event");
    }
    if (!e->staging.copy_pool) e->staging.copy_pool.reset(new gft::CopyPool(pin_threads() - 1));
    return GFT_OK;
}

// pageable host memory -> device through the pinned bounce buffers
static int h2d_staged(gft_engine* e, void* dst, const void* src, size_t bytes) {
    if (bytes < (8u << 20)) {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e->stream), "upload");
        return GFT_OK;
    }
    if (int rc = ensure_bounce(e)) return rc;
    size_t done = 0;
    // (the first chunks are small and double: the link idles while the very first one is filled)
    size_t chunk = std::min<size_t>(pin_chunk(), 4u << 20);
    for (int k = 0; done < bytes; k ^= 1, chunk = std::min(pin_chunk(), chunk * 2)) {
        const size_t n = std::min(chunk, bytes - done);
        HIP_TRY(hipEventSynchronize(e->staging.pin_ev[k]), "staging");        // the copy out of this buffer has finished
        e->staging.copy_pool->copy(e->staging.pin[k], (const uint8_t*)src + done, n);
        HIP_TRY(hipMemcpyAsync((uint8_t*)dst + done, e->staging.pin[k], n, hipMemcpyHostToDevice, e->stream), "upload");
        HIP_TRY(hipEventRecord(e->staging.pin_ev[k], e->stream), "staging");
        done += n;
    }
    return GFT_OK;
}

// device -> pageable host memory through the same bounce buffers (a copy straight into pageable memory is staged by the
// runtime through one thread); synchronous: returns when dst holds the bytes
int d2h_staged(gft_engine* e, void* dst, const void* src, size_t bytes) {
    if (bytes < (8u << 20)) {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream), "download");
        HIP_TRY(hipStreamSynchronize(e->stream), "download");
        return GFT_OK;
    }
    if (int rc = ensure_bounce(e)) return rc;
    size_t issued = 0, done = 0;
    size_t len[2] = {0, 0};
    int ki = 0, kd = 0;
    // chunk i + 1 is on the wire while chunk i is copied out of its buffer (a result smaller than two buffers goes in
    // quarters, so that there is a chunk i + 1)
    const size_t chunk = std::min(pin_chunk(), std::max<size_t>(4u << 20, (bytes / 4 + 4095) & ~(size_t)4095));
    while (done < bytes) {
        while (issued < bytes && len[ki] == 0) {                  // (a buffer is free again once it has been copied out)
            const size_t n = std::min(chunk, bytes - issued);
            HIP_TRY(hipMemcpyAsync(e->staging.pin[ki], (const uint8_t*)src + issued, n, hipMemcpyDeviceToHost, e->stream), "download");
            HIP_TRY(hipEventRecord(e->staging.pin_ev[ki], e->stream), "staging");
            len[ki] = n; issued += n; ki ^= 1;
        }
        HIP_TRY(hipEventSynchronize(e->staging.pin_ev[kd]), "staging");
        const size_t n = len[kd];
        e->staging.copy_pool->copy((uint8_t*)dst + done, e->staging.pin[kd], n);
        len[kd] = 0; done += n; kd ^= 1;
    }
    return GFT_OK;
}

int stage_docs(gft_engine* e, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs) {
    const uint64_t bytes = n_docs ? doc_off[n_docs] : 0;
    HIP_TRY(e->d_text.ensure(bytes + 64), "text alloc");
    HIP_TRY(e->d_doc_off.ensure((n_docs + 1) * 8), "doc_off alloc");
    if (bytes) { int rc = h2d_staged(e, e->d_text.p, text_blob, bytes); if (rc) return rc; }
    if (n_docs) HIP_TRY(hipMemcpyAsync(e->d_doc_off.p, doc_off, (n_docs + 1) * 8, hipMemcpyHostToDevice, e->stream), "doc_off upload");
    return GFT_OK;
}

}  // namespace gft::api
