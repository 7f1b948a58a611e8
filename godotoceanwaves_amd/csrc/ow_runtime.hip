// ow_runtime.hip -- the context's housekeeping behind include/ocean_waves.h: the WaveGenerator of
// assets/water/wave_generator.gd re-expressed as a HIP stream program.
//
//   init_gpu (:17-54)  -> ow_create : one allocation per resource for all array layers
// and errors, ow_destroy, the status word and sync_stream, the scratch allocation, the timing event pool, dma-buf export and import, the
// readback hand-off, the debug getters and setters and the probe.  Which launches a call turns into (update, _process, _update: :56-109)
// is ow_schedule.hip; ow_schedule.h lists what crosses between the two.
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ow_schedule.h"
#include "ow_tables.h"

namespace {
thread_local std::string g_last_error;
}

namespace ow {
ow_status fail(ow_status st, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return st;
}
void set_last_error(const char *message) { g_last_error = message ? message : ""; }
}  // namespace ow

using ow::base_scratch_slots, ow::check_cascade, ow::ensure_scratch, ow::fail, ow::lookahead_scratch_slots, ow::main_stream, ow::plan_tick_groups, ow::plane,
    ow::refuse_faulted, ow::sync_stream;
constexpr double kHostG = 9.81;  // wave_generator.gd:5

ow_status ow::ensure_scratch(ow_context *c, int slots) {
    if (slots <= c->scratch_slots) return OW_OK;
    const size_t pl = (size_t)c->n * c->n;
    ow::cplx *T = nullptr, *pcol = nullptr, *rrow = nullptr;
    if (hipMalloc((void **)&T, (size_t)slots * pl * ow::kLayers * sizeof(ow::cplx)) != hipSuccess ||
        hipMalloc((void **)&pcol, (size_t)slots * c->n * sizeof(ow::cplx)) != hipSuccess ||
        hipMalloc((void **)&rrow, (size_t)slots * c->n * 4 * sizeof(ow::cplx)) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(T);
        (void)hipFree(pcol);
        (void)hipFree(rrow);
        return fail(OW_ERR_NOMEM, "hipMalloc failed for %d launch slots of scratch intermediate (%zu bytes)", slots, (size_t)slots * pl * ow::kLayers * sizeof(ow::cplx));
    }
    // the old scratch may still be in use by launches already enqueued (it is dead once they have finished: scratch of one batch)
    if (c->buf.T && hipStreamSynchronize(main_stream(c)) != hipSuccess) {
        (void)hipFree(T);
        (void)hipFree(pcol);
        (void)hipFree(rrow);
        return fail(OW_ERR_HIP, "hipStreamSynchronize failed while growing the scratch intermediate");
    }
    (void)hipFree(c->buf.T);
    (void)hipFree(c->buf.pcol);
    (void)hipFree(c->buf.rrow);
    c->buf.T = T;
    c->buf.pcol = pcol;
    c->buf.rrow = rrow;
    c->scratch_slots = slots;
    drop_computed_ahead(c);              // (a speculated pass 1 went with the old buffer, too)
    for (int &sl : c->slot_of) sl = -1;  // (the reference-layout view of the last batch's intermediate went with the old buffer)
    return OW_OK;
}

namespace {
// The runtime carves allocations below 2 MiB out of shared 2 MiB buffer objects, and a dma-buf always covers the whole object
// (measured: scripts/dmabuf_probe.py -- an import of the second 1 MiB allocation saw the first one's bytes).  The two output arrays
// are therefore allocated in whole multiples of 2 MiB: each is a buffer object of its own and ow_export_maps' descriptors map it
// from offset 0.
constexpr size_t kExportGranule = (size_t)2 << 20;
size_t exportable_bytes(size_t bytes) { return (bytes + kExportGranule - 1) / kExportGranule * kExportGranule; }

constexpr size_t kMaxTimedBatches = 4096;

ow_status collect_timing(ow_context *c) {
    if (c->ev_used == 0) return OW_OK;
    OW_HIP(hipEventSynchronize(c->ev[c->ev_used - 1]));
    for (size_t i = 0; i + 4 <= c->ev_used; i += 4) {
        float a = 0, b = 0;
        OW_HIP(hipEventElapsedTime(&a, c->ev[i], c->ev[i + 1]));
        if (i / 4 < c->ev_single.size() && c->ev_single[i / 4]) {
            c->tg_ms += a;
            c->tg_launches += 1;
            continue;
        }
        OW_HIP(hipEventElapsedTime(&b, c->ev[i + 2], c->ev[i + 3]));
        c->t1_ms += a;
        c->t2_ms += b;
        c->t_launches += 1;
    }
    c->ev_used = 0;
    return OW_OK;
}
}  // namespace

ow_status ow::next_events(ow_context *c, hipEvent_t **out, bool single) {
    if (c->ev_used + 4 > 4 * kMaxTimedBatches) {
        ow_status st = collect_timing(c);
        if (st != OW_OK) return st;
    }
    while (c->ev.size() < c->ev_used + 4) {
        hipEvent_t e;
        OW_HIP(hipEventCreate(&e));
        c->ev.push_back(e);
    }
    *out = &c->ev[c->ev_used];
    if (c->ev_single.size() < c->ev_used / 4 + 1) c->ev_single.resize(c->ev_used / 4 + 1);
    c->ev_single[c->ev_used / 4] = single ? 1 : 0;
    c->ev_used += 4;
    return OW_OK;
}

namespace {
// the status word, consumed: marks what the faulted batches left behind (shared by sync_stream and ow::poll_status)
ow_status consume_status(ow_context *c) {
    if (!c->status_host || *c->status_host == 0u) {
        return OW_OK;
    }
    const uint32_t bits = *c->status_host;
    *c->status_host = 0u;                          // the word is consumed; later batches start clean ...
    c->maps_faulted |= c->enqueued_since_sync;     // ... but what the faulted batches left behind stays marked until those layers are recomputed
    c->enqueued_since_sync = 0;
    // ... and so does whatever those launches computed AHEAD: a speculated pass 1 (of cascades that are not even enqueued yet, or of the same
    // cascade one tick later at 2048^2, where pass 1 has a bounded wait of its own) may be as corrupt as the maps.  The queue is dropped: the
    // ticks after a fault recompute their pass 1.
    ow::drop_computed_ahead(c);
    for (int i = 0; i < OW_MAX_CASCADES; ++i)
        if (c->copy_pending[i]) c->readback_faulted |= 1u << i;
    return fail(OW_ERR_HIP, "device-side failure reported by a frame kernel (status 0x%x%s): the maps of the batches enqueued since "
                            "the last synchronisation are invalid", bits, (bits & ow::kStatusRowSyncTimeout) ? ": wave-pair rendezvous timed out" : "");
}
}  // namespace
ow_status ow::refuse_faulted(const ow_context *c, uint32_t layer_mask) {
    if (c->maps_faulted & layer_mask)
        return fail(OW_ERR_HIP, "layer mask 0x%x holds maps of a batch that reported a device-side failure (already returned by an earlier call); "
                                "they stay invalid until a later batch has recomputed those layers (faulted: 0x%x)", layer_mask, c->maps_faulted);
    return OW_OK;
}
ow_status ow::sync_stream(ow_context *c, uint32_t layer_mask) {
    ++c->host_syncs;
    OW_HIP(hipStreamSynchronize(main_stream(c)));
    if (ow_status st = consume_status(c); st != OW_OK) return st;
    c->enqueued_since_sync = 0;  // everything enqueued so far has finished cleanly
    return refuse_faulted(c, layer_mask);
}

namespace ow {
// The device status word WITHOUT synchronising: for a caller that has waited by other means (the group's gather waits on its own
// copy events) and is about to hand out map bytes.  Same consumption / stickiness as sync_stream.
ow_status poll_status(ow_context *c) {
    if (ow_status st = consume_status(c); st != OW_OK) return st;
    return refuse_faulted(c, layer_mask(c->cascades));
}
}  // namespace ow
ow_status ow::check_cascade(const ow_context *c, int cascade) {
    if (!c) return fail(OW_ERR_INVALID, "null context");
    if (cascade < 0 || cascade >= c->layers) return fail(OW_ERR_INVALID, "cascade %d out of range [0,%d)", cascade, c->layers);
    return OW_OK;
}

extern "C" {

const char *ow_last_error(void) { return g_last_error.c_str(); }
int32_t ow_abi_version(void) { return OW_ABI_VERSION; }

double ow_jonswap_alpha(double wind_speed, double fetch_length_m) {  // wave_generator.gd:116-117
    return 0.076 * std::pow(std::pow(wind_speed, 2.0) / (fetch_length_m * kHostG), 0.22);  // `wind_speed**2` is pow() in GDScript
}
double ow_jonswap_peak_angular_frequency(double wind_speed, double fetch_length_m) {  // wave_generator.gd:120-121
    return 22.0 * std::pow(kHostG * kHostG / (wind_speed * fetch_length_m), 1.0 / 3.0);
}

ow_status ow_create(const ow_config *cfg, ow_context **out) {
    if (!cfg || !out) return fail(OW_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!ow::supported_map_size(cfg->map_size))
        return fail(OW_ERR_INVALID, "map_size %d unsupported (128, 256, 512, 1024, 2048)", cfg->map_size);
    if (cfg->num_cascades < 1 || cfg->num_cascades > OW_MAX_CASCADES)
        return fail(OW_ERR_INVALID, "num_cascades %d outside [1,%d]", cfg->num_cascades, OW_MAX_CASCADES);

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(OW_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    int dev = cfg->device_id, caller_dev = 0;
    OW_HIP(hipGetDevice(&caller_dev));
    if (dev < 0) dev = caller_dev;
    if (dev >= ndev) return fail(OW_ERR_INVALID, "device_id %d >= device count %d", dev, ndev);
    // the caller's current device is put back on every way out (a library must not change it behind the caller's back)
    struct DeviceRestore {
        int dev;
        ~DeviceRestore() { (void)hipSetDevice(dev); }
    } restore{caller_dev};
    OW_HIP(hipSetDevice(dev));
    hipDeviceProp_t prop;
    OW_HIP(hipGetDeviceProperties(&prop, dev));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(OW_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 only", dev, prop.gcnArchName);

    ow_context *c = new (std::nothrow) ow_context();
    if (!c) return fail(OW_ERR_NOMEM, "out of host memory");
    c->n = cfg->map_size;
    c->cascades = cfg->num_cascades;
    c->layers = cfg->num_cascades < 2 ? 2 : cfg->num_cascades;  // init_gpu(maxi(2, n)), water.gd:91
    c->device = dev;
    c->depth = cfg->depth > 0.0f ? cfg->depth : 20.0f;  // DEPTH, wave_generator.gd:6
    {
        const bool lp = cfg->flags & OW_FLAG_KERNELS_LAYER_PARALLEL, cp = cfg->flags & OW_FLAG_KERNELS_COMPACT;
        c->kernel_mode = (cfg->flags & OW_FLAG_KERNELS_STANDARD) ? 1 : (lp && cp) ? 4 : lp ? 2 : cp ? 3 : 0;
    }

    c->bodies_mode = (cfg->flags & OW_FLAG_BODIES_FUSED) ? 1 : (cfg->flags & OW_FLAG_BODIES_SPLIT) ? 2 : 0;

    auto bail = [&](ow_status st) {
        ow_destroy(c);
        return st;
    };
    if (cfg->stream) {
        c->stream = (hipStream_t)cfg->stream;
    } else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess)
            return bail(fail(OW_ERR_HIP, "hipStreamCreate failed"));
        c->own_stream = true;
    }
    // the second chain's stream (ow_kernels.h "TWO CHAINS"): only where a launch can be split at all -- 1024^2 with at least four cascades, 512^2 with eight
    if (!(cfg->flags & OW_FLAG_SINGLE_STREAM) && ((c->n == 1024 && c->cascades >= 4) || (c->n == 512 && c->cascades >= 8))) {
        if (hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&c->side_fork_ev, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->side_join_ev, hipEventDisableTiming) != hipSuccess)
            return bail(fail(OW_ERR_HIP, "second stream / events: creation failed"));
    }
    const size_t pl = plane(c), L = (size_t)c->layers;
#define OW_ALLOC(ptr, bytes)                                                                              \
    if (hipMalloc((void **)&(ptr), (bytes)) != hipSuccess)                                                \
        return bail(fail(OW_ERR_NOMEM, "hipMalloc of %zu bytes failed for " #ptr, (size_t)(bytes)));
    OW_ALLOC(c->buf.h0, L * pl * sizeof(ow::cplx));                   // h0(k): the non-redundant half of the spectrum texture (:31)
    OW_ALLOC(c->buf.omega, L * pl * sizeof(float));
    // scratch between pass 1 and pass 2 of one batch (half of the reference's fft_buffer, :33): one batch worth only, so it
    // is the same <= 128 MiB for every batch and stays in the Infinity Cache
    c->no_merge = (cfg->flags & OW_FLAG_NO_TICK_GROUPS) != 0;
    c->run_as_calls = (cfg->flags & OW_FLAG_RUN_AS_CALLS) != 0;
    c->run_as_reference = (cfg->flags & OW_FLAG_RUN_AS_REFERENCE_SCHEDULE) != 0;
    c->always_regenerate = (cfg->flags & OW_FLAG_ALWAYS_REGENERATE_SPECTRUM) != 0;
    plan_tick_groups(c, cfg->flags);
    // (OW_FLAG_LAZY_SCRATCH: one batch now, the look-ahead's share on its first use -- a context that is only ever driven through ow_run's tick groups,
    //  or one of many shards on a device, need not hold it)
    const bool lazy_scratch = (cfg->flags & OW_FLAG_LAZY_SCRATCH) != 0;
    if (ensure_scratch(c, lazy_scratch ? base_scratch_slots(c) : std::max(base_scratch_slots(c), lookahead_scratch_slots(c))) != OW_OK) return bail(OW_ERR_NOMEM);
    if (cfg->displacement_map) {
        c->buf.disp = (ow::u16x4 *)cfg->displacement_map;
    } else {
        OW_ALLOC(c->buf.disp, exportable_bytes(L * pl * sizeof(ow::u16x4)));  // R16G16B16A16_SFLOAT (:34)
        c->own_disp = true;
    }
    if (cfg->normal_map) {
        c->buf.norm = (ow::u16x4 *)cfg->normal_map;
    } else {
        OW_ALLOC(c->buf.norm, exportable_bytes(L * pl * sizeof(ow::u16x4)));  // (:35)
        c->own_norm = true;
    }
    OW_ALLOC(c->buf.foam, L * pl * sizeof(uint16_t));                 // FP16 foam state in pass-2 lane order
    if (cfg->flags & OW_FLAG_DEBUG_F32) { OW_ALLOC(c->buf.f32, L * pl * 8 * sizeof(float)); }
    if (hipHostMalloc((void **)&c->status_host, 64, hipHostMallocMapped) != hipSuccess)
        return bail(fail(OW_ERR_NOMEM, "hipHostMalloc failed for the device status word"));
    *c->status_host = 0u;
    if (hipHostGetDevicePointer((void **)&c->buf.status, c->status_host, 0) != hipSuccess)
        return bail(fail(OW_ERR_HIP, "hipHostGetDevicePointer failed for the device status word"));
    std::vector<ow::cplx> tw;
    ow::make_twiddles(c->n, tw);
    OW_ALLOC(c->tw_dev, tw.size() * sizeof(ow::cplx));
    std::vector<ow::cplx> tw_split;
    if (ow::make_split_twiddles(c->n, tw_split)) { OW_ALLOC(c->tw_split_dev, tw_split.size() * sizeof(ow::cplx)); }
    std::vector<ow::cplx> tw_half;
    if (ow::make_half_twiddles(c->n, tw_half)) { OW_ALLOC(c->tw_half_dev, tw_half.size() * sizeof(ow::cplx)); }
#undef OW_ALLOC
    c->buf.tw = c->tw_dev;
    c->buf.tw_split = c->tw_split_dev;
    c->buf.tw_half = c->tw_half_dev;
    if (c->tw_half_dev && hipMemcpyAsync(c->tw_half_dev, tw_half.data(), tw_half.size() * sizeof(ow::cplx), hipMemcpyHostToDevice, main_stream(c)) != hipSuccess)
        return bail(fail(OW_ERR_HIP, "twiddle upload failed"));
    if (c->tw_split_dev && hipMemcpyAsync(c->tw_split_dev, tw_split.data(), tw_split.size() * sizeof(ow::cplx), hipMemcpyHostToDevice, main_stream(c)) != hipSuccess)
        return bail(fail(OW_ERR_HIP, "twiddle upload failed"));
    // Vulkan images start undefined; foam must start from a defined state: zero
    if (hipMemcpyAsync(c->tw_dev, tw.data(), tw.size() * sizeof(ow::cplx), hipMemcpyHostToDevice, main_stream(c)) != hipSuccess ||
        hipMemsetAsync(c->buf.disp, 0, L * pl * sizeof(ow::u16x4), main_stream(c)) != hipSuccess ||
        hipMemsetAsync(c->buf.norm, 0, L * pl * sizeof(ow::u16x4), main_stream(c)) != hipSuccess ||
        hipMemsetAsync(c->buf.foam, 0, L * pl * sizeof(uint16_t), main_stream(c)) != hipSuccess ||
        hipMemsetAsync(c->buf.h0, 0, L * pl * sizeof(ow::cplx), main_stream(c)) != hipSuccess ||
        hipMemsetAsync(c->buf.omega, 0, L * pl * sizeof(float), main_stream(c)) != hipSuccess ||
        hipStreamSynchronize(main_stream(c)) != hipSuccess)
        return bail(fail(OW_ERR_HIP, "initial upload failed: %s", hipGetErrorString(hipGetLastError())));
    for (int &sl : c->slot_of) sl = -1;
    *out = c;
    return OW_OK;
}

void ow_destroy(ow_context *c) {
    if (!c) return;
    int caller_dev = -1;
    (void)hipGetDevice(&caller_dev);
    (void)hipSetDevice(c->device);
    if (c->side_stream) (void)hipStreamSynchronize(c->side_stream);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (ow::Handle *h : c->handles) {  // handles the caller has not destroyed: their memory goes with the context, they stay valid to destroy
        (void)hipFree(h->block);
        h->block = nullptr;
        h->ctx = nullptr;
    }
    (void)hipFree(c->buf.h0);
    (void)hipFree(c->buf.omega);
    (void)hipFree(c->buf.T);
    if (c->own_disp) (void)hipFree(c->buf.disp);
    if (c->own_norm) (void)hipFree(c->buf.norm);
    (void)hipFree(c->buf.foam);
    (void)hipFree(c->buf.f32);
    (void)hipFree(c->buf.pcol);
    (void)hipFree(c->buf.rrow);
    (void)hipFree(c->tw_dev);
    (void)hipFree(c->tw_split_dev);
    (void)hipFree(c->tw_half_dev);
    if (c->status_host) (void)hipHostFree(c->status_host);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    (void)hipFree(c->snap_dev);
    if (c->snap_host) (void)hipHostFree(c->snap_host);
    for (auto &e : c->snap_ready)
        if (e) (void)hipEventDestroy(e);
    for (auto &e : c->copy_done)
        if (e) (void)hipEventDestroy(e);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    for (ow::DeviceScratch *s : {&c->query_scratch, &c->buoy_scratch, &c->ray_scratch, &c->render_rgba, &c->render_pixels, &c->mesh_vis, &c->billboard, &c->solid, &c->solid_cast, &c->mist, &c->mirror}) s->release();
    (void)hipFree(c->ray_bound);
    (void)hipFree(c->vel);
    (void)hipFree(c->vel_scratch);
    (void)hipFree(c->vel_tw);
    for (auto &e : c->ev)
        if (e) (void)hipEventDestroy(e);
    if (c->side_fork_ev) (void)hipEventDestroy(c->side_fork_ev);
    if (c->side_join_ev) (void)hipEventDestroy(c->side_join_ev);
    if (c->side_stream) (void)hipStreamDestroy(c->side_stream);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    if (caller_dev >= 0) (void)hipSetDevice(caller_dev);
}

ow_status ow_debug_inject_fault(ow_context *c, uint32_t fault_bits) {
    if (!c) return fail(OW_ERR_INVALID, "null context");
    if (fault_bits & 2u) {  // the status word as a faulting launch would leave it -- of the launches IN FLIGHT (look-ahead included), not of the next batch
        if (c->status_host) __atomic_store_n(c->status_host, (uint32_t)ow::kStatusRowSyncTimeout, __ATOMIC_RELEASE);
        fault_bits &= ~2u;
        if (fault_bits == 0) return OW_OK;
    }
    c->inject_fault = fault_bits;
    return OW_OK;
}

ow_status ow_sync(ow_context *c) {
    if (!c) return fail(OW_ERR_INVALID, "null context");
    OW_HIP(hipSetDevice(c->device));
    return sync_stream(c, 0u);
}

ow_status ow_get_device_ptrs(ow_context *c, void **disp, void **norm, size_t *stride) {
    if (!c) return fail(OW_ERR_INVALID, "null context");
    if (disp) *disp = c->buf.disp;
    if (norm) *norm = c->buf.norm;
    if (stride) *stride = plane(c) * sizeof(ow::u16x4);
    return OW_OK;
}

// ---- zero-copy hand-off: dma-buf export of the two arrays, import of a foreign allocation (ocean_waves.h) ----
ow_status ow_export_maps(ow_context *c, int32_t *disp_fd, int32_t *norm_fd, size_t *bytes_each) {
    if (!c) return fail(OW_ERR_INVALID, "null context");
    OW_HIP(hipSetDevice(c->device));
    const size_t bytes = (size_t)c->layers * plane(c) * sizeof(ow::u16x4);
    int fds[2] = {-1, -1};
    void *ptrs[2] = {c->buf.disp, c->buf.norm};
    const bool own[2] = {c->own_disp, c->own_norm};
    for (int i = 0; i < 2; ++i) {
        if ((i == 0 && !disp_fd) || (i == 1 && !norm_fd)) continue;
        if (!own[i]) {  // caller-owned memory: exportable only if it is a whole buffer object (see exportable_bytes)
            void *base = nullptr;
            size_t range = 0;
            if (hipMemGetAddressRange((hipDeviceptr_t *)&base, &range, (hipDeviceptr_t)ptrs[i]) != hipSuccess || base != ptrs[i] || range < kExportGranule ||
                ((uintptr_t)base & (kExportGranule - 1)) != 0) {
                (void)hipGetLastError();
                if (fds[0] >= 0) close(fds[0]);
                return fail(OW_ERR_STATE, "the caller-owned %s array is not the start of an allocation of at least 2 MiB: a dma-buf covers whole buffer "
                                          "objects, so the descriptor would not map the array from offset 0", i ? "normal" : "displacement");
            }
        }
        const hipError_t e = hipMemGetHandleForAddressRange(&fds[i], (hipDeviceptr_t)ptrs[i], bytes, hipMemRangeHandleTypeDmaBufFd, 0);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            if (fds[0] >= 0) close(fds[0]);
            return fail(OW_ERR_HIP, "hipMemGetHandleForAddressRange (dma-buf export of the %s array, %zu bytes) failed: %s", i ? "normal" : "displacement",
                        bytes, hipGetErrorString(e));
        }
    }
    if (disp_fd) *disp_fd = fds[0];
    if (norm_fd) *norm_fd = fds[1];
    if (bytes_each) *bytes_each = bytes;
    return OW_OK;
}

struct ow_imported {
    hipExternalMemory_t ext = nullptr;
    void *ptr = nullptr;
    int device = 0;
    int fd = -1;  // our duplicate of the caller's descriptor: this runtime neither takes ownership of an imported descriptor nor closes it
                  // (measured: forty import / release cycles left forty descriptors open), so it is closed by ow_release_buffer
};

ow_status ow_import_buffer(int32_t device_id, int32_t fd, size_t offset, size_t bytes, ow_imported **out, void **device_ptr) {
    if (!out || !device_ptr) return fail(OW_ERR_INVALID, "null argument");
    *out = nullptr;
    *device_ptr = nullptr;
    if (fd < 0 || bytes == 0) return fail(OW_ERR_INVALID, "bad file descriptor or size");
    int ndev = 0, caller_dev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(OW_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    OW_HIP(hipGetDevice(&caller_dev));
    const int dev = device_id < 0 ? caller_dev : device_id;
    if (dev >= ndev) return fail(OW_ERR_INVALID, "device_id %d >= device count %d", dev, ndev);
    struct DeviceRestore {
        int dev;
        ~DeviceRestore() { (void)hipSetDevice(dev); }
    } restore{caller_dev};
    OW_HIP(hipSetDevice(dev));
    const int own = dup(fd);  // the import consumes a descriptor; the caller's stays the caller's
    if (own < 0) return fail(OW_ERR_INVALID, "dup(%d) failed", fd);
    hipExternalMemoryHandleDesc hd;
    std::memset(&hd, 0, sizeof(hd));
    hd.type = hipExternalMemoryHandleTypeOpaqueFd;
    hd.handle.fd = own;
    hd.size = offset + bytes;
    hipExternalMemory_t ext = nullptr;
    hipError_t e = hipImportExternalMemory(&ext, &hd);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        close(own);
        return fail(OW_ERR_HIP, "hipImportExternalMemory(fd, %zu bytes) failed: %s", offset + bytes, hipGetErrorString(e));
    }
    hipExternalMemoryBufferDesc bd;
    std::memset(&bd, 0, sizeof(bd));
    bd.offset = 0;             // the window is applied to the mapped pointer below: given a non-zero offset, this runtime's
    bd.size = offset + bytes;  // GetMappedBuffer did not return the window's bytes (round 3, first version of tests/test_interop.py)
    void *ptr = nullptr;
    e = hipExternalMemoryGetMappedBuffer(&ptr, ext, &bd);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)hipDestroyExternalMemory(ext);
        close(own);
        return fail(OW_ERR_HIP, "hipExternalMemoryGetMappedBuffer failed: %s", hipGetErrorString(e));
    }
    ow_imported *im = new (std::nothrow) ow_imported();
    if (!im) {
        (void)hipDestroyExternalMemory(ext);
        close(own);
        return fail(OW_ERR_NOMEM, "out of host memory");
    }
    im->fd = own;
    im->ext = ext;
    im->ptr = ptr;
    im->device = dev;
    *out = im;
    *device_ptr = static_cast<char *>(ptr) + offset;
    return OW_OK;
}

void ow_release_buffer(ow_imported *im) {
    if (!im) return;
    int caller_dev = -1;
    (void)hipGetDevice(&caller_dev);
    (void)hipSetDevice(im->device);
    (void)hipDestroyExternalMemory(im->ext);
    if (im->fd >= 0) close(im->fd);
    delete im;
    if (caller_dev >= 0) (void)hipSetDevice(caller_dev);
}

ow_status ow_get_maps(ow_context *c, int32_t cascade, void *disp, void *norm) {
    ow_status st = check_cascade(c, cascade);
    if (st != OW_OK) return st;
    OW_HIP(hipSetDevice(c->device));
    const size_t bytes = plane(c) * sizeof(ow::u16x4);
    if (disp) OW_HIP(hipMemcpyAsync(disp, c->buf.disp + cascade * plane(c), bytes, hipMemcpyDeviceToHost, main_stream(c)));
    if (norm) OW_HIP(hipMemcpyAsync(norm, c->buf.norm + cascade * plane(c), bytes, hipMemcpyDeviceToHost, main_stream(c)));
    return sync_stream(c, 1u << cascade);
}

ow_status ow_readback_begin(ow_context *c, uint32_t mask) {
    if (!c) return fail(OW_ERR_INVALID, "null context");
    if (mask == 0 || (mask >> c->layers) != 0) return fail(OW_ERR_INVALID, "cascade_mask 0x%x selects no layer or one >= %d", mask, c->layers);
    OW_HIP(hipSetDevice(c->device));
    const size_t pl = plane(c), L = (size_t)c->layers, bytes = pl * sizeof(ow::u16x4);
    if (!c->snap_host) {  // first use: second stream, snapshot planes, page-locked staging, events -- committed only when ALL succeeded
        hipStream_t cs = nullptr;
        ow::u16x4 *sd = nullptr, *sh = nullptr;
        hipEvent_t ready[OW_MAX_CASCADES] = {}, done[OW_MAX_CASCADES] = {};
        bool ok = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) == hipSuccess && hipMalloc((void **)&sd, 2 * L * bytes) == hipSuccess &&
                  hipHostMalloc((void **)&sh, 2 * L * bytes, hipHostMallocDefault) == hipSuccess;
        for (size_t i = 0; ok && i < L; ++i)
            ok = hipEventCreateWithFlags(&ready[i], hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&done[i], hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            const hipError_t e = hipGetLastError();
            for (auto &x : ready)
                if (x) (void)hipEventDestroy(x);
            for (auto &x : done)
                if (x) (void)hipEventDestroy(x);
            if (sh) (void)hipHostFree(sh);
            (void)hipFree(sd);
            if (cs) (void)hipStreamDestroy(cs);
            return fail(OW_ERR_NOMEM, "readback resources (2 x %zu bytes, device + page-locked host) could not be created: %s", 2 * L * bytes, hipGetErrorString(e));
        }
        c->copy_stream = cs;
        c->snap_dev = sd;
        c->snap_host = sh;
        for (size_t i = 0; i < L; ++i) {
            c->snap_ready[i] = ready[i];
            c->copy_done[i] = done[i];
        }
    }
    for (int i = 0; i < c->layers; ++i) {
        if (!((mask >> i) & 1u)) continue;
        ow::u16x4 *sd = c->snap_dev + (size_t)i * pl, *sn = c->snap_dev + (L + i) * pl;
        ow::u16x4 *hd = c->snap_host + (size_t)i * pl, *hn = c->snap_host + (L + i) * pl;
        // the snapshot slot may still be feeding an earlier PCIe copy
        if (c->copy_pending[i]) OW_HIP(hipStreamWaitEvent(main_stream(c), c->copy_done[i], 0));
        c->readback_faulted &= ~(1u << i);  // a new snapshot of this layer
        OW_HIP(hipMemcpyAsync(sd, c->buf.disp + (size_t)i * pl, bytes, hipMemcpyDeviceToDevice, main_stream(c)));
        OW_HIP(hipMemcpyAsync(sn, c->buf.norm + (size_t)i * pl, bytes, hipMemcpyDeviceToDevice, main_stream(c)));
        OW_HIP(hipEventRecord(c->snap_ready[i], main_stream(c)));
        OW_HIP(hipStreamWaitEvent(c->copy_stream, c->snap_ready[i], 0));
        OW_HIP(hipMemcpyAsync(hd, sd, bytes, hipMemcpyDeviceToHost, c->copy_stream));
        OW_HIP(hipMemcpyAsync(hn, sn, bytes, hipMemcpyDeviceToHost, c->copy_stream));
        OW_HIP(hipEventRecord(c->copy_done[i], c->copy_stream));
        c->copy_pending[i] = true;
    }
    return OW_OK;
}

ow_status ow_readback_wait(ow_context *c, int32_t cascade, const void **disp, const void **norm) {
    ow_status st = check_cascade(c, cascade);
    if (st != OW_OK) return st;
    if (!c->copy_stream || !c->copy_pending[cascade]) return fail(OW_ERR_STATE, "no readback of cascade %d is outstanding", cascade);
    OW_HIP(hipSetDevice(c->device));
    OW_HIP(hipEventSynchronize(c->copy_done[cascade]));
    c->copy_pending[cascade] = false;
    if (*c->status_host != 0u) {  // a frame kernel reported a failure: the bytes that landed are not maps
        c->readback_faulted |= 1u << cascade;  // (copy_pending was just cleared: mark this layer by hand, the others are marked by sync_stream)
        (void)sync_stream(c, 0u);
    }
    if ((c->readback_faulted >> cascade) & 1u) {  // every layer of the faulted batch fails, not only the first one waited for
        c->readback_faulted &= ~(1u << cascade);
        return fail(OW_ERR_HIP, "the readback of cascade %d carries maps of a batch that reported a device-side failure", cascade);
    }
    const size_t pl = plane(c), L = (size_t)c->layers;
    if (disp) *disp = c->snap_host + (size_t)cascade * pl;
    if (norm) *norm = c->snap_host + (L + cascade) * pl;
    return OW_OK;
}

ow_status ow_set_normal_map(ow_context *c, int32_t cascade, const void *norm) {
    ow_status st = check_cascade(c, cascade);
    if (st != OW_OK) return st;
    if (!norm) return fail(OW_ERR_INVALID, "null normal map");
    OW_HIP(hipSetDevice(c->device));
    // the foam channel (.a) also goes into the context's private FP16 foam plane, in pass-2 lane order
    // (ow_device.h Pass2::foam_index): that plane, not normal.a, is what the recurrence reads back
    const size_t n = (size_t)c->n, tl = n / 16;
    std::vector<uint16_t> foam(plane(c));
    const uint16_t *src = static_cast<const uint16_t *>(norm);
    for (size_t xp = 0; xp < n; ++xp)
        for (size_t yp = 0; yp < n; ++yp) foam[xp * n + (yp % tl) * 16 + yp / tl] = src[(xp * n + yp) * 4 + 3];
    OW_HIP(hipMemcpyAsync(c->buf.norm + cascade * plane(c), norm, plane(c) * sizeof(ow::u16x4), hipMemcpyHostToDevice, main_stream(c)));
    OW_HIP(hipMemcpyAsync(c->buf.foam + cascade * plane(c), foam.data(), plane(c) * sizeof(uint16_t), hipMemcpyHostToDevice, main_stream(c)));
    OW_HIP(hipStreamSynchronize(main_stream(c)));
    return OW_OK;
}

ow_status ow_get_maps_f32(ow_context *c, int32_t cascade, float *out) {
    ow_status st = check_cascade(c, cascade);
    if (st != OW_OK) return st;
    if (!c->buf.f32) return fail(OW_ERR_STATE, "context was created without OW_FLAG_DEBUG_F32");
    if (!out) return fail(OW_ERR_INVALID, "null output");
    OW_HIP(hipSetDevice(c->device));
    OW_HIP(hipMemcpyAsync(out, c->buf.f32 + cascade * plane(c) * 8, plane(c) * 8 * sizeof(float), hipMemcpyDeviceToHost, main_stream(c)));
    return sync_stream(c, 1u << cascade);
}

ow_status ow_get_spectrum(ow_context *c, int32_t cascade, float *h0, float *omega) {
    ow_status st = check_cascade(c, cascade);
    if (st != OW_OK) return st;
    OW_HIP(hipSetDevice(c->device));
    std::vector<ow::cplx> a;
    if (h0) {
        a.resize(plane(c));
        OW_HIP(hipMemcpyAsync(a.data(), c->buf.h0 + cascade * plane(c), plane(c) * sizeof(ow::cplx), hipMemcpyDeviceToHost, main_stream(c)));
    }
    if (omega) OW_HIP(hipMemcpyAsync(omega, c->buf.omega + cascade * plane(c), plane(c) * sizeof(float), hipMemcpyDeviceToHost, main_stream(c)));
    OW_HIP(hipStreamSynchronize(main_stream(c)));
    if (h0) {  // rebuild the reference's texel (h0(k), conj(h0(-k))) from the stored half (spectrum_compute.glsl:121-124)
        const size_t n = (size_t)c->n;
        for (size_t y = 0; y < n; ++y)
            for (size_t x = 0; x < n; ++x) {
                const ow::cplx v = a[y * n + x], m = a[((n - y) % n) * n + (n - x) % n];
                float *o = h0 + (y * n + x) * 4;
                o[0] = v.x;
                o[1] = v.y;
                o[2] = m.x;
                o[3] = -m.y;
            }
    }
    return OW_OK;
}

ow_status ow_debug_set_spectrum(ow_context *c, int32_t cascade, const float *h0, const float *omega) {
    ow_status st = check_cascade(c, cascade);
    if (st != OW_OK) return st;
    if (!h0) return fail(OW_ERR_INVALID, "null spectrum");
    if (cascade >= OW_MAX_CASCADES || !c->spectrum_resident[cascade])
        return fail(OW_ERR_STATE, "cascade %d has no resident spectrum yet: its push-constant words exist only after its first generation", cascade);
    OW_HIP(hipSetDevice(c->device));
    // everything launched so far read the old planes: drained first (both chains: main_stream joins the second one) ...
    if (st = sync_stream(c, 0u); st != OW_OK) return st;
    // ... and whatever was computed AHEAD from them does not survive -- the look-ahead queue (a pre-armed ow_process queue is the same queue), what a
    // run armed for the next run -- exactly as where a batch regenerates a spectrum (enqueue)
    ow::drop_computed_ahead(c);
    c->velocity_stale |= 1u << cascade;  // (V is made from the resident spectrum)
    OW_HIP(hipMemcpyAsync(c->buf.h0 + cascade * plane(c), h0, plane(c) * sizeof(ow::cplx), hipMemcpyHostToDevice, main_stream(c)));
    if (omega) OW_HIP(hipMemcpyAsync(c->buf.omega + cascade * plane(c), omega, plane(c) * sizeof(float), hipMemcpyHostToDevice, main_stream(c)));
    OW_HIP(hipStreamSynchronize(main_stream(c)));
    return OW_OK;  // spectrum_resident and pc_words stay: a clean record, or a dirty one that packs to the resident words, keeps these planes
}

ow_status ow_get_push_constants(const ow_context *c, int32_t cascade, ow_push_constants *out) {
    ow_status st = check_cascade(c, cascade);
    if (st != OW_OK) return st;
    if (!out) return fail(OW_ERR_INVALID, "null output");
    if (cascade >= OW_MAX_CASCADES || !c->pc_valid[cascade]) return fail(OW_ERR_STATE, "cascade %d has not been launched yet", cascade);
    *out = c->pc_words[cascade];
    return OW_OK;
}

ow_status ow_get_intermediate(ow_context *c, int32_t cascade, float *out) {
    ow_status st = check_cascade(c, cascade);
    if (st != OW_OK) return st;
    if (!out) return fail(OW_ERR_INVALID, "null output");
    OW_HIP(hipSetDevice(c->device));
    const size_t pl = plane(c), n = (size_t)c->n;
    std::vector<ow::cplx> t(pl * ow::kLayers);
    if (c->slot_of[cascade] < 0)
        return fail(OW_ERR_STATE, "cascade %d was not part of the most recent batch: its intermediate has been overwritten", cascade);
    if (c->last_family >= 3)
        return fail(OW_ERR_STATE, "the most recent batch used the compact (three-layer) intermediate, which has no counterpart in the "
                                  "reference's fft_buffer: create the context with OW_FLAG_KERNELS_STANDARD to inspect it");
    OW_HIP(hipMemcpyAsync(t.data(), c->buf.T + (size_t)c->slot_of[cascade] * pl * ow::kLayers, t.size() * sizeof(ow::cplx), hipMemcpyDeviceToHost, main_stream(c)));
    OW_HIP(hipStreamSynchronize(main_stream(c)));
    // device layout T[layer][y/16][x'][y%16]  ->  reference half-0-after-transpose layout [layer][row = x'][col = y].
    // The device rows carry the x' half of the ifftshift sign, (-1)^x' (see Pass1::rot): taken out again here.
    for (int layer = 0; layer < ow::kLayers; ++layer)
        for (size_t xp = 0; xp < n; ++xp) {
            const float sgn = (xp & 1) ? -1.0f : 1.0f;
            for (size_t y = 0; y < n; ++y) {
                const ow::cplx v = t[ow::t_unit((int)n, layer, (int)xp, (int)y)];
                float *o = out + (((size_t)layer * n + xp) * n + y) * 2;
                o[0] = v.x * sgn;
                o[1] = v.y * sgn;
            }
        }
    return OW_OK;
}

ow_status ow_probe_kernel_times(ow_context *c, int32_t reps, float *p1_ms, float *p2_ms, int32_t *cascades_per_launch) {
    if (!c) return fail(OW_ERR_INVALID, "null context");
    if (reps < 1 || c->last_count < 1) return fail(OW_ERR_STATE, "nothing has been launched yet (or reps < 1)");
    OW_HIP(hipSetDevice(c->device));
    ow::drop_computed_ahead(c);  // (the probe launches write the scratch intermediate from slot 0 on)
    hipEvent_t e[3] = {};
    float a = 0, b = 0;
    auto run = [&]() -> ow_status {
        for (auto &x : e) OW_HIP(hipEventCreate(&x));
        OW_HIP(hipEventRecord(e[0], main_stream(c)));
        for (int i = 0; i < reps; ++i) OW_HIP(ow::launch_pass1(c->n, c->last_count, c->kernel_mode, c->last_args, c->buf, main_stream(c)));
        OW_HIP(hipEventRecord(e[1], main_stream(c)));
        for (int i = 0; i < reps; ++i) OW_HIP(ow::launch_pass2(c->n, c->last_count, c->kernel_mode, c->last_args, c->buf, main_stream(c)));
        OW_HIP(hipEventRecord(e[2], main_stream(c)));
        OW_HIP(hipEventSynchronize(e[2]));
        OW_HIP(hipEventElapsedTime(&a, e[0], e[1]));
        OW_HIP(hipEventElapsedTime(&b, e[1], e[2]));
        return OW_OK;
    };
    const ow_status st = run();
    for (auto &x : e)
        if (x) (void)hipEventDestroy(x);  // on every way out
    if (st != OW_OK) return st;
    if (p1_ms) *p1_ms = a / reps;
    if (p2_ms) *p2_ms = b / reps;
    if (cascades_per_launch) *cascades_per_launch = c->last_count;
    return OW_OK;
}

ow_status ow_timing_enable(ow_context *c, int32_t enable) {
    if (!c) return fail(OW_ERR_INVALID, "null context");
    if (!enable) {
        ow_status st = collect_timing(c);
        if (st != OW_OK) return st;
    }
    c->timing = enable == 2 ? 2 : enable != 0;
    return OW_OK;
}

ow_status ow_timing_read(ow_context *c, float *p1, float *p2, int32_t *launches, int32_t reset) {
    if (!c) return fail(OW_ERR_INVALID, "null context");
    ow_status st = collect_timing(c);
    if (st != OW_OK) return st;
    const int n = c->t_launches;
    if (p1) *p1 = n ? (float)(c->t1_ms / n) : 0.0f;
    if (p2) *p2 = n ? (float)(c->t2_ms / n) : 0.0f;
    if (launches) *launches = n;
    if (reset) {
        c->t1_ms = c->t2_ms = 0;
        c->t_launches = 0;
    }
    return OW_OK;
}

ow_status ow_timing_read_launches(ow_context *c, float *launch_ms_avg, int32_t *launches, int32_t reset) {
    if (!c) return fail(OW_ERR_INVALID, "null context");
    ow_status st = collect_timing(c);
    if (st != OW_OK) return st;
    if (launch_ms_avg) *launch_ms_avg = c->tg_launches ? (float)(c->tg_ms / c->tg_launches) : 0.0f;
    if (launches) *launches = c->tg_launches;
    if (reset) {
        c->tg_ms = 0;
        c->tg_launches = 0;
    }
    return OW_OK;
}

}  // extern "C"
