// zj_api.cpp -- C ABI of libzjhip.so (see include/zjhip.h).  Host side of the HIP arm: argument
// validation that mirrors the reference's panics, geometry (zj_plan.h), buffer management and
// kernel launches.  There is no CPU compute path in this library.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/zjhip.h"
#include "zj_internal.h"
#include "zj_launch.h"
#include "zj_crop_tensor_launch.h"
#include "zj_mixed_launch.h"
#include "zj_orient_launch.h"
#include "zj_expand_launch.h"
#include "zj_cmyk_launch.h"
#include "zj_color_launch.h"
#include "zj_tone_launch.h"
#include "zj_planes_launch.h"
#include "zj_plan.h"
#include "zj_resize_launch.h"
#include "zj_rzgroup.h"
#include "zj_scaled_launch.h"
#include "zj_stage_pack.h"
#include "zj_to_tensor_launch.h"
#include "zj_warp_fixed.h"
#include "zj_warp_launch.h"

using namespace zj;
static_assert(SCATTER_MAX == ZJ_SCATTER_MAX, "include/zjhip.h and zj_device.h disagree");
static_assert(ZJ_TONE_IDENTITY == TONE_IDENTITY && ZJ_TONE_INVERT == TONE_INVERT && ZJ_TONE_POSTERIZE == TONE_POSTERIZE &&
                  ZJ_TONE_SOLARIZE == TONE_SOLARIZE && ZJ_TONE_AUTOCONTRAST == TONE_AUTOCONTRAST && ZJ_TONE_EQUALIZE == TONE_EQUALIZE,
              "include/zjhip.h and zj_tone_ops.h disagree");
static_assert(sizeof(CropParams) <= 4096 && sizeof(CropZero) <= 4096 && sizeof(ResizeParams) <= 4096, "kernel arguments: 4 KB");

namespace {
constexpr int N_SCRATCH = 4;
constexpr int N_SLOTS = 3;                  // H2D of unit i+1 | kernel of unit i | D2H of unit i-1
constexpr size_t UNIT_TARGET_DEFAULT = 16u << 20; // coefficient bytes per pipeline unit: every copy costs ~15 us of
                                                   // launch overhead (tools/pcie_probe.py), so units stay large

// one buffer set of the host-buffer pipeline (zj_decode_planes_batch).  Three streams, one per engine:
// `up` carries every H2D copy, `run` every kernel, `down` every D2H copy (a stream per direction is what
// lets the two DMA directions overlap, tools/pcie_probe.py); events order the stages of a unit and the
// reuse of its buffers.
struct PipeSlot {
    void* buf[N_SCRATCH] = {nullptr, nullptr, nullptr, nullptr}; // y, cb, cr, out
    size_t cap[N_SCRATCH] = {0, 0, 0, 0};
    hipEvent_t up_done = nullptr, run_done = nullptr, down_done = nullptr;
    bool used = false; // events recorded at least once since the last full synchronisation
};
}

struct zj_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    void* scratch[N_SCRATCH] = {nullptr, nullptr, nullptr, nullptr};
    size_t scratch_cap[N_SCRATCH] = {0, 0, 0, 0};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    PipeSlot slots[N_SLOTS];
    hipStream_t s_up = nullptr, s_run = nullptr, s_down = nullptr;
    int pipeline = 1;             // 0: one unit per call (no overlap), for A/B timing only
    // a frame whose planes are still being written (zj_frame_begin ... zj_frame_end)
    struct FrameStream {
        bool active = false;
        zj_frame_desc d;
        const int16_t* y = nullptr; const int16_t* cb = nullptr; const int16_t* cr = nullptr;
        uint8_t* out = nullptr;
        int on_device = 0;
        bool staged = false;      // host output in pageable memory: decoded into a device buffer, ONE copy at the end (an
                                  // asynchronous copy into pageable memory blocks its caller until the data has arrived)
        size_t submitted = 0, unit = 1, units = 0; // strips handed to the GPU so far | strips per unit | units so far
    } fs;
    std::string last_error;
#if defined(ZJ_ABLATION)
    int debug = 0;                // ablation switches, diagnostic build only (results are WRONG when set)
#endif
    int variant = 0;              // kernel variant: 0 packed generation (default), 1 wide generation (round 1), 2 packed with direct stores
    // first-wave stagger of short launches (zj_kernels.hip: stagger_start, launch_params below): CUs of the device, delay
    // per step
    int cus = 256, stagger_delay = 0;
    // GPU entropy stage (zj_decode_scan): blob + working set, the three planes (contiguous), control words read back
    // one slot per scan of a batch (zj_decode_scans): blob + working set | planes | pixels on their way to host memory
    struct HuffSlot { void* buf = nullptr; size_t cap = 0; void* planes = nullptr; void* out = nullptr; };
    HuffSlot hslot[ZJ_SCAN_BATCH_MAX];
    // planes and staged pixels of the slots live in two arenas at a uniform stride, so that scans of one geometry can go
    // through the pixel kernel as frames of ONE launch (zj_decode_scans)
    void* harena = nullptr; size_t harena_stride = 0; int harena_slots = 0;
    void* hout = nullptr; size_t hout_stride = 0; int hout_slots = 0;
    uint32_t* d_ctl = nullptr;    // the slots' control words, contiguous: one clear, one copy back per call
    uint32_t* h_ctl = nullptr;    // pinned: HUFF_CTL_WORDS per slot

    // the u8 crops of the resized crop decode (zj_decode_crops_resized_device): their buffer, and the event after the last
    // resize that read it, recorded on whichever stream that call ran on (the next user waits for it on ITS stream)
    void* rz_buf = nullptr; size_t rz_cap = 0;
    hipEvent_t rz_done = nullptr; bool rz_used = false;
    // the histograms and tables of the tone stage (zj_tone_device), and the event after the last lookup that
    // read them, recorded on whichever stream that call ran on (rz_done's rule)
    void* tone_buf = nullptr; size_t tone_cap = 0;
    hipEvent_t tone_done = nullptr; bool tone_used = false;
    // mixed-geometry crops (zj_decode_crops_resized_mixed_device): the per-frame records of a launch group,
    // built in pinned staging and copied to the device table on the caller's stream.  mx_up: after the last copy out of the
    // staging (the host waits for it before writing the staging again); mx_done: after the last launch that read the device
    // table, on whichever stream that ran (the next copy into it waits for it on ITS stream).  mx_arena: the plane rows of a
    // decoder batch's files (zj_decoder_finish_pixels_resized_crop_batch_device), on the context stream only.
    void* mx_host = nullptr; void* mx_dev = nullptr; size_t mx_cap = 0;
    hipEvent_t mx_up = nullptr, mx_done = nullptr; bool mx_used = false;
    void* mx_arena = nullptr; void* mx_stage = nullptr; size_t mx_arena_cap = 0; // (mx_stage: pinned, the same size)
    bool scan_planes_only = false; // zjint_scan_to_planes: the entropy stage alone, the planes stay in the slot (crop windows)
    int huff_rounds = 0;          // synchronisation rounds of the last scan
    int huff_plane_slot = 0;
    size_t huff_plane_off[3] = {0, 0, 0}, huff_plane_len[3] = {0, 0, 0}; // the last call's first scan: its planes inside the slot (bytes / int16 elements)
    int huff_recent = 0;          // the most rounds a scan of the last few needed (decays): how many to launch ahead
    float huff_submit_ms = 0;     // host time of the last scan's submission (everything up to the final synchronisation)
    float huff_ms[3] = {0, 0, 0}; // with ZJ_HUFF_TIME: upload + sync rounds | scan + write + cut | pixel kernel (+ download) of the last scan
};

#define ZJ_HIP(ctx, call)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            (ctx)->last_error = std::string(#call) + ": " + hipGetErrorString(e_);                 \
            return ZJ_ERR_HIP;                                                                     \
        }                                                                                          \
    } while (0)

static int ensure_scratch(zj_ctx* c, int i, size_t bytes)
{
    if (bytes <= c->scratch_cap[i]) return ZJ_OK;
    if (c->scratch[i]) { ZJ_HIP(c, hipStreamSynchronize(c->stream)); ZJ_HIP(c, hipFree(c->scratch[i])); c->scratch[i] = nullptr; c->scratch_cap[i] = 0; }
    size_t cap = bytes + bytes / 4 + 4096;
    ZJ_HIP(c, hipMalloc(&c->scratch[i], cap));
    c->scratch_cap[i] = cap;
    return ZJ_OK;
}

static int pipe_sync(zj_ctx* c)
{
    ZJ_HIP(c, hipStreamSynchronize(c->s_up));
    ZJ_HIP(c, hipStreamSynchronize(c->s_run));
    ZJ_HIP(c, hipStreamSynchronize(c->s_down));
    for (PipeSlot& sl : c->slots) sl.used = false;
    return ZJ_OK;
}

static int pipe_init(zj_ctx* c)
{
    if (c->s_up) return ZJ_OK;
    ZJ_HIP(c, hipStreamCreateWithFlags(&c->s_up, hipStreamNonBlocking));
    ZJ_HIP(c, hipStreamCreateWithFlags(&c->s_run, hipStreamNonBlocking));
    ZJ_HIP(c, hipStreamCreateWithFlags(&c->s_down, hipStreamNonBlocking));
    for (PipeSlot& sl : c->slots) {
        ZJ_HIP(c, hipEventCreateWithFlags(&sl.up_done, hipEventDisableTiming));
        ZJ_HIP(c, hipEventCreateWithFlags(&sl.run_done, hipEventDisableTiming));
        ZJ_HIP(c, hipEventCreateWithFlags(&sl.down_done, hipEventDisableTiming));
    }
    return ZJ_OK;
}

static int ensure_slot(zj_ctx* c, PipeSlot& sl, int i, size_t bytes)
{
    if (bytes <= sl.cap[i]) return ZJ_OK;
    if (sl.buf[i]) { int rc = pipe_sync(c); if (rc) return rc; ZJ_HIP(c, hipFree(sl.buf[i])); sl.buf[i] = nullptr; sl.cap[i] = 0; }
    const size_t cap = bytes + bytes / 8 + 4096;
    ZJ_HIP(c, hipMalloc(&sl.buf[i], cap));
    sl.cap[i] = cap;
    return ZJ_OK;
}

extern "C" {

int zj_abi_version(void) { return ZJ_ABI_VERSION; }

int zj_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return ZJ_ERR_NO_DEVICE;
    return n;
}

const char* zj_strerror(int status)
{
    switch (status) {
    case ZJ_OK: return "ok";
    case ZJ_ERR_ARG: return "invalid argument";
    case ZJ_ERR_UNSUPPORTED: return "valid for the reference but not supported by the HIP arm";
    case ZJ_ERR_HIP: return "HIP runtime error (see zj_last_error)";
    case ZJ_ERR_NOMEM: return "out of memory";
    case ZJ_ERR_PANIC: return "the reference would panic on these arguments";
    case ZJ_ERR_NO_DEVICE: return "no usable HIP device";
    case ZJ_ERR_BACKEND: return "only ZJ_BACKEND_HIP is implemented by this library";
    default: return "unknown status";
    }
}

const char* zj_last_error(const zj_ctx* ctx) { return ctx ? ctx->last_error.c_str() : ""; }

zj_ctx* zj_ctx_create(int backend, int device, int* status)
{
    int dummy;
    if (!status) status = &dummy;
    if (backend != ZJ_BACKEND_HIP) { *status = ZJ_ERR_BACKEND; return nullptr; }
    int n = zj_device_count();
    if (n <= 0 || device < 0 || device >= n) { *status = ZJ_ERR_NO_DEVICE; return nullptr; }
    zj_ctx* c = new (std::nothrow) zj_ctx();
    if (!c) { *status = ZJ_ERR_NOMEM; return nullptr; }
    c->device = device;
    if (const char* e = getenv("ZJ_VARIANT")) { int v = atoi(e); if (v >= 0 && v <= 2 && (v != 1 || fused_has_wide())) c->variant = v; }
    {
        hipDeviceProp_t prop;
        c->cus = hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        c->stagger_delay = 16;                        // x 128 cycles per slot group; 0 = off (ZJ_STAGGER: the escape hatch)
        // ZJ_STAGGER = 0..255 (round 4's "delay + 256 * mode" encoding is gone: anything else is refused aloud, not ignored)
        if (const char* e = getenv("ZJ_STAGGER")) {
            char* end = nullptr;
            const long v = strtol(e, &end, 10);
            if (end != e && *end == 0 && v >= 0 && v < 256) c->stagger_delay = (int)v;
            else fprintf(stderr, "libzjhip: ZJ_STAGGER=%s is out of range (0..255, 0 = off); keeping %d\n", e, c->stagger_delay);
        }
    }
    // ZJ_BLOCKING_SYNC=1 (experiment, profiles/r06_pool_sync.txt): threads that wait for the device sleep instead of polling
    if (const char* e = getenv("ZJ_BLOCKING_SYNC")) { if (atoi(e) == 1 && hipSetDevice(device) == hipSuccess) { (void)hipSetDeviceFlags(hipDeviceScheduleBlockingSync); (void)hipGetLastError(); } }
    bool ok = hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreate(&c->ev0) == hipSuccess && hipEventCreate(&c->ev1) == hipSuccess;
    if (!ok) { zj_ctx_destroy(c); *status = ZJ_ERR_NO_DEVICE; return nullptr; }
    *status = ZJ_OK;
    return c;
}

void zj_ctx_destroy(zj_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (int i = 0; i < N_SCRATCH; i++)
        if (c->scratch[i]) (void)hipFree(c->scratch[i]);
    for (auto& sl : c->hslot)
        if (sl.buf) (void)hipFree(sl.buf);
    if (c->harena) (void)hipFree(c->harena);
    if (c->hout) (void)hipFree(c->hout);
    if (c->d_ctl) (void)hipFree(c->d_ctl);
    if (c->h_ctl) (void)hipHostFree(c->h_ctl);
    if (c->rz_done) { if (c->rz_used) (void)hipEventSynchronize(c->rz_done); (void)hipEventDestroy(c->rz_done); }
    if (c->rz_buf) (void)hipFree(c->rz_buf);
    if (c->tone_done) { if (c->tone_used) (void)hipEventSynchronize(c->tone_done); (void)hipEventDestroy(c->tone_done); }
    if (c->tone_buf) (void)hipFree(c->tone_buf);
    if (c->mx_done) { if (c->mx_used) (void)hipEventSynchronize(c->mx_done); (void)hipEventDestroy(c->mx_done); }
    if (c->mx_up) (void)hipEventDestroy(c->mx_up);
    if (c->mx_dev) (void)hipFree(c->mx_dev);
    if (c->mx_host) (void)hipHostFree(c->mx_host);
    if (c->mx_arena) (void)hipFree(c->mx_arena);
    if (c->mx_stage) (void)hipHostFree(c->mx_stage);

    for (hipStream_t st : {c->s_up, c->s_run, c->s_down})
        if (st) (void)hipStreamSynchronize(st);
    for (PipeSlot& sl : c->slots) {
        for (int i = 0; i < N_SCRATCH; i++)
            if (sl.buf[i]) (void)hipFree(sl.buf[i]);
        for (hipEvent_t ev : {sl.up_done, sl.run_done, sl.down_done})
            if (ev) (void)hipEventDestroy(ev);
    }
    for (hipStream_t st : {c->s_up, c->s_run, c->s_down})
        if (st) (void)hipStreamDestroy(st);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// The reference's fn-pointer types carry no context argument and are called concurrently from its
// worker threads (src/mcu.rs:356), so the context the shims use is per calling thread.  The reference
// makes a fresh pool for every decode (src/mcu.rs:135): contexts of finished threads go to a free list
// and are handed to the next new thread instead of being rebuilt (streams, scratch, tables).
namespace {
std::mutex g_def_mu;
std::vector<zj_ctx*> g_def_free;
struct TlsDefaultCtx {
    zj_ctx* c = nullptr;
    ~TlsDefaultCtx() // no HIP calls here: thread-exit order against the runtime's teardown is not ours
    {
        if (!c) return;
        std::lock_guard<std::mutex> lk(g_def_mu);
        g_def_free.push_back(c);
    }
};
}

zj_ctx* zj_default_ctx(void)
{
    thread_local TlsDefaultCtx t;
    if (!t.c) {
        std::lock_guard<std::mutex> lk(g_def_mu);
        if (!g_def_free.empty()) { t.c = g_def_free.back(); g_def_free.pop_back(); }
    }
    if (!t.c) { int st; t.c = zj_ctx_create(ZJ_BACKEND_HIP, 0, &st); }
    return t.c;
}

int zj_num_components(int cs) { return ncomp_of(cs); }

size_t zj_plane_len(const zj_frame_desc* d, int comp)
{
    if (!d || d->width == 0 || d->height == 0) return 0;
    if (!((d->h_max == 1 || d->h_max == 2) && (d->v_max == 1 || d->v_max == 2))) return 0;
    if (comp < 0 || comp >= (int)d->in_components || d->in_components > 3) return 0;
    const size_t mcu_x = (d->width + 8 * d->h_max - 1) / (8 * d->h_max);  // headers.rs:317
    const size_t mcu_y = (d->height + 8 * d->v_max - 1) / (8 * d->v_max); // headers.rs:319
    const size_t hs = comp == 0 ? d->h_max : 1, vs = comp == 0 ? d->v_max : 1;
    return mcu_x * 64 * vs * hs * mcu_y; // mcu_prog.rs:76
}

size_t zj_out_len(const zj_frame_desc* d)
{
    if (!d) return 0;
    // (make_plan's arithmetic without its checks: a length for any descriptor, as before)
    const bool chw = d->out_layout == ZJ_LAYOUT_CHW && d->out_colorspace == ZJ_CS_RGB;
    const size_t row = chw ? (size_t)d->width : (size_t)d->width * (size_t)ncomp_of(d->out_colorspace);
    const size_t pitch = d->out_pitch > row ? (size_t)d->out_pitch : row;
    return pitch * d->height * (chw ? 3 : 1);
}

/* ---- memory helpers ------------------------------------------------------------------------- */
// ZJ_PINNED_KIND chooses how zj_alloc_pinned gets its memory (an A/B switch: profiles/r06_feeder_ab.txt):
//   0 hipHostMalloc, portable (the default: the planes of a zj_pool are filled by entropy threads and read by submitter
//     threads' contexts, possibly on another device)
//   1 hipHostMalloc, default flags      2 hipHostMalloc, portable | NumaUser (the pages follow the calling thread's policy)
//   3 page-aligned heap memory, touched by the calling thread, then hipHostRegister'ed (portable)
//   4 hipHostMalloc, portable | non-coherent
// Registered blocks are remembered so that zj_free_pinned can undo them.
// Freed hipHostMalloc blocks are kept for the next caller (round 6): pinning 200 MB of planes costs tens of milliseconds, and
// a caller that makes a new decoder per file, as the reference's own benchmark does (benches/decode.rs:9-14), would pay it
// per file.  A block is handed out again to a request of at least half its size with the same flags on the same device (its
// pages live on that device's NUMA node); at most ZJ_PINNED_CACHE_MB (default 512, 0 = off) stay cached.
namespace {
std::mutex g_reg_mu;
std::vector<void*> g_registered;
struct PinnedBlock { void* p; size_t bytes; unsigned flags; int device; };
std::vector<PinnedBlock> g_pin_live, g_pin_free;
size_t g_pin_free_bytes = 0;
size_t pinned_cache_limit()
{
    static const size_t lim = [] {
        long mb = 512;
        if (const char* e = getenv("ZJ_PINNED_CACHE_MB")) mb = atol(e);
        return mb > 0 ? (size_t)mb << 20 : (size_t)0;
    }();
    return lim;
}
}
void* zj_alloc_pinned(size_t bytes)
{
    void* p = nullptr;
    int kind = 0;
    if (const char* e = getenv("ZJ_PINNED_KIND")) kind = atoi(e);
    if (!bytes) bytes = 1;
    if (kind == 3) {
        const size_t len = (bytes + 4095) & ~(size_t)4095;
        p = aligned_alloc(4096, len);
        if (!p) return nullptr;
        for (size_t o = 0; o < len; o += 4096) ((volatile char*)p)[o] = 0; // first touch: the pages land on this thread's node
        if (hipHostRegister(p, len, hipHostRegisterPortable) != hipSuccess) { (void)hipGetLastError(); free(p); return nullptr; }
        std::lock_guard<std::mutex> lk(g_reg_mu);
        g_registered.push_back(p);
        return p;
    }
    const unsigned flags = kind == 1 ? hipHostMallocDefault
                         : kind == 2 ? (hipHostMallocPortable | hipHostMallocNumaUser)
                         : kind == 4 ? (hipHostMallocPortable | hipHostMallocNonCoherent)
                                     : hipHostMallocPortable;
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) { (void)hipGetLastError(); device = 0; }
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        size_t best = g_pin_free.size();
        for (size_t i = 0; i < g_pin_free.size(); i++) {
            const PinnedBlock& f = g_pin_free[i];
            if (f.flags == flags && f.device == device && f.bytes >= bytes && f.bytes / 2 <= bytes &&
                (best == g_pin_free.size() || f.bytes < g_pin_free[best].bytes)) best = i;
        }
        if (best != g_pin_free.size()) {
            const PinnedBlock f = g_pin_free[best];
            g_pin_free.erase(g_pin_free.begin() + (long)best);
            g_pin_free_bytes -= f.bytes;
            g_pin_live.push_back(f);
            return f.p;
        }
    }
    if (hipHostMalloc(&p, bytes, flags) != hipSuccess) {
        (void)hipGetLastError();
        // out of pinned memory with blocks lying idle: give them back and try once more
        std::vector<PinnedBlock> idle;
        {
            std::lock_guard<std::mutex> lk(g_reg_mu);
            idle.swap(g_pin_free);
            g_pin_free_bytes = 0;
        }
        if (idle.empty()) return nullptr;
        for (const PinnedBlock& f : idle) (void)hipHostFree(f.p);
        if (hipHostMalloc(&p, bytes, flags) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    }
    std::lock_guard<std::mutex> lk(g_reg_mu);
    g_pin_live.push_back(PinnedBlock{p, bytes, flags, device});
    return p;
}
int zj_device_pci_bus_id(int device, char* buf, size_t cap)
{
    if (!buf || cap < 16) return ZJ_ERR_ARG;
    const int n = zj_device_count();
    if (n <= 0) return ZJ_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return ZJ_ERR_ARG;
    if (hipDeviceGetPCIBusId(buf, (int)cap, device) != hipSuccess) { (void)hipGetLastError(); return ZJ_ERR_HIP; }
    return ZJ_OK;
}
int zj_set_thread_device(int device)
{
    const int n = zj_device_count();
    if (n <= 0) return ZJ_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return ZJ_ERR_ARG;
    return hipSetDevice(device) == hipSuccess ? ZJ_OK : ZJ_ERR_HIP;
}
void zj_free_pinned(void* p)
{
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        for (size_t i = 0; i < g_registered.size(); i++)
            if (g_registered[i] == p) {
                g_registered.erase(g_registered.begin() + (long)i);
                (void)hipHostUnregister(p);
                free(p);
                return;
            }
        for (size_t i = 0; i < g_pin_live.size(); i++)
            if (g_pin_live[i].p == p) {
                const PinnedBlock f = g_pin_live[i];
                g_pin_live.erase(g_pin_live.begin() + (long)i);
                if (g_pin_free_bytes + f.bytes <= pinned_cache_limit()) { g_pin_free.push_back(f); g_pin_free_bytes += f.bytes; return; }
                break;
            }
    }
    (void)hipHostFree(p);
}
int zj_pointer_device(const void* p)
{
    if (!p) return ZJ_ERR_ARG;
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof a);
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return ZJ_ERR_ARG; }
    if (a.type != hipMemoryTypeDevice) return ZJ_ERR_ARG;
    return a.device;
}
void* zj_device_alloc(zj_ctx* c, size_t bytes)
{
    if (!c || hipSetDevice(c->device) != hipSuccess) return nullptr;
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) return nullptr;
    return p;
}
void zj_device_free(zj_ctx* c, void* p) { if (c && p) { (void)hipSetDevice(c->device); (void)hipFree(p); } }
int zj_memcpy_h2d(zj_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c) return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    ZJ_HIP(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    ZJ_HIP(c, hipStreamSynchronize(c->stream));
    return ZJ_OK;
}
int zj_memcpy_d2h(zj_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c) return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    ZJ_HIP(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    ZJ_HIP(c, hipStreamSynchronize(c->stream));
    return ZJ_OK;
}
int zj_sync(zj_ctx* c)
{
    if (!c) return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    ZJ_HIP(c, hipStreamSynchronize(c->stream));
    return ZJ_OK;
}

// The launch itself, shared by the contiguous / strided form and the scattered form.
static int launch_params(zj_ctx* c, const Plan& pl, Params& p, hipStream_t s, bool may_stagger = true)
{
#if defined(ZJ_ABLATION)
    p.debug = c->debug;
#endif
    // Short launches of the 4:2:0 kernels (between one and two waves of workgroups: one 4096x4096 frame at a time, BASELINE
    // configs[1] read literally) start their first wave staggered, see stagger_start in zj_kernels.hip: 27.9 -> 24.3 us per
    // frame (profiles/r04_single_frame.txt).  That is the only regime it was measured in, so it is the only one that gets
    // it: a grid smaller than one wave of workgroups, or longer than two, starts as the hardware dispatches it.  The slots
    // per CU are the occupancy of the instantiation that is launched, not a constant.
    // (may_stagger false: the units of the pipelined host path -- strip ranges of a frame that overlap with copies on two
    // other streams; a unit can land in the 1..2-wave window, but nobody has measured the stagger there)
    if (may_stagger && c->stagger_delay > 0 && pl.hs == 2 && pl.vs == 2 && pl.out != OUT_GRAY && c->variant != 1) {
        const int slots = pl.fast ? fused_slots_per_cu(pl.hs, pl.vs, pl.out, c->variant, 1, p) : 0;
        const int wgs = c->cus * slots;
        if (slots >= 2 && p.total_tiles > wgs && p.total_tiles <= 2 * wgs) {
            p.stagger_wgs = wgs; p.stagger_delay = c->stagger_delay;
            const Magic g = magic_u31((uint32_t)c->cus);
            p.stagger_magic = g.m; p.stagger_shift = g.s;
        }
    }
    ZJ_HIP(c, launch_fused(pl.hs, pl.vs, pl.out, c->variant, launch_mode(pl, c->variant), p, s));
    return ZJ_OK;
}

/* ---- frame / batch level -------------------------------------------------------------------- */
// y_stride / c_stride (int16 elements) / out_stride (bytes): distance between the frames' planes / pixels when they are
// not packed back to back (0: they are)
static int decode_device_impl(zj_ctx* c, const zj_frame_desc* d, const Plan& pl, size_t nframes,
                              const int16_t* d_y, const int16_t* d_cb, const int16_t* d_cr,
                              uint8_t* d_out, hipStream_t s, int zero_fill, long long y_stride = 0, long long c_stride = 0,
                              long long out_stride = 0)
{
    Params p; // carries the quantisation tables by value: nothing to stage, nothing to order across streams
    fill_params(d, pl, nframes, d_y, d_cb, d_cr, d_out, zero_fill, p);
    if (y_stride) p.y_frame_stride = y_stride;
    if (c_stride) p.c_frame_stride = c_stride;
    if (out_stride) p.out_frame_stride = out_stride;
    const size_t ostride = out_stride ? (size_t)out_stride : pl.out_len;
    if (zero_fill) {
        // rows below the last complete strip are never written by the reference (Q6): zeros
        size_t off[3], len[3];
        ZeroRows z{};
        z.nr = uncovered_ranges(d, pl, off, len);
        for (int r = 0; r < z.nr; r++) { z.off[r] = off[r]; z.len[r] = len[r]; }
        z.frame_stride = (long long)ostride;
        for (size_t f0 = 0; z.nr && f0 < nframes; f0 += 16384) { // (grid.y <= 65535)
            z.out = d_out + f0 * ostride;
            z.nframes = (int)(nframes - f0 < 16384 ? nframes - f0 : 16384);
            ZJ_HIP(c, launch_zero_rows(z, s));
        }
    }
#if defined(ZJ_ABLATION)
    // Experiment of round 4, diagnostic build only: ONE frame cut into ZJ_SPLIT strip ranges (strips
    // are independent, src/mcu.rs:225-226) launched on internal streams that are forked from and joined to the caller's
    // stream by events.  Measured in profiles/r04_single_frame.txt: the fork / join costs more than the overlap gains.
    static const int split = [] { const char* e = getenv("ZJ_SPLIT"); const int v = e ? atoi(e) : 0; return v >= 2 && v <= 4 ? v : 0; }();
    if (split && nframes == 1 && pl.n_strips >= 2 * split) {
        static hipStream_t in[4] = {nullptr, nullptr, nullptr, nullptr};
        static hipEvent_t fork = nullptr, join[4];
        if (!fork) {
            ZJ_HIP(c, hipEventCreateWithFlags(&fork, hipEventDisableTiming));
            for (int i = 0; i < 4; i++) { ZJ_HIP(c, hipStreamCreateWithFlags(&in[i], hipStreamNonBlocking)); ZJ_HIP(c, hipEventCreateWithFlags(&join[i], hipEventDisableTiming)); }
        }
        ZJ_HIP(c, hipEventRecord(fork, s));
        const int per = (pl.n_strips + split - 1) / split;
        for (int r = 0; r < split; r++) {
            const int s0 = r * per, s1 = (s0 + per < pl.n_strips) ? s0 + per : pl.n_strips;
            Params q = p;
            size_t yrow, crow;
            plan_strip_elems(pl, yrow, crow);
            q.y = p.y + s0 * yrow; q.cb = p.cb ? p.cb + s0 * crow : nullptr; q.cr = p.cr ? p.cr + s0 * crow : nullptr;
            q.out = p.out + (size_t)s0 * pl.strip_rows * pl.out_pitch;
            q.height = (int)d->height - s0 * pl.strip_rows;
            set_grid(q, 1, s1 - s0, pl.tiles_per_row);
            ZJ_HIP(c, hipStreamWaitEvent(in[r], fork, 0));
            { const int rc = launch_params(c, pl, q, in[r]); if (rc) return rc; }
            ZJ_HIP(c, hipEventRecord(join[r], in[r]));
            ZJ_HIP(c, hipStreamWaitEvent(s, join[r], 0));
        }
        return ZJ_OK;
    }
#endif
    return launch_params(c, pl, p, s);
}

// Frames that are independent allocations (device pointers in HOST arrays, read during the call): launches of up to
// SCATTER_MAX frames whose addresses travel in the kernel arguments.  Frames that turn out to be equally spaced -- the
// images of one tensor, the slots of an arena -- take the strided form instead: one launch whatever their number.
static int decode_frames_device_impl(zj_ctx* c, const zj_frame_desc* d, const Plan& pl, size_t nframes, const int16_t* const* y,
                                     const int16_t* const* cb, const int16_t* const* cr, uint8_t* const* out, hipStream_t s,
                                     int zero_fill)
{
    const bool chroma = pl.out != OUT_GRAY;
    if (nframes == 1) return decode_device_impl(c, d, pl, 1, y[0], chroma ? cb[0] : nullptr, chroma ? cr[0] : nullptr, out[0], s, zero_fill);
    {
        const long long ys = y[1] - y[0], cs = chroma ? cb[1] - cb[0] : 0, os = out[1] - out[0];
        bool uniform = ys >= (long long)pl.y_len && os >= (long long)pl.out_len && (!chroma || (cs >= (long long)pl.c_len && cr[1] - cr[0] == cs));
        for (size_t f = 2; f < nframes && uniform; f++)
            uniform = y[f] - y[f - 1] == ys && out[f] - out[f - 1] == os && (!chroma || (cb[f] - cb[f - 1] == cs && cr[f] - cr[f - 1] == cs));
        if (uniform) return decode_device_impl(c, d, pl, nframes, y[0], chroma ? cb[0] : nullptr, chroma ? cr[0] : nullptr, out[0], s, zero_fill, ys, cs, os);
    }
    size_t off[3], len[3];
    const int nr = zero_fill ? uncovered_ranges(d, pl, off, len) : 0;
    for (size_t f0 = 0; f0 < nframes; f0 += SCATTER_MAX) {
        const int n = (int)(nframes - f0 < (size_t)SCATTER_MAX ? nframes - f0 : (size_t)SCATTER_MAX);
        Params p;
        fill_params(d, pl, (size_t)n, nullptr, nullptr, nullptr, nullptr, zero_fill, p);
        set_scatter(p, y, chroma ? cb : nullptr, chroma ? cr : nullptr, out, f0, n);
        if (nr) {
            ZeroRows z{};
            z.out = nullptr; z.frame_stride = 0; z.nr = nr; z.nframes = n;
            for (int r = 0; r < nr; r++) { z.off[r] = off[r]; z.len[r] = len[r]; }
            for (int f = 0; f < n; f++) z.fptr[f] = (uint64_t)(uintptr_t)out[f0 + f];
            ZJ_HIP(c, launch_zero_rows(z, s));
        }
        const int rc = launch_params(c, pl, p, s);
        if (rc) return rc;
    }
    return ZJ_OK;
}

static int check_frame_args(zj_ctx* c, const zj_frame_desc* d, size_t nframes, const void* y,
                            const void* cb, const void* cr, const void* out, Plan& pl)
{
    if (!c) return ZJ_ERR_ARG;
    int rc = make_plan(d, pl);
    if (rc) return rc;
    if (nframes == 0 || nframes > (size_t)1 << 20) return ZJ_ERR_ARG;
    if (!y || !out) return ZJ_ERR_ARG;
    if (pl.out != OUT_GRAY && (!cb || !cr)) return ZJ_ERR_ARG;
    if ((long long)nframes * pl.n_strips * pl.tiles_per_row > 0x7fffffffLL) return ZJ_ERR_ARG;
    return ZJ_OK;
}

int zj_decode_planes_device(zj_ctx* c, const zj_frame_desc* d, size_t nframes, const int16_t* d_y,
                            const int16_t* d_cb, const int16_t* d_cr, uint8_t* d_out, void* stream)
{
    Plan pl;
    int rc = check_frame_args(c, d, nframes, d_y, d_cb, d_cr, d_out, pl);
    if (rc) return rc;
    // planes: 16-byte aligned; pixels: 16-byte aligned when the rows are (width % 16 == 0) -- the rows of a ragged width
    // start at any byte anyway, and so may its frames (packed frames of 2500 x 1786 x 3 bytes are 8 bytes apart from it)
    if (((uintptr_t)d_y | (uintptr_t)d_cb | (uintptr_t)d_cr | (pl.fast ? (uintptr_t)d_out : 0)) & 15) return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return decode_device_impl(c, d, pl, nframes, d_y, d_cb, d_cr, d_out, s, 1);
}

int zj_decode_planes_device_strided(zj_ctx* c, const zj_frame_desc* d, size_t nframes, const int16_t* d_y, const int16_t* d_cb,
                                    const int16_t* d_cr, uint8_t* d_out, size_t y_stride, size_t c_stride, size_t out_stride,
                                    void* stream)
{
    Plan pl;
    int rc = check_frame_args(c, d, nframes, d_y, d_cb, d_cr, d_out, pl);
    if (rc) return rc;
    if (((uintptr_t)d_y | (uintptr_t)d_cb | (uintptr_t)d_cr | (pl.fast ? (uintptr_t)d_out : 0)) & 15) return ZJ_ERR_ARG;
    // 0 = packed; otherwise at least a frame, and every frame as aligned as the first
    if ((y_stride && (y_stride < pl.y_len || (y_stride & 7))) || (c_stride && (c_stride < pl.c_len || (c_stride & 7))) ||
        (out_stride && (out_stride < pl.out_len || (pl.fast && (out_stride & 15))))) return ZJ_ERR_ARG;
    if ((y_stride | c_stride | out_stride) >> 62) return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return decode_device_impl(c, d, pl, nframes, d_y, d_cb, d_cr, d_out, s, 1, (long long)y_stride, (long long)c_stride, (long long)out_stride);
}

int zj_decode_frames_device(zj_ctx* c, const zj_frame_desc* d, size_t nframes, const int16_t* const* d_y,
                            const int16_t* const* d_cb, const int16_t* const* d_cr, uint8_t* const* d_out, void* stream)
{
    Plan pl;
    int rc = check_frame_args(c, d, nframes, d_y, d_cb, d_cr, d_out, pl);
    if (rc) return rc;
    const bool chroma = pl.out != OUT_GRAY;
    for (size_t f = 0; f < nframes; f++) {
        if (!d_y[f] || !d_out[f] || (chroma && (!d_cb[f] || !d_cr[f]))) return ZJ_ERR_ARG;
        if (((uintptr_t)d_y[f] | (pl.fast ? (uintptr_t)d_out[f] : 0) | (chroma ? (uintptr_t)d_cb[f] | (uintptr_t)d_cr[f] : 0)) & 15) return ZJ_ERR_ARG;
    }
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return decode_frames_device_impl(c, d, pl, nframes, d_y, d_cb, d_cr, d_out, s, 1);
}

/* ---- crop windows ----------------------------------------------------------- */
size_t zj_crop_out_len(const zj_frame_desc* d, unsigned crop_w, unsigned crop_h, unsigned out_pitch)
{
    Plan pl;
    CropPlan cp;
    if (zero_output(d)) return make_zero_crop(d, crop_w, crop_h, out_pitch, cp) == ZJ_OK ? cp.out_len : 0;
    return make_crop_plan(d, crop_w, crop_h, out_pitch, pl, cp) == ZJ_OK ? cp.out_len : 0;
}

// every plane of frames [0, nframes): there, and 16-byte aligned (the kernels' loads)
static int check_plane_ptrs(const int16_t* const* d_y, const int16_t* const* d_cb, const int16_t* const* d_cr, bool chroma,
                            size_t nframes)
{
    if (!d_y || (chroma && (!d_cb || !d_cr))) return ZJ_ERR_ARG;
    for (size_t f = 0; f < nframes; f++) {
        if (!d_y[f] || (chroma && (!d_cb[f] || !d_cr[f]))) return ZJ_ERR_ARG;
        if (((uintptr_t)d_y[f] | (chroma ? (uintptr_t)d_cb[f] | (uintptr_t)d_cr[f] : 0)) & 15) return ZJ_ERR_ARG;
    }
    return ZJ_OK;
}

// Host planes to the context's scratch, on the context stream: the elements [r0, r1) x yrow of y (x crow of cb and cr, with
// chroma) at their full-frame offsets -- whole strips or MCU rows are contiguous ranges of a plane, and nothing reads across
// one.  dev: the device planes.
static int upload_plane_rows(zj_ctx* c, const Plan& pl, bool chroma, const int16_t* y, const int16_t* cb, const int16_t* cr,
                             size_t r0, size_t r1, size_t yrow, size_t crow, const int16_t* dev[3])
{
    int rc;
    if ((rc = ensure_scratch(c, 0, pl.y_len * 2))) return rc;
    if (chroma && ((rc = ensure_scratch(c, 1, pl.c_len * 2)) || (rc = ensure_scratch(c, 2, pl.c_len * 2)))) return rc;
    if (r1 > r0) {
        ZJ_HIP(c, hipMemcpyAsync((int16_t*)c->scratch[0] + r0 * yrow, y + r0 * yrow, (r1 - r0) * yrow * 2, hipMemcpyHostToDevice, c->stream));
        if (chroma) {
            ZJ_HIP(c, hipMemcpyAsync((int16_t*)c->scratch[1] + r0 * crow, cb + r0 * crow, (r1 - r0) * crow * 2, hipMemcpyHostToDevice, c->stream));
            ZJ_HIP(c, hipMemcpyAsync((int16_t*)c->scratch[2] + r0 * crow, cr + r0 * crow, (r1 - r0) * crow * 2, hipMemcpyHostToDevice, c->stream));
        }
    }
    dev[0] = (const int16_t*)c->scratch[0];
    dev[1] = chroma ? (const int16_t*)c->scratch[1] : nullptr; dev[2] = chroma ? (const int16_t*)c->scratch[2] : nullptr;
    return ZJ_OK;
}

// Zeros for the rows of the crops of frames [f0, f0 + n) that lie at or below rows_covered (Q6; rows_covered 0: every row,
// the all-zero output), from a launch of their own, if any frame has such rows.  win, stride: as fill_crop_params_win's
// (stride 2: every window cp.w x cp.h at cp.out_pitch; stride 4: each crop tight at its own size).
static int crop_zero_launch(zj_ctx* c, int rows_covered, const CropPlan& cp, const unsigned* win, int stride, uint8_t* const* out,
                            size_t f0, int n, hipStream_t s)
{
    CropZero z{};
    z.rows_covered = rows_covered; z.nplanes = cp.nplanes; z.bpp = cp.bpp; z.nframes = n;
    if (stride == 2) {
        z.crop_h = cp.h; z.nbytes = cp.w * cp.bpp;
        z.out_pitch = (int)cp.out_pitch; z.crop_plane = (long long)cp.out_pitch * cp.h;
    }
    bool any = false;
    for (int f = 0; f < n; f++) {
        const unsigned* const w = win + (size_t)stride * (f0 + f);
        unsigned h = (unsigned)cp.h;
        z.fptr[f] = (uint64_t)(uintptr_t)out[f0 + f];
        z.y0[f] = w[1];
        if (stride == 4) {
            h = w[3];
            z.size[f] = w[2] | (w[3] << 16);
            if ((int)w[3] > z.crop_h) z.crop_h = (int)w[3];
            if ((int)(w[2] * cp.bpp) > z.nbytes) z.nbytes = (int)(w[2] * cp.bpp);
        }
        any = any || (long long)w[1] + h > rows_covered;
    }
    if (any) ZJ_HIP(c, launch_crop_zero(z, s));
    return ZJ_OK;
}

// frames [0, nframes) of ONE geometry, each cut to its own window (win, stride: as fill_crop_params_win's); launches of up
// to SCATTER_MAX frames (grid.z)
static int decode_crops_impl(zj_ctx* c, const zj_frame_desc* d, const Plan& pl, const CropPlan& cp, size_t nframes,
                             const int16_t* const* y, const int16_t* const* cb, const int16_t* const* cr, const unsigned* win,
                             int stride, uint8_t* const* out, hipStream_t s)
{
    const bool chroma = pl.out != OUT_GRAY;
    for (size_t f0 = 0; f0 < nframes; f0 += SCATTER_MAX) {
        const int n = (int)(nframes - f0 < (size_t)SCATTER_MAX ? nframes - f0 : (size_t)SCATTER_MAX);
        CropParams p;
        int nstrips = 0, ncols = 0;
        fill_crop_params_win(d, pl, cp, y, chroma ? cb : nullptr, chroma ? cr : nullptr, out, win, stride, f0, n, p, nstrips, ncols);
        const int rc = crop_zero_launch(c, pl.rows_covered, cp, win, stride, out, f0, n, s);
        if (rc) return rc;
        ZJ_HIP(c, launch_crop(pl.hs, pl.vs, pl.out, p, s));
    }
    return ZJ_OK;
}

static int check_crop_args(zj_ctx* c, const zj_frame_desc* d, size_t nframes, const unsigned* origins, unsigned crop_w,
                           unsigned crop_h, unsigned out_pitch, Plan& pl, CropPlan& cp)
{
    if (!c || !origins || nframes == 0 || nframes > (size_t)1 << 20) return ZJ_ERR_ARG;
    int rc = make_crop_plan(d, crop_w, crop_h, out_pitch, pl, cp);
    if (rc) return rc;
    for (size_t f = 0; f < nframes; f++) {
        int s0, s1, k0, k1;
        if ((rc = crop_window(d, pl, cp, origins[2 * f], origins[2 * f + 1], s0, s1, k0, k1))) return rc;
    }
    return ZJ_OK;
}

int zj_decode_crops_device(zj_ctx* c, const zj_frame_desc* d, size_t nframes, const int16_t* const* d_y,
                           const int16_t* const* d_cb, const int16_t* const* d_cr, const unsigned* origins,
                           unsigned crop_w, unsigned crop_h, uint8_t* const* d_out, unsigned out_pitch, void* stream)
{
    Plan pl;
    CropPlan cp;
    int rc = check_crop_args(c, d, nframes, origins, crop_w, crop_h, out_pitch, pl, cp);
    if (rc) return rc;
    if (!d_out || (rc = check_plane_ptrs(d_y, d_cb, d_cr, pl.out != OUT_GRAY, nframes))) return ZJ_ERR_ARG;
    for (size_t f = 0; f < nframes; f++)
        if (!d_out[f]) return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return decode_crops_impl(c, d, pl, cp, nframes, d_y, d_cb, d_cr, origins, 2, d_out, s);
}

// Library-internal (zj_jpeg.cpp: zj_decoder_finish_pixels_crop_device).  One frame's window on the context stream, from
// planes in host memory -- only the strips the window needs are uploaded, each at its full-frame offset in the context's
// scratch (strips are contiguous row ranges of a plane and no filter reads across one) -- or from planes already in HBM.
int zjint_crop_frame(zj_ctx* c, const zj_frame_desc* d, const int16_t* y, const int16_t* cb, const int16_t* cr,
                     int planes_on_device, unsigned x, unsigned yy, unsigned w, unsigned h, uint8_t* d_out, unsigned out_pitch)
{
    Plan pl;
    CropPlan cp;
    const unsigned origin[2] = {x, yy};
    int rc = check_crop_args(c, d, 1, origin, w, h, out_pitch, pl, cp);
    if (rc) return rc;
    const bool chroma = pl.out != OUT_GRAY;
    if (!y || !d_out || (chroma && (!cb || !cr))) return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    const int16_t* p[3] = {y, cb, cr};
    if (!planes_on_device) {
        int s0, s1, k0, k1;
        crop_window(d, pl, cp, x, yy, s0, s1, k0, k1);
        // i16 elements per strip (the split of decode_device_impl's ZJ_SPLIT experiment)
        size_t yrow, crow;
        plan_strip_elems(pl, yrow, crow);
        if ((rc = upload_plane_rows(c, pl, chroma, y, cb, cr, (size_t)s0, (size_t)s1, yrow, crow, p))) return rc;
    }
    if ((rc = decode_crops_impl(c, d, pl, cp, 1, &p[0], &p[1], &p[2], origin, 2, &d_out, c->stream))) return rc;
    ZJ_HIP(c, hipStreamSynchronize(c->stream));
    return ZJ_OK;
}

// Library-internal: the window of an all-zero output (zj_plan.h: make_zero_crop): zeros in the window's rows, the pitch
// padding untouched
int zjint_crop_zeros(zj_ctx* c, const zj_frame_desc* d, unsigned x, unsigned yy, unsigned w, unsigned h, uint8_t* d_out, unsigned out_pitch)
{
    CropPlan cp;
    if (!c || !d_out || !zero_output(d)) return ZJ_ERR_ARG;
    int rc = make_zero_crop(d, w, h, out_pitch, cp);
    if (rc) return rc;
    if ((size_t)x + w > d->width || (size_t)yy + h > d->height) return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    const unsigned origin[2] = {x, yy};
    if ((rc = crop_zero_launch(c, 0, cp, origin, 2, &d_out, 0, 1, c->stream))) return rc;
    ZJ_HIP(c, hipStreamSynchronize(c->stream));
    return ZJ_OK;
}

/* ---- resize + normalise ---------------------------------------------------------- */
namespace {
// The output side of a resized call, as every layer below the entry points takes it: the dense tensor at d_out, image i of
// the call at d_out + i * img_bytes, flipped if flip[i] (nullptr: none).
struct ResizeOut {
    unsigned out_w, out_h;
    int dtype, layout;          // ZJ_DTYPE_*, ZJ_TENSOR_*
    const float *scale, *bias;  // the caller's (nullptr: 1, 0)
    const uint8_t* flip;
    int filter;
    uint8_t* d_out;
    // resize_out_args:
    int ch;                     // channels of the u8 images
    float s[3], b[3];           // the per-channel factors of the kernel (s_c = scale_c * 2^-16)
    size_t img_bytes;           // of one image of the output
    bool chw;                   // the u8 images are CHW planes (the caller's to set)
};

// The affine warp's own arguments next to a ResizeOut (whose flip and filter it ignores): the fill bytes,
// fill[c] << 8 c, and the edge mode
struct WarpTail { uint32_t fill; int edge; };

ResizeOut resize_out(unsigned out_w, unsigned out_h, int dtype, int out_layout, const float* scale, const float* bias,
                     const uint8_t* flip, int filter, void* d_out)
{
    ResizeOut o{};
    o.out_w = out_w; o.out_h = out_h; o.dtype = dtype; o.layout = out_layout;
    o.scale = scale; o.bias = bias; o.flip = flip; o.filter = filter; o.d_out = (uint8_t*)d_out;
    return o;
}

// the check of the output's arguments, for u8 images of `channels`
int resize_out_args(ResizeOut& o, int channels)
{
    o.ch = channels;
    o.img_bytes = resized_len(channels, o.out_w, o.out_h, o.dtype);
    if (!o.img_bytes) return ZJ_ERR_ARG; // (the size or the dtype)
    if (o.layout != ZJ_TENSOR_NCHW && o.layout != ZJ_TENSOR_NHWC) return ZJ_ERR_ARG;
    return kernel_factors(o.scale, o.bias, channels, o.s, o.b) ? ZJ_OK : ZJ_ERR_ARG;
}

// the tensor of the stage records (zj_stage_pack.h) that o names
StageTensor stage_tensor(const ResizeOut& o)
{
    StageTensor t{o.d_out, o.img_bytes, (int)o.out_w, (int)o.out_h, o.dtype, o.layout == ZJ_TENSOR_NHWC, {}, {}};
    for (int k = 0; k < 3; k++) { t.s[k] = o.s[k]; t.b[k] = o.b[k]; }
    return t;
}

// images [0, n) -> images [first, first + n) of the output, launches of up to RESIZE_BATCH images; wh[2i], wh[2i + 1]: image
// i's size, pitch[i] (bytes between its rows) already resolved
int resize_launches(zj_ctx* c, size_t n, const uint8_t* const* in, const unsigned* wh, const unsigned* pitch, const ResizeOut& o,
                    size_t first, hipStream_t st)
{
    const StageTensor t = stage_tensor(o);
    ResizeParams p{};
    return stage_batches<RESIZE_BATCH>(n, [&](size_t f0, int m) {
        pack_resize(p, in, wh, pitch, o.flip ? o.flip + first : nullptr, t, first, f0, m);
        ZJ_HIP(c, o.filter == ZJ_RESIZE_BICUBIC_AA    ? launch_resize_bicubic(o.ch, o.chw, o.dtype, t.nhwc, p, st)
                  : o.filter == ZJ_RESIZE_BILINEAR_AA ? launch_resize_aa(o.ch, o.chw, o.dtype, t.nhwc, p, st)
                                                      : launch_resize(o.ch, o.chw, o.dtype, t.nhwc, p, st));
        return ZJ_OK;
    });
}

// the crop buffer, at least `bytes`, free for writing on stream st: st waits for the last resize that read it (whichever
// stream that ran on); growing it waits for that resize on the host first
int resize_scratch(zj_ctx* c, size_t bytes, hipStream_t st, uint8_t** p)
{
    if (!c->rz_done) ZJ_HIP(c, hipEventCreateWithFlags(&c->rz_done, hipEventDisableTiming));
    if (bytes > c->rz_cap) {
        if (c->rz_used) ZJ_HIP(c, hipEventSynchronize(c->rz_done));
        if (c->rz_buf) { ZJ_HIP(c, hipFree(c->rz_buf)); c->rz_buf = nullptr; c->rz_cap = 0; }
        const size_t cap = bytes + bytes / 4 + 4096;
        ZJ_HIP(c, hipMalloc(&c->rz_buf, cap));
        c->rz_cap = cap;
    } else if (c->rz_used) {
        ZJ_HIP(c, hipStreamWaitEvent(st, c->rz_done, 0));
    }
    *p = (uint8_t*)c->rz_buf;
    return ZJ_OK;
}

int resize_scratch_done(zj_ctx* c, hipStream_t st)
{
    ZJ_HIP(c, hipEventRecord(c->rz_done, st));
    c->rz_used = true;
    return ZJ_OK;
}

// the end of a library-internal call of one image (zjint_*_one) on the context stream: the context's crop buffer counts as
// read by it; synchronised
int one_image_done(zj_ctx* c)
{
    if (!c->rz_done) ZJ_HIP(c, hipEventCreateWithFlags(&c->rz_done, hipEventDisableTiming));
    const int rc = resize_scratch_done(c, c->stream);
    if (rc) return rc;
    ZJ_HIP(c, hipStreamSynchronize(c->stream));
    return ZJ_OK;
}

// images [0, n) -> their displayed form, launches of up to ORIENT_BATCH images; wh: STORED w, h pairs, the
// pitches resolved, every o[i] 1..8
int orient_launches(zj_ctx* c, size_t n, const uint8_t* const* in, const unsigned* wh, const unsigned* in_pitch, int channels,
                    int in_chw, const uint8_t* o, uint8_t* const* out, const unsigned* out_pitch, hipStream_t st)
{
    OrientParams p{};
    return stage_batches<ORIENT_BATCH>(n, [&](size_t f0, int m) {
        pack_orient(p, in, wh, in_pitch, o, out, out_pitch, f0, m);
        ZJ_HIP(c, launch_orient(channels, in_chw, p, st));
        return ZJ_OK;
    });
}

// planes [0, n) -> 3-channel images with every channel the plane, launches of up to EXPAND_BATCH images; wh:
// w, h pairs, the pitches resolved
int expand_launches(zj_ctx* c, size_t n, const uint8_t* const* in, const unsigned* wh, const unsigned* in_pitch, int out_chw,
                    uint8_t* const* out, const unsigned* out_pitch, hipStream_t st)
{
    ExpandParams p{};
    return stage_batches<EXPAND_BATCH>(n, [&](size_t f0, int m) {
        pack_expand(p, in, wh, in_pitch, out, out_pitch, f0, m);
        ZJ_HIP(c, launch_expand(out_chw, p, st));
        return ZJ_OK;
    });
}

// image pairs [0, n) -> out[c] = (a[c] * k + 127) / 255, launches of up to CMYK_BATCH pairs; wh: w, h pairs, the
// pitches resolved, inverted[i] != 0: the samples are used as stored, else complemented first
int cmyk_launches(zj_ctx* c, size_t n, const uint8_t* const* a, const uint8_t* const* k, const unsigned* wh, const unsigned* a_pitch,
                  const unsigned* k_pitch, int chw, const uint8_t* inverted, uint8_t* const* out, const unsigned* out_pitch,
                  hipStream_t st)
{
    CmykParams p{};
    return stage_batches<CMYK_BATCH>(n, [&](size_t f0, int m) {
        pack_cmyk(p, a, k, wh, a_pitch, k_pitch, inverted, out, out_pitch, f0, m);
        ZJ_HIP(c, launch_cmyk(chw, p, st));
        return ZJ_OK;
    });
}

// images [0, n) under their colour matrices, launches of up to COLOR_BATCH images; wh: w, h pairs, the pitches
// resolved, q: 12 integers per image (color_fixed)
int color_launches(zj_ctx* c, size_t n, const uint8_t* const* in, const unsigned* wh, const unsigned* in_pitch, int chw,
                   const int32_t* q, uint8_t* const* out, const unsigned* out_pitch, hipStream_t st)
{
    ColorParams p{};
    return stage_batches<COLOR_BATCH>(n, [&](size_t f0, int m) {
        pack_color(p, in, wh, in_pitch, q, out, out_pitch, f0, m);
        ZJ_HIP(c, launch_color(chw, p, st));
        return ZJ_OK;
    });
}

// the 12 integers of each of n matrices of doubles, 12 each
int color_matrices(const double* matrices, size_t n, std::vector<int32_t>& q)
{
    q.resize(12 * n);
    for (size_t f = 0; f < n; f++)
        if (!color_fixed(matrices + 12 * f, q.data() + 12 * f)) return ZJ_ERR_ARG;
    return ZJ_OK;
}

/* ---- the tone stages' launches ---- */
// images [0, n) counted into their tables hist[f] (uint32 [channels][256], zeroed on the stream in front of this), launches of
// up to HIST_BATCH images; wh: w, h pairs, the pitches resolved
int hist_launches(zj_ctx* c, size_t n, const uint8_t* const* in, const unsigned* wh, const unsigned* pitch, int channels, int chw,
                  const uint8_t* const* hist, hipStream_t st)
{
    HistParams p{};
    return stage_batches<HIST_BATCH>(n, [&](size_t f0, int m) {
        pack_hist(p, in, wh, pitch, hist, f0, m);
        ZJ_HIP(c, launch_hist(channels, chw, p, st));
        return ZJ_OK;
    });
}

// the tables of n ops (op, param pairs, all valid) into luts, uint8 [n][channels][256]; hist: uint32 [n][channels][256], read
// for the ops that need one (nullptr: none does)
int tone_lut_launches(zj_ctx* c, size_t n, int channels, const int32_t* ops, const uint32_t* hist, uint8_t* luts, hipStream_t st)
{
    ToneLutParams p{};
    return stage_batches<TONE_LUT_BATCH>(n, [&](size_t f0, int m) {
        pack_tone_lut(p, ops, hist, luts, channels, f0, m);
        ZJ_HIP(c, launch_tone_lut(p, st));
        return ZJ_OK;
    });
}

// images [0, n) through their tables luts[f][c][.], launches of up to LUT_BATCH images
int lut_launches(zj_ctx* c, size_t n, const uint8_t* const* in, const unsigned* wh, const unsigned* in_pitch, int channels, int chw,
                 const uint8_t* luts, uint8_t* const* out, const unsigned* out_pitch, hipStream_t st)
{
    LutParams p{};
    return stage_batches<LUT_BATCH>(n, [&](size_t f0, int m) {
        pack_lut(p, in, wh, in_pitch, luts, channels, out, out_pitch, f0, m);
        ZJ_HIP(c, launch_lut(channels, chw, p, st));
        return ZJ_OK;
    });
}

// the tone stage's buffer, at least `bytes`, free for writing on stream st: resize_scratch's rule with the tone stage's event
int tone_scratch(zj_ctx* c, size_t bytes, hipStream_t st, uint8_t** p)
{
    if (!c->tone_done) ZJ_HIP(c, hipEventCreateWithFlags(&c->tone_done, hipEventDisableTiming));
    if (bytes > c->tone_cap) {
        if (c->tone_used) ZJ_HIP(c, hipEventSynchronize(c->tone_done));
        if (c->tone_buf) { ZJ_HIP(c, hipFree(c->tone_buf)); c->tone_buf = nullptr; c->tone_cap = 0; }
        const size_t cap = bytes + bytes / 4 + 4096;
        ZJ_HIP(c, hipMalloc(&c->tone_buf, cap));
        c->tone_cap = cap;
    } else if (c->tone_used) {
        ZJ_HIP(c, hipStreamWaitEvent(st, c->tone_done, 0));
    }
    *p = (uint8_t*)c->tone_buf;
    return ZJ_OK;
}

// n ops of two int32 each: all of them ones the stage takes
bool tone_ops_valid(const int32_t* ops, size_t n)
{
    for (size_t f = 0; f < n; f++)
        if (!tone_op_valid(ops[2 * f], ops[2 * f + 1])) return false;
    return true;
}

// zj_tone_device behind its checks: images [0, n) under their ops (op, param pairs, all valid), every image of the list in
// every launch it needs -- the histogram for the ops that need one, into the context's buffer, zeroed in front; the table
// build; the lookup.  All on st: the kernel boundaries are the only ordering.
int tone_launches(zj_ctx* c, size_t n, const uint8_t* const* in, const unsigned* wh, const unsigned* in_pitch, int channels, int chw,
                  const int32_t* ops, uint8_t* const* out, const unsigned* out_pitch, hipStream_t st)
{
    const size_t tab = (size_t)channels * 256, hist_bytes = n * tab * 4;
    uint8_t* buf = nullptr;
    int rc = tone_scratch(c, hist_bytes + n * tab, st, &buf);
    if (rc) return rc;
    uint32_t* const hist = (uint32_t*)buf;
    uint8_t* const luts = buf + hist_bytes;
    std::vector<const uint8_t*> hin, htab;
    std::vector<unsigned> hwh, hp;
    for (size_t f = 0; f < n; f++)
        if (tone_needs_hist(ops[2 * f])) {
            hin.push_back(in[f]); htab.push_back((const uint8_t*)(hist + f * tab));
            hwh.push_back(wh[2 * f]); hwh.push_back(wh[2 * f + 1]);
            hp.push_back(in_pitch[f]);
        }
    // (whatever was queued reads or writes the buffer: the event is recorded behind it on the error paths as well, so that
    // the next user, on whichever stream, and a call that grows the buffer wait for it)
    const auto queue = [&]() -> int {
        if (!hin.empty()) {
            ZJ_HIP(c, hipMemsetAsync(hist, 0, hist_bytes, st));
            if (const int e = hist_launches(c, hin.size(), hin.data(), hwh.data(), hp.data(), channels, chw, htab.data(), st)) return e;
        }
        if (const int e = tone_lut_launches(c, n, channels, ops, hin.empty() ? nullptr : hist, luts, st)) return e;
        return lut_launches(c, n, in, wh, in_pitch, channels, chw, luts, out, out_pitch, st);
    };
    rc = queue();
    if (hipEventRecord(c->tone_done, st) == hipSuccess) c->tone_used = true;
    else if (!rc) { c->last_error = "hipEventRecord(c->tone_done, st) failed"; rc = ZJ_ERR_HIP; }
    return rc;
}

// images [0, n) -> their three component planes box-replicated and converted, launches of up to PLANES_BATCH
// images; wh: w, h pairs of the outputs, geo: planes_component of the three components, pitch: three per image, all resolved
int planes_launches(zj_ctx* c, size_t n, const uint8_t* const* p0, const uint8_t* const* p1, const uint8_t* const* p2,
                    const unsigned* wh, const uint32_t* geo, const unsigned* pitch, int stored_rgb, int chw, uint8_t* const* out,
                    const unsigned* out_pitch, hipStream_t st)
{
    const uint8_t* const* const planes[3] = {p0, p1, p2};
    PlanesParams p{};
    return stage_batches<PLANES_BATCH>(n, [&](size_t f0, int m) {
        pack_planes(p, planes, 1, pitch, wh, geo, out, out_pitch, f0, m);
        ZJ_HIP(c, launch_planes(chw, stored_rgb, p, st));
        return ZJ_OK;
    });
}

// The end of the launch group [g0, g1) of a resized call, its crops written into buf where `place` says (zj_rzgroup.h):
// the turned frames, gathered: crop -> its displayed form, tight, in the second region; the resize over the images place[f].in
// names, in order, into images [g0, g1) of the output; the event that orders the buffer's reuse.
// warp (nullptr: the resize): the group ends in the affine warp instead, frame f under the integers
// warp_q[6f .. 6f + 5].  Only the warp's calls have frames of an EMPTY window (w == 0: the output sees nothing of the frame,
// fill mode): such a frame has no crop, passes no stage in front of the warp -- the `p.in.w` below -- and gets a record no
// lane loads from (warp_launches).  The resized calls refuse an empty window before they come here.
// color_q (nullptr: none): frame f's image, the one the last stage reads, passes the colour stage in place
// under the integers color_q[12f .. 12f + 11] first; a frame with the identity's integers is left out of the launch.
// tone (nullptr: none): the same image then passes the tone stage in place under the op tone[2f], tone[2f + 1];
// ZJ_TONE_IDENTITY frames are left out of its launches.  Colour first, then tone.
int warp_launches(zj_ctx* c, size_t n, const uint8_t* const* in, const unsigned* wh, const unsigned* pitch, const int64_t* q,
                  const ResizeOut& o, const WarpTail& t, size_t first, hipStream_t st);

int rz_finish_group(zj_ctx* c, const RzFrame* fr, const RzPlace* place, size_t g0, size_t g1, uint8_t* buf, const ResizeOut& o,
                    hipStream_t st, const WarpTail* warp = nullptr, const int64_t* warp_q = nullptr, const int32_t* color_q = nullptr,
                    const int32_t* tone = nullptr)
{
    // the images of one stage of the group, gathered
    struct Stage {
        std::vector<const uint8_t*> in;
        std::vector<uint8_t*> out;
        std::vector<unsigned> wh, ip, op;
        std::vector<uint8_t> o;
        void add(uint8_t* buf, const RzImage& from, const RzImage& to, int orientation)
        {
            in.push_back(buf + from.off); out.push_back(buf + to.off);
            wh.push_back(from.w); wh.push_back(from.h);
            ip.push_back(from.pitch); op.push_back(to.pitch);
            o.push_back((uint8_t)orientation);
        }
    };
    const size_t ng = g1 - g0;
    std::vector<const uint8_t*> in(ng);
    std::vector<unsigned> wh(2 * ng), pitch(ng);
    Stage turn, turn_gray, expand, color, toned; // (the gray frames of a 3-channel call are turned as the 1-channel images they still are)
    std::vector<int32_t> cq, tq;
    for (size_t f = g0; f < g1; f++) {
        const RzPlace& p = place[f];
        in[f - g0] = buf + p.in.off;
        wh[2 * (f - g0)] = p.in.w; wh[2 * (f - g0) + 1] = p.in.h;
        pitch[f - g0] = p.in.pitch;
        if (p.turned) (p.expand ? turn_gray : turn).add(buf, p.crop, p.gray, fr[f].o);
        if (p.expand && p.in.w) expand.add(buf, p.gray, p.in, 1);
        if (color_q && p.in.w && !color_is_identity(color_q + 12 * f)) {
            color.add(buf, p.in, p.in, 1);
            cq.insert(cq.end(), color_q + 12 * f, color_q + 12 * f + 12);
        }
        if (tone && p.in.w && tone[2 * f] != TONE_IDENTITY) {
            toned.add(buf, p.in, p.in, 1);
            tq.insert(tq.end(), tone + 2 * f, tone + 2 * f + 2);
        }
    }
    int rc;
    if (!turn.in.empty() && (rc = orient_launches(c, turn.in.size(), turn.in.data(), turn.wh.data(), turn.ip.data(), o.ch, o.chw,
                                                  turn.o.data(), turn.out.data(), turn.op.data(), st)))
        return rc;
    if (!turn_gray.in.empty() && (rc = orient_launches(c, turn_gray.in.size(), turn_gray.in.data(), turn_gray.wh.data(),
                                                       turn_gray.ip.data(), 1, 0, turn_gray.o.data(), turn_gray.out.data(),
                                                       turn_gray.op.data(), st)))
        return rc;
    if (!expand.in.empty() && (rc = expand_launches(c, expand.in.size(), expand.in.data(), expand.wh.data(), expand.ip.data(),
                                                    o.chw, expand.out.data(), expand.op.data(), st)))
        return rc;
    if (!color.in.empty() && (rc = color_launches(c, color.in.size(), color.in.data(), color.wh.data(), color.ip.data(), o.chw,
                                                  cq.data(), color.out.data(), color.op.data(), st)))
        return rc;
    if (!toned.in.empty() && (rc = tone_launches(c, toned.in.size(), toned.in.data(), toned.wh.data(), toned.ip.data(), o.ch, o.chw,
                                                 tq.data(), toned.out.data(), toned.op.data(), st)))
        return rc;
    if ((rc = warp ? warp_launches(c, ng, in.data(), wh.data(), pitch.data(), warp_q + 6 * g0, o, *warp, g0, st)
                   : resize_launches(c, ng, in.data(), wh.data(), pitch.data(), o, g0, st)))
        return rc;
    return resize_scratch_done(c, st);
}
} // namespace

size_t zj_resized_out_len(const zj_frame_desc* d, unsigned out_w, unsigned out_h, int dtype)
{
    Plan pl;
    CropPlan cp;
    const int ch = resize_channels(d);
    if (!ch || gray_to_rgb_refused(d)) return 0;
    const zj_frame_desc e = resized_stage_desc(d); // (ZJ_FLAG_GRAY_TO_RGB: planned as the GRAYSCALE frame it is decoded as)
    if (zero_output(&e) ? make_zero_crop(&e, 1, 1, 0, cp) : make_crop_plan(&e, 1, 1, 0, pl, cp)) return 0;
    return resized_len(ch, out_w, out_h, dtype);
}

int zj_resize_device(zj_ctx* c, size_t n, const uint8_t* const* d_in, const unsigned* in_wh, const unsigned* in_pitch,
                     int channels, int in_layout, unsigned out_w, unsigned out_h, int dtype, int out_layout,
                     const float* scale, const float* bias, const uint8_t* flip, void* d_out, void* stream)
{
    return zj_resize_filtered_device(c, n, d_in, in_wh, in_pitch, channels, in_layout, out_w, out_h, dtype, out_layout, scale,
                                     bias, flip, ZJ_RESIZE_BILINEAR, d_out, stream);
}

int zj_resize_filtered_device(zj_ctx* c, size_t n, const uint8_t* const* d_in, const unsigned* in_wh, const unsigned* in_pitch,
                              int channels, int in_layout, unsigned out_w, unsigned out_h, int dtype, int out_layout,
                              const float* scale, const float* bias, const uint8_t* flip, int filter, void* d_out,
                              void* stream)
{
    if (!resize_filter_valid(filter)) return ZJ_ERR_ARG;
    if (!c || n == 0 || n > (size_t)1 << 20 || !d_in || !in_wh || !d_out) return ZJ_ERR_ARG;
    if (channels != 1 && channels != 3) return ZJ_ERR_ARG;
    if (in_layout != ZJ_LAYOUT_HWC && in_layout != ZJ_LAYOUT_CHW) return ZJ_ERR_ARG;
    ResizeOut ro = resize_out(out_w, out_h, dtype, out_layout, scale, bias, flip, filter, d_out);
    int rc = resize_out_args(ro, channels);
    if (rc) return rc;
    const bool chw = ro.chw = in_layout == ZJ_LAYOUT_CHW && channels == 3;
    std::vector<unsigned> pitch;
    if (!stage_images(n, d_in, in_wh, in_pitch, chw ? 1 : channels, pitch)) return ZJ_ERR_ARG;
    for (size_t f = 0; chw && f < n; f++)
        if ((size_t)pitch[f] * in_wh[2 * f + 1] * 3 > ((size_t)1 << 31)) return ZJ_ERR_ARG; // (the kernel's plane offsets)
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return resize_launches(c, n, d_in, in_wh, pitch.data(), ro, 0, st);
}

int zj_decode_crops_resized_device(zj_ctx* c, const zj_frame_desc* d, size_t nframes, const int16_t* const* d_y,
                                   const int16_t* const* d_cb, const int16_t* const* d_cr, const unsigned* windows,
                                   unsigned out_w, unsigned out_h, int dtype, int out_layout, const float* scale,
                                   const float* bias, const uint8_t* flip, void* d_out, void* stream)
{
    return zj_decode_crops_resized_filtered_device(c, d, nframes, d_y, d_cb, d_cr, windows, out_w, out_h, dtype, out_layout,
                                                   scale, bias, flip, ZJ_RESIZE_BILINEAR, d_out, stream);
}

/* the reduced-size decode's launches, which the prescaled resized crops below use as well */
// frames [0, nframes) of ONE geometry at one scale, each cut to its own window (win == nullptr: the whole reduced frame);
// launches of up to SCATTER_MAX frames (grid.z).  Arguments checked by the caller.
static int scaled_launches(zj_ctx* c, const zj_frame_desc* d, const Plan& pl, const ScaledPlan& sp, size_t nframes,
                           const int16_t* const* y, const int16_t* const* cb, const int16_t* const* cr, const unsigned* win,
                           uint8_t* const* out, unsigned out_pitch, hipStream_t s)
{
    const bool chroma = pl.out != OUT_GRAY;
    for (size_t f0 = 0; f0 < nframes; f0 += SCATTER_MAX) {
        const int n = (int)(nframes - f0 < (size_t)SCATTER_MAX ? nframes - f0 : (size_t)SCATTER_MAX);
        if (sp.zero) { // a single-component frame with a colour output: zeros in the windows' rows (zj_crop_out_len's rule)
            for (int f = 0; f < n; f++) { // (one launch each: with a pitch every window has a plane size of its own)
                const unsigned origin[2] = {0, 0};
                CropPlan zc{};
                zc.w = win ? (int)win[4 * (f0 + f) + 2] : sp.rw; zc.h = win ? (int)win[4 * (f0 + f) + 3] : sp.rh;
                zc.bpp = sp.bpp; zc.nplanes = sp.nplanes; zc.out_pitch = out_pitch ? out_pitch : (size_t)zc.w * sp.bpp;
                const int rc = crop_zero_launch(c, 0, zc, origin, 2, out + f0 + f, 0, 1, s);
                if (rc) return rc;
            }
            continue;
        }
        ScaledParams p;
        fill_scaled_params(d, pl, sp, y, chroma ? cb : nullptr, chroma ? cr : nullptr, out, win, out_pitch, f0, n, p);
        ZJ_HIP(c, launch_scaled(pl.hs, pl.vs, pl.out, sp.sl, p, s));
    }
    return ZJ_OK;
}

int zj_decode_crops_resized_filtered_device(zj_ctx* c, const zj_frame_desc* d, size_t nframes, const int16_t* const* d_y,
                                            const int16_t* const* d_cb, const int16_t* const* d_cr, const unsigned* windows,
                                            unsigned out_w, unsigned out_h, int dtype, int out_layout, const float* scale,
                                            const float* bias, const uint8_t* flip, int filter, void* d_out, void* stream)
{
    return zj_decode_crops_resized_prescaled_device(c, d, nframes, d_y, d_cb, d_cr, windows, out_w, out_h, dtype, out_layout,
                                                    scale, bias, flip, filter, 0, d_out, stream);
}

// Every image at its own scale (zj_plan.h: prescale_pick): scale 1 through the crop kernel exactly as before, the others
// through the reduced decode at the reduced window (prescale_window); then the resize over the group's crops, in order.
// orientation (nullptr: none, and nothing below differs from the call without it): the windows are in
// DISPLAYED pixels; each is mapped to its stored window first (orient_window), which is decoded as ever; the crops of the
// frames with o != 1 are then turned into a second region of the buffer, behind the group's crops, and the resize reads
// those.  The scale is picked from the displayed window's sides, the ones the resize sees.
static int crops_resized_impl(zj_ctx* c, const zj_frame_desc* caller_d, size_t nframes, const int16_t* const* d_y,
                              const int16_t* const* d_cb, const int16_t* const* d_cr, const unsigned* windows, ResizeOut ro,
                              int max_prescale_log2, const uint8_t* orientation, void* stream)
{
    if (!resize_filter_valid(ro.filter) || max_prescale_log2 < 0 || max_prescale_log2 > 3) return ZJ_ERR_ARG;
    if (!c || !caller_d || !windows || nframes == 0 || nframes > (size_t)1 << 20 || !d_y || !ro.d_out) return ZJ_ERR_ARG;
    // ZJ_FLAG_GRAY_TO_RGB: the stages in front of the resize run with the frames as GRAYSCALE ones (d), the
    // output has the caller's 3 channels, and every frame passes the expand stage on the way (rz_finish_group)
    const bool gray = gray_to_rgb(caller_d);
    const zj_frame_desc stage_d = resized_stage_desc(caller_d);
    const zj_frame_desc* const d = &stage_d;
    const unsigned* const shown = windows; // the caller's windows: displayed pixels
    std::vector<unsigned> stored_store;
    if (orientation) {
        if (!d->width || !d->height) return ZJ_ERR_ARG;
        stored_store.resize(4 * nframes);
        for (size_t f = 0; f < nframes; f++)
            if (!orient_window(orientation[f], d->width, d->height, shown + 4 * f, stored_store.data() + 4 * f)) return ZJ_ERR_ARG;
        windows = stored_store.data();
    }
    const int ch = resize_channels(caller_d);
    if (!ch || gray_to_rgb_refused(caller_d)) return ZJ_ERR_UNSUPPORTED;
    Plan pl;
    CropPlan cp;
    int rc = make_crop_plan(d, 1, 1, 0, pl, cp);
    if (rc) return rc;
    if ((rc = resize_out_args(ro, ch))) return rc;
    const bool chroma = pl.out != OUT_GRAY;
    if ((rc = check_plane_ptrs(d_y, d_cb, d_cr, chroma, nframes))) return rc;
    for (size_t f = 0; f < nframes; f++) {
        const unsigned* w = windows + 4 * f;
        if (w[2] == 0 || w[3] == 0) return ZJ_ERR_ARG;
        CropPlan cw = cp;
        cw.w = (int)w[2]; cw.h = (int)w[3];
        int s0, s1, k0, k1;
        if ((size_t)w[2] > d->width || (size_t)w[3] > d->height) return ZJ_ERR_ARG;
        if ((rc = crop_window(d, pl, cw, w[0], w[1], s0, s1, k0, k1))) return rc;
    }
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    const bool chw = ro.chw = ch == 3 && caller_d->out_layout == ZJ_LAYOUT_CHW; // (of RGB: make_plan refuses YCbCr planes)
    // per image: its scale and the window the crop stage decodes (scale 1: the window itself)
    std::vector<unsigned> cwin_store;
    std::vector<int> klog;
    if (max_prescale_log2 > 0) { cwin_store.assign(windows, windows + 4 * nframes); klog.assign(nframes, 0); }
    unsigned* const cwin_w = cwin_store.data();
    const unsigned* const cwin = max_prescale_log2 > 0 ? cwin_w : windows;
    ScaledPlan sps[4];
    Plan spl;
    for (int k = 1; k <= max_prescale_log2; k++)
        if ((rc = make_scaled_plan(d, k, spl, sps[k]))) return rc;
    if (max_prescale_log2 > 0)
        for (size_t f = 0; f < nframes; f++) {
            const unsigned* w = windows + 4 * f;
            klog[f] = prescale_pick(shown[4 * f + 2], shown[4 * f + 3], ro.out_w, ro.out_h, max_prescale_log2);
            if (klog[f]) prescale_window(w, klog[f], d->width, d->height, cwin_w + 4 * f);
        }
    // launch groups (zj_rzgroup.h): frames whose crops fit RZ_GROUP_CAP together, the buffer sized for the largest
    std::vector<RzFrame> rzf(nframes);
    for (size_t f = 0; f < nframes; f++) rzf[f] = RzFrame{cwin[4 * f + 2], cwin[4 * f + 3], orientation ? orientation[f] : 1, gray};
    uint8_t* buf = nullptr;
    if ((rc = resize_scratch(c, rz_scratch_need(rzf.data(), nframes, ch, chw, RZ_GROUP_CAP), st, &buf))) return rc;
    std::vector<RzPlace> place(nframes);
    std::vector<uint8_t*> crops(nframes);
    std::vector<const int16_t*> gy, gcb, gcr; // the frames of one scale of a group, gathered
    std::vector<uint8_t*> gout;
    std::vector<unsigned> gwin;
    for (size_t g0 = 0, g1, bytes; g0 < nframes; g0 = g1) {
        g1 = rz_group_next(rzf.data(), nframes, g0, ch, chw, RZ_GROUP_CAP, place.data(), &bytes);
        for (size_t f = g0; f < g1; f++) crops[f] = buf + place[f].crop.off;
        // the crops of the group, each tight at its own size (CropParams.out_pitch 0); the group before it has been read by
        // then (the same stream)
        for (int k = 0; k <= max_prescale_log2; k++) {
            // the frames of scale k: without prescaling the caller's arrays as they are, else gathered
            const int16_t* const* py = d_y + g0; const int16_t* const* pcb = chroma ? d_cb + g0 : nullptr;
            const int16_t* const* pcr = chroma ? d_cr + g0 : nullptr;
            uint8_t* const* pout = crops.data() + g0;
            const unsigned* pwin = windows + 4 * g0;
            size_t ng = g1 - g0;
            if (max_prescale_log2 > 0) {
                gy.clear(); gcb.clear(); gcr.clear(); gout.clear(); gwin.clear();
                for (size_t f = g0; f < g1; f++) {
                    if (klog[f] != k) continue;
                    gy.push_back(d_y[f]); gcb.push_back(chroma ? d_cb[f] : nullptr); gcr.push_back(chroma ? d_cr[f] : nullptr);
                    gout.push_back(crops[f]);
                    gwin.insert(gwin.end(), cwin + 4 * f, cwin + 4 * f + 4);
                }
                py = gy.data(); pcb = chroma ? gcb.data() : nullptr; pcr = chroma ? gcr.data() : nullptr;
                pout = gout.data(); pwin = gwin.data(); ng = gy.size();
            }
            if (!ng) continue;
            if ((rc = k > 0 ? scaled_launches(c, d, pl, sps[k], ng, py, pcb, pcr, pwin, pout, 0, st)
                            : decode_crops_impl(c, d, pl, cp, ng, py, pcb, pcr, pwin, 4, pout, st)))
                return rc;
        }
        if ((rc = rz_finish_group(c, rzf.data(), place.data(), g0, g1, buf, ro, st))) return rc;
    }
    return ZJ_OK;
}

int zj_decode_crops_resized_prescaled_device(zj_ctx* c, const zj_frame_desc* d, size_t nframes, const int16_t* const* d_y,
                                             const int16_t* const* d_cb, const int16_t* const* d_cr, const unsigned* windows,
                                             unsigned out_w, unsigned out_h, int dtype, int out_layout, const float* scale,
                                             const float* bias, const uint8_t* flip, int filter, int max_prescale_log2,
                                             void* d_out, void* stream)
{
    return zj_decode_crops_resized_oriented_device(c, d, nframes, d_y, d_cb, d_cr, windows, out_w, out_h, dtype, out_layout, scale,
                                                   bias, flip, filter, max_prescale_log2, nullptr, d_out, stream);
}

/* ---- EXIF orientation ----------------------------------------------------------- */
int zj_decode_crops_resized_oriented_device(zj_ctx* c, const zj_frame_desc* d, size_t nframes, const int16_t* const* d_y,
                                            const int16_t* const* d_cb, const int16_t* const* d_cr, const unsigned* windows,
                                            unsigned out_w, unsigned out_h, int dtype, int out_layout, const float* scale,
                                            const float* bias, const uint8_t* flip, int filter, int max_prescale_log2,
                                            const uint8_t* orientation, void* d_out, void* stream)
{
    return crops_resized_impl(c, d, nframes, d_y, d_cb, d_cr, windows,
                              resize_out(out_w, out_h, dtype, out_layout, scale, bias, flip, filter, d_out), max_prescale_log2,
                              orientation, stream);
}

/* ---- affine warp ----------------------------------------------------------------- */
namespace {
int warp_tail_args(const uint8_t* fill, int edge, int channels, WarpTail& t)
{
    if (edge != ZJ_WARP_FILL && edge != ZJ_WARP_REPLICATE) return ZJ_ERR_ARG;
    t.edge = edge;
    t.fill = warp_fill(fill, channels);
    return ZJ_OK;
}

// the six integers of n matrices of doubles, 6 each
int warp_matrices(const double* matrices, size_t n, std::vector<int64_t>& q)
{
    if (!matrices) return ZJ_ERR_ARG;
    q.resize(6 * n);
    for (size_t f = 0; f < n; f++)
        if (!warp_fixed(matrices + 6 * f, q.data() + 6 * f)) return ZJ_ERR_ARG;
    return ZJ_OK;
}

// images [0, n) -> images [first, first + n) of the output, launches of up to WARP_BATCH images; wh[2i], wh[2i + 1]: image
// i's size (wh[2i] == 0: no image at all, pack_warp), pitch[i] resolved, q: its six integers
int warp_launches(zj_ctx* c, size_t n, const uint8_t* const* in, const unsigned* wh, const unsigned* pitch, const int64_t* q,
                  const ResizeOut& o, const WarpTail& t, size_t first, hipStream_t st)
{
    const StageTensor tensor = stage_tensor(o);
    WarpParams p{};
    return stage_batches<WARP_BATCH>(n, [&](size_t f0, int m) {
        pack_warp(p, in, wh, pitch, q, t.fill, t.edge, tensor, first, f0, m);
        ZJ_HIP(c, launch_warp(o.ch, p, st));
        return ZJ_OK;
    });
}
} // namespace

int zj_warp_fixed(const double matrix[6], int64_t fixed[6])
{
    if (!matrix || !fixed) return ZJ_ERR_ARG;
    int64_t q[6];
    if (!warp_fixed(matrix, q)) return ZJ_ERR_ARG;
    for (int k = 0; k < 6; k++) fixed[k] = q[k];
    return ZJ_OK;
}

int zj_warp_source_window(const int64_t fixed[6], unsigned frame_w, unsigned frame_h, unsigned out_w, unsigned out_h, int edge,
                          unsigned window[4], int64_t shifted[6])
{
    if (!fixed || !window || !shifted || !warp_ints_valid(fixed)) return ZJ_ERR_ARG;
    if (frame_w == 0 || frame_h == 0 || frame_w > 65535 || frame_h > 65535) return ZJ_ERR_ARG;
    if (out_w == 0 || out_h == 0 || out_w > (unsigned)RESIZE_MAX_OUT || out_h > (unsigned)RESIZE_MAX_OUT) return ZJ_ERR_ARG;
    if (edge != ZJ_WARP_FILL && edge != ZJ_WARP_REPLICATE) return ZJ_ERR_ARG;
    unsigned w[4];
    int64_t s[6];
    warp_source_window(fixed, frame_w, frame_h, out_w, out_h, edge == ZJ_WARP_REPLICATE, w, s);
    for (int k = 0; k < 4; k++) window[k] = w[k];
    for (int k = 0; k < 6; k++) shifted[k] = s[k];
    return ZJ_OK;
}

int zj_warp_device(zj_ctx* c, size_t n, const uint8_t* const* d_in, const unsigned* in_wh, const unsigned* in_pitch, int channels,
                   const double* matrices, unsigned out_w, unsigned out_h, int dtype, int out_layout, const float* scale,
                   const float* bias, const uint8_t* fill, int edge, void* d_out, void* stream)
{
    if (!c || n == 0 || n > (size_t)1 << 20 || !d_in || !in_wh || !d_out) return ZJ_ERR_ARG;
    if (channels != 1 && channels != 3) return ZJ_ERR_ARG;
    ResizeOut ro = resize_out(out_w, out_h, dtype, out_layout, scale, bias, nullptr, ZJ_RESIZE_BILINEAR, d_out);
    int rc = resize_out_args(ro, channels);
    if (rc) return rc;
    if ((uintptr_t)d_out % (uintptr_t)resize_elem_bytes(dtype)) return ZJ_ERR_ARG; // (the kernel's stores are whole elements)
    WarpTail wt;
    if ((rc = warp_tail_args(fill, edge, channels, wt))) return rc;
    std::vector<int64_t> q;
    if ((rc = warp_matrices(matrices, n, q))) return rc;
    std::vector<unsigned> pitch;
    if (!stage_images(n, d_in, in_wh, in_pitch, channels, pitch)) return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return warp_launches(c, n, d_in, in_wh, pitch.data(), q.data(), ro, wt, 0, st);
}

// Each frame's source window (zj_warp_fixed.h: warp_source_window of its matrix, in frame pixels) through the crop stage into
// the context's buffer, in the launch groups of the resized calls (zj_rzgroup.h) and under their reuse events; then the warp
// over the group's crops with the integers relative to the windows.  A frame whose output sees nothing of the frame (fill
// mode) decodes nothing.  ZJ_FLAG_GRAY_TO_RGB as in crops_resized_impl: the crop is one channel, the expand stage makes
// the image the warp reads.
int zj_decode_crops_warped_device(zj_ctx* c, const zj_frame_desc* caller_d, size_t nframes, const int16_t* const* d_y,
                                  const int16_t* const* d_cb, const int16_t* const* d_cr, const double* matrices, unsigned out_w,
                                  unsigned out_h, int dtype, int out_layout, const float* scale, const float* bias,
                                  const uint8_t* fill, int edge, void* d_out, void* stream)
{
    if (!c || !caller_d || !matrices || nframes == 0 || nframes > (size_t)1 << 20 || !d_y || !d_out) return ZJ_ERR_ARG;
    const bool gray = gray_to_rgb(caller_d);
    const zj_frame_desc stage_d = resized_stage_desc(caller_d);
    const zj_frame_desc* const d = &stage_d;
    const int ch = resize_channels(caller_d);
    if (!ch || gray_to_rgb_refused(caller_d)) return ZJ_ERR_UNSUPPORTED;
    Plan pl;
    CropPlan cp;
    int rc = make_crop_plan(d, 1, 1, 0, pl, cp);
    if (rc) return rc;
    ResizeOut ro = resize_out(out_w, out_h, dtype, out_layout, scale, bias, nullptr, ZJ_RESIZE_BILINEAR, d_out);
    if ((rc = resize_out_args(ro, ch))) return rc;
    if ((uintptr_t)d_out % (uintptr_t)resize_elem_bytes(dtype)) return ZJ_ERR_ARG;
    WarpTail wt;
    if ((rc = warp_tail_args(fill, edge, ch, wt))) return rc;
    const bool chroma = pl.out != OUT_GRAY;
    if ((rc = check_plane_ptrs(d_y, d_cb, d_cr, chroma, nframes))) return rc;
    if (caller_d->out_layout != ZJ_LAYOUT_HWC) return ZJ_ERR_UNSUPPORTED; // (the warp reads interleaved images)
    if (d->width == 0 || d->height == 0 || d->width > 65535 || d->height > 65535) return ZJ_ERR_ARG;
    std::vector<int64_t> q, qs(6 * nframes);
    if ((rc = warp_matrices(matrices, nframes, q))) return rc;
    std::vector<unsigned> windows(4 * nframes);
    for (size_t f = 0; f < nframes; f++) {
        unsigned* const w = windows.data() + 4 * f;
        warp_source_window(q.data() + 6 * f, (unsigned)d->width, (unsigned)d->height, out_w, out_h, edge == ZJ_WARP_REPLICATE, w,
                           qs.data() + 6 * f);
        if (w[2] == 0) continue;
        CropPlan cw = cp;
        cw.w = (int)w[2]; cw.h = (int)w[3];
        int s0, s1, k0, k1;
        if ((rc = crop_window(d, pl, cw, w[0], w[1], s0, s1, k0, k1))) return rc;
    }
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    ro.chw = false;
    std::vector<RzFrame> rzf(nframes);
    for (size_t f = 0; f < nframes; f++) rzf[f] = RzFrame{windows[4 * f + 2], windows[4 * f + 3], 1, gray};
    uint8_t* buf = nullptr;
    if ((rc = resize_scratch(c, rz_scratch_need(rzf.data(), nframes, ch, false, RZ_GROUP_CAP) + 16, st, &buf))) return rc;
    std::vector<RzPlace> place(nframes);
    std::vector<const int16_t*> gy, gcb, gcr; // the frames of a group that decode something, gathered
    std::vector<uint8_t*> gout;
    std::vector<unsigned> gwin;
    for (size_t g0 = 0, g1, bytes; g0 < nframes; g0 = g1) {
        g1 = rz_group_next(rzf.data(), nframes, g0, ch, false, RZ_GROUP_CAP, place.data(), &bytes);
        gy.clear(); gcb.clear(); gcr.clear(); gout.clear(); gwin.clear();
        for (size_t f = g0; f < g1; f++) {
            if (windows[4 * f + 2] == 0) continue;
            gy.push_back(d_y[f]); gcb.push_back(chroma ? d_cb[f] : nullptr); gcr.push_back(chroma ? d_cr[f] : nullptr);
            gout.push_back(buf + place[f].crop.off);
            gwin.insert(gwin.end(), windows.begin() + 4 * f, windows.begin() + 4 * f + 4);
        }
        if (!gy.empty() && (rc = decode_crops_impl(c, d, pl, cp, gy.size(), gy.data(), chroma ? gcb.data() : nullptr,
                                                   chroma ? gcr.data() : nullptr, gwin.data(), 4, gout.data(), st)))
            return rc;
        if ((rc = rz_finish_group(c, rzf.data(), place.data(), g0, g1, buf, ro, st, &wt, qs.data()))) return rc;
    }
    return ZJ_OK;
}

/* ---- mixed-geometry resized crops ----------------------------------------------- */
namespace {
// the pinned staging and the device table, at least `bytes` each, the staging free for the host to write: the last copy out
// of it has finished; growing them waits for the last launch that read the device table as well
int mixed_tables(zj_ctx* c, size_t bytes)
{
    if (!c->mx_up) {
        ZJ_HIP(c, hipEventCreateWithFlags(&c->mx_up, hipEventDisableTiming));
        ZJ_HIP(c, hipEventCreateWithFlags(&c->mx_done, hipEventDisableTiming));
    }
    if (c->mx_used) ZJ_HIP(c, hipEventSynchronize(c->mx_up));
    if (bytes <= c->mx_cap) return ZJ_OK;
    if (c->mx_used) ZJ_HIP(c, hipEventSynchronize(c->mx_done));
    if (c->mx_dev) { ZJ_HIP(c, hipFree(c->mx_dev)); c->mx_dev = nullptr; }
    if (c->mx_host) { ZJ_HIP(c, hipHostFree(c->mx_host)); c->mx_host = nullptr; }
    c->mx_cap = 0;
    const size_t cap = bytes + bytes / 4 + 4096;
    ZJ_HIP(c, hipHostMalloc(&c->mx_host, cap, hipHostMallocDefault));
    ZJ_HIP(c, hipMalloc(&c->mx_dev, cap));
    c->mx_cap = cap;
    return ZJ_OK;
}

// The records the caller has written into the pinned staging (after mixed_tables) -> the device table in one copy of `bytes`,
// then launches(table), the launches that read it, all on st.  st waits for the last launch that read the table before the
// copy; mx_up says when the staging may be written again, mx_done when the table may.
extern "C++" template <class Launches>
int mixed_submit(zj_ctx* c, size_t bytes, hipStream_t st, Launches launches)
{
    if (c->mx_used) ZJ_HIP(c, hipStreamWaitEvent(st, c->mx_done, 0));
    ZJ_HIP(c, hipMemcpyAsync(c->mx_dev, c->mx_host, bytes, hipMemcpyHostToDevice, st));
    ZJ_HIP(c, hipEventRecord(c->mx_up, st));
    c->mx_used = true;
    const hipError_t e = launches((const uint8_t*)c->mx_dev);
    // (recorded whether or not a launch failed: the table may be in use by the ones that went out)
    (void)hipEventRecord(c->mx_done, st);
    ZJ_HIP(c, e);
    return ZJ_OK;
}

// The plane rows one frame's crop stage reads: rows [r0, r1) of yrow (luma) / crow (each chroma plane) i16 elements
struct PlaneRows { size_t r0, r1, yrow, crow; bool chroma; };

// The rows of n frames' planes in HOST memory, packed: host planes -> pinned staging -> ONE copy into the context's arena on
// st (mixed_tables first: it waits for the last copy out of the staging).  py / pcb / pcr[f]: the address the plane's row 0
// would have -- every address a lane forms lies in a strip or MCU row of its own window (zj_device.h: locate, halo_locate;
// zj_scaled.h: scaled_block_loc), all of them uploaded; nullptr for the chroma planes of a frame without.
int upload_host_planes(zj_ctx* c, size_t n, const PlaneRows* rows, const int16_t* const* y, const int16_t* const* cb,
                       const int16_t* const* cr, const int16_t** py, const int16_t** pcb, const int16_t** pcr, hipStream_t st)
{
    size_t total = 0;
    for (size_t f = 0; f < n; f++) total += (rows[f].r1 - rows[f].r0) * (rows[f].yrow + (rows[f].chroma ? 2 * rows[f].crow : 0)) * 2;
    if (total > c->mx_arena_cap) {
        ZJ_HIP(c, hipStreamSynchronize(st));
        if (c->mx_arena) { ZJ_HIP(c, hipFree(c->mx_arena)); c->mx_arena = nullptr; }
        if (c->mx_stage) { ZJ_HIP(c, hipHostFree(c->mx_stage)); c->mx_stage = nullptr; }
        c->mx_arena_cap = 0;
        const size_t cap = total + total / 4 + 4096;
        ZJ_HIP(c, hipHostMalloc(&c->mx_stage, cap, hipHostMallocDefault));
        ZJ_HIP(c, hipMalloc(&c->mx_arena, cap));
        c->mx_arena_cap = cap;
    }
    size_t at = 0; // i16 elements into staging and arena alike
    for (size_t f = 0; f < n; f++) {
        const PlaneRows& r = rows[f];
        const int16_t* const src[3] = {y[f], r.chroma ? cb[f] : nullptr, r.chroma ? cr[f] : nullptr};
        const int16_t** const dst[3] = {&py[f], &pcb[f], &pcr[f]};
        for (int k = 0; k < 3; k++) {
            const size_t row = k ? r.crow : r.yrow, len = (r.r1 - r.r0) * row;
            *dst[k] = nullptr;
            if (!src[k]) continue;
            *dst[k] = (const int16_t*)((uintptr_t)c->mx_arena + 2 * at - 2 * r.r0 * row);
            if (len) memcpy((int16_t*)c->mx_stage + at, src[k] + r.r0 * row, len * 2);
            at += len;
        }
    }
    if (at) ZJ_HIP(c, hipMemcpyAsync(c->mx_arena, c->mx_stage, at * 2, hipMemcpyHostToDevice, st));
    return ZJ_OK;
}

// The tail of the zjint_*_mixed_host calls: the context stream synchronised (the caller's planes are free again); a
// synchronise error is reported only when the call itself succeeded
int mixed_host_end(zj_ctx* c, int rc)
{
    if (c && c->stream) {
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (rc == ZJ_OK && e != hipSuccess) { c->last_error = std::string("hipStreamSynchronize: ") + hipGetErrorString(e); return ZJ_ERR_HIP; }
    }
    return rc;
}

// The call behind both mixed entry points.  host_planes: y / cb / cr are the CPU walker's planes in host memory; the rows
// each frame's window needs go into the context's arena, a group's uploads all queued before its launches (the planes must
// stay as they are until the stream has run: the caller synchronises).  Otherwise they are device planes.
int crops_resized_mixed_impl(zj_ctx* c, const zj_frame_desc* descs, size_t nframes, const int16_t* const* d_y,
                             const int16_t* const* d_cb, const int16_t* const* d_cr, bool host_planes, const unsigned* windows,
                             ResizeOut ro, int max_prescale_log2, const uint8_t* orientation, void* stream,
                             const WarpTail* warp = nullptr, const int64_t* warp_q = nullptr, const int32_t* color_q = nullptr,
                             const int32_t* tone = nullptr)
{
    if (!resize_filter_valid(ro.filter) || max_prescale_log2 < 0 || max_prescale_log2 > 3) return ZJ_ERR_ARG;
    if (!c || !descs || !windows || nframes == 0 || nframes > (size_t)1 << 20 || !d_y || !ro.d_out) return ZJ_ERR_ARG;
    // every frame's checks, in the one-geometry call's order, before anything is launched
    std::vector<MixedFrame> fr(nframes);
    const int ch = resize_channels(&descs[0]);
    const auto planes = [&](size_t f, bool chroma) {
        if (chroma && (!d_cb || !d_cr)) return (int)ZJ_ERR_ARG;
        return check_plane_ptrs(d_y + f, chroma ? d_cb + f : nullptr, chroma ? d_cr + f : nullptr, chroma, 1);
    };
    int rc = mixed_check_frames(descs, nframes, windows, orientation, ch ? resize_out_args(ro, ch) : 0, ro.out_w, ro.out_h,
                                max_prescale_log2, planes, fr.data());
    if (rc) return rc;
    if (color_q && ch != 3) return ZJ_ERR_UNSUPPORTED; // (a colour matrix maps three channels)
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    const bool chw = ro.chw = ch == 3 && descs[0].out_layout == ZJ_LAYOUT_CHW; // (of RGB: make_plan refuses YCbCr planes)
    // launch groups (zj_rzgroup.h), as the one-geometry call's
    std::vector<RzFrame> rzf(nframes);
    for (size_t f = 0; f < nframes; f++) rzf[f] = RzFrame{fr[f].cwin[2], fr[f].cwin[3], fr[f].o, fr[f].gray};
    uint8_t* buf = nullptr;
    if ((rc = resize_scratch(c, rz_scratch_need(rzf.data(), nframes, ch, chw, RZ_GROUP_CAP), st, &buf))) return rc;
    std::vector<RzPlace> place(nframes);
    std::vector<uint8_t*> crops(nframes);
    std::vector<const int16_t*> py(nframes), pcb(nframes), pcr(nframes);
    MixedTables tabs;
    std::vector<PlaneRows> rows;
    for (size_t g0 = 0, g1, bytes; g0 < nframes; g0 = g1) {
        g1 = rz_group_next(rzf.data(), nframes, g0, ch, chw, RZ_GROUP_CAP, place.data(), &bytes);
        for (size_t f = g0; f < g1; f++) crops[f] = buf + place[f].crop.off;
        const size_t ng = g1 - g0;
        // (first: it waits until the copies out of the pinned staging, the planes' and the tables', have finished)
        if ((rc = mixed_tables(c, mixed_table_bytes(fr.data() + g0, ng)))) return rc;
        if (host_planes) {
            // the rows each window of the group needs (mixed_plane_rows)
            rows.resize(ng);
            for (size_t f = g0; f < g1; f++) {
                PlaneRows& r = rows[f - g0];
                mixed_plane_rows(&descs[f], fr[f], r.r0, r.r1, r.yrow, r.crow);
                r.chroma = fr[f].pl.out != OUT_GRAY;
            }
            // (a frame without chroma: its d_cb / d_cr entries are not read, and the arrays may be null)
            if ((rc = upload_host_planes(c, ng, rows.data(), d_y + g0, d_cb ? d_cb + g0 : nullptr, d_cr ? d_cr + g0 : nullptr,
                                         py.data() + g0, pcb.data() + g0, pcr.data() + g0, st)))
                return rc;
        } else {
            for (size_t f = g0; f < g1; f++) {
                const bool chroma = fr[f].pl.out != OUT_GRAY;
                py[f] = d_y[f]; pcb[f] = chroma ? d_cb[f] : nullptr; pcr[f] = chroma ? d_cr[f] : nullptr;
            }
        }
        // the group's records: staging -> device table, then one launch per run
        mixed_fill_tables(descs + g0, fr.data() + g0, ng, py.data() + g0, pcb.data() + g0, pcr.data() + g0, crops.data() + g0,
                          (uint8_t*)c->mx_host, tabs);
        rc = mixed_submit(c, tabs.bytes, st, [&](const uint8_t* tab) {
            hipError_t e = hipSuccess;
            if (tabs.zero.n) e = launch_crop_zero_mixed((const MixedZero*)(tab + tabs.zero.off), tabs.zero.n, tabs.zero.gx, tabs.zero.gy, st);
            for (size_t i = 0; e == hipSuccess && i < tabs.crop.size(); i++) {
                const MixedLaunch& l = tabs.crop[i];
                e = launch_crop_mixed(l.hs, l.vs, l.out, (const CropParams*)(tab + l.off), l.n, l.gx, l.gy, st);
            }
            for (size_t i = 0; e == hipSuccess && i < tabs.scaled.size(); i++) {
                const MixedLaunch& l = tabs.scaled[i];
                e = launch_scaled_mixed(l.hs, l.vs, l.out, l.sl, (const ScaledParams*)(tab + l.off), l.n, l.gx, l.gy, st);
            }
            return e;
        });
        if (rc) return rc;
        if ((rc = rz_finish_group(c, rzf.data(), place.data(), g0, g1, buf, ro, st, warp, warp_q, color_q, tone))) return rc;
    }
    return ZJ_OK;
}
} // namespace

int zj_decode_crops_resized_mixed_device(zj_ctx* c, const zj_frame_desc* descs, size_t nframes, const int16_t* const* d_y,
                                         const int16_t* const* d_cb, const int16_t* const* d_cr, const unsigned* windows,
                                         unsigned out_w, unsigned out_h, int dtype, int out_layout, const float* scale,
                                         const float* bias, const uint8_t* flip, int filter, int max_prescale_log2,
                                         const uint8_t* orientation, void* d_out, void* stream)
{
    return crops_resized_mixed_impl(c, descs, nframes, d_y, d_cb, d_cr, false, windows,
                                    resize_out(out_w, out_h, dtype, out_layout, scale, bias, flip, filter, d_out),
                                    max_prescale_log2, orientation, stream);
}

// Library-internal (zj_jpeg.cpp: zj_decoder_finish_pixels_resized_crop_batch_device): the same over the CPU walker's planes
// in host memory, on the context stream, synchronised (the planes are free again when it returns)
int zjint_crops_resized_mixed_host(zj_ctx* c, const zj_frame_desc* descs, size_t nframes, const int16_t* const* y,
                                   const int16_t* const* cb, const int16_t* const* cr, const unsigned* windows, unsigned out_w,
                                   unsigned out_h, int dtype, int out_layout, const float* scale, const float* bias,
                                   const uint8_t* flip, int filter, int max_prescale_log2, const uint8_t* orientation, void* d_out)
{
    const int rc = crops_resized_mixed_impl(c, descs, nframes, y, cb, cr, true, windows,
                                            resize_out(out_w, out_h, dtype, out_layout, scale, bias, flip, filter, d_out),
                                            max_prescale_log2, orientation, nullptr);
    return mixed_host_end(c, rc);
}

/* ---- colour matrices in the resized-crop calls ------------------------------------ */
// color (nullptr: zj_decode_crops_resized_mixed_device itself): 12 doubles per frame, all checked before anything is launched
int zj_decode_crops_resized_mixed_colored_device(zj_ctx* c, const zj_frame_desc* descs, size_t nframes, const int16_t* const* d_y,
                                                 const int16_t* const* d_cb, const int16_t* const* d_cr, const unsigned* windows,
                                                 unsigned out_w, unsigned out_h, int dtype, int out_layout, const float* scale,
                                                 const float* bias, const uint8_t* flip, int filter, int max_prescale_log2,
                                                 const uint8_t* orientation, const double* color, void* d_out, void* stream)
{
    std::vector<int32_t> q;
    if (color) {
        if (nframes == 0 || nframes > (size_t)1 << 20) return ZJ_ERR_ARG;
        if (const int rc = color_matrices(color, nframes, q)) return rc;
    }
    return crops_resized_mixed_impl(c, descs, nframes, d_y, d_cb, d_cr, false, windows,
                                    resize_out(out_w, out_h, dtype, out_layout, scale, bias, flip, filter, d_out),
                                    max_prescale_log2, orientation, stream, nullptr, nullptr, color ? q.data() : nullptr);
}

// Library-internal (zj_jpeg.cpp: zj_decoder_finish_pixels_resized_crop_batch_colored_device): zjint_crops_resized_mixed_host
// with file f's image under the integers color_q[12f .. 12f + 11] (nullptr: none) in front of the resize
int zjint_crops_resized_mixed_colored_host(zj_ctx* c, const zj_frame_desc* descs, size_t nframes, const int16_t* const* y,
                                           const int16_t* const* cb, const int16_t* const* cr, const unsigned* windows,
                                           unsigned out_w, unsigned out_h, int dtype, int out_layout, const float* scale,
                                           const float* bias, const uint8_t* flip, int filter, int max_prescale_log2,
                                           const uint8_t* orientation, const int32_t* color_q, void* d_out)
{
    const int rc = crops_resized_mixed_impl(c, descs, nframes, y, cb, cr, true, windows,
                                            resize_out(out_w, out_h, dtype, out_layout, scale, bias, flip, filter, d_out),
                                            max_prescale_log2, orientation, nullptr, nullptr, nullptr, color_q);
    return mixed_host_end(c, rc);
}

/* ---- tone curves in the resized-crop calls ---------------------------------------- */
// tone (nullptr: zj_decode_crops_resized_mixed_colored_device itself): an op of two int32 per frame, all checked before
// anything is launched
int zj_decode_crops_resized_mixed_toned_device(zj_ctx* c, const zj_frame_desc* descs, size_t nframes, const int16_t* const* d_y,
                                               const int16_t* const* d_cb, const int16_t* const* d_cr, const unsigned* windows,
                                               unsigned out_w, unsigned out_h, int dtype, int out_layout, const float* scale,
                                               const float* bias, const uint8_t* flip, int filter, int max_prescale_log2,
                                               const uint8_t* orientation, const double* color, const int32_t* tone, void* d_out,
                                               void* stream)
{
    std::vector<int32_t> q;
    if (color || tone) {
        if (nframes == 0 || nframes > (size_t)1 << 20) return ZJ_ERR_ARG;
        if (color)
            if (const int rc = color_matrices(color, nframes, q)) return rc;
        if (tone && !tone_ops_valid(tone, nframes)) return ZJ_ERR_ARG;
    }
    return crops_resized_mixed_impl(c, descs, nframes, d_y, d_cb, d_cr, false, windows,
                                    resize_out(out_w, out_h, dtype, out_layout, scale, bias, flip, filter, d_out),
                                    max_prescale_log2, orientation, stream, nullptr, nullptr, color ? q.data() : nullptr, tone);
}

// Library-internal (zj_jpeg.cpp: zj_decoder_finish_pixels_resized_crop_batch_toned_device): zjint_crops_resized_mixed_colored_host
// with file f's image under the op tone[2f], tone[2f + 1] (nullptr: none; every op valid) behind the colour stage
int zjint_crops_resized_mixed_toned_host(zj_ctx* c, const zj_frame_desc* descs, size_t nframes, const int16_t* const* y,
                                         const int16_t* const* cb, const int16_t* const* cr, const unsigned* windows,
                                         unsigned out_w, unsigned out_h, int dtype, int out_layout, const float* scale,
                                         const float* bias, const uint8_t* flip, int filter, int max_prescale_log2,
                                         const uint8_t* orientation, const int32_t* color_q, const int32_t* tone, void* d_out)
{
    if (tone && (!nframes || !tone_ops_valid(tone, nframes))) return ZJ_ERR_ARG;
    const int rc = crops_resized_mixed_impl(c, descs, nframes, y, cb, cr, true, windows,
                                            resize_out(out_w, out_h, dtype, out_layout, scale, bias, flip, filter, d_out),
                                            max_prescale_log2, orientation, nullptr, nullptr, nullptr, color_q, tone);
    return mixed_host_end(c, rc);
}

// Library-internal (zj_jpeg.cpp: zj_decoder_finish_pixels_warped_batch_device): the mixed-geometry crops of several files'
// host planes -- windows: each file's source window, not empty, in displayed pixels with `orientation` -- and, in place of the
// resize, the warp of each group's images under q[6f .. 6f + 5], the integers relative to the windows; on the
// context stream, synchronised
int zjint_crops_warped_mixed_host(zj_ctx* c, const zj_frame_desc* descs, size_t nframes, const int16_t* const* y,
                                  const int16_t* const* cb, const int16_t* const* cr, const unsigned* windows, const int64_t* q,
                                  unsigned out_w, unsigned out_h, int dtype, int out_layout, const float* scale, const float* bias,
                                  const uint8_t* fill, int edge, const uint8_t* orientation, void* d_out)
{
    if (!c || !descs || !nframes || !q || !d_out) return ZJ_ERR_ARG;
    if (descs[0].out_layout != ZJ_LAYOUT_HWC) return ZJ_ERR_UNSUPPORTED; // (the warp reads interleaved images)
    if ((uintptr_t)d_out % (uintptr_t)(resize_elem_bytes(dtype) ? resize_elem_bytes(dtype) : 1)) return ZJ_ERR_ARG;
    WarpTail wt;
    int rc = warp_tail_args(fill, edge, resize_channels(&descs[0]) == 1 ? 1 : 3, wt);
    if (rc) return rc;
    rc = crops_resized_mixed_impl(c, descs, nframes, y, cb, cr, true, windows,
                                  resize_out(out_w, out_h, dtype, out_layout, scale, bias, nullptr, ZJ_RESIZE_BILINEAR, d_out), 0,
                                  orientation, nullptr, &wt, q);
    return mixed_host_end(c, rc);
}

/* ---- crop windows into a normalised tensor, no resize ------------------------------ */
size_t zj_crop_tensor_out_len(const zj_frame_desc* d, unsigned w, unsigned h, int dtype)
{
    Plan pl;
    CropPlan cp;
    if (!d || !crop_tensor_desc_ok(d) || make_crop_plan(d, w, h, 0, pl, cp) != ZJ_OK) return 0;
    return crop_tensor_len(resize_channels(d), w, h, dtype);
}

namespace {
// The checks of a tensor call in the order that decides a bad call's status: the pointers, the descriptor's kind, the
// output's arguments, the crop plan and the windows (zj_decode_crops_device's).  s, b: the kernel's factors.
int crop_tensor_args(zj_ctx* c, const zj_frame_desc* d, size_t nframes, const unsigned* origins, unsigned w, unsigned h, int dtype,
                     int out_layout, const float* scale, const float* bias, const void* d_out, Plan& pl, CropPlan& cp, float s[3],
                     float b[3], size_t& img_bytes)
{
    if (!c || !d || !origins || !d_out || nframes == 0 || nframes > (size_t)1 << 20) return ZJ_ERR_ARG;
    if (!crop_tensor_desc_ok(d)) return ZJ_ERR_UNSUPPORTED;
    const int ch = resize_channels(d);
    if (!resize_elem_bytes(dtype) || (out_layout != ZJ_TENSOR_NCHW && out_layout != ZJ_TENSOR_NHWC)) return ZJ_ERR_ARG;
    if ((uintptr_t)d_out % (uintptr_t)resize_elem_bytes(dtype)) return ZJ_ERR_ARG;
    if (!kernel_factors(scale, bias, ch, s, b)) return ZJ_ERR_ARG;
    int rc = make_crop_plan(d, w, h, 0, pl, cp);
    if (rc) return rc;
    if (!(img_bytes = crop_tensor_len(ch, w, h, dtype))) return ZJ_ERR_ARG;
    for (size_t f = 0; f < nframes; f++) {
        int s0, s1, k0, k1;
        if ((rc = crop_window(d, pl, cp, origins[2 * f], origins[2 * f + 1], s0, s1, k0, k1))) return rc;
    }
    return ZJ_OK;
}

// One launch of the tensor kernels: the n records from record `first` of the table, each of up to 2^shift frames of the
// kernel (hs, vs, out); gx x gy: the widest tile-column / strip ranges over them
struct CropTensorRun { int hs, vs, out, shift, gx, gy; size_t first; int n; };

// The records into the context's pinned staging, one copy into its device table, then the zero launch and one launch per
// run, all on st.  The staging and the table are the mixed-geometry calls' (mixed_tables): the host waits for the last
// copy out of the staging before it writes it, st waits for the last launch that read the table before the copy.
int crop_tensor_submit(zj_ctx* c, const std::vector<CropTensorParams>& recs, const std::vector<CropTensorZero>& zeros,
                       const std::vector<CropTensorRun>& runs, hipStream_t st)
{
    const size_t rb = recs.size() * sizeof(CropTensorParams), zb = zeros.size() * sizeof(CropTensorZero);
    int rc = mixed_tables(c, rb + zb);
    if (rc) return rc;
    memcpy(c->mx_host, recs.data(), rb);
    if (zb) memcpy((uint8_t*)c->mx_host + rb, zeros.data(), zb);
    return mixed_submit(c, rb + zb, st, [&](const uint8_t* tab) {
        hipError_t e = hipSuccess;
        if (!zeros.empty()) {
            int rows = 0, frames = 0;
            for (const CropTensorZero& z : zeros) {
                if (z.h - z.rmin > rows) rows = z.h - z.rmin;
                if (z.nframes > frames) frames = z.nframes;
            }
            e = launch_crop_tensor_zero((const CropTensorZero*)(tab + rb), (int)zeros.size(), rows, frames, st);
        }
        for (size_t i = 0; e == hipSuccess && i < runs.size(); i++) {
            const CropTensorRun& r = runs[i];
            e = launch_crop_tensor(r.hs, r.vs, r.out, (const CropTensorParams*)tab + r.first, r.n, r.shift, r.gx, r.gy, st);
        }
        return e;
    });
}

// frames [0, nframes) of ONE geometry, checked: one record per SCATTER_MAX frames, all of them one launch, with the
// converted zero for the windows' rows at or below rows_covered, if any has such rows
int crop_tensor_launches(zj_ctx* c, const zj_frame_desc* d, const Plan& pl, const CropPlan& cp, size_t nframes,
                         const int16_t* const* y, const int16_t* const* cb, const int16_t* const* cr, const unsigned* origins,
                         int dtype, int out_layout, const float* s, const float* b, const uint8_t* flip, uint8_t* d_out,
                         size_t img_bytes, hipStream_t st)
{
    const size_t nrec = (nframes + SCATTER_MAX - 1) / SCATTER_MAX;
    std::vector<CropTensorParams> recs(nrec);
    std::vector<CropTensorZero> zeros;
    CropTensorRun run{pl.hs, pl.vs, pl.out, CROP_TENSOR_SHIFT, 0, 0, 0, (int)nrec};
    for (size_t r = 0; r < nrec; r++) {
        const size_t f0 = r * SCATTER_MAX;
        const int n = (int)(nframes - f0 < (size_t)SCATTER_MAX ? nframes - f0 : (size_t)SCATTER_MAX);
        CropTensorZero z;
        if (crop_tensor_fill(d, pl, cp, y, cb, cr, d_out, img_bytes, origins, dtype, out_layout == ZJ_TENSOR_NHWC, s, b, flip, f0, n,
                             recs[r], z))
            zeros.push_back(z);
        if (recs[r].cp.ncols > run.gx) run.gx = recs[r].cp.ncols;
        if (recs[r].cp.nstrips > run.gy) run.gy = recs[r].cp.nstrips;
    }
    return crop_tensor_submit(c, recs, zeros, std::vector<CropTensorRun>(1, run), st);
}

// The call behind both mixed entry points: frames that each bring their own descriptor, one window size, one tensor.
// host_planes: y / cb / cr are the CPU walker's planes in host memory; the strips each window needs go into the context's
// arena in one copy (crops_resized_mixed_impl's way; the planes must stay as they are until the stream has run: the caller
// synchronises).  Every frame is checked before anything is launched; the status is the single-frame call's for the first
// failing frame.
int crops_tensor_mixed_impl(zj_ctx* c, const zj_frame_desc* descs, size_t nframes, const int16_t* const* y,
                            const int16_t* const* cb, const int16_t* const* cr, bool host_planes, const unsigned* origins,
                            unsigned w, unsigned h, int dtype, int out_layout, const float* scale, const float* bias,
                            const uint8_t* flip, void* d_out, void* stream)
{
    if (!c || !descs || !origins || !d_out || !y || nframes == 0 || nframes > (size_t)1 << 20) return ZJ_ERR_ARG;
    if (!mixed_descs_agree(descs, nframes)) return ZJ_ERR_ARG;
    std::vector<Plan> pls(nframes);
    std::vector<CropPlan> cps(nframes);
    float s[3], b[3];
    size_t img = 0;
    for (size_t f = 0; f < nframes; f++) {
        int rc = crop_tensor_args(c, &descs[f], 1, origins + 2 * f, w, h, dtype, out_layout, scale, bias, d_out, pls[f], cps[f], s, b, img);
        if (rc) return rc;
        const bool chroma = pls[f].out != OUT_GRAY;
        if (chroma && (!cb || !cr)) return ZJ_ERR_ARG;
        if (host_planes) { if (!y[f] || (chroma && (!cb[f] || !cr[f]))) return ZJ_ERR_ARG; }
        else if ((rc = check_plane_ptrs(y + f, chroma ? cb + f : nullptr, chroma ? cr + f : nullptr, chroma, 1))) return rc;
    }
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    // (first: it waits until the copies out of the pinned stagings, the planes' and the tables', have finished)
    int rc = mixed_tables(c, nframes * (sizeof(CropTensorParams) + sizeof(CropTensorZero)));
    if (rc) return rc;
    std::vector<const int16_t*> py(nframes), pcb(nframes), pcr(nframes);
    if (host_planes) {
        // the strips each window needs
        std::vector<PlaneRows> rows(nframes);
        for (size_t f = 0; f < nframes; f++) {
            int s0, s1, k0, k1;
            crop_window(&descs[f], pls[f], cps[f], origins[2 * f], origins[2 * f + 1], s0, s1, k0, k1);
            rows[f].r0 = (size_t)s0; rows[f].r1 = (size_t)s1;
            plan_strip_elems(pls[f], rows[f].yrow, rows[f].crow);
            rows[f].chroma = pls[f].out != OUT_GRAY;
        }
        if ((rc = upload_host_planes(c, nframes, rows.data(), y, cb, cr, py.data(), pcb.data(), pcr.data(), st))) return rc;
    } else {
        for (size_t f = 0; f < nframes; f++) {
            const bool chroma = pls[f].out != OUT_GRAY;
            py[f] = y[f]; pcb[f] = chroma ? cb[f] : nullptr; pcr[f] = chroma ? cr[f] : nullptr;
        }
    }
    // one record per frame, the frames of one kernel in one run
    std::vector<CropTensorParams> recs(nframes);
    std::vector<CropTensorZero> zeros;
    std::vector<CropTensorRun> runs;
    size_t at = 0;
    for (int mode = 0; mode < 4; mode++)
        for (int gray = 0; gray < 2; gray++) {
            const int hs = 1 + (mode & 1), vs = 1 + (mode >> 1);
            CropTensorRun run{hs, vs, 0, 0, 0, 0, at, 0};
            for (size_t f = 0; f < nframes; f++) {
                const Plan& pl = pls[f];
                if (pl.hs != hs || pl.vs != vs || (pl.out == OUT_GRAY) != (gray != 0)) continue;
                CropTensorZero z;
                if (crop_tensor_fill(&descs[f], pl, cps[f], py.data(), pcb.data(), pcr.data(), (uint8_t*)d_out, img, origins, dtype,
                                     out_layout == ZJ_TENSOR_NHWC, s, b, flip, f, 1, recs[at], z))
                    zeros.push_back(z);
                run.out = pl.out;
                if (recs[at].cp.ncols > run.gx) run.gx = recs[at].cp.ncols;
                if (recs[at].cp.nstrips > run.gy) run.gy = recs[at].cp.nstrips;
                run.n++; at++;
            }
            if (run.n) runs.push_back(run);
        }
    return crop_tensor_submit(c, recs, zeros, runs, st);
}
} // namespace

int zj_decode_crops_tensor_mixed_device(zj_ctx* c, const zj_frame_desc* descs, size_t nframes, const int16_t* const* d_y,
                                        const int16_t* const* d_cb, const int16_t* const* d_cr, const unsigned* origins,
                                        unsigned crop_w, unsigned crop_h, int dtype, int out_layout, const float* scale,
                                        const float* bias, const uint8_t* flip, void* d_out, void* stream)
{
    return crops_tensor_mixed_impl(c, descs, nframes, d_y, d_cb, d_cr, false, origins, crop_w, crop_h, dtype, out_layout, scale, bias,
                                   flip, d_out, stream);
}

// Library-internal (zj_jpeg.cpp: zj_decoder_finish_pixels_crop_tensor_batch_device): the same over the CPU walker's planes in
// host memory, on the context stream, synchronised (the planes are free again when it returns)
int zjint_crops_tensor_mixed_host(zj_ctx* c, const zj_frame_desc* descs, size_t nframes, const int16_t* const* y,
                                  const int16_t* const* cb, const int16_t* const* cr, const unsigned* origins, unsigned w, unsigned h,
                                  int dtype, int out_layout, const float* scale, const float* bias, const uint8_t* flip, void* d_out)
{
    const int rc = crops_tensor_mixed_impl(c, descs, nframes, y, cb, cr, true, origins, w, h, dtype, out_layout, scale, bias, flip,
                                           d_out, nullptr);
    return mixed_host_end(c, rc);
}

int zj_decode_crops_tensor_device(zj_ctx* c, const zj_frame_desc* d, size_t nframes, const int16_t* const* d_y,
                                  const int16_t* const* d_cb, const int16_t* const* d_cr, const unsigned* origins,
                                  unsigned crop_w, unsigned crop_h, int dtype, int out_layout, const float* scale,
                                  const float* bias, const uint8_t* flip, void* d_out, void* stream)
{
    Plan pl;
    CropPlan cp;
    float s[3], b[3];
    size_t img_bytes = 0;
    int rc = crop_tensor_args(c, d, nframes, origins, crop_w, crop_h, dtype, out_layout, scale, bias, d_out, pl, cp, s, b, img_bytes);
    if (rc) return rc;
    if ((rc = check_plane_ptrs(d_y, d_cb, d_cr, pl.out != OUT_GRAY, nframes))) return rc;
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return crop_tensor_launches(c, d, pl, cp, nframes, d_y, d_cb, d_cr, origins, dtype, out_layout, s, b, flip, (uint8_t*)d_out,
                                img_bytes, st);
}

// Library-internal (zj_jpeg.cpp: zj_decoder_finish_pixels_crop_tensor_device): one frame's window on the context stream,
// synchronised, from planes in host memory (only the strips the window needs are uploaded, as zjint_crop_frame) or in HBM
int zjint_crop_tensor_frame(zj_ctx* c, const zj_frame_desc* d, const int16_t* y, const int16_t* cb, const int16_t* cr,
                            int planes_on_device, unsigned x, unsigned yy, unsigned w, unsigned h, int dtype, int out_layout,
                            const float* scale, const float* bias, int flip, void* d_out)
{
    Plan pl;
    CropPlan cp;
    float s[3], b[3];
    size_t img_bytes = 0;
    const unsigned origin[2] = {x, yy};
    int rc = crop_tensor_args(c, d, 1, origin, w, h, dtype, out_layout, scale, bias, d_out, pl, cp, s, b, img_bytes);
    if (rc) return rc;
    const bool chroma = pl.out != OUT_GRAY;
    if (!y || (chroma && (!cb || !cr))) return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    const int16_t* p[3] = {y, cb, cr};
    if (!planes_on_device) {
        int s0, s1, k0, k1;
        crop_window(d, pl, cp, x, yy, s0, s1, k0, k1);
        size_t yrow, crow;
        plan_strip_elems(pl, yrow, crow);
        if ((rc = upload_plane_rows(c, pl, chroma, y, cb, cr, (size_t)s0, (size_t)s1, yrow, crow, p))) return rc;
    }
    const uint8_t fl = flip ? 1 : 0;
    if ((rc = crop_tensor_launches(c, d, pl, cp, 1, &p[0], &p[1], &p[2], origin, dtype, out_layout, s, b, &fl, (uint8_t*)d_out,
                                   img_bytes, c->stream)))
        return rc;
    ZJ_HIP(c, hipStreamSynchronize(c->stream));
    return ZJ_OK;
}

int zj_oriented_size(int orientation, unsigned w, unsigned h, unsigned* ow, unsigned* oh)
{
    unsigned a, b;
    if (!orient_size(orientation, w, h, &a, &b)) return ZJ_ERR_ARG;
    if (ow) *ow = a;
    if (oh) *oh = b;
    return ZJ_OK;
}

int zj_orient_window(int orientation, unsigned frame_w, unsigned frame_h, const unsigned window[4], unsigned stored[4])
{
    if (!window || !stored) return ZJ_ERR_ARG;
    unsigned s[4];
    if (!orient_window(orientation, frame_w, frame_h, window, s)) return ZJ_ERR_ARG;
    for (int k = 0; k < 4; k++) stored[k] = s[k];
    return ZJ_OK;
}

int zj_orient_device(zj_ctx* c, size_t n, const uint8_t* const* d_in, const unsigned* in_wh, const unsigned* in_pitch,
                     int channels, int in_layout, const uint8_t* orientation, uint8_t* const* d_out, const unsigned* out_pitch,
                     void* stream)
{
    if (!c || n == 0 || n > (size_t)1 << 20 || !d_in || !in_wh || !d_out) return ZJ_ERR_ARG;
    if (channels != 1 && channels != 3) return ZJ_ERR_ARG;
    if (in_layout != ZJ_LAYOUT_HWC && in_layout != ZJ_LAYOUT_CHW) return ZJ_ERR_ARG;
    const bool chw = in_layout == ZJ_LAYOUT_CHW && channels == 3;
    const int bpp = chw ? 1 : channels;
    std::vector<unsigned> ip, op;
    std::vector<uint8_t> o(n, 1);
    if (!stage_images(n, d_in, in_wh, in_pitch, bpp, ip)) return ZJ_ERR_ARG;
    for (size_t f = 0; f < n; f++) {
        if (orientation) o[f] = orientation[f];
        if (!orient_valid(o[f])) return ZJ_ERR_ARG;
    }
    const auto shown_row = [&](size_t f) { // (the output's rows are the DISPLAYED width)
        unsigned dw = 0, dh = 0;
        orient_size(o[f], in_wh[2 * f], in_wh[2 * f + 1], &dw, &dh);
        return (size_t)dw * bpp;
    };
    if (!stage_side(n, d_out, out_pitch, shown_row, op)) return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return orient_launches(c, n, d_in, in_wh, ip.data(), channels, chw, o.data(), d_out, op.data(), st);
}

/* ---- gray to RGB ---------------------------------------------------------------- */
int zj_gray_to_rgb_device(zj_ctx* c, size_t n, const uint8_t* const* d_in, const unsigned* in_wh, const unsigned* in_pitch,
                          int out_layout, uint8_t* const* d_out, const unsigned* out_pitch, void* stream)
{
    if (!c || n == 0 || n > (size_t)1 << 20 || !d_in || !in_wh || !d_out) return ZJ_ERR_ARG;
    if (out_layout != ZJ_LAYOUT_HWC && out_layout != ZJ_LAYOUT_CHW) return ZJ_ERR_ARG;
    const int bpp = out_layout == ZJ_LAYOUT_CHW ? 1 : 3;
    std::vector<unsigned> ip, op;
    if (!stage_images(n, d_in, in_wh, in_pitch, 1, ip) || !stage_side(n, d_out, out_pitch, in_wh, bpp, op)) return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return expand_launches(c, n, d_in, in_wh, ip.data(), out_layout == ZJ_LAYOUT_CHW, d_out, op.data(), st);
}

// Library-internal (zj_jpeg.cpp: the single-file resized crop of a gray file shown as RGB): one tight plane expanded on the
// context stream into a tight image of out_layout; the context's crop buffer counts as read by it; synchronised
int zjint_gray_to_rgb_one(zj_ctx* c, const uint8_t* in, unsigned w, unsigned h, int out_layout, uint8_t* d_out)
{
    if (!c) return ZJ_ERR_ARG;
    const unsigned wh[2] = {w, h};
    int rc = zj_gray_to_rgb_device(c, 1, &in, wh, nullptr, out_layout, &d_out, nullptr, nullptr);
    return rc ? rc : one_image_done(c);
}

/* ---- CMYK to RGB ---------------------------------------------------------------- */
int zj_cmyk_to_rgb_device(zj_ctx* c, size_t n, const uint8_t* const* d_a, const uint8_t* const* d_k, const unsigned* in_wh,
                          const unsigned* a_pitch, const unsigned* k_pitch, int layout, const uint8_t* inverted,
                          uint8_t* const* d_out, const unsigned* out_pitch, void* stream)
{
    if (!c || n == 0 || n > (size_t)1 << 20 || !d_a || !d_k || !in_wh || !d_out) return ZJ_ERR_ARG;
    if (layout != ZJ_LAYOUT_HWC && layout != ZJ_LAYOUT_CHW) return ZJ_ERR_ARG;
    const int bpp = layout == ZJ_LAYOUT_CHW ? 1 : 3;
    std::vector<unsigned> ap, kp, op;
    if (!stage_images(n, d_a, in_wh, a_pitch, bpp, ap) || !stage_side(n, d_k, k_pitch, in_wh, 1, kp) ||
        !stage_side(n, d_out, out_pitch, in_wh, bpp, op))
        return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return cmyk_launches(c, n, d_a, d_k, in_wh, ap.data(), kp.data(), layout == ZJ_LAYOUT_CHW, inverted, d_out, op.data(), st);
}

// Library-internal (zj_jpeg.cpp: the single-file resized crop of a four-component file): one tight image combined in place with
// one tight plane on the context stream; the context's crop buffer counts as read by it; synchronised
int zjint_cmyk_to_rgb_one(zj_ctx* c, uint8_t* a, const uint8_t* k, unsigned w, unsigned h, int layout, int inverted)
{
    if (!c) return ZJ_ERR_ARG;
    const unsigned wh[2] = {w, h};
    const uint8_t inv = inverted ? 1 : 0;
    const uint8_t* ca = a;
    int rc = zj_cmyk_to_rgb_device(c, 1, &ca, &k, wh, nullptr, nullptr, layout, &inv, &a, nullptr, nullptr);
    return rc ? rc : one_image_done(c);
}

/* ---- colour matrices -------------------------------------------------------------- */
int zj_color_fixed(const double matrix[12], int32_t fixed[12])
{
    if (!matrix || !fixed) return ZJ_ERR_ARG;
    int32_t q[12];
    if (!color_fixed(matrix, q)) return ZJ_ERR_ARG;
    for (int k = 0; k < 12; k++) fixed[k] = q[k];
    return ZJ_OK;
}

int zj_color_device(zj_ctx* c, size_t n, const uint8_t* const* d_in, const unsigned* in_wh, const unsigned* in_pitch, int layout,
                    const double* matrices, uint8_t* const* d_out, const unsigned* out_pitch, void* stream)
{
    if (!c || n == 0 || n > (size_t)1 << 20 || !d_in || !in_wh || !matrices || !d_out) return ZJ_ERR_ARG;
    if (layout != ZJ_LAYOUT_HWC && layout != ZJ_LAYOUT_CHW) return ZJ_ERR_ARG;
    const int bpp = layout == ZJ_LAYOUT_CHW ? 1 : 3;
    std::vector<unsigned> ip, op;
    if (!stage_images(n, d_in, in_wh, in_pitch, bpp, ip) || !stage_side(n, d_out, out_pitch, in_wh, bpp, op)) return ZJ_ERR_ARG;
    std::vector<int32_t> q;
    int rc = color_matrices(matrices, n, q);
    if (rc) return rc;
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return color_launches(c, n, d_in, in_wh, ip.data(), layout == ZJ_LAYOUT_CHW, q.data(), d_out, op.data(), st);
}

// Library-internal (zj_jpeg.cpp: the single-file resized crop under a colour matrix): one tight image mapped in place under the
// 12 integers q on the context stream (the identity's: nothing is launched); the context's crop buffer counts as read by it;
// synchronised
int zjint_color_one(zj_ctx* c, uint8_t* img, unsigned w, unsigned h, int layout, const int32_t q[12])
{
    if (!c || !img || !q || !stage_size(w, h)) return ZJ_ERR_ARG;
    if (layout != ZJ_LAYOUT_HWC && layout != ZJ_LAYOUT_CHW) return ZJ_ERR_ARG;
    if (color_is_identity(q)) return ZJ_OK;
    const unsigned wh[2] = {w, h}, pitch = layout == ZJ_LAYOUT_CHW ? w : 3 * w;
    const uint8_t* in = img;
    ZJ_HIP(c, hipSetDevice(c->device));
    int rc = color_launches(c, 1, &in, wh, &pitch, layout == ZJ_LAYOUT_CHW, q, &img, &pitch, c->stream);
    return rc ? rc : one_image_done(c);
}

/* ---- tone curves: histogram, table build, lookup ----------------------------------- */
static bool tone_layout_ok(int channels, int layout)
{
    return (channels == 1 || channels == 3) && (layout == ZJ_LAYOUT_HWC || layout == ZJ_LAYOUT_CHW);
}
// bytes of a pixel inside a row: three only for interleaved 3-channel images
static int tone_bpp(int channels, int layout) { return channels == 3 && layout == ZJ_LAYOUT_HWC ? 3 : 1; }

int zj_histogram_device(zj_ctx* c, size_t n, const uint8_t* const* d_in, const unsigned* in_wh, const unsigned* in_pitch, int channels,
                        int layout, unsigned* d_hist, void* stream)
{
    if (!c || n == 0 || n > (size_t)1 << 20 || !d_in || !in_wh || !d_hist || ((uintptr_t)d_hist & 3u)) return ZJ_ERR_ARG;
    if (!tone_layout_ok(channels, layout)) return ZJ_ERR_ARG;
    std::vector<unsigned> ip;
    if (!stage_images(n, d_in, in_wh, in_pitch, tone_bpp(channels, layout), ip)) return ZJ_ERR_ARG;
    std::vector<const uint8_t*> tabs(n);
    for (size_t f = 0; f < n; f++) tabs[f] = (const uint8_t*)(d_hist + f * (size_t)channels * 256);
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    ZJ_HIP(c, hipMemsetAsync(d_hist, 0, n * (size_t)channels * 1024, st));
    return hist_launches(c, n, d_in, in_wh, ip.data(), channels, layout == ZJ_LAYOUT_CHW, tabs.data(), st);
}

int zj_tone_luts_device(zj_ctx* c, size_t n, int channels, const int32_t* ops, const unsigned* d_hist, uint8_t* d_luts, void* stream)
{
    if (!c || n == 0 || n > (size_t)1 << 20 || !ops || !d_luts || (channels != 1 && channels != 3)) return ZJ_ERR_ARG;
    if (!tone_ops_valid(ops, n) || ((uintptr_t)d_hist & 3u)) return ZJ_ERR_ARG;
    for (size_t f = 0; f < n; f++)
        if (tone_needs_hist(ops[2 * f]) && !d_hist) return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return tone_lut_launches(c, n, channels, ops, d_hist, d_luts, st);
}

int zj_lut_device(zj_ctx* c, size_t n, const uint8_t* const* d_in, const unsigned* in_wh, const unsigned* in_pitch, int channels,
                  int layout, const uint8_t* d_luts, uint8_t* const* d_out, const unsigned* out_pitch, void* stream)
{
    if (!c || n == 0 || n > (size_t)1 << 20 || !d_in || !in_wh || !d_luts || !d_out) return ZJ_ERR_ARG;
    if (!tone_layout_ok(channels, layout)) return ZJ_ERR_ARG;
    const int bpp = tone_bpp(channels, layout);
    std::vector<unsigned> ip, op;
    if (!stage_images(n, d_in, in_wh, in_pitch, bpp, ip) || !stage_side(n, d_out, out_pitch, in_wh, bpp, op)) return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return lut_launches(c, n, d_in, in_wh, ip.data(), channels, layout == ZJ_LAYOUT_CHW, d_luts, d_out, op.data(), st);
}

int zj_tone_device(zj_ctx* c, size_t n, const uint8_t* const* d_in, const unsigned* in_wh, const unsigned* in_pitch, int channels,
                   int layout, const int32_t* ops, uint8_t* const* d_out, const unsigned* out_pitch, void* stream)
{
    if (!c || n == 0 || n > (size_t)1 << 20 || !d_in || !in_wh || !ops || !d_out) return ZJ_ERR_ARG;
    if (!tone_layout_ok(channels, layout) || !tone_ops_valid(ops, n)) return ZJ_ERR_ARG;
    const int bpp = tone_bpp(channels, layout);
    std::vector<unsigned> ip, op;
    if (!stage_images(n, d_in, in_wh, in_pitch, bpp, ip) || !stage_side(n, d_out, out_pitch, in_wh, bpp, op)) return ZJ_ERR_ARG;
    // an identity image that is its own output is left out of every launch
    std::vector<const uint8_t*> in;
    std::vector<uint8_t*> out;
    std::vector<unsigned> wh, gip, gop;
    std::vector<int32_t> q;
    for (size_t f = 0; f < n; f++) {
        if (ops[2 * f] == TONE_IDENTITY && d_out[f] == d_in[f] && ip[f] == op[f]) continue;
        in.push_back(d_in[f]); out.push_back(d_out[f]);
        wh.push_back(in_wh[2 * f]); wh.push_back(in_wh[2 * f + 1]);
        gip.push_back(ip[f]); gop.push_back(op[f]);
        q.push_back(ops[2 * f]); q.push_back(ops[2 * f + 1]);
    }
    if (in.empty()) return ZJ_OK;
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return tone_launches(c, in.size(), in.data(), wh.data(), gip.data(), channels, layout == ZJ_LAYOUT_CHW, q.data(), out.data(),
                         gop.data(), st);
}

// Library-internal (zj_jpeg.cpp: the single-file resized crop under a tone op): one tight image mapped in place under the op
// on the context stream (ZJ_TONE_IDENTITY: nothing is launched); the context's crop buffer counts as read by it; synchronised
int zjint_tone_one(zj_ctx* c, uint8_t* img, unsigned w, unsigned h, int channels, int layout, const int32_t op[2])
{
    if (!c || !img || !op || !stage_size(w, h) || !tone_layout_ok(channels, layout) || !tone_op_valid(op[0], op[1])) return ZJ_ERR_ARG;
    if (op[0] == TONE_IDENTITY) return ZJ_OK;
    const unsigned wh[2] = {w, h}, pitch = w * (unsigned)tone_bpp(channels, layout);
    const uint8_t* in = img;
    ZJ_HIP(c, hipSetDevice(c->device));
    int rc = tone_launches(c, 1, &in, wh, &pitch, channels, layout == ZJ_LAYOUT_CHW, op, &img, &pitch, c->stream);
    return rc ? rc : one_image_done(c);
}

/* ---- component planes to RGB ------------------------------------------------------ */
// the checks and launches of zj_planes_to_rgb_device; phases: three (x mod rx, y mod ry) pairs per image, NULL: all 0
static int planes_to_rgb(zj_ctx* c, size_t n, const uint8_t* const* d_p0, const uint8_t* const* d_p1, const uint8_t* const* d_p2,
                         const unsigned* in_wh, const uint8_t* ratios, const uint8_t* phases, const unsigned* pitches, int stored_rgb,
                         int layout, uint8_t* const* d_out, const unsigned* out_pitch, void* stream)
{
    if (!c || n == 0 || n > (size_t)1 << 20 || !d_p0 || !d_p1 || !d_p2 || !in_wh || !ratios || !d_out) return ZJ_ERR_ARG;
    if (layout != ZJ_LAYOUT_HWC && layout != ZJ_LAYOUT_CHW) return ZJ_ERR_ARG;
    std::vector<unsigned> pp(3 * n), op;
    std::vector<uint32_t> geo(n);
    if (!stage_sizes(n, in_wh) || !stage_side(n, d_out, out_pitch, in_wh, layout == ZJ_LAYOUT_CHW ? 1 : 3, op)) return ZJ_ERR_ARG;
    for (size_t f = 0; f < n; f++) {
        if (!d_p0[f] || !d_p1[f] || !d_p2[f]) return ZJ_ERR_ARG;
        geo[f] = 0;
        for (int k = 0; k < 3; k++) {
            const size_t r = 6 * f + 2 * k;
            unsigned pw;
            uint32_t g;
            if (!planes_component(in_wh[2 * f], ratios[r], ratios[r + 1], phases ? phases[r] : 0, phases ? phases[r + 1] : 0, pw, g) ||
                !stage_pitch(pitches, 3 * f + k, pw, pp[3 * f + k]))
                return ZJ_ERR_ARG;
            geo[f] |= g << (8 * k);
        }
    }
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return planes_launches(c, n, d_p0, d_p1, d_p2, in_wh, geo.data(), pp.data(), stored_rgb ? 1 : 0, layout == ZJ_LAYOUT_CHW, d_out,
                           op.data(), st);
}

int zj_planes_to_rgb_device(zj_ctx* c, size_t n, const uint8_t* const* d_p0, const uint8_t* const* d_p1, const uint8_t* const* d_p2,
                            const unsigned* in_wh, const uint8_t* ratios, const unsigned* pitches, int stored_rgb, int layout,
                            uint8_t* const* d_out, const unsigned* out_pitch, void* stream)
{
    return planes_to_rgb(c, n, d_p0, d_p1, d_p2, in_wh, ratios, nullptr, pitches, stored_rgb, layout, d_out, out_pitch, stream);
}

// Library-internal (zj_jpeg.cpp: the single-file resized crop of an odd-sampled file): one image from three tight planes that
// begin at the window's first samples, with the window's phases, on the context stream; the context's crop buffer counts as
// read by it; synchronised
int zjint_planes_to_rgb_one(zj_ctx* c, const uint8_t* const planes[3], unsigned w, unsigned h, const uint8_t ratios[6],
                            const uint8_t phases[6], int stored_rgb, int layout, uint8_t* d_out)
{
    if (!c) return ZJ_ERR_ARG;
    const unsigned wh[2] = {w, h};
    int rc = planes_to_rgb(c, 1, &planes[0], &planes[1], &planes[2], wh, ratios, phases, nullptr, stored_rgb, layout, &d_out, nullptr,
                           nullptr);
    return rc ? rc : one_image_done(c);
}

// Library-internal (zj_jpeg.cpp: the decoder's oriented outputs): one image turned on the context stream, tight on both
// sides; the context's crop buffer counts as read by it; synchronised
int zjint_orient_one(zj_ctx* c, const uint8_t* in, unsigned w, unsigned h, int channels, int in_layout, int o, uint8_t* d_out)
{
    if (!c || o < 1 || o > 8) return ZJ_ERR_ARG;
    const unsigned wh[2] = {w, h};
    const uint8_t oo = (uint8_t)o;
    int rc = zj_orient_device(c, 1, &in, wh, nullptr, channels, in_layout, &oo, &d_out, nullptr, nullptr);
    return rc ? rc : one_image_done(c);
}

/* ---- reduced-size decode -------------------------------------------------------- */
int zj_scaled_size(const zj_frame_desc* d, int scale_log2, unsigned* w, unsigned* h)
{
    Plan pl;
    ScaledPlan sp;
    const int rc = make_scaled_plan(d, scale_log2, pl, sp);
    if (rc) return rc;
    if (w) *w = (unsigned)sp.rw;
    if (h) *h = (unsigned)sp.rh;
    return ZJ_OK;
}

size_t zj_scaled_crop_out_len(const zj_frame_desc* d, int scale_log2, unsigned w, unsigned h, unsigned out_pitch)
{
    Plan pl;
    ScaledPlan sp;
    if (make_scaled_plan(d, scale_log2, pl, sp)) return 0;
    return scaled_window_len(sp, 0, 0, w, h, out_pitch);
}

int zj_decode_crops_scaled_device(zj_ctx* c, const zj_frame_desc* d, size_t nframes, const int16_t* const* d_y,
                                  const int16_t* const* d_cb, const int16_t* const* d_cr, int scale_log2,
                                  const unsigned* windows, uint8_t* const* d_out, unsigned out_pitch, void* stream)
{
    if (!c || nframes == 0 || nframes > (size_t)1 << 20 || !d_out) return ZJ_ERR_ARG;
    Plan pl;
    ScaledPlan sp;
    int rc = make_scaled_plan(d, scale_log2, pl, sp);
    if (rc) return rc;
    const bool chroma = !sp.zero && pl.out != OUT_GRAY;
    if (!sp.zero && (rc = check_plane_ptrs(d_y, d_cb, d_cr, chroma, nframes))) return rc;
    for (size_t f = 0; f < nframes; f++) {
        const unsigned whole[4] = {0, 0, (unsigned)sp.rw, (unsigned)sp.rh};
        const unsigned* w = windows ? windows + 4 * f : whole;
        if (!scaled_window_len(sp, w[0], w[1], w[2], w[3], out_pitch)) return ZJ_ERR_ARG;
        if (!d_out[f]) return ZJ_ERR_ARG;
    }
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return scaled_launches(c, d, pl, sp, nframes, d_y, d_cb, d_cr, windows, d_out, out_pitch, s);
}

// Library-internal (zj_jpeg.cpp: zj_decoder_finish_pixels_scaled_device).  One frame's window of the reduced frame on the
// context stream, from planes in host memory -- only the MCU rows the window's blocks lie in are uploaded, each at its
// full-frame offset in the context's scratch -- or from planes already in HBM.  w == 0 && h == 0: the whole reduced frame.
int zjint_scaled_frame(zj_ctx* c, const zj_frame_desc* d, const int16_t* y, const int16_t* cb, const int16_t* cr,
                       int planes_on_device, int scale_log2, unsigned x, unsigned yy, unsigned w, unsigned h, uint8_t* d_out,
                       unsigned out_pitch)
{
    if (!c || !d_out) return ZJ_ERR_ARG;
    Plan pl;
    ScaledPlan sp;
    int rc = make_scaled_plan(d, scale_log2, pl, sp);
    if (rc) return rc;
    if (w == 0 && h == 0 && x == 0 && yy == 0) { w = (unsigned)sp.rw; h = (unsigned)sp.rh; }
    if (!scaled_window_len(sp, x, yy, w, h, out_pitch)) return ZJ_ERR_ARG;
    const bool chroma = !sp.zero && pl.out != OUT_GRAY;
    if (!sp.zero && (!y || (chroma && (!cb || !cr)))) return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    const int16_t* p[3] = {y, chroma ? cb : nullptr, chroma ? cr : nullptr};
    if (!planes_on_device && !sp.zero) {
        const size_t r0 = yy / sp.mh, r1 = ((size_t)yy + h + sp.mh - 1) / sp.mh; // MCU rows [r0, r1)
        const size_t yrow = (size_t)pl.mcu_x * pl.hs * pl.vs * 64, crow = (size_t)pl.mcu_x * 64; // i16 elements per MCU row
        if ((rc = upload_plane_rows(c, pl, chroma, y, cb, cr, r0, r1, yrow, crow, p))) return rc;
    }
    const unsigned win[4] = {x, yy, w, h};
    if ((rc = scaled_launches(c, d, pl, sp, 1, &p[0], &p[1], &p[2], win, &d_out, out_pitch, c->stream))) return rc;
    ZJ_HIP(c, hipStreamSynchronize(c->stream));
    return ZJ_OK;
}

// Library-internal (zj_jpeg.cpp: zj_decoder_finish_pixels_resized_crop_device): the crop buffer for one crop of `bytes` on
// the context stream, and the resize of that crop into d_out (on the context stream, synchronised)
int zjint_resize_scratch(zj_ctx* c, size_t bytes, uint8_t** p)
{
    if (!c || !p) return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    return resize_scratch(c, bytes, c->stream, p);
}

// ... the same buffer once nothing reads it any more: for a writer that is not ordered on the context stream
int zjint_scratch_idle(zj_ctx* c, size_t bytes, uint8_t** p)
{
    const int rc = zjint_resize_scratch(c, bytes, p);
    if (rc) return rc;
    ZJ_HIP(c, hipStreamSynchronize(c->stream));
    return ZJ_OK;
}

/* ---- u8 images to a normalised tensor, not resized --------------------------------- */
int zj_to_tensor_device(zj_ctx* c, size_t n, const uint8_t* const* d_in, unsigned w, unsigned h, const unsigned* in_pitch,
                        int in_channels, int channels, int dtype, int out_layout, const float* scale, const float* bias,
                        const uint8_t* flip, void* d_out, void* stream)
{
    if (!c || n == 0 || n > (size_t)1 << 20 || !d_in || !d_out) return ZJ_ERR_ARG;
    if (!((in_channels == 1 && (channels == 1 || channels == 3)) || (in_channels == 3 && channels == 3))) return ZJ_ERR_ARG;
    if (!stage_size(w, h)) return ZJ_ERR_ARG;
    const int E = resize_elem_bytes(dtype);
    if (!E || (out_layout != ZJ_TENSOR_NCHW && out_layout != ZJ_TENSOR_NHWC)) return ZJ_ERR_ARG;
    if ((uintptr_t)d_out % (uintptr_t)E) return ZJ_ERR_ARG; // (the kernel's blocks are counted from element boundaries)
    StageTensor t{(uint8_t*)d_out, (size_t)channels * w * h * (size_t)E, (int)w, (int)h, dtype, out_layout == ZJ_TENSOR_NHWC, {}, {}};
    if (!kernel_factors(scale, bias, channels, t.s, t.b)) return ZJ_ERR_ARG;
    std::vector<unsigned> pitch;
    if (!stage_side(n, d_in, in_pitch, [&](size_t) { return (size_t)w * in_channels; }, pitch)) return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    ToTensorParams p{};
    return stage_batches<TT_BATCH>(n, [&](size_t f0, int m) {
        pack_to_tensor(p, d_in, pitch.data(), flip, in_channels, channels, t, f0, m);
        ZJ_HIP(c, launch_to_tensor(p, st));
        return ZJ_OK;
    });
}

// Library-internal (zj_jpeg.cpp: the crop-tensor file calls of the files that pass through u8 stages): one tight image of the
// context's crop buffer converted on the context stream into d_out; the buffer counts as read by it; synchronised
int zjint_to_tensor_one(zj_ctx* c, const uint8_t* in, unsigned w, unsigned h, int in_channels, int channels, int dtype,
                        int out_layout, const float* scale, const float* bias, int flip, void* d_out)
{
    const uint8_t fl = flip ? 1 : 0;
    int rc = zj_to_tensor_device(c, 1, &in, w, h, nullptr, in_channels, channels, dtype, out_layout, scale, bias, &fl, d_out, nullptr);
    return rc ? rc : one_image_done(c);
}

// ... and the warp of that image under the integers q; w == 0: there is no image, the output is all fill
int zjint_warp_one(zj_ctx* c, const uint8_t* in, unsigned w, unsigned h, int channels, const int64_t q[6], unsigned out_w,
                   unsigned out_h, int dtype, int out_layout, const float* scale, const float* bias, const uint8_t* fill, int edge,
                   void* d_out)
{
    if (!c || !q || !d_out || (w != 0 && !in) || (channels != 1 && channels != 3)) return ZJ_ERR_ARG;
    if (w != 0 && !stage_size(w, h)) return ZJ_ERR_ARG;
    ResizeOut ro = resize_out(out_w, out_h, dtype, out_layout, scale, bias, nullptr, ZJ_RESIZE_BILINEAR, d_out);
    int rc = resize_out_args(ro, channels);
    if (rc) return rc;
    if ((uintptr_t)d_out % (uintptr_t)resize_elem_bytes(dtype)) return ZJ_ERR_ARG;
    WarpTail wt;
    if ((rc = warp_tail_args(fill, edge, channels, wt))) return rc;
    if (w == 0 && edge != ZJ_WARP_FILL) return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    const unsigned wh[2] = {w, h}, pitch = w * (unsigned)channels;
    rc = warp_launches(c, 1, &in, wh, &pitch, q, ro, wt, 0, c->stream);
    return rc ? rc : one_image_done(c);
}

int zjint_resize_one(zj_ctx* c, const uint8_t* in, unsigned w, unsigned h, int channels, int in_layout, unsigned out_w,
                     unsigned out_h, int dtype, int out_layout, const float* scale, const float* bias, int flip, int filter,
                     void* d_out)
{
    const unsigned wh[2] = {w, h};
    const uint8_t fl = flip ? 1 : 0;
    int rc = zj_resize_filtered_device(c, 1, &in, wh, nullptr, channels, in_layout, out_w, out_h, dtype, out_layout, scale,
                                       bias, &fl, filter, d_out, nullptr);
    return rc ? rc : one_image_done(c);
}

int zj_time_decode_device(zj_ctx* c, const zj_frame_desc* d, size_t nframes, const int16_t* d_y,
                          const int16_t* d_cb, const int16_t* d_cr, uint8_t* d_out, void* stream,
                          int iters, float* ms_total, float* ms_each, const char** kernel_name)
{
    Plan pl;
    int rc = check_frame_args(c, d, nframes, d_y, d_cb, d_cr, d_out, pl);
    if (rc) return rc;
    if (iters <= 0 || !ms_total) return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (kernel_name) {
        Params p;
        fill_params(d, pl, nframes, d_y, d_cb, d_cr, d_out, 1, p);
        *kernel_name = fused_kernel_name(pl.hs, pl.vs, pl.out, c->variant, launch_mode(pl, c->variant), p);
    }
    // (1) `iters` back-to-back launches between one event pair
    ZJ_HIP(c, hipEventRecord(c->ev0, s));
    for (int i = 0; i < iters; i++) {
        rc = decode_device_impl(c, d, pl, nframes, d_y, d_cb, d_cr, d_out, s, 1);
        if (rc) return rc;
    }
    ZJ_HIP(c, hipEventRecord(c->ev1, s));
    ZJ_HIP(c, hipEventSynchronize(c->ev1));
    ZJ_HIP(c, hipEventElapsedTime(ms_total, c->ev0, c->ev1));
    // (2) every launch bracketed by its own event pair: the per-dispatch duration a profiler reports
    if (ms_each) {
        double sum = 0;
        for (int i = 0; i < iters; i++) {
            ZJ_HIP(c, hipEventRecord(c->ev0, s));
            rc = decode_device_impl(c, d, pl, nframes, d_y, d_cb, d_cr, d_out, s, 1);
            if (rc) return rc;
            ZJ_HIP(c, hipEventRecord(c->ev1, s));
            ZJ_HIP(c, hipEventSynchronize(c->ev1));
            float t = 0;
            ZJ_HIP(c, hipEventElapsedTime(&t, c->ev0, c->ev1));
            sum += t;
        }
        *ms_each = (float)(sum / iters);
    }
    return ZJ_OK;
}

namespace {
// the host frames of a batch: packed back to back behind one base pointer per plane (zj_decode_planes_batch), or
// independent allocations named by pointer arrays (zj_decode_frames)
struct HostFrames {
    const int16_t* y = nullptr; const int16_t* cb = nullptr; const int16_t* cr = nullptr; uint8_t* out = nullptr;
    const int16_t* const* ys = nullptr; const int16_t* const* cbs = nullptr; const int16_t* const* crs = nullptr; uint8_t* const* outs = nullptr;
    size_t y_len = 0, c_len = 0, out_len = 0;
    bool packed() const { return ys == nullptr; }
    const int16_t* Y(size_t f) const { return ys ? ys[f] : y + f * y_len; }
    const int16_t* Cb(size_t f) const { return cbs ? cbs[f] : (cb ? cb + f * c_len : nullptr); }
    const int16_t* Cr(size_t f) const { return crs ? crs[f] : (cr ? cr + f * c_len : nullptr); }
    uint8_t* Out(size_t f) const { return outs ? outs[f] : out + f * out_len; }
};
}

static int decode_planes_batch_impl(zj_ctx* c, const zj_frame_desc* d, const Plan& pl, size_t nframes, const HostFrames& hf);

// drains what an error half way left in flight on the three streams before the caller may free or reuse its buffers
// (the first error stays in last_error)
static int batch_guard(zj_ctx* c, int rc)
{
    if (rc && c && c->s_up) {
        const std::string keep = c->last_error;
        (void)pipe_sync(c);
        c->last_error = keep;
    }
    return rc;
}

int zj_decode_planes_batch(zj_ctx* c, const zj_frame_desc* d, size_t nframes, const int16_t* y,
                           const int16_t* cb, const int16_t* cr, uint8_t* out)
{
    Plan pl;
    const int rc = check_frame_args(c, d, nframes, y, cb, cr, out, pl);
    if (rc) return rc;
    HostFrames hf;
    hf.y = y; hf.cb = cb; hf.cr = cr; hf.out = out;
    hf.y_len = pl.y_len; hf.c_len = pl.c_len; hf.out_len = pl.out_len;
    return batch_guard(c, decode_planes_batch_impl(c, d, pl, nframes, hf));
}

int zj_decode_frames(zj_ctx* c, const zj_frame_desc* d, size_t nframes, const int16_t* const* y, const int16_t* const* cb,
                     const int16_t* const* cr, uint8_t* const* out)
{
    Plan pl;
    int rc = check_frame_args(c, d, nframes, y, cb, cr, out, pl);
    if (rc) return rc;
    const bool chroma = pl.out != OUT_GRAY;
    for (size_t f = 0; f < nframes; f++)
        if (!y[f] || !out[f] || (chroma && (!cb[f] || !cr[f]))) return ZJ_ERR_ARG;
    HostFrames hf;
    hf.ys = y; hf.cbs = chroma ? cb : nullptr; hf.crs = chroma ? cr : nullptr; hf.outs = out;
    hf.y_len = pl.y_len; hf.c_len = pl.c_len; hf.out_len = pl.out_len;
    return batch_guard(c, decode_planes_batch_impl(c, d, pl, nframes, hf));
}

// One unit of the three-stream host pipeline: strips [s0, s1) of frames [f0, f0 + nfr) -- whole frames (s0 == 0, s1 == n_strips)
// or a strip range of ONE frame -- uploaded on s_up, decoded on s_run, and (d_out null) downloaded on s_down into the host
// frames' pixels, or (d_out: the frame's device output) decoded straight into place with no copy back.  `u` numbers the units
// of the call: unit u uses buffer set u % N_SLOTS.
static int submit_unit(zj_ctx* c, const zj_frame_desc* d, const Plan& pl, const HostFrames& hf, size_t f0, size_t nfr, size_t s0, size_t s1,
                       size_t u, size_t covered, uint8_t* d_out)
{
    int rc;
    const bool chroma = pl.out != OUT_GRAY;
    const int mrps = pl.hs == 2 ? 2 : 1;                                     // MCU rows per strip
    const size_t ystrip = (size_t)pl.mcu_x * 64 * pl.hs * pl.vs * mrps;      // i16 per strip
    const size_t cstrip = (size_t)pl.mcu_x * 64 * mrps;
    const size_t ostrip = (size_t)d->width * pl.ncomp_out * pl.strip_rows;   // bytes per strip
    const size_t covered_bytes = covered * d->width * pl.ncomp_out;
    const bool planar = pl.out == OUT_RGB_CHW;
    const bool whole = s0 == 0 && s1 == (size_t)pl.n_strips;
    PipeSlot& sl = c->slots[u % N_SLOTS];
    // unit extents: whole frames keep the frame strides; a strip range is one short "frame"
    const size_t yel = whole ? nfr * pl.y_len : (s1 - s0) * ystrip;
    const size_t cel = whole ? nfr * pl.c_len : (s1 - s0) * cstrip;
    size_t obytes = whole ? nfr * pl.out_len : (s1 - s0) * ostrip;
    if (!whole && s0 * ostrip + obytes > covered_bytes) obytes = covered_bytes - s0 * ostrip;
    if ((rc = ensure_slot(c, sl, 0, yel * 2))) return rc;
    if (chroma && ((rc = ensure_slot(c, sl, 1, cel * 2)) || (rc = ensure_slot(c, sl, 2, cel * 2)))) return rc;
    if (!d_out && (rc = ensure_slot(c, sl, 3, whole ? nfr * pl.out_len : (s1 - s0) * ostrip))) return rc;
    // up: the slot's planes are free once the kernel of its previous unit has run
    if (sl.used) ZJ_HIP(c, hipStreamWaitEvent(c->s_up, sl.run_done, 0));
    if (!whole || hf.packed()) {
        const size_t yo = whole ? 0 : s0 * ystrip, co = whole ? 0 : s0 * cstrip;
        ZJ_HIP(c, hipMemcpyAsync(sl.buf[0], hf.Y(f0) + yo, yel * 2, hipMemcpyHostToDevice, c->s_up));
        if (chroma) {
            ZJ_HIP(c, hipMemcpyAsync(sl.buf[1], hf.Cb(f0) + co, cel * 2, hipMemcpyHostToDevice, c->s_up));
            ZJ_HIP(c, hipMemcpyAsync(sl.buf[2], hf.Cr(f0) + co, cel * 2, hipMemcpyHostToDevice, c->s_up));
        }
    } else {
        for (size_t f = 0; f < nfr; f++) {
            ZJ_HIP(c, hipMemcpyAsync((int16_t*)sl.buf[0] + f * pl.y_len, hf.Y(f0 + f), pl.y_len * 2, hipMemcpyHostToDevice, c->s_up));
            if (chroma) {
                ZJ_HIP(c, hipMemcpyAsync((int16_t*)sl.buf[1] + f * pl.c_len, hf.Cb(f0 + f), pl.c_len * 2, hipMemcpyHostToDevice, c->s_up));
                ZJ_HIP(c, hipMemcpyAsync((int16_t*)sl.buf[2] + f * pl.c_len, hf.Cr(f0 + f), pl.c_len * 2, hipMemcpyHostToDevice, c->s_up));
            }
        }
    }
    ZJ_HIP(c, hipEventRecord(sl.up_done, c->s_up));
    // run: after this unit's upload and after the slot's previous download has drained its pixels
    ZJ_HIP(c, hipStreamWaitEvent(c->s_run, sl.up_done, 0));
    if (sl.used && !d_out) ZJ_HIP(c, hipStreamWaitEvent(c->s_run, sl.down_done, 0));
    Params p;
    fill_params(d, pl, whole ? nfr : 1, (const int16_t*)sl.buf[0], (const int16_t*)sl.buf[1],
                (const int16_t*)sl.buf[2], d_out ? d_out + (whole ? 0 : s0 * (size_t)pl.strip_rows * pl.out_pitch) : (uint8_t*)sl.buf[3], 1, p);
    if (!whole) { // strips [s0, s1) of frame f0 as a frame of its own
        p.height = (int)d->height - (int)s0 * pl.strip_rows;
        set_grid(p, 1, (int)(s1 - s0), pl.tiles_per_row);
    }
    if ((rc = launch_params(c, pl, p, c->s_run, whole))) return rc;
    ZJ_HIP(c, hipEventRecord(sl.run_done, c->s_run));
    if (d_out) { sl.used = true; return ZJ_OK; } // the pixels are where they belong
    // down
    ZJ_HIP(c, hipStreamWaitEvent(c->s_down, sl.run_done, 0));
    if (planar) { // the covered rows of every plane of every frame
        for (size_t f = 0; f < nfr; f++)
            for (size_t pc = 0; pc < 3; pc++) {
                const size_t po = pc * (size_t)d->width * d->height;
                ZJ_HIP(c, hipMemcpyAsync(hf.Out(f0 + f) + po, (uint8_t*)sl.buf[3] + f * pl.out_len + po, covered * d->width,
                                         hipMemcpyDeviceToHost, c->s_down));
            }
    } else if (whole && (covered_bytes < pl.out_len || !hf.packed())) { // frame by frame, without the never-written rows
        for (size_t f = 0; f < nfr; f++)
            ZJ_HIP(c, hipMemcpyAsync(hf.Out(f0 + f), (uint8_t*)sl.buf[3] + f * pl.out_len, covered_bytes,
                                     hipMemcpyDeviceToHost, c->s_down));
    } else {
        ZJ_HIP(c, hipMemcpyAsync(hf.Out(f0) + (whole ? 0 : s0 * ostrip), sl.buf[3], obytes,
                                 hipMemcpyDeviceToHost, c->s_down));
    }
    ZJ_HIP(c, hipEventRecord(sl.down_done, c->s_down));
    sl.used = true;
    return ZJ_OK;
}

static int decode_planes_batch_impl(zj_ctx* c, const zj_frame_desc* d, const Plan& pl, size_t nframes, const HostFrames& hf)
{
    // Host planes -> host pixels.  The batch is cut into units of about 16 MB of coefficients (ZJ_UNIT_MB) --
    // several whole frames, or a strip range of one large frame (strips are independent: no filter tap
    // crosses a strip, Q3/Q4).  Uploads, kernels and downloads run on a stream each, chained by events over
    // N_SLOTS buffer sets, so the upload of one unit, the kernel of the previous and the download of the one
    // before overlap (PCIe is full duplex).  Pinned host buffers (zj_alloc_pinned) make the copies asynchronous.
    //   Frames that are independent allocations (zj_decode_frames) differ only in the copies: one per frame and plane
    // where packed frames take one per unit and plane; on the device a unit is packed either way.
    int rc;
    // a padded row pitch is a layout for outputs that stay on the device (the kernels never write the padding; the copies
    // of this pipeline move whole strips): host outputs are tight, as the reference's are
    if (pl.out_pitch != pl.row_bytes) return ZJ_ERR_UNSUPPORTED;
    ZJ_HIP(c, hipSetDevice(c->device));
    const bool chroma = pl.out != OUT_GRAY;
    const size_t covered = (size_t)pl.rows_covered < d->height ? (size_t)pl.rows_covered : d->height;
    // rows below the last complete strip are never written by the reference (Q6)
    {
        size_t off[3], len[3];
        const int nr = uncovered_ranges(d, pl, off, len);
        for (size_t f = 0; f < nframes; f++)
            for (int r = 0; r < nr; r++) memset(hf.Out(f) + off[r], 0, len[r]);
    }
    if (pl.n_strips == 0) return ZJ_OK;

    size_t UNIT_TARGET = UNIT_TARGET_DEFAULT;
    if (const char* e = getenv("ZJ_UNIT_MB")) { const long v = atol(e); if (v > 0 && v < 4096) UNIT_TARGET = (size_t)v << 20; }
    const size_t in_frame = (pl.y_len + (chroma ? 2 * pl.c_len : 0)) * 2;
    size_t split = 1, group = 1; // strip ranges per frame | frames per unit
    const bool planar = pl.out == OUT_RGB_CHW; // a strip range is not contiguous in a planar frame: whole frames only
    if (c->pipeline) {
        if (in_frame >= 2 * UNIT_TARGET && !planar) {
            split = (in_frame + UNIT_TARGET - 1) / UNIT_TARGET;
            if (split > (size_t)pl.n_strips) split = (size_t)pl.n_strips;
        } else {
            group = UNIT_TARGET / (in_frame ? in_frame : 1);
            if (group < 1) group = 1;
            if (group * N_SLOTS > nframes) group = (nframes + N_SLOTS - 1) / N_SLOTS; // keep every slot busy
        }
    } else group = nframes;
    const size_t strips_per_unit = ((size_t)pl.n_strips + split - 1) / split;

    if ((rc = pipe_init(c))) return rc;

    size_t u = 0;
    for (size_t f0 = 0; f0 < nframes; f0 += group) {
        const size_t nfr = f0 + group <= nframes ? group : nframes - f0;
        for (size_t s0 = 0; s0 < (size_t)pl.n_strips; s0 += strips_per_unit, u++) {
            const size_t s1 = s0 + strips_per_unit < (size_t)pl.n_strips ? s0 + strips_per_unit : (size_t)pl.n_strips;
            if ((rc = submit_unit(c, d, pl, hf, f0, nfr, s0, s1, u, covered, nullptr))) return rc;
        }
    }
    return pipe_sync(c);
}

/* ---- one frame whose planes are still being written: strips go to the GPU as they become final ----------------------
 * The reference runs post_process on strip N while its Huffman decoder is in strip N + 1 (src/mcu.rs:356-368).  Here the
 * caller names the frame (zj_frame_begin), says every now and then how many MCU rows are final (zj_frame_rows_ready),
 * and the library pushes the strips that became complete through the three-stream pipeline in units of a few MB while
 * the caller goes on filling the planes; zj_frame_end submits the rest and waits.  Every call returns at once (the copies
 * are asynchronous when the planes are pinned). */
static int frame_submit(zj_ctx* c, size_t upto, bool last)
{
    zj_ctx::FrameStream& f = c->fs;
    Plan pl;
    int rc = make_plan(&f.d, pl);
    if (rc) return rc;
    HostFrames hf;
    uint8_t* const d_out = f.on_device ? f.out : (f.staged ? (uint8_t*)c->scratch[3] : nullptr);
    hf.y = f.y; hf.cb = f.cb; hf.cr = f.cr; hf.out = d_out ? nullptr : f.out;
    hf.y_len = pl.y_len; hf.c_len = pl.c_len; hf.out_len = pl.out_len;
    const size_t covered = (size_t)pl.rows_covered < f.d.height ? (size_t)pl.rows_covered : f.d.height;
    if (upto > (size_t)pl.n_strips) upto = (size_t)pl.n_strips;
    while (f.submitted < upto && (last || upto - f.submitted >= f.unit)) {
        size_t s1 = f.submitted + f.unit;
        if (s1 > upto || (last && (size_t)pl.n_strips - s1 < f.unit / 2)) s1 = last ? (size_t)pl.n_strips : upto; // (no tiny last unit)
        if (s1 > (size_t)pl.n_strips) s1 = (size_t)pl.n_strips;
        if ((rc = submit_unit(c, &f.d, pl, hf, 0, 1, f.submitted, s1, f.units, covered, d_out))) return rc;
        f.units++;
        f.submitted = s1;
    }
    return ZJ_OK;
}

int zj_frame_begin(zj_ctx* c, const zj_frame_desc* d, const int16_t* y, const int16_t* cb, const int16_t* cr, uint8_t* out, int out_on_device)
{
    if (!c || c->fs.active) return ZJ_ERR_ARG;
    Plan pl;
    int rc = check_frame_args(c, d, 1, y, cb, cr, out, pl);
    if (rc) return rc;
    if (out_on_device && ((uintptr_t)out & 15)) return ZJ_ERR_ARG;
    if (!out_on_device && pl.out_pitch != pl.row_bytes) return ZJ_ERR_UNSUPPORTED; // (host outputs are tight)
    if (pl.out == OUT_RGB_CHW) return ZJ_ERR_UNSUPPORTED; // a strip range is not contiguous in a planar frame
    ZJ_HIP(c, hipSetDevice(c->device));
    if ((rc = pipe_init(c))) return rc;
    zj_ctx::FrameStream& f = c->fs;
    f.d = *d; f.y = y; f.cb = cb; f.cr = cr; f.out = out; f.on_device = out_on_device ? 1 : 0;
    f.submitted = 0; f.units = 0;
    f.staged = false;
    if (!out_on_device) {
        hipPointerAttribute_t a;
        memset(&a, 0, sizeof a);
        const bool pinned = hipPointerGetAttributes(&a, out) == hipSuccess && a.type == hipMemoryTypeHost;
        if (!pinned) { (void)hipGetLastError(); f.staged = true; if ((rc = ensure_scratch(c, 3, pl.out_len))) return rc; }
    }
    const bool to_device = out_on_device || f.staged;
    // units: an eighth of the frame, at least ZJ_STREAM_UNIT_MB (4) of coefficients -- every copy costs ~15 us of the calling
    // thread and of the link, and the part that cannot overlap with the caller's work is the last unit
    const bool chroma = pl.out != OUT_GRAY;
    const size_t in_frame = (pl.y_len + (chroma ? 2 * pl.c_len : 0)) * 2;
    size_t min_unit = (size_t)4 << 20;
    if (const char* e = getenv("ZJ_STREAM_UNIT_MB")) { const long v = atol(e); if (v > 0 && v < 4096) min_unit = (size_t)v << 20; }
    const size_t per_strip = pl.n_strips ? in_frame / (size_t)pl.n_strips : in_frame;
    size_t unit = ((size_t)pl.n_strips + 7) / 8;
    if (per_strip && unit * per_strip < min_unit) unit = (min_unit + per_strip - 1) / per_strip;
    if (unit < 1) unit = 1;
    f.unit = unit;
    // the buffer sets at their final size now (growing one later would synchronise the pipeline in mid-frame)
    const int mrps = pl.hs == 2 ? 2 : 1;
    const size_t span = (unit + unit / 2 + 1 < (size_t)pl.n_strips ? unit + unit / 2 + 1 : (size_t)pl.n_strips);
    for (PipeSlot& sl : c->slots) {
        if ((rc = ensure_slot(c, sl, 0, span * (size_t)pl.mcu_x * 64 * pl.hs * pl.vs * mrps * 2))) return rc;
        if (chroma && ((rc = ensure_slot(c, sl, 1, span * (size_t)pl.mcu_x * 64 * mrps * 2)) || (rc = ensure_slot(c, sl, 2, span * (size_t)pl.mcu_x * 64 * mrps * 2)))) return rc;
        if (!to_device && (rc = ensure_slot(c, sl, 3, span * (size_t)d->width * pl.ncomp_out * pl.strip_rows))) return rc;
    }
    // rows below the last complete strip are never written by the reference (Q6)
    {
        size_t off[3], len[3];
        const int nr = uncovered_ranges(d, pl, off, len);
        if (!out_on_device) { for (int r = 0; r < nr; r++) memset(out + off[r], 0, len[r]); }
        else if (nr) {
            ZeroRows z{};
            z.out = out; z.frame_stride = 0; z.nr = nr; z.nframes = 1;
            for (int r = 0; r < nr; r++) { z.off[r] = off[r]; z.len[r] = len[r]; }
            ZJ_HIP(c, launch_zero_rows(z, c->s_run));
        }
    }
    f.active = true;
    return ZJ_OK;
}

int zj_frame_rows_ready(zj_ctx* c, size_t mcu_rows)
{
    if (!c || !c->fs.active) return ZJ_ERR_ARG;
    const size_t mrps = c->fs.d.h_max == 2 ? 2 : 1; // MCU rows per strip (zj_plan.h)
    return batch_guard(c, frame_submit(c, mcu_rows / mrps, false));
}

int zj_frame_end(zj_ctx* c)
{
    if (!c || !c->fs.active) return ZJ_ERR_ARG;
    int rc = frame_submit(c, (size_t)-1, true);
    c->fs.active = false;
    if (!rc) rc = pipe_sync(c);
    if (!rc && c->fs.staged) { // the rows the strips cover (the rest was cleared in zj_frame_begin)
        Plan pl;
        if (!(rc = make_plan(&c->fs.d, pl))) {
            const size_t covered = (size_t)pl.rows_covered < c->fs.d.height ? (size_t)pl.rows_covered : c->fs.d.height;
            const hipError_t e = hipMemcpy(c->fs.out, c->scratch[3], covered * pl.out_pitch, hipMemcpyDeviceToHost);
            if (e != hipSuccess) { c->last_error = std::string("hipMemcpy (zj_frame_end): ") + hipGetErrorString(e); rc = ZJ_ERR_HIP; }
        }
    }
    return batch_guard(c, rc);
}

int zj_frame_abort(zj_ctx* c)
{
    if (!c) return ZJ_ERR_ARG;
    if (!c->fs.active) return ZJ_OK;
    c->fs.active = false;
    return c->s_up ? pipe_sync(c) : ZJ_OK;
}

int zj_decode_planes(zj_ctx* c, const zj_frame_desc* d, const int16_t* y, const int16_t* cb,
                     const int16_t* cr, uint8_t* out)
{
    return zj_decode_planes_batch(c, d, 1, y, cb, cr, out);
}

/* Host planes -> pixels that STAY in HBM (d_out: device pointer, 16-byte aligned): for consumers on the same GPU. */
int zj_decode_planes_to_device(zj_ctx* c, const zj_frame_desc* d, const int16_t* y, const int16_t* cb, const int16_t* cr,
                               uint8_t* d_out)
{
    Plan pl;
    int rc = check_frame_args(c, d, 1, y, cb, cr, d_out, pl);
    if (rc) return rc;
    if ((uintptr_t)d_out & 15) return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    const bool chroma = pl.out != OUT_GRAY;
    if ((rc = ensure_scratch(c, 0, pl.y_len * 2))) return rc;
    if (chroma && ((rc = ensure_scratch(c, 1, pl.c_len * 2)) || (rc = ensure_scratch(c, 2, pl.c_len * 2)))) return rc;
    ZJ_HIP(c, hipMemcpyAsync(c->scratch[0], y, pl.y_len * 2, hipMemcpyHostToDevice, c->stream));
    if (chroma) {
        ZJ_HIP(c, hipMemcpyAsync(c->scratch[1], cb, pl.c_len * 2, hipMemcpyHostToDevice, c->stream));
        ZJ_HIP(c, hipMemcpyAsync(c->scratch[2], cr, pl.c_len * 2, hipMemcpyHostToDevice, c->stream));
    }
    rc = decode_device_impl(c, d, pl, 1, (const int16_t*)c->scratch[0], (const int16_t*)c->scratch[1],
                            (const int16_t*)c->scratch[2], d_out, c->stream, 1);
    if (rc) return rc;
    ZJ_HIP(c, hipStreamSynchronize(c->stream));
    return ZJ_OK;
}

int zj_device_memset(zj_ctx* c, void* d_ptr, int value, size_t bytes)
{
    if (!c || !d_ptr) return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    ZJ_HIP(c, hipMemsetAsync(d_ptr, value, bytes, c->stream));
    ZJ_HIP(c, hipStreamSynchronize(c->stream));
    return ZJ_OK;
}

/* ---- GPU entropy stage + pixel path: a prepared baseline scan (zj_huff.h) -> pixels ------------------------------- */
static int ensure_buf(zj_ctx* c, void** p, size_t* cap, size_t bytes)
{
    if (bytes <= *cap) return ZJ_OK;
    if (*p) { ZJ_HIP(c, hipStreamSynchronize(c->stream)); ZJ_HIP(c, hipFree(*p)); *p = nullptr; *cap = 0; }
    const size_t want = bytes + bytes / 4 + 4096;
    ZJ_HIP(c, hipMalloc(p, want));
    *cap = want;
    return ZJ_OK;
}

namespace {
struct ScanJob {
    const zj_frame_desc* d = nullptr;
    const HuffScan* h = nullptr;
    const void* blob = nullptr;
    size_t blob_bytes = 0, nsub = 0, yb = 0, cbytes = 0, ylen = 0, clen = 0;
    bool chroma = false;
    Plan pl;
    HuffArgs a;            // device pointers of the slot
    uint8_t* out = nullptr;    // the caller's
    uint8_t* d_out = nullptr;  // where the pixel kernel writes
    uint32_t* h_ctl = nullptr; // this slot's control words on the host
    int slot = 0, max_rounds = 0, planned = 0, rounds = 0;
    int rc = ZJ_OK;        // ZJ_OK while the job is alive
    bool synced = false;
};
size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// the arenas hold `slots` slots of `plane_bytes` / `out_bytes` each
int scan_arenas(zj_ctx* c, int slots, size_t plane_bytes, size_t out_bytes)
{
    auto grow = [&](void** p, size_t* stride, int* have, size_t need) -> int {
        if (*p && need <= *stride && slots <= *have) return ZJ_OK;
        const size_t st = need > *stride ? up256(need + need / 8) : *stride;
        const int n = slots > *have ? slots : *have;
        // nothing is remembered of an arena that is gone: if the hipMalloc below fails, the next call must not pass the
        // early-out on the strength of the freed arena's size
        if (*p) { ZJ_HIP(c, hipStreamSynchronize(c->stream)); ZJ_HIP(c, hipFree(*p)); *p = nullptr; }
        *stride = 0; *have = 0;
        ZJ_HIP(c, hipMalloc(p, st * (size_t)n));
        *stride = st; *have = n;
        return ZJ_OK;
    };
    int rc = grow(&c->harena, &c->harena_stride, &c->harena_slots, plane_bytes);
    if (rc) return rc;
    return out_bytes ? grow(&c->hout, &c->hout_stride, &c->hout_slots, out_bytes) : (int)ZJ_OK;
}

// A prepared scan is public input (zj_decode_scan / zj_decode_scans take any blob): every field the kernels index with is
// bounded here, so that a stale or malformed blob is an argument error and not an out-of-bounds access on the device.
bool scan_header_ok(const HuffScan* h, size_t blob_bytes)
{
    auto inside = [&](uint64_t off, uint64_t bytes) { return (off & 15) == 0 && off >= sizeof(HuffScan) && off + bytes <= blob_bytes; };
    if (h->ncomp != 1 && h->ncomp != 3) return false;
    if (h->bpm < 1 || h->bpm > (uint32_t)HUFF_MAX_BPM || h->nseg < 1 || h->nseg > h->nsub) return false;
    if (h->tab_entries == 0 || h->tab_entries > (uint32_t)HUFF_TAB_BUDGET || (h->tab_entries & 1)) return false;
    if (h->sub_bytes < 16 || h->sub_bytes > (uint32_t)HUFF_SUB_MAX || (h->sub_bytes & 15)) return false;
    if ((h->stream_bytes & 15) || h->stream_bytes < 32) return false;
    if (!inside(h->off_tab, (uint64_t)h->tab_entries * 2) || !inside(h->off_sub, ((uint64_t)h->nsub + 1) * sizeof(HuffSub)) ||
        !inside(h->off_seg, (uint64_t)h->nseg * sizeof(HuffSeg)) || !inside(h->off_per, (uint64_t)h->nsub * 4) ||
        !inside(h->off_stream, h->stream_bytes)) return false;
    if (h->mcu_x == 0 || h->mcu_y == 0 || (uint64_t)h->mcu_x * h->mcu_y != h->total_mcus || h->ri_mcus == 0 || h->rowlen == 0) return false;
    const uint16_t* tab = (const uint16_t*)((const uint8_t*)h + h->off_tab);
    // a decoding table: 2^l1 first-level entries at `base`, then the second-level tables its entries name (bit 15 set:
    // low byte = table number, 2^(16 - l1) entries each; huff_decode_* index base + 2^l1 + (number << (16 - l1)) + x)
    auto table_ok = [&](uint32_t base, uint32_t l1) {
        const uint64_t n1 = 1ull << l1, n2 = 1ull << (16 - l1);
        if ((uint64_t)base + n1 > h->tab_entries) return false;
        for (uint64_t q = 0; q < n1; q++) {
            const uint16_t e = tab[base + q];
            if ((e & 0x8000u) && (uint64_t)base + n1 + ((uint64_t)(e & 0xffu) + 1) * n2 > h->tab_entries) return false;
        }
        return true;
    };
    for (uint32_t k = 0; k < h->ncomp; k++) {
        if (h->comp[k].h < 1 || h->comp[k].h > 2 || h->comp[k].v < 1 || h->comp[k].v > 2) return false;
        // huff_block_ptr writes block (my * v + vy, mx * h + hx) of a plane of bw x bh blocks: the plane must hold the grid
        if ((uint64_t)h->comp[k].bw < (uint64_t)h->mcu_x * h->comp[k].h || (uint64_t)h->comp[k].bh < (uint64_t)h->mcu_y * h->comp[k].v) return false;
        if (!table_ok(h->dc_off[k], (uint32_t)HUFF_L1_DC) || !table_ok(h->ac_off[k], (uint32_t)HUFF_L1_AC)) return false;
    }
    uint32_t per_comp[3] = {0, 0, 0};
    for (uint32_t b = 0; b < h->bpm; b++) {
        const HuffBlk& k = h->blk[b];
        if (k.comp >= h->ncomp || k.hx >= h->comp[k.comp].h || k.vy >= h->comp[k.comp].v) return false;
        if (((h->comp_of_blk >> (2 * b)) & 3u) != k.comp) return false;
        per_comp[k.comp]++;
    }
    for (uint32_t k = 0; k < h->ncomp; k++)
        if (per_comp[k] != h->comp[k].h * h->comp[k].v) return false;
    // the grid and the segments: ascending, inside the stream
    const uint8_t* base = (const uint8_t*)h;
    const HuffSub* subs = (const HuffSub*)(base + h->off_sub);
    const HuffSeg* segs = (const HuffSeg*)(base + h->off_seg);
    for (uint32_t i = 0; i < h->nseg; i++)
        if (segs[i].start > segs[i].end || segs[i].end > h->stream_bytes - 32 || (segs[i].start & 15)) return false;
    for (uint32_t i = 0; i < h->nsub; i++) {
        const uint32_t sg = subs[i].seg & HUFF_SEG_MASK;
        if (sg >= h->nseg || subs[i].start < segs[sg].start || subs[i].start > segs[sg].end) return false;
        if (i && !(subs[i].seg & HUFF_FIRST) && subs[i].start <= subs[i - 1].start) return false;
    }
    // periodic-run words (zj_huff.h): huff_periodic_thread reads exit[r0 + q - 1], exit[r0 + 2q - 1] and
    // exit[r0 + q + (i - r0 - q) % q] for word i = (q << 28) | r0: a period of 1..8 sub-sequences, two whole periods in
    // front of i, all of it inside i's restart segment
    const uint32_t* per = (const uint32_t*)(base + h->off_per);
    for (uint32_t i = 0; i < h->nsub; i++) {
        const uint32_t w = per[i];
        if (!w) continue;
        const uint64_t q = w >> HUFF_PER_QSHIFT, r0 = w & HUFF_PER_MASK;
        if (q < 1 || q > HUFF_PER_MAXQ || r0 + 2 * q > i) return false;
        if ((subs[r0].seg & HUFF_SEG_MASK) != (subs[i].seg & HUFF_SEG_MASK)) return false;
    }
    return true;
}

// validates one scan, sizes its slot, fills the working-set pointers
int scan_setup(zj_ctx* c, ScanJob& j, int slot, const zj_frame_desc* d, const void* blob, size_t blob_bytes, uint8_t* out, int out_on_device)
{
    // (no output at all for the entropy stage alone, zjint_scan_to_planes: nothing of j.d_out is used then)
    if (!d || !blob || (!out && !c->scan_planes_only) || blob_bytes < sizeof(HuffScan)) return ZJ_ERR_ARG;
    const HuffScan* h = (const HuffScan*)blob;
    if (h->magic != HUFF_MAGIC || h->blob_bytes != blob_bytes || h->nsub == 0 || h->ncomp != d->in_components) return ZJ_ERR_ARG;
    if (!scan_header_ok(h, blob_bytes)) return ZJ_ERR_ARG;
    int rc = make_plan(d, j.pl);
    if (rc) return rc;
    // a padded pitch is a layout for outputs that stay in HBM (include/zjhip.h): the host copy moves pitch x height bytes out
    // of a reused staging arena, and the kernels never write the padding -- stale pixels of earlier decodes would go along
    if (!out_on_device && j.pl.out_pitch != j.pl.row_bytes) return ZJ_ERR_UNSUPPORTED;
    j.d = d; j.h = h; j.blob = blob; j.blob_bytes = blob_bytes; j.out = out; j.slot = slot;
    j.chroma = h->ncomp == 3;
    j.ylen = zj_plane_len(d, 0);
    j.clen = j.chroma ? zj_plane_len(d, 1) : 0;
    // the blob's grid is the descriptor's: same MCU counts, sampling factors and plane sizes as the plan the pixel kernel runs
    if ((int)h->mcu_x != j.pl.mcu_x || (int)h->mcu_y != j.pl.mcu_y || (int)h->comp[0].h != j.pl.hs || (int)h->comp[0].v != j.pl.vs) return ZJ_ERR_ARG;
    for (uint32_t k = 0; k < h->ncomp; k++) {
        if (k && (h->comp[k].h != 1 || h->comp[k].v != 1)) return ZJ_ERR_ARG;
        if (h->comp[k].bw != h->mcu_x * h->comp[k].h || h->comp[k].bh != h->mcu_y * h->comp[k].v) return ZJ_ERR_ARG;
    }
    if (j.ylen != (size_t)h->comp[0].bw * h->comp[0].bh * 64) return ZJ_ERR_ARG;
    if (j.chroma && (j.clen != (size_t)h->comp[1].bw * h->comp[1].bh * 64 || j.clen != (size_t)h->comp[2].bw * h->comp[2].bh * 64)) return ZJ_ERR_ARG;
    if (out_on_device && ((uintptr_t)out & 15)) return ZJ_ERR_ARG;
    j.nsub = h->nsub;
    const size_t nsub = j.nsub, nscan = (nsub + HUFF_SCAN_WG - 1) / HUFF_SCAN_WG;
    const size_t o_exit = up256(blob_bytes), o_aux = o_exit + up256(nsub * 8), o_base = o_aux + up256(nsub * 16),
                 o_lst = o_base + up256(nsub * 16), o_rel = o_lst + up256(nsub * 8 * HUFF_LIST_FACTOR),
                 o_agg = o_rel + up256(nsub), o_pre = o_agg + up256(nscan * sizeof(HuffAgg)),
                 total = o_pre + up256(nscan * sizeof(HuffAgg));
    zj_ctx::HuffSlot& sl = c->hslot[slot];
    if ((rc = ensure_buf(c, &sl.buf, &sl.cap, total))) return rc;
    j.yb = up256(j.ylen * 2);
    j.cbytes = up256(j.clen * 2);
    sl.planes = (uint8_t*)c->harena + (size_t)slot * c->harena_stride; // (the caller has sized the arenas for this call)
    sl.out = out_on_device ? nullptr : (uint8_t*)c->hout + (size_t)slot * c->hout_stride;
    uint8_t* base = (uint8_t*)sl.buf;
    HuffArgs& a = j.a;
    a.blob = base;
    a.exit = (unsigned long long*)(base + o_exit);
    a.aux = (HuffI4*)(base + o_aux);
    a.base = (HuffI4*)(base + o_base);
    a.exit_rd = a.exit;
    a.list = (uint32_t*)(base + o_lst);
    a.rel = base + o_rel;
    a.ctl = c->d_ctl + (size_t)slot * HUFF_CTL_WORDS;
    a.wgagg = (HuffAgg*)(base + o_agg);
    a.wgpre = (HuffAgg*)(base + o_pre);
    a.plane[0] = (int16_t*)sl.planes;
    a.plane[1] = (int16_t*)((uint8_t*)sl.planes + j.yb);
    a.plane[2] = (int16_t*)((uint8_t*)sl.planes + j.yb + j.cbytes);
    a.round = 0;
    a.spread = 1;
    a.zero_base = (uint8_t*)sl.planes;
    a.zero_pieces = (uint32_t)((j.yb + 2 * j.cbytes) / 16);
    j.d_out = out_on_device ? out : (uint8_t*)sl.out;
    j.h_ctl = c->h_ctl + (size_t)slot * HUFF_CTL_WORDS;
    const uint32_t sub_bytes = h->sub_bytes >= 16 && h->sub_bytes <= (uint32_t)HUFF_SUB_MAX ? h->sub_bytes : (uint32_t)HUFF_SUB_MAX;
    j.max_rounds = h->round_budget >= 1 && h->round_budget <= (uint32_t)HUFF_MAX_ROUNDS ? (int)h->round_budget : HUFF_MAX_ROUNDS;
    // Rounds launched ahead: a wrong guess falls into step within ~1 KB of 4:2:0 data, i.e. after 1024 / sub_bytes
    // rounds; files of one source need about the same number (quality 98 needs 24, a page with flat runs 40): two more
    // than the context's recent maximum, which decays by one per file
    j.planned = (int)(1536 / sub_bytes) + 2;
    if (c->huff_recent > 0) j.planned = c->huff_recent + 2;
    if (const char* e = getenv("ZJ_HUFF_ROUNDS")) { const int v = atoi(e); if (v >= 1) j.planned = v; }
    if (j.planned > j.max_rounds) j.planned = j.max_rounds;
    return ZJ_OK;
}

// before the write pass runs a second time: status, first-seen MCU and the prefix sums' ticket start over, and the planes
// hold coefficients of a wrong parse
int scan_clear_again(zj_ctx* c, ScanJob& j, hipStream_t s)
{
    ZJ_HIP(c, hipMemsetAsync(j.a.ctl, 0, (size_t)HUFF_CTL_ROUND0 * 4, s));
    ZJ_HIP(c, hipMemsetAsync(c->hslot[j.slot].planes, 0, j.yb + 2 * j.cbytes, s));
    return ZJ_OK;
}

// pixel kernel over the slot's planes, the pixels and the control words on their way back
int scan_pixels(zj_ctx* c, ScanJob& j, hipStream_t s, int out_on_device)
{
    if (!c->scan_planes_only) {
        const int rc = decode_device_impl(c, j.d, j.pl, 1, j.a.plane[0], j.chroma ? j.a.plane[1] : nullptr, j.chroma ? j.a.plane[2] : nullptr, j.d_out, s, 1);
        if (rc) return rc;
    }
    if (!out_on_device) ZJ_HIP(c, hipMemcpyAsync(j.out, j.d_out, j.pl.out_len, hipMemcpyDeviceToHost, s));
    ZJ_HIP(c, hipMemcpyAsync(j.h_ctl, j.a.ctl, (size_t)HUFF_CTL_WORDS * 4, hipMemcpyDeviceToHost, s));
    return ZJ_OK;
}

bool scan_check(ScanJob& j, int launched)
{
    for (int r = 1; r <= launched; r++)
        if (j.h_ctl[HUFF_CTL_ROUND0 + r] == 0) { j.synced = true; j.rounds = r; return true; }
    j.rounds = launched;
    return false;
}
} // namespace

// The scans of up to ZJ_SCAN_BATCH_MAX files as ONE launch per phase (blockIdx.y = file): a file's entropy kernels are
// latency-bound at under half a wave per SIMD (DESIGN_ENTROPY.md), several at once cost hardly more than one.
//   Synchronisation rounds are launched ahead and turn into no-ops once one of them changed nothing; a look at the
// counters costs a stream synchronisation, so it happens once, after the pixels.  A scan whose last planned round still
// changed something gets more rounds on its own (looking after each group), has what its premature write pass
// scattered cleared, and runs the rest again.
static int decode_scans_impl(zj_ctx* c, size_t n, const zj_frame_desc* descs, const void* const* blobs, const size_t* blob_bytes,
                             uint8_t* const* outs, int outs_on_device, int* rcs, unsigned* status_bits);

int zj_decode_scans(zj_ctx* c, size_t n, const zj_frame_desc* descs, const void* const* blobs, const size_t* blob_bytes,
                    uint8_t* const* outs, int outs_on_device, int* rcs, unsigned* status_bits)
{
    if (!c || !n || n > (size_t)ZJ_SCAN_BATCH_MAX || !descs || !blobs || !blob_bytes || !outs || !rcs) return ZJ_ERR_ARG;
    const int rc = decode_scans_impl(c, n, descs, blobs, blob_bytes, outs, outs_on_device, rcs, status_bits);
    if (rc) {
        // an error half way leaves copies and kernels in flight that read the caller's blobs and write its outputs:
        // drain them before the caller may free or reuse its buffers (the first error stays in last_error)
        const std::string keep = c->last_error;
        (void)hipStreamSynchronize(c->stream);
        c->last_error = keep;
        for (size_t k = 0; k < n; k++) if (rcs[k] == ZJ_OK) rcs[k] = rc;
    }
    return rc;
}

static int decode_scans_impl(zj_ctx* c, size_t n, const zj_frame_desc* descs, const void* const* blobs, const size_t* blob_bytes,
                             uint8_t* const* outs, int outs_on_device, int* rcs, unsigned* status_bits)
{
    ZJ_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (!c->h_ctl) ZJ_HIP(c, hipHostMalloc((void**)&c->h_ctl, (size_t)ZJ_SCAN_BATCH_MAX * HUFF_CTL_WORDS * 4, hipHostMallocPortable));
    if (!c->d_ctl) ZJ_HIP(c, hipMalloc((void**)&c->d_ctl, (size_t)ZJ_SCAN_BATCH_MAX * HUFF_CTL_WORDS * 4));
    static_assert(ZJ_SCAN_BATCH_MAX == HUFF_BATCH_MAX, "include/zjhip.h and zj_huff.h disagree");
    HuffBatch batch;
    const bool timing = getenv("ZJ_HUFF_TIME") != nullptr;
    const auto t_submit0 = std::chrono::steady_clock::now();
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    if (timing) { for (auto& e : ev) ZJ_HIP(c, hipEventCreate(&e)); ZJ_HIP(c, hipEventRecord(ev[0], s)); }
    {   // size the arenas for the largest scan of the call (a scan that fails validation below asks for nothing)
        size_t pmax = 0, omax = 0;
        for (size_t k = 0; k < n; k++) {
            if (!blobs[k] || blob_bytes[k] < sizeof(HuffScan)) continue;
            const HuffScan* h = (const HuffScan*)blobs[k];
            Plan pl;
            if (h->magic != HUFF_MAGIC || make_plan(&descs[k], pl)) continue;
            const size_t pb = up256(zj_plane_len(&descs[k], 0) * 2) + 2 * up256((h->ncomp == 3 ? zj_plane_len(&descs[k], 1) : 0) * 2);
            if (pb > pmax) pmax = pb;
            if (!outs_on_device && pl.out_len > omax) omax = pl.out_len;
        }
        if (pmax) { const int rc = scan_arenas(c, (int)n, pmax, omax); if (rc) return rc; }
    }
    std::vector<ScanJob> jobs(n);
    int live[ZJ_SCAN_BATCH_MAX], nlive = 0; // jobs that passed validation, packed: the kernels' argument array
    uint32_t max_nsub = 0;
    int planned = 1;
    for (size_t k = 0; k < n; k++) {
        if (status_bits) status_bits[k] = 0;
        rcs[k] = jobs[k].rc = scan_setup(c, jobs[k], (int)k, &descs[k], blobs[k], blob_bytes[k], outs[k], outs_on_device);
        if (jobs[k].rc) continue;
        live[nlive] = (int)k;
        batch.a[nlive++] = jobs[k].a;
        if (jobs[k].nsub > max_nsub) max_nsub = (uint32_t)jobs[k].nsub;
        if (jobs[k].planned > planned) planned = jobs[k].planned;
    }
    if (!nlive) return ZJ_OK;
    {   // alone on the GPU a scan's sparse rounds spread out (one entry per wave), in a batch they pack (HuffArgs::spread)
        int spread = nlive == 1 ? 64 : nlive == 2 ? 16 : nlive <= 4 ? 4 : 1;
        if (const char* e = getenv("ZJ_HUFF_SPREAD")) { const int v = atoi(e); if (v >= 1 && v <= 64) spread = v; }
        for (int q = 0; q < nlive; q++) batch.a[q].spread = spread;
    }
    ZJ_HIP(c, hipMemsetAsync(c->d_ctl, 0, n * (size_t)HUFF_CTL_WORDS * 4, s)); // (the planes: round 0 clears them on the side)
    for (int q = 0; q < nlive; q++) {
        ScanJob& j = jobs[(size_t)live[q]];
        ZJ_HIP(c, hipMemcpyAsync((void*)j.a.blob, j.blob, j.blob_bytes, hipMemcpyHostToDevice, s));
    }
    bool periodic = false; // some scan has periodic runs (flat areas): the rule of zj_huff.h runs between the rounds
    for (int q = 0; q < nlive; q++) periodic = periodic || jobs[(size_t)live[q]].h->nper != 0;
    for (int round = 0; round <= planned; round++) ZJ_HIP(c, launch_huff_sync(batch, nlive, max_nsub, round, periodic, s));
    if (timing) ZJ_HIP(c, hipEventRecord(ev[1], s));
    ZJ_HIP(c, launch_huff_finish(batch, nlive, max_nsub, s));
    if (timing) ZJ_HIP(c, hipEventRecord(ev[2], s));
    // Pixel kernel: the scans of one geometry and one set of tables go through it as the frames of ONE launch, wherever
    // their planes (arena slots) and their pixels (the staging arena, or whatever the caller's pointers are) happen to lie:
    // equally spaced frames take the strided form, anything else the scattered form (decode_frames_device_impl)
    if (!c->scan_planes_only) {
        bool launched[ZJ_SCAN_BATCH_MAX] = {};
        for (int q = 0; q < nlive; q++) {
            if (launched[q]) continue;
            const ScanJob& j0 = jobs[(size_t)live[q]];
            const int16_t* fy[ZJ_SCAN_BATCH_MAX]; const int16_t* fcb[ZJ_SCAN_BATCH_MAX]; const int16_t* fcr[ZJ_SCAN_BATCH_MAX];
            uint8_t* fo[ZJ_SCAN_BATCH_MAX];
            size_t run = 0;
            for (int r = q; r < nlive; r++) {
                const ScanJob& jn = jobs[(size_t)live[r]];
                if (launched[r] || memcmp(jn.d, j0.d, sizeof(zj_frame_desc)) != 0) continue;
                fy[run] = jn.a.plane[0]; fcb[run] = jn.a.plane[1]; fcr[run] = jn.a.plane[2]; fo[run] = jn.d_out;
                launched[r] = true;
                run++;
            }
            const int rc = decode_frames_device_impl(c, j0.d, j0.pl, run, fy, fcb, fcr, fo, s, 1);
            if (rc) return rc;
        }
    }
    for (int q = 0; q < nlive && !outs_on_device; q++) {
        ScanJob& j = jobs[(size_t)live[q]];
        ZJ_HIP(c, hipMemcpyAsync(j.out, j.d_out, j.pl.out_len, hipMemcpyDeviceToHost, s));
    }
    ZJ_HIP(c, hipMemcpyAsync(c->h_ctl, c->d_ctl, n * (size_t)HUFF_CTL_WORDS * 4, hipMemcpyDeviceToHost, s)); // every slot's control words
    if (timing) ZJ_HIP(c, hipEventRecord(ev[3], s));
    c->huff_submit_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_submit0).count();
    ZJ_HIP(c, hipStreamSynchronize(s));
    if (timing) {
        for (int k = 0; k < 3; k++) ZJ_HIP(c, hipEventElapsedTime(&c->huff_ms[k], ev[k], ev[k + 1]));
        for (auto& e : ev) (void)hipEventDestroy(e);
    }
    int most = 0;
    c->huff_rounds = 0;
    for (int q = 0; q < nlive; q++) {
        ScanJob& j = jobs[(size_t)live[q]];
        if (!scan_check(j, planned)) {
            // the slow way, this scan alone
            HuffBatch one;
            one.a[0] = j.a;
            one.a[0].spread = 64;
            int round = planned, group = 16;
            while (!j.synced && round < j.max_rounds) {
                const int first = round + 1;
                for (int k = 0; k < group && round < j.max_rounds; k++) ZJ_HIP(c, launch_huff_sync(one, 1, (uint32_t)j.nsub, ++round, j.h->nper != 0, s));
                ZJ_HIP(c, hipMemcpyAsync(j.h_ctl, j.a.ctl, (size_t)HUFF_CTL_WORDS * 4, hipMemcpyDeviceToHost, s));
                ZJ_HIP(c, hipStreamSynchronize(s));
                for (int r = first; r <= round; r++)
                    if (j.h_ctl[HUFF_CTL_ROUND0 + r] == 0) { j.synced = true; j.rounds = r; break; }
                group *= 2;
            }
            if (!j.synced) { // the CPU walker is the faster way out (nothing to learn from for the next files)
                j.rounds = round;
                rcs[live[q]] = ZJ_RETRY_CPU;
                if (status_bits) status_bits[live[q]] = HUFF_ST_NO_SYNC;
                if (j.rounds > c->huff_rounds) c->huff_rounds = j.rounds;
                continue;
            }
            int rc = scan_clear_again(c, j, s);
            if (rc) return rc;
            ZJ_HIP(c, launch_huff_finish(one, 1, (uint32_t)j.nsub, s));
            if ((rc = scan_pixels(c, j, s, outs_on_device))) return rc;
            ZJ_HIP(c, hipStreamSynchronize(s));
        }
        if (j.rounds > most) most = j.rounds;
        if (status_bits) status_bits[live[q]] = j.h_ctl[HUFF_CTL_STATUS];
        rcs[live[q]] = j.h_ctl[HUFF_CTL_STATUS] ? ZJ_RETRY_CPU : ZJ_OK;
    }
    if (most > c->huff_rounds) c->huff_rounds = most;
    // (rounds in units of the scans' sub-sequence size; a context is normally fed one kind of file; an outlier fades
    // by a quarter per call)
    if (most >= c->huff_recent) c->huff_recent = most;
    else { const int faded = c->huff_recent - (c->huff_recent / 4 > 1 ? c->huff_recent / 4 : 1); c->huff_recent = faded > most ? faded : most; }
    const ScanJob& j0 = jobs[(size_t)live[0]]; // zj_scan_planes looks at the first scan of the last call
    c->huff_plane_slot = j0.slot;
    c->huff_plane_off[0] = 0; c->huff_plane_off[1] = j0.yb; c->huff_plane_off[2] = j0.yb + j0.cbytes;
    c->huff_plane_len[0] = j0.ylen; c->huff_plane_len[1] = c->huff_plane_len[2] = j0.clen;
    return ZJ_OK;
}

int zj_decode_scan(zj_ctx* c, const zj_frame_desc* d, const void* blob, size_t blob_bytes, uint8_t* out, int out_on_device,
                   unsigned* status_bits)
{
    if (status_bits) *status_bits = 0;
    if (!c || !d) return ZJ_ERR_ARG;
    int rc1 = ZJ_OK;
    const int rc = zj_decode_scans(c, 1, d, &blob, &blob_bytes, &out, out_on_device, &rc1, status_bits);
    return rc ? rc : rc1;
}

// Library-internal (zj_jpeg.cpp): the entropy stage of one prepared scan on the device WITHOUT the pixel kernel; on ZJ_OK
// *planes are the three coefficient planes in the context's slot (valid until the next scan on this context)
int zjint_scan_to_planes(zj_ctx* c, const zj_frame_desc* d, const void* blob, size_t blob_bytes, const int16_t* planes[3],
                         unsigned* status_bits)
{
    if (!c || !d || !planes) return ZJ_ERR_ARG;
    c->scan_planes_only = true; // (scan_setup then takes a null output, and nothing launches a write to one)
    const int rc = zj_decode_scan(c, d, blob, blob_bytes, nullptr, 1, status_bits);
    c->scan_planes_only = false;
    if (rc) return rc;
    const uint8_t* base = (const uint8_t*)c->hslot[c->huff_plane_slot].planes;
    for (int k = 0; k < 3; k++) planes[k] = c->huff_plane_len[k] ? (const int16_t*)(base + c->huff_plane_off[k]) : nullptr;
    return ZJ_OK;
}

int zj_scan_planes(zj_ctx* c, int16_t* y, int16_t* cb, int16_t* cr, size_t len[3])
{
    if (!c || !c->hslot[c->huff_plane_slot].planes || !c->huff_plane_len[0]) return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    int16_t* dst[3] = {y, cb, cr};
    for (int k = 0; k < 3; k++) {
        if (len) len[k] = c->huff_plane_len[k];
        if (dst[k] && c->huff_plane_len[k])
            ZJ_HIP(c, hipMemcpyAsync(dst[k], (const uint8_t*)c->hslot[c->huff_plane_slot].planes + c->huff_plane_off[k], c->huff_plane_len[k] * 2, hipMemcpyDeviceToHost, c->stream));
    }
    ZJ_HIP(c, hipStreamSynchronize(c->stream));
    return ZJ_OK;
}

int zj_scan_stats(const zj_ctx* c, int* rounds, float ms[4])
{
    if (!c) return ZJ_ERR_ARG;
    if (rounds) *rounds = c->huff_rounds;
    if (ms) { for (int k = 0; k < 3; k++) ms[k] = c->huff_ms[k]; ms[3] = c->huff_submit_ms; }
    return ZJ_OK;
}

/* ---- strip level ---------------------------------------------------------------------------- */
int zj_idct_strip(zj_ctx* c, const int16_t* coeff, size_t n, const int32_t qt[64], size_t stride,
                  size_t samp_factors, size_t v_samp, int16_t* out)
{
    if (!c || !qt || (n && (!coeff || !out))) return ZJ_ERR_ARG;
    if (samp_factors == 0) return ZJ_ERR_PANIC;          // division by zero, scalar.rs:30
    if (n == 0) return ZJ_OK;
    for (int k = 0; k < 64; k++)
        if (qt[k] < 0 || qt[k] > 255) return ZJ_ERR_UNSUPPORTED;
    const size_t chunks = n * v_samp / samp_factors;     // scalar.rs:30
    if (chunks == 0) return ZJ_ERR_PANIC;                // chunks_exact(0)
    const size_t nchunks = n / chunks, bpc = chunks / 64;
    // get_mut(pos..pos+8).unwrap() (scalar.rs:52,249): the last block's last row must fit the chunk
    if (bpc > 0 && (bpc - 1) * 8 + 7 * stride + 8 > chunks) return ZJ_ERR_PANIC;
    ZJ_HIP(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_scratch(c, 0, n * 2)) || (rc = ensure_scratch(c, 1, n * 2))) return rc;
    hipStream_t s = c->stream;
    ZJ_HIP(c, hipMemcpyAsync(c->scratch[0], coeff, n * 2, hipMemcpyHostToDevice, s));
    ZJ_HIP(c, hipMemsetAsync(c->scratch[1], 0, n * 2, s)); // vec![0; len], scalar.rs:26
    ZJ_HIP(c, launch_idct_strip((const int16_t*)c->scratch[0], qt, (int16_t*)c->scratch[1],
                                (long long)(nchunks * bpc), (long long)chunks, (long long)bpc, (long long)stride, s));
    ZJ_HIP(c, hipMemcpyAsync(out, c->scratch[1], n * 2, hipMemcpyDeviceToHost, s));
    ZJ_HIP(c, hipStreamSynchronize(s));
    return ZJ_OK;
}

// runs one flat filter on device buffers (scratch[si] -> scratch[so]); no sync
static int upsample_h_dev(zj_ctx* c, int si, size_t n, int so, size_t out_len)
{
    if (!(out_len > 4 && n > 2)) return ZJ_ERR_PANIC; // assert!, upsampler/scalar.rs:9-12
    const size_t m = ((out_len - 2) / 2 < n - 2) ? (out_len - 2) / 2 : n - 2; // zip(chunks_exact_mut(2), windows(3))
    ZJ_HIP(c, hipMemsetAsync(c->scratch[so], 0, out_len * 2, c->stream));
    ZJ_HIP(c, launch_upsample_h((const int16_t*)c->scratch[si], (long long)n, (int16_t*)c->scratch[so],
                                (long long)out_len, (long long)m, c->stream));
    return ZJ_OK;
}
static int upsample_v_dev(zj_ctx* c, int si, size_t n, int so, size_t out_len)
{
    const size_t stride = n >> 3; // upsampler/scalar.rs:73
    if (stride == 0) return ZJ_ERR_PANIC;
    // out[i..].split_at_mut(stride) for i = 0, 2*stride, ... 14*stride (scalar.rs:95-110)
    if (14 * stride + stride > out_len) return ZJ_ERR_PANIC;
    ZJ_HIP(c, hipMemsetAsync(c->scratch[so], 0, out_len * 2, c->stream));
    ZJ_HIP(c, launch_upsample_v((const int16_t*)c->scratch[si], (long long)stride, (int16_t*)c->scratch[so],
                                (long long)out_len, c->stream));
    return ZJ_OK;
}

static int upsample_common(zj_ctx* c, int kind, const int16_t* in, size_t n, int16_t* out, size_t out_len)
{
    if (!c || !in || !out) return ZJ_ERR_ARG;
    ZJ_HIP(c, hipSetDevice(c->device));
    int rc;
    const size_t mid = n * 2;
    if ((rc = ensure_scratch(c, 0, (n ? n : 1) * 2)) || (rc = ensure_scratch(c, 1, (out_len ? out_len : 1) * 2)) ||
        (rc = ensure_scratch(c, 2, (mid ? mid : 1) * 2))) return rc;
    ZJ_HIP(c, hipMemcpyAsync(c->scratch[0], in, n * 2, hipMemcpyHostToDevice, c->stream));
    if (kind == 0) rc = upsample_h_dev(c, 0, n, 1, out_len);
    else if (kind == 1) rc = upsample_v_dev(c, 0, n, 1, out_len);
    else { // upsample_hv = horizontal(vertical(input, 2*len), output_len), scalar.rs:148-166
        rc = upsample_v_dev(c, 0, n, 2, mid);
        if (!rc) rc = upsample_h_dev(c, 2, mid, 1, out_len);
    }
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    ZJ_HIP(c, hipMemcpyAsync(out, c->scratch[1], out_len * 2, hipMemcpyDeviceToHost, c->stream));
    ZJ_HIP(c, hipStreamSynchronize(c->stream));
    return ZJ_OK;
}

int zj_upsample_h(zj_ctx* c, const int16_t* in, size_t n, int16_t* out, size_t out_len) { return upsample_common(c, 0, in, n, out, out_len); }
int zj_upsample_v(zj_ctx* c, const int16_t* in, size_t n, int16_t* out, size_t out_len) { return upsample_common(c, 1, in, n, out, out_len); }
int zj_upsample_hv(zj_ctx* c, const int16_t* in, size_t n, int16_t* out, size_t out_len) { return upsample_common(c, 2, in, n, out, out_len); }

int zj_ycbcr_to_rgb16(zj_ctx* c, const int16_t y[16], const int16_t cb[16], const int16_t cr[16],
                      uint8_t* out, size_t out_len, size_t* pos)
{
    if (!c || !y || !cb || !cr || !out || !pos) return ZJ_ERR_ARG;
    if (*pos > out_len || out_len - *pos < 48) return ZJ_ERR_PANIC; // "Slice to small cannot write", scalar.rs:57-64
    ZJ_HIP(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_scratch(c, 0, 96)) || (rc = ensure_scratch(c, 1, 48))) return rc;
    int16_t h[48];
    memcpy(h, y, 32); memcpy(h + 16, cb, 32); memcpy(h + 32, cr, 32);
    ZJ_HIP(c, hipMemcpyAsync(c->scratch[0], h, 96, hipMemcpyHostToDevice, c->stream));
    ZJ_HIP(c, hipStreamSynchronize(c->stream)); // `h` is pageable stack memory
    ZJ_HIP(c, launch_rgb16((const int16_t*)c->scratch[0], (uint8_t*)c->scratch[1], c->stream));
    ZJ_HIP(c, hipMemcpyAsync(out + *pos, c->scratch[1], 48, hipMemcpyDeviceToHost, c->stream));
    ZJ_HIP(c, hipStreamSynchronize(c->stream));
    *pos += 48;
    return ZJ_OK;
}

int zj_post_process_strip(zj_ctx* c, const int16_t* const coeff[3], const size_t len[3],
                          const zj_component comps[3], int in_cs, int out_cs, uint8_t* out,
                          size_t out_len, size_t width)
{
    if (!c || !coeff || !len || !comps || !out) return ZJ_ERR_ARG;
    const size_t hs = comps[0].horizontal_sample, vs = comps[0].vertical_sample; // worker.rs:43-45
    if (!((hs == 1 || hs == 2) && (vs == 1 || vs == 2))) return ZJ_ERR_UNSUPPORTED;
    if (in_cs != ZJ_CS_YCBCR && in_cs != ZJ_CS_GRAYSCALE) return ZJ_ERR_UNSUPPORTED;
    if (width == 0 || width > 65535) return ZJ_ERR_ARG;
    // One strip == a frame that is exactly one strip tall (mcu.rs:225-226).
    zj_frame_desc d;
    memset(&d, 0, sizeof d);
    d.width = (uint32_t)width;
    d.h_max = (uint32_t)hs; d.v_max = (uint32_t)vs;
    d.in_components = in_cs == ZJ_CS_YCBCR ? 3 : 1;
    d.out_colorspace = out_cs;
    const uint32_t strip_rows = (hs == 2 && vs == 2) ? 32 : ((hs == 2 || vs == 2) ? 16 : 8);
    d.height = strip_rows;
    for (int k = 0; k < 3; k++) memcpy(d.qt[k], comps[k < (int)d.in_components ? k : 0].quantization_table, 256);
    Plan pl;
    int rc = make_plan(&d, pl);
    if (rc) return rc;
    // the strip must have the geometry the reference's callers produce (headers.rs:338, mcu.rs:238-250)
    if (comps[0].width_stride != (size_t)pl.mcu_x * 8 * hs || len[0] != pl.y_len) return ZJ_ERR_UNSUPPORTED;
    const bool chroma = pl.out != OUT_GRAY;
    if (chroma && (len[1] != pl.c_len || len[2] != pl.c_len || comps[1].width_stride != (size_t)pl.mcu_x * 8 ||
                   comps[2].width_stride != (size_t)pl.mcu_x * 8)) return ZJ_ERR_UNSUPPORTED;
    if (!coeff[0] || (chroma && (!coeff[1] || !coeff[2]))) return ZJ_ERR_ARG;
    if (out_len < pl.out_len) return ZJ_ERR_PANIC; // &mut output[start..end], worker.rs:174
    ZJ_HIP(c, hipSetDevice(c->device));
    const size_t yb = pl.y_len * 2, cbytes = chroma ? pl.c_len * 2 : 0;
    if ((rc = ensure_scratch(c, 0, yb))) return rc;
    if (chroma && ((rc = ensure_scratch(c, 1, cbytes)) || (rc = ensure_scratch(c, 2, cbytes)))) return rc;
    if ((rc = ensure_scratch(c, 3, pl.out_len))) return rc;
    hipStream_t s = c->stream;
    ZJ_HIP(c, hipMemcpyAsync(c->scratch[0], coeff[0], yb, hipMemcpyHostToDevice, s));
    if (chroma) {
        ZJ_HIP(c, hipMemcpyAsync(c->scratch[1], coeff[1], cbytes, hipMemcpyHostToDevice, s));
        ZJ_HIP(c, hipMemcpyAsync(c->scratch[2], coeff[2], cbytes, hipMemcpyHostToDevice, s));
    }
    // bytes the reference never writes keep the caller's content: round-trip the caller's buffer
    ZJ_HIP(c, hipMemcpyAsync(c->scratch[3], out, pl.out_len, hipMemcpyHostToDevice, s));
    rc = decode_device_impl(c, &d, pl, 1, (const int16_t*)c->scratch[0], (const int16_t*)c->scratch[1],
                            (const int16_t*)c->scratch[2], (uint8_t*)c->scratch[3], s, 0);
    if (rc) return rc;
    ZJ_HIP(c, hipMemcpyAsync(out, c->scratch[3], pl.out_len, hipMemcpyDeviceToHost, s));
    ZJ_HIP(c, hipStreamSynchronize(s));
    return ZJ_OK;
}

/* ---- dispatch mirror ------------------------------------------------------------------------ */
zj_idct_fn zj_choose_idct_func(int backend) { return backend == ZJ_BACKEND_HIP ? zj_idct_strip : nullptr; }
zj_upsample_fn zj_choose_upsample_func(int backend, int h_max, int v_max)
{
    if (backend != ZJ_BACKEND_HIP) return nullptr;
    if (h_max == 2 && v_max == 1) return zj_upsample_h;  // decoder.rs:480-491
    if (h_max == 1 && v_max == 2) return zj_upsample_v;  // decoder.rs:492-501
    if (h_max == 2 && v_max == 2) return zj_upsample_hv; // decoder.rs:502-511
    return nullptr;                                      // (1,1): upsample_no_op / unknown ratio
}
zj_color_convert16_fn zj_choose_ycbcr_to_rgb_convert_func(int backend, int out_cs)
{
    // the reference only ever asks for ColorSpace::RGB (decoder.rs:127-128)
    if (backend != ZJ_BACKEND_HIP || out_cs != ZJ_CS_RGB) return nullptr;
    return zj_ycbcr_to_rgb16;
}

/* kernel-variant switch for A/B measurements (both variants are bit-exact) */
int zj_variant_available(int variant) { return variant == 0 || variant == 2 || (variant == 1 && fused_has_wide()) ? 1 : 0; }
int zj_set_variant(zj_ctx* c, int variant)
{
    if (!c || variant < 0 || variant > 2) return ZJ_ERR_ARG;
    if (variant == 1 && !fused_has_wide()) return ZJ_ERR_UNSUPPORTED; // round 1's generation: `make VARIANTS=all` builds (tests, A/B)
    c->variant = variant;
    return ZJ_OK;
}
/* 0 = one unit per zj_decode_planes_batch call (no copy/compute overlap); A/B timing only */
int zj_set_pipeline(zj_ctx* c, int on) { if (!c) return ZJ_ERR_ARG; c->pipeline = on ? 1 : 0; return ZJ_OK; }
} // extern "C"

#if defined(ZJ_ABLATION)
/* diagnostic build only (tools/build_variant.sh ablate "-DZJ_ABLATION"; never in the product library) */
/* occupancy probe (tools/occupancy.py): pad every fused launch with dynamic LDS; query workgroups per CU */
extern "C" __attribute__((visibility("default"))) int zj_set_pad_lds(int bytes) { set_pad_lds(bytes); return ZJ_OK; }
extern "C" __attribute__((visibility("default"))) int zj_fused_occupancy(int pad_lds) { return fused_occupancy_420_rgb(pad_lds); }
/* ablation for tools/ablate.py: bit 0 skips the IDCT, bit 1 the colour math; output is WRONG when non-zero */
extern "C" __attribute__((visibility("default"))) int zj_set_ablation(zj_ctx* c, int mask) { if (!c) return ZJ_ERR_ARG; c->debug = mask; return ZJ_OK; }
#endif

