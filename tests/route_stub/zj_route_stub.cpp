// TEST ONLY (tests/route_stub_c.py, tests/test_batch_routing.py).  The front-end zj_jpeg.cpp as it is, with every function
// it reaches outside itself -- the library-internal zjint_* calls and the few public zj_* ones -- replaced by a stand-in
// that launches nothing and writes down that it was called: which path a file of a batch takes is then readable on a
// machine without a GPU.  Never part of the product library.
#include "../../zune-jpeg_amd/csrc/zj_jpeg.cpp"

#include <vector>

namespace {
struct Rec {
    const char* name;
    long file;    // (d_out - base) / img when d_out lies in the batch's output, -1 otherwise (the context's buffer)
    long nframes; // of a *_mixed_host call, 0 otherwise
};
std::vector<Rec> g_log;
const uint8_t* g_base = nullptr;
size_t g_img = 0, g_n = 0;
int g_fail_nth = 0, g_mixed_calls = 0, g_scan_rc = ZJ_OK;
std::vector<uint8_t> g_scratch;
int16_t g_plane[64];

int note(const char* name, const void* d_out, size_t nframes = 0)
{
    long file = -1;
    const uint8_t* p = (const uint8_t*)d_out;
    if (g_img && g_base && p >= g_base && p < g_base + g_n * g_img) file = (long)((size_t)(p - g_base) / g_img);
    g_log.push_back(Rec{name, file, (long)nframes});
    return ZJ_OK;
}
int mixed(const char* name, const void* d_out, size_t nframes)
{
    note(name, d_out, nframes);
    return ++g_mixed_calls == g_fail_nth ? (int)ZJ_ERR_HIP : (int)ZJ_OK;
}
int scratch(size_t bytes, uint8_t** p)
{
    if (g_scratch.size() < bytes + 256) g_scratch.resize(bytes + 256);
    *p = g_scratch.data();
    return ZJ_OK;
}
} // namespace

extern "C" {
// the recorder: a batch whose output is n images of img bytes at base; fail_nth: the n-th *_mixed_host call from here on
// returns an error (0: none); scan_rc: what the entropy-stage stand-in returns
void zjrs_begin(const void* base, size_t img, size_t n, int fail_nth, int scan_rc)
{
    g_log.clear();
    g_base = (const uint8_t*)base; g_img = img; g_n = n;
    g_fail_nth = fail_nth; g_mixed_calls = 0; g_scan_rc = scan_rc;
}
size_t zjrs_count(void) { return g_log.size(); }
const char* zjrs_name(size_t i) { return i < g_log.size() ? g_log[i].name : ""; }
long zjrs_file(size_t i) { return i < g_log.size() ? g_log[i].file : -2; }
long zjrs_nframes(size_t i) { return i < g_log.size() ? g_log[i].nframes : -2; }

// ---- the public calls the front-end uses -----------------------------------------------------------------------------
void* zj_alloc_pinned(size_t bytes) { return malloc(bytes ? bytes : 1); }
void zj_free_pinned(void* p) { free(p); }
size_t zj_out_len(const zj_frame_desc* d)
{
    const int cs = d->out_colorspace;
    const size_t nc = (cs == ZJ_CS_GRAYSCALE) ? 1 : ((cs == ZJ_CS_RGB || cs == ZJ_CS_YCBCR) ? 3 : 4);
    return (size_t)d->width * d->height * nc;
}
int zj_decode_planes(zj_ctx*, const zj_frame_desc*, const int16_t*, const int16_t*, const int16_t*, uint8_t* out) { return note("zj_decode_planes", out); }
int zj_decode_planes_to_device(zj_ctx*, const zj_frame_desc*, const int16_t*, const int16_t*, const int16_t*, uint8_t* out) { return note("zj_decode_planes_to_device", out); }
int zj_decode_scan(zj_ctx*, const zj_frame_desc*, const void*, size_t, uint8_t* out, int, unsigned* st) { if (st) *st = 0; note("zj_decode_scan", out); return g_scan_rc; }
int zj_decode_scans(zj_ctx*, size_t, const zj_frame_desc*, const void* const*, const size_t*, uint8_t* const*, int, int*, unsigned*) { note("zj_decode_scans", nullptr); return ZJ_ERR_HIP; }
int zj_device_memset(zj_ctx*, void* p, int, size_t) { return note("zj_device_memset", p); }
int zj_frame_begin(zj_ctx*, const zj_frame_desc*, const int16_t*, const int16_t*, const int16_t*, uint8_t* out, int) { note("zj_frame_begin", out); return ZJ_ERR_NO_DEVICE; }
int zj_frame_rows_ready(zj_ctx*, size_t) { return ZJ_ERR_NO_DEVICE; }
int zj_frame_end(zj_ctx*) { return ZJ_ERR_NO_DEVICE; }
int zj_frame_abort(zj_ctx*) { return ZJ_OK; }
const char* zj_strerror(int) { return "stub"; }
const char* zj_last_error(const zj_ctx*) { return ""; }

// ---- the library-internal calls ------------------------------------------------------------------------------------------
int zjint_crop_frame(zj_ctx*, const zj_frame_desc*, const int16_t*, const int16_t*, const int16_t*, int, unsigned, unsigned, unsigned, unsigned,
                     uint8_t* d_out, unsigned)
{
    return note("zjint_crop_frame", d_out);
}
int zjint_scan_to_planes(zj_ctx*, const zj_frame_desc*, const void*, size_t, const int16_t* planes[3], unsigned* status_bits)
{
    if (status_bits) *status_bits = 0;
    planes[0] = planes[1] = planes[2] = g_plane;
    note("zjint_scan_to_planes", nullptr);
    return g_scan_rc;
}
int zjint_crop_zeros(zj_ctx*, const zj_frame_desc*, unsigned, unsigned, unsigned, unsigned, uint8_t* d_out, unsigned) { return note("zjint_crop_zeros", d_out); }
int zjint_resize_scratch(zj_ctx*, size_t bytes, uint8_t** p) { return scratch(bytes, p); }
int zjint_resize_one(zj_ctx*, const uint8_t*, unsigned, unsigned, int, int, unsigned, unsigned, int, int, const float*, const float*, int, int,
                     void* d_out)
{
    return note("zjint_resize_one", d_out);
}
int zjint_scratch_idle(zj_ctx*, size_t bytes, uint8_t** p) { return scratch(bytes, p); }
int zjint_orient_one(zj_ctx*, const uint8_t*, unsigned, unsigned, int, int, int, uint8_t* d_out) { return note("zjint_orient_one", d_out); }
int zjint_gray_to_rgb_one(zj_ctx*, const uint8_t*, unsigned, unsigned, int, uint8_t* d_out) { return note("zjint_gray_to_rgb_one", d_out); }
int zjint_cmyk_to_rgb_one(zj_ctx*, uint8_t* a, const uint8_t*, unsigned, unsigned, int, int) { return note("zjint_cmyk_to_rgb_one", a); }
int zjint_crops_resized_mixed_host(zj_ctx*, const zj_frame_desc*, size_t nframes, const int16_t* const*, const int16_t* const*,
                                   const int16_t* const*, const unsigned*, unsigned, unsigned, int, int, const float*, const float*,
                                   const uint8_t*, int, int, const uint8_t*, void* d_out)
{
    return mixed("zjint_crops_resized_mixed_host", d_out, nframes);
}
int zjint_scaled_frame(zj_ctx*, const zj_frame_desc*, const int16_t*, const int16_t*, const int16_t*, int, int, unsigned, unsigned, unsigned,
                       unsigned, uint8_t* d_out, unsigned)
{
    return note("zjint_scaled_frame", d_out);
}
int zjint_to_tensor_one(zj_ctx*, const uint8_t*, unsigned, unsigned, int, int, int, int, const float*, const float*, int, void* d_out)
{
    return note("zjint_to_tensor_one", d_out);
}
int zjint_warp_one(zj_ctx*, const uint8_t*, unsigned, unsigned, int, const int64_t[6], unsigned, unsigned, int, int, const float*, const float*,
                   const uint8_t*, int, void* d_out)
{
    return note("zjint_warp_one", d_out);
}
int zjint_crops_warped_mixed_host(zj_ctx*, const zj_frame_desc*, size_t nframes, const int16_t* const*, const int16_t* const*,
                                  const int16_t* const*, const unsigned*, const int64_t*, unsigned, unsigned, int, int, const float*,
                                  const float*, const uint8_t*, int, const uint8_t*, void* d_out)
{
    return mixed("zjint_crops_warped_mixed_host", d_out, nframes);
}
int zjint_planes_to_rgb_one(zj_ctx*, const uint8_t* const[3], unsigned, unsigned, const uint8_t[6], const uint8_t[6], int, int, uint8_t* d_out)
{
    return note("zjint_planes_to_rgb_one", d_out);
}
int zjint_crop_tensor_frame(zj_ctx*, const zj_frame_desc*, const int16_t*, const int16_t*, const int16_t*, int, unsigned, unsigned, unsigned,
                            unsigned, int, int, const float*, const float*, int, void* d_out)
{
    return note("zjint_crop_tensor_frame", d_out);
}
int zjint_crops_tensor_mixed_host(zj_ctx*, const zj_frame_desc*, size_t nframes, const int16_t* const*, const int16_t* const*,
                                  const int16_t* const*, const unsigned*, unsigned, unsigned, int, int, const float*, const float*,
                                  const uint8_t*, void* d_out)
{
    return mixed("zjint_crops_tensor_mixed_host", d_out, nframes);
}
}
