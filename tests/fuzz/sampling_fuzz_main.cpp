// sampling_fuzz_main.cpp -- a stand-alone program that feeds damaged three-component JPEG files of odd samplings to the
// front-end (zune-jpeg_amd/csrc/zj_jpeg.cpp with ZJ_FLAG_ANY_SAMPLING).  TEST ONLY: tests/test_sampling_fuzz.py
// builds it with zj_jpeg.cpp and tests/fuzz/jpeg_stubs.cpp under AddressSanitizer + UBSan and runs it on the files it wrote.
//
//   sampling_fuzz_main ITERATIONS SEED FILE...
// Every iteration takes one file and damages it in one of these ways, all from a seeded generator: 1-4 bit flips anywhere; a
// truncation; the sampling bytes and ids of the frame header rewritten (to another pair of factors 1, 2, 4 or to anything);
// the length field of the Adobe APP14 segment set to a random value; the component list of an SOS segment rewritten; a few
// bytes overwritten by a random marker.  The damaged file is decoded with the flag set (every third one through
// zj_decoder_prepare with the device entropy option, which must leave a non-standard file to the CPU walk), and the planes it
// yields are read whole, each checked against the size its sampling gives.  Any status is fine; what counts is that the
// sanitizers stay silent.  Exit status 0 and the line "sampling-fuzz-clean" on success.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/zjhip.h"

static uint64_t g_state = 1;
static uint32_t rnd()
{   // xorshift64*
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}
static size_t below(size_t n) { return n ? rnd() % n : 0; }

static long find_marker(const std::vector<uint8_t>& f, uint8_t m, size_t from)
{
    for (size_t i = from; i + 1 < f.size(); i++)
        if (f[i] == 0xFF && f[i + 1] == m) return (long)i;
    return -1;
}

static void damage(std::vector<uint8_t>& f)
{
    switch (rnd() % 8) {
    case 6: case 7: {
        long at = find_marker(f, 0xC0, 0);
        if (at < 0) at = find_marker(f, 0xC2, 0);
        if (at >= 0 && (size_t)at + 19 <= f.size()) {
            static const uint8_t hv[] = {0x11, 0x21, 0x12, 0x22, 0x41, 0x14, 0x42, 0x24, 0x44};
            for (int c = 0; c < 3; c++) {
                if (rnd() % 3) f[at + 11 + 3 * c] = rnd() % 8 ? hv[rnd() % sizeof hv] : (uint8_t)rnd();
                if (rnd() % 4 == 0) f[at + 10 + 3 * c] = (uint8_t)rnd();
            }
            if (rnd() % 8 == 0) { f[at + 7] = (uint8_t)rnd(); f[at + 8] = (uint8_t)(1 + rnd() % 200); } // (the width)
        } else f[below(f.size())] ^= 0x40;
        break;
    }
    case 0: case 1:
        for (unsigned k = 0, n = 1 + rnd() % 4; k < n; k++) f[below(f.size())] ^= (uint8_t)(1u << (rnd() % 8));
        break;
    case 2:
        f.resize(2 + below(f.size() - 2));
        break;
    case 3: {
        const long at = find_marker(f, 0xEE, 0);
        if (at >= 0 && (size_t)at + 3 < f.size()) { f[at + 2] = (uint8_t)(rnd() % 3 ? 0 : rnd()); f[at + 3] = (uint8_t)rnd(); }
        else f[below(f.size())] ^= 0x80;
        break;
    }
    case 4: {
        long at = find_marker(f, 0xDA, 0);
        for (unsigned skip = rnd() % 6; skip && at >= 0; skip--) { const long nx = find_marker(f, 0xDA, (size_t)at + 2); if (nx < 0) break; at = nx; }
        if (at >= 0 && (size_t)at + 4 < f.size()) {
            if (rnd() & 1) f[at + 4] = (uint8_t)(1 + rnd() % 4); // Ns, whatever the segment's length says
            else for (size_t i = (size_t)at + 5; i < f.size() && i < (size_t)at + 13; i++) if (rnd() & 1) f[i] = (uint8_t)rnd();
        }
        break;
    }
    default: {
        const size_t at = below(f.size() - 1);
        static const uint8_t ms[] = {0xC0, 0xC2, 0xC4, 0xDA, 0xDB, 0xDD, 0xEE, 0xD0, 0xD9, 0xE1};
        f[at] = 0xFF; f[at + 1] = ms[rnd() % sizeof ms];
        break;
    }
    }
}

int main(int argc, char** argv)
{
    if (argc < 4) { fprintf(stderr, "usage: %s ITERATIONS SEED FILE...\n", argv[0]); return 2; }
    const long iters = atol(argv[1]);
    g_state = (uint64_t)atoll(argv[2]) * 2654435761ull + 1;
    std::vector<std::vector<uint8_t>> files;
    for (int i = 3; i < argc; i++) {
        FILE* fp = fopen(argv[i], "rb");
        if (!fp) { fprintf(stderr, "cannot read %s\n", argv[i]); return 2; }
        std::vector<uint8_t> b;
        uint8_t buf[4096];
        for (size_t n; (n = fread(buf, 1, sizeof buf, fp)) > 0;) b.insert(b.end(), buf, buf + n);
        fclose(fp);
        if (b.size() < 4) { fprintf(stderr, "%s is no JPEG file\n", argv[i]); return 2; }
        files.push_back(b);
    }
    long ok = 0, odd = 0, whole = 0;
    long long sum = 0;
    for (long it = 0; it < iters; it++) {
        const bool first_pass = it < (long)files.size(); // (the first pass: every file in turn, as it is)
        std::vector<uint8_t> f = files[first_pass ? (size_t)it : below(files.size())];
        if (!first_pass) damage(f);
        zj_options o;
        memset(&o, 0, sizeof o);
        o.out_colorspace = ZJ_CS_RGB;
        o.num_threads = 1 + (int)(rnd() % 4);
        o.flags = ZJ_FLAG_ANY_SAMPLING | (rnd() & 1 ? ZJ_FLAG_FULL_AC_VALUES : 0u) | (rnd() % 4 == 0 ? ZJ_FLAG_CMYK_TO_RGB : 0u);
        o.entropy = it % 3 == 2 ? ZJ_ENTROPY_GPU_ALWAYS : ZJ_ENTROPY_CPU;
        zj_decoder* d = zj_decoder_new(&o);
        if (!d) return 3;
        // an exact-size copy: a read past the end of the file is a read past the end of the allocation
        uint8_t* buf = (uint8_t*)malloc(f.size());
        memcpy(buf, f.data(), f.size());
        zj_image_info info;
        zj_frame_desc fd;
        memset(&info, 0, sizeof info);
        int rc = zj_decoder_read_headers(d, buf, f.size(), &info);
        if (rc == ZJ_OK)
            rc = o.entropy ? zj_decoder_prepare(d, buf, f.size(), &fd, &info) : zj_decoder_decode_coefficients(d, buf, f.size(), &fd, nullptr, nullptr, &info);
        if (rc == ZJ_OK) {
            ok++;
            whole += first_pass;
            (void)zj_decoder_adobe_transform(d);
            const bool stored = zj_decoder_stored_rgb(d) != 0;
            bool own_layout = info.components == 3;
            for (int c = 0; c < 5; c++) {
                const int16_t* p = nullptr;
                size_t len = 0;
                unsigned bw = 0, bh = 0, ch = 0, cv = 0;
                if (zj_decoder_plane(d, c, &p, &len, &bw, &bh) != ZJ_OK) continue;
                if (len != (size_t)bw * bh * 64) { fprintf(stderr, "plane %d: %zu elements for %u x %u blocks\n", c, len, bw, bh); return 4; }
                if (zj_decoder_component_sampling(d, c, &ch, &cv) != ZJ_OK || !ch || !cv) { fprintf(stderr, "plane %d has no sampling\n", c); return 4; }
                const unsigned cw = (info.width * ch + info.h_max - 1) / info.h_max, chh = (info.height * cv + info.v_max - 1) / info.v_max;
                own_layout = own_layout && bw == (cw + 7) / 8 && bh == (chh + 7) / 8;
                for (size_t i = 0; i < len; i++) sum += p[i];
            }
            // (a file outside the known modes, or stored RGB, must have come out in the layout of its own sizes)
            if (info.components == 3 && (info.h_max > 2 || info.v_max > 2 || stored) && !own_layout) { fprintf(stderr, "a non-standard file in the MCU layout\n"); return 7; }
            odd += info.components == 3 && (info.h_max > 2 || info.v_max > 2 || stored);
        } else if (!zj_decoder_error(d)[0]) {
            fprintf(stderr, "status %d without a text\n", rc);
            return 5;
        }
        free(buf);
        zj_decoder_free(d);
    }
    if (iters >= (long)files.size() && whole < (long)files.size()) { fprintf(stderr, "the undamaged files did not all decode (%ld of %zu)\n", whole, files.size()); return 6; }
    printf("sampling-fuzz-clean %ld iterations, %ld decoded (%ld with a ratio of 4 or stored RGB), checksum %lld\n", iters, ok, odd, sum);
    return 0;
}
