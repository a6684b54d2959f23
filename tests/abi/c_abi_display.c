/* tests/abi/c_abi_display.c -- the display transform and auto exposure through the C ABI
 * alone, from a C (not C++) translation unit: include/pnrt.h compiled as C, linked
 * against libpnrt.so.  TEST INFRASTRUCTURE: built in-tree by pnraytracing_amd/build.py,
 * checked against tests/display_ref.py by tests/test_gpu_display_c_abi.py.
 *
 * usage: c_abi_display <scene.bin> <n_frames> <out.bin>
 * scene.bin: the "PND1" file of scenes.export_pnd1 (see tests/abi/c_abi_dloop.cpp).
 * Renders n_frames frames, takes the luminance histogram of the accumulation image,
 * derives the exposure (50, 950 permille, key 0.18), displays with ACES + sRGB and
 * writes the accumulation image (width * height * 4 floats), then the display image
 * (width * height * 4 bytes).  Prints the histogram's counts and the exposure's bits. */
#include "pnrt.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

_Static_assert(sizeof(pnrt_display_params) == 32, "pnrt_display_params is 32 bytes");
_Static_assert(sizeof(pnrt_luma_histogram) == 4112, "pnrt_luma_histogram is 4112 bytes");

static int rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s scene.bin n_frames out.bin\n", argv[0]); return 2; }
    const uint32_t n_frames = (uint32_t)strtoul(argv[2], NULL, 10);
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    char magic[4];
    int32_t n[5], fr[6];
    float sum_area = 0.f, cam12[12];
    if (!rd(f, magic, 4) || memcmp(magic, "PND1", 4) || !rd(f, n, sizeof n) || !rd(f, &sum_area, 4) ||
        !rd(f, fr, sizeof fr) || !rd(f, cam12, sizeof cam12)) {
        fprintf(stderr, "bad scene file\n");
        return 2;
    }
    const int W = fr[0], H = fr[1], depth = fr[2], ew = fr[3], eh = fr[4], ntex = fr[5];
    const int width[5] = {15, 18, 6, 12, 3};
    float* a[5];
    for (int k = 0; k < 5; ++k) {
        const size_t bytes = (size_t)n[k] * width[k] * 4;
        a[k] = (float*)malloc(bytes ? bytes : 4);
        if (!a[k] || !rd(f, a[k], bytes)) { fprintf(stderr, "short scene file\n"); return 2; }
    }
    float *env = NULL, *table = NULL;
    if (ew > 0) {
        const size_t bytes = (size_t)ew * eh * 3 * 4;
        env = (float*)malloc(bytes);
        table = (float*)malloc(bytes);
        if (!env || !table || !rd(f, env, bytes) || !rd(f, table, bytes)) { fprintf(stderr, "short env\n"); return 2; }
    }
    pnrt_ctx* rt = NULL;
    if (pnrt_create(0, &rt) != PNRT_OK) { fprintf(stderr, "pnrt_create failed: no MI355X\n"); return 3; }
    /* out of order: no frame yet -- a code and a message, nothing exits */
    if (pnrt_display(rt, NULL) != PNRT_E_STATE) { fprintf(stderr, "display before set_frame was not refused\n"); return 4; }
    printf("expected error: %s\n", pnrt_last_error(rt));
    if (pnrt_display_device_ptr(rt) != NULL) { fprintf(stderr, "a display image before the first display\n"); return 4; }
    int rc = pnrt_upload_scene(rt, a[0], n[0], a[1], n[1], a[2], n[2], a[3], n[3], n[4] ? a[4] : NULL, n[4], sum_area);
    for (int t = 0; rc == PNRT_OK && t < ntex; ++t) {
        int32_t th[3];
        if (!rd(f, th, sizeof th)) { fprintf(stderr, "short texture\n"); return 2; }
        const size_t bytes = (size_t)th[0] * th[1] * th[2];
        uint8_t* px = (uint8_t*)malloc(bytes);
        if (!px || !rd(f, px, bytes)) { fprintf(stderr, "short texture\n"); return 2; }
        rc = pnrt_upload_texture(rt, t, px, th[0], th[1], th[2]);
        free(px);
    }
    fclose(f);
    if (rc == PNRT_OK) rc = pnrt_upload_env(rt, env, table, ew, eh);
    pnrt_camera cam;
    memcpy(cam.eye, cam12, 12);
    memcpy(cam.lower_left, cam12 + 3, 12);
    memcpy(cam.horizontal, cam12 + 6, 12);
    memcpy(cam.vertical, cam12 + 9, 12);
    if (rc == PNRT_OK) rc = pnrt_set_frame(rt, W, H, &cam, depth);
    if (rc != PNRT_OK) { fprintf(stderr, "setup: %s\n", pnrt_last_error(rt)); return 5; }
    /* a bad parameter */
    pnrt_display_params bad = {PNRT_DISPLAY_ACCUM, 3, PNRT_TRANSFER_LINEAR, 0, 1.0f, 4.0f, NULL};
    if (pnrt_display(rt, &bad) != PNRT_E_ARG) { fprintf(stderr, "tone 3 was not refused\n"); return 4; }

    rc = pnrt_render(rt, 0, n_frames, 1, 1, 0);
    pnrt_luma_histogram hist;
    float exposure = 0.f;
    if (rc == PNRT_OK) rc = pnrt_luma_histogram_read(rt, PNRT_DISPLAY_ACCUM, NULL, 1, 1, 0, &hist);
    if (rc == PNRT_OK) rc = pnrt_exposure_from_histogram(&hist, 50, 950, 0.18f, &exposure);
    pnrt_display_params dp = {PNRT_DISPLAY_ACCUM, PNRT_TONE_ACES, PNRT_TRANSFER_SRGB, 0, 1.0f, 4.0f, NULL};
    dp.exposure = exposure;
    if (rc == PNRT_OK) rc = pnrt_display(rt, &dp);
    if (rc != PNRT_OK) { fprintf(stderr, "render / display: %s\n", pnrt_last_error(rt)); return 8; }
    uint32_t ebits;
    memcpy(&ebits, &exposure, 4);
    printf("hist %lld %lld exposure 0x%08X\n", (long long)hist.n_pixels, (long long)hist.n_counted, (unsigned)ebits);
    const size_t count = (size_t)W * H * 4;
    float* acc = (float*)malloc(count * 4);
    uint8_t* img = (uint8_t*)malloc(count);
    if (!acc || !img) return 9;
    if ((rc = pnrt_read_accum(rt, acc)) || (rc = pnrt_read_display(rt, img))) {
        fprintf(stderr, "read: %s\n", pnrt_last_error(rt));
        return 9;
    }
    FILE* o = fopen(argv[3], "wb");
    if (!o || fwrite(acc, 4, count, o) != count || fwrite(img, 1, count, o) != count) { perror(argv[3]); return 10; }
    fclose(o);
    pnrt_destroy(rt);
    for (int k = 0; k < 5; ++k) free(a[k]);
    free(env); free(table); free(acc); free(img);
    return 0;
}
