/* tests/abi/c_abi_denoise_variance.c -- the variance-guided denoised preview through
 * the C ABI alone, from a C (not C++) translation unit: include/pnrt.h compiled as
 * C, linked against libpnrt.so.  TEST INFRASTRUCTURE: built in-tree by
 * pnraytracing_amd/build.py, checked against the Python path's image by
 * tests/test_gpu_denoise_variance_c_abi.py.
 *
 * usage: c_abi_denoise_variance <scene.bin> <frames> <levels> <sigma_variance> <sigma_normal> <sigma_position> <out.bin>
 * scene.bin: the "PND1" file of scenes.export_pnd1 (see tests/abi/c_abi_dloop.cpp).
 * levels 0: pnrt_denoise_variance(ctx, NULL).  Writes the denoised image, then the
 * moments image (width * height * 4 floats each). */
#include "pnrt.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 8) { fprintf(stderr, "usage: %s scene.bin frames levels sv sn sp out.bin\n", argv[0]); return 2; }
    const int frames = atoi(argv[2]);
    pnrt_denoise_variance_params dp;
    dp.levels = atoi(argv[3]);
    dp.sigma_variance = strtof(argv[4], NULL);
    dp.sigma_normal = strtof(argv[5], NULL);
    dp.sigma_position = strtof(argv[6], NULL);
    if (sizeof dp != 16) { fprintf(stderr, "pnrt_denoise_variance_params is %d bytes\n", (int)sizeof dp); return 2; }
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
    if (rc == PNRT_OK) rc = pnrt_render_guides(rt);
    if (rc != PNRT_OK) { fprintf(stderr, "setup: %s\n", pnrt_last_error(rt)); return 5; }
    /* out of order: the moments were never enabled -- a code and a message, nothing exits */
    if (pnrt_denoise_variance(rt, NULL) != PNRT_E_STATE) { fprintf(stderr, "denoise_variance without moments was not refused\n"); return 4; }
    printf("expected error: %s\n", pnrt_last_error(rt));
    if (pnrt_denoised_device_ptr(rt) != NULL) { fprintf(stderr, "the denoised image was allocated by a refused call\n"); return 4; }
    /* a bad parameter */
    pnrt_denoise_variance_params bad = {6, 4.0f, 0.25f, 0.5f};
    if (pnrt_denoise_variance(rt, &bad) != PNRT_E_ARG) { fprintf(stderr, "levels 6 was not refused\n"); return 4; }

    rc = pnrt_enable_moments(rt, 1);
    /* one dispatch per frame; then the preview, without waiting in between */
    for (int k = 0; k < frames && rc == PNRT_OK; ++k) rc = pnrt_render(rt, (uint32_t)k, 1, 1, 1, 0);
    if (rc == PNRT_OK) rc = pnrt_denoise_variance(rt, dp.levels ? &dp : NULL);
    if (rc != PNRT_OK) { fprintf(stderr, "render / denoise_variance: %s\n", pnrt_last_error(rt)); return 8; }
    const size_t count = (size_t)W * H * 4;
    float* den = (float*)malloc(count * 4);
    float* mom = (float*)malloc(count * 4);
    if (!den || !mom) return 9;
    if ((rc = pnrt_read_denoised(rt, den)) || (rc = pnrt_read_moments(rt, mom))) {
        fprintf(stderr, "read: %s\n", pnrt_last_error(rt));
        return 9;
    }
    FILE* o = fopen(argv[7], "wb");
    if (!o || fwrite(den, 4, count, o) != count || fwrite(mom, 4, count, o) != count) { perror(argv[7]); return 10; }
    fclose(o);
    printf("denoised %dx%d after %d frames, levels %d\n", W, H, frames, dp.levels);
    pnrt_destroy(rt);
    for (int k = 0; k < 5; ++k) free(a[k]);
    free(env); free(table); free(den); free(mom);
    return 0;
}
