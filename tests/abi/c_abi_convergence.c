/* tests/abi/c_abi_convergence.c -- the sample moments and the convergence statistics
 * through the C ABI alone, from a C (not C++) translation unit: include/pnrt.h
 * compiled as C, linked against libpnrt.so.  TEST INFRASTRUCTURE: built in-tree by
 * pnraytracing_amd/build.py, checked against the Python path's numbers by
 * tests/test_gpu_moments_c_abi.py.
 *
 * usage: c_abi_convergence <scene.bin> <frames> <threshold> <band_rows> <n_shards> <shard> <out.bin>
 * scene.bin: the "PND1" file of scenes.export_pnd1 (see tests/abi/c_abi_dloop.cpp).
 * Writes the moments image (width * height * 4 floats), then the 48 bytes of the
 * pnrt_convergence_stats record of the selector. */
#include "pnrt.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

_Static_assert(sizeof(pnrt_convergence_stats) == 48, "pnrt_convergence_stats is 48 bytes");

static int rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 8) { fprintf(stderr, "usage: %s scene.bin frames threshold band n_shards shard out.bin\n", argv[0]); return 2; }
    const int frames = atoi(argv[2]);
    const float threshold = strtof(argv[3], NULL);
    const int band = atoi(argv[4]), n_shards = atoi(argv[5]), shard = atoi(argv[6]);
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
    if (rc != PNRT_OK) { fprintf(stderr, "setup: %s\n", pnrt_last_error(rt)); return 5; }

    const size_t count = (size_t)W * H * 4;
    float* mom = (float*)malloc(count * 4);
    if (!mom) return 9;
    pnrt_convergence_stats st;
    /* out of order: never enabled -- a code and a message, nothing exits */
    if (pnrt_moments_device_ptr(rt) != NULL) { fprintf(stderr, "a moments image before it was asked for\n"); return 4; }
    if (pnrt_read_moments(rt, mom) != PNRT_E_STATE || pnrt_convergence(rt, threshold, 1, 1, 0, &st) != PNRT_E_STATE) {
        fprintf(stderr, "moments before enable were not refused\n");
        return 4;
    }
    printf("expected error: %s\n", pnrt_last_error(rt));
    if (pnrt_enable_moments(rt, 2) != PNRT_E_ARG) { fprintf(stderr, "enable_moments(2) was not refused\n"); return 4; }
    if ((rc = pnrt_enable_moments(rt, 1)) != PNRT_OK) { fprintf(stderr, "enable: %s\n", pnrt_last_error(rt)); return 6; }
    if (pnrt_convergence(rt, -1.0f, 1, 1, 0, &st) != PNRT_E_ARG) { fprintf(stderr, "a negative threshold was not refused\n"); return 4; }

    /* main.cpp:587-628: one dispatch per frame, without waiting in between */
    for (int k = 0; k < frames && rc == PNRT_OK; ++k) rc = pnrt_render(rt, (uint32_t)k, 1, 1, 1, 0);
    if (rc == PNRT_OK) rc = pnrt_convergence(rt, threshold, band, n_shards, shard, &st);
    if (rc == PNRT_OK) rc = pnrt_read_moments(rt, mom);
    if (rc != PNRT_OK) { fprintf(stderr, "render / convergence: %s\n", pnrt_last_error(rt)); return 8; }
    FILE* o = fopen(argv[7], "wb");
    if (!o || fwrite(mom, 4, count, o) != count || fwrite(&st, sizeof st, 1, o) != 1) { perror(argv[7]); return 10; }
    fclose(o);
    printf("%dx%d after %d frames: %lld of %lld measured pixels above %g, max %g, frames %u..%u\n", W, H, frames,
           (long long)st.n_above, (long long)st.n_measured, (double)threshold, (double)st.max_error, st.min_frames,
           st.max_frames);
    pnrt_destroy(rt);
    for (int k = 0; k < 5; ++k) free(a[k]);
    free(env); free(table); free(mom);
    return 0;
}
