/* tests/abi/c_abi_reproject_view.c -- temporal reprojection under the camera models through
 * the C ABI alone, from a C (not C++) translation unit: include/pnrt.h compiled as C, linked
 * against libpnrt.so.  TEST INFRASTRUCTURE: built in-tree by pnraytracing_amd/build.py,
 * checked against the Python path's statistics and images by
 * tests/test_gpu_reproject_view_c_abi.py.
 *
 * usage: c_abi_reproject_view <scene.bin> <threshold> <from model> <to model> <fov_deg>
 *                             <position_tolerance> <out.bin> <12 floats: the camera to move to>
 * scene.bin: the "PND1" file of scenes.export_pnd1 (see tests/abi/c_abi_dloop.cpp).
 * Renders frames 0, 1 and adaptive calls of frames 3, 7, 15 (threshold, min_frames 2) at
 * the file's camera, then reprojects from the view of <from model> at that camera into the
 * view of <to model> at the given one.  Prints the statistics and writes the accumulation,
 * then the moments image (width * height * 4 floats each). */
#include "pnrt.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

_Static_assert(sizeof(pnrt_reproject_params) == 16, "pnrt_reproject_params is 16 bytes");
_Static_assert(sizeof(pnrt_reproject_stats) == 48, "pnrt_reproject_stats is 48 bytes");
_Static_assert(sizeof(pnrt_ray_camera) == 76, "pnrt_ray_camera is 76 bytes");

static int rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 20) {
        fprintf(stderr, "usage: %s scene.bin threshold from_model to_model fov_deg position_tolerance out.bin cam[12]\n", argv[0]);
        return 2;
    }
    const float threshold = strtof(argv[2], NULL);
    pnrt_ray_camera from, to;
    memset(&from, 0, sizeof from);
    memset(&to, 0, sizeof to);
    from.model = atoi(argv[3]);
    to.model = atoi(argv[4]);
    from.fov_deg = to.fov_deg = strtof(argv[5], NULL);
    pnrt_reproject_params rp = {0.9f, 0.02f, 32u, 0u};
    rp.position_tolerance = strtof(argv[6], NULL);
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
    memcpy(from.camera.eye, cam12, 12);
    memcpy(from.camera.lower_left, cam12 + 3, 12);
    memcpy(from.camera.horizontal, cam12 + 6, 12);
    memcpy(from.camera.vertical, cam12 + 9, 12);
    float* t12[4] = {to.camera.eye, to.camera.lower_left, to.camera.horizontal, to.camera.vertical};
    for (int k = 0; k < 12; ++k) t12[k / 3][k % 3] = strtof(argv[8 + k], NULL);
    if (rc == PNRT_OK) rc = pnrt_set_frame(rt, W, H, &from.camera, depth);
    if (rc != PNRT_OK) { fprintf(stderr, "setup: %s\n", pnrt_last_error(rt)); return 5; }
    /* out of order: the moments were never enabled -- a code and a message, nothing exits */
    if (pnrt_reproject_view(rt, &from, &to, NULL, NULL) != PNRT_E_STATE) { fprintf(stderr, "reproject_view without moments was not refused\n"); return 4; }
    printf("expected error: %s\n", pnrt_last_error(rt));
    rc = pnrt_enable_moments(rt, 1);
    /* a bad view: the message names which of the two */
    pnrt_ray_camera bad = to;
    bad.per_pixel = 2;
    if (rc == PNRT_OK && pnrt_reproject_view(rt, &from, &bad, &rp, NULL) != PNRT_E_ARG) { fprintf(stderr, "per_pixel 2 was not refused\n"); return 4; }
    printf("expected error: %s\n", pnrt_last_error(rt));
    if (rc == PNRT_OK && pnrt_reproject_view(rt, NULL, &to, &rp, NULL) != PNRT_E_ARG) { fprintf(stderr, "a NULL view was not refused\n"); return 4; }

    if (rc == PNRT_OK) rc = pnrt_render(rt, 0, 2, 1, 1, 0);
    const uint32_t frames[3] = {3, 7, 15};
    for (int k = 0; k < 3 && rc == PNRT_OK; ++k) rc = pnrt_render_adaptive(rt, frames[k], 1, threshold, 2, 1, 1, 0, NULL);
    pnrt_reproject_stats st;
    if (rc == PNRT_OK) rc = pnrt_reproject_view(rt, &from, &to, &rp, &st);
    if (rc != PNRT_OK) { fprintf(stderr, "render / reproject_view: %s\n", pnrt_last_error(rt)); return 8; }
    printf("stats %lld %lld %lld %lld %lld %u\n", (long long)st.n_pixels, (long long)st.n_reprojected, (long long)st.n_disoccluded,
           (long long)st.n_missed, (long long)st.sum_frames, (unsigned)st.max_frames);
    /* the guide images are the new view's: the preview needs no further call */
    if ((rc = pnrt_denoise(rt, NULL)) != PNRT_OK) { fprintf(stderr, "denoise: %s\n", pnrt_last_error(rt)); return 8; }
    const size_t count = (size_t)W * H * 4;
    float* acc = (float*)malloc(count * 4);
    float* mom = (float*)malloc(count * 4);
    if (!acc || !mom) return 9;
    if ((rc = pnrt_read_accum(rt, acc)) || (rc = pnrt_read_moments(rt, mom))) {
        fprintf(stderr, "read: %s\n", pnrt_last_error(rt));
        return 9;
    }
    FILE* o = fopen(argv[7], "wb");
    if (!o || fwrite(acc, 4, count, o) != count || fwrite(mom, 4, count, o) != count) { perror(argv[7]); return 10; }
    fclose(o);
    pnrt_destroy(rt);
    for (int k = 0; k < 5; ++k) free(a[k]);
    free(env); free(table); free(acc); free(mom);
    return 0;
}
