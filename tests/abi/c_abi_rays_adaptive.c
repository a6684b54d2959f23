/* tests/abi/c_abi_rays_adaptive.c -- adaptive sampling over caller ray buffers through the C
 * ABI alone, from a C (not C++) translation unit: include/pnrt.h compiled as C, linked against
 * libpnrt.so.  The device buffer comes from the HIP runtime, whose entry points used here are
 * declared by hand (hip_runtime_api.h is not a C11 header everywhere).
 * TEST INFRASTRUCTURE: built in-tree by pnraytracing_amd/build.py, checked against the
 * Python path's images by tests/test_gpu_rays_adaptive_c_abi.py.
 *
 * usage: c_abi_rays_adaptive <scene.bin> <n_frames> <model> <fov_deg> <aa_width> <threshold> <out.bin>
 * scene.bin: the "PND1" file of scenes.export_pnd1 (see tests/abi/c_abi_dloop.cpp).
 * Makes a set per frame for frames 0 .. 3 + n_frames with pnrt_make_rays around the file's
 * camera, renders frames 0 .. 3 with pnrt_render_rays (moments enabled), then frames
 * 4 .. 3 + n_frames with one pnrt_render_rays_adaptive call (min_frames 2), prints the call's
 * statistics and writes the accumulation and the moments (width * height * 4 floats each). */
#include "pnrt.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

_Static_assert(sizeof(pnrt_ray) == 32, "pnrt_ray is 32 bytes");
_Static_assert(sizeof(pnrt_adaptive_stats) == 40, "pnrt_adaptive_stats is 40 bytes");

extern int hipMalloc(void** ptr, size_t size);
extern int hipFree(void* ptr);

static int rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 8) { fprintf(stderr, "usage: %s scene.bin n model fov_deg aa_width threshold out.bin\n", argv[0]); return 2; }
    const uint32_t nf = (uint32_t)strtoul(argv[2], NULL, 10), total = 4u + nf;
    const float threshold = strtof(argv[6], NULL);
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
    pnrt_ray_camera rc_cam;
    memset(&rc_cam, 0, sizeof rc_cam);
    rc_cam.model = atoi(argv[3]);
    memcpy(rc_cam.camera.eye, cam12, 12);
    memcpy(rc_cam.camera.lower_left, cam12 + 3, 12);
    memcpy(rc_cam.camera.horizontal, cam12 + 6, 12);
    memcpy(rc_cam.camera.vertical, cam12 + 9, 12);
    rc_cam.fov_deg = strtof(argv[4], NULL);
    rc_cam.aa_width = strtof(argv[5], NULL);
    rc_cam.per_pixel = 1;

    pnrt_ctx* rt = NULL;
    if (pnrt_create(0, &rt) != PNRT_OK) { fprintf(stderr, "pnrt_create failed: no MI355X\n"); return 3; }
    const size_t pix = (size_t)W * H;
    const int64_t stride = (int64_t)pix + 3;             /* a gap of three records between the sets */
    void* rays = NULL;
    if (hipMalloc(&rays, ((size_t)(total - 1) * (size_t)stride + pix) * sizeof(pnrt_ray)) != 0) { fprintf(stderr, "hipMalloc failed\n"); return 9; }
    pnrt_adaptive_stats st;
    /* out of order: no scene, no frame yet */
    if (pnrt_render_rays_adaptive(rt, 4, nf, rays, stride, threshold, 2, 1, 1, 0, &st) != PNRT_E_STATE) { fprintf(stderr, "a call before upload was not refused\n"); return 4; }
    printf("expected error: %s\n", pnrt_last_error(rt));
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
    if (rc == PNRT_OK) rc = pnrt_set_frame(rt, W, H, &rc_cam.camera, depth);
    if (rc != PNRT_OK) { fprintf(stderr, "setup: %s\n", pnrt_last_error(rt)); return 5; }
    /* the moments are not enabled yet */
    if (pnrt_render_rays_adaptive(rt, 4, nf, rays, stride, threshold, 2, 1, 1, 0, &st) != PNRT_E_STATE) { fprintf(stderr, "a call without moments was not refused\n"); return 4; }
    printf("expected error: %s\n", pnrt_last_error(rt));
    if ((rc = pnrt_enable_moments(rt, 1))) { fprintf(stderr, "enable_moments: %s\n", pnrt_last_error(rt)); return 5; }
    if ((rc = pnrt_make_rays(rt, &rc_cam, 0, total, rays, stride))) { fprintf(stderr, "make_rays: %s\n", pnrt_last_error(rt)); return 8; }
    if ((rc = pnrt_render_rays(rt, 0, 4, rays, stride, 1, 1, 0))) { fprintf(stderr, "render_rays: %s\n", pnrt_last_error(rt)); return 8; }
    /* bad arguments: a misaligned buffer, a stride inside a set, a negative threshold */
    const pnrt_ray* later = (const pnrt_ray*)rays + 4 * stride;      /* frame 4's set */
    if (pnrt_render_rays_adaptive(rt, 4, nf, (const char*)later + 8, stride, threshold, 2, 1, 1, 0, &st) != PNRT_E_ARG) { fprintf(stderr, "a misaligned buffer was not refused\n"); return 4; }
    printf("expected error: %s\n", pnrt_last_error(rt));
    if (pix > 1 && pnrt_render_rays_adaptive(rt, 4, nf, later, (int64_t)pix - 1, threshold, 2, 1, 1, 0, &st) != PNRT_E_ARG) { fprintf(stderr, "a short stride was not refused\n"); return 4; }
    printf("expected error: %s\n", pnrt_last_error(rt));
    if (pnrt_render_rays_adaptive(rt, 4, nf, later, stride, -1.0f, 2, 1, 1, 0, &st) != PNRT_E_ARG) { fprintf(stderr, "a negative threshold was not refused\n"); return 4; }
    printf("expected error: %s\n", pnrt_last_error(rt));

    if ((rc = pnrt_render_rays_adaptive(rt, 4, nf, later, stride, threshold, 2, 1, 1, 0, &st))) { fprintf(stderr, "render_rays_adaptive: %s\n", pnrt_last_error(rt)); return 8; }
    printf("stats %lld %lld %lld %lld %u %u\n", (long long)st.n_pixels, (long long)st.n_active_pixels, (long long)st.n_tiles,
           (long long)st.n_active_tiles, st.frames_per_batch, st.n_batches);
    if ((rc = pnrt_render_rays_adaptive(rt, 4 + nf, 0, NULL, 0, threshold, 2, 1, 1, 0, NULL))) { fprintf(stderr, "n_frames == 0, out == NULL: %s\n", pnrt_last_error(rt)); return 8; }
    float* acc = (float*)malloc(pix * 16);
    float* mom = (float*)malloc(pix * 16);
    if (!acc || !mom) return 9;
    if ((rc = pnrt_read_accum(rt, acc)) || (rc = pnrt_read_moments(rt, mom))) { fprintf(stderr, "read: %s\n", pnrt_last_error(rt)); return 9; }
    FILE* o = fopen(argv[7], "wb");
    if (!o || fwrite(acc, 4, pix * 4, o) != pix * 4 || fwrite(mom, 4, pix * 4, o) != pix * 4) {
        perror(argv[7]);
        return 10;
    }
    fclose(o);
    pnrt_destroy(rt);
    hipFree(rays);
    for (int k = 0; k < 5; ++k) free(a[k]);
    free(env); free(table); free(acc); free(mom);
    return 0;
}
