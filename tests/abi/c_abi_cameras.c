/* tests/abi/c_abi_cameras.c -- per-frame cameras through the C ABI alone, from a C (not
 * C++) translation unit: include/pnrt.h and include/pnrt_host.h compiled as C, linked
 * against libpnrt.so and libpnrt_host.so.
 * TEST INFRASTRUCTURE: built in-tree by pnraytracing_amd/build.py, checked against the
 * Python path's image by tests/test_gpu_cameras.py.
 *
 * usage: c_abi_cameras <scene.bin> <first_frame> <n_frames> <aa_width> <lens_radius> <focus_distance> <out.bin>
 * scene.bin: the "PND1" file of scenes.export_pnd1 (see tests/abi/c_abi_dloop.cpp).
 * Makes the frames' cameras with pnrt_camera_sequence around the file's camera, renders
 * them with one pnrt_render_cameras call, overwrites the array at once, and writes the
 * accumulation (width * height * 4 floats). */
#include "pnrt.h"
#include "pnrt_host.h"

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

_Static_assert(sizeof(pnrt_lens_params) == 16, "pnrt_lens_params is 16 bytes");
_Static_assert(sizeof(pnrt_camera) == 48, "pnrt_camera is twelve floats: pnrt_camera_sequence's records are pnrt_render_cameras'");

static int rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 8) { fprintf(stderr, "usage: %s scene.bin first n aa_width lens_radius focus_distance out.bin\n", argv[0]); return 2; }
    const uint32_t first = (uint32_t)strtoul(argv[2], NULL, 10), nf = (uint32_t)strtoul(argv[3], NULL, 10);
    pnrt_lens_params lp = {strtof(argv[4], NULL), strtof(argv[5], NULL), strtof(argv[6], NULL), 0u};
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
    pnrt_camera* cams = (pnrt_camera*)malloc((size_t)(nf ? nf : 1) * sizeof(pnrt_camera));
    if (!cams) return 9;
    /* the sequence: a refusal first (a code and a message, nothing exits), then the frames' cameras */
    pnrt_lens_params bad = lp;
    bad.reserved = 1u;
    if (pnrt_camera_sequence(cam12, W, H, &bad, first, nf, (float*)cams) != PNRT_E_ARG) { fprintf(stderr, "reserved != 0 was not refused\n"); return 4; }
    printf("expected error: %s\n", pnrt_host_last_error());
    if (pnrt_camera_sequence(cam12, W, H, &lp, first, nf, (float*)cams) != 0) { fprintf(stderr, "camera_sequence: %s\n", pnrt_host_last_error()); return 5; }

    pnrt_ctx* rt = NULL;
    if (pnrt_create(0, &rt) != PNRT_OK) { fprintf(stderr, "pnrt_create failed: no MI355X\n"); return 3; }
    /* out of order: no scene yet */
    if (pnrt_render_cameras(rt, first, nf, cams, 1, 1, 0) != PNRT_E_STATE) { fprintf(stderr, "render_cameras before upload was not refused\n"); return 4; }
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
    pnrt_camera centre;
    memcpy(centre.eye, cam12, 12);
    memcpy(centre.lower_left, cam12 + 3, 12);
    memcpy(centre.horizontal, cam12 + 6, 12);
    memcpy(centre.vertical, cam12 + 9, 12);
    if (rc == PNRT_OK) rc = pnrt_set_frame(rt, W, H, &centre, depth);
    if (rc != PNRT_OK) { fprintf(stderr, "setup: %s\n", pnrt_last_error(rt)); return 5; }
    /* bad arguments: no array, a camera that is not finite */
    if (nf > 0 && pnrt_render_cameras(rt, first, nf, NULL, 1, 1, 0) != PNRT_E_ARG) { fprintf(stderr, "cameras == NULL was not refused\n"); return 4; }
    if (nf > 0) {
        const float keep = cams[nf - 1].vertical[2];
        cams[nf - 1].vertical[2] = NAN;
        if (pnrt_render_cameras(rt, first, nf, cams, 1, 1, 0) != PNRT_E_ARG) { fprintf(stderr, "a NaN camera was not refused\n"); return 4; }
        printf("expected error: %s\n", pnrt_last_error(rt));
        cams[nf - 1].vertical[2] = keep;
    }
    uint32_t fpb = 0, nb = 0;
    int64_t bytes = 0, bytes_plain = 0;
    if ((rc = pnrt_cameras_batch_plan(rt, nf, 1, 1, 0, &fpb, &nb, &bytes)) || (rc = pnrt_batch_plan(rt, nf, 1, 1, 0, NULL, NULL, &bytes_plain))) {
        fprintf(stderr, "batch plan: %s\n", pnrt_last_error(rt));
        return 8;
    }
    printf("plan %u %u %lld %lld\n", (unsigned)fpb, (unsigned)nb, (long long)bytes, (long long)bytes_plain);
    rc = pnrt_render_cameras(rt, first, nf, cams, 1, 1, 0);
    memset(cams, 0xff, (size_t)(nf ? nf : 1) * sizeof(pnrt_camera));     /* the array is the caller's again */
    if (rc != PNRT_OK) { fprintf(stderr, "render_cameras: %s\n", pnrt_last_error(rt)); return 8; }
    const size_t count = (size_t)W * H * 4;
    float* acc = (float*)malloc(count * 4);
    if (!acc) return 9;
    if ((rc = pnrt_read_accum(rt, acc))) { fprintf(stderr, "read: %s\n", pnrt_last_error(rt)); return 9; }
    FILE* o = fopen(argv[7], "wb");
    if (!o || fwrite(acc, 4, count, o) != count) { perror(argv[7]); return 10; }
    fclose(o);
    pnrt_destroy(rt);
    for (int k = 0; k < 5; ++k) free(a[k]);
    free(env); free(table); free(acc); free(cams);
    return 0;
}
