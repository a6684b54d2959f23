/* tests/abi/c_abi_refit.c -- an in-place geometry edit through the C ABI alone, from a C
 * (not C++) translation unit: include/pnrt.h compiled as C, linked against libpnrt.so.
 * TEST INFRASTRUCTURE: built in-tree by pnraytracing_amd/build.py, checked against the
 * Python path's bytes by tests/test_gpu_refit_c_abi.py.
 *
 * usage: c_abi_refit <scene.bin> <edit.bin> <out.bin>
 * scene.bin: the "PND1" file of scenes.export_pnd1 (see tests/abi/c_abi_dloop.cpp), a
 *   scene without environment and textures.
 * edit.bin: int32 first, count, with_lights; float lights_sum_area; count x 15 floats;
 *   with_lights: the scene's n_lights x 3 floats.
 * Uploads, edits, reads the boxes back, renders frames 0 and 1; writes the n_nodes x 12
 * node floats, then the width x height x 4 image floats. */
#include "pnrt.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s scene.bin edit.bin out.bin\n", argv[0]); return 2; }
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
    const int width[5] = {15, 18, 6, 12, 3};
    float* a[5];
    for (int k = 0; k < 5; ++k) {
        const size_t bytes = (size_t)n[k] * width[k] * 4;
        a[k] = (float*)malloc(bytes ? bytes : 4);
        if (!a[k] || !rd(f, a[k], bytes)) { fprintf(stderr, "short scene file\n"); return 2; }
    }
    fclose(f);
    if (fr[3] || fr[4] || fr[5]) { fprintf(stderr, "a scene without environment and textures, please\n"); return 2; }

    FILE* ef = fopen(argv[2], "rb");
    if (!ef) { perror(argv[2]); return 2; }
    int32_t ed[3];
    float new_sum = 0.f;
    if (!rd(ef, ed, sizeof ed) || !rd(ef, &new_sum, 4) || ed[1] < 0) { fprintf(stderr, "bad edit file\n"); return 2; }
    float* rec = (float*)malloc(ed[1] ? (size_t)ed[1] * 60 : 4);
    float* lights = (float*)malloc(n[4] ? (size_t)n[4] * 12 : 4);
    if (!rec || !lights || !rd(ef, rec, (size_t)ed[1] * 60) || (ed[2] && !rd(ef, lights, (size_t)n[4] * 12))) {
        fprintf(stderr, "short edit file\n");
        return 2;
    }
    fclose(ef);

    pnrt_ctx* rt = NULL;
    if (pnrt_create(0, &rt) != PNRT_OK) { fprintf(stderr, "pnrt_create failed: no MI355X\n"); return 3; }
    /* out of order: no scene yet -- a code and a message, nothing exits */
    if (pnrt_update_vertices(rt, ed[0], ed[1], rec, NULL, 0.f) != PNRT_E_STATE ||
        pnrt_read_bvh_boxes(rt, a[3], n[3]) != PNRT_E_STATE) {
        fprintf(stderr, "an edit before upload_scene was not refused\n");
        return 4;
    }
    printf("expected error: %s\n", pnrt_last_error(rt));
    pnrt_camera cam;
    memcpy(cam.eye, cam12, 12); memcpy(cam.lower_left, cam12 + 3, 12);
    memcpy(cam.horizontal, cam12 + 6, 12); memcpy(cam.vertical, cam12 + 9, 12);
    int rc = pnrt_upload_scene(rt, a[0], n[0], a[1], n[1], a[2], n[2], a[3], n[3], n[4] ? a[4] : NULL, n[4], sum_area);
    if (rc == PNRT_OK) rc = pnrt_set_frame(rt, fr[0], fr[1], &cam, fr[2]);
    if (rc != PNRT_OK) { fprintf(stderr, "setup: %s\n", pnrt_last_error(rt)); return 5; }
    if (pnrt_update_vertices(rt, n[0] - ed[1] + 1, ed[1], rec, NULL, 0.f) != PNRT_E_ARG) {
        fprintf(stderr, "a range past the vertex array was not refused\n");
        return 4;
    }

    rc = pnrt_update_vertices(rt, ed[0], ed[1], rec, ed[2] ? lights : NULL, new_sum);
    if (rc == PNRT_OK) rc = pnrt_read_bvh_boxes(rt, a[3], n[3]);
    if (rc == PNRT_OK) rc = pnrt_reset_accum(rt);
    if (rc == PNRT_OK) rc = pnrt_render(rt, 0, 2, 1, 1, 0);
    const size_t pix = (size_t)fr[0] * fr[1];
    float* img = (float*)malloc(pix * 16);
    if (!img) return 2;
    if (rc == PNRT_OK) rc = pnrt_read_accum(rt, img);
    if (rc != PNRT_OK) { fprintf(stderr, "edit: %s\n", pnrt_last_error(rt)); return 8; }
    FILE* o = fopen(argv[3], "wb");
    if (!o || fwrite(a[3], 48, (size_t)n[3], o) != (size_t)n[3] || fwrite(img, 16, pix, o) != pix) { perror(argv[3]); return 10; }
    fclose(o);
    printf("%d vertices from %d edited, root box (%g %g %g) .. (%g %g %g)\n", ed[1], ed[0], a[3][0], a[3][1], a[3][2], a[3][3],
           a[3][4], a[3][5]);
    pnrt_destroy(rt);
    for (int k = 0; k < 5; ++k) free(a[k]);
    free(rec); free(lights); free(img);
    return 0;
}
