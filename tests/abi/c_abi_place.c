/* tests/abi/c_abi_place.c -- a model defined and moved by a matrix through the C ABI alone,
 * from a C (not C++) translation unit: include/pnrt.h compiled as C, linked against
 * libpnrt.so.  TEST INFRASTRUCTURE: built in-tree by pnraytracing_amd/build.py, checked
 * against the Python path by tests/test_gpu_place_c_abi.py.
 *
 * usage: c_abi_place <scene.bin> <place.bin>
 * scene.bin: the "PND1" file of scenes.export_pnd1 (see tests/abi/c_abi_dloop.cpp), a
 *   scene without environment and textures.
 * place.bin: int32 first, count, relight; 16 floats, the matrix (column major); count x 8
 *   floats, the model-space records.
 * Uploads, defines the model, places it, reads the model's vertices back and prints the
 * 64-bit FNV-1a hash of their bytes. */
#include "pnrt.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s scene.bin place.bin\n", argv[0]); return 2; }
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

    FILE* pf = fopen(argv[2], "rb");
    if (!pf) { perror(argv[2]); return 2; }
    int32_t hd[3];
    pnrt_placement pl;
    memset(&pl, 0, sizeof pl);
    if (!rd(pf, hd, sizeof hd) || !rd(pf, pl.matrix, sizeof pl.matrix) || hd[1] < 1) { fprintf(stderr, "bad placement file\n"); return 2; }
    float* model = (float*)malloc((size_t)hd[1] * 32);
    float* got = (float*)malloc((size_t)hd[1] * 32);
    if (!model || !got || !rd(pf, model, (size_t)hd[1] * 32)) { fprintf(stderr, "short placement file\n"); return 2; }
    fclose(pf);

    pnrt_ctx* rt = NULL;
    if (pnrt_create(0, &rt) != PNRT_OK) { fprintf(stderr, "pnrt_create failed: no MI355X\n"); return 3; }
    int id = -1;
    /* out of order: no scene yet -- a code and a message, nothing exits */
    if (pnrt_define_model(rt, hd[0], hd[1], model, &id) != PNRT_E_STATE || pnrt_place_models(rt, &pl, 1, 0) != PNRT_E_STATE ||
        pnrt_read_vertices(rt, hd[0], hd[1], got) != PNRT_E_STATE) {
        fprintf(stderr, "a call before upload_scene was not refused\n");
        return 4;
    }
    printf("expected error: %s\n", pnrt_last_error(rt));
    int rc = pnrt_upload_scene(rt, a[0], n[0], a[1], n[1], a[2], n[2], a[3], n[3], n[4] ? a[4] : NULL, n[4], sum_area);
    if (rc != PNRT_OK) { fprintf(stderr, "setup: %s\n", pnrt_last_error(rt)); return 5; }
    if (pnrt_place_models(rt, &pl, 1, 0) != PNRT_E_ARG) { fprintf(stderr, "an undefined model was not refused\n"); return 4; }
    printf("expected error: %s\n", pnrt_last_error(rt));

    rc = pnrt_define_model(rt, hd[0], hd[1], model, &id);
    pl.model = id;
    if (rc == PNRT_OK) rc = pnrt_place_models(rt, &pl, 1, hd[2]);
    if (rc == PNRT_OK) rc = pnrt_read_vertices(rt, hd[0], hd[1], got);
    if (rc != PNRT_OK) { fprintf(stderr, "place: %s\n", pnrt_last_error(rt)); return 8; }
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char* b = (const unsigned char*)got;
    for (size_t i = 0; i < (size_t)hd[1] * 32; ++i) { h ^= b[i]; h *= 0x100000001b3ull; }
    printf("model %d: %d vertices from %d placed, sizeof(pnrt_placement) %d, hash %016llx\n", id, hd[1], hd[0],
           (int)sizeof(pnrt_placement), (unsigned long long)h);
    pnrt_destroy(rt);
    for (int k = 0; k < 5; ++k) free(a[k]);
    free(model); free(got);
    return 0;
}
