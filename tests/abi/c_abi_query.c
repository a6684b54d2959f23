/* tests/abi/c_abi_query.c -- ray queries through the C ABI alone, from a C (not C++)
 * translation unit: include/pnrt.h compiled as C, linked against libpnrt.so.  TEST
 * INFRASTRUCTURE: built in-tree by pnraytracing_amd/build.py, checked against the Python
 * path's records by tests/test_gpu_query_c_abi.py.
 *
 * usage: c_abi_query <scene.bin> <rays.bin> <out.bin>
 * scene.bin: the "PND1" file of scenes.export_pnd1 (see tests/abi/c_abi_dloop.cpp).
 * rays.bin: n x 7 floats (origin, direction, tMax); n is the file's size / 28.
 * Writes the n 64-byte records of the closest-hit query, then those of the any-hit one.
 * No pnrt_set_frame: a query needs the scene only. */
#include "pnrt.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

_Static_assert(sizeof(pnrt_hit) == 64, "pnrt_hit is 64 bytes");

static int rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s scene.bin rays.bin out.bin\n", argv[0]); return 2; }
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
    fclose(f);                       /* (the environment and the textures do not matter to a query) */

    FILE* rf = fopen(argv[2], "rb");
    if (!rf) { perror(argv[2]); return 2; }
    fseek(rf, 0, SEEK_END);
    const long rbytes = ftell(rf);
    fseek(rf, 0, SEEK_SET);
    if (rbytes < 0 || rbytes % 28) { fprintf(stderr, "rays.bin is not n x 7 floats\n"); return 2; }
    const int64_t nr = rbytes / 28;
    float* rays = (float*)malloc(rbytes ? (size_t)rbytes : 4);
    pnrt_hit* hits = (pnrt_hit*)malloc(nr ? (size_t)nr * 2 * sizeof(pnrt_hit) : 4);
    if (!rays || !hits || !rd(rf, rays, (size_t)rbytes)) { fprintf(stderr, "short ray file\n"); return 2; }
    fclose(rf);

    pnrt_ctx* rt = NULL;
    if (pnrt_create(0, &rt) != PNRT_OK) { fprintf(stderr, "pnrt_create failed: no MI355X\n"); return 3; }
    /* out of order: no scene yet -- a code and a message, nothing exits */
    if (pnrt_query_rays(rt, rays, nr, PNRT_QUERY_CLOSEST, hits) != PNRT_E_STATE) {
        fprintf(stderr, "a query before upload_scene was not refused\n");
        return 4;
    }
    printf("expected error: %s\n", pnrt_last_error(rt));
    int rc = pnrt_upload_scene(rt, a[0], n[0], a[1], n[1], a[2], n[2], a[3], n[3], n[4] ? a[4] : NULL, n[4], sum_area);
    if (rc != PNRT_OK) { fprintf(stderr, "setup: %s\n", pnrt_last_error(rt)); return 5; }
    if (pnrt_query_rays(rt, rays, nr, 2, hits) != PNRT_E_ARG) { fprintf(stderr, "kind 2 was not refused\n"); return 4; }

    rc = pnrt_query_rays(rt, rays, nr, PNRT_QUERY_CLOSEST, hits);
    if (rc == PNRT_OK) rc = pnrt_query_rays(rt, rays, nr, PNRT_QUERY_ANY, hits + nr);
    if (rc != PNRT_OK) { fprintf(stderr, "query: %s\n", pnrt_last_error(rt)); return 8; }
    FILE* o = fopen(argv[3], "wb");
    if (!o || fwrite(hits, sizeof(pnrt_hit), (size_t)nr * 2, o) != (size_t)nr * 2) { perror(argv[3]); return 10; }
    fclose(o);
    int64_t closest = 0, any = 0;
    for (int64_t i = 0; i < nr; ++i) { closest += hits[i].w[0]; any += hits[nr + i].w[0]; }
    printf("%lld rays: %lld closest hits, %lld occluded\n", (long long)nr, (long long)closest, (long long)any);
    pnrt_destroy(rt);
    for (int k = 0; k < 5; ++k) free(a[k]);
    free(rays); free(hits);
    return 0;
}
