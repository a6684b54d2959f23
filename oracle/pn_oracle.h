/*
 * oracle/pn_oracle.h -- TEST INFRASTRUCTURE.  CPU restatement of the radiance
 * integrator in PnRayTracing's shaders/ray_tracing.comp (the GLSL reference),
 * used ONLY as the parity checker (tests/, __graft_entry__.smoke()) and as
 * bench.py's cpu_baseline ("kind": "port").  The product path never loads it.
 *
 * Pinning status (see DESIGN.md "Oracle"):
 *   - RNG (wang_hash), Sobol, camera, host arrays: pinned by known answers
 *     computed from the reference's own sources (SURVEY 8c KATs, oracle/_ref).
 *   - Ray/triangle, slab and BVH traversal arithmetic: PINNED bit for bit to
 *     the reference's own CPU code (triangle.hpp, bound.hpp, BVH.hpp compiled
 *     here, oracle/ref/isect_driver.cpp) on ~3.4M seeded ray queries per
 *     scene over C1/C2/C4/C5, with the three documented rule differences
 *     (ties, slab clipping, glm::normalize) switched by pno_intersect's `sem`
 *     (tests/test_isect_pin.py).
 *   - The shading half (Disney BRDF and its sampling, light and environment
 *     sampling, MIS, the path loop, the order of the RNG draws) and the
 *     intersection code under the GLSL's own rules (sem 0): PINNED bit for bit
 *     to the shader's own text.  shaders/ray_tracing.comp is translated to C++
 *     by text surgery and compiled here (oracle/shader/, oracle/_ref/
 *     shader_driver); pno_shade_eval, pno_intersect and pno_render equal it
 *     word for word per function and per image (tests/test_shader_pin.py).
 *     What stays by definition is what the text does not carry: the built-ins
 *     (libm, vector forms, min/max, samplers), listed in DESIGN.md 7.
 *
 * Inputs are the reference's own flattened float arrays exactly as main.cpp
 * packs them (main.cpp:409-524): vertex 15 f, material 18 f, triangle 6 f,
 * BVH node 12 f, light 3 f; integers stored as floats.
 */
#ifndef PN_ORACLE_H
#define PN_ORACLE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PNO_MAX_TEXTURES 20

typedef struct {
    const float* vertices;   int n_vertices;    /* 15 floats / vertex  */
    const float* materials;  int n_materials;   /* 18 floats / material */
    const float* triangles;  int n_triangles;   /* 6 floats / triangle */
    const float* nodes;      int n_nodes;       /* 12 floats / node    */
    const float* lights;     int n_lights;      /* 3 floats / light    */
    float lights_sum_area;
    /* albedo textures (units 5..24): GL-unpacked rows, row stride
     * = align4(w*channels) bytes (GL_UNPACK_ALIGNMENT 4, main.cpp:545) */
    int n_textures;
    const uint8_t* tex_data[PNO_MAX_TEXTURES];
    int tex_w[PNO_MAX_TEXTURES], tex_h[PNO_MAX_TEXTURES], tex_ch[PNO_MAX_TEXTURES];
    /* environment (units 29/30, shader.hpp:126-225) */
    int has_hdr, hdr_w, hdr_h;
    const float* hdr_rgb;     /* w*h*3, row 0 = first row of the file */
    const float* random_hdr;  /* w*h*3 inverse-CDF table              */
} pno_scene;

typedef struct {
    float eye[3], lower_left[3], horizontal[3], vertical[3]; /* camera.hpp:28-30 */
    int width, height;          /* SCREEN_WIDTH / SCREEN_HEIGHT uniforms */
    int max_bounce_depth;       /* MAX_BOUNCE_DEPTH uniform (1..4)       */
} pno_frame;

/* Algorithmic-byte counters, summed over all samples. */
typedef struct {
    uint64_t samples;
    uint64_t node_pops, sibling_tests, tri_tests, tri_hits;
    uint64_t material_fetches, light_probes, light_samples, env_samples;
    uint64_t env_lookups, albedo_bytes, accum_rmw;
    uint64_t traversals;
    int stack_overflow;          /* set if any traversal needed > 128 entries */
    /* the camera-ray share of node_pops / sibling_tests / tri_tests / tri_hits
     * (the GPU traces the un-jittered camera ray once per pixel per call, the
     * bounce rays in its per-bounce traversal kernel) */
    uint64_t prim_node_pops, prim_sibling_tests, prim_tri_tests, prim_tri_hits;
} pno_stats;

/* Render frames [first_frame, first_frame + n_frames) for the rows
 * y = y_begin, y_begin + y_step, ... < y_end of a width*height RGBA32F
 * accumulation image (row 0 = bottom, as imagePos.y), blending each frame
 * with the progressive mean of ray_tracing.comp:988-991.  `threads` = OpenMP
 * threads (<=0: all).  Returns 0, or <0 on invalid input. */
int pno_render(const pno_scene* scene, const pno_frame* frame,
               uint32_t first_frame, uint32_t n_frames,
               int y_begin, int y_end, int y_step,
               float* accum, int threads, pno_stats* stats);

/* The same frames' clamped colours before the blend (:975-987), for the same rows:
 * colors is n_frames x height x width x 3 floats, frame k of the call first; the rows
 * outside the selection and the stats' accum_rmw are left alone. */
int pno_render_colors(const pno_scene* scene, const pno_frame* frame,
                      uint32_t first_frame, uint32_t n_frames,
                      int y_begin, int y_end, int y_step,
                      float* colors, int threads, pno_stats* stats);

/* Evaluate one PN-libm / IEEE primitive over n inputs (math parity test).
 * fn: 0 sin, 1 cos, 2 atan2(a,b), 3 asin, 4 log, 5 pow(a,b), 6 exp2,
 *     7 sqrt, 8 a/b, 9 float(uint32 bits of a), 10 wang_hash(bits of a) */
void pno_math_eval(int fn, const float* a, const float* b, float* out, int n);

/* Pinning hook (tests only): the oracle's intersection routines on caller
 * rays, n x 7 floats (origin, dir, tMax).  kind 0: closest hit over the BVH
 * (BVHIntersect, :429-461), 1: any hit (BVHIntersectP, :464-494), 2: one
 * triangle idx[i] (TriangleIntersect, :254-357), 3: TriangleIntersectP
 * (:360-427), 4: the box of node idx[i] (BoundIntersect, :213-228).
 * sem 0: the GLSL's rules (as rendered); otherwise a mask of the reference
 * CPU headers' rules: 1 triangle.hpp:75-76 `>=` ties, 2 bound.hpp:31-47
 * [0,tMax] slab clipping with std::max/min, 4 glm::normalize; sem 7 makes the
 * shared arithmetic comparable bit for bit with the reference compiled here
 * (oracle/ref/isect_driver.cpp).
 * out: n x 13 words: hit, position[3], normal[3], texcoord[2], textureId,
 * materialId, time (floats as bits; zeros when no hit), ray tMax after; for
 * kind 4 with sem & 2: hit, t0, t1.  Returns 0, -1 bad args, -6 stack overflow. */
int pno_intersect(const pno_scene* scene, const float* rays, int n, int kind, int sem,
                  const int* idx, uint32_t* out, int threads);

/* Pinning hook (tests only): one of the shading functions pno_render itself
 * runs, on n caller records of 32-bit words (floats as bits); tests/test_shader_pin.py
 * compares the words with those of the reference's shader text compiled as C++
 * (oracle/shader/shader_driver.cpp `FUNC`, the same table).  Material = the 18
 * floats of the struct in declaration order (:19-26), set directly.
 *  fn  function (ray_tracing.comp)   words in                          words out
 *   0  DisneyBRDF                    V N L X Y Material (33)           3
 *   1  SampleDisneyBRDF              seed V N T B Material r1 r2 (33)  L pdf seed (5)
 *   2  SampleGTR1   3 SampleGTR2     n t b v r1 r2 alpha (15)          3
 *   4  SampleCosineHemisphere        seed n t b (10)                   dir seed (4)
 *   5  BuildTangentSpace             n (3)                             t b (6)
 *   6  GTR1   7 GTR2   9 smithG_GGX  2                                 1
 *   8  GTR2_aniso  10 smithG_GGX_aniso  5                              1
 *  11  toSphericalCoord              v (3)                             2
 *  12  GetHDRImageColor              v (3)                             3
 *  13  SampleHDRImage                seed (1)                          colour L pdf seed (8)
 *  14  GetLightIndex                 u (1)                             index (1)
 *  15  TriangleSample                triangle u (3)                    position normal texcoord textureId materialId (10)
 *  16  UniformSampleTriangle         u (2)                             2
 *  17  sobolVec2                     i b (2)                           2
 *  18  CranleyPattersonRotation      x y p (4)                         2
 *  19  wang_hash                     seed (1)                          value seed (2)
 *  20  CameraGetRay                  s t (2)                           origin dir tMax (7)
 *  21  GetMaterial                   index (1)                         Material (18)
 * Returns the words written per record, or -1 on bad arguments. */
int pno_shade_eval(const pno_scene* scene, const pno_frame* frame, int fn,
                   const uint32_t* in, int n, uint32_t* out);

/* Known-answer helpers. */
uint32_t pno_wang_hash(uint32_t* seed);
float pno_sobol(uint32_t d, uint32_t i);

#ifdef __cplusplus
}
#endif
#endif
