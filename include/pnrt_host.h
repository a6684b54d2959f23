/*
 * include/pnrt_host.h -- C ABI of libpnrt_host.so, the host-side scene
 * library.  It rebuilds, bit for bit, the flattened arrays PnRayTracing's
 * main.cpp uploads to its compute shader (main.cpp:409-524), so the device
 * library (include/pnrt.h) receives exactly what the reference would:
 *
 *   reference interface replaced             here
 *   ----------------------------------------  ------------------------------
 *   Model ctor + ModelOutput (model.hpp:22-135) pnrt_scene_add_material/_mesh
 *   BVH::BuildBVH (BVH.hpp:92-173)             pnrt_scene_build (or libpnrt.so
 *                                              pnrt_bvh_build + pnrt_scene_set_bvh)
 *   light prefix list (main.cpp:374-383)       pnrt_scene_build
 *   packing loops (main.cpp:409-524)           pnrt_scene_pack
 *   (none: models are placed once)             pnrt_bvh_refit_cpu, pnrt_scene_relight
 *   Camera::UpdateCamera (camera.hpp:11-31)    pnrt_camera_update, pnrt_camera_state_init
 *   Camera::UpdateRotate/TranslateUV/Fov       pnrt_camera_rotate/_translate/_zoom
 *     (camera.hpp:33-65, main.cpp:118-142)
 *   glm::translate/rotate/scale (main.cpp:207-237)  pnrt_model_matrix
 *   stbi_loadf RGBE (stb_image.h:6839-6990)    pnrt_hdr_decode_rgbe
 *   LoadHDRImage CDF table (shader.hpp:145-203) pnrt_hdr_build_table
 *
 * Assimp OBJ import is not reproduced (no asset files, no Linux library):
 * meshes arrive as model-space arrays (pnrt_scene_add_mesh) or from the
 * deterministic procedural generators below (bunny/teapot/marry stand-ins).
 *
 * All functions return 0 on success and a negative code on error; the
 * message is available from pnrt_host_last_error().
 */
#ifndef PNRT_HOST_H
#define PNRT_HOST_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PNRT_VERTEX_SIZE 15   /* PnRT.hpp:45 */
#define PNRT_MATERIAL_SIZE 18 /* PnRT.hpp:46 */
#define PNRT_TRIANGLE_SIZE 6  /* PnRT.hpp:47 */
#define PNRT_BVHNODE_SIZE 12  /* PnRT.hpp:48 */
#define PNRT_LIGHT_SIZE 3     /* PnRT.hpp:49 */

typedef struct pnrt_scene pnrt_scene;

/* one factor of a glm model matrix: kind 0 = translate(v), 1 = rotate(angle_deg
 * about axis v), 2 = scale(v); factors multiply left to right from identity,
 * exactly as glm::translate(mat4(1),..) * glm::rotate(mat4(1),..) * ... */
typedef struct { int kind; float angle_deg; float v[3]; } pnrt_xform;

const char* pnrt_host_last_error(void);

int pnrt_model_matrix(const pnrt_xform* ops, int n_ops, float out_col_major[16]);
/* transpose(inverse(m)) in glm's compute_inverse expression order, column major: the
 * matrix ModelOutput (model.hpp:101-135) takes a model's normals through, and the N of
 * libpnrt.so's pnrt_place_models.  A singular m gives non-finite entries. */
int pnrt_normal_matrix(const float m_col_major[16], float out_col_major[16]);

pnrt_scene* pnrt_scene_create(void);
void pnrt_scene_destroy(pnrt_scene* s);
/* Material record in main.cpp:438-456 order (18 floats).  Returns its id. */
int pnrt_scene_add_material(pnrt_scene* s, const float material18[18]);
/* One Assimp mesh of one Model (model.hpp:131-178 output): model-space
 * vertices (positions/normals/tangents/bitangents 3 f each, texcoords 2 f;
 * NULL -> zeros), triangle index list, the model's matrix and ids.  Appended
 * with ModelOutput semantics (model.hpp:101-135). */
int pnrt_scene_add_mesh(pnrt_scene* s, int material_id, int texture_id,
                        const float model_matrix[16],
                        const float* positions, const float* normals,
                        const float* tangents, const float* bitangents,
                        const float* texcoords, int n_vertices,
                        const int32_t* indices, int n_indices);
/* BuildBVH over all triangles + emissive light list. */
int pnrt_scene_build(pnrt_scene* s);
/* GPU BuildBVH support (libpnrt.so pnrt_bvh_build): the builder's input,
 * Bound + boundCenter of every triangle in the current order (9 floats:
 * pMin.xyz pMax.xyz centre.xyz), and installing its output (triangle order,
 * main.cpp-layout nodes) in place of pnrt_scene_build's; the light list is
 * rebuilt in the new order as pnrt_scene_build does. */
int pnrt_scene_tri_bounds(const pnrt_scene* s, float* out9);
int pnrt_scene_set_bvh(pnrt_scene* s, const int32_t* order, const float* bvh_nodes12, int n_nodes,
                       int max_depth);
/* The host BuildBVH over bare bounds, with pnrt_bvh_build's signature (no
 * context): the CPU counterpart the GPU build is checked against. */
int pnrt_bvh_build_cpu(const float* tri_bounds9, int n_triangles, float* nodes_out, int node_capacity,
                       int* n_nodes_out, int32_t* order_out, int* max_depth_out);
/* After a geometry edit (libpnrt.so pnrt_update_vertices; not in the reference,
 * which never moves a model): bare-array functions on the main.cpp-layout
 * arrays, as pnrt_bvh_build_cpu.
 * pnrt_bvh_refit_cpu: the CPU counterpart of the device refit.  Floats 0-5 of
 * every node of the pre-order array are recomputed bottom-up for the vertices
 * given, topology unchanged, with Bound::Union (bound.hpp:4-28) and this
 * library's min/max, (y < x) ? y : x and (x < y) ? y : x -- on a tie the earlier
 * operand stays: a non-empty leaf is the fold of its triangles in ascending
 * order, vertices p0, p1, p2, from (FLT_MAX, lowest); an interior node is
 * fold(left box, right box); an empty leaf (start == end) keeps its box.  With
 * unchanged vertices BuildBVH's own boxes come back bit for bit. */
int pnrt_bvh_refit_cpu(const float* vertices15, int n_vertices, const float* triangles6, int n_triangles,
                       float* bvh_nodes12, int n_nodes);
/* pnrt_scene_relight: float 5 of every triangle record (its area) recomputed as
 * pnrt_scene_add_mesh does, (float)((double)length(cross(p1-p0, p2-p0)) * 0.5),
 * and the light list rebuilt as pnrt_scene_build does (main.cpp:374-383) into
 * lights3_out (3 floats each, at most n_lights_capacity entries; NULL with
 * capacity 0 only counts); *sum_area = the last prefix, 0 without lights
 * (main.cpp:392). */
int pnrt_scene_relight(const float* vertices15, int n_vertices, float* triangles6, int n_triangles,
                       const float* materials18, int n_materials, float* lights3_out, int n_lights_capacity,
                       int* n_lights, float* sum_area);
typedef struct {
    int n_vertices, n_materials, n_triangles, n_nodes, n_lights;
    float lights_sum_area;
    int max_depth;           /* deepest node (root = 0) */
} pnrt_scene_info;
int pnrt_scene_get_info(const pnrt_scene* s, pnrt_scene_info* info);
/* Write the main.cpp-layout arrays (any pointer may be NULL). */
int pnrt_scene_pack(const pnrt_scene* s, float* vertices, float* materials,
                    float* triangles, float* bvh_nodes, float* lights);

/* camera.hpp:11-31 -> eye, lowerLeftCorner, horizontal, vertical */
int pnrt_camera_update(const float eye[3], const float center[3], const float up[3],
                       float fov_deg, float aspect, float out12[12]);

/* CameraGetRay (ray_tracing.comp:205-211) for pixel (px, py), row 0 = bottom, as the
 * renderer calls it: s = (float)px / (float)width, t = (float)py / (float)height, no
 * jitter; cam12 = pnrt_camera_update's out12.  ray7_out: origin, normalised
 * direction, tMax 1e7 -- a ray of libpnrt.so's pnrt_query_rays, bit for bit the one
 * pnrt_render traces for that pixel (picking). */
int pnrt_camera_pixel_ray(const float cam12[12], int px, int py, int width, int height, float ray7_out[7]);

/* The cameras of frames first_frame .. first_frame + n_frames - 1 for libpnrt.so's
 * pnrt_render_cameras: a box pixel filter and a thin lens around the pinhole camera
 * cam12 (pnrt_camera_update's out12) of a width x height frame.
 *   aa_width        the box filter's width in pixels (0 none, 1 one pixel), centred on
 *                   the reference's own sample point (px / width, py / height), so the
 *                   image stays registered with the guide images
 *   lens_radius     in world units (0 pinhole)
 *   focus_distance  from the eye to the plane in focus; read only when lens_radius > 0
 * Frame f draws four numbers of a 4-D additive-recurrence sequence, independent of the
 * path's own Sobol dimensions: with n = (uint32_t)(f + 1) and the multipliers
 * A = {0xDB4F0B91, 0xBBE05633, 0xA0F2EC77, 0x89E18285} (2^32 * phi^-k, k = 1..4, phi the
 * real root of x^5 = x + 1; the third made odd),
 *   u_k = (float)((uint32_t)(n * A_k) >> 8) * 2^-24                        (exact).
 * The twelve floats of a frame are computed in double from the float inputs, each
 * rounded to float once; sums run left to right:
 *   jx = (u1 - 0.5) * aa_width,  jy = (u2 - 0.5) * aa_width
 *   lens_radius > 0:
 *     c = ((ll + 0.5 hor) + 0.5 ver) - eye,  |v| = sqrt((vx vx + vy vy) + vz vz),
 *     s = focus_distance / |c|,  r = lens_radius * sqrt(u3),  phi = (2 pi) * u4
 *     eye' = (eye + (r cos phi) * (hor / |hor|)) + (r sin phi) * (ver / |ver|)
 *     ll_f = eye + (ll - eye) * s,  hor' = hor * s,  ver' = ver * s
 *     (the plane in focus stays fixed while the eye moves over the lens disc, so points
 *     on it stay sharp: the accumulation-buffer method)
 *   lens_radius == 0: eye' = eye, hor' = hor, ver' = ver, ll_f = ll, copied
 *   ll' = (ll_f + (jx / width) * hor') + (jy / height) * ver'   (aa_width == 0: ll_f)
 * with ll_f, hor', ver' unrounded inside ll'.  aa_width == 0 && lens_radius == 0 returns
 * cam12 bit for bit in every frame.  cams12_out: 12 * n_frames floats (eye',
 * ll', hor', ver' per frame).
 * PNRT_E_ARG (-1): a NULL pointer; width or height < 1; aa_width or lens_radius not
 * finite or < 0; lens_radius > 0 with a focus_distance that is not finite and > 0;
 * reserved != 0; a degenerate plane (|c|, |hor| or |ver| zero or not finite). */
typedef struct { float aa_width, lens_radius, focus_distance; uint32_t reserved; } pnrt_lens_params; /* 16 bytes */
int pnrt_camera_sequence(const float cam12[12], int width, int height, const pnrt_lens_params* p,
                         uint32_t first_frame, uint32_t n_frames, float* cams12_out);

/* Camera state (camera.hpp:4-77) and the interactive controls that
 * main.cpp's mouse callbacks call (main.cpp:118-142): left drag ->
 * UpdateRotate(dx, dy), right drag -> UpdateTranslateUV(-dx, dy), scroll ->
 * UpdateFov(yoffset).  eye/lower_left/horizontal/vertical feed pnrt_set_frame.
 * rotate/zoom return 1 if applied, 0 if the reference rejects the move
 * (rotation within 0.9995 of the up axis; fov outside (1, 89)). */
typedef struct {
    float eye[3], center[3], up[3];
    float fov_deg, aspect;
    float u[3], v[3], w[3];
    float distance;
    float lower_left[3], horizontal[3], vertical[3];
} pnrt_camera_state;
int pnrt_camera_state_init(pnrt_camera_state* c, const float eye[3], const float center[3], const float up[3],
                           float fov_deg, float aspect);
int pnrt_camera_rotate(pnrt_camera_state* c, float phi, float theta);
int pnrt_camera_translate(pnrt_camera_state* c, float dx, float dy);
int pnrt_camera_zoom(pnrt_camera_state* c, float delta);

/* Radiance RGBE decode with stbi_loadf semantics (3 channels, row 0 = first
 * scanline).  out_rgb may be NULL to query w/h; caller allocates w*h*3. */
int pnrt_hdr_decode_rgbe(const uint8_t* bytes, int64_t n_bytes, int* w, int* h, float* out_rgb);
/* LoadHDRImage's luminance CDF + inverse lookup table (RandomHDR). */
int pnrt_hdr_build_table(const float* rgb, int w, int h, float* out_random_hdr);

/* ---- deterministic procedural stand-ins (model space, unshared vertices) --
 * Output arrays sized by the *_count functions: positions/normals 3*nv,
 * texcoords 2*nv, indices 3*nt.  Pass NULL outputs to get counts only. */
/* floor.obj stand-in: quad in XZ at y=0, |x|,|z| <= half, normal +Y. */
int pnrt_mesh_quad(float half, float* positions, float* normals, float* texcoords,
                   int32_t* indices, int* nv, int* nt);
/* displaced UV sphere: nu x nv quads (2 tris each), radius r at center c,
 * radial value-noise displacement of relative amplitude amp, seed. */
int pnrt_mesh_displaced_sphere(int nu, int nvv, float radius, const float center[3],
                               float amp, uint32_t seed,
                               float* positions, float* normals, float* texcoords,
                               int32_t* indices, int* nv, int* nt);
/* teapot-class lathe body + spout + handle (~6.1k tris). */
int pnrt_mesh_teapot(float* positions, float* normals, float* texcoords,
                     int32_t* indices, int* nv, int* nt);
/* synthetic HDR environment (sky gradient + sun lobe + seeded noise). */
int pnrt_hdr_synthetic(int w, int h, uint32_t seed, float* out_rgb);

#ifdef __cplusplus
}
#endif
#endif
