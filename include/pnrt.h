/*
 * include/pnrt.h -- C ABI of libpnrt.so, the MI355X (gfx950) path-tracing
 * library that replaces PnRayTracing's OpenGL compute-shader hot path
 * (shaders/ray_tracing.comp, dispatched from main.cpp:613).
 *
 * Each entry point replaces one piece of the GL binding contract main.cpp
 * fills today (the reference interface is cited per function).  Inputs are the
 * SAME host-built float arrays main.cpp uploads (integers stored as floats);
 * the library copies caller memory during upload* and never keeps pointers to
 * it.  No torch or HIP types appear in the signatures: streams are passed as
 * opaque pointers (a hipStream_t, or NULL for the context's own stream).
 *
 * Threading: a context belongs to one HIP device and is not thread-safe; use
 * one context per device (one process per GPU in the multi-GPU driver).
 * Errors: every int-returning call returns 0 on success or a negative PNRT_E*
 * code, with a message in pnrt_last_error(ctx).  Nothing calls exit().
 */
#ifndef PNRT_H
#define PNRT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PNRT_OK 0
#define PNRT_E_ARG (-1)       /* invalid argument                      */
#define PNRT_E_HIP (-2)       /* HIP runtime error                     */
#define PNRT_E_STATE (-3)     /* call out of order (e.g. render before upload) */
#define PNRT_E_SCENE (-4)     /* scene arrays inconsistent / unsupported */
#define PNRT_E_NOMEM (-5)
#define PNRT_E_TRACE (-6)     /* a trace launch may have left queued rays untraced (a bounded */
                              /* wait of its ray queue ran out, or a ray count check failed): */
                              /* the accumulation image is invalid.  Returned by pnrt_render,  */
                              /* pnrt_synchronize, pnrt_read_accum and pnrt_pack_rows once the */
                              /* faulting work has completed (pnrt_synchronize / read_accum    */
                              /* always see it); sticky until pnrt_reset_accum.                */

typedef struct pnrt_ctx pnrt_ctx;

/* camera.hpp:28-30 / the camera.* uniforms set at main.cpp:606-610 */
typedef struct {
    float eye[3], lower_left[3], horizontal[3], vertical[3];
} pnrt_camera;

typedef struct {
    int n_interior;      /* interior BVH nodes in the device layout          */
    int n_triangles;
    int max_depth;       /* deepest reference node (root = 0)                */
    int64_t device_bytes;/* scene bytes resident in HBM                      */
    int root_is_leaf;
    int stack_limit;     /* traversal stack entries available per lane       */
    int has_leaf_table;  /* a leaf too large for an inline ref: the scene runs the */
                         /* leaf-table instantiation of the trace kernels          */
} pnrt_device_info;

/* Options (pnrt_set_options): a traversal mode, optionally | a kernel variant. */
#define PNRT_TRAVERSE_EXACT 0   /* the reference's box visits (no tMax culling)      */
#define PNRT_TRAVERSE_ZCULL 1   /* + provably result-neutral z-slab culling (default) */
#define PNRT_KERNEL_V1 0x100    /* A/B baseline: one lane per pixel, frames in-lane        */
#define PNRT_SERIAL 0x200       /* measurement: one pnrt_render call in flight and a full- */
                                /* occupancy trace grid, so a kernel's launch duration is  */
                                /* its exclusive time (same images; slower end to end)     */
                                /* default: wavefront (setup / trace / shade per bounce)   */

/* "pnrt-mi355x <version> (gfx950) src <sha256[:16] of the device sources>" */
const char* pnrt_version(void);

/* Replaces WindowInit's GL context (main.cpp:64-94): bind HIP device. */
int pnrt_create(int device, pnrt_ctx** out);
void pnrt_destroy(pnrt_ctx* ctx);
const char* pnrt_last_error(pnrt_ctx* ctx);
/* Launch work on `hip_stream` (a hipStream_t; NULL = the context's stream).
 * The new stream is ordered after the last operation the context queued on the
 * previous one (an event the context records with every such operation), so
 * frame-ordered blends never overtake each other; the previous stream itself
 * is not touched again and may already be destroyed. */
int pnrt_set_stream(pnrt_ctx* ctx, void* hip_stream);
/* The context's own stream (created with it, before its worker streams): a caller
 * that wraps it (e.g. torch.cuda.ExternalStream) adds no stream of its own. */
void* pnrt_get_stream(pnrt_ctx* ctx);

/* Replaces the five TBO/texture uploads main.cpp:409-524 (texture units 0-4)
 * and the lightsSize/lightsSumArea uniforms (main.cpp:391-392):
 *   vertices  15 f each (main.cpp:412-428)     materials 18 f (main.cpp:438-456)
 *   triangles  6 f each (main.cpp:470-477)     bvh_nodes 12 f (main.cpp:488-501)
 *   lights     3 f each (main.cpp:513-517)     (lights may be NULL when n_lights = 0)
 * The arrays are validated and re-laid out for gfx950.
 * A triangle's texture id (float 4 of its record) is -1 (no texture) or a slot
 * 0..19 -- the reference binds 20 samplers, other ids are undefined there -- and
 * any other id returns PNRT_E_SCENE naming the triangle.  A slot 0..19 that no
 * pnrt_upload_texture call filled is legal: an unbound sampler, such a hit is
 * black.  The BVH may be at most stack_limit - 2 levels deep (pnrt_device_info),
 * its root may be a leaf, and a leaf may be empty (start == end). */
int pnrt_upload_scene(pnrt_ctx* ctx,
                      const float* vertices, int n_vertices,
                      const float* materials, int n_materials,
                      const float* triangles, int n_triangles,
                      const float* bvh_nodes, int n_nodes,
                      const float* lights, int n_lights, float lights_sum_area);

/* Replaces the material panel's in-place edit of the material texture
 * (include/ImGuiLayer.hpp:73-83: glTexSubImage1D on unit 1 when a slider
 * moves, followed by main.cpp:592-596's redraw): overwrite materials
 * first .. first + count - 1 with count records of 18 floats in the
 * main.cpp:438-456 layout, without re-uploading or re-laying out the scene.
 * Calls already issued render with the old records (the call waits for them);
 * later calls see the new ones.  The caller resets the accumulation as the
 * reference's redraw does (pnrt_reset_accum). */
int pnrt_update_materials(pnrt_ctx* ctx, int first, int count, const float* materials18);

/* In-place geometry edit.  Not in the reference, which places every model once
 * with a matrix (main.cpp:207-237) and offers no edit of geometry; what it
 * replaces here is a whole pnrt_upload_scene after a model was moved, scaled
 * or deformed.  Overwrites vertex records first .. first + count - 1 with count
 * records of 15 floats in the main.cpp:412-428 layout, world space, and brings
 * every record derived from them (per-triangle positions and attributes, the
 * light records) and every BVH box up to date on the device.  Tree topology,
 * triangle order, material and texture ids, child refs and the leaf table do
 * not change.  Synchronous: it waits for the calls in flight, which render
 * with the old geometry, and returns when the scene is current.  The caller
 * resets the accumulation as a redraw does (pnrt_reset_accum).  Nothing is
 * allocated per call beyond a staging buffer that grows to the largest edit.
 *
 * The refit rule is Bound::Union (bound.hpp:4-28) with the comparisons
 * min(x, y) = (y < x) ? y : x and max(x, y) = (x < y) ? y : x, so on a tie --
 * -0 against +0 -- the EARLIER operand stays, and a NaN coordinate never
 * enters a box:
 *   non-empty leaf  the fold of its triangles in ascending order, vertices p0,
 *                   p1, p2, starting from (FLT_MAX, lowest);
 *   interior node   fold(left child's box, right child's box);
 *   empty leaf      (start == end) keeps its uploaded box, which takes part in
 *                   its parent's fold.
 * With unchanged vertices this gives back BuildBVH's own boxes bit for bit.
 * Positions are not validated (pnrt_upload_scene does not either): a box with
 * a non-finite coordinate switches the traversal to PNRT_TRAVERSE_EXACT, as at
 * upload.  A refit tree and a tree rebuilt for the new positions can render
 * different image bits (a triangle is tested only when every box above it
 * passes the slab test): the image is what ray_tracing.comp renders from the
 * refit node array, which pnrt_read_bvh_boxes returns.
 *
 * lights: the set and order of light triangles cannot change, their areas can.
 * NULL keeps the uploaded prefix areas and lights_sum_area -- the caller's
 * statement that no emissive triangle changed area -- and lights_sum_area is
 * then ignored; otherwise exactly the uploaded n_lights records of 3 floats
 * with the same triangle index in every entry, and the prefix areas and
 * lights_sum_area are taken as pnrt_upload_scene takes them.
 *
 * Afterwards the guide images are stale (pnrt_denoise* answer PNRT_E_STATE
 * until pnrt_render_guides).  Errors: PNRT_E_STATE before pnrt_upload_scene;
 * PNRT_E_ARG, with nothing changed, for a range outside the uploaded vertex
 * array, NULL vertices with count > 0, a device pointer that is not 4-byte
 * aligned, or a lights entry naming another triangle than the uploaded one
 * (the message names the entry); PNRT_E_TRACE as pnrt_read_accum returns it.
 * count == 0 with lights == NULL does nothing.  The _device form reads the
 * records from device memory of the context's device. */
int pnrt_update_vertices(pnrt_ctx* ctx, int first, int count, const float* vertices15,
                         const float* lights, float lights_sum_area);
int pnrt_update_vertices_device(pnrt_ctx* ctx, int first, int count, const void* vertices15_dev,
                                const float* lights, float lights_sum_area);

/* Models moved on the device by a matrix.  Not in the reference, which places
 * every model once at load (main.cpp:207-237, ModelOutput model.hpp:101-135):
 * this is that step, on the device, in front of pnrt_update_vertices's refit,
 * so that moving a model costs its matrix and not its vertices.
 *
 * pnrt_define_model keeps a device copy (32 bytes a vertex) of the MODEL-space
 * records of vertices first_vertex .. first_vertex + count - 1, 8 floats each:
 * position 3, normal 3, texcoord 2 (the device keeps no tangent or bitangent).
 * It changes nothing in the scene and returns ids 0, 1, 2, ... in definition
 * order.  Errors, each with nothing kept: PNRT_E_STATE before
 * pnrt_upload_scene; PNRT_E_ARG for count < 1, a range outside the uploaded
 * vertex array or overlapping an already defined model's, a NULL pointer, or
 * (the _device form, which reads device memory of the context's device) a
 * pointer that is not 4-byte aligned.  pnrt_upload_scene forgets every model
 * and frees the copies: the ids are invalid afterwards.
 *
 * pnrt_place_models writes, for each of the n placements (1 .. 1024), the
 * world-space records of that model's range, then refits once as
 * pnrt_update_vertices does: synchronous, it waits for the calls in flight,
 * and the guide images and kept primary records go stale.  With
 * N = transpose(inverse(M)) in glm's expression order (libpnrt_host.so's
 * pnrt_normal_matrix), every product and sum rounded on its own, for row r:
 *   pos[r]    = (M[0][r] * p.x + M[1][r] * p.y) + (M[2][r] * p.z + M[3][r] * 1.0f)
 *   normal[r] = (N[0][r] * n.x + N[1][r] * n.y) + (N[2][r] * n.z + N[3][r] * 1.0f)
 * and the texcoords copied: the bits of libpnrt_host.so's pnrt_scene_add_mesh.
 * The normal is not normalised (ModelOutput does not).  The result is defined
 * from the model-space copy, never from the current records: placing M1 then
 * M2 gives the bits of placing M2 alone.  A later pnrt_update_vertices on a
 * model's range is legal; the model's next placement overwrites it.
 *
 * relight = 0 keeps the prefix areas and lights_sum_area, as lights == NULL
 * does in pnrt_update_vertices.  relight = 1 recomputes them from the new
 * positions: area = (float)((double)length(cross(p1 - p0, p2 - p0)) * 0.5) per
 * light triangle and the float prefix of main.cpp:374-383, which is
 * libpnrt_host.so's pnrt_scene_relight.  This replaces EVERY entry's area, those
 * of untouched lights included: a caller with areas of its own follows with
 * pnrt_update_vertices(ctx, 0, 0, NULL, lights, lights_sum_area).
 *
 * Errors, with nothing changed: PNRT_E_STATE before pnrt_upload_scene;
 * PNRT_E_ARG for n outside 1 .. 1024, NULL placements, relight not 0 or 1,
 * and -- the message names the placement -- an unknown id, an id named twice,
 * reserved != 0, a matrix float that is not finite, or a matrix whose N has a
 * non-finite entry (a singular one); PNRT_E_TRACE as pnrt_read_accum returns it. */
typedef struct {
    int model;                /* pnrt_define_model's id */
    float matrix[16];         /* column major, as libpnrt_host.so's pnrt_model_matrix writes it */
    int reserved;             /* 0 */
} pnrt_placement;             /* 72 bytes */
int pnrt_define_model(pnrt_ctx* ctx, int first_vertex, int count, const float* model8, int* model_id_out);
int pnrt_define_model_device(pnrt_ctx* ctx, int first_vertex, int count, const void* model8_dev, int* model_id_out);
int pnrt_place_models(pnrt_ctx* ctx, const pnrt_placement* placements, int n, int relight);

/* The vertex records the device currently holds, 8 floats each (position 3,
 * normal 3, texcoord 2), first .. first + count - 1, to the host.  Synchronous.
 * PNRT_E_STATE before pnrt_upload_scene; PNRT_E_ARG for a range outside the
 * uploaded array. */
int pnrt_read_vertices(pnrt_ctx* ctx, int first, int count, float* out8);

/* The boxes the device currently holds, into floats 0-5 of every node of the
 * caller's pre-order node array (main.cpp:488-501 layout); floats 6-11 are
 * read, not written.  Not in the reference.  The array must be the topology
 * that was uploaded -- the library keeps no host copy of the scene --:
 * PNRT_E_ARG, with nothing written, when its interior-node count or a child's
 * kind (leaf or interior) disagrees with the uploaded tree.  An empty leaf's
 * box comes back as uploaded.  Synchronous. */
int pnrt_read_bvh_boxes(pnrt_ctx* ctx, float* bvh_nodes12, int n_nodes);

/* Replaces the albedo texture uploads (main.cpp:527-554, units 5..24):
 * tightly packed 8-bit rows as stbi_load returns them; GL's default
 * UNPACK_ALIGNMENT of 4 is applied as glTexImage2D would. slot 0..19. */
int pnrt_upload_texture(pnrt_ctx* ctx, int slot, const uint8_t* pixels, int width, int height,
                        int channels);

/* Replaces LoadHDRImage's two glTexImage2D calls (shader.hpp:136-214, units
 * 29/30) and the HDRImageWidth/Height/HasHDRImage uniforms.  hdr_rgb == NULL
 * clears the environment (HasHDRImage = 0). */
int pnrt_upload_env(pnrt_ctx* ctx, const float* hdr_rgb, const float* random_hdr_rgb, int width,
                    int height);

/* LoadHDRImage (shader.hpp:126-225) with its RandomHDR table built on the
 * GPU instead of on the host: the same table, bit for bit, as the
 * host restatement pnrt_hdr_build_table (every float sum in the reference's
 * order).  hdr_rgb: width*height*3 floats as stbi_loadf returns them. */
int pnrt_upload_env_build(pnrt_ctx* ctx, const float* hdr_rgb, int width, int height);
/* Copy the bound RandomHDR table (width*height*3 floats) to the host. */
int pnrt_read_env_table(pnrt_ctx* ctx, float* random_hdr_out);

/* Replaces the per-frame uniforms SCREEN_WIDTH/HEIGHT (main.cpp:389-390),
 * camera.* (main.cpp:606-610) and MAX_BOUNCE_DEPTH (main.cpp:593,599).
 * (Re)allocates a zeroed width*height RGBA32F accumulation image when the
 * size changes -- and, from the first pnrt_enable_moments on, a zeroed moments
 * image, which then covers the accumulation again.  A call with the size
 * unchanged touches neither image: a camera move or another depth alone does
 * not clear the accumulation.  The caller resets it (pnrt_reset_accum) or goes
 * on, and later frames blend into the old image by their frame numbers (frame 0,
 * whose weight is 1, overwrites the rows it renders).
 * The guide images stay what they were rendered for: under another camera or
 * size pnrt_denoise* refuse them until pnrt_render_guides (the depth does not
 * enter: a first hit has none), and a call that comes back to the camera and
 * size they were rendered for, with the scene and the traversal mode unchanged,
 * makes them current again.  The denoised and the display image keep the size
 * they were made at; their readers and PNRT_DISPLAY_DENOISED refuse them while
 * the frame size is another one. */
int pnrt_set_frame(pnrt_ctx* ctx, int width, int height, const pnrt_camera* camera,
                   int max_bounce_depth);

/* Takes effect with the next call; no image changes.  The traversal mode is part of
 * what the guide images were rendered for (pnrt_denoise* refuse guides of the other
 * mode); PNRT_KERNEL_V1 and PNRT_SERIAL are not. */
int pnrt_set_options(pnrt_ctx* ctx, int options);

/* Replaces glDispatchCompute (main.cpp:613) called once per frame for frames
 * first_frame .. first_frame + n_frames - 1 (frameCount uniform), blended in
 * order into the accumulation image with the progressive mean of
 * ray_tracing.comp:988-991.  Shard selector (multi-GPU row bands): only rows
 * y with (y / band_rows) % n_shards == shard are rendered; full image =
 * (band_rows >= 1, n_shards = 1, shard = 0).  band_rows may be any positive int
 * (up to INT_MAX; here and in pnrt_batch_plan, pnrt_pack_rows, pnrt_unpack_rows):
 * with band_rows >= height the image is one band, shard 0 renders all of it and
 * every other shard has no rows (the call returns PNRT_OK and queues nothing).
 * Asynchronous on the stream.
 * The frames run in batches of up to 128 frames and 2^28 paths (~310 B of
 * device memory per path; the environment variable PNRT_BATCH_BYTES, read when
 * the context is created, caps one batch's bytes -- the batching changes no
 * pixel; pnrt_batch_plan reports it).
 * Frame numbers end at 0xFFFFFFFE: frame 0xFFFFFFFF would blend with the weight
 * 1 / (float)(frameCount + 1) = 1 / 0, and the frames after it would wrap to 0.
 * A call with first_frame + n_frames > 0xFFFFFFFF returns PNRT_E_ARG, queues
 * nothing and leaves the accumulation image untouched. */
int pnrt_render(pnrt_ctx* ctx, uint32_t first_frame, uint32_t n_frames, int band_rows,
                int n_shards, int shard);

/* The batches pnrt_render would run for a call of n_frames frames with this
 * shard selector at the current frame size (read-only, queues nothing; the
 * PNRT_KERNEL_V1 path has no batches, the wavefront plan is reported all the
 * same): frames per full batch, the number of batches (the last may be
 * shorter), and batch_bytes, the measure PNRT_BATCH_BYTES caps -- the path
 * state and colour bytes of one full batch.  Under a cap, frames_per_batch is
 * the largest count whose batch_bytes fit it, and 1 when not even one frame
 * does.  All three are 0 for n_frames = 0 or a shard with no rows.  Out
 * pointers may be NULL.  PNRT_E_STATE before pnrt_set_frame.
 *
 * PNRT_BATCH_BYTES is read by pnrt_create: decimal digits only, a value that
 * fits 64 bits, 0 = no cap.  Any other spelling ("3e9", "abc", "-1", "",
 * trailing characters) makes pnrt_create return PNRT_E_ARG. */
int pnrt_batch_plan(pnrt_ctx* ctx, uint32_t n_frames, int band_rows, int n_shards, int shard,
                    uint32_t* frames_per_batch, uint32_t* n_batches, int64_t* batch_bytes);

/* Per-frame cameras (not in the reference, whose camera ray goes through the same
 * point of the pixel in every frame, ray_tracing.comp:980): frame first_frame + k is
 * rendered as pnrt_render would render it if cameras[k] were the camera of
 * pnrt_set_frame -- the camera ray, the miss colour of its direction, V at bounce 0
 * and everything downstream.  The seed, the Sobol index, the blend weight
 * 1 / (float)(frame + 1), the clamp, the frame order, the shard selector and the
 * traversal mode are pnrt_render's, so the accumulation is the reference's shader
 * run once per frame with that frame's camera uniforms.  A sub-pixel shift of
 * lower_left per frame gives a box pixel filter; an eye moved over a lens disc with
 * the image plane held at the focus distance a thin lens; an eye moved along a path
 * camera motion blur (pnrt_camera_sequence, pnrt_host.h, makes the first two).
 *
 * Frame size and depth are pnrt_set_frame's; its camera is ignored by this call and
 * stays current for pnrt_render, pnrt_render_guides and pnrt_reproject.  The
 * per-pixel camera-ray records pnrt_render keeps are neither used nor invalidated,
 * and the guide images stay those of the pnrt_set_frame camera (the centre view).
 * Asynchronous on the stream and ordered like pnrt_render.  `cameras` (n_frames
 * records, host memory) is copied during the call: the caller may overwrite it as
 * soon as the call returns, and several calls may be in flight.
 * Batches follow pnrt_batch_plan's rules with 48 more bytes per path (the camera
 * ray's record, one per path instead of one per pixel); PNRT_BATCH_BYTES caps that
 * larger measure, batch b uses cameras[b * frames_per_batch + k], and
 * pnrt_cameras_batch_plan reports the plan.  Sample moments are updated when
 * enabled, and for pnrt_render_adaptive's "moments cover the accumulation" rule the
 * frames count like pnrt_render's.  Profile classes: the camera rays are
 * PNRT_K_PRIMARY (one launch per batch), the rest as pnrt_render's.
 *
 * Errors (nothing queued, accumulation untouched): PNRT_E_STATE before
 * pnrt_upload_scene or pnrt_set_frame, or under PNRT_KERNEL_V1; PNRT_E_ARG for a bad
 * selector, first_frame + n_frames > 0xFFFFFFFF, cameras == NULL with n_frames > 0,
 * or any of the 12 * n_frames floats not finite (the message names the frame);
 * PNRT_E_TRACE as pnrt_render.  n_frames == 0 or a shard without rows: PNRT_OK,
 * nothing queued.
 * Out of scope: an adaptive variant over `cameras` (adaptive sampling goes through
 * rays: pnrt_make_rays makes these cameras' rays, pnrt_render_rays_adaptive renders
 * them), a device-array form of `cameras`, and per-pixel (rather than per-frame)
 * lens samples. */
int pnrt_render_cameras(pnrt_ctx* ctx, uint32_t first_frame, uint32_t n_frames, const pnrt_camera* cameras,
                        int band_rows, int n_shards, int shard);
/* pnrt_batch_plan for a pnrt_render_cameras call: the same rules over the larger
 * per-path measure (batch_bytes includes the 48-byte camera-ray record per path). */
int pnrt_cameras_batch_plan(pnrt_ctx* ctx, uint32_t n_frames, int band_rows, int n_shards, int shard,
                            uint32_t* frames_per_batch, uint32_t* n_batches, int64_t* batch_bytes);

/* Caller ray buffers (not in the reference, whose CameraGetRay is a pinhole): the image
 * whose pixel (x, y) of frame first_frame + k starts from a ray the caller supplies --
 * what ray_tracing.comp renders there when CameraGetRay returns Ray(origin, direction):
 * the camera ray, the miss colour of its direction, V = -direction at bounce 0 and
 * everything downstream.  The seed, the Sobol index, the blend weight
 * 1 / (float)(frame + 1), the clamp, the frame order, the selector and the traversal
 * mode are pnrt_render's.  Any camera model, per-pixel jitter, lens or motion sample is
 * a choice of rays (pnrt_make_rays below makes four models' on the device).
 *
 * rays_dev: device memory of the context's device, 16-byte aligned, one pnrt_ray per
 * pixel of the WHOLE image whatever the selector; the ray of pixel (x, y) is record
 * y * width + x, row 0 = bottom.  frame_stride counts records: frame first_frame + k
 * reads the set that starts at record k * frame_stride; 0 (one set serves every
 * frame: a camera model) or >= width * height (a set per frame).  The direction is used
 * as given, never normalised: only unit directions are meaningful, any finite one is
 * memory-safe.  reserved0 / reserved1 are never read.
 * A record with a non-finite float among its six, or a direction of three zeros, is
 * "no ray" (pnrt_query_rays' rule): that pixel's colour for that frame is (0, 0, 0),
 * blended and folded into the moments like any other frame colour; no path starts.
 *
 * The pnrt_set_frame camera is ignored and stays current for pnrt_render,
 * pnrt_render_guides and pnrt_reproject; the kept per-pixel camera-ray records are
 * neither used nor invalidated.  Asynchronous; the buffer is not copied: every batch's
 * reads are ordered after everything queued on the context's stream at the time of the
 * call (whichever worker stream runs the batch), and the caller keeps the buffer
 * unchanged until the call's work has completed.  Batches, PNRT_BATCH_BYTES, moments
 * and profile classes are pnrt_render_cameras' (the same 48-byte record per path slot;
 * pnrt_cameras_batch_plan reports the plan; batch b, frame slot k reads set
 * b * frames_per_batch + k; the ray launch is PNRT_K_PRIMARY).
 *
 * Errors (nothing queued, accumulation untouched): PNRT_E_STATE before
 * pnrt_upload_scene or pnrt_set_frame, or under PNRT_KERNEL_V1; PNRT_E_ARG for
 * rays_dev == NULL with n_frames > 0, a pointer that is not 16-byte aligned,
 * frame_stride < 0 or in 1 .. width * height - 1 or so large that the last set's end
 * passes 2^63 bytes, a bad selector,
 * first_frame + n_frames > 0xFFFFFFFF; PNRT_E_TRACE as pnrt_render.  n_frames == 0 or a
 * shard without rows: PNRT_OK, nothing queued.
 * The adaptive variant is pnrt_render_rays_adaptive.
 * Out of scope: reprojection across arbitrary ray sets (the views of pnrt_make_rays' four
 * models go through pnrt_reproject_view), a host-array form, a tMax or near clip per ray. */
typedef struct { float origin[3], reserved0, direction[3], reserved1; } pnrt_ray;   /* 32 bytes */
int pnrt_render_rays(pnrt_ctx* ctx, uint32_t first_frame, uint32_t n_frames, const void* rays_dev, int64_t frame_stride,
                     int band_rows, int n_shards, int shard);
/* pnrt_render_guides with the camera rays taken from one set of width * height records
 * (alignment and state errors as above): always the whole image, asynchronous and
 * ordered like pnrt_render_rays; one PNRT_K_PRIMARY launch into the guides' own record
 * buffer, then the guide images.  A no-ray pixel is a miss whose albedo is 0.  These
 * guides carry no camera: they stay valid -- pnrt_denoise, pnrt_denoise_variance,
 * pnrt_read_aov and pnrt_aov_device_ptr accept them; that they match the accumulation
 * is the caller's statement -- until pnrt_render_guides or pnrt_reproject replaces them
 * or the frame size, the scene or the traversal mode changes.  pnrt_reproject never
 * uses them as `from`'s guides: it renders its own. */
int pnrt_render_guides_rays(pnrt_ctx* ctx, const void* rays_dev);

/* A ray generator on the device: n_sets sets (frames first_frame ..) of the current
 * frame size into rays_dev_out (alignment and stride rules as above; gap records
 * between sets are left untouched; with frame_stride 0 the sets coincide and the one of
 * first_frame is written).  Asynchronous on the context's stream, class PNRT_K_BLEND.
 * With s = px / width, t = py / height (the reference's sample point):
 *   PNRT_CAM_PINHOLE   origin eye, direction CameraGetRay's operations in its order:
 *                      without jitter and lens pnrt_render_rays on these rays is
 *                      pnrt_render, bit for bit
 *   PNRT_CAM_ORTHO     origin (lower_left + s * horizontal) + t * vertical, direction
 *                      f = normalize(cross(vertical, horizontal))
 *   PNRT_CAM_EQUIRECT  origin eye; r = normalize(horizontal), u = normalize(vertical);
 *                      phi = (s - 0.5) * 2 pi, theta = (t - 0.5) * pi; direction
 *                      normalize((cos theta sin phi) r + sin theta u + (cos theta cos phi) f)
 *   PNRT_CAM_FISHEYE   equidistant, fov_deg in (0, 360]: a = 2s - 1, b = 2t - 1,
 *                      rho = sqrt(a^2 + b^2); rho > 1: no ray (a record of zeros);
 *                      rho == 0: f; else theta = rho * fov / 2, direction
 *                      normalize(sin theta ((a / rho) r + (b / rho) u) + cos theta f)
 * Samples: u_i = (float)(((n * A_i + h_i) & 0xFFFFFFFF) >> 8) * 2^-24, n = frame + 1, A
 * pnrt_camera_sequence's constants; per_pixel 0: h_i = 0 (the per-frame samples);
 * per_pixel 1: h_i = wang_hash of the seed 4 * (py * width + px) + i, so every pixel
 * walks its own rotation of the sequence.  aa_width > 0 shifts (s, t) by
 * ((u_0 - 0.5) * aa_width / width, (u_1 - 0.5) * aa_width / height), any model;
 * lens_radius > 0 is pnrt_camera_sequence's thin lens (u_2, u_3), PNRT_CAM_PINHOLE only.
 * All arithmetic is binary32, every operation rounded on its own, in the order of
 * DESIGN.md section 29.
 * PNRT_E_ARG: an unknown model, a non-finite camera float, fov_deg outside its range
 * (fisheye), a negative or non-finite aa_width or lens_radius, a lens with another
 * model or with focus_distance not > 0, per_pixel not 0 or 1, reserved != 0, the
 * buffer rules above.  PNRT_E_STATE before pnrt_set_frame. */
#define PNRT_CAM_PINHOLE 0
#define PNRT_CAM_ORTHO 1
#define PNRT_CAM_EQUIRECT 2
#define PNRT_CAM_FISHEYE 3
typedef struct {
    int model;                 /* PNRT_CAM_* */
    pnrt_camera camera;        /* eye, lower_left, horizontal, vertical */
    float fov_deg;             /* PNRT_CAM_FISHEYE */
    float aa_width, lens_radius, focus_distance;   /* as pnrt_lens_params */
    int per_pixel;             /* 0 or 1 */
    int reserved;              /* must be 0 */
} pnrt_ray_camera;             /* 76 bytes */
int pnrt_make_rays(pnrt_ctx* ctx, const pnrt_ray_camera* cam, uint32_t first_frame, uint32_t n_sets, void* rays_dev_out,
                   int64_t frame_stride);

/* Redraw semantics (main.cpp:592-596): zero the accumulation image.  Waits
 * for the calls in flight first, and clears a PNRT_E_TRACE fault. */
int pnrt_reset_accum(pnrt_ctx* ctx);
/* Synchronise and copy the width*height*4 floats (row 0 = bottom) to host. */
int pnrt_read_accum(pnrt_ctx* ctx, float* rgba_out);
/* Device pointer of the accumulation image (for collectives / zero-copy use). */
void* pnrt_accum_device_ptr(pnrt_ctx* ctx);
/* Copy this shard's rows, in increasing y, into a contiguous device buffer
 * (rows_of_shard * width * 4 floats), on the context stream. */
int pnrt_pack_rows(pnrt_ctx* ctx, void* dst_device, int band_rows, int n_shards, int shard);
/* The inverse, on the receiving rank of the gather: shard `shard`'s packed rows
 * (as pnrt_pack_rows wrote them on that rank) into their rows of a
 * width*height*4-float device image (row 0 = bottom), on the context stream --
 * the gathered frame assembled by the library's own kernel (the main.cpp
 * display reads one image, main.cpp:613-628). */
int pnrt_unpack_rows(pnrt_ctx* ctx, const void* src_device, void* image_device, int band_rows, int n_shards,
                     int shard);
int pnrt_synchronize(pnrt_ctx* ctx);
int pnrt_get_device_info(pnrt_ctx* ctx, pnrt_device_info* info);

/* First-hit guide images (not in the reference, which shows the raw accumulation:
 * main.cpp:618-628): what the un-jittered camera ray (ray_tracing.comp:205-211,
 * 980) hits in every pixel, as three width*height RGBA32F images, row 0 = bottom
 * -- the inputs of pnrt_denoise and of any external denoiser. */
#define PNRT_AOV_POSITION 0   /* P.xyz of the camera ray's closest hit; w = 1 hit, 0 miss (xyz = 0) */
#define PNRT_AOV_NORMAL   1   /* the shading normal of the hit (ray_tracing.comp:320-355, facing the ray, */
                              /* normalised); w = (float)materialId, -1 on a miss (xyz = 0)               */
#define PNRT_AOV_ALBEDO   2   /* hit: the baseColor the first bounce shades with (ray_tracing.comp:871:   */
                              /* the bilinear REPEAT texture fetch at (u, v) when textureId != -1, else   */
                              /* material.baseColor) -- or, on an emissive material (any emission         */
                              /* component != 0), the emission; miss: the env colour of the primary       */
                              /* direction (0 without an env); w = (float)textureId, -1 when none or on a */
                              /* miss                                                                     */
#define PNRT_AOV_COUNT 3
/* Render the three images for the current frame size, camera, scene and
 * traversal mode -- always the whole image, whatever shards pnrt_render is
 * called with.  Asynchronous on the stream.  The per-pixel records pnrt_render
 * keeps of the camera rays' hits are reused when a call in this context rendered
 * the whole image with the same camera (then no ray is traced), and are never
 * changed; otherwise the camera rays are traced into a buffer of the guides' own
 * (one launch of class PNRT_K_PRIMARY).  PNRT_E_STATE before pnrt_upload_scene
 * or pnrt_set_frame.  The buffers are allocated by the first call. */
int pnrt_render_guides(pnrt_ctx* ctx);
/* Synchronise and copy one guide image, width*height*4 floats (row 0 = bottom), to
 * the host.  PNRT_E_STATE before pnrt_render_guides, or when the frame size has
 * changed since.  Only the size is checked: guide images that a scene edit, a camera
 * move or a mode change left stale are still handed out, as they were rendered. */
int pnrt_read_aov(pnrt_ctx* ctx, int which, float* rgba_out);
/* Device pointer of a guide image (NULL before the first pnrt_render_guides). */
void* pnrt_aov_device_ptr(pnrt_ctx* ctx, int which);

/* Ray queries (not in the reference, whose only caller of BVHIntersect / BVHIntersectP
 * is its shader, ray_tracing.comp:429-494): the closest hit, or any hit, of caller
 * rays against the uploaded scene -- picking (which material is under this pixel, for
 * pnrt_update_materials), visibility and probe rays.  The traversal is the renderer's:
 * the same visit order, `>` tie rule (a later triangle at an equal distance wins) and
 * traversal mode (pnrt_set_options), so a query sees what a rendered ray would.
 *   rays7: n rays of 7 floats -- origin, direction, tMax -- 28 bytes apart.  The
 * direction need not be normalised (time is in its units) and any tMax is taken as
 * it is (tMax <= 0 hits nothing).  A ray with a float that is not finite, or with a
 * direction of three zeros, is invalid: it is not traced and its record says so.
 *   Rays are traced in the caller's order, 64 neighbours to a wavefront: coherent
 * neighbours trace faster.
 *   out: one 64-byte record per ray, words (floats as their bits):
 *     0      hit: 1 or 0
 *     1-3    position      4-6  normal (facing the ray, normalised)    7-8  texcoord
 *     9      textureId (int32, -1 none)     10  materialId (int32)     11   time
 *            -- words 1-11 are 0 without a hit, and for PNRT_QUERY_ANY
 *     12     the ray's tMax afterwards: time on a closest hit, else as given
 *     13     int32: the accepted triangle's index in the uploaded `triangles` array
 *            (PNRT_QUERY_ANY: the triangle that ended the ray), -1 without a hit
 *     14     flags: bit 0 = invalid ray (then every other word is 0, word 13 is -1)
 *     15     0
 * A query reads the scene only: the accumulation image, the moments, the guide
 * images and the records pnrt_render keeps of the camera rays stay as they are, and
 * pnrt_set_frame is not needed.  Its launches are timed as class PNRT_K_PRIMARY (as
 * the guide images' own trace launch is).
 *   PNRT_E_ARG: a kind other than the two, n < 0, a NULL pointer with n > 0.
 * PNRT_E_STATE before pnrt_upload_scene.  n == 0 returns PNRT_OK and queues nothing. */
#define PNRT_QUERY_CLOSEST 0
#define PNRT_QUERY_ANY     1
typedef struct { uint32_t w[16]; } pnrt_hit;   /* 64 bytes, layout above */
/* Host arrays: copies the rays in (through buffers the context grows), queries,
 * copies the records out and synchronises.  PNRT_E_TRACE as pnrt_read_accum returns it. */
int pnrt_query_rays(pnrt_ctx* ctx, const float* rays7, int64_t n, int kind, pnrt_hit* out);
/* Device arrays (rays7_dev 4-byte aligned; out_dev 16-byte aligned, else PNRT_E_ARG):
 * asynchronous on the context's stream, ordered after everything already queued there. */
int pnrt_query_rays_device(pnrt_ctx* ctx, const void* rays7_dev, int64_t n, int kind, void* out_dev);

/* The denoised preview: the edge-avoiding a-trous wavelet filter (Dammertz et al.
 * 2010) over the accumulation image divided by max(albedo, 1/256), guided by the
 * normal and position images, multiplied by the albedo again -- a second image
 * beside the accumulation image, which is read and never written.  `levels`
 * passes (1..5); pass i = 0.. takes the 5x5 B3-spline taps at spacing 2^i, a tap
 * weighing h * exp2(-(|dc|^2 / (sigma_color * 2^-i)^2 + |dn|^2 / sigma_normal^2 +
 * |dp|^2 / sigma_position^2)); taps outside the image are skipped.  Misses and
 * hits on emissive materials pass through: their pixels are the accumulation's,
 * bit for bit, and they weigh 0 as taps.  Alpha is 1 elsewhere.  The result is
 * defined bit for bit.
 * Asynchronous on the stream: ordered after the blends of the pnrt_render calls
 * already issued, and later calls are ordered after it.
 * params == NULL: levels 5, sigma_color 2, sigma_normal 0.25, sigma_position 0.5.
 * PNRT_E_ARG: levels outside 1..5, a sigma that is not finite and > 0 (the denoised
 * image is left as it was).  PNRT_E_STATE: no guide images, or guide images that
 * were rendered for another camera, frame size, scene (pnrt_upload_scene,
 * pnrt_update_materials, pnrt_upload_texture, pnrt_upload_env*) or traversal mode
 * -- call pnrt_render_guides again.  PNRT_E_TRACE as pnrt_pack_rows returns it. */
typedef struct {
    int levels;
    float sigma_color, sigma_normal, sigma_position;
} pnrt_denoise_params;
int pnrt_denoise(pnrt_ctx* ctx, const pnrt_denoise_params* params);
/* Synchronise and copy the denoised image (width*height*4 floats, row 0 = bottom). */
int pnrt_read_denoised(pnrt_ctx* ctx, float* rgba_out);
/* Device pointer of the denoised image (NULL before the first pnrt_denoise; the
 * same pointer after every call at one frame size). */
void* pnrt_denoised_device_ptr(pnrt_ctx* ctx);

/* The variance-guided denoised preview: the same a-trous filter, guide images,
 * pass-through rule and output image as pnrt_denoise, with the edge-stopping
 * function of SVGF (Schied et al. 2017, section 4.4) in place of the global
 * sigma_color.  A variance image is filtered alongside the colour; it starts as the
 * variance of the mean luminance from the sample moments, in albedo-demodulated
 * units, (M2 / (n - 1)) / n / lum(max(albedo, 1/256))^2, and as lum(c)^2 for an
 * unmeasured pixel (n < 2).  In pass i a tap weighs
 *   h * exp2(-(|lum(c_tap) - lum(c_centre)| / (sigma_variance * sqrt(g) + 2^-20)
 *              + |dn|^2 / sigma_normal^2 + |dp|^2 / sigma_position^2))
 * with g the 3x3 (1/4, 1/2, 1/4)^2 average, at unit spacing, of the variance around
 * the centre, and the variance becomes sum(w^2 v) / (sum w)^2.  sigma_variance counts
 * standard errors of the centre pixel and is not scaled per pass: a converged pixel
 * is barely touched, a noisy one is smoothed hard.  Defined bit for bit (DESIGN.md
 * section 24).  The filtered variance is not exposed.
 * Writes the image pnrt_denoise writes: pnrt_read_denoised and
 * pnrt_denoised_device_ptr serve both, the pointer is the same, and the image
 * holds whichever filter ran last.  The accumulation and moments images are read
 * and never written.  Asynchronous on the stream, ordered as pnrt_denoise.
 * params == NULL: levels 5, sigma_variance 4, sigma_normal 0.25, sigma_position 0.5.
 * (4 is the paper's sigma_l; it is not tuned here.)
 * PNRT_E_ARG: levels outside 1..5, a sigma that is not finite and > 0 (the denoised
 * image is left as it was).  PNRT_E_STATE: the sample moments were never enabled, or
 * frames were rendered while they were disabled so that they do not cover the
 * accumulation (as pnrt_render_adaptive refuses it); then every case of
 * pnrt_denoise.  PNRT_E_TRACE as pnrt_pack_rows returns it. */
typedef struct {
    int levels;
    float sigma_variance, sigma_normal, sigma_position;
} pnrt_denoise_variance_params;   /* 16 bytes */
int pnrt_denoise_variance(pnrt_ctx* ctx, const pnrt_denoise_variance_params* params);

/* Per-pixel sample moments and a convergence measure (not in the reference, which
 * counts frames: main.cpp:628).  Opt-in: while enabled, the blend of every
 * pnrt_render batch also folds the batch's per-frame colours into a moments image,
 * one 16-byte record per pixel, width*height records, row 0 = bottom:
 *   x = running mean of the luminance    y = M2, the sum of squared deviations
 *   z = 0 (reserved)                     w = n, the frames folded in, as uint32 bits
 * For each frame, in frame order, with the frame's colour c:
 *   Y = ((0.2126f * c.x) + (0.7152f * c.y)) + (0.0722f * c.z)
 *   frame number 0: n = 0, mean = 0, M2 = 0 first (frame 0 overwrites the accumulation)
 *   n = n + 1 (saturating);  d = Y - mean;  mean = mean + d * (1.0f / (float)n);
 *   M2 = M2 + d * (Y - mean)
 * The accumulation image, the launch count and the profile classes are the same with
 * and without (the blend-with-moments kernel is timed as PNRT_K_BLEND); a context
 * that never enables them launches what it always did.
 *
 * on = 1 / 0 (anything else PNRT_E_ARG).  Waits for the calls in flight.  The first
 * enable allocates the image, zeroed (with the frame, when pnrt_set_frame comes
 * later); enabling again keeps the data; disabling stops the updates and keeps the
 * image.  From the first enable on, pnrt_reset_accum zeroes the moments and a size
 * change in pnrt_set_frame reallocates them zeroed.  While enabled, pnrt_render under
 * PNRT_KERNEL_V1 returns PNRT_E_STATE and queues nothing (the one-kernel path has no
 * per-frame colours). */
int pnrt_enable_moments(pnrt_ctx* ctx, int on);
/* Device pointer of the moments image (NULL before the first enable). */
void* pnrt_moments_device_ptr(pnrt_ctx* ctx);
/* Synchronise and copy the width*height*4 floats of the moments image (w: uint32
 * bits) to the host.  PNRT_E_STATE when moments were never enabled. */
int pnrt_read_moments(pnrt_ctx* ctx, float* rgba_out);
/* The per-pixel relative standard error of the mean, width*height floats, row 0 =
 * bottom: for n >= 2
 *   var = M2 / (float)(n - 1);  sem = sqrtf(var / (float)n);
 *   e = sem / fmaxf(mean, 1.0f / 256.0f);  e_c = (e <= 65535.0f) ? e : 65535.0f
 * (IEEE division and square root; the comparison also sends NaN to 65535), and +inf
 * for an unmeasured pixel (n < 2).  Synchronous.  PNRT_E_STATE as pnrt_read_moments. */
int pnrt_read_error(pnrt_ctx* ctx, float* out);
/* Statistics of e_c over the rows of a shard selector (as pnrt_pack_rows takes it).
 * Every field is an integer or a maximum, combined on the device with integer
 * atomics, so the result does not depend on the order the blocks finish in.
 * Statistics of disjoint selectors add up: sum the counts and sum_q16, take the
 * max of max_error and max_frames and the min of min_frames -- N ranks combine
 * their own rows' numbers. */
typedef struct {
    int64_t  n_pixels;      /* pixels of the selector's rows                         */
    int64_t  n_measured;    /* ... with n >= 2                                       */
    int64_t  n_above;       /* measured pixels with e_c > threshold                  */
    int64_t  sum_q16;       /* sum over measured pixels of (uint32)(e_c * 65536.0f)  */
    float    max_error;     /* max e_c over measured pixels, 0 when none             */
    uint32_t min_frames, max_frames;   /* n over all pixels of the rows, 0 when none */
    uint32_t reserved;      /* 0 */
} pnrt_convergence_stats;   /* 48 bytes */
/* Synchronous; a shard without rows gives all zeros.  threshold must be finite and
 * >= 0 (PNRT_E_ARG otherwise, as a bad selector).  PNRT_E_STATE when moments were
 * never enabled.  PNRT_E_TRACE as pnrt_read_accum returns it. */
int pnrt_convergence(pnrt_ctx* ctx, float threshold, int band_rows, int n_shards, int shard,
                     pnrt_convergence_stats* out);

/* Adaptive sampling (not in the reference, which renders every pixel every frame):
 * render frames first_frame .. first_frame + n_frames - 1 only for the pixels of the
 * selector's rows that have not converged.  The call waits for
 * the calls in flight (as pnrt_enable_moments does), then evaluates once, on the
 * moments image as it stands, with m = max(min_frames, 2):
 *   a pixel is active iff n < m || e_c > threshold
 * (n, e_c as pnrt_read_error computes them; an unmeasured pixel is active).  The mask
 * holds for all batches of the call.  Tiles are 8x8 over (x, local row) of the
 * selector; a tile is active iff one of its pixels is.
 *   An active pixel receives every frame of the call -- the colour pnrt_render would
 * produce for that pixel and frame, bit for bit -- folded in frame order: the moments
 * update of pnrt_enable_moments, and the accumulation blended with
 * a = 1.0f / (float)n, n the pixel's own count after the increment (pnrt_render uses
 * 1.0f / (float)(frame + 1); the same for a pixel that got every frame since frame 0).
 * An inactive pixel receives nothing: its accumulation and moments stay, bit for bit.
 *   PNRT_E_STATE, and nothing queued: before pnrt_upload_scene / pnrt_set_frame; the
 * moments never enabled or disabled; frames rendered by pnrt_render while the moments
 * were disabled since they were last zeroed together with the accumulation
 * (pnrt_reset_accum, a resize) or first enabled; PNRT_KERNEL_V1.  PNRT_E_ARG: a
 * threshold that is not finite and >= 0, a bad selector, first_frame + n_frames >
 * 0xFFFFFFFF.  PNRT_E_TRACE as pnrt_read_accum returns it.
 *   n_frames == 0 evaluates the mask, fills `out` and queues nothing; so does a call
 * without an active pixel.  After the mask step (one synchronisation) the call is
 * asynchronous on the stream, like pnrt_render.  The batch plan (pnrt_batch_plan's
 * rules) runs on 64 * n_active_tiles path slots per frame. */
typedef struct {
    int64_t  n_pixels;         /* pixels of the selector's rows                       */
    int64_t  n_active_pixels;  /* ... that this call renders                          */
    int64_t  n_tiles;          /* 8x8 tiles of the selector's rows (local-row tiling) */
    int64_t  n_active_tiles;   /* ... with at least one active pixel                  */
    uint32_t frames_per_batch, n_batches;   /* the plan the call ran (0, 0: nothing queued) */
} pnrt_adaptive_stats;         /* 40 bytes */
int pnrt_render_adaptive(pnrt_ctx* ctx, uint32_t first_frame, uint32_t n_frames,
                         float threshold, uint32_t min_frames,
                         int band_rows, int n_shards, int shard,
                         pnrt_adaptive_stats* out /* may be NULL */);
/* pnrt_render_adaptive over caller ray buffers: the conjunction of that call and
 * pnrt_render_rays.  The mask, the tiles, the waiting, the fold
 * of an active pixel's frames, the untouched inactive pixel, the moments-state and
 * PNRT_KERNEL_V1 refusals, n_frames == 0 and `out` are pnrt_render_adaptive's; the
 * colour of an active pixel is the one pnrt_render_rays would produce for that pixel,
 * frame and ray record, bit for bit (a "no ray" record: (0, 0, 0), folded like any
 * other), and the buffer, its rules, its read ordering, which set a batch's frame slot
 * reads, and what the call leaves alone (the pnrt_set_frame camera, the kept per-pixel
 * camera-ray records, the guide images) are pnrt_render_rays'.  The values of inactive
 * pixels' records do not matter: no result depends on them.  The batch plan runs on
 * 64 * n_active_tiles path slots per frame with pnrt_render_rays' 48 more bytes per
 * path, which PNRT_BATCH_BYTES caps; the ray launch is PNRT_K_PRIMARY, one per batch,
 * the other classes are pnrt_render_adaptive's.  PNRT_E_ARG, with nothing queued and
 * nothing changed: either call's argument errors. */
int pnrt_render_rays_adaptive(pnrt_ctx* ctx, uint32_t first_frame, uint32_t n_frames,
                              const void* rays_dev, int64_t frame_stride,
                              float threshold, uint32_t min_frames,
                              int band_rows, int n_shards, int shard,
                              pnrt_adaptive_stats* out /* may be NULL */);

/* Temporal reprojection (not in the reference, whose redraw starts the image again from
 * one sample: main.cpp:592-596): after a camera move, resample the accumulation and the
 * moments images from the view they were rendered with into the current one, so that the
 * frames rendered before the move still count (bit for bit).
 *   `from` is the camera the accumulation was rendered with; the current camera
 * (pnrt_set_frame) is the one to reproject into.  Frame size, scene and traversal mode
 * are the current ones: only the camera may differ.  Always the whole image: a context
 * that rendered a shard has no whole image to resample, and sharded or multi-GPU
 * reprojection is not provided.
 *   Every pixel of the new view whose camera ray hits is projected into `from`'s image
 * plane and takes the four bilinear taps there.  A tap counts only when it lies in the
 * image, hits the same material, has dot(n_tap, n) >= normal_min and
 * |P_tap - P|^2 <= (position_tolerance * |P - eye_from|)^2 (the guide images of both
 * views), and holds at least one frame.  The pixel receives the taps' normalised blend of
 * the colour, the mean luminance and the sample variance, and a frame count
 * n' = min(the taps' smallest count, max_history); a hit without a valid tap (a
 * disocclusion) and a primary miss start again at zero, colour and count.  The capped
 * count bounds the weight of what was carried -- biased wherever shading depends on the
 * view -- against the frames that follow.
 *   Continue with pnrt_render_adaptive(first_frame >= 1, ...): its blend weighs every
 * pixel by its own count, 1 / (float)n, so a disoccluded pixel takes the next frame whole
 * and a long history takes it lightly.  pnrt_render stays legal and blends with its
 * frame-number weight 1 / (float)(frame + 1), as ever, whatever the pixels' counts.
 *   The call waits for the calls in flight (as pnrt_render_adaptive does) and is
 * synchronous.  It needs the guide images of `from`: the current ones when they were
 * rendered for it, else it renders them first (as pnrt_render_guides would, lent records
 * included); their position and normal images are kept in two buffers of the context,
 * allocated by the first call like the two images the result is written through.  Then it
 * renders the guide images of the current camera: on return they are valid for it, and
 * pnrt_denoise* needs no pnrt_render_guides.  pnrt_accum_device_ptr,
 * pnrt_moments_device_ptr and pnrt_aov_device_ptr return what they returned before, the
 * moments still cover the accumulation, and the records pnrt_render keeps of the camera
 * rays are left alone.  Launches are timed as PNRT_K_PRIMARY (the guide traces) and
 * PNRT_K_BLEND (the reprojection kernel and the copies).
 *   PNRT_E_STATE, with nothing changed: before pnrt_upload_scene / pnrt_set_frame; the
 * moments never enabled, disabled, or not covering the accumulation (the rule of
 * pnrt_render_adaptive); PNRT_KERNEL_V1.  PNRT_E_ARG, with nothing changed: from NULL or
 * one of its 12 floats not finite; normal_min not finite or outside [-1, 1];
 * position_tolerance not finite or not > 0; max_history == 0; reserved != 0.
 * PNRT_E_TRACE as pnrt_read_accum returns it. */
typedef struct {
    float    normal_min;          /* a tap needs dot(n_tap, n) >= normal_min      */
    float    position_tolerance;  /* ... and |P_tap - P|^2 <= (tol * |P - eye_from|)^2 */
    uint32_t max_history;         /* n' is at most this (>= 1)                    */
    uint32_t reserved;            /* 0 */
} pnrt_reproject_params;          /* 16 bytes; NULL: 0.9, 0.02, 32 */
typedef struct {
    int64_t  n_pixels;            /* width * height                               */
    int64_t  n_reprojected;       /* pixels that received history (n' >= 1)       */
    int64_t  n_disoccluded;       /* hits in the new view without a valid tap     */
    int64_t  n_missed;            /* primary misses in the new view               */
    int64_t  sum_frames;          /* sum of n' over the image                     */
    uint32_t max_frames, reserved;
} pnrt_reproject_stats;           /* 48 bytes */
int pnrt_reproject(pnrt_ctx* ctx, const pnrt_camera* from,
                   const pnrt_reproject_params* params, pnrt_reproject_stats* out /* may be NULL */);

/* pnrt_reproject with both views given as camera models (bit for
 * bit): `from` is the view the accumulation was rendered with, `to` the view to continue
 * in.  Each view is the centre rays of its model -- what pnrt_make_rays writes for it with
 * aa_width 0 and lens_radius 0, the same for every frame.  aa_width, lens_radius,
 * focus_distance and per_pixel are validated as pnrt_make_rays validates them and otherwise
 * ignored.  The pnrt_set_frame camera is ignored and stays current; frame size, scene and
 * traversal mode are the current ones.  Whole image, synchronous: the call waits for the
 * calls in flight, as pnrt_reproject does.
 *   Every pixel of `to` whose centre ray hits is mapped into `from`'s image by the inverse
 * of `from`'s model -- the pinhole's image-plane algebra (pnrt_reproject's), the
 * orthographic projection, or the direction's angles (PN-libm's atan2) for the
 * equirectangular and the fisheye view -- and takes pnrt_reproject's four bilinear taps
 * there, with its validity tests, its blend, its capped count and its statistics.  The
 * position test measures against |P - eye_from|, the orthographic view against P's depth
 * along the view direction.  An equirectangular `from` wraps in x: a point beyond column
 * width - 1 takes its right taps from column 0 (rows do not wrap).  A pixel of `to` without
 * a ray (a fisheye's corners) is a primary miss: counted in n_missed, started at zero.  A
 * pixel of `from` without a ray holds no history: a tap on it is invalid.
 *   The call makes the centre rays of `from` in a buffer of the context (width * height
 * records, allocated by the first call; one pnrt_make_rays launch, PNRT_K_BLEND), renders
 * their guide images as pnrt_render_guides_rays does (one PNRT_K_PRIMARY launch) and keeps
 * the position and normal images as the history; then the same for `to`.  Guide images
 * made from rays carry no camera, so the library cannot tell that the current ones belong
 * to `from`: both views' are always rendered -- no lent records, no key match.  On return
 * the guide images are what pnrt_make_rays(to's centre rays) and pnrt_render_guides_rays
 * leave, bit for bit, valid under that call's rules: pnrt_denoise* needs no further call.
 * pnrt_accum_device_ptr, pnrt_moments_device_ptr and pnrt_aov_device_ptr return what they
 * returned before, the moments still cover the accumulation, and the kept per-pixel
 * camera-ray records are left alone.  Continue with pnrt_render_rays_adaptive (threshold
 * 0, min_frames 0xFFFFFFFF: every pixel, each at its own count's weight).
 *   PNRT_E_STATE and the `params` errors are pnrt_reproject's; PNRT_E_ARG for from or to
 * NULL and for every argument rule of pnrt_make_rays broken by either (the message names
 * which of the two); PNRT_E_TRACE as pnrt_read_accum returns it.  A refusal changes
 * nothing.
 *   Not provided: a from / to given as ray buffers (an arbitrary ray set has no inverse);
 * sample-aware reprojection (jitter, lens); sharded or multi-GPU reprojection; reuse or
 * lending of guide records for model views. */
int pnrt_reproject_view(pnrt_ctx* ctx, const pnrt_ray_camera* from, const pnrt_ray_camera* to,
                        const pnrt_reproject_params* params, pnrt_reproject_stats* out /* may be NULL */);

/* The display transform (not in the reference, whose render.frag shows the clamped
 * accumulation, and whose GL blit stays out of scope): one of the context's float
 * images to an 8-bit RGBA image on the device, with an exposure, a tone curve and a
 * transfer function, so that a displayed frame copies width*height*4 bytes to the
 * host instead of width*height*16 -- or none, through pnrt_display_device_ptr.
 * Defined bit for bit; every product and sum below is rounded
 * on its own.  For source pixel (x, y), row 0 = bottom, and each of r, g, b:
 *   v = c * exposure;  s = (v > 0.0f) ? v : 0.0f   (NaN, negatives and -0 give +0)
 *   s = fminf(s, 65536.0f)
 *   PNRT_TONE_CLAMP     t = s
 *   PNRT_TONE_REINHARD  w2 = white * white;  t = (s * (1.0f + s / w2)) / (1.0f + s)
 *   PNRT_TONE_ACES      t = (s * (2.51f * s + 0.03f)) / (s * (2.43f * s + 0.59f) + 0.14f)
 *   t = fminf(t, 1.0f)
 *   PNRT_TRANSFER_LINEAR  u = t
 *   PNRT_TRANSFER_SRGB    u = (t <= 0.0031308f) ? 12.92f * t : 1.055f * pow(t, e) - 0.055f,
 *                         u = fminf(u, 1.0f); e the float 0x3ED55555 (1.0f / 2.4f), pow the
 *                         library's own PN-libm pow (pnrt_debug_math fn 5)
 *   q = (uint8_t)floorf(u * 255.0f + 0.5f)
 * and alpha = 255.  The pixel goes to row height - 1 - y of the display image (top row
 * first, as a PNG has it), or to row y with bottom_first = 1.  With params == NULL this
 * is the reference's display: clamp, no gamma, top row first.
 *   Asynchronous on the context's stream: ordered after the blends and filters already
 * queued, and later calls that write the source are ordered after it (the rule of
 * pnrt_denoise).  Reads its source and writes only the display image -- one RGBA8 image,
 * allocated by the first call and again when the frame size has changed; the pointer is
 * the same after every call at one frame size.  Launches are timed as PNRT_K_BLEND.
 *   With an error nothing is queued and the display image is left as it was.
 * PNRT_E_STATE: before pnrt_set_frame; PNRT_DISPLAY_DENOISED when no pnrt_denoise* has
 * run at this frame size.  PNRT_E_ARG: an unknown source, tone or transfer; bottom_first
 * not 0 or 1; exposure or white not finite or not > 0; PNRT_DISPLAY_EXTERNAL with a NULL
 * or misaligned src_device.  PNRT_E_TRACE as pnrt_pack_rows returns it. */
#define PNRT_DISPLAY_ACCUM    0   /* the accumulation image                          */
#define PNRT_DISPLAY_DENOISED 1   /* the image pnrt_denoise / pnrt_denoise_variance wrote */
#define PNRT_DISPLAY_EXTERNAL 2   /* src_device: width*height float4, row 0 = bottom, 16-byte aligned
                                     (e.g. the gathered multi-GPU frame on rank 0)   */
#define PNRT_TONE_CLAMP    0      /* the reference's display (render.frag: none)     */
#define PNRT_TONE_REINHARD 1      /* extended Reinhard per channel, white point `white` */
#define PNRT_TONE_ACES     2      /* Narkowicz's fitted ACES curve per channel       */
#define PNRT_TRANSFER_LINEAR 0    /* the reference's (no gamma)                      */
#define PNRT_TRANSFER_SRGB   1    /* the piecewise sRGB encoding                     */
typedef struct {
    int   source, tone, transfer, bottom_first;   /* bottom_first 0: top row first, as to_display and PNG */
    float exposure, white;
    const void* src_device;                       /* read only for PNRT_DISPLAY_EXTERNAL, else ignored */
} pnrt_display_params;            /* 32 bytes; NULL: ACCUM, CLAMP, LINEAR, top first, exposure 1, white 4 */
int pnrt_display(pnrt_ctx* ctx, const pnrt_display_params* params);
/* Synchronise and copy the width*height*4 bytes of the display image to the host.
 * PNRT_E_STATE before the first pnrt_display, or when the frame size has changed since. */
int pnrt_read_display(pnrt_ctx* ctx, uint8_t* rgba8_out);
/* Device pointer of the display image (NULL before the first pnrt_display). */
void* pnrt_display_device_ptr(pnrt_ctx* ctx);

/* Auto exposure: a histogram of the luminance of a display source over the rows of a
 * shard selector (as pnrt_pack_rows takes it), and the exposure derived from it.
 *   Y = ((0.2126f * c.x) + (0.7152f * c.y)) + (0.0722f * c.z) of the unexposed colour; a
 * pixel is counted iff Y > 0 and Y is finite, in bin
 *   clamp((int)(bits(Y) >> 19) - 1776, 0, 511)
 * -- 16 bins per octave from the exponent and the top four mantissa bits, 2^-16 .. 2^16,
 * 1.0 in bin 256, no libm.  n_pixels counts all pixels of the rows.  Every field is an
 * integer combined with integer atomics, so the result does not depend on the order the
 * blocks finish in, and histograms of disjoint selectors add up field by field (N ranks
 * combine their own rows').  Synchronous; a shard without rows gives zeros.  The source
 * is only read; the kernel is timed as PNRT_K_BLEND.  Errors as pnrt_display's for the
 * source, and PNRT_E_ARG for a bad selector or a NULL `out`. */
#define PNRT_LUMA_BINS 512
typedef struct { int64_t n_pixels, n_counted; int64_t bins[PNRT_LUMA_BINS]; } pnrt_luma_histogram; /* 4112 bytes */
int pnrt_luma_histogram_read(pnrt_ctx* ctx, int source, const void* src_device,
                             int band_rows, int n_shards, int shard, pnrt_luma_histogram* out);
/* Host only, no context: the exposure that brings the trimmed mean bin to `key`, in
 * integer arithmetic.  N = n_counted; lo = N * low_permille / 1000, hi = N * high_permille
 * / 1000; with cum_b the running sum of the bins, bin b contributes
 * cnt_b = max(0, min(cum_b, hi) - max(cum_(b-1), lo)); S = sum cnt_b * b, C = sum cnt_b.
 * C == 0: exposure 1.  Otherwise m = (2S + C) / (2C), k = 256 - m, e = floor(k / 16),
 * j = k - 16e, exposure = key * ldexpf(T[j], e) with T[j] the float nearest 2^(j/16): a
 * 1/16-stop grid, which also keeps the exposure from flickering frame to frame.
 * PNRT_E_ARG: a NULL pointer, permille outside 0 <= low < high <= 1000, key not finite
 * or not > 0. */
int pnrt_exposure_from_histogram(const pnrt_luma_histogram* hist, int low_permille, int high_permille,
                                 float key, float* exposure_out);

/* Per-kernel timing (not in the reference, which has no GPU timers): while
 * enabled, every launch of a kernel class is bracketed by HIP events recorded on
 * the launch stream; pnrt_profile_read synchronises and returns the summed
 * event durations (ms) and launch counts.  Enabling (or disabling) resets. */
#define PNRT_K_PRIMARY 0   /* primary hits, one trace per pixel per render call; ray queries */
#define PNRT_K_GEN 1       /* path state for the call's frames                  */
#define PNRT_K_SETUP 2     /* per bounce: sampling + speculative BSDF, shadow rays */
#define PNRT_K_TRACE 3     /* per bounce: persistent BVH traversal of all rays  */
#define PNRT_K_SHADE 4     /* per bounce: MIS + continuation                    */
#define PNRT_K_BLEND 5     /* progressive mean into the accumulation image      */
#define PNRT_K_V1 6        /* PNRT_KERNEL_V1 single-kernel path                 */
#define PNRT_K_COUNT 7
typedef struct {
    double ms[PNRT_K_COUNT];
    int64_t launches[PNRT_K_COUNT];
} pnrt_profile;
int pnrt_profile_enable(pnrt_ctx* ctx, int on);
int pnrt_profile_read(pnrt_ctx* ctx, pnrt_profile* out);
/* Kernel classes bracketed while profiling is enabled: bit k = PNRT_K_k (default
 * all).  Timing only the dominant class keeps the event records off the other
 * launches (each record is a queue packet between kernels). */
int pnrt_profile_select(pnrt_ctx* ctx, int class_mask);

/* GPU BuildBVH: the reference's binned-SAH build
 * (include/BVH.hpp:92-173, called from the BVH ctor :16-19 via main.cpp's
 * scene setup) run on the device, returning the SAME node array (pre-order,
 * main.cpp:488-501 layout, 12 floats per node) and the SAME triangle order as
 * the host build, bit for bit.  Input per triangle, in the current order: its
 * Bound and boundCenter (triangle.hpp:11-12) as 9 floats pMin.xyz pMax.xyz
 * centre.xyz.  Output: order_out[i] = input index of the triangle at BVH
 * position i; nodes_out needs room for 2 * n_triangles - 1 nodes.  Stateless
 * with respect to the scene (the caller packs and uploads as usual).  Bounds
 * must be finite; synchronous. */
int pnrt_bvh_build(pnrt_ctx* ctx, const float* tri_bounds9, int n_triangles, float* nodes_out,
                   int node_capacity, int* n_nodes_out, int32_t* order_out, int* max_depth_out);

/* Test hook: evaluate one PN-libm / IEEE primitive on the device (same fn
 * codes as the oracle's pno_math_eval); host in/out arrays of n floats. */
int pnrt_debug_math(pnrt_ctx* ctx, int fn, const float* a, const float* b, float* out, int n);

#ifdef __cplusplus
}
#endif
#endif
