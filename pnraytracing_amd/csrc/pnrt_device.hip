// pnraytracing_amd/csrc/pnrt_device.hip -- libpnrt.so: C ABI (include/pnrt.h),
// scene re-layout and the gfx950 radiance-integrator kernel that replaces
// PnRayTracing's shaders/ray_tracing.comp.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-fast-math
//        -fPIC -shared  (pnraytracing_amd/build.py)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pnrt.h"

#include "pt_path.h"
#include "pt_wf.h"
#include "pt_env.h"
#include "pt_bvh.h"
#include "pt_denoise.h"
#include "pt_moments.h"
#include "pt_denoise_var.h"
#include "pt_adaptive.h"
#include "pt_query.h"
#include "pt_reproject.h"
#include "pt_reproject_view.h"
#include "pt_display.h"
#include "pt_refit.h"
#include "pt_place.h"
#include "pn_glm.h"
#include "pt_cameras.h"
#include "pt_rays.h"

__global__ void pt_pack_rows_kernel(const float4* accum, float4* dst, int width, int rows, int band,
                                    int n_shards, int shard) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t total = (size_t)rows * width;
    if (i >= total) return;
    int r = (int)(i / width), x = (int)(i - (size_t)r * width);
    int y = shard_row(r, band, n_shards, shard);
    dst[i] = accum[(size_t)y * width + x];
}

// the inverse of pt_pack_rows_kernel: a shard's packed rows into their image rows
__global__ void pt_unpack_rows_kernel(const float4* src, float4* img, int width, int rows, int band, int n_shards,
                                      int shard) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t total = (size_t)rows * width;
    if (i >= total) return;
    int r = (int)(i / width), x = (int)(i - (size_t)r * width);
    int y = shard_row(r, band, n_shards, shard);
    img[(size_t)y * width + x] = src[i];
}

__global__ void pt_math_kernel(int fn, const float* a, const float* b, float* out, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x = a[i], y = b[i], r;
    uint32_t u;
    switch (fn) {
    case 0: r = pnm_sin(x); break;
    case 1: r = pnm_cos(x); break;
    case 2: r = pnm_atan2(x, y); break;
    case 3: r = pnm_asin(x); break;
    case 4: r = pnm_log(x); break;
    case 5: r = pnm_pow(x, y); break;
    case 6: r = pnm_exp2(x); break;
    case 7: r = sqrtf(x); break;
    case 8: r = x / y; break;
    case 9: u = __float_as_uint(x); r = (float)u; break;
    case 10: u = __float_as_uint(x); wang_hash(u); r = __uint_as_float(u); break;
    default: r = pnm_nan(); break;
    }
    out[i] = r;
}

// =====================================================================================
// host side
// =====================================================================================
static int set_err(pnrt_ctx* c, int code, const std::string& m);
static hipError_t sync_all(pnrt_ctx* c);
#define HIPCHK(ctx, expr)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return set_err(ctx, PNRT_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

namespace {
// A device allocation (Pinned: a pinned host one) and its capacity in bytes, freed with its
// owner.  Move-only; reads as the pointer it holds.
template <class T, bool Pinned = false>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }
    operator T*() const { return p; }
    void reset() {
        if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
    // a fresh block of exactly `bytes` in place of the old one, whose readers the caller has waited for
    hipError_t alloc(size_t bytes, unsigned pinned_flags = hipHostMallocDefault) {
        reset();
        const hipError_t e = Pinned ? hipHostMalloc((void**)&p, bytes, pinned_flags) : hipMalloc((void**)&p, bytes);
        if (e == hipSuccess) cap = bytes;
        else p = nullptr;
        return e;
    }
    // at least `bytes`, kept across calls; *moved: the block is another one now
    int reserve(pnrt_ctx* c, size_t bytes, bool* moved = nullptr) {
        if (cap >= bytes) return 0;
        if (p) (void)sync_all(c);          // the old buffer may still be in use by calls in flight
        if (moved) *moved = true;
        HIPCHK(c, alloc(bytes));           // (a failure leaves no buffer and no capacity)
        return 0;
    }
};
template <class T> using PinnedBuf = DevBuf<T, true>;
}  // namespace

struct pnrt_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    // trace faults (pt_wf.h wf_fault): WF_FAULT_WORDS words in host-mapped memory the
    // kernels write only when a check trips; `faulted` latches until reset_accum
    PinnedBuf<uint32_t> fault_host;
    uint32_t* fault_dev = nullptr;         // the device's address of fault_host
    bool faulted = false;
    std::string fault_msg;
    // scene
    std::vector<DevBuf<void>> scene_allocs;
    DevScene scene{};
    bool has_scene = false;
    int max_depth = 0, n_interior = 0, root_is_leaf = 0;
    int64_t scene_bytes = 0;
    std::vector<int> light_mat;            // material of each light record's triangle (pnrt_update_materials)
    std::vector<float4> light_rec_host;    // host copy of the light records (patched, then one upload)
    std::vector<float> mat_emit;           // host copy of every material's emission (3 floats each)
    std::vector<int> light_tri;            // triangle of each uploaded light entry (pnrt_update_vertices checks them)
    std::vector<int> level_off;            // interior nodes of tree level d are indices level_off[d] .. level_off[d + 1] - 1
    float env_max = 0.f;                   // largest |texel| component of the env image (NaN: a NaN texel)
    // env + textures
    DevBuf<float4> hdr, rnd;
    DevBuf<float4> hdr_q, rnd_q;    // footprint records of both (DevScene::hdr_q)
    DevBuf<uint32_t> tex[PT_MAX_TEXTURES];
    int tex_w[PT_MAX_TEXTURES] = {}, tex_h[PT_MAX_TEXTURES] = {};
    DevBuf<float> unorm8;
    // frame
    int width = 0, height = 0, max_bounce = 4;
    pnrt_camera cam{};
    bool has_frame = false;
    DevBuf<float4> accum;
    int mode = PNRT_TRAVERSE_ZCULL;
    bool boxes_finite = true;              // every BVH box coordinate finite: z-slab culling allowed (pt_wf.h box_slabs)
    int kernel = 3;                        // 3 = wavefront (default), 1 = v1 one-lane-per-pixel
    bool serial = false;                   // PNRT_SERIAL: one call in flight, full trace grid (measurement)
    // Pipelined wavefront rendering.  pnrt_render calls rotate over the pipes -- the
    // first WF_PIPES_LARGE of them, or all WF_PIPES for small calls (a multi-GPU
    // rank's share: its kernels are short, so a fourth call in flight fills the
    // gaps of the other three's dependent chains; measured at N = 8).  A pipe is its own
    // worker stream and primary / colour / path buffers, so call k+1 starts
    // while call k's kernels drain (one call's kernels fill the CUs the other's
    // trace kernel leaves idle while its last rays drain).  Only the blends are
    // ordered: they run in call order on the context stream, which therefore
    // sees each call's finished image.  The fourth pipe (small calls only) is
    // created only when the process has more than 4 hardware queues
    // (GPU_MAX_HW_QUEUES, HIP's default 4): with 4, its worker would share the
    // context stream's queue and serialise behind the blends, so small calls
    // rotate over the first three like large ones (n_pipes_small).
    // (Splitting a call into two concurrent half-batches on two worker streams
    // as well measured slower: 1 006 vs 1 105 Msamples/s.)
    struct PrimKey {        // what a pipe's primary records were traced for (render_wavefront)
        uint64_t epoch = 0; // scene_epoch at the time
        float cam[12] = {};
        int width = 0, height = 0, rows = 0, band = 0, n_shards = 0, shard = 0, mode = -1;
        bool valid = false;
    };
    struct Pipe {
        hipStream_t w = nullptr;
        hipEvent_t ev_join = nullptr, ev_blend = nullptr;
        hipEvent_t ev_stage = nullptr;   // WF_STAGGER: the call has reached its drain-heavy end
        hipEvent_t ev_rays = nullptr;    // pnrt_render_rays: the context stream at the time of the call
        bool stage_set = false;
        DevBuf<float4> primary;
        PrimKey prim;
        DevBuf<float4> colors;
        DevBuf<char> wf;
        DevBuf<uint2> ovf;
        bool blend_pending = false;  // ev_blend guards the colour buffer's last reader
        // pnrt_render_cameras / pnrt_render_rays: the batch's camera-ray record per path slot; the camera table
        DevBuf<float4> camrec;
        DevBuf<float> camtab;
    };
    Pipe pipe[WF_PIPES];
    unsigned n_pipes_small = WF_PIPES;     // pipes small calls rotate over (pipes_init)
    size_t batch_bytes_cap = 0;            // PNRT_BATCH_BYTES: device bytes of one batch's buffers at most (0: none)
    unsigned last_pipe = 0;                // the pipe of the last call
    // bumped by every change of what the primary records depend on besides the
    // frame (camera, size, shard, traversal mode: compared per call): the scene
    // arrays, the materials (emission) and the environment (a miss's colour)
    uint64_t scene_epoch = 1;
    hipEvent_t ev_last = nullptr;          // recorded after every op the context queues on `stream`, so a
    bool last_valid = false;               // pnrt_set_stream orders the new stream after it without
                                           // touching the old stream (which the caller may have destroyed)
    bool pipes_ready = false;
    uint64_t ncall = 0;
    unsigned next_pipe = 0;
    int trace_grid = 0;
    int trace_grid_cc = 0;     // full occupancy of the lone calls' trace instantiation (WF_TRACE_WAVES_CC)
    int wf_stack_need = 0;                 // wide-traversal stack entries per lane (from upload)
    // per-kernel-class HIP event timing (pnrt_profile_enable / pnrt_profile_read)
    bool prof_on = false;
    int prof_mask = -1;     // kernel classes bracketed while profiling (pnrt_profile_select)
    std::vector<hipEvent_t> ev_pool;
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> ev_pending;
    double prof_ms[PNRT_K_COUNT] = {};
    int64_t prof_n[PNRT_K_COUNT] = {};
    // guide images and the denoised preview (pnrt_render_guides / pnrt_denoise): every
    // buffer is allocated on first use, so a context that never asks holds none
    struct GuideKey {       // what the guide images were rendered for
        uint64_t epoch = 0, tex_epoch = 0;
        float cam[12] = {};
        int width = 0, height = 0, mode = -1;
        bool valid = false;
        bool rays = false;  // rendered from a caller's ray set (pnrt_render_guides_rays): they carry no camera
    };
    uint64_t tex_epoch = 1;                // bumped by pnrt_upload_texture (the albedo image reads the textures)
    DevBuf<float4> aov[PNRT_AOV_COUNT];
    GuideKey guide_key;
    DevBuf<float4> g_primary;              // records of the guides' own trace, when no
    PrimKey g_prim;                        // pipe holds the full image's
    DevBuf<uint2> g_ovf;                   // ... and its stack spill area
    DevBuf<float4> dn_guide;               // compact guide records (pt_denoise.h)
    DevBuf<float4> dn_img[2];              // [0] the denoised image, [1] its ping-pong partner
    int dn_width = 0, dn_height = 0;       // size of the denoised image (0: none yet)
    // per-pixel sample moments (pnrt_enable_moments; pt_moments.h): none until the first enable
    bool moments_on = false;               // the blends update them
    bool moments_ever = false;             // enabled at least once: the image follows the frame size from then on
    DevBuf<float4> moments;                // width * height records, as the accumulation image
    DevBuf<float> mom_err;                 // pnrt_read_error's image
    DevBuf<MomentsStats> mom_stats;        // pnrt_convergence's device record
    // adaptive sampling (pnrt_render_adaptive; pt_adaptive.h): none until the first call
    bool mom_cover = false;                // the moments count every frame the accumulation holds
    DevBuf<unsigned long long> ad_masks;   // per tile of the selector's rows: activity mask,
    DevBuf<int> ad_flags, ad_offs;         // "any pixel active" and its exclusive scan
    DevBuf<WfTile> ad_list;                // the active-tile list
    DevBuf<AdaptCounts> ad_counts;         // the counts the host reads back
    // ray queries (pnrt_query_rays; pt_query.h): none until the first call
    DevBuf<uint2> q_ovf;                   // the query kernel's stack spill area
    DevBuf<float> q_rays;                  // the host form's staging buffers: rays in,
    DevBuf<uint4> q_out;                   // records out
    // temporal reprojection (pnrt_reproject; pt_reproject.h): none until the first call
    DevBuf<float4> rp_pos, rp_nrm;         // the history: position and normal images of the view the
                                           // accumulation was rendered with
    DevBuf<float4> rp_acc, rp_mom;         // the resampled accumulation and moments, before they are
                                           // copied over the images themselves
    DevBuf<ReprojectCounts> rp_counts;     // the counts the host reads back
    DevBuf<float4> rp_rays;                // pnrt_reproject_view: the centre rays of one view, then of the other
    // the display transform (pnrt_display; pt_display.h): none until the first call
    DevBuf<uint32_t> disp;                 // the RGBA8 display image
    int disp_width = 0, disp_height = 0;   // its size (0: none yet)
    DevBuf<LumaHist> luma_hist;            // pnrt_luma_histogram_read's device record
    // in-place geometry edits (pnrt_update_vertices; pt_refit.h): none until the first call
    DevBuf<float> rf_stage;                // the host form's staging buffer: vertex records in
    DevBuf<RefitResult> rf_res;            // the root box and the non-finite flag the host reads back
    // models placed by a matrix (pnrt_define_model, pnrt_place_models; pt_place.h): none until the first
    // definition; forgotten, their copies freed, with the scene
    struct PlaceModel {
        int first = 0, count = 0;          // the model's vertex range
        DevBuf<float4> rec;                // its model-space records, two float4 per vertex
    };
    std::vector<PlaceModel> models;        // the index is the model's id
    DevBuf<PlaceEntry> pl_table;           // a call's placement table, PLACE_MAX entries
    // per-frame cameras (pnrt_render_cameras; pt_cameras.h): none until the first call.  A call's array is
    // copied into a pinned staging block, from which each batch's table is copied to its pipe in stream
    // order; a block is reused once the event behind its call's last copy has completed
    struct CamStage {
        PinnedBuf<float> host;
        hipEvent_t ev = nullptr;
        bool pending = false;
    };
    std::vector<CamStage> cam_stage;
};

static int set_err(pnrt_ctx* c, int code, const std::string& m) {
    if (c) c->err = m;
    return code;
}

// PNRT_E_TRACE once a fault word is set by completed work (see pnrt.h)
static int check_fault(pnrt_ctx* c) {
    if (!c->faulted && c->fault_host) {
        static const char* what[WF_FAULT_WORDS] = {
            "a bounded wait of the trace kernel's block ray queue ran out",
            "a trace block loaded fewer rays than it dequeued",
            "a trace launch ended with ray-queue items never dequeued",
            "diagnostic bounds check: a fetch / store index out of range at site "};
        static const char* site[] = {"?", "node", "triangle", "leaf table", "stack spill", "trace result", "ray record",
                                     "hit attributes", "light record", "env footprint", "albedo texel", "primary record",
                                     "colour", "path state", "segment", "cooperative frontier", "active-tile list"};
        std::string m;
        for (int k = 0; k < WF_FAULT_WORDS; ++k) {
            const uint32_t v = __atomic_load_n(c->fault_host + k, __ATOMIC_ACQUIRE);
            if (!v) continue;
            m += (m.empty() ? "" : "; ") + std::string(what[k]);
            if (k == WF_FAULT_BOUNDS) m += std::string(v < sizeof site / sizeof *site ? site[v] : "?") + " (" + std::to_string(v) + ")";
        }
        if (!m.empty()) {
            c->faulted = true;
            c->fault_msg = "trace fault: " + m + " -- queued rays may be untraced, the accumulation image is "
                           "invalid (pnrt_reset_accum clears it)";
        }
    }
    return c->faulted ? set_err(c, PNRT_E_TRACE, c->fault_msg) : PNRT_OK;
}
// Record ev_last after an op queued on c->stream (see pnrt_set_stream).
static int mark_stream(pnrt_ctx* c) {
    HIPCHK(c, c->ev_last ? hipSuccess : hipEventCreateWithFlags(&c->ev_last, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->ev_last, c->stream));
    c->last_valid = true;
    return PNRT_OK;
}

// every stream the context launches on (the caller's / blend stream, the workers)
static hipError_t sync_all(pnrt_ctx* c) {
    hipError_t e = hipStreamSynchronize(c->stream);
    for (auto& P : c->pipe)
        if (e == hipSuccess && P.w) e = hipStreamSynchronize(P.w);
    return e;
}

// ---- event timing: a start/stop event pair around every launch of a class ----------------
static hipEvent_t ev_get(pnrt_ctx* c) {
    if (!c->ev_pool.empty()) { hipEvent_t e = c->ev_pool.back(); c->ev_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}
struct ProfScope {     // records on the launch stream, so it times exactly that stream's launches
    pnrt_ctx* c; int k; hipStream_t st; hipEvent_t a = nullptr;
    ProfScope(pnrt_ctx* c_, int k_, hipStream_t st_ = nullptr) : c(c_), k(k_), st(st_ ? st_ : c_->stream) {
        if (c->prof_on && ((c->prof_mask >> k) & 1) && (a = ev_get(c))) (void)hipEventRecord(a, st);
    }
    ~ProfScope() {
        if (!a) return;
        hipEvent_t b = ev_get(c);
        if (!b) { c->ev_pool.push_back(a); return; }
        (void)hipEventRecord(b, st);
        c->ev_pending.push_back({k, {a, b}});
    }
};
static int prof_collect(pnrt_ctx* c) {
    if (c->ev_pending.empty()) return PNRT_OK;
    HIPCHK(c, sync_all(c));
    for (auto& p : c->ev_pending) {
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, p.second.first, p.second.second));
        c->prof_ms[p.first] += ms;
        c->prof_n[p.first] += 1;
        c->ev_pool.push_back(p.second.first);
        c->ev_pool.push_back(p.second.second);
    }
    c->ev_pending.clear();
    return PNRT_OK;
}

#ifndef WF_MAX_CHUNK_FRAMES
#define WF_MAX_CHUNK_FRAMES 128  // frames per batch at most (bench.py's calls: 16 frames of a 1080p frame; a
                                 // multi-GPU rank's share: its timed steps in as few one-batch calls as fit --
                                 // 80 frames of a quarter / eighth at N = 4 / 8, profiles/r06/h/: +3 to +5 %)
#endif

static void free_scene(pnrt_ctx* c) {
    c->scene_allocs.clear();
    c->models.clear();
    c->has_scene = false;
}

// A new block of the scene's, freed with it.
static hipError_t scene_block(pnrt_ctx* c, size_t bytes, void** p) {
    c->scene_allocs.emplace_back();
    const hipError_t e = c->scene_allocs.back().alloc(bytes);
    *p = c->scene_allocs.back();
    return e;
}

template <class T>
static int upload(pnrt_ctx* c, const std::vector<T>& v, const T** out) {
    void* p = nullptr;
    size_t bytes = v.size() * sizeof(T);
    if (bytes == 0) { *out = nullptr; return 0; }
    HIPCHK(c, scene_block(c, bytes, &p));
    HIPCHK(c, hipMemcpy(p, v.data(), bytes, hipMemcpyHostToDevice));
    c->scene_bytes += (int64_t)bytes;
    *out = static_cast<const T*>(p);
    return 0;
}

static inline int fint(float f) { return (int)f; }   // GLSL int(float)

#ifndef WF_TRACE_GRID_PCT
#define WF_TRACE_GRID_PCT 50         // cap of the trace grid, % of full occupancy, for batches of fewer than
#endif                               // WF_SMALL_CALL_PATHS paths (multi-GPU shares: the calls in flight share the chip)
#ifndef WF_TRACE_GRID_PCT_LARGE
#define WF_TRACE_GRID_PCT_LARGE 80   // ... and for larger batches (16-frame 1080p calls: C2 +1.6 %, C5 +2.9 %, C4 -3.4 %)
#endif
#ifndef WF_TRACE_PATHS_PER_BLOCK
#define WF_TRACE_PATHS_PER_BLOCK (8 * WF_TRACE_BLOCK) // > 0: trace grid <= paths / this (small multi-GPU shares)
#endif
#ifndef WF_STAGGER
#define WF_STAGGER 3        // k > 0: calls of >= WF_STAGGER_PATHS paths run on two pipes with the full trace
#endif                      // grid, each starting when the previous one is k trace / shade launches from its end
#ifndef WF_TRACE_GRID_PCT_ONE
#define WF_TRACE_GRID_PCT_ONE 100   // trace grid of a staggered call, % of full occupancy
#endif
#ifndef WF_STAGGER_PATHS
#define WF_STAGGER_PATHS 12000000   // (1080p calls of >= 6 frames; a rank's share at N = 2 with 16-frame calls)
#endif
#ifndef WF_CC_MAX_PATHS
#define WF_CC_MAX_PATHS 4000000     // lone calls of fewer paths per batch run the CC trace instantiation (the
#endif                              // reference's 512x512 frame: 262k); larger ones the pipelined one at 8 waves
#ifndef WF_ALONE_ON_CALLER
#define WF_ALONE_ON_CALLER 1        // a call with nothing in flight runs on the caller's stream (no worker hop)
#endif
#ifndef WF_TRACE_PATHS_PER_BLOCK_ALONE
#define WF_TRACE_PATHS_PER_BLOCK_ALONE WF_TRACE_BLOCK  // ... for a call with no other call in flight
#endif

// Wavefront buffers of one batch of n path slots, carved from `base` (wf_layout):
// two path-state sets (P0-P7 + block counts), hit / occ, the env ray records,
// the light and continuation entry lists (a byte per path each), segment counts, dequeue counters + census words (+ the timing builds' stamps).
#define WF_SOBOL_BYTES (4 * WF_MAX_CHUNK_FRAMES * 8)   // the batch's Sobol table: bounces 1..3 x frames, float2
static size_t wf_bytes(size_t n) {
    const size_t npad = (n + 255) / 256 * 256, nseg = npad / 256;
    return 2 * (npad * 16 * 8 + nseg * 4 + 256) + n * (4 + 2) + 256 + npad * 32 + npad * 2 + nseg * 12 + 256 + WF_SOBOL_BYTES +
           WF_COUNTER_BYTES + 512 +
           (WF_TIMING ? (size_t)64 * 1024 * 1024 : 0);
}
// The two path-state sets of a batch (entries are indexed up to npad: a block's
// live paths are compacted to the front of its 256 entries).
struct WfLayout {
    WfBufs b;
    PathSet set[2];
    uint8_t *lidx, *cidx;      // [npad] each
};
static WfLayout wf_layout(char* base, size_t n) {
    WfLayout L;
    WfBufs& b = L.b;
    const size_t npad = (n + 255) / 256 * 256;
    size_t off = 0;
    for (PathSet& ps : L.set) {
        float4** f4[] = {&ps.P0, &ps.P1, &ps.P2, &ps.P3, &ps.P4, &ps.P5, &ps.P6, &ps.P7};
        for (float4** q : f4) {
            *q = reinterpret_cast<float4*>(base + off); off += npad * 16;
        }
        ps.bcount = reinterpret_cast<uint32_t*>(base + off); off += (npad / 256) * 4;
        off = (off + 255) & ~(size_t)255;
    }
    b.rd = L.set[1];
    b.wr = L.set[0];
    b.hit = reinterpret_cast<int*>(base + off); off += n * 4;
    b.occ = reinterpret_cast<uint8_t*>(base + off); off += n * 2;
    off = (off + 255) & ~(size_t)255;
    b.npad = (uint32_t)((n + 255) / 256 * 256);
    b.nseg_k = b.npad / 256;
    // ray records of the queued kind (env shadow rays; the others are traced from the state)
    const size_t rec = (size_t)b.npad * 16;
    b.rayO = reinterpret_cast<float4*>(base + off); off += rec;
    b.rayD = reinterpret_cast<float4*>(base + off); off += rec;
    // entry lists of the state-traced kinds: WfLayout keeps them, a launch gets the ones it uses (render_batch)
    L.lidx = reinterpret_cast<uint8_t*>(base + off); off += b.npad;
    L.cidx = reinterpret_cast<uint8_t*>(base + off); off += b.npad;
    b.lidx = b.cidx = nullptr;
    b.segcount = reinterpret_cast<unsigned int*>(base + off); off += (size_t)b.nseg_k * 12;
    off = (off + 255) & ~(size_t)255;
    b.sobol = reinterpret_cast<float2*>(base + off); off += WF_SOBOL_BYTES;
    b.counter = reinterpret_cast<unsigned int*>(base + off);               // WF_QSHARDS counters, WF_QSTRIDE dwords apart
    b.stats = reinterpret_cast<unsigned long long*>(base + off + WF_COUNTER_BYTES);
    b.n = (uint32_t)n;
    return L;
}

// Trace grid for a batch of n paths: small batches (a rank's share of a
// multi-GPU frame) take a proportional part of the chip, and no launch more than
// WF_TRACE_GRID_PCT % (WF_TRACE_GRID_PCT_LARGE % for large batches), so the calls
// in flight trace side by side instead of queueing.  A call submitted while no
// other call is in flight (`alone`: an interactive loop that waits for every
// frame, the reference's own 512x512 one-frame dispatch) has the chip to itself:
// full occupancy, one block per WF_TRACE_PATHS_PER_BLOCK_ALONE paths.
static unsigned trace_grid_for(const pnrt_ctx* c, size_t n, bool alone = false, bool one = false, bool cc = false) {
    const unsigned pct = (c->serial || alone) ? 100u : one ? WF_TRACE_GRID_PCT_ONE : n < (size_t)WF_SMALL_CALL_PATHS ? WF_TRACE_GRID_PCT : WF_TRACE_GRID_PCT_LARGE;
    // (cc: the lone calls' instantiation, resident at its own occupancy -- no block waits for a slot)
    const size_t gmax = (size_t)(cc && c->trace_grid_cc > 0 ? c->trace_grid_cc : c->trace_grid) * pct / 100;
    const size_t ppb = alone ? WF_TRACE_PATHS_PER_BLOCK_ALONE : WF_TRACE_PATHS_PER_BLOCK;
    return ppb ? (unsigned)std::min<size_t>(gmax, std::max<size_t>(64, (n + ppb - 1) / ppb)) : (unsigned)gmax;
}

// WF_STATS / WF_TIMING builds: the trace launch's census / per-wave drain
// timestamps, printed to stderr (tools/census.py, tools/trace_stats.py)
static int report_trace_diag(pnrt_ctx* c, const WfBufs& b, hipStream_t st, int bounce, unsigned grid) {
    if (WF_TIMING) {   // tail census: when the queue ran dry vs when the last wave ended
        const size_t nw = (size_t)grid * (WF_TRACE_BLOCK / 64);   // waves launched
        std::vector<unsigned long long> t(4 * nw);
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipMemcpy(t.data(), b.stats + 8, t.size() * 8, hipMemcpyDeviceToHost));
        unsigned long long t0 = ~0ull, tex = ~0ull, tend = 0;
        std::vector<unsigned long long> ends;
        for (size_t w = 0; w < nw; ++w) {
            t0 = std::min(t0, t[4 * w]);
            if (t[4 * w + 1]) tex = std::min(tex, t[4 * w + 1]);
            tend = std::max(tend, t[4 * w + 2]);
            ends.push_back(t[4 * w + 2]);
        }
        std::sort(ends.begin(), ends.end());
        auto us = [&](unsigned long long v) { return (double)(v - t0) / 100.0; };
        fprintf(stderr, "[trace timing] bounce %d n=%u first-empty %.1f us, wave ends p10 %.1f p50 %.1f p90 %.1f "
                "max %.1f us\n", bounce, b.n, us(tex), us(ends[nw / 10]), us(ends[nw / 2]), us(ends[nw * 9 / 10]),
                us(tend));
        // the slowest 1 % of waves: end time and their longest last ray (kind, lane steps)
        std::vector<std::pair<unsigned long long, unsigned long long>> we;
        for (size_t w = 0; w < nw; ++w) we.push_back({t[4 * w + 2], w});
        std::sort(we.begin(), we.end());
        fprintf(stderr, "[trace tail] bounce %d (end us, kind/lane steps of the last ray, iterations and us after the queue ran dry):", bounce);
        for (size_t q = nw - std::max<size_t>(1, nw / 100); q < nw; q += std::max<size_t>(1, nw / 1000)) {
            const size_t w = we[q].second;
            const unsigned long long v = t[4 * w + 3];
            fprintf(stderr, " %.0f:k%llu/%llu:%llu/%.0f", us(t[4 * w + 2]), (v >> 16) & 0xffff, v & 0xffff, v >> 32,
                    (double)(t[4 * w + 2] - t[4 * w + 1]) / 100.0);
        }
        fprintf(stderr, "\n");
    }
    if (WF_DIAG_COOP) {   // cooperative-finish hand-overs of the launch (tests/test_gpu_coop.py)
        unsigned long long cc[5];
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipMemcpy(cc, b.stats, sizeof cc, hipMemcpyDeviceToHost));
        fprintf(stderr, "[coop] bounce %d n=%u anyhit=%llu closest=%llu restarts=%llu multi=%llu deep=%llu\n", bounce, b.n,
                cc[0], cc[1], cc[2], cc[3], cc[4]);
    }
    if (WF_DIAG_COOPSTAT) {   // the lone calls' drain finish (pt_wf.h): finishes, rays, waves it could not take
        unsigned long long cc[9];
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipMemcpy(cc, b.stats, sizeof cc, hipMemcpyDeviceToHost));
        fprintf(stderr, "[coopstat] bounce %d n=%u finishes=%llu rays=%llu deep_stacks=%llu given_back=%llu\n", bounce, b.n,
                cc[5], cc[8], cc[6], cc[7]);
    }
    if (WF_STATS) {
        unsigned long long stt[8 + 48 + 8];
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipMemcpy(stt, b.stats, sizeof stt, hipMemcpyDeviceToHost));
        // shadow rays the bounce's setup found moot (pt_wf.h WF_SKIP_MOOT: not traced)
        fprintf(stderr, "[trace moot] bounce %d light=%llu env=%llu cont=%llu\n", bounce, stt[56], stt[57], stt[58]);
        // the live path entries the setup left, and the rays the trace loaded, by kind
        fprintf(stderr, "[trace loaded] bounce %d entries=%llu light=%llu env=%llu cont=%llu\n", bounce, stt[62], stt[59],
                stt[60], stt[61]);
        HIPCHK(c, hipMemsetAsync(b.stats + 56, 0, 64, st));
        for (int k = 0; k < 3; ++k) {        // lane steps per ray, log2 buckets, by ray kind
            fprintf(stderr, "[trace hist] bounce %d kind %d:", bounce, k);
            for (int q = 0; q < 16; ++q) fprintf(stderr, " %llu", stt[8 + 16 * k + q]);
            fprintf(stderr, "\n");
        }
        fprintf(stderr, "[trace stats] bounce %d n=%u iters=%llu active/iter=%.1f tri=%llu node=%llu uniform-fetch iters=%llu "
                "refills=%llu rays=%llu  lane-steps/ray=%.1f  continuation lane-steps=%.1f%%\n", bounce, b.n, stt[0],
                stt[0] ? (double)stt[1] / stt[0] : 0.0, stt[2], stt[3], stt[4], stt[5], stt[6],
                stt[6] ? (double)stt[1] / stt[6] : 0.0, stt[1] ? 100.0 * stt[7] / stt[1] : 0.0);
    }
    return PNRT_OK;
}

// f(std::true_type{}) or f(std::false_type{}): a run-time flag as a kernel's template argument
template <class F>
static void with_bool(bool v, F&& f) {
    if (v) f(std::true_type{});
    else f(std::false_type{});
}

#define CAM_REC_BYTES 48       // pt_primary_wf's record (q0, q1, q2), one per path slot of a camera batch
// Where a call's first-bounce rays come from, made once by its entry point and passed down unchanged:
// the pipe's per-pixel primary records (PrimKey), a camera per frame (pt_cameras.h) or the caller's ray
// sets (pt_rays.h); and, independently, whether its path slots are an active-tile list (pt_adaptive.h).
// Only the calls the ABI has can be made: cameras take no tile list.
class PathSource {
    PathSource(int k, const WfAdapt* t, const float* cm, const void* ry, int64_t stride)
        : kind(k), tiles(t), cams(cm), rays(static_cast<const float4*>(ry)), ray_stride(stride) {}

public:
    enum { RECORDS, CAMERAS, RAYS };
    const int kind;
    const WfAdapt* const tiles;    // an adaptive call's active-tile list, or null
    const float* const cams;       // CAMERAS: the call's cameras (pinned host memory, 12 floats per frame)
    const float4* const rays;      // RAYS: the call's first set (device memory),
    const int64_t ray_stride;      // and the records between the sets of consecutive frames
    static PathSource records(const WfAdapt* tiles = nullptr) { return {RECORDS, tiles, nullptr, nullptr, 0}; }
    static PathSource cameras(const float* cams) { return {CAMERAS, nullptr, cams, nullptr, 0}; }
    static PathSource ray_sets(const void* rays, int64_t stride, const WfAdapt* tiles = nullptr) {
        return {RAYS, tiles, nullptr, rays, stride};
    }
    // further bytes per path slot: the batch's camera-ray records, one per slot
    size_t slot_bytes() const { return kind == RECORDS ? 0 : CAM_REC_BYTES; }
    // the call reads the pipe's per-pixel records, traced or still valid by their key
    bool per_pixel_records() const { return kind == RECORDS; }
    // the call's workers read what the caller queued on the context stream before it (ev_rays)
    bool after_caller_stream() const { return kind == RAYS; }
    // f(the tile list), or f(): the pack pt_rays_wf ends with
    template <class F>
    void with_tiles(F&& f) const {
        if (tiles) f(*tiles);
        else f();
    }
    // f(the pack the gen and shade kernels end with) for a batch with the camera table cm or the rays ry:
    // one of (), (WfAdapt), (WfCams), (WfRays), (WfAdapt, WfRays)
    template <class F>
    void with_pack(const WfCams& cm, const WfRays& ry, F&& f) const {
        switch (kind) {
            case RECORDS: with_tiles(f); break;
            case CAMERAS: f(cm); break;
            case RAYS: with_tiles([&](auto... t) { f(t..., ry); }); break;
        }
    }
};

// One batch of frames (gen -> {trace -> shade/setup} x depth) on one stream;
// its colours land in frame slots [0, cf) of `colors`.  cm, ry: the batch's camera table or rays, as
// src takes them (then primary = the batch's records per slot).
static int render_batch(pnrt_ctx* c, const DevScene& s, const FrameParams& fp, const WfLayout& L, hipStream_t st,
                        const float4* primary, float4* colors, bool alone, bool one, hipEvent_t stage, const PathSource& src,
                        const WfCams& cm, const WfRays& ry) {
    WfBufs b = L.b;
    if (b.n > WF_META_SLOT) return set_err(c, PNRT_E_ARG, "render: too many paths per batch");
    // the cooperative finish of closest-hit rays pays where the drain leaves the chip
    // idle -- a call with nothing else in flight (the reference's loop: D2 sync -19 %);
    // beside other calls' kernels the wave's 64 lanes on one ray cost more than they
    // save (C2 -2.3 %), so pipelined calls run the instantiation without it
    // (only for batches below WF_CC_MAX_PATHS: the lone call's instantiation runs at
    // WF_TRACE_WAVES_CC waves per SIMD, fewer than a large batch's stepping wants)
    const bool cc = alone && WF_COOP_TAIL >= 2 && (size_t)b.n < (size_t)WF_CC_MAX_PATHS && !s.has_leaf_table;
    const dim3 g((unsigned)((b.n + 255) / 256));
    b.wr = L.set[0];
    if (WF_STATS) HIPCHK(c, hipMemsetAsync(b.stats + 56, 0, 64, st));    // the setups' moot-ray counts
    {   // path state + bounce-0 sampling
        ProfScope ps(c, PNRT_K_GEN, st);
        src.with_pack(cm, ry, [&](auto... pk) {
            hipLaunchKernelGGL((pt_wf_gen_setup<decltype(pk)...>), g, dim3(256), 0, st, s, fp, b, primary, colors, pk...);
        });
    }
    HIPCHK(c, hipGetLastError());
    const unsigned tg = trace_grid_for(c, b.n, alone, one, cc);
    // (launch position 2 b: bounce b's trace, 2 b + 1: its shade)
    const int stage_at = std::max(2 * fp.max_depth - WF_STAGGER, 0);
    for (int bounce = 0; bounce < fp.max_depth; ++bounce) {
        if (stage && 2 * bounce == stage_at) HIPCHK(c, hipEventRecord(stage, st));
        // segment dequeue counters: zeroed by the setup kernel that queued the rays
        // (the census builds also clear their words)
        if (WF_STATS || WF_TIMING || WF_DIAG_COOP || WF_DIAG_COOPSTAT)
            HIPCHK(c, hipMemsetAsync(b.counter, 0, WF_COUNTER_BYTES + (WF_STATS ? 448 : 512), st));
        {
            ProfScope ps(c, PNRT_K_TRACE, st);
            if (cc)                     // (only scenes without a leaf table have the instantiation)
                hipLaunchKernelGGL((pt_wf_trace<WF_STACK, false, true>), dim3(tg), dim3(WF_TRACE_BLOCK), 0, st, s, b, fp.mode);
            else
                with_bool(s.has_leaf_table, [&](auto tbl) {
                    hipLaunchKernelGGL((pt_wf_trace<WF_STACK, decltype(tbl)::value>), dim3(tg), dim3(WF_TRACE_BLOCK), 0, st, s, b,
                                       fp.mode);
                });
        }
        HIPCHK(c, hipGetLastError());
        if (WF_STATS || WF_TIMING || WF_DIAG_COOP || WF_DIAG_COOPSTAT)
            if (int rc = report_trace_diag(c, b, st, bounce, tg)) return rc;
        if (stage && 2 * bounce + 1 == stage_at) HIPCHK(c, hipEventRecord(stage, st));
        {
            ProfScope ps(c, PNRT_K_SHADE, st);
            // MIS + continuation, then the next bounce's sampling (sets alternate)
            b.rd = L.set[bounce & 1];
            b.wr = L.set[(bounce + 1) & 1];
            // this setup's moot test drops light rays, and continuation rays where it sets up
            // the last bounce: those kinds go through their entry lists, in the setup and in
            // the trace launch that follows it (gen has no test: whole ranges, no lists)
            b.lidx = L.lidx;
            b.cidx = bounce + 2 == fp.max_depth ? L.cidx : nullptr;
            // (the last bounce's: every path ends -- no setup half, no rays)
            with_bool(bounce + 1 == fp.max_depth, [&](auto fin) {
                src.with_pack(cm, ry, [&](auto... pk) {
                    hipLaunchKernelGGL((pt_wf_shade_setup<decltype(fin)::value, decltype(pk)...>), g, dim3(256), 0, st, s, fp, b,
                                       primary, colors, pk...);
                });
            });
        }
        HIPCHK(c, hipGetLastError());
    }
    if (stage && fp.max_depth <= 0) HIPCHK(c, hipEventRecord(stage, st));
    return PNRT_OK;
}

// PNRT_BATCH_BYTES: decimal digits only, a value that fits 64 bits (0: no cap).
// Anything else -- "3e9", "abc", "-1", "", trailing junk -- is refused, not guessed at.
static bool parse_batch_bytes(const char* s, uint64_t* out) {
    if (!s || !*s) return false;
    uint64_t v = 0;
    for (; *s; ++s) {
        if (*s < '0' || *s > '9') return false;
        const uint64_t d = (uint64_t)(*s - '0');
        if (v > (UINT64_MAX - d) / 10) return false;
        v = v * 10 + d;
    }
    *out = v;
    return true;
}

// Path slots of one frame of `rows` rows (8x8-pixel tiles) and the bytes the cap
// measures for a batch of k such frames: the wavefront buffers and the colours.
static size_t frame_paths(int width, int rows) {
    return (size_t)((width + 7) / 8) * (size_t)((rows + 7) / 8) * 64;
}
// (per_path: further bytes per path slot -- PathSource::slot_bytes)
static size_t batch_bytes(size_t per_frame, size_t pix, uint32_t k, size_t per_path) {
    return wf_bytes(per_frame * k) + pix * 16 * k + per_frame * k * per_path;
}
// Frames per batch of a call of nf frames (the one plan: render_wavefront and
// pnrt_batch_plan): at most WF_MAX_CHUNK_FRAMES, few enough that every path slot
// fits the path state's slot field (large frames take fewer per batch), and under
// PNRT_BATCH_BYTES the largest count whose batch_bytes fit the cap -- one frame when
// not even one does.  0: a frame too large for one batch.
static uint32_t plan_chunk(const pnrt_ctx* c, size_t per_frame, size_t pix, uint32_t nf, size_t per_path) {
    if (per_frame == 0 || per_frame > (size_t)WF_META_SLOT) return 0;
    const uint32_t fit = (uint32_t)std::min<size_t>(WF_MAX_CHUNK_FRAMES, (size_t)WF_META_SLOT / per_frame);
    uint32_t chunk = nf < fit ? nf : fit;
    // (batch_bytes grows with the frame count, so the first count that fits is the largest)
    while (c->batch_bytes_cap && chunk > 1 && batch_bytes(per_frame, pix, chunk, per_path) > c->batch_bytes_cap) --chunk;
    return chunk;
}

static int pipes_init(pnrt_ctx* c) {
    if (c->pipes_ready) return PNRT_OK;
    c->pipes_ready = true;
    const char* q = getenv("GPU_MAX_HW_QUEUES");
    const int hw_queues = (q && atoi(q) > 0) ? atoi(q) : 4;
    c->n_pipes_small = hw_queues > 4 ? WF_PIPES : WF_PIPES_LARGE;
    for (unsigned i = 0; i < c->n_pipes_small; ++i) {
        auto& P = c->pipe[i];
        HIPCHK(c, hipStreamCreateWithFlags(&P.w, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&P.ev_join, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&P.ev_blend, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&P.ev_stage, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&P.ev_rays, hipEventDisableTiming));
    }
    return PNRT_OK;
}

// The trace grid at full occupancy (and that of the lone calls' instantiation), asked once.
static int trace_grid_init(pnrt_ctx* c) {
    if (c->trace_grid == 0) {
        int per_cu = 0, cus = 0;
        HIPCHK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, pt_wf_trace<WF_STACK, false>, WF_TRACE_BLOCK, 0));
        HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
        c->trace_grid = (per_cu > 0 ? per_cu : 1) * cus;
        int per_cu_cc = 0;
        HIPCHK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_cc, pt_wf_trace<WF_STACK, false, true>, WF_TRACE_BLOCK, 0));
        c->trace_grid_cc = std::min(c->trace_grid, (per_cu_cc > 0 ? per_cu_cc : 1) * cus);
    }
    return PNRT_OK;
}

// The per-lane spill area of the trace kernel's stack (LDS holds WF_STACK entries), for a
// launch of up to the full trace grid (after trace_grid_init).
struct OvfSize {
    int stride;
    size_t bytes;
};
static OvfSize ovf_size(const pnrt_ctx* c) {
    const int stride = c->wf_stack_need > WF_STACK ? c->wf_stack_need - WF_STACK : 1;
    return {stride, (size_t)c->trace_grid * WF_TRACE_BLOCK * stride * 8};
}

// The traversal mode the kernels run: z-slab culling only over finite boxes (pnrt_upload_scene).
static int traverse_mode(const pnrt_ctx* c) { return c->boxes_finite ? c->mode : PNRT_TRAVERSE_EXACT; }

// A camera's twelve floats -- eye, lower-left corner, horizontal, vertical -- from one form that
// holds them into another.
static void cam_floats(float* eye, float* llc, float* hor, float* ver, const float* e, const float* l, const float* h,
                       const float* v) {
    std::memcpy(eye, e, 12); std::memcpy(llc, l, 12);
    std::memcpy(hor, h, 12); std::memcpy(ver, v, 12);
}
static void cam_floats(float* eye, float* llc, float* hor, float* ver, const pnrt_camera& cam) {
    cam_floats(eye, llc, hor, ver, cam.eye, cam.lower_left, cam.horizontal, cam.vertical);
}

static int shard_rows(int h, int band, int n, int shard) {
    // 64-bit row positions: band may be any positive int (band >= h: one band), and
    // shard * band or band * n leave int long before that
    int64_t rows = 0;
    const int64_t step = (int64_t)band * n;
    for (int64_t y0 = (int64_t)shard * band; y0 < h; y0 += step) rows += (h - y0 < band) ? h - y0 : band;
    return (int)rows;
}

// The frame parameters of a call that renders frames first .. first + nf - 1 with camera `cam`
// over a shard selector's rows, in the effective traversal mode.
static FrameParams frame_params(const pnrt_ctx* c, const pnrt_camera& cam, uint32_t first, uint32_t nf, int band, int nsh,
                                int shard) {
    FrameParams fp;
    cam_floats(fp.eye, fp.llc, fp.hor, fp.ver, cam);
    fp.width = c->width; fp.height = c->height; fp.max_depth = c->max_bounce;
    fp.first_frame = first; fp.n_frames = nf;
    fp.band = band; fp.n_shards = nsh; fp.shard = shard;
    fp.rows = shard_rows(c->height, band, nsh, shard);
    fp.mode = traverse_mode(c);
    return fp;
}
// ... and of the whole image (one band, one shard), one frame: the guide images
static FrameParams full_frame_params(const pnrt_ctx* c, const pnrt_camera& cam) { return frame_params(c, cam, 0, 1, 1, 1, 0); }

// The primary records (camera ray's closest hit per pixel of the shard) depend
// on the camera, the frame size, the shard, the traversal mode and the scene
// (scene_epoch: arrays, materials, environment) -- not on the frame number: the
// camera ray has no jitter (ray_tracing.comp:205-211, 980).  Records that were
// traced for the same key are reused (read-only since), exactly.
static pnrt_ctx::PrimKey prim_key(const pnrt_ctx* c, const FrameParams& fp) {
    pnrt_ctx::PrimKey key;
    key.epoch = c->scene_epoch;
    cam_floats(key.cam, key.cam + 3, key.cam + 6, key.cam + 9, fp.eye, fp.llc, fp.hor, fp.ver);
    key.width = fp.width; key.height = fp.height; key.rows = fp.rows;
    key.band = fp.band; key.n_shards = fp.n_shards; key.shard = fp.shard; key.mode = fp.mode;
    key.valid = true;
    return key;
}
// `have` names the records `want` asks for.  any_band: whatever band they were traced with
// (the same rows in the same order when one shard owns them all).
static bool prim_key_eq(const pnrt_ctx::PrimKey& have, const pnrt_ctx::PrimKey& want, bool any_band = false) {
    return have.valid && have.epoch == want.epoch && !std::memcmp(have.cam, want.cam, sizeof want.cam) &&
           have.width == want.width && have.height == want.height && have.rows == want.rows &&
           (any_band || have.band == want.band) && have.n_shards == want.n_shards && have.shard == want.shard &&
           have.mode == want.mode;
}
// `b` with the trace kernel's spill area `ovf` (sized by ovf_size, after trace_grid_init) and the fault words
static WfBufs spill_bufs(const pnrt_ctx* c, uint2* ovf, WfBufs b = WfBufs{}) {
    b.ovf = ovf;
    b.fault = c->fault_dev;
    b.ovf_stride = (uint32_t)ovf_size(c).stride;
    return b;
}
// One launch of the trace kernel's step over n items, grid-stride, on stream st: launch(TBL, grid) names
// the kernel.  Class PNRT_K_PRIMARY.
template <class L>
static int trace_step(pnrt_ctx* c, const DevScene& s, hipStream_t st, size_t n, L&& launch) {
    ProfScope ps(c, PNRT_K_PRIMARY, st);
    const dim3 grid((unsigned)std::min<size_t>((n + WF_TRACE_BLOCK - 1) / WF_TRACE_BLOCK, (size_t)c->trace_grid));
    with_bool(s.has_leaf_table, [&](auto tbl) { launch(tbl, grid); });
    HIPCHK(c, hipGetLastError());
    return PNRT_OK;
}

// Ensure `primary` holds the records of fp's shard (render_wavefront's pipes and
// pnrt_render_guides): traced on stream w -- the trace kernel's step, grid-stride,
// with the spill area `ovf` -- unless `have` says they are there already.  One
// launch of class PNRT_K_PRIMARY, or none.
static int ensure_primary(pnrt_ctx* c, const DevScene& s, const FrameParams& fp, hipStream_t w, uint2* ovf, float4* primary,
                          pnrt_ctx::PrimKey& have) {
    const pnrt_ctx::PrimKey key = prim_key(c, fp);
    if (prim_key_eq(have, key)) return PNRT_OK;
    const WfBufs pb = spill_bufs(c, ovf);
    const auto launch = [&](auto tbl, dim3 grid) {
        hipLaunchKernelGGL((pt_primary_wf<WF_STACK, decltype(tbl)::value>), grid, dim3(WF_TRACE_BLOCK), 0, w, s, fp, pb, primary);
    };
    if (int rc = trace_step(c, s, w, (size_t)fp.rows * fp.width, launch)) return rc;
    have = key;
    return PNRT_OK;
}

// A pipe's buffers for batches of `slots` path slots and `color_bytes` of frame colours
// over a shard of `pix` pixels of a call of source `src` (start_call).
static int pipe_size(pnrt_ctx* c, pnrt_ctx::Pipe& Q, const PathSource& src, size_t pix, size_t color_bytes, size_t slots) {
    bool moved = false;
    int rc = Q.primary.reserve(c, pix * 48, &moved);
    if (moved) Q.prim.valid = false;
    if (rc || (rc = Q.colors.reserve(c, color_bytes)) || (rc = Q.wf.reserve(c, wf_bytes(slots) + 512)) ||
        (rc = Q.ovf.reserve(c, ovf_size(c).bytes)) || (rc = Q.camrec.reserve(c, slots * src.slot_bytes())) ||
        (src.cams && (rc = Q.camtab.reserve(c, (size_t)WF_MAX_CHUNK_FRAMES * 48))))
        return rc;
    return PNRT_OK;
}

// How a call's batches run (render_wavefront decides it by call size and what is in
// flight; render_adaptive is always a lone call).
struct BatchRoute {
    hipStream_t w;           // the stream of the batches' kernels (the caller's for a lone call)
    bool alone, one, stagger;
    int ovf_stride, tiles_x;
};
// The batches of one call on pipe P: per group of `chunk` frames one batch (gen ->
// {trace -> shade} x depth) of per_frame path slots per frame on R.w, then the
// frame-ordered blend on the context stream.
static int run_batches(pnrt_ctx* c, const DevScene& s, const FrameParams& fp, pnrt_ctx::Pipe& P, const PathSource& src,
                       const BatchRoute& R, size_t per_frame, uint32_t chunk, uint32_t first, uint32_t nf) {
    int rc;
    const size_t pix = (size_t)fp.rows * c->width;
    hipStream_t w = R.w;
    for (uint32_t f0 = 0; f0 < nf; f0 += chunk) {
        const uint32_t cf = (nf - f0) < chunk ? (nf - f0) : chunk;
        WfLayout a = wf_layout(static_cast<char*>(P.wf), per_frame * cf);
        a.b.ovf = P.ovf;
        a.b.fault = c->fault_dev;
        a.b.ovf_stride = (uint32_t)R.ovf_stride;
        a.b.chunk_frames = (int)cf;
        a.b.tiles_x = R.tiles_x;
        a.b.first_frame = first + f0;
        if (f0 && w != c->stream) HIPCHK(c, hipStreamWaitEvent(w, P.ev_blend, 0));   // the previous group's blend has read the colours
        const bool last = f0 + cf >= nf;
        const WfCams cm{P.camtab};
        const WfRays ry{src.rays + 2 * ((size_t)f0 * (size_t)src.ray_stride), src.ray_stride};
        if (src.kind == PathSource::CAMERAS) {
            // the batch's cameras, then its camera rays: one per path slot (pt_cameras.h).  Both follow
            // the previous batch's kernels on w, the last readers of the table and the records
            HIPCHK(c, hipMemcpyAsync(P.camtab, src.cams + 12 * (size_t)f0, (size_t)cf * 48, hipMemcpyHostToDevice, w));
            const auto launch = [&](auto tbl, dim3 grid) {
                hipLaunchKernelGGL((pt_camera_rays_wf<WF_STACK, decltype(tbl)::value>), grid, dim3(WF_TRACE_BLOCK), 0, w, s, fp, a.b, cm,
                                   P.camrec);
            };
            if ((rc = trace_step(c, s, w, a.b.n, launch))) return rc;
        }
        if (src.kind == PathSource::RAYS) {
            // the batch's camera rays from the caller's sets f0 .. f0 + cf - 1: one per path slot (pt_rays.h; an
            // adaptive call's: the list's slots), behind the previous batch's kernels on w, the last readers of the records
            const auto launch = [&](auto tbl, dim3 grid) {
                src.with_tiles([&](auto... ad) {
                    hipLaunchKernelGGL((pt_rays_wf<WF_STACK, decltype(tbl)::value, false, decltype(ad)...>), grid, dim3(WF_TRACE_BLOCK),
                                       0, w, s, fp, a.b, ry, P.camrec, ad...);
                });
            };
            if ((rc = trace_step(c, s, w, a.b.n, launch))) return rc;
        }
        if ((rc = render_batch(c, s, fp, a, w, src.per_pixel_records() ? P.primary : P.camrec, P.colors, R.alone, R.one,
                               R.stagger && last ? P.ev_stage : nullptr, src, cm, ry)))
            return rc;
        if (R.stagger && last) P.stage_set = true;
        if (w != c->stream) {
            HIPCHK(c, hipEventRecord(P.ev_join, w));
            HIPCHK(c, hipStreamWaitEvent(c->stream, P.ev_join, 0));
        }
        {   // the blends run in call order on the caller's stream
            ProfScope ps(c, PNRT_K_BLEND);
            if (src.tiles)              // the active pixels' blend and moments (pt_adaptive.h)
                hipLaunchKernelGGL(pt_blend_adaptive_kernel, dim3((unsigned)(((size_t)src.tiles->n_tiles * 64 + 255) / 256)), dim3(256),
                                   0, c->stream, fp, *src.tiles, R.tiles_x, (const float4*)P.colors, c->accum, c->moments, (int)cf,
                                   first + f0);
            else if (c->moments_on)     // the same blend, and the moments of the batch's frames (pt_moments.h)
                hipLaunchKernelGGL(pt_blend_moments_kernel, dim3((unsigned)((pix + 255) / 256)), dim3(256), 0, c->stream, fp,
                                   (const float4*)P.colors, c->accum, c->moments, (int)cf, first + f0);
            else
                hipLaunchKernelGGL(pt_blend_kernel, dim3((unsigned)((pix + 255) / 256)), dim3(256), 0, c->stream, fp,
                                   (const float4*)P.colors, c->accum, (int)cf, first + f0);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(P.ev_blend, c->stream));
        P.blend_pending = true;
        if ((rc = mark_stream(c))) return rc;
    }
    return PNRT_OK;
}

// What render_wavefront and render_adaptive decide about a call before it starts on its pipe.
struct CallShape {
    unsigned pipe, prev_pipe;        // the call's pipe; the pipe of the call before it
    unsigned npipes;                 // the pipes sized now: the ones this call size rotates over, from `pipe` on
    size_t per_frame, color_bytes;   // path slots per frame; a batch's colours
    uint32_t chunk;                  // frames per batch
    bool alone, one, stagger;
};
// Start a call of source `src` on its pipe: the buffers, the order against what used them last (and, for a
// source that reads the caller's memory, against the context stream), the pipe's primary records where the
// source uses them, the batches.
static int start_call(pnrt_ctx* c, const DevScene& s, const FrameParams& fp, const PathSource& src, const CallShape& k,
                      uint32_t first, uint32_t nf) {
    int rc;
    pnrt_ctx::Pipe& P = c->pipe[k.pipe];
    // every buffer set this call size rotates over is sized now, so no later call of
    // the same size reallocates (a reallocation waits for all calls in flight)
    for (unsigned q = 0; q < k.npipes; ++q)
        if ((rc = pipe_size(c, c->pipe[q ? (k.pipe + q) % k.npipes : k.pipe], src, (size_t)fp.rows * c->width, k.color_bytes,
                            k.per_frame * k.chunk)))
            return rc;
    ++c->ncall;
    // A call with nothing in flight runs on the caller's stream itself: no worker
    // stream to order against it, so no event wait before its first kernel and no
    // join before its blend (the reference's loop: one frame, then display)
    const bool on_caller = k.alone && WF_ALONE_ON_CALLER;
    hipStream_t w = on_caller ? c->stream : P.w;
    // this pipe's buffers were last read by the blend of the call that used it last
    // (already complete for a call with nothing in flight: `alone` queried it)
    if (P.blend_pending && !k.alone) HIPCHK(c, hipStreamWaitEvent(w, P.ev_blend, 0));
    // staggered calls: this one starts when the previous one reaches its last bounces
    if (k.stagger && !k.alone && k.prev_pipe != k.pipe && k.prev_pipe < WF_PIPES && c->pipe[k.prev_pipe].stage_set)
        HIPCHK(c, hipStreamWaitEvent(w, c->pipe[k.prev_pipe].ev_stage, 0));
    P.stage_set = false;
    // the pipe's primary records: traced now, or still valid from an earlier call (PrimKey)
    if (src.per_pixel_records() && (rc = ensure_primary(c, s, fp, w, P.ovf, P.primary, P.prim))) return rc;
    if (src.after_caller_stream() && w != c->stream) {   // the caller's writes of the rays, queued on the context stream, before the worker's reads
        HIPCHK(c, hipEventRecord(P.ev_rays, c->stream));
        HIPCHK(c, hipStreamWaitEvent(w, P.ev_rays, 0));
    }
    const BatchRoute R = {w, k.alone, k.one, k.stagger, ovf_size(c).stride, (c->width + 7) / 8};
    if ((rc = run_batches(c, s, fp, P, src, R, k.per_frame, k.chunk, first, nf))) return rc;
    if (src.cams) {             // behind the call's last table copy: the staging block is free once it completes
        pnrt_ctx::CamStage& S = c->cam_stage.back();
        HIPCHK(c, hipEventRecord(S.ev, w));
        S.pending = true;
    }
    return PNRT_OK;
}

// v3 wavefront, one pnrt_render call on a pipe: the primary pass (unless the
// pipe's records are still valid, PrimKey), then per group of <= WF_MAX_CHUNK_FRAMES frames one
// batch (gen -> {trace -> shade} x depth) on the pipe's worker stream, then the
// frame-ordered blend on the context stream.  Consecutive calls are independent
// path sets, so running them concurrently changes nothing in the result; the
// blends keep frame order.
// A camera call (pnrt_render_cameras) or a ray call (pnrt_render_rays) is planned with its camera-ray
// records' bytes; its batches trace their own camera rays (run_batches) and leave the pipe's per-pixel
// records and their key alone.
static int render_wavefront(pnrt_ctx* c, const DevScene& s, const FrameParams& fp, const PathSource& src, uint32_t first,
                            uint32_t nf) {
    int rc;
    if ((rc = pipes_init(c))) return rc;
    const size_t pix = (size_t)fp.rows * c->width;
    const size_t per_frame = frame_paths(c->width, fp.rows);
    const uint32_t chunk = plan_chunk(c, per_frame, pix, nf, src.slot_bytes());   // frames per batch
    if (chunk == 0) return set_err(c, PNRT_E_ARG, "render: frame too large for one batch");
    // calls in flight by call size (paths per batch): small (< 5M: multi-GPU shares)
    // 4 with > 4 hardware queues; 5M-12M 2 -- their launches are long enough to fill
    // each other's drains (measured on 8-frame 1080p calls before the staggering: C2
    // +1.8 %, C3 +2.7 %, C4 +1.6 % against 3).
    // From 12M (1080p calls of 6+ frames, 4K calls) the calls are staggered (round 4):
    // two pipes, the full trace grid, and a call starts only when the previous one
    // has finished its second-to-last trace launch, so the two overlap just in the
    // drain-heavy end (last shade / trace / shade / blend) instead of contending for
    // the chip throughout (same box, 2 rounds: C2 +2.5 %, C3 +3.3 %, C4 +1.2 %, C5
    // +1.1 %; one call in flight: C2 +1.8 %, C4 -1.8 %).
    // Without staggering (WF_STAGGER 0): 2 pipes up to 32M, 3 above.
    const size_t call_paths = per_frame * chunk;
    const bool stagger = !c->serial && WF_STAGGER > 0 && call_paths >= (size_t)WF_STAGGER_PATHS;
    const bool one = c->serial || stagger;       // the trace launch may take the whole chip
    const unsigned want = stagger ? 2u : one ? 1u
                        : call_paths < (size_t)WF_SMALL_CALL_PATHS ? c->n_pipes_small
                        : call_paths < (size_t)WF_HUGE_CALL_PATHS ? WF_PIPES_MEDIUM : WF_PIPES_LARGE;
    const unsigned npipes = std::max(1u, std::min(want, c->n_pipes_small));   // only sets pipes_init made
    // no other call in flight: every pipe's last blend (its last work) has completed
    bool alone = !c->serial;
    for (auto& Q : c->pipe)
        if (alone && Q.blend_pending && hipEventQuery(Q.ev_blend) != hipSuccess) alone = false;
    // A call with nothing in flight stays on the last call's pipe (its buffers are
    // free, its primary records likely still valid, its lines still in the caches);
    // otherwise the calls rotate over the pipes
    const unsigned prev_pipe = c->last_pipe;
    const unsigned pi = (alone && c->last_pipe < npipes) ? c->last_pipe : c->next_pipe % npipes;
    c->next_pipe = (pi + 1) % npipes;
    c->last_pipe = pi;
    if ((rc = trace_grid_init(c))) return rc;
    return start_call(c, s, fp, src, {pi, prev_pipe, npipes, per_frame, pix * 16 * chunk, chunk, alone, one, stagger}, first, nf);
}

// pnrt_render_adaptive's frames: the batches over the active tiles' path slots.  The
// call has waited for everything in flight, so it is a lone call: the last call's pipe
// (its primary records likely still valid, PrimKey) with no rotation, the caller's stream.
// (pnrt_render_rays_adaptive's: the batches trace the list's camera rays into the pipe's per-slot records.)
static int render_adaptive(pnrt_ctx* c, const DevScene& s, const FrameParams& fp, const PathSource& src, uint32_t chunk,
                           uint32_t first, uint32_t nf) {
    int rc;
    if ((rc = pipes_init(c)) || (rc = trace_grid_init(c))) return rc;
    const size_t per_frame = (size_t)src.tiles->n_tiles * 64;
    const unsigned pi = c->last_pipe < c->n_pipes_small ? c->last_pipe : 0;
    c->last_pipe = pi;
    return start_call(c, s, fp, src, {pi, pi, 1, per_frame, per_frame * 16 * chunk, chunk, !c->serial, c->serial, false}, first, nf);
}

// The scene as the kernels take it: the uploaded arrays with the environment,
// the textures and the fault words bound now.
static DevScene launch_scene(const pnrt_ctx* c) {
    DevScene s = c->scene;
    s.hdr = c->hdr;
    s.rnd = c->rnd;
    s.hdr_q = c->hdr_q;
    s.rnd_q = c->rnd_q;
    s.n_tex = PT_MAX_TEXTURES;
    for (int i = 0; i < PT_MAX_TEXTURES; ++i) {
        s.tex[i] = c->tex[i];
        s.tex_w[i] = c->tex_w[i]; s.tex_h[i] = c->tex_h[i];
    }
    s.unorm8 = c->unorm8;
    s.fault = c->fault_dev;
    s.diag_force = 0;
    return s;
}

// ---- guide images and the denoised preview -------------------------------------------------
// What guide images rendered now for camera `cam` would be rendered for.
static pnrt_ctx::GuideKey guide_key_for(const pnrt_ctx* c, const pnrt_camera& cam) {
    pnrt_ctx::GuideKey k;
    k.epoch = c->scene_epoch;
    k.tex_epoch = c->tex_epoch;
    cam_floats(k.cam, k.cam + 3, k.cam + 6, k.cam + 9, cam);
    k.width = c->width; k.height = c->height;
    k.mode = traverse_mode(c);
    k.valid = true;
    return k;
}
// ... for the current camera (pnrt_denoise compares)
static pnrt_ctx::GuideKey guide_key_now(const pnrt_ctx* c) { return guide_key_for(c, c->cam); }
// (the guides `a` of a ray set match any camera -- that they match the accumulation is the caller's statement --
// unless camera-keyed ones are asked for: pnrt_reproject's `from`)
static bool guide_key_eq(const pnrt_ctx::GuideKey& a, const pnrt_ctx::GuideKey& b, bool camera_keyed = false) {
    return a.valid && b.valid && a.epoch == b.epoch && a.tex_epoch == b.tex_epoch &&
           (a.rays ? !camera_keyed : !std::memcmp(a.cam, b.cam, sizeof a.cam)) &&
           a.width == b.width && a.height == b.height && a.mode == b.mode;
}

// The guide images of camera `cam` (the current one for pnrt_render_guides; the one the
// accumulation was rendered with, then the current one, for pnrt_reproject) or, with `rays`, of one ray
// set (pnrt_render_guides_rays; both views of pnrt_reproject_view: the camera's floats are not read).
// A camera's records are lent by a pipe or traced into the guides' own buffer under its key; a set's are
// traced there, one launch of class PNRT_K_PRIMARY, and have no key.  The checks are the caller's.
static int render_guides(pnrt_ctx* c, const pnrt_camera& cam, const void* rays) {
    int rc;
    if ((rc = pipes_init(c)) || (rc = trace_grid_init(c))) return rc;
    const DevScene s = launch_scene(c);
    const FrameParams fp = full_frame_params(c, cam);
    const size_t pix = (size_t)c->width * c->height;
    if (pix > 0xFFFFFFFFull / 64) return set_err(c, PNRT_E_ARG, std::string(rays ? "render_guides_rays" : "render_guides") + ": frame too large");
    for (int k = 0; k < PNRT_AOV_COUNT; ++k)
        if ((rc = c->aov[k].reserve(c, pix * 16))) return rc;
    // A pipe that holds the records of the whole image (any band: one shard owns
    // every row, in row order) for this camera, scene and mode lends them, read-only.
    // Its worker wrote them before the call's blend, which the context stream has
    // waited for; the pipe's next call waits for ev_blend before it may retrace
    // them, so the event is recorded again behind the kernel that reads them here.
    const pnrt_ctx::PrimKey want = prim_key(c, fp);    // one shard of one band: shard 0 of 1
    pnrt_ctx::Pipe* lender = nullptr;
    for (auto& Q : c->pipe)
        if (!rays && !lender && Q.primary && Q.blend_pending && prim_key_eq(Q.prim, want, /* any_band */ true)) lender = &Q;
    if (!lender) {      // records of the guides' own, in a buffer and a spill area no pipe uses
        bool moved = false;
        rc = c->g_primary.reserve(c, pix * 48, &moved);
        if (moved || rays) c->g_prim.valid = false;
        if (rc || (rc = c->g_ovf.reserve(c, ovf_size(c).bytes))) return rc;
        if (rays) {
            WfBufs pb = spill_bufs(c, c->g_ovf);
            pb.n = (uint32_t)frame_paths(c->width, c->height);       // one frame's slots: wf_coords' tiles
            pb.chunk_frames = 1;
            pb.tiles_x = (c->width + 7) / 8;
            const WfRays ry{static_cast<const float4*>(rays), 0};
            const auto launch = [&](auto tbl, dim3 grid) {
                hipLaunchKernelGGL((pt_rays_wf<WF_STACK, decltype(tbl)::value, true>), grid, dim3(WF_TRACE_BLOCK), 0, c->stream, s, fp,
                                   pb, ry, c->g_primary.p);
            };
            if ((rc = trace_step(c, s, c->stream, pb.n, launch))) return rc;
        } else if ((rc = ensure_primary(c, s, fp, c->stream, c->g_ovf, c->g_primary, c->g_prim))) {
            return rc;
        }
    }
    const float4* rec = lender ? lender->primary : c->g_primary;
    hipLaunchKernelGGL(pt_guides, dim3((unsigned)((pix + 255) / 256)), dim3(256), 0, c->stream, s, rec,
                       c->aov[PNRT_AOV_POSITION], c->aov[PNRT_AOV_NORMAL], c->aov[PNRT_AOV_ALBEDO], (uint32_t)pix);
    HIPCHK(c, hipGetLastError());
    if (lender) HIPCHK(c, hipEventRecord(lender->ev_blend, c->stream));
    c->guide_key = guide_key_for(c, cam);
    c->guide_key.rays = rays != nullptr;
    return mark_stream(c);
}

// ---- ray queries (pt_query.h) ------------------------------------------------------------------
// Rays of one launch at most (the kernel counts rays in 32 bits) and of one staging
// pass of the host form (28 + 64 bytes of the context's buffers each).
#define QUERY_MAX_LAUNCH ((int64_t)1 << 30)
#define QUERY_MAX_STAGE ((int64_t)1 << 22)
// Queue the query of n > 0 device rays into device records on the context stream: the
// scene as it stands, the context's traversal mode, a spill area sized as the guides'
// (render_guides).  Reads the scene only.  Launches of class PNRT_K_PRIMARY.
static int query_launch(pnrt_ctx* c, const float* rays, int64_t n, int kind, uint4* out) {
    int rc;
    if ((rc = trace_grid_init(c))) return rc;
    const DevScene s = launch_scene(c);
    if ((rc = c->q_ovf.reserve(c, ovf_size(c).bytes))) return rc;
    const WfBufs qb = spill_bufs(c, c->q_ovf);
    const int mode = traverse_mode(c);
    const int any = kind == PNRT_QUERY_ANY;
    for (int64_t at = 0; at < n; at += QUERY_MAX_LAUNCH) {
        const uint32_t m = (uint32_t)std::min<int64_t>(n - at, QUERY_MAX_LAUNCH);
        const auto launch = [&](auto tbl, dim3 grid) {
            hipLaunchKernelGGL((pt_query_wf<WF_STACK, decltype(tbl)::value>), grid, dim3(WF_TRACE_BLOCK), 0, c->stream, s, qb,
                               rays + 7 * at, m, any, mode, out + 4 * at);
        };
        if ((rc = trace_step(c, s, c->stream, m, launch))) return rc;
    }
    return mark_stream(c);
}
// The checks both forms share; PNRT_OK with *go = false for n == 0 (nothing to queue).
static int query_check(pnrt_ctx* c, const void* rays, int64_t n, int kind, const void* out, bool* go) {
    *go = false;
    if (!c) return PNRT_E_ARG;
    if (kind != PNRT_QUERY_CLOSEST && kind != PNRT_QUERY_ANY) return set_err(c, PNRT_E_ARG, "query_rays: unknown kind");
    if (n < 0) return set_err(c, PNRT_E_ARG, "query_rays: n < 0");
    if (n > 0 && (!rays || !out)) return set_err(c, PNRT_E_ARG, "query_rays: NULL rays or records");
    if (!c->has_scene) return set_err(c, PNRT_E_STATE, "query_rays: upload_scene first");
    if (n == 0) return PNRT_OK;
    if (int rc = check_fault(c)) return rc;      // completed work that faulted
    *go = true;
    return PNRT_OK;
}

// The images both denoisers filter in and their launch grid: the compact guide records and
// the ping-pong pair.
static int denoise_reserve(pnrt_ctx* c, dim3* grid) {
    int rc;
    const size_t pix = (size_t)c->width * c->height;
    if ((rc = c->dn_guide.reserve(c, pix * 32)) || (rc = c->dn_img[0].reserve(c, pix * 16)) ||
        (rc = c->dn_img[1].reserve(c, pix * 16)))
        return rc;
    *grid = dim3((unsigned)((c->width + 15) / 16), (unsigned)((c->height + 15) / 16));
    return PNRT_OK;
}

// Both denoisers (pt_denoise.h; VAR: pnrt_denoise_variance): the prep launch, then one launch per
// level.  sigma_c: sigma_color, halved per level (VAR: sigma_variance, the same at every level).
template <bool VAR>
static int denoise_run(pnrt_ctx* c, int levels, float sigma_c, float sigma_n, float sigma_p) {
    dim3 grid;
    if (int rc = denoise_reserve(c, &grid)) return rc;
    DenoiseParams d{};
    d.width = c->width; d.height = c->height;
    if (VAR) d.colour = sigma_c;             // (the fixed filter's is set per level, below; the prep reads neither)
    d.inv_n = 1.0f / (sigma_n * sigma_n);
    d.inv_p = 1.0f / (sigma_p * sigma_p);
    // level i reads image (first + i) & 1 and writes the other, so the last one writes dn_img[0]
    const int first = levels & 1;
    // (VAR: the moments are written by the blend launches, which this stream has queued before)
    hipLaunchKernelGGL(pt_denoise_prep<VAR>, grid, dim3(256), 0, c->stream, d, c->scene.materials, c->scene.n_materials,
                       (const float4*)c->accum, (const float4*)c->aov[PNRT_AOV_POSITION], (const float4*)c->aov[PNRT_AOV_NORMAL],
                       (const float4*)c->aov[PNRT_AOV_ALBEDO], VAR ? (const float4*)c->moments : nullptr, c->dn_guide,
                       c->dn_img[first]);
    HIPCHK(c, hipGetLastError());
    for (int i = 0; i < levels; ++i) {
        if (!VAR) {
            const float sc = sigma_c * std::ldexp(1.0f, -i);
            d.colour = 1.0f / (sc * sc);
        }
        d.step = 1 << i;
        const float4* src = c->dn_img[(first + i) & 1];
        float4* dst = c->dn_img[(first + i + 1) & 1];
        const bool last = i + 1 == levels;
        // spacings 1, 2, 4 through an LDS tile with halo, 8 and 16 through the caches (pt_denoise.h)
        auto launch = [&](auto lds_step) {
            constexpr int STEP = decltype(lds_step)::value;
            const auto kernel = last ? pt_denoise_pass<VAR, STEP, true> : pt_denoise_pass<VAR, STEP, false>;
            hipLaunchKernelGGL(kernel, grid, dim3(256), 0, c->stream, d, (const float4*)c->dn_guide, src, dst,
                               (const float4*)c->accum, (const float4*)c->aov[PNRT_AOV_ALBEDO]);
        };
        switch (d.step <= DN_LDS_MAX_STEP ? d.step : 0) {
            case 1: launch(std::integral_constant<int, 1>{}); break;
            case 2: launch(std::integral_constant<int, 2>{}); break;
            case 4: launch(std::integral_constant<int, 4>{}); break;
            default: launch(std::integral_constant<int, 0>{});
        }
        HIPCHK(c, hipGetLastError());
    }
    c->dn_width = c->width; c->dn_height = c->height;
    return mark_stream(c);
}

// A zeroed moments image of the current frame size, in place of the old one (the
// caller has waited for the calls in flight).
static int moments_alloc(pnrt_ctx* c) {
    const size_t bytes = (size_t)c->width * c->height * 16;
    HIPCHK(c, c->moments.alloc(bytes));
    HIPCHK(c, hipMemsetAsync(c->moments, 0, bytes, c->stream));
    c->mom_cover = true;             // first enabled, or zeroed with the accumulation (a resize)
    return mark_stream(c);
}

// ---- preconditions several entry points share: PNRT_OK, or the error set in `who`'s name -------
// (The two denoisers keep their own: they ask for the accumulation image and the guide images as
// well, and tests/test_denoise_variance_api.py reads pnrt_denoise_variance's messages from its body.)
static int need_scene_frame(pnrt_ctx* c, const char* who) {
    if (!c->has_scene || !c->has_frame) return set_err(c, PNRT_E_STATE, std::string(who) + ": upload_scene and set_frame first");
    return PNRT_OK;
}
static int check_selector(pnrt_ctx* c, const char* who, int band, int nsh, int shard) {
    if (band < 1 || nsh < 1 || shard < 0 || shard >= nsh) return set_err(c, PNRT_E_ARG, std::string(who) + ": bad shard selector");
    return PNRT_OK;
}
// frame 0xFFFFFFFF has the blend weight 1 / (float)0 (frameCount + 1 wraps), and the
// frames after it would restart at 0: refused before anything is queued
static int check_frame_range(pnrt_ctx* c, const char* who, uint32_t first, uint32_t nf) {
    if ((uint64_t)first + nf > 0xFFFFFFFFull)
        return set_err(c, PNRT_E_ARG, std::string(who) + ": first_frame + n_frames exceeds 0xFFFFFFFF (the last frame number is 0xFFFFFFFE)");
    return PNRT_OK;
}
// there is a moments image to read
static int need_moments_image(pnrt_ctx* c, const char* who) {
    if (!c->moments_ever) return set_err(c, PNRT_E_STATE, std::string(who) + ": enable_moments first");
    if (!c->moments) return set_err(c, PNRT_E_STATE, std::string(who) + ": no frame");
    return PNRT_OK;
}
// the sample moments are enabled and count every frame the accumulation holds
static int need_moments(pnrt_ctx* c, const char* who) {
    if (!c->moments_on || !c->moments)
        return set_err(c, PNRT_E_STATE, std::string(who) + ": the sample moments are not enabled (pnrt_enable_moments(ctx, 1) first)");
    if (!c->mom_cover)
        return set_err(c, PNRT_E_STATE, std::string(who) + ": frames were rendered while the moments were disabled, so they do not "
                                              "cover the accumulation (pnrt_reset_accum first)");
    return PNRT_OK;
}

// The stretch the frame-rendering entry points share once their arguments have passed: the faults of
// completed work, then the call's frame parameters and the scene as its kernels take it.  A call of no
// frames, or whose shard has no rows, queues nothing (each entry point returns there in its own way).
static int frame_call(pnrt_ctx* c, uint32_t first, uint32_t nf, int band, int nsh, int shard, FrameParams* fp, DevScene* s) {
    if (int rc = check_fault(c)) return rc;      // an earlier call's trace fault (completed work)
    if (nf) HIPCHK(c, hipSetDevice(c->device));
    *fp = frame_params(c, c->cam, first, nf, band, nsh, shard);
    *s = launch_scene(c);
    return PNRT_OK;
}
// frames the sample moments do not count (pnrt_render_adaptive refuses from then on)
static void moments_uncover(pnrt_ctx* c) {
    if (!c->moments_on) c->mom_cover = false;
}

// The tail of the pnrt_read_* calls: `bytes` of a device image to the caller behind everything
// queued, then the faults of the work that completed.
static int read_back(pnrt_ctx* c, void* out, const void* src, size_t bytes) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, sync_all(c));
    return check_fault(c);
}

// What a new context holds on its device (pnrt_create).  A failure leaves the context as
// far as it got, for pnrt_destroy.
static int ctx_init(pnrt_ctx* c) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    // the pipelined renderer's worker streams are created with the context, so
    // they take hardware queues of their own before the caller creates more streams
    if (int rc = pipes_init(c)) return rc;
    void* fd = nullptr;
    HIPCHK(c, c->fault_host.alloc(256, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(c, hipHostGetDevicePointer(&fd, c->fault_host, 0));
    std::memset(c->fault_host, 0, 256);
    c->fault_dev = static_cast<uint32_t*>(fd);
    HIPCHK(c, hipMemcpyToSymbol(HIP_SYMBOL(c_sobolV), kSobolV, sizeof kSobolV));
    float lut[256];
    for (int i = 0; i < 256; ++i) lut[i] = (float)i / 255.0f;   // GL UNORM8 -> float
    HIPCHK(c, c->unorm8.alloc(sizeof lut));
    HIPCHK(c, hipMemcpy(c->unorm8, lut, sizeof lut, hipMemcpyHostToDevice));
    return PNRT_OK;
}

extern "C" {

#ifndef PNRT_SRC_HASH
#define PNRT_SRC_HASH "unknown"
#endif
// the build stamps the sha256 of the device sources (pnraytracing_amd/build.py),
// so a stale prebuilt library shipped beside newer sources is detectable
const char* pnrt_version(void) {
    return PNRT_IS_DIAG_BUILD ? "pnrt-mi355x 0.2 (gfx950) DIAGNOSTIC BUILD src " PNRT_SRC_HASH
                              : "pnrt-mi355x 0.2 (gfx950) src " PNRT_SRC_HASH;
}

int pnrt_create(int device, pnrt_ctx** out) {
    if (!out) return PNRT_E_ARG;
    *out = nullptr;
    // a caller short of device memory (another tenant, a smaller part) caps one batch's
    // buffers; frames per batch shrink to fit, which changes no pixel.  Read here, once,
    // and strictly: a misspelt cap must not turn into a 3-byte cap or into none
    // (there is no context yet to carry a message: the code is the report)
    uint64_t cap = 0;
    const char* bb = getenv("PNRT_BATCH_BYTES");
    if (bb && !parse_batch_bytes(bb, &cap)) return PNRT_E_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return PNRT_E_HIP;
    pnrt_ctx* c = new pnrt_ctx();
    c->device = device;
    c->batch_bytes_cap = (size_t)cap;
    if (ctx_init(c) != PNRT_OK) {
        pnrt_destroy(c);
        return PNRT_E_HIP;
    }
    *out = c;
    return PNRT_OK;
}

// The streams and events are destroyed here, and only here; the buffers go with the context.
// (Also pnrt_create's failure path: any of the streams and events may not exist yet.)
void pnrt_destroy(pnrt_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)sync_all(c);
    for (auto& P : c->pipe) {
        if (P.w) (void)hipStreamDestroy(P.w);
        for (hipEvent_t e : {P.ev_join, P.ev_blend, P.ev_stage, P.ev_rays})
            if (e) (void)hipEventDestroy(e);
    }
    for (auto& S : c->cam_stage)
        if (S.ev) (void)hipEventDestroy(S.ev);
    for (auto& p : c->ev_pending) { c->ev_pool.push_back(p.second.first); c->ev_pool.push_back(p.second.second); }
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    if (c->ev_last) (void)hipEventDestroy(c->ev_last);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

const char* pnrt_last_error(pnrt_ctx* c) { return c ? c->err.c_str() : "null context"; }

void* pnrt_get_stream(pnrt_ctx* c) { return c ? static_cast<void*>(c->own_stream) : nullptr; }

int pnrt_set_stream(pnrt_ctx* c, void* s) {
    if (!c) return PNRT_E_ARG;
    hipStream_t ns = s ? static_cast<hipStream_t>(s) : c->own_stream;
    if (ns == c->stream) return PNRT_OK;
    // blends (frame-ordered read-modify-writes of accum), pack_rows and
    // read_accum run on c->stream: the new stream starts after the last op the
    // context queued on the old one (ev_last, recorded with it), so no blend of
    // a later call overtakes a pending one -- and the old stream itself is not
    // touched (the caller may have destroyed it since)
    HIPCHK(c, hipSetDevice(c->device));
    if (c->last_valid) HIPCHK(c, hipStreamWaitEvent(ns, c->ev_last, 0));
    c->stream = ns;
    return PNRT_OK;
}

int pnrt_set_options(pnrt_ctx* c, int options) {
    if (!c) return PNRT_E_ARG;
    int mode = options & 0xff;
    if ((mode != PNRT_TRAVERSE_EXACT && mode != PNRT_TRAVERSE_ZCULL) || (options & ~0x3ff))
        return set_err(c, PNRT_E_ARG, "unknown option bits");
    c->mode = mode;
    c->kernel = (options & PNRT_KERNEL_V1) ? 1 : 3;
    const bool serial = (options & PNRT_SERIAL) != 0;
    if (serial != c->serial) HIPCHK(c, sync_all(c));   // the pipe rotation restarts from an idle context
    c->serial = serial;
    return PNRT_OK;
}

// DevScene::emit_max (pt_wf.h WF_SKIP_MOOT): a bound on every component of the
// emission a continuation ray can bring back -- any material's, or the env
// radiance (bilinear taps of the texels: 2^-16 above the largest texel covers the
// filter's rounding).  A NaN anywhere makes it NaN (then nothing is found moot).
static float abs_max(const float* v, size_t n, float m) {
    for (size_t k = 0; k < n; ++k) {
        const float a = std::fabs(v[k]);
        if (std::isnan(a) || std::isnan(m)) return std::numeric_limits<float>::quiet_NaN();
        m = std::max(m, a);
    }
    return m;
}
static void set_emit_max(pnrt_ctx* c) {
    float m = abs_max(c->mat_emit.data(), c->mat_emit.size(), 0.f);
    if (c->scene.has_hdr) {
        const float e = c->env_max * (1.0f + 0x1p-16f);
        m = (std::isnan(e) || std::isnan(m)) ? std::numeric_limits<float>::quiet_NaN() : std::max(m, e);
    }
    c->scene.emit_max = m;
}

// The light list's prefix areas as the kernels take them (pnrt_upload_scene,
// pnrt_update_vertices): lights_sum_area, and the kernel-argument copy of a short list.
// GetLightIndex is a lower bound: a linear scan returns the same index iff the
// prefix areas are non-decreasing (they are for main.cpp:374-383's list)
static void set_light_areas(DevScene& s, const std::vector<float2>& lights, int nl, float lsum) {
    s.lights_sum_area = lsum;
    bool mono = nl <= WF_LIGHT_SCAN;
    for (int k = 1; mono && k < nl; ++k) mono = lights[k].y >= lights[k - 1].y;
    for (int k = 0; mono && k < nl; ++k) mono = lights[k].y == lights[k].y;
    s.light_scan = mono ? 1 : 0;
    for (int k = 0; k < WF_LIGHT_SCAN; ++k) s.lscan[k] = k < nl ? lights[k].y : 0.f;
}

int pnrt_upload_scene(pnrt_ctx* c, const float* V, int nv, const float* M, int nm, const float* T, int nt,
                      const float* N, int nn, const float* Lt, int nl, float lsum) {
    if (!c) return PNRT_E_ARG;
    if (!V || !M || !T || !N || nv <= 0 || nm <= 0 || nt <= 0 || nn <= 0 || nl < 0 || (nl > 0 && !Lt))
        return set_err(c, PNRT_E_ARG, "upload_scene: missing or empty arrays");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_all(c));
    free_scene(c);
    c->scene_bytes = 0;
    ++c->scene_epoch;                    // primary records of the old scene are stale

    // triangles: positions gathered in BVH order, ids validated
    std::vector<float4> tris((size_t)nt * 3 + 1);   // +1: the trace kernel reads 64 B per record
    std::vector<int4> tidx(nt);
    for (int i = 0; i < nt; ++i) {
        const float* t = T + 6 * (size_t)i;
        int id[3] = {fint(t[0]), fint(t[1]), fint(t[2])};
        for (int k = 0; k < 3; ++k)
            if (id[k] < 0 || id[k] >= nv) return set_err(c, PNRT_E_SCENE, "triangle " + std::to_string(i) + " has an out-of-range vertex index");
        int mat = fint(t[3]), tex = fint(t[4]);
        if (mat < 0 || mat >= nm) return set_err(c, PNRT_E_SCENE, "triangle " + std::to_string(i) + " has an out-of-range material id");
        // the reference binds PT_MAX_TEXTURES samplers; the wavefront records keep tex + 1 in 8 bits
        if (tex < -1 || tex >= PT_MAX_TEXTURES) return set_err(c, PNRT_E_SCENE, "triangle " + std::to_string(i) + " has an out-of-range texture id");
        const float* p0 = V + 15 * (size_t)id[0];
        const float* p1 = V + 15 * (size_t)id[1];
        const float* p2 = V + 15 * (size_t)id[2];
        float4 a, b, d;
        a.x = p0[0]; a.y = p0[1]; a.z = p0[2]; a.w = p1[0];
        b.x = p1[1]; b.y = p1[2]; b.z = p2[0]; b.w = p2[1];
        d.x = p2[2];
        std::memcpy(&d.y, &mat, 4); std::memcpy(&d.z, &tex, 4); d.w = 0.f;
        tris[3 * (size_t)i] = a; tris[3 * (size_t)i + 1] = b; tris[3 * (size_t)i + 2] = d;
        tidx[i] = make_int4(id[0], id[1], id[2], 0);
    }
    std::vector<float4> verts((size_t)nv * 2);
    for (int i = 0; i < nv; ++i) {
        const float* v = V + 15 * (size_t)i;
        verts[2 * (size_t)i] = make_float4(v[0], v[1], v[2], v[3]);
        verts[2 * (size_t)i + 1] = make_float4(v[4], v[5], v[12], v[13]);
    }
    // per-triangle shading attributes (normals, uvs of its three vertices), so a
    // hit's attributes are one fetch away from the triangle index instead of two
    std::vector<float4> tattr((size_t)nt * 4);
    for (int i = 0; i < nt; ++i) {
        const float* v0 = V + 15 * (size_t)tidx[i].x;
        const float* v1 = V + 15 * (size_t)tidx[i].y;
        const float* v2 = V + 15 * (size_t)tidx[i].z;
        tattr[4 * (size_t)i + 0] = make_float4(v0[3], v0[4], v0[5], v1[3]);
        tattr[4 * (size_t)i + 1] = make_float4(v1[4], v1[5], v2[3], v2[4]);
        tattr[4 * (size_t)i + 2] = make_float4(v2[5], v0[12], v0[13], v1[12]);
        tattr[4 * (size_t)i + 3] = make_float4(v1[13], v2[12], v2[13], 0.f);
    }
    // BVH: validate the reference tree (pre-order, left = id + 1) from the root,
    // number interior nodes, and store child boxes in the parent.
    std::vector<int> dn(nn, -1), depth(nn, 0), order;
    std::vector<int> st{0};
    std::vector<char> seen(nn, 0);
    int maxd = 0;
    while (!st.empty()) {
        int i = st.back(); st.pop_back();
        if (i < 0 || i >= nn || seen[i]) return set_err(c, PNRT_E_SCENE, "BVH node array is not a tree");
        seen[i] = 1;
        const float* n = N + 12 * (size_t)i;
        int rc = fint(n[7]), s0 = fint(n[8]), e0 = fint(n[9]);
        if (rc == -1) {
            if (s0 < 0 || e0 > nt || s0 > e0) return set_err(c, PNRT_E_SCENE, "BVH leaf with bad triangle range");
            continue;
        }
        int ax = fint(n[6]);
        if (ax < 0 || ax > 2 || i + 1 >= nn || rc <= 0 || rc >= nn) return set_err(c, PNRT_E_SCENE, "BVH interior node with bad axis/children");
        dn[i] = (int)order.size();
        order.push_back(i);
        depth[i + 1] = depth[rc] = depth[i] + 1;
        if (depth[i] + 1 > maxd) maxd = depth[i] + 1;
        st.push_back(rc);
        st.push_back(i + 1);
    }
    if (maxd >= PT_STACK - 1)
        return set_err(c, PNRT_E_SCENE, "BVH depth " + std::to_string(maxd) + " exceeds the kernel stack");
    // device numbering: breadth-first, so the top levels are the first indices
    // (the top levels share cache lines); the visit order is
    // carried by the child refs and the axis, not by the numbering
    order.clear();
    std::vector<int> level_off;              // depth is non-decreasing along the order: one index range per level
    if (fint(N[7]) != -1) order.push_back(0);
    for (size_t q = 0; q < order.size(); ++q) {
        const int i = order[q];
        dn[i] = (int)q;
        if (depth[i] == (int)level_off.size()) level_off.push_back((int)q);
        const float* n = N + 12 * (size_t)i;
        const int rc = fint(n[7]);
        if (fint(N[12 * (size_t)(i + 1) + 7]) != -1) order.push_back(i + 1);
        if (fint(N[12 * (size_t)rc + 7]) != -1) order.push_back(rc);
    }
    // child reference (pt_common.h): interior -> node index, leaf -> range, in the
    // packed encoding when every leaf fits it, else the wide one (+ leaf table)
    bool packed = nt < (1 << 24) - 1;
    for (size_t i = 0; i < (size_t)nn && packed; ++i) {
        const float* n = N + 12 * i;
        if (fint(n[7]) == -1 && fint(n[9]) - fint(n[8]) > 127) packed = false;
    }
    std::vector<int2> leaf_table;
    auto childref = [&](int ci) -> uint32_t {
        const float* n = N + 12 * (size_t)ci;
        if (fint(n[7]) != -1) return (uint32_t)dn[ci];
        int s0 = fint(n[8]), cnt = fint(n[9]) - s0;
        if (cnt <= 0) return REF_LEAF;
        if (packed) return REF_LEAF | ((uint32_t)cnt << 24) | (uint32_t)s0;
        if (cnt <= 127 && s0 < (1 << 23)) return REF_LEAF | ((uint32_t)s0 << 7) | (uint32_t)cnt;
        leaf_table.push_back(make_int2(s0, cnt));
        return REF_LEAF | REF_TABLE | (uint32_t)(leaf_table.size() - 1);
    };
    if ((int64_t)order.size() >= (1 << 25)) return set_err(c, PNRT_E_SCENE, "too many BVH nodes (2 GB node buffer limit)");
    if (nm >= (1 << 24)) return set_err(c, PNRT_E_SCENE, "too many materials");
    std::vector<float4> nodes(order.size() * 4);
    for (size_t k = 0; k < order.size(); ++k) {
        int i = order[k];
        const float* n = N + 12 * (size_t)i;
        int rc = fint(n[7]);
        const float* L = N + 12 * (size_t)(i + 1);
        const float* R = N + 12 * (size_t)rc;
        nodes[4 * k + 0] = make_float4(L[0], L[1], L[2], L[3]);
        nodes[4 * k + 1] = make_float4(L[4], L[5], R[0], R[1]);
        nodes[4 * k + 2] = make_float4(R[2], R[3], R[4], R[5]);
        uint32_t meta[4] = {childref(i + 1), childref(rc), 16u << fint(n[6]), (uint32_t)fint(n[6])};
        std::memcpy(&nodes[4 * k + 3], meta, 16);
    }
    uint32_t root_ref = childref(0);
    const int has_leaf_table = packed ? 0 : 1;
    if (leaf_table.empty()) leaf_table.push_back(make_int2(0, 0));

    // trace-kernel stack bound: at most one deferred sibling per BVH level
    c->wf_stack_need = maxd + 2;
    std::vector<float2> lights(nl > WF_LIGHT_SCAN ? nl : WF_LIGHT_SCAN, make_float2(0.f, 0.f));
    std::vector<int> light_tri(nl);
    for (int i = 0; i < nl; ++i) {
        lights[i] = make_float2(Lt[3 * (size_t)i], Lt[3 * (size_t)i + 1]);
        int li = fint(Lt[3 * (size_t)i]);
        if (li < 0 || li >= nt) return set_err(c, PNRT_E_SCENE, "light references an out-of-range triangle");
        light_tri[i] = li;
    }
    std::vector<float> mats(M, M + 18 * (size_t)nm);
    // light records: what TriangleSample (:598-624) and the emission (:887) read for
    // light entry k -- its triangle's vertex records and material emission -- in one
    // place; entry nl is triangle 0 (GetLightIndex's fallback index)
    std::vector<float4> lrec((size_t)(nl + 1) * 7);
    c->light_mat.assign((size_t)nl + 1, 0);
    for (int e = 0; e <= nl; ++e) {
        const int t = e < nl ? fint(Lt[3 * (size_t)e]) : 0;
        for (int k = 0; k < 3; ++k) {
            const int vi = k == 0 ? tidx[t].x : (k == 1 ? tidx[t].y : tidx[t].z);
            lrec[7 * (size_t)e + 2 * k] = verts[2 * (size_t)vi];
            lrec[7 * (size_t)e + 2 * k + 1] = verts[2 * (size_t)vi + 1];
        }
        const int mat = fint(T[6 * (size_t)t + 3]);
        const float* em = M + 18 * (size_t)mat;
        lrec[7 * (size_t)e + 6] = make_float4(em[0], em[1], em[2], 0.f);
        c->light_mat[e] = mat;
    }
    c->light_rec_host = lrec;

    DevScene& s = c->scene;
    int rc;
    {   // nodes and triangle records in one allocation: the trace kernel addresses both
        // through one buffer resource with 32-bit offsets
        const size_t nb = nodes.size() * 16, tb = tris.size() * 16;
        if (nb + tb >= ((size_t)1 << 32) - 64)
            return set_err(c, PNRT_E_SCENE, "scene too large: nodes + triangles must stay below 4 GiB");
        void* g = nullptr;
        HIPCHK(c, scene_block(c, nb + tb, &g));
        if (nb) HIPCHK(c, hipMemcpy(g, nodes.data(), nb, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(static_cast<char*>(g) + nb, tris.data(), tb, hipMemcpyHostToDevice));
        c->scene_bytes += (int64_t)(nb + tb);
        s.nodes = static_cast<const float4*>(g);
        s.tris = reinterpret_cast<const float4*>(static_cast<char*>(g) + nb);
        s.geo_tri_off = (uint32_t)nb;
        s.geo_bytes = (uint32_t)(nb + tb);
    }
    if ((rc = upload(c, leaf_table, &s.leaf_table)) || (rc = upload(c, tidx, &s.tri_idx)) ||
        (rc = upload(c, verts, &s.verts)) || (rc = upload(c, mats, &s.materials)) || (rc = upload(c, lights, &s.lights)) ||
        (rc = upload(c, tattr, &s.tri_attr)) || (rc = upload(c, lrec, &s.light_rec)) ||
        (rc = upload(c, std::vector<float4>(1, make_float4(0.f, 0.f, 0.f, 0.f)), &s.zero4)))
        return rc;
    s.n_nodes = (int)order.size(); s.n_tris = nt; s.n_verts = nv; s.n_materials = nm; s.n_lights = nl;
    const float* root = N;
    for (int k = 0; k < 3; ++k) { s.root_min[k] = root[k]; s.root_max[k] = root[3 + k]; }
    // z-slab culling's proof needs finite boxes (then a culling-enabled ray's
    // z-slab distances are never NaN); a scene with a non-finite box coordinate
    // is traversed without culling, which is the reference's exact traversal
    c->boxes_finite = true;
    for (size_t i = 0; i < (size_t)nn && c->boxes_finite; ++i)
        for (int k = 0; k < 6; ++k)
            if (!std::isfinite(N[12 * i + k])) { c->boxes_finite = false; break; }
    s.root_ref = root_ref;
    s.has_leaf_table = has_leaf_table;
    s.n_leaf_table = (int)leaf_table.size();
    set_light_areas(s, lights, nl, lsum);
    c->light_tri = light_tri;
    level_off.push_back((int)order.size());
    c->level_off = level_off;
    c->mat_emit.resize(3 * (size_t)nm);
    for (int m = 0; m < nm; ++m)
        for (int k = 0; k < 3; ++k) c->mat_emit[3 * (size_t)m + k] = M[18 * (size_t)m + k];
    set_emit_max(c);
    c->root_is_leaf = fint(root[7]) == -1;
    c->n_interior = (int)order.size();
    c->max_depth = maxd;
    c->has_scene = true;
    return PNRT_OK;
}

int pnrt_update_materials(pnrt_ctx* c, int first, int count, const float* rec) {
    if (!c) return PNRT_E_ARG;
    if (!c->has_scene) return set_err(c, PNRT_E_STATE, "update_materials: upload_scene first");
    if (first < 0 || count < 0 || first > c->scene.n_materials - count || (count > 0 && !rec))
        return set_err(c, PNRT_E_ARG, "update_materials: material range outside the uploaded array");
    if (count == 0) return PNRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    // the calls in flight render with the old records (the reference's
    // glTexSubImage1D is ordered after the dispatches issued before it)
    HIPCHK(c, sync_all(c));
    HIPCHK(c, hipMemcpy(const_cast<float*>(c->scene.materials) + 18 * (size_t)first, rec, 18 * sizeof(float) * (size_t)count,
                        hipMemcpyHostToDevice));
    // light records carry a copy of their triangle's emission (upload_scene): patched
    // in the host copy, then the span of changed records goes up in ONE copy (an
    // emissive mesh of thousands of light triangles sharing one material is one
    // transfer per edit, as the reference's single glTexSubImage1D)
    size_t lo = c->light_mat.size(), hi = 0;
    for (size_t e = 0; e < c->light_mat.size(); ++e) {
        const int m = c->light_mat[e];
        if (m < first || m >= first + count) continue;
        const float* em = rec + 18 * (size_t)(m - first);
        c->light_rec_host[7 * e + 6] = make_float4(em[0], em[1], em[2], 0.f);
        lo = std::min(lo, e);
        hi = e + 1;
    }
    if (lo < hi)
        HIPCHK(c, hipMemcpy(const_cast<float4*>(c->scene.light_rec) + 7 * lo, c->light_rec_host.data() + 7 * lo,
                            (hi - lo) * 7 * sizeof(float4), hipMemcpyHostToDevice));
    for (int m = 0; m < count; ++m)
        for (int k = 0; k < 3; ++k) c->mat_emit[3 * (size_t)(first + m) + k] = rec[18 * (size_t)m + k];
    set_emit_max(c);
    ++c->scene_epoch;                    // primary records hold the hit material's emission
    return PNRT_OK;
}

#ifndef REFIT_MAX_STAGE
#define REFIT_MAX_STAGE (1 << 20)    // vertex records per staged copy of the host form (60 MB)
#endif

// The tail of every edit of `verts` (pnrt_update_vertices, pnrt_place_models), queued behind the writes
// on the context's stream: every per-triangle record regathered, the light records, the leaves, the
// levels, the root box and the non-finite flag, the host copy of the light records -- then the scene
// is another one.  c->rf_res is reserved by the caller, before it changes anything.
static int refit_tail(pnrt_ctx* c) {
    DevScene& s = c->scene;
    hipStream_t st = c->stream;
    const int nl = s.n_lights;
    float4* nodes = const_cast<float4*>(s.nodes);
    RefitResult res0{};
    for (int k = 0; k < 3; ++k) { res0.root[k] = s.root_min[k]; res0.root[3 + k] = s.root_max[k]; }
    HIPCHK(c, hipMemcpyAsync(c->rf_res, &res0, sizeof res0, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(pt_refit_gather_kernel, dim3((s.n_tris + 255) / 256), dim3(256), 0, st, s.tri_idx, s.verts,
                       const_cast<float4*>(s.tris), const_cast<float4*>(s.tri_attr), s.n_tris, s.n_verts);
    hipLaunchKernelGGL(pt_refit_lights_kernel, dim3((nl + 1 + 255) / 256), dim3(256), 0, st, s.lights, s.tri_idx, s.verts,
                       const_cast<float4*>(s.light_rec), nl, s.n_tris, s.n_verts);
    const int nn = s.n_nodes;
    hipLaunchKernelGGL(pt_refit_leaves_kernel, dim3(nn ? (2 * (unsigned)nn + 255) / 256 : 1), dim3(256), 0, st, nodes, nn,
                       s.tris, s.n_tris, s.leaf_table, s.n_leaf_table, s.has_leaf_table, s.root_ref, c->rf_res);
    // the deepest level has leaf children only; level 0 is the root's launch
    const int levels = (int)c->level_off.size() - 1;
    for (int d = levels - 2; d >= 1; --d) {
        const int lo = c->level_off[d], hi = c->level_off[d + 1];
        hipLaunchKernelGGL(pt_refit_level_kernel, dim3((2 * (unsigned)(hi - lo) + 255) / 256), dim3(256), 0, st, nodes, nn, lo,
                           hi, 0, c->rf_res);
    }
    if (nn > 0) hipLaunchKernelGGL(pt_refit_level_kernel, dim3(1), dim3(64), 0, st, nodes, nn, 0, 1, 1, c->rf_res);
    HIPCHK(c, hipGetLastError());
    RefitResult res{};
    HIPCHK(c, hipMemcpyAsync(&res, c->rf_res, sizeof res, hipMemcpyDeviceToHost, st));
    // pnrt_update_materials patches the host copy of the light records and uploads spans of it
    HIPCHK(c, hipMemcpyAsync(c->light_rec_host.data(), s.light_rec, c->light_rec_host.size() * sizeof(float4),
                             hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    for (int k = 0; k < 3; ++k) { s.root_min[k] = res.root[k]; s.root_max[k] = res.root[3 + k]; }
    c->boxes_finite = res.nonfinite == 0;
    ++c->scene_epoch;                    // primary records, guide images: traced through the old geometry
    return PNRT_OK;
}

// pnrt_update_vertices / _device: `src_host` or `src_dev` holds the records (pt_refit.h)
static int update_vertices(pnrt_ctx* c, const char* who, int first, int count, const float* src_host, const float* src_dev,
                           const float* Lt, float lsum) {
    if (!c) return PNRT_E_ARG;
    if (!c->has_scene) return set_err(c, PNRT_E_STATE, std::string(who) + ": upload_scene first");
    DevScene& s = c->scene;
    if (first < 0 || count < 0 || first > s.n_verts - count)
        return set_err(c, PNRT_E_ARG, std::string(who) + ": vertex range outside the uploaded array");
    if (count > 0 && !src_host && !src_dev) return set_err(c, PNRT_E_ARG, std::string(who) + ": vertices is NULL");
    if ((uintptr_t)src_dev & 3u) return set_err(c, PNRT_E_ARG, std::string(who) + ": vertices must be 4-byte aligned");
    if (count == 0 && !Lt) return PNRT_OK;
    const int nl = s.n_lights;
    std::vector<float2> lights;
    if (Lt) {
        lights.assign(nl > WF_LIGHT_SCAN ? nl : WF_LIGHT_SCAN, make_float2(0.f, 0.f));
        for (int i = 0; i < nl; ++i) {
            if (fint(Lt[3 * (size_t)i]) != c->light_tri[i])
                return set_err(c, PNRT_E_ARG, std::string(who) + ": lights entry " + std::to_string(i) + " names triangle " +
                                                  std::to_string(fint(Lt[3 * (size_t)i])) + ", the uploaded one " +
                                                  std::to_string(c->light_tri[i]) + " (the light list cannot change)");
            lights[i] = make_float2(Lt[3 * (size_t)i], Lt[3 * (size_t)i + 1]);
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    // the calls in flight render with the old geometry
    HIPCHK(c, sync_all(c));
    if (count > 0) {
        int rc;
        if ((rc = c->rf_res.reserve(c, sizeof(RefitResult)))) return rc;
        if (src_host && (rc = c->rf_stage.reserve(c, (size_t)std::min(count, REFIT_MAX_STAGE) * 60))) return rc;
        hipStream_t st = c->stream;
        float4* verts = const_cast<float4*>(s.verts);
        if (src_dev)
            hipLaunchKernelGGL(pt_refit_scatter_kernel, dim3((count + 255) / 256), dim3(256), 0, st, src_dev, verts, first, count,
                               s.n_verts);
        else
            for (int at = 0; at < count; at += REFIT_MAX_STAGE) {
                const int m = std::min(count - at, REFIT_MAX_STAGE);
                // (a pageable copy: the staging buffer is free again when it returns)
                HIPCHK(c, hipMemcpyAsync(c->rf_stage, src_host + 15 * (size_t)at, (size_t)m * 60, hipMemcpyHostToDevice, st));
                hipLaunchKernelGGL(pt_refit_scatter_kernel, dim3((m + 255) / 256), dim3(256), 0, st, c->rf_stage, verts, first + at, m,
                                   s.n_verts);
                HIPCHK(c, hipStreamSynchronize(st));
            }
        if ((rc = refit_tail(c))) return rc;
    } else ++c->scene_epoch;             // (the areas alone)
    if (Lt) {
        HIPCHK(c, hipMemcpy(const_cast<float2*>(s.lights), lights.data(), lights.size() * sizeof(float2), hipMemcpyHostToDevice));
        set_light_areas(s, lights, nl, lsum);
    }
    return check_fault(c);
}

int pnrt_update_vertices(pnrt_ctx* c, int first, int count, const float* v, const float* lights, float lsum) {
    return update_vertices(c, "update_vertices", first, count, v, nullptr, lights, lsum);
}

int pnrt_update_vertices_device(pnrt_ctx* c, int first, int count, const void* v, const float* lights, float lsum) {
    return update_vertices(c, "update_vertices_device", first, count, nullptr, static_cast<const float*>(v), lights, lsum);
}

// pnrt_define_model / _device: `src_host` or `src_dev` holds the model-space records (pt_place.h)
static int define_model(pnrt_ctx* c, const char* who, int first, int count, const float* src_host, const void* src_dev, int* id_out) {
    if (!c) return PNRT_E_ARG;
    if (!c->has_scene) return set_err(c, PNRT_E_STATE, std::string(who) + ": upload_scene first");
    if (count < 1) return set_err(c, PNRT_E_ARG, std::string(who) + ": a model has at least one vertex");
    if (first < 0 || first > c->scene.n_verts - count)
        return set_err(c, PNRT_E_ARG, std::string(who) + ": vertex range outside the uploaded array");
    if (!src_host && !src_dev) return set_err(c, PNRT_E_ARG, std::string(who) + ": records is NULL");
    if (!id_out) return set_err(c, PNRT_E_ARG, std::string(who) + ": model_id_out is NULL");
    if ((uintptr_t)src_dev & 3u) return set_err(c, PNRT_E_ARG, std::string(who) + ": records must be 4-byte aligned");
    for (size_t m = 0; m < c->models.size(); ++m)
        if (first < c->models[m].first + c->models[m].count && c->models[m].first < first + count)
            return set_err(c, PNRT_E_ARG, std::string(who) + ": vertices " + std::to_string(first) + " .. " +
                                              std::to_string(first + count - 1) + " overlap model " + std::to_string(m));
    HIPCHK(c, hipSetDevice(c->device));
    pnrt_ctx::PlaceModel m;
    m.first = first;
    m.count = count;
    const size_t bytes = (size_t)count * 32;
    HIPCHK(c, m.rec.alloc(bytes));
    HIPCHK(c, hipMemcpyAsync(m.rec, src_host ? (const void*)src_host : src_dev, bytes,
                             src_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->models.push_back(std::move(m));
    *id_out = (int)c->models.size() - 1;
    return PNRT_OK;
}

int pnrt_define_model(pnrt_ctx* c, int first, int count, const float* model8, int* id_out) {
    return define_model(c, "define_model", first, count, model8, nullptr, id_out);
}

int pnrt_define_model_device(pnrt_ctx* c, int first, int count, const void* model8, int* id_out) {
    return define_model(c, "define_model_device", first, count, nullptr, model8, id_out);
}

int pnrt_place_models(pnrt_ctx* c, const pnrt_placement* pl, int n, int relight) {
    if (!c) return PNRT_E_ARG;
    if (!c->has_scene) return set_err(c, PNRT_E_STATE, "place_models: upload_scene first");
    if (n < 1 || n > PLACE_MAX) return set_err(c, PNRT_E_ARG, "place_models: 1 .. " + std::to_string(PLACE_MAX) + " placements a call");
    if (!pl) return set_err(c, PNRT_E_ARG, "place_models: placements is NULL");
    if (relight != 0 && relight != 1) return set_err(c, PNRT_E_ARG, "place_models: relight is 0 or 1");
    DevScene& s = c->scene;
    std::vector<PlaceEntry> table((size_t)n);
    std::vector<char> placed(c->models.size(), 0);
    int total = 0;
    for (int k = 0; k < n; ++k) {
        const std::string who = "place_models: placement " + std::to_string(k);
        if (pl[k].reserved != 0) return set_err(c, PNRT_E_ARG, who + ": reserved must be 0");
        if (pl[k].model < 0 || (size_t)pl[k].model >= c->models.size())
            return set_err(c, PNRT_E_ARG, who + " names the unknown model " + std::to_string(pl[k].model));
        if (placed[pl[k].model]) return set_err(c, PNRT_E_ARG, who + " names model " + std::to_string(pl[k].model) + " a second time");
        placed[pl[k].model] = 1;
        for (int j = 0; j < 16; ++j)
            if (!std::isfinite(pl[k].matrix[j])) return set_err(c, PNRT_E_ARG, who + ": matrix float " + std::to_string(j) + " is not finite");
        const pnglm::mat4 M = pnglm::mat4::load(pl[k].matrix), N = pnglm::normal_matrix(M);
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j)
                if (!std::isfinite(N.c[i][j])) return set_err(c, PNRT_E_ARG, who + ": the matrix is singular (its normal matrix is not finite)");
        const pnrt_ctx::PlaceModel& m = c->models[pl[k].model];
        PlaceEntry& e = table[k];
        e.prefix = total;
        e.first = m.first;
        e.model = m.rec;
        for (int r = 0; r < 3; ++r) {
            e.M[r] = make_float4(M.c[0][r], M.c[1][r], M.c[2][r], M.c[3][r]);
            e.N[r] = make_float4(N.c[0][r], N.c[1][r], N.c[2][r], N.c[3][r]);
        }
        total += m.count;                 // (disjoint ranges of one array: at most n_verts)
    }
    HIPCHK(c, hipSetDevice(c->device));
    // the calls in flight render with the old geometry
    HIPCHK(c, sync_all(c));
    int rc;
    if ((rc = c->rf_res.reserve(c, sizeof(RefitResult))) || (rc = c->pl_table.reserve(c, PLACE_MAX * sizeof(PlaceEntry)))) return rc;
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(c->pl_table, table.data(), table.size() * sizeof(PlaceEntry), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(pt_place_kernel, dim3((total + 255) / 256), dim3(256), 0, st, c->pl_table, n, total,
                       const_cast<float4*>(s.verts), s.n_verts);
    if ((rc = refit_tail(c))) return rc;
    if (relight) {
        // the areas of the light triangles as ModelOutput has them, from the records just read back; the
        // float prefix of main.cpp:374-383
        const int nl = s.n_lights;
        std::vector<float2> lights(nl > WF_LIGHT_SCAN ? nl : WF_LIGHT_SCAN, make_float2(0.f, 0.f));
        float prefix = 0.f;
        for (int e = 0; e < nl; ++e) {
            const float4* r = c->light_rec_host.data() + 7 * (size_t)e;
            const float area = pnglm::tri_area(pnglm::vec3(r[0].x, r[0].y, r[0].z), pnglm::vec3(r[2].x, r[2].y, r[2].z),
                                               pnglm::vec3(r[4].x, r[4].y, r[4].z));
            prefix = e ? area + prefix : area;
            lights[e] = make_float2((float)c->light_tri[e], prefix);
        }
        HIPCHK(c, hipMemcpy(const_cast<float2*>(s.lights), lights.data(), lights.size() * sizeof(float2), hipMemcpyHostToDevice));
        set_light_areas(s, lights, nl, nl ? prefix : 0.f);
    }
    return check_fault(c);
}

int pnrt_read_vertices(pnrt_ctx* c, int first, int count, float* out8) {
    if (!c) return PNRT_E_ARG;
    if (!c->has_scene) return set_err(c, PNRT_E_STATE, "read_vertices: upload_scene first");
    if (first < 0 || count < 0 || first > c->scene.n_verts - count)
        return set_err(c, PNRT_E_ARG, "read_vertices: vertex range outside the uploaded array");
    if (count > 0 && !out8) return set_err(c, PNRT_E_ARG, "read_vertices: out is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_all(c));
    if (count > 0) HIPCHK(c, hipMemcpy(out8, c->scene.verts + 2 * (size_t)first, (size_t)count * 32, hipMemcpyDeviceToHost));
    return check_fault(c);
}

int pnrt_read_bvh_boxes(pnrt_ctx* c, float* N, int nn) {
    if (!c) return PNRT_E_ARG;
    if (!c->has_scene) return set_err(c, PNRT_E_STATE, "read_bvh_boxes: upload_scene first");
    if (!N || nn <= 0) return set_err(c, PNRT_E_ARG, "read_bvh_boxes: no node array");
    // the upload's breadth-first numbering, recovered from the caller's pre-order array
    std::vector<int> order;
    if (fint(N[7]) != -1) order.push_back(0);
    for (size_t q = 0; q < order.size(); ++q) {
        const int i = order[q];
        const int rc = fint(N[12 * (size_t)i + 7]);
        if (order.size() > (size_t)c->n_interior)
            return set_err(c, PNRT_E_ARG, "read_bvh_boxes: the node array has more interior nodes than the uploaded tree's " +
                                              std::to_string(c->n_interior));
        if (i + 1 >= nn || rc <= 0 || rc >= nn)
            return set_err(c, PNRT_E_ARG, "read_bvh_boxes: the node array is not the uploaded tree");
        if (fint(N[12 * (size_t)(i + 1) + 7]) != -1) order.push_back(i + 1);
        if (fint(N[12 * (size_t)rc + 7]) != -1) order.push_back(rc);
    }
    if ((int)order.size() != c->n_interior)
        return set_err(c, PNRT_E_ARG, "read_bvh_boxes: the node array has " + std::to_string(order.size()) +
                                          " interior nodes, the uploaded tree " + std::to_string(c->n_interior));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_all(c));
    std::vector<float> dev(order.size() * 16);
    if (!dev.empty()) HIPCHK(c, hipMemcpy(dev.data(), c->scene.nodes, dev.size() * 4, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < order.size(); ++k) {
        const int ch[2] = {order[k] + 1, fint(N[12 * (size_t)order[k] + 7])};
        for (int side = 0; side < 2; ++side) {
            uint32_t ref;
            std::memcpy(&ref, &dev[16 * k + 12 + side], 4);
            if (((ref & REF_LEAF) != 0) != (fint(N[12 * (size_t)ch[side] + 7]) == -1))
                return set_err(c, PNRT_E_ARG, "read_bvh_boxes: node " + std::to_string(ch[side]) +
                                                  " is a leaf in one tree and interior in the other");
        }
    }
    for (size_t k = 0; k < order.size(); ++k) {
        const int ch[2] = {order[k] + 1, fint(N[12 * (size_t)order[k] + 7])};
        for (int side = 0; side < 2; ++side) std::memcpy(N + 12 * (size_t)ch[side], &dev[16 * k + 6 * side], 24);
    }
    for (int k = 0; k < 3; ++k) { N[k] = c->scene.root_min[k]; N[3 + k] = c->scene.root_max[k]; }
    return check_fault(c);
}

int pnrt_upload_texture(pnrt_ctx* c, int slot, const uint8_t* px, int w, int h, int ch) {
    if (!c) return PNRT_E_ARG;
    if (slot < 0 || slot >= PT_MAX_TEXTURES || !px || w <= 0 || h <= 0 || ch < 1 || ch > 4)
        return set_err(c, PNRT_E_ARG, "upload_texture: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    // glTexImage2D with the default GL_UNPACK_ALIGNMENT 4 (main.cpp:545): row j
    // starts at j * align4(w * ch) in the caller's tightly packed buffer; bytes
    // past the buffer read as 0.  GL_RED -> (r, 0, 0).
    size_t stride = ((size_t)w * ch + 3) & ~(size_t)3, avail = (size_t)w * h * ch;
    std::vector<uint32_t> texels((size_t)w * h);
    for (int j = 0; j < h; ++j)
        for (int i = 0; i < w; ++i) {
            uint32_t rgb[3] = {0, 0, 0};
            for (int k = 0; k < (ch >= 3 ? 3 : ch); ++k) {
                size_t o = (size_t)j * stride + (size_t)i * ch + k;
                rgb[k] = o < avail ? px[o] : 0;
            }
            texels[(size_t)j * w + i] = rgb[0] | (rgb[1] << 8) | (rgb[2] << 16);
        }
    HIPCHK(c, sync_all(c));             // pipelined calls may still sample the old texture
    HIPCHK(c, c->tex[slot].alloc(texels.size() * 4));
    HIPCHK(c, hipMemcpy(c->tex[slot], texels.data(), texels.size() * 4, hipMemcpyHostToDevice));
    c->tex_w[slot] = w; c->tex_h[slot] = h;
    ++c->tex_epoch;                      // the albedo guide image samples the textures
    return PNRT_OK;
}

// Footprint records (DevScene::hdr_q / rnd_q) of a w x h image: record (qj, qi)
// = texels (bottom, left), (bottom, right), (top, left), (top, right) with
// left = clamp(qi - 1), right = clamp(qi), bottom = clamp(qj - 1), top = clamp(qj).
__global__ void env_quad_kernel(const float4* img, int w, int h, float4* q) {
    const size_t n = (size_t)(w + 1) * (h + 1);
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int qj = (int)(r / (size_t)(w + 1)), qi = (int)(r - (size_t)qj * (w + 1));
    const int l = qi > 0 ? qi - 1 : 0, rt = qi < w ? qi : w - 1;
    const int bo = qj > 0 ? qj - 1 : 0, tp = qj < h ? qj : h - 1;
    q[4 * r] = img[(size_t)bo * w + l];
    q[4 * r + 1] = img[(size_t)bo * w + rt];
    q[4 * r + 2] = img[(size_t)tp * w + l];
    q[4 * r + 3] = img[(size_t)tp * w + rt];
}

static void free_env(pnrt_ctx* c) {
    c->hdr.reset(); c->rnd.reset(); c->hdr_q.reset(); c->rnd_q.reset();
}

// The two env uploads begin by dropping the old environment, once the calls in flight have
// rendered with it ...
static int env_begin(pnrt_ctx* c) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_all(c));
    free_env(c);
    c->scene.has_hdr = 0;
    set_emit_max(c);
    ++c->scene_epoch;                    // a primary miss records the env colour
    return PNRT_OK;
}
// ... allocate both w x h images and fill hdr with `rgb` ...
static int env_images(pnrt_ctx* c, const float* rgb, size_t n) {
    std::vector<float4> a(n);
    for (size_t i = 0; i < n; ++i) a[i] = make_float4(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], 0.f);
    HIPCHK(c, c->hdr.alloc(n * 16));
    HIPCHK(c, c->rnd.alloc(n * 16));
    HIPCHK(c, hipMemcpy(c->hdr, a.data(), n * 16, hipMemcpyHostToDevice));
    return PNRT_OK;
}
// ... and finish, with rnd filled too, by the footprint records of both and the scene's env fields.
static int env_finish(pnrt_ctx* c, const float* rgb, int w, int h) {
    const size_t n = (size_t)(w + 1) * (h + 1);
    HIPCHK(c, c->hdr_q.alloc(n * 64));
    HIPCHK(c, c->rnd_q.alloc(n * 64));
    const unsigned g = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(env_quad_kernel, dim3(g), dim3(256), 0, c->stream, (const float4*)c->hdr, w, h, (float4*)c->hdr_q);
    hipLaunchKernelGGL(env_quad_kernel, dim3(g), dim3(256), 0, c->stream, (const float4*)c->rnd, w, h, (float4*)c->rnd_q);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->scene.has_hdr = 1;
    c->scene.hdr_w = w; c->scene.hdr_h = h;
    c->env_max = abs_max(rgb, 3 * (size_t)w * h, 0.f);
    set_emit_max(c);
    return PNRT_OK;
}

int pnrt_upload_env(pnrt_ctx* c, const float* rgb, const float* rnd, int w, int h) {
    if (!c) return PNRT_E_ARG;
    if (int rc = env_begin(c)) return rc;
    if (!rgb) return PNRT_OK;
    if (!rnd || w <= 0 || h <= 0) return set_err(c, PNRT_E_ARG, "upload_env: bad arguments");
    const size_t n = (size_t)w * h;
    std::vector<float4> b(n);
    for (size_t i = 0; i < n; ++i) b[i] = make_float4(rnd[3 * i], rnd[3 * i + 1], rnd[3 * i + 2], 0.f);
    if (int rc = env_images(c, rgb, n)) return rc;
    HIPCHK(c, hipMemcpy(c->rnd, b.data(), n * 16, hipMemcpyHostToDevice));
    return env_finish(c, rgb, w, h);
}

int pnrt_upload_env_build(pnrt_ctx* c, const float* rgb, int w, int h) {
    if (!c) return PNRT_E_ARG;
    if (!rgb || w <= 0 || h <= 0) return set_err(c, PNRT_E_ARG, "upload_env_build: bad arguments");
    if (int rc = env_begin(c)) return rc;
    const size_t n = (size_t)w * h;
    if (int rc = env_images(c, rgb, n)) return rc;
    DevBuf<float> tmp;                        // lumY/pdfY | lumX | cdfY | marginX | cdfX | sum
    HIPCHK(c, tmp.alloc((3 * n + 2 * (size_t)w + 64) * 4));
    float *pdfY = tmp.p, *lumX = pdfY + n, *cdfY = pdfY + 2 * n, *marginX = pdfY + 3 * n, *cdfX = marginX + w,
          *sum = cdfX + w;
    const unsigned gp = (unsigned)((n + 255) / 256), gx = (unsigned)((w + 255) / 256);
    hipLaunchKernelGGL(env_lumen_kernel, dim3(gp), dim3(256), 0, c->stream, (const float4*)c->hdr, pdfY, lumX, w, h);
    hipLaunchKernelGGL(env_sum_kernel, dim3(1), dim3(64), 0, c->stream, (const float*)lumX, n, sum);
    hipLaunchKernelGGL(env_margin_kernel, dim3(gx), dim3(256), 0, c->stream, pdfY, (const float*)sum, marginX, w, h);
    hipLaunchKernelGGL(env_cdfx_kernel, dim3(1), dim3(64), 0, c->stream, (const float*)marginX, cdfX, w);
    hipLaunchKernelGGL(env_cdfy_kernel, dim3(gx), dim3(256), 0, c->stream, (const float*)pdfY, (const float*)marginX, cdfY, w, h);
    hipLaunchKernelGGL(env_table_kernel, dim3(gp), dim3(256), 0, c->stream, (const float*)cdfX, (const float*)cdfY,
                       (const float*)pdfY, c->rnd.p, w, h);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return set_err(c, PNRT_E_HIP, std::string("upload_env_build: ") + hipGetErrorString(e));
    return env_finish(c, rgb, w, h);
}

int pnrt_read_env_table(pnrt_ctx* c, float* out) {
    if (!c || !out) return PNRT_E_ARG;
    if (!c->rnd) return set_err(c, PNRT_E_STATE, "read_env_table: no environment");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_all(c));
    const size_t n = (size_t)c->scene.hdr_w * c->scene.hdr_h;
    std::vector<float4> t(n);
    HIPCHK(c, hipMemcpy(t.data(), c->rnd, n * 16, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) { out[3 * i] = t[i].x; out[3 * i + 1] = t[i].y; out[3 * i + 2] = t[i].z; }
    return PNRT_OK;
}

int pnrt_set_frame(pnrt_ctx* c, int w, int h, const pnrt_camera* cam, int depth) {
    if (!c) return PNRT_E_ARG;
    if (w <= 0 || h <= 0 || !cam || depth < 0 || depth > 4)
        return set_err(c, PNRT_E_ARG, "set_frame: bad arguments (MAX_BOUNCE_DEPTH must be 0..4: 8 Sobol dims)");
    HIPCHK(c, hipSetDevice(c->device));
    if (w != c->width || h != c->height || !c->accum) {
        HIPCHK(c, sync_all(c));
        HIPCHK(c, c->accum.alloc((size_t)w * h * 16));
        HIPCHK(c, hipMemsetAsync(c->accum, 0, (size_t)w * h * 16, c->stream));
        c->width = w; c->height = h;
        if (int rc = mark_stream(c)) return rc;
        if (c->moments_ever)
            if (int rc = moments_alloc(c)) return rc;
    }
    c->cam = *cam;
    c->max_bounce = depth;
    c->has_frame = true;
    return PNRT_OK;
}

int pnrt_render(pnrt_ctx* c, uint32_t first, uint32_t nf, int band, int nsh, int shard) {
    if (!c) return PNRT_E_ARG;
    if (int rc = need_scene_frame(c, "render")) return rc;
    if (int rc = check_selector(c, "render", band, nsh, shard)) return rc;
    if (int rc = check_frame_range(c, "render", first, nf)) return rc;
    // the one-kernel path keeps its frames in registers: no per-frame colours to take moments of
    if (c->kernel == 1 && c->moments_on)
        return set_err(c, PNRT_E_STATE, "render: PNRT_KERNEL_V1 cannot update the sample moments (pnrt_enable_moments(ctx, 0) first)");
    FrameParams fp;
    DevScene s;
    if (int rc = frame_call(c, first, nf, band, nsh, shard, &fp, &s)) return rc;
    if (nf == 0) return PNRT_OK;
    moments_uncover(c);                          // (here before the shard's rows are known, unlike the other entry points)
    if (fp.rows == 0) return PNRT_OK;
    if (WF_DIAG_BOUNDS) {                // the bounds check's own test (diagnostic builds only)
        const char* f = getenv("PNRT_DIAG_FORCE_OOB");
        s.diag_force = (f && atoi(f) > 0) ? 1 : 0;
    }
    if (c->kernel == 1) {
        dim3 grid((c->width + 15) / 16, (fp.rows + 15) / 16);
        {
            ProfScope ps(c, PNRT_K_V1);
            hipLaunchKernelGGL(pt_render_kernel, grid, dim3(256), 0, c->stream, s, fp, c->accum);
        }
        HIPCHK(c, hipGetLastError());
        return mark_stream(c);           // (every op queued on c->stream records ev_last)
    }
    return render_wavefront(c, s, fp, PathSource::records(), first, nf);
}

// A staging block for a call's cameras, moved to the back of the list: one whose last copy has
// completed (grown if too small), or a new one.
static int cam_stage_get(pnrt_ctx* c, size_t bytes) {
    size_t at = c->cam_stage.size();
    for (size_t i = 0; i < c->cam_stage.size() && at == c->cam_stage.size(); ++i) {
        pnrt_ctx::CamStage& S = c->cam_stage[i];
        if (!S.pending || hipEventQuery(S.ev) == hipSuccess) at = i;
    }
    if (at == c->cam_stage.size()) {
        hipEvent_t ev = nullptr;
        HIPCHK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        c->cam_stage.emplace_back();
        c->cam_stage.back().ev = ev;
    }
    std::swap(c->cam_stage[at], c->cam_stage.back());
    pnrt_ctx::CamStage& S = c->cam_stage.back();
    S.pending = false;
    if (S.host.cap < bytes) HIPCHK(c, S.host.alloc(std::max<size_t>(bytes, 4096)));
    return PNRT_OK;
}

int pnrt_render_cameras(pnrt_ctx* c, uint32_t first, uint32_t nf, const pnrt_camera* cameras, int band, int nsh, int shard) {
    if (!c) return PNRT_E_ARG;
    if (int rc = need_scene_frame(c, "render_cameras")) return rc;
    if (c->kernel == 1)
        return set_err(c, PNRT_E_STATE, "render_cameras: PNRT_KERNEL_V1 renders the pnrt_set_frame camera only");
    if (int rc = check_selector(c, "render_cameras", band, nsh, shard)) return rc;
    if (int rc = check_frame_range(c, "render_cameras", first, nf)) return rc;
    if (nf > 0 && !cameras) return set_err(c, PNRT_E_ARG, "render_cameras: cameras is NULL");
    static_assert(sizeof(pnrt_camera) == 48, "twelve floats per camera");
    const float* cf = reinterpret_cast<const float*>(cameras);
    for (uint64_t i = 0; i < 12ull * nf; ++i)
        if (!std::isfinite(cf[i]))
            return set_err(c, PNRT_E_ARG, "render_cameras: a camera component is not finite: frame " +
                                              std::to_string((uint64_t)first + i / 12) + " (cameras[" + std::to_string(i / 12) +
                                              "], float " + std::to_string(i % 12) + ")");
    FrameParams fp;
    DevScene s;
    if (int rc = frame_call(c, first, nf, band, nsh, shard, &fp, &s)) return rc;
    if (nf == 0 || fp.rows == 0) return PNRT_OK;
    moments_uncover(c);
    // the array is the caller's again when this returns: the batches read the copy
    if (int rc = cam_stage_get(c, (size_t)nf * 48)) return rc;
    std::memcpy(c->cam_stage.back().host, cf, (size_t)nf * 48);
    return render_wavefront(c, s, fp, PathSource::cameras(c->cam_stage.back().host), first, nf);
}

// pnrt_batch_plan / pnrt_cameras_batch_plan: the plan of a call of source `src`.
static int batch_plan(pnrt_ctx* c, const std::string& who, const PathSource& src, uint32_t nf, int band, int nsh, int shard,
                      uint32_t* frames_per_batch, uint32_t* n_batches, int64_t* bytes) {
    if (!c) return PNRT_E_ARG;
    if (!c->has_frame) return set_err(c, PNRT_E_STATE, who + ": set_frame first");
    if (int rc = check_selector(c, who.c_str(), band, nsh, shard)) return rc;
    uint32_t chunk = 0, nb = 0;
    int64_t by = 0;
    const int rows = shard_rows(c->height, band, nsh, shard);
    if (nf > 0 && rows > 0) {                    // (the render call queues nothing otherwise)
        const size_t per_frame = frame_paths(c->width, rows), pix = (size_t)rows * c->width;
        chunk = plan_chunk(c, per_frame, pix, nf, src.slot_bytes());
        if (chunk == 0) return set_err(c, PNRT_E_ARG, who + ": frame too large for one batch");
        nb = nf / chunk + (nf % chunk ? 1u : 0u);
        by = (int64_t)batch_bytes(per_frame, pix, chunk, src.slot_bytes());
    }
    if (frames_per_batch) *frames_per_batch = chunk;
    if (n_batches) *n_batches = nb;
    if (bytes) *bytes = by;
    return PNRT_OK;
}

int pnrt_cameras_batch_plan(pnrt_ctx* c, uint32_t nf, int band, int nsh, int shard, uint32_t* frames_per_batch,
                            uint32_t* n_batches, int64_t* bytes) {
    return batch_plan(c, "cameras_batch_plan", PathSource::cameras(nullptr), nf, band, nsh, shard, frames_per_batch, n_batches, bytes);
}

int pnrt_batch_plan(pnrt_ctx* c, uint32_t nf, int band, int nsh, int shard, uint32_t* frames_per_batch,
                    uint32_t* n_batches, int64_t* bytes) {
    return batch_plan(c, "batch_plan", PathSource::records(), nf, band, nsh, shard, frames_per_batch, n_batches, bytes);
}

int pnrt_reset_accum(pnrt_ctx* c) {
    if (!c) return PNRT_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    // a new accumulation: wait for the calls in flight first, so a fault of one of
    // them (whose contribution the reset erases) is read and cleared here, not
    // reported against the new accumulation later
    HIPCHK(c, sync_all(c));
    (void)check_fault(c);
    if (c->faulted) {
        for (int k = 0; k < WF_FAULT_WORDS; ++k) __atomic_store_n(c->fault_host + k, 0u, __ATOMIC_RELEASE);
        c->faulted = false;
        c->fault_msg.clear();
    }
    if (!c->accum) return PNRT_OK;
    HIPCHK(c, hipMemsetAsync(c->accum, 0, (size_t)c->width * c->height * 16, c->stream));
    if (c->moments) {
        HIPCHK(c, hipMemsetAsync(c->moments, 0, (size_t)c->width * c->height * 16, c->stream));
        c->mom_cover = true;         // zeroed together: the moments cover the accumulation again
    }
    return mark_stream(c);
}

int pnrt_read_accum(pnrt_ctx* c, float* out) {
    if (!c || !out) return PNRT_E_ARG;
    if (!c->accum) return set_err(c, PNRT_E_STATE, "read_accum: no frame");
    return read_back(c, out, c->accum, (size_t)c->width * c->height * 16);
}

void* pnrt_accum_device_ptr(pnrt_ctx* c) { return c ? c->accum.p : nullptr; }

int pnrt_render_guides(pnrt_ctx* c) {
    if (!c) return PNRT_E_ARG;
    if (int rc = need_scene_frame(c, "render_guides")) return rc;
    if (int rc = check_fault(c)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return render_guides(c, c->cam, nullptr);
}

// ---- caller ray buffers (pt_rays.h) -------------------------------------
// The buffer rules pnrt_render_rays, pnrt_render_guides_rays and pnrt_make_rays share, for a call over n sets
// (n == 0: no record is read or written, so NULL passes).
static_assert(PT_CAM_PINHOLE == PNRT_CAM_PINHOLE && PT_CAM_ORTHO == PNRT_CAM_ORTHO && PT_CAM_EQUIRECT == PNRT_CAM_EQUIRECT &&
                  PT_CAM_FISHEYE == PNRT_CAM_FISHEYE, "pt_rays.h's models are the header's");
static int check_ray_buffer(pnrt_ctx* c, const std::string& who, const void* rays, int64_t stride, uint32_t n = 1) {
    if (!rays && n > 0) return set_err(c, PNRT_E_ARG, who + ": the ray buffer is NULL");
    if ((uintptr_t)rays & 15u) return set_err(c, PNRT_E_ARG, who + ": the ray buffer must be 16-byte aligned");
    if (stride < 0 || (stride > 0 && stride < (int64_t)c->width * c->height))
        return set_err(c, PNRT_E_ARG, who + ": frame_stride must be 0 or >= width * height records");
    // the last set's end, in bytes, fits 63 bits: no record address wraps
    const int64_t pix = (int64_t)c->width * c->height, max_records = INT64_MAX / (int64_t)sizeof(pnrt_ray);
    if (n > 1 && stride > (max_records - pix) / (int64_t)(n - 1))
        return set_err(c, PNRT_E_ARG, who + ": (n - 1) * frame_stride + width * height records do not fit 63 bits of bytes");
    return PNRT_OK;
}

int pnrt_render_rays(pnrt_ctx* c, uint32_t first, uint32_t nf, const void* rays, int64_t stride, int band, int nsh, int shard) {
    if (!c) return PNRT_E_ARG;
    if (int rc = need_scene_frame(c, "render_rays")) return rc;
    if (c->kernel == 1) return set_err(c, PNRT_E_STATE, "render_rays: PNRT_KERNEL_V1 renders the pnrt_set_frame camera only");
    if (int rc = check_selector(c, "render_rays", band, nsh, shard)) return rc;
    if (int rc = check_frame_range(c, "render_rays", first, nf)) return rc;
    if (int rc = check_ray_buffer(c, "render_rays", rays, stride, nf)) return rc;
    FrameParams fp;
    DevScene s;
    if (int rc = frame_call(c, first, nf, band, nsh, shard, &fp, &s)) return rc;
    if (nf == 0 || fp.rows == 0) return PNRT_OK;
    moments_uncover(c);
    return render_wavefront(c, s, fp, PathSource::ray_sets(rays, stride), first, nf);
}

int pnrt_render_guides_rays(pnrt_ctx* c, const void* rays) {
    if (!c) return PNRT_E_ARG;
    if (int rc = need_scene_frame(c, "render_guides_rays")) return rc;
    if (int rc = check_ray_buffer(c, "render_guides_rays", rays, 0)) return rc;
    if (int rc = check_fault(c)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return render_guides(c, c->cam, rays);
}

// pnrt_make_rays' rules for its camera (`who`: the call, or the call and which of its views)
static int check_ray_camera(pnrt_ctx* c, const std::string& who, const pnrt_ray_camera* cam) {
    if (!cam) return set_err(c, PNRT_E_ARG, who + ": cam is NULL");
    if (cam->model < PNRT_CAM_PINHOLE || cam->model > PNRT_CAM_FISHEYE) return set_err(c, PNRT_E_ARG, who + ": unknown model");
    const float* cf = reinterpret_cast<const float*>(&cam->camera);
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(cf[i])) return set_err(c, PNRT_E_ARG, who + ": a camera component is not finite");
    if (!std::isfinite(cam->fov_deg) || !std::isfinite(cam->focus_distance))
        return set_err(c, PNRT_E_ARG, who + ": fov_deg or focus_distance is not finite");
    if (cam->model == PNRT_CAM_FISHEYE && !(cam->fov_deg > 0.0f && cam->fov_deg <= 360.0f))
        return set_err(c, PNRT_E_ARG, who + ": a fisheye's fov_deg must be in (0, 360]");
    if (!(std::isfinite(cam->aa_width) && cam->aa_width >= 0.0f) || !(std::isfinite(cam->lens_radius) && cam->lens_radius >= 0.0f))
        return set_err(c, PNRT_E_ARG, who + ": aa_width and lens_radius must be finite and >= 0");
    if (cam->lens_radius > 0.0f && cam->model != PNRT_CAM_PINHOLE)
        return set_err(c, PNRT_E_ARG, who + ": a lens needs PNRT_CAM_PINHOLE");
    if (cam->lens_radius > 0.0f && !(cam->focus_distance > 0.0f))
        return set_err(c, PNRT_E_ARG, who + ": a lens needs focus_distance > 0");
    if (cam->per_pixel != 0 && cam->per_pixel != 1) return set_err(c, PNRT_E_ARG, who + ": per_pixel must be 0 or 1");
    if (cam->reserved != 0) return set_err(c, PNRT_E_ARG, who + ": reserved must be 0");
    return PNRT_OK;
}

int pnrt_make_rays(pnrt_ctx* c, const pnrt_ray_camera* cam, uint32_t first, uint32_t n_sets, void* out, int64_t stride) {
    if (!c) return PNRT_E_ARG;
    static_assert(sizeof(pnrt_ray) == 32 && sizeof(pnrt_ray_camera) == 76, "the documented sizes");
    if (!c->has_frame) return set_err(c, PNRT_E_STATE, "make_rays: set_frame first");
    if (int rc = check_ray_camera(c, "make_rays", cam)) return rc;
    if (int rc = check_frame_range(c, "make_rays", first, n_sets)) return rc;
    if (int rc = check_ray_buffer(c, "make_rays", out, stride, n_sets)) return rc;
    const size_t pix = (size_t)c->width * c->height;
    if (pix > 0x7FFFFFFFull) return set_err(c, PNRT_E_ARG, "make_rays: frame too large");
    if (n_sets == 0) return PNRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    MakeRays m;
    cam_floats(m.eye, m.llc, m.hor, m.ver, cam->camera);
    m.model = cam->model; m.fov_deg = cam->fov_deg;
    m.aa_width = cam->aa_width; m.lens_radius = cam->lens_radius; m.focus_distance = cam->focus_distance;
    m.per_pixel = cam->per_pixel;
    m.width = c->width; m.height = c->height;
    m.first_frame = first;
    m.n_sets = stride == 0 ? 1u : n_sets;        // (sets 0 records apart are one set: first_frame's)
    m.frame_stride = stride;
    const size_t total = pix * m.n_sets;
    if ((total + 255) / 256 > 0x7FFFFFFFull) return set_err(c, PNRT_E_ARG, "make_rays: too many records for one call");
    {
        ProfScope ps(c, PNRT_K_BLEND);
        hipLaunchKernelGGL(pt_make_rays_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, m,
                           static_cast<float4*>(out));
    }
    HIPCHK(c, hipGetLastError());
    return mark_stream(c);
}

int pnrt_read_aov(pnrt_ctx* c, int which, float* out) {
    if (!c || !out) return PNRT_E_ARG;
    if (which < 0 || which >= PNRT_AOV_COUNT) return set_err(c, PNRT_E_ARG, "read_aov: unknown guide image");
    if (!c->guide_key.valid || !c->aov[which]) return set_err(c, PNRT_E_STATE, "read_aov: render_guides first");
    if (c->guide_key.width != c->width || c->guide_key.height != c->height)
        return set_err(c, PNRT_E_STATE, "read_aov: the guide images have another size than the frame: render_guides again");
    return read_back(c, out, c->aov[which], (size_t)c->guide_key.width * c->guide_key.height * 16);
}

void* pnrt_aov_device_ptr(pnrt_ctx* c, int which) {
    return (c && which >= 0 && which < PNRT_AOV_COUNT) ? c->aov[which].p : nullptr;
}

int pnrt_query_rays_device(pnrt_ctx* c, const void* rays, int64_t n, int kind, void* out) {
    bool go;
    if (int rc = query_check(c, rays, n, kind, out, &go)) return rc;
    if (!go) return PNRT_OK;
    if (((uintptr_t)rays & 3u) || ((uintptr_t)out & 15u))
        return set_err(c, PNRT_E_ARG, "query_rays_device: rays must be 4-byte aligned, records 16-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    return query_launch(c, static_cast<const float*>(rays), n, kind, static_cast<uint4*>(out));
}

int pnrt_query_rays(pnrt_ctx* c, const float* rays, int64_t n, int kind, pnrt_hit* out) {
    bool go;
    if (int rc = query_check(c, rays, n, kind, out, &go)) return rc;
    if (!go) return PNRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t stage = std::min<int64_t>(n, QUERY_MAX_STAGE);
    int rc;
    if ((rc = c->q_rays.reserve(c, (size_t)stage * 28)) || (rc = c->q_out.reserve(c, (size_t)stage * 64))) return rc;
    for (int64_t at = 0; at < n; at += stage) {
        const int64_t m = std::min<int64_t>(n - at, stage);
        HIPCHK(c, hipMemcpyAsync(c->q_rays, rays + 7 * at, (size_t)m * 28, hipMemcpyHostToDevice, c->stream));
        if ((rc = query_launch(c, c->q_rays, m, kind, c->q_out))) return rc;
        HIPCHK(c, hipMemcpyAsync(out + at, c->q_out, (size_t)m * 64, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, sync_all(c));
    return check_fault(c);
}

int pnrt_denoise(pnrt_ctx* c, const pnrt_denoise_params* params) {
    if (!c) return PNRT_E_ARG;
    pnrt_denoise_params p = {5, 2.0f, 0.25f, 0.5f};      // the defaults (pnrt.h)
    if (params) p = *params;
    if (p.levels < 1 || p.levels > 5) return set_err(c, PNRT_E_ARG, "denoise: levels must be 1..5");
    for (float sg : {p.sigma_color, p.sigma_normal, p.sigma_position})
        if (!std::isfinite(sg) || !(sg > 0.0f)) return set_err(c, PNRT_E_ARG, "denoise: every sigma must be finite and > 0");
    if (!c->has_scene || !c->has_frame || !c->accum) return set_err(c, PNRT_E_STATE, "denoise: upload_scene and set_frame first");
    if (!c->guide_key.valid) return set_err(c, PNRT_E_STATE, "denoise: render_guides first");
    if (!guide_key_eq(c->guide_key, guide_key_now(c)))
        return set_err(c, PNRT_E_STATE, "denoise: the guide images are stale (camera, size, scene, materials, textures, "
                                        "environment or traversal mode changed): render_guides again");
    if (int rc = check_fault(c)) return rc;      // completed work that faulted
    HIPCHK(c, hipSetDevice(c->device));
    return denoise_run<false>(c, p.levels, p.sigma_color, p.sigma_normal, p.sigma_position);
}

int pnrt_denoise_variance(pnrt_ctx* c, const pnrt_denoise_variance_params* params) {
    if (!c) return PNRT_E_ARG;
    pnrt_denoise_variance_params p = {5, 4.0f, 0.25f, 0.5f};      // the defaults (pnrt.h)
    if (params) p = *params;
    if (p.levels < 1 || p.levels > 5) return set_err(c, PNRT_E_ARG, "denoise_variance: levels must be 1..5");
    for (float sg : {p.sigma_variance, p.sigma_normal, p.sigma_position})
        if (!std::isfinite(sg) || !(sg > 0.0f))
            return set_err(c, PNRT_E_ARG, "denoise_variance: every sigma must be finite and > 0");
    if (!c->has_scene || !c->has_frame || !c->accum)
        return set_err(c, PNRT_E_STATE, "denoise_variance: upload_scene and set_frame first");
    if (!c->moments_ever || !c->moments)
        return set_err(c, PNRT_E_STATE, "denoise_variance: the sample moments were never enabled (pnrt_enable_moments(ctx, 1) "
                                        "before the frames are rendered)");
    if (!c->mom_cover)
        return set_err(c, PNRT_E_STATE, "denoise_variance: frames were rendered while the moments were disabled, so they do not "
                                        "cover the accumulation (pnrt_reset_accum first)");
    if (!c->guide_key.valid) return set_err(c, PNRT_E_STATE, "denoise_variance: render_guides first");
    if (!guide_key_eq(c->guide_key, guide_key_now(c)))
        return set_err(c, PNRT_E_STATE, "denoise_variance: the guide images are stale (camera, size, scene, materials, textures, "
                                        "environment or traversal mode changed): render_guides again");
    if (int rc = check_fault(c)) return rc;      // completed work that faulted
    HIPCHK(c, hipSetDevice(c->device));
    return denoise_run<true>(c, p.levels, p.sigma_variance, p.sigma_normal, p.sigma_position);
}

int pnrt_read_denoised(pnrt_ctx* c, float* out) {
    if (!c || !out) return PNRT_E_ARG;
    if (!c->dn_width || !c->dn_img[0]) return set_err(c, PNRT_E_STATE, "read_denoised: denoise first");
    if (c->dn_width != c->width || c->dn_height != c->height)
        return set_err(c, PNRT_E_STATE, "read_denoised: the denoised image has another size than the frame: denoise again");
    return read_back(c, out, c->dn_img[0], (size_t)c->width * c->height * 16);
}

void* pnrt_denoised_device_ptr(pnrt_ctx* c) { return c ? c->dn_img[0].p : nullptr; }

int pnrt_enable_moments(pnrt_ctx* c, int on) {
    if (!c) return PNRT_E_ARG;
    if (on != 0 && on != 1) return set_err(c, PNRT_E_ARG, "enable_moments: on must be 0 or 1");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_all(c));                      // the calls in flight blend as they were issued
    if (on && !c->moments && c->accum)           // (before pnrt_set_frame: allocated with the frame)
        if (int rc = moments_alloc(c)) return rc;
    if (on) c->moments_ever = true;
    c->moments_on = on != 0;
    return PNRT_OK;
}

void* pnrt_moments_device_ptr(pnrt_ctx* c) { return c ? c->moments.p : nullptr; }

int pnrt_read_moments(pnrt_ctx* c, float* out) {
    if (!c || !out) return PNRT_E_ARG;
    if (int rc = need_moments_image(c, "read_moments")) return rc;
    return read_back(c, out, c->moments, (size_t)c->width * c->height * 16);
}

int pnrt_read_error(pnrt_ctx* c, float* out) {
    if (!c || !out) return PNRT_E_ARG;
    if (int rc = need_moments_image(c, "read_error")) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t pix = (size_t)c->width * c->height;
    if (pix > 0xFFFFFFFFull) return set_err(c, PNRT_E_ARG, "read_error: frame too large");
    if (int rc = c->mom_err.reserve(c, pix * 4)) return rc;
    hipLaunchKernelGGL(pt_moments_error_kernel, dim3((unsigned)((pix + 255) / 256)), dim3(256), 0, c->stream,
                       (const float4*)c->moments, c->mom_err, (uint32_t)pix);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, c->mom_err, pix * 4, hipMemcpyDeviceToHost, c->stream));
    if (int rc = mark_stream(c)) return rc;
    HIPCHK(c, sync_all(c));
    return check_fault(c);
}

int pnrt_convergence(pnrt_ctx* c, float threshold, int band, int nsh, int shard, pnrt_convergence_stats* out) {
    if (!c || !out) return PNRT_E_ARG;
    if (!std::isfinite(threshold) || !(threshold >= 0.0f))
        return set_err(c, PNRT_E_ARG, "convergence: threshold must be finite and >= 0");
    if (int rc = check_selector(c, "convergence", band, nsh, shard)) return rc;
    if (int rc = need_moments_image(c, "convergence")) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    std::memset(out, 0, sizeof *out);
    const int rows = shard_rows(c->height, band, nsh, shard);
    const size_t total = (size_t)rows * c->width;
    MomentsStats st{};
    if (total) {
        // the identities of the record's atomics (static: the copy may read it after this call returns)
        static const MomentsStats kIdentity = {0, 0, 0, 0, 0u, 0xFFFFFFFFu, 0u, 0u};
        if (int rc = c->mom_stats.reserve(c, sizeof(MomentsStats))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->mom_stats, &kIdentity, sizeof kIdentity, hipMemcpyHostToDevice, c->stream));
        const unsigned grid = (unsigned)std::min<size_t>((total + MOMENTS_REDUCE_BLOCK - 1) / MOMENTS_REDUCE_BLOCK, 2048);
        hipLaunchKernelGGL(pt_moments_reduce_kernel, dim3(grid), dim3(MOMENTS_REDUCE_BLOCK), 0, c->stream,
                           (const float4*)c->moments, c->mom_stats, c->width, rows, band, nsh, shard, threshold);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&st, c->mom_stats, sizeof st, hipMemcpyDeviceToHost, c->stream));
        if (int rc = mark_stream(c)) return rc;
    }
    HIPCHK(c, sync_all(c));
    if (total) {
        out->n_pixels = (int64_t)st.n_pixels;
        out->n_measured = (int64_t)st.n_measured;
        out->n_above = (int64_t)st.n_above;
        out->sum_q16 = (int64_t)st.sum_q16;
        std::memcpy(&out->max_error, &st.max_error_bits, 4);
        out->min_frames = st.min_frames;
        out->max_frames = st.max_frames;
    }
    return check_fault(c);
}

// pnrt_render_adaptive (rays: false -- the pnrt_set_frame camera) and pnrt_render_rays_adaptive (the caller's sets,
// pnrt_render_rays' buffer rules) as `who`.
static int adaptive_call(pnrt_ctx* c, const char* who, uint32_t first, uint32_t nf, float threshold, uint32_t min_frames, int band,
                         int nsh, int shard, pnrt_adaptive_stats* out, bool rays = false, const void* ray_buf = nullptr,
                         int64_t ray_stride = 0) {
    if (!c) return PNRT_E_ARG;
    if (int rc = need_scene_frame(c, who)) return rc;
    if (!std::isfinite(threshold) || !(threshold >= 0.0f))
        return set_err(c, PNRT_E_ARG, std::string(who) + ": threshold must be finite and >= 0");
    if (int rc = check_selector(c, who, band, nsh, shard)) return rc;
    if (int rc = check_frame_range(c, who, first, nf)) return rc;
    if (rays)
        if (int rc = check_ray_buffer(c, who, ray_buf, ray_stride, nf)) return rc;
    if (int rc = need_moments(c, who)) return rc;
    if (c->kernel == 1) return set_err(c, PNRT_E_STATE, std::string(who) + ": PNRT_KERNEL_V1 has no per-frame colours");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_all(c));                      // the predicate reads the moments as every earlier call left them
    FrameParams fp;
    DevScene s;
    if (int rc = frame_call(c, first, nf, band, nsh, shard, &fp, &s)) return rc;
    pnrt_adaptive_stats st{};
    const int tiles_x = (c->width + 7) / 8;
    const size_t n_tiles = (size_t)tiles_x * (size_t)((fp.rows + 7) / 8);
    st.n_pixels = (int64_t)fp.rows * c->width;
    st.n_tiles = (int64_t)n_tiles;
    WfAdapt ad{};
    if (n_tiles) {
        if (n_tiles > 0x7FFFFFFFull) return set_err(c, PNRT_E_ARG, std::string(who) + ": frame too large");
        int rc;
        if ((rc = c->ad_masks.reserve(c, n_tiles * 8)) || (rc = c->ad_flags.reserve(c, n_tiles * 4)) ||
            (rc = c->ad_offs.reserve(c, n_tiles * 4)) || (rc = c->ad_list.reserve(c, n_tiles * sizeof(WfTile))) ||
            (rc = c->ad_counts.reserve(c, sizeof(AdaptCounts))))
            return rc;
        // mask -> scan -> scatter, then the call's one synchronisation: the two counts
        const uint32_t m = min_frames > 2u ? min_frames : 2u;
        AdaptCounts cnt{};
        HIPCHK(c, hipMemsetAsync(c->ad_counts, 0, sizeof(AdaptCounts), c->stream));
        hipLaunchKernelGGL(pt_adaptive_mask_kernel, dim3((unsigned)((n_tiles + ADAPT_MASK_BLOCK / 64 - 1) / (ADAPT_MASK_BLOCK / 64))),
                           dim3(ADAPT_MASK_BLOCK), 0, c->stream, (const float4*)c->moments, c->width, fp.rows, band, nsh, shard,
                           tiles_x, (uint32_t)n_tiles, threshold, m, c->ad_masks, c->ad_flags);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(bvh_scan_kernel, dim3(1), dim3(1024), 0, c->stream, (const int*)c->ad_flags, c->ad_offs, (int)n_tiles);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(pt_adaptive_scatter_kernel, dim3((unsigned)((n_tiles + 255) / 256)), dim3(256), 0, c->stream,
                           (const unsigned long long*)c->ad_masks, (const int*)c->ad_flags, (const int*)c->ad_offs,
                           (uint32_t)n_tiles, c->ad_list, c->ad_counts);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&cnt, c->ad_counts, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
        if (int rc2 = mark_stream(c)) return rc2;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if ((size_t)cnt.n_active_tiles > n_tiles)
            return set_err(c, PNRT_E_HIP, std::string(who) + ": the active-tile count is out of range");
        st.n_active_pixels = (int64_t)cnt.n_active_pixels;
        st.n_active_tiles = (int64_t)cnt.n_active_tiles;
        ad.tiles = c->ad_list;
        ad.n_tiles = cnt.n_active_tiles;
    }
    const PathSource src = rays ? PathSource::ray_sets(ray_buf, ray_stride, &ad) : PathSource::records(&ad);
    uint32_t chunk = 0;
    if (nf > 0 && ad.n_tiles > 0) {
        // the plan runs on the active tiles' slots: the colours are compact, 16 bytes per slot (a ray call's slots
        // hold their camera-ray records besides)
        const size_t per_frame = (size_t)ad.n_tiles * 64;
        chunk = plan_chunk(c, per_frame, per_frame, nf, src.slot_bytes());
        if (chunk == 0) return set_err(c, PNRT_E_ARG, std::string(who) + ": frame too large for one batch");
        st.frames_per_batch = chunk;
        st.n_batches = nf / chunk + (nf % chunk ? 1u : 0u);
    }
    if (out) *out = st;
    if (chunk == 0) return PNRT_OK;              // nothing to render: nothing queued
    return render_adaptive(c, s, fp, src, chunk, first, nf);
}

int pnrt_render_adaptive(pnrt_ctx* c, uint32_t first, uint32_t nf, float threshold, uint32_t min_frames, int band, int nsh,
                         int shard, pnrt_adaptive_stats* out) {
    return adaptive_call(c, "render_adaptive", first, nf, threshold, min_frames, band, nsh, shard, out);
}

int pnrt_render_rays_adaptive(pnrt_ctx* c, uint32_t first, uint32_t nf, const void* rays, int64_t stride, float threshold,
                              uint32_t min_frames, int band, int nsh, int shard, pnrt_adaptive_stats* out) {
    return adaptive_call(c, "render_rays_adaptive", first, nf, threshold, min_frames, band, nsh, shard, out, true, rays, stride);
}

// ---- temporal reprojection (pt_reproject.h, pt_reproject_view.h; DESIGN.md sections 25 and 31) ------------
// The state rules, then the parameter rules, that pnrt_reproject and pnrt_reproject_view share; *p: the
// parameters in force.
static int reproject_check_state(pnrt_ctx* c, const char* who) {
    if (int rc = need_scene_frame(c, who)) return rc;
    if (int rc = need_moments(c, who)) return rc;
    if (c->kernel == 1) return set_err(c, PNRT_E_STATE, std::string(who) + ": PNRT_KERNEL_V1 keeps no sample moments");
    return PNRT_OK;
}
static int reproject_check_params(pnrt_ctx* c, const char* who, const pnrt_reproject_params* params, pnrt_reproject_params* p) {
    const std::string w(who);
    *p = {0.9f, 0.02f, 32u, 0u};                 // the defaults (pnrt.h)
    if (params) *p = *params;
    if (!std::isfinite(p->normal_min) || p->normal_min < -1.0f || p->normal_min > 1.0f)
        return set_err(c, PNRT_E_ARG, w + ": normal_min must be in [-1, 1]");
    if (!std::isfinite(p->position_tolerance) || !(p->position_tolerance > 0.0f))
        return set_err(c, PNRT_E_ARG, w + ": position_tolerance must be finite and > 0");
    if (p->max_history == 0u) return set_err(c, PNRT_E_ARG, w + ": max_history must be >= 1");
    if (p->reserved != 0u) return set_err(c, PNRT_E_ARG, w + ": reserved must be 0");
    if ((size_t)c->width * c->height > 0xFFFFFFFFull / 64) return set_err(c, PNRT_E_ARG, w + ": frame too large");     // (render_guides' limit)
    return PNRT_OK;
}

// Waits for the calls in flight (the images as every earlier call left them) and reserves the call's buffers.
static int reproject_begin(pnrt_ctx* c) {
    const size_t pix = (size_t)c->width * c->height;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_all(c));
    int rc;
    if ((rc = check_fault(c))) return rc;
    if ((rc = c->rp_pos.reserve(c, pix * 16)) || (rc = c->rp_nrm.reserve(c, pix * 16)) ||
        (rc = c->rp_acc.reserve(c, pix * 16)) || (rc = c->rp_mom.reserve(c, pix * 16)) ||
        (rc = c->rp_counts.reserve(c, REPROJECT_SLOTS * sizeof(ReprojectCounts))))
        return rc;
    return PNRT_OK;
}

// The current guide images become the history (rp_pos / rp_nrm): view A's.
static int reproject_keep_history(pnrt_ctx* c) {
    const size_t pix = (size_t)c->width * c->height;
    ProfScope ps(c, PNRT_K_BLEND);
    HIPCHK(c, hipMemcpyAsync(c->rp_pos, c->aov[PNRT_AOV_POSITION], pix * 16, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->rp_nrm, c->aov[PNRT_AOV_NORMAL], pix * 16, hipMemcpyDeviceToDevice, c->stream));
    return PNRT_OK;
}

// The kernel of view A's model over the history and the current guide images (view B's), the copies back and
// the counts.  cam: view A's camera; fov_deg: a fisheye's.
static int reproject_run(pnrt_ctx* c, const pnrt_reproject_params& p, int model, const pnrt_camera& cam, float fov_deg,
                         pnrt_reproject_stats* out) {
    const size_t pix = (size_t)c->width * c->height;
    int rc;
    ReprojectArgs ra;
    cam_floats(ra.eye, ra.llc, ra.hor, ra.ver, cam);
    ra.normal_min = p.normal_min; ra.position_tolerance = p.position_tolerance; ra.max_history = p.max_history;
    ra.width = c->width; ra.height = c->height;
    ra.tiles_x = (c->width + 7) / 8;
    ra.n_tiles = (uint32_t)((size_t)ra.tiles_x * (size_t)((c->height + 7) / 8));      // <= pix: fits
    std::vector<ReprojectCounts> slots(REPROJECT_SLOTS);
    HIPCHK(c, hipMemsetAsync(c->rp_counts, 0, REPROJECT_SLOTS * sizeof(ReprojectCounts), c->stream));
    {
        ProfScope ps(c, PNRT_K_BLEND);
        const dim3 grid(std::min<uint32_t>(ra.n_tiles, REPROJECT_MAX_GRID)), block(REPROJECT_BLOCK);
        const float4 *acc = c->accum, *mom = c->moments, *pos_a = c->rp_pos, *nrm_a = c->rp_nrm;
        const float4 *pos_b = c->aov[PNRT_AOV_POSITION], *nrm_b = c->aov[PNRT_AOV_NORMAL];
        switch (model) {
        case PNRT_CAM_ORTHO:
            hipLaunchKernelGGL(pt_reproject_view_kernel<PT_CAM_ORTHO>, grid, block, 0, c->stream, ra, fov_deg, acc, mom, pos_a, nrm_a,
                               pos_b, nrm_b, c->rp_acc.p, c->rp_mom.p, c->rp_counts.p);
            break;
        case PNRT_CAM_EQUIRECT:
            hipLaunchKernelGGL(pt_reproject_view_kernel<PT_CAM_EQUIRECT>, grid, block, 0, c->stream, ra, fov_deg, acc, mom, pos_a,
                               nrm_a, pos_b, nrm_b, c->rp_acc.p, c->rp_mom.p, c->rp_counts.p);
            break;
        case PNRT_CAM_FISHEYE:
            hipLaunchKernelGGL(pt_reproject_view_kernel<PT_CAM_FISHEYE>, grid, block, 0, c->stream, ra, fov_deg, acc, mom, pos_a,
                               nrm_a, pos_b, nrm_b, c->rp_acc.p, c->rp_mom.p, c->rp_counts.p);
            break;
        default:
            hipLaunchKernelGGL(pt_reproject_kernel, grid, block, 0, c->stream, ra, acc, mom, pos_a, nrm_a, pos_b, nrm_b, c->rp_acc.p,
                               c->rp_mom.p, c->rp_counts.p);
        }
    }
    HIPCHK(c, hipGetLastError());
    {
        ProfScope ps(c, PNRT_K_BLEND);
        HIPCHK(c, hipMemcpyAsync(c->accum, c->rp_acc, pix * 16, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->moments, c->rp_mom, pix * 16, hipMemcpyDeviceToDevice, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(slots.data(), c->rp_counts, REPROJECT_SLOTS * sizeof(ReprojectCounts), hipMemcpyDeviceToHost,
                             c->stream));
    if ((rc = mark_stream(c))) return rc;
    HIPCHK(c, sync_all(c));
    ReprojectCounts cnt{};                       // integers: the same whatever order the blocks arrived in
    for (const ReprojectCounts& s : slots) {
        cnt.n_reprojected += s.n_reprojected; cnt.n_disoccluded += s.n_disoccluded; cnt.n_missed += s.n_missed;
        cnt.sum_frames += s.sum_frames;
        cnt.max_frames = std::max(cnt.max_frames, s.max_frames);
    }
    if (out) {
        std::memset(out, 0, sizeof *out);
        out->n_pixels = (int64_t)pix;
        out->n_reprojected = (int64_t)cnt.n_reprojected;
        out->n_disoccluded = (int64_t)cnt.n_disoccluded;
        out->n_missed = (int64_t)cnt.n_missed;
        out->sum_frames = (int64_t)cnt.sum_frames;
        out->max_frames = cnt.max_frames;
    }
    return check_fault(c);
}

int pnrt_reproject(pnrt_ctx* c, const pnrt_camera* from, const pnrt_reproject_params* params, pnrt_reproject_stats* out) {
    if (!c) return PNRT_E_ARG;
    pnrt_reproject_params p;
    if (int rc = reproject_check_state(c, "reproject")) return rc;
    if (!from) return set_err(c, PNRT_E_ARG, "reproject: the camera the accumulation was rendered with is NULL");
    for (const float* v : {from->eye, from->lower_left, from->horizontal, from->vertical})
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(v[k])) return set_err(c, PNRT_E_ARG, "reproject: a camera float is not finite");
    if (int rc = reproject_check_params(c, "reproject", params, &p)) return rc;
    int rc;
    if ((rc = reproject_begin(c))) return rc;
    // the guide images of `from` (the current ones when they were rendered for it), kept as the history
    if (!guide_key_eq(c->guide_key, guide_key_for(c, *from), /* camera_keyed */ true))
        if ((rc = render_guides(c, *from, nullptr))) return rc;
    if ((rc = reproject_keep_history(c))) return rc;
    if ((rc = render_guides(c, c->cam, nullptr))) return rc;
    return reproject_run(c, p, PNRT_CAM_PINHOLE, *from, 0.0f, out);
}

// The centre rays of `view` (aa_width 0, no lens: no sample, so any frame's) into the context's ray buffer, and
// their guide images.
static int reproject_view_guides(pnrt_ctx* c, const pnrt_ray_camera& view) {
    const size_t pix = (size_t)c->width * c->height;
    MakeRays m{};
    cam_floats(m.eye, m.llc, m.hor, m.ver, view.camera);
    m.model = view.model; m.fov_deg = view.fov_deg;
    m.width = c->width; m.height = c->height;
    m.n_sets = 1;
    {
        ProfScope ps(c, PNRT_K_BLEND);
        hipLaunchKernelGGL(pt_make_rays_kernel, dim3((unsigned)((pix + 255) / 256)), dim3(256), 0, c->stream, m, c->rp_rays.p);
    }
    HIPCHK(c, hipGetLastError());
    return render_guides(c, c->cam, c->rp_rays.p);
}

int pnrt_reproject_view(pnrt_ctx* c, const pnrt_ray_camera* from, const pnrt_ray_camera* to, const pnrt_reproject_params* params,
                        pnrt_reproject_stats* out) {
    if (!c) return PNRT_E_ARG;
    pnrt_reproject_params p;
    if (int rc = reproject_check_state(c, "reproject_view")) return rc;
    if (int rc = reproject_check_params(c, "reproject_view", params, &p)) return rc;
    if (!from) return set_err(c, PNRT_E_ARG, "reproject_view: from (the view the accumulation was rendered with) is NULL");
    if (!to) return set_err(c, PNRT_E_ARG, "reproject_view: to (the view to continue in) is NULL");
    if (int rc = check_ray_camera(c, "reproject_view: from", from)) return rc;
    if (int rc = check_ray_camera(c, "reproject_view: to", to)) return rc;
    int rc;
    if ((rc = reproject_begin(c))) return rc;
    if ((rc = c->rp_rays.reserve(c, (size_t)c->width * c->height * 32))) return rc;
    // Ray-made guide images carry no camera: the current ones cannot be known to be `from`'s, so both views' are rendered
    if ((rc = reproject_view_guides(c, *from))) return rc;
    if ((rc = reproject_keep_history(c))) return rc;
    if ((rc = reproject_view_guides(c, *to))) return rc;
    return reproject_run(c, p, from->model, from->camera, from->fov_deg, out);
}

// The image a display source names, or NULL with the error set (`what` names the caller).
static const float4* display_source(pnrt_ctx* c, const char* what, int source, const void* src_device, int* rc) {
    *rc = PNRT_OK;
    const std::string w(what);
    if (source != PNRT_DISPLAY_ACCUM && source != PNRT_DISPLAY_DENOISED && source != PNRT_DISPLAY_EXTERNAL) {
        *rc = set_err(c, PNRT_E_ARG, w + ": unknown source");
        return nullptr;
    }
    if (source == PNRT_DISPLAY_EXTERNAL && (!src_device || ((uintptr_t)src_device & 15u))) {
        *rc = set_err(c, PNRT_E_ARG, w + ": PNRT_DISPLAY_EXTERNAL needs a 16-byte aligned src_device");
        return nullptr;
    }
    if (!c->has_frame || !c->accum) {
        *rc = set_err(c, PNRT_E_STATE, w + ": set_frame first");
        return nullptr;
    }
    if ((size_t)c->width * c->height > 0x7FFFFFFFull) {
        *rc = set_err(c, PNRT_E_ARG, w + ": frame too large");
        return nullptr;
    }
    if (source == PNRT_DISPLAY_DENOISED) {
        if (!c->dn_img[0] || c->dn_width != c->width || c->dn_height != c->height) {
            *rc = set_err(c, PNRT_E_STATE, w + ": no denoised image of this frame size (pnrt_denoise or pnrt_denoise_variance first)");
            return nullptr;
        }
        return c->dn_img[0];
    }
    return source == PNRT_DISPLAY_EXTERNAL ? static_cast<const float4*>(src_device) : c->accum.p;
}

int pnrt_display(pnrt_ctx* c, const pnrt_display_params* params) {
    if (!c) return PNRT_E_ARG;
    pnrt_display_params p = {PNRT_DISPLAY_ACCUM, PNRT_TONE_CLAMP, PNRT_TRANSFER_LINEAR, 0, 1.0f, 4.0f, nullptr};   // the defaults (pnrt.h)
    if (params) p = *params;
    if (p.tone != PNRT_TONE_CLAMP && p.tone != PNRT_TONE_REINHARD && p.tone != PNRT_TONE_ACES)
        return set_err(c, PNRT_E_ARG, "display: unknown tone curve");
    if (p.transfer != PNRT_TRANSFER_LINEAR && p.transfer != PNRT_TRANSFER_SRGB)
        return set_err(c, PNRT_E_ARG, "display: unknown transfer");
    if (p.bottom_first != 0 && p.bottom_first != 1) return set_err(c, PNRT_E_ARG, "display: bottom_first must be 0 or 1");
    for (float v : {p.exposure, p.white})
        if (!std::isfinite(v) || !(v > 0.0f)) return set_err(c, PNRT_E_ARG, "display: exposure and white must be finite and > 0");
    int rc;
    const float4* src = display_source(c, "display", p.source, p.src_device, &rc);
    if (!src) return rc;
    if ((rc = check_fault(c))) return rc;        // completed work that faulted
    HIPCHK(c, hipSetDevice(c->device));
    const uint32_t npix = (uint32_t)((size_t)c->width * c->height);
    if (!c->disp || c->disp_width != c->width || c->disp_height != c->height) {
        // the new image before the old one is freed: its pointer differs, and a failure leaves the old one
        DevBuf<uint32_t> img;
        HIPCHK(c, img.alloc((size_t)npix * 4));
        if (c->disp) (void)sync_all(c);
        c->disp = std::move(img);
        c->disp_width = c->width; c->disp_height = c->height;
    }
    const float w2 = p.white * p.white;
    const unsigned grid = (npix + DISPLAY_BLOCK * DISPLAY_PIXELS_PER_LANE - 1) / (DISPLAY_BLOCK * DISPLAY_PIXELS_PER_LANE);
    // the source's writers (blends, filters) were queued on this stream before, its next writers come after
    auto launch = [&](auto kernel) {
        ProfScope ps(c, PNRT_K_BLEND);
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(DISPLAY_BLOCK), 0, c->stream, src, c->disp, (uint32_t)c->width,
                           (uint32_t)c->height, npix, p.bottom_first, p.exposure, w2);
    };
    const bool srgb = p.transfer == PNRT_TRANSFER_SRGB;
    if (p.tone == PNRT_TONE_CLAMP) srgb ? launch(pt_display_kernel<DISPLAY_TONE_CLAMP, DISPLAY_TRANSFER_SRGB>)
                                        : launch(pt_display_kernel<DISPLAY_TONE_CLAMP, DISPLAY_TRANSFER_LINEAR>);
    else if (p.tone == PNRT_TONE_REINHARD) srgb ? launch(pt_display_kernel<DISPLAY_TONE_REINHARD, DISPLAY_TRANSFER_SRGB>)
                                                : launch(pt_display_kernel<DISPLAY_TONE_REINHARD, DISPLAY_TRANSFER_LINEAR>);
    else srgb ? launch(pt_display_kernel<DISPLAY_TONE_ACES, DISPLAY_TRANSFER_SRGB>)
              : launch(pt_display_kernel<DISPLAY_TONE_ACES, DISPLAY_TRANSFER_LINEAR>);
    HIPCHK(c, hipGetLastError());
    return mark_stream(c);
}

int pnrt_read_display(pnrt_ctx* c, uint8_t* out) {
    if (!c || !out) return PNRT_E_ARG;
    if (!c->disp) return set_err(c, PNRT_E_STATE, "read_display: display first");
    if (c->disp_width != c->width || c->disp_height != c->height)
        return set_err(c, PNRT_E_STATE, "read_display: the display image has another size than the frame: display again");
    return read_back(c, out, c->disp, (size_t)c->width * c->height * 4);
}

void* pnrt_display_device_ptr(pnrt_ctx* c) { return c ? c->disp.p : nullptr; }

int pnrt_luma_histogram_read(pnrt_ctx* c, int source, const void* src_device, int band, int nsh, int shard,
                             pnrt_luma_histogram* out) {
    if (!c || !out) return PNRT_E_ARG;
    int rc;
    if ((rc = check_selector(c, "luma_histogram_read", band, nsh, shard))) return rc;
    const float4* src = display_source(c, "luma_histogram_read", source, src_device, &rc);
    if (!src) return rc;
    if ((rc = check_fault(c))) return rc;        // completed work that faulted
    HIPCHK(c, hipSetDevice(c->device));
    static_assert(sizeof(LumaHist) == sizeof(pnrt_luma_histogram), "the device record is the public one");
    std::memset(out, 0, sizeof *out);
    const int rows = shard_rows(c->height, band, nsh, shard);
    const size_t total = (size_t)rows * c->width;
    if (total) {
        if ((rc = c->luma_hist.reserve(c, sizeof(LumaHist)))) return rc;
        HIPCHK(c, hipMemsetAsync(c->luma_hist, 0, sizeof(LumaHist), c->stream));
        const unsigned grid = (unsigned)std::min<size_t>((total + LUMA_HIST_BLOCK - 1) / LUMA_HIST_BLOCK, LUMA_HIST_MAX_BLOCKS);
        {
            ProfScope ps(c, PNRT_K_BLEND);
            hipLaunchKernelGGL(pt_luma_hist_kernel, dim3(grid), dim3(LUMA_HIST_BLOCK), 0, c->stream, src, c->luma_hist,
                               (uint32_t)c->width, (uint32_t)rows, band, nsh, shard);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(out, c->luma_hist, sizeof(LumaHist), hipMemcpyDeviceToHost, c->stream));
        if ((rc = mark_stream(c))) return rc;
    }
    HIPCHK(c, sync_all(c));
    return check_fault(c);
}

// Host only: the exposure that puts the trimmed mean bin of the histogram at `key`
// (DESIGN.md section 26), in integer arithmetic up to the one float multiply.
int pnrt_exposure_from_histogram(const pnrt_luma_histogram* h, int low, int high, float key, float* exposure_out) {
    if (!h || !exposure_out) return PNRT_E_ARG;
    if (!(0 <= low && low < high && high <= 1000)) return PNRT_E_ARG;
    if (!std::isfinite(key) || !(key > 0.0f)) return PNRT_E_ARG;
    static const uint32_t kT[16] = {0x3F800000u, 0x3F85AAC3u, 0x3F8B95C2u, 0x3F91C3D3u, 0x3F9837F0u, 0x3F9EF532u,
                                    0x3FA5FED7u, 0x3FAD583Fu, 0x3FB504F3u, 0x3FBD08A4u, 0x3FC5672Au, 0x3FCE248Cu,
                                    0x3FD744FDu, 0x3FE0CCDFu, 0x3FEAC0C7u, 0x3FF5257Du};      // the floats nearest 2^(j/16)
    const int64_t n = h->n_counted;
    const int64_t lo = n * low / 1000, hi = n * high / 1000;
    int64_t cum = 0, S = 0, C = 0;
    for (int b = 0; b < PNRT_LUMA_BINS; ++b) {
        const int64_t prev = cum;
        cum += h->bins[b];
        const int64_t cnt = std::min(cum, hi) - std::max(prev, lo);
        if (cnt > 0) { S += cnt * b; C += cnt; }
    }
    if (C == 0) { *exposure_out = 1.0f; return PNRT_OK; }
    const int m = (int)((2 * S + C) / (2 * C));
    const int k = 256 - m;
    const int e = k >= 0 ? k / 16 : -((-k + 15) / 16);
    const int j = k - 16 * e;
    float t;
    std::memcpy(&t, &kT[j], 4);
    *exposure_out = key * std::ldexp(t, e);
    return PNRT_OK;
}

int pnrt_profile_enable(pnrt_ctx* c, int on) {
    if (!c) return PNRT_E_ARG;
    int rc = prof_collect(c);
    if (rc) return rc;
    c->prof_on = on != 0;
    for (int k = 0; k < PNRT_K_COUNT; ++k) { c->prof_ms[k] = 0.0; c->prof_n[k] = 0; }
    return PNRT_OK;
}

int pnrt_profile_select(pnrt_ctx* c, int mask) {
    if (!c) return PNRT_E_ARG;
    c->prof_mask = mask;
    return PNRT_OK;
}

int pnrt_profile_read(pnrt_ctx* c, pnrt_profile* out) {
    if (!c || !out) return PNRT_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = prof_collect(c);
    if (rc) return rc;
    for (int k = 0; k < PNRT_K_COUNT; ++k) { out->ms[k] = c->prof_ms[k]; out->launches[k] = c->prof_n[k]; }
    return PNRT_OK;
}

int pnrt_pack_rows(pnrt_ctx* c, void* dst, int band, int nsh, int shard) {
    if (!c || !dst) return PNRT_E_ARG;
    if (!c->accum) return set_err(c, PNRT_E_STATE, "pack_rows: no frame");
    if (int rc = check_selector(c, "pack_rows", band, nsh, shard)) return rc;
    if (int rc = check_fault(c)) return rc;      // completed work that faulted
    HIPCHK(c, hipSetDevice(c->device));
    int rows = shard_rows(c->height, band, nsh, shard);
    size_t total = (size_t)rows * c->width;
    if (total == 0) return PNRT_OK;
    hipLaunchKernelGGL(pt_pack_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream,
                       c->accum, static_cast<float4*>(dst), c->width, rows, band, nsh, shard);
    HIPCHK(c, hipGetLastError());
    return mark_stream(c);
}

int pnrt_unpack_rows(pnrt_ctx* c, const void* src, void* image, int band, int nsh, int shard) {
    if (!c || !src || !image) return PNRT_E_ARG;
    if (c->width <= 0 || c->height <= 0) return set_err(c, PNRT_E_STATE, "unpack_rows: no frame");
    if (int rc = check_selector(c, "unpack_rows", band, nsh, shard)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    int rows = shard_rows(c->height, band, nsh, shard);
    size_t total = (size_t)rows * c->width;
    if (total == 0) return PNRT_OK;
    hipLaunchKernelGGL(pt_unpack_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream,
                       static_cast<const float4*>(src), static_cast<float4*>(image), c->width, rows, band, nsh, shard);
    HIPCHK(c, hipGetLastError());
    return mark_stream(c);
}

int pnrt_synchronize(pnrt_ctx* c) {
    if (!c) return PNRT_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_all(c));
    return check_fault(c);
}

int pnrt_get_device_info(pnrt_ctx* c, pnrt_device_info* info) {
    if (!c || !info) return PNRT_E_ARG;
    info->n_interior = c->n_interior;
    info->n_triangles = c->scene.n_tris;
    info->max_depth = c->max_depth;
    info->device_bytes = c->scene_bytes;
    info->root_is_leaf = c->root_is_leaf;
    info->stack_limit = PT_STACK;
    info->has_leaf_table = c->scene.has_leaf_table ? 1 : 0;
    return PNRT_OK;
}

int pnrt_debug_math(pnrt_ctx* c, int fn, const float* a, const float* b, float* out, int n) {
    if (!c || !a || !out || n <= 0) return PNRT_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<float> da, db, dout;
    size_t bytes = (size_t)n * 4;
    HIPCHK(c, da.alloc(bytes));
    HIPCHK(c, db.alloc(bytes));
    HIPCHK(c, dout.alloc(bytes));
    HIPCHK(c, hipMemcpy(da, a, bytes, hipMemcpyHostToDevice));
    if (b) HIPCHK(c, hipMemcpy(db, b, bytes, hipMemcpyHostToDevice));
    else HIPCHK(c, hipMemset(db, 0, bytes));
    hipLaunchKernelGGL(pt_math_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, fn, da, db, dout, n);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, sync_all(c));
    HIPCHK(c, hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
    return PNRT_OK;
}

}  // extern "C"

// ---- GPU BuildBVH (pt_bvh.h) -----------------------------------------------------------------
namespace {
struct DevAllocs {                     // device scratch of one build, freed on every return path
    std::vector<DevBuf<void>> p;
    template <typename T> hipError_t get(T** out, size_t count) {
        p.emplace_back();
        hipError_t e = p.back().alloc(count * sizeof(T) + 16);
        if (e == hipSuccess) *out = static_cast<T*>(p.back().p);
        return e;
    }
};
}  // namespace

static unsigned blocks_for(long long n, int per) { return (unsigned)((n + per - 1) / per); }

extern "C" int pnrt_bvh_build(pnrt_ctx* c, const float* tb, int n, float* nodes_out, int cap, int* n_nodes_out,
                              int32_t* order_out, int* max_depth_out) {
    if (!c) return PNRT_E_ARG;
    if (!tb || n <= 0 || !nodes_out || !n_nodes_out || !order_out) return set_err(c, PNRT_E_ARG, "bvh_build: bad arguments");
    if (n >= (1 << 24)) return set_err(c, PNRT_E_ARG, "bvh_build: >= 2^24 triangles cannot be stored as exact floats");
    if (cap < 2 * n - 1) return set_err(c, PNRT_E_ARG, "bvh_build: node capacity must be >= 2 * n_triangles - 1");
    HIPCHK(c, hipSetDevice(c->device));
    // triangle bounds + centres: A = (pMin, cx), B = (pMax, cy), C = cz
    std::vector<float4> hA(n), hB(n);
    std::vector<float> hC(n);
    for (int i = 0; i < n; ++i) {
        const float* t = tb + 9 * (size_t)i;
        for (int k = 0; k < 9; ++k)
            if (!std::isfinite(t[k])) return set_err(c, PNRT_E_SCENE, "bvh_build: triangle " + std::to_string(i) + " has a non-finite bound");
        hA[i] = make_float4(t[0], t[1], t[2], t[6]);
        hB[i] = make_float4(t[3], t[4], t[5], t[7]);
        hC[i] = t[8];
    }
    const size_t segcap = (size_t)n / (BVH_SMALL + 1) + 2;
    const size_t chcap = (size_t)n / BVH_CHUNK + segcap + 2;
    DevAllocs m;
    float4 *A, *B; float* C; int *order, *Fpos, *Tpos, *ctrue, *excl;
    BvhSeg* segs[2]; BvhChunk* chunks[2]; BvhAcc* acc; BvhTop* top; BvhSmall* small; BvhLocal* loc; BvhCtr* ctr;
    HIPCHK(c, m.get(&A, n)); HIPCHK(c, m.get(&B, n)); HIPCHK(c, m.get(&C, n));
    HIPCHK(c, m.get(&order, n)); HIPCHK(c, m.get(&Fpos, n)); HIPCHK(c, m.get(&Tpos, n));
    HIPCHK(c, m.get(&ctrue, chcap)); HIPCHK(c, m.get(&excl, chcap));
    HIPCHK(c, m.get(&segs[0], segcap)); HIPCHK(c, m.get(&segs[1], segcap));
    HIPCHK(c, m.get(&chunks[0], chcap)); HIPCHK(c, m.get(&chunks[1], chcap));
    HIPCHK(c, m.get(&acc, segcap)); HIPCHK(c, m.get(&top, 2 * (size_t)n + 2));
    HIPCHK(c, m.get(&small, (size_t)n + 1)); HIPCHK(c, m.get(&loc, 2 * (size_t)n + 2));
    HIPCHK(c, m.get(&ctr, 1));
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(A, hA.data(), n * sizeof(float4), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(B, hB.data(), n * sizeof(float4), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(C, hC.data(), n * sizeof(float), hipMemcpyHostToDevice, st));
    {
        std::vector<int> iota(n);
        for (int i = 0; i < n; ++i) iota[i] = i;
        HIPCHK(c, hipMemcpyAsync(order, iota.data(), n * sizeof(int), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    BvhCtr h{};
    int nseg = 0, nch = 0, cur = 0;
    if (n > BVH_SMALL) {                      // root = large range 0 (temporary id 0)
        BvhSeg s0{}; s0.L = 0; s0.R = n; s0.depth = 0; s0.tmp = 0; s0.chunk0 = 0;
        std::vector<BvhChunk> ck;
        for (int p = 0; p < n; p += BVH_CHUNK) ck.push_back({0, p, std::min(p + BVH_CHUNK, n), 0});
        nseg = 1; nch = (int)ck.size();
        HIPCHK(c, hipMemcpy(segs[0], &s0, sizeof s0, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(chunks[0], ck.data(), ck.size() * sizeof(BvhChunk), hipMemcpyHostToDevice));
        h.ntop = 1;
    } else {                                  // root = small range 0
        BvhSmall s0{}; s0.L = 0; s0.R = n; s0.depth = 0;
        HIPCHK(c, hipMemcpy(small, &s0, sizeof s0, hipMemcpyHostToDevice));
        h.nsmall = 1;
    }
    HIPCHK(c, hipMemcpy(ctr, &h, sizeof h, hipMemcpyHostToDevice));
    int levels = 0;
    while (nseg > 0) {
        if (++levels > 100000) return set_err(c, PNRT_E_SCENE, "bvh_build: tree too deep");
        h.nseg = 0; h.nch = 0;
        HIPCHK(c, hipMemcpyAsync(ctr, &h, sizeof h, hipMemcpyHostToDevice, st));
        BvhSeg* sg = segs[cur]; BvhChunk* ck = chunks[cur];
        const unsigned gs = blocks_for(nseg, 256);
        hipLaunchKernelGGL(bvh_init_kernel, dim3(gs), dim3(256), 0, st, acc, nseg);
        hipLaunchKernelGGL(bvh_bounds_kernel, dim3(nch), dim3(256), 0, st, (const BvhChunk*)ck, acc, (const int*)order,
                           (const float4*)A, (const float4*)B, (const float*)C);
        hipLaunchKernelGGL(bvh_axis_kernel, dim3(gs), dim3(256), 0, st, (const BvhSeg*)sg, acc, nseg, (const int*)order,
                           (const float4*)A, (const float4*)B);
        hipLaunchKernelGGL(bvh_bucket_kernel, dim3(nch), dim3(256), 0, st, (const BvhChunk*)ck, acc, (const int*)order,
                           (const float4*)A, (const float4*)B, (const float*)C);
        hipLaunchKernelGGL(bvh_split_kernel, dim3(gs), dim3(256), 0, st, (const BvhSeg*)sg, acc, nseg);
        hipLaunchKernelGGL(bvh_count_kernel, dim3(nch), dim3(256), 0, st, (const BvhChunk*)ck, (const BvhAcc*)acc,
                           (const int*)order, (const float4*)A, (const float4*)B, (const float*)C, ctrue);
        hipLaunchKernelGGL(bvh_scan_kernel, dim3(1), dim3(1024), 0, st, (const int*)ctrue, excl, nch);
        hipLaunchKernelGGL(bvh_lists_kernel, dim3(nch), dim3(256), 0, st, (const BvhChunk*)ck, (const BvhSeg*)sg, acc,
                           (const int*)order, (const float4*)A, (const float4*)B, (const float*)C, (const int*)excl,
                           Fpos, Tpos);
        hipLaunchKernelGGL(bvh_swap_kernel, dim3(nch), dim3(256), 0, st, (const BvhChunk*)ck, (const BvhSeg*)sg,
                           (const BvhAcc*)acc, order, (const int*)Fpos, (const int*)Tpos);
        hipLaunchKernelGGL(bvh_emit_kernel, dim3(gs), dim3(256), 0, st, (const BvhSeg*)sg, (const BvhAcc*)acc, nseg, top,
                           segs[cur ^ 1], chunks[cur ^ 1], small, ctr);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&h, ctr, sizeof h, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        nseg = h.nseg; nch = h.nch; cur ^= 1;
        if ((size_t)nseg > segcap || (size_t)nch > chcap || h.ntop > 2 * n + 2 || h.nsmall > n + 1)
            return set_err(c, PNRT_E_SCENE, "bvh_build: internal capacity exceeded");
    }
    if (h.nsmall > 0) {
        hipLaunchKernelGGL(bvh_small_kernel, dim3(blocks_for(h.nsmall, 4)), dim3(256), 0, st, small, h.nsmall, order,
                           (const float4*)A, (const float4*)B, (const float*)C, loc, ctr);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpyAsync(&h, ctr, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (h.ntop < 0 || h.ntop > 2 * n + 2 || h.nsmall < 0 || h.nsmall > n + 1 || h.small_nodes > 2 * n)
        return set_err(c, PNRT_E_SCENE, "bvh_build: internal capacity exceeded");
    std::vector<BvhTop> ht(h.ntop);
    std::vector<BvhSmall> hs(h.nsmall);
    if (h.ntop) HIPCHK(c, hipMemcpyAsync(ht.data(), top, h.ntop * sizeof(BvhTop), hipMemcpyDeviceToHost, st));
    if (h.nsmall) HIPCHK(c, hipMemcpyAsync(hs.data(), small, h.nsmall * sizeof(BvhSmall), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    // pre-order ids (the static nodeId counter of BVH.hpp:94-95): left subtree, then right
    std::vector<int> ftop(h.ntop + 1, 0), fsmall(h.nsmall + 1, 0);
    std::vector<int> stk{h.ntop ? 0 : -1};
    int counter = 0;
    while (!stk.empty()) {
        const int ref = stk.back();
        stk.pop_back();
        if (ref >= 0) {
            ftop[ref] = counter++;
            if (ht[ref].axis != -1) { stk.push_back(ht[ref].right); stk.push_back(ht[ref].left); }
        } else {
            fsmall[-ref - 1] = counter;
            counter += hs[-ref - 1].count;
        }
    }
    if (counter > cap) return set_err(c, PNRT_E_SCENE, "bvh_build: node capacity exceeded");
    int *dft, *dfs; float* dout;
    HIPCHK(c, m.get(&dft, ftop.size())); HIPCHK(c, m.get(&dfs, fsmall.size())); HIPCHK(c, m.get(&dout, 12 * (size_t)counter));
    HIPCHK(c, hipMemcpyAsync(dft, ftop.data(), ftop.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(dfs, fsmall.data(), fsmall.size() * sizeof(int), hipMemcpyHostToDevice, st));
    if (h.ntop)
        hipLaunchKernelGGL(bvh_scatter_top_kernel, dim3(blocks_for(h.ntop, 256)), dim3(256), 0, st, (const BvhTop*)top,
                           h.ntop, (const int*)dft, (const int*)dfs, dout);
    if (h.nsmall)
        hipLaunchKernelGGL(bvh_scatter_small_kernel, dim3(blocks_for(h.nsmall, 4)), dim3(256), 0, st,
                           (const BvhSmall*)small, h.nsmall, (const BvhLocal*)loc, (const int*)dfs, dout);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(nodes_out, dout, 12 * (size_t)counter * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(order_out, order, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    *n_nodes_out = counter;
    if (max_depth_out) *max_depth_out = h.max_depth;
    return PNRT_OK;
}
