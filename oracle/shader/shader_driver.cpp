// oracle/shader/shader_driver.cpp -- TEST INFRASTRUCTURE (golden-vector generator).
//
// Runs the reference's OWN shader text on the CPU: shaders/ray_tracing.comp,
// translated to C++ by translate.py into oracle/_ref/ray_tracing_comp.inc and
// compiled here against glsl_shim.hpp (oracle/shader/Makefile).  Its outputs pin
// the oracle's shading half -- the Disney BRDF and its sampling, light and
// environment sampling, the path loop, the order of the RNG draws -- and its
// intersection code under the GLSL's own rules (oracle/pn_oracle.c, sem 0).
//
// stdin:  "PNSH", the scene in the reference's flattened arrays, textures, the
//         environment, the frame (tests/shader_pin.py scene_blob), then one command:
//   "IMAG" u32 first, u32 n, i32 y0, i32 y1
//          shader_main() for every pixel of rows [y0, y1), frames first..first+n-1,
//          into a zeroed RGBA32F accumulation image; stdout: H*W*4 floats
//   "FUNC" i32 fn, i32 n, i32 words_in, then n * words_in u32
//          one shader function per record (the table below); stdout: n * words_out u32
// stderr: one line with the count of texel fetches that fell outside their buffer.
#include "glsl_shim.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace glsl {
uint64_t fetches_out_of_range = 0;
ivec3 gl_GlobalInvocationID;
#include "ray_tracing_comp.inc"
}  // namespace glsl

using namespace glsl;

static void rd(void* p, size_t n) {
    if (n && fread(p, 1, n, stdin) != n) { fprintf(stderr, "short read\n"); exit(2); }
}
template <class T> static T rd1() { T v; rd(&v, sizeof v); return v; }
static std::vector<float> rdf(size_t n) { std::vector<float> v(n); rd(v.data(), n * 4); return v; }

static uint32_t fb(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float bf(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

struct In {
    const uint32_t* p;
    float f() { return bf(*p++); }
    uint32_t u() { return *p++; }
    int i() { return (int)*p++; }
    vec2 v2() { float a = f(), b = f(); return vec2(a, b); }
    vec3 v3() { float a = f(), b = f(), c = f(); return vec3(a, b, c); }
    Material mat() {
        Material m;
        m.emssive = v3(); m.baseColor = v3();
        m.subsurface = f(); m.metallic = f(); m.specular = f();
        m.specularTint = f(); m.roughness = f(); m.anisotropic = f();
        m.sheen = f(); m.sheenTint = f(); m.clearcoat = f();
        m.clearcoatGloss = f(); m.IOR = f(); m.transmission = f();
        return m;
    }
    Ray ray() { Ray r; r.origin = v3(); r.dir = v3(); r.tMax = f(); return r; }
};
struct Out {
    uint32_t* p;
    void f(float x) { *p++ = fb(x); }
    void u(uint32_t x) { *p++ = x; }
    void v2(vec2 v) { f(v.x); f(v.y); }
    void v3(vec3 v) { f(v.x); f(v.y); f(v.z); }
    void isect(bool hit, const Interaction* is, float tmax_after) {
        uint32_t* o = p;
        memset(o, 0, 13 * 4);
        o[0] = hit;
        if (hit && is) {
            p = o + 1; v3(is->position); v3(is->normal); v2(is->texcoord);
            u((uint32_t)is->textureId); u((uint32_t)is->materialId); f(is->time);
        }
        o[12] = fb(tmax_after);
        p = o + 13;
    }
};

// fn -> words in, words out (the same table as pno_shade_eval, oracle/pn_oracle.h)
static const int WORDS[27][2] = {
    {33, 3}, {33, 5}, {15, 3}, {15, 3}, {10, 4}, {3, 6}, {2, 1}, {2, 1}, {5, 1}, {2, 1}, {5, 1}, {3, 2}, {3, 3},
    {1, 8}, {1, 1}, {3, 10}, {2, 2}, {2, 2}, {4, 2}, {1, 2}, {2, 7}, {1, 18},
    {8, 13}, {8, 13}, {8, 13}, {7, 13}, {7, 13}};

static void eval(int fn, In in, Out out) {
    switch (fn) {
    case 0: { vec3 V = in.v3(), N = in.v3(), L = in.v3(), X = in.v3(), Y = in.v3(); Material m = in.mat();
              out.v3(DisneyBRDF(V, N, L, X, Y, m)); break; }
    case 1: { seed = in.u(); vec3 V = in.v3(), N = in.v3(), T = in.v3(), B = in.v3(); Material m = in.mat();
              float r1 = in.f(), r2 = in.f(), pdf = 0.0f;
              vec3 L = SampleDisneyBRDF(V, N, T, B, m, r1, r2, pdf); out.v3(L); out.f(pdf); out.u(seed); break; }
    case 2: case 3: { vec3 n = in.v3(), t = in.v3(), b = in.v3(), v = in.v3(); float r1 = in.f(), r2 = in.f(), a = in.f();
              out.v3(fn == 2 ? SampleGTR1(n, t, b, v, r1, r2, a) : SampleGTR2(n, t, b, v, r1, r2, a)); break; }
    case 4: { seed = in.u(); vec3 n = in.v3(), t = in.v3(), b = in.v3();
              out.v3(SampleCosineHemisphere(n, t, b)); out.u(seed); break; }
    case 5: { vec3 n = in.v3(), t, b; BuildTangentSpace(n, t, b); out.v3(t); out.v3(b); break; }
    case 6: { float a = in.f(), b = in.f(); out.f(GTR1(a, b)); break; }
    case 7: { float a = in.f(), b = in.f(); out.f(GTR2(a, b)); break; }
    case 8: { float a = in.f(), b = in.f(), c = in.f(), d = in.f(), e = in.f(); out.f(GTR2_aniso(a, b, c, d, e)); break; }
    case 9: { float a = in.f(), b = in.f(); out.f(smithG_GGX(a, b)); break; }
    case 10: { float a = in.f(), b = in.f(), c = in.f(), d = in.f(), e = in.f(); out.f(smithG_GGX_aniso(a, b, c, d, e)); break; }
    case 11: out.v2(toSphericalCoord(in.v3())); break;
    case 12: out.v3(GetHDRImageColor(in.v3())); break;
    case 13: { seed = in.u(); vec3 L; float pdf = 0.0f; vec3 c = SampleHDRImage(L, pdf);
               out.v3(c); out.v3(L); out.f(pdf); out.u(seed); break; }
    case 14: out.u((uint32_t)GetLightIndex(in.f())); break;
    case 15: { int t = in.i(); vec2 u = in.v2(); Interaction r = TriangleSample(GetTriangle(t), u);
               out.v3(r.position); out.v3(r.normal); out.v2(r.texcoord);
               out.u((uint32_t)r.textureId); out.u((uint32_t)r.materialId); break; }
    case 16: out.v2(UniformSampleTriangle(in.v2())); break;
    case 17: { uint32_t i = in.u(), b = in.u(); out.v2(sobolVec2(i, b)); break; }
    case 18: { int x = in.i(), y = in.i(); imagePos = ivec2(x, y); out.v2(CranleyPattersonRotation(in.v2())); break; }
    case 19: { uint32_t s = in.u(); uint32_t r = wang_hash(s); out.u(r); out.u(s); break; }
    case 20: { float s = in.f(), t = in.f(); Ray r = CameraGetRay(s, t); out.v3(r.origin); out.v3(r.dir); out.f(r.tMax); break; }
    case 21: { Material m = GetMaterial(in.i()); out.v3(m.emssive); out.v3(m.baseColor);
               out.f(m.subsurface); out.f(m.metallic); out.f(m.specular); out.f(m.specularTint); out.f(m.roughness);
               out.f(m.anisotropic); out.f(m.sheen); out.f(m.sheenTint); out.f(m.clearcoat); out.f(m.clearcoatGloss);
               out.f(m.IOR); out.f(m.transmission); break; }
    case 22: { Ray r = in.ray(); int k = in.i(); bool h = BoundIntersect(GetBVHNode(k).bound, r);
               memset(out.p, 0, 13 * 4); out.p[0] = h; break; }
    case 23: { Ray r = in.ray(); int k = in.i(); Interaction is; bool h = TriangleIntersect(GetTriangle(k), r, is);
               out.isect(h, &is, r.tMax); break; }
    case 24: { Ray r = in.ray(); int k = in.i(); bool h = TriangleIntersectP(GetTriangle(k), r); out.isect(h, nullptr, r.tMax); break; }
    case 25: { Ray r = in.ray(); Interaction is; bool h = BVHIntersect(r, is); out.isect(h, &is, r.tMax); break; }
    case 26: { Ray r = in.ray(); bool h = BVHIntersectP(r); out.isect(h, nullptr, r.tMax); break; }
    }
}

int main() {
    char magic[4];
    rd(magic, 4);
    if (memcmp(magic, "PNSH", 4) != 0) { fprintf(stderr, "bad magic\n"); return 2; }
    int32_t nv = rd1<int32_t>(); std::vector<float> verts = rdf((size_t)nv * 15);
    int32_t nm = rd1<int32_t>(); std::vector<float> mats = rdf((size_t)nm * 18);
    int32_t nt = rd1<int32_t>(); std::vector<float> tris = rdf((size_t)nt * 6);
    int32_t nn = rd1<int32_t>(); std::vector<float> nodes = rdf((size_t)nn * 12);
    int32_t nl = rd1<int32_t>(); std::vector<float> lts = rdf((size_t)nl * 3);
    lightsSumArea = rd1<float>();
    lightsSize = nl;
    vertices.p = verts.data(); vertices.n = nv * 5;
    materials.p = mats.data(); materials.n = nm * 6;
    triangles.p = tris.data(); triangles.n = nt * 2;
    bvh_nodes.p = nodes.data(); bvh_nodes.n = nn * 4;
    lights.p = lts.data(); lights.n = nl;
    int32_t ntex = rd1<int32_t>();
    if (ntex < 0 || ntex > 20) { fprintf(stderr, "bad texture count\n"); return 2; }
    std::vector<std::vector<uint8_t>> tex(ntex);
    for (int t = 0; t < ntex; ++t) {
        int32_t w = rd1<int32_t>(), h = rd1<int32_t>(), ch = rd1<int32_t>();
        tex[t].resize((size_t)((w * ch + 3) & ~3) * h);
        rd(tex[t].data(), tex[t].size());
        textures[t].kind = 2; textures[t].u8 = tex[t].data();
        textures[t].w = w; textures[t].h = h; textures[t].ch = ch;
    }
    HasHDRImage = rd1<int32_t>();
    HDRImageWidth = rd1<int32_t>();
    HDRImageHeight = rd1<int32_t>();
    std::vector<float> hdr, table;
    if (HasHDRImage) {
        hdr = rdf((size_t)HDRImageWidth * HDRImageHeight * 3);
        table = rdf((size_t)HDRImageWidth * HDRImageHeight * 3);
        HDRImage.kind = 1; HDRImage.f = hdr.data(); HDRImage.w = HDRImageWidth; HDRImage.h = HDRImageHeight;
        RandomHDR = HDRImage; RandomHDR.f = table.data();
    }
    float cam[12];
    rd(cam, sizeof cam);
    camera.eye = vec3(cam[0], cam[1], cam[2]);
    camera.lowerLeftCorner = vec3(cam[3], cam[4], cam[5]);
    camera.horizontal = vec3(cam[6], cam[7], cam[8]);
    camera.vertical = vec3(cam[9], cam[10], cam[11]);
    CameraEye = camera.eye;
    SCREEN_WIDTH = rd1<int32_t>();
    SCREEN_HEIGHT = rd1<int32_t>();
    MAX_BOUNCE_DEPTH = rd1<int32_t>();
    imagePos = ivec2(0, 0);
    bounce = 0;
    seed = 1u;

    rd(magic, 4);
    if (memcmp(magic, "IMAG", 4) == 0) {
        uint32_t first = rd1<uint32_t>(), n = rd1<uint32_t>();
        int32_t y0 = rd1<int32_t>(), y1 = rd1<int32_t>();
        if (y0 < 0) y0 = 0;
        if (y1 > SCREEN_HEIGHT) y1 = SCREEN_HEIGHT;
        std::vector<float> accum((size_t)SCREEN_WIDTH * SCREEN_HEIGHT * 4, 0.0f);
        output_image.p = accum.data(); output_image.w = SCREEN_WIDTH; output_image.h = SCREEN_HEIGHT;
        for (int y = y0; y < y1; ++y)
            for (int x = 0; x < SCREEN_WIDTH; ++x)
                for (uint32_t k = 0; k < n; ++k) {
                    frameCount = first + k;
                    gl_GlobalInvocationID = ivec3(x, y, 0);
                    shader_main();
                }
        fwrite(accum.data(), 4, accum.size(), stdout);
    } else if (memcmp(magic, "FUNC", 4) == 0) {
        int32_t fn = rd1<int32_t>(), n = rd1<int32_t>(), win = rd1<int32_t>();
        if (fn < 0 || fn >= 27 || n < 0 || win != WORDS[fn][0]) { fprintf(stderr, "bad function record\n"); return 2; }
        const int wout = WORDS[fn][1];
        std::vector<uint32_t> in((size_t)n * win + 1), out((size_t)n * wout + 1, 0u);
        rd(in.data(), (size_t)n * win * 4);
        frameCount = 0;
        for (int i = 0; i < n; ++i) eval(fn, In{in.data() + (size_t)i * win}, Out{out.data() + (size_t)i * wout});
        fwrite(out.data(), 4, (size_t)n * wout, stdout);
    } else {
        fprintf(stderr, "bad command\n");
        return 2;
    }
    fprintf(stderr, "texel fetches out of range: %llu\n", (unsigned long long)fetches_out_of_range);
    return 0;
}
