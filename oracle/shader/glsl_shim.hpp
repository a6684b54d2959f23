// oracle/shader/glsl_shim.hpp -- TEST INFRASTRUCTURE.  The part of GLSL 4.50 that
// shaders/ray_tracing.comp uses, as C++, so that the shader's own text (translated
// by translate.py, never committed) compiles with g++ -ffp-contract=off and runs
// on the CPU (shader_driver.cpp).
//
// Everything here is a DEFINITION the shader text does not carry; each is bound to
// the oracle's documented choice (oracle/pn_oracle.c, oracle/pn_libm.h), so the pin
// cannot reach them -- DESIGN.md 7 lists them in one table:
//   sin cos asin atan(y,x) log pow      pn_libm.h (PN-libm v1)
//   sqrt, /                             IEEE binary32, correctly rounded
//   dot cross length normalize mix      GLSL 4.50 8.3/8.5 formulas, summed left to right
//   min max clamp                       NaN-dropping, first operand on ties
//   texelFetch (buffer, 1-D)            RGB32F texels, out of range -> 0
//   texture (HDRImage, RandomHDR)       RGB32F, CLAMP_TO_EDGE, LINEAR, level 0
//   texture (textures[i])               UNORM8, REPEAT, LINEAR, level 0, rows aligned to 4 bytes
//   unbound sampler                     (0, 0, 0)
//   imageLoad / imageStore              RGBA32F array, row 0 = bottom
//   in / out / inout                    by value / by reference (translate.py)
//   uninitialised variables             0 (PNSH_POISON: a NaN pattern, to show none is read)
#pragma once
#include <cstdint>
#include <cstring>
#include <cmath>
#include "../pn_libm.h"

namespace glsl {

typedef uint32_t uint;

#ifdef PNSH_POISON
static inline float undef_f() { return pnl_bits2f(0x7fc0deadu); }
static inline int undef_i() { return 0x7fdead00; }
#else
static inline float undef_f() { return 0.0f; }
static inline int undef_i() { return 0; }
#endif

struct vec2 {
    union { struct { float x, y; }; struct { float r, g; }; };
    vec2() : x(undef_f()), y(undef_f()) {}
    explicit vec2(float s) : x(s), y(s) {}
    vec2(float a, float b) : x(a), y(b) {}
    float& operator[](int i) { return i == 0 ? x : y; }
    float operator[](int i) const { return i == 0 ? x : y; }
    vec2 xy() const { return *this; }
};
struct vec3 {
    union { struct { float x, y, z; }; struct { float r, g, b; }; };
    vec3() : x(undef_f()), y(undef_f()), z(undef_f()) {}
    explicit vec3(float s) : x(s), y(s), z(s) {}
    vec3(float a, float b, float c) : x(a), y(b), z(c) {}
    float& operator[](int i) { return i == 0 ? x : i == 1 ? y : z; }
    float operator[](int i) const { return i == 0 ? x : i == 1 ? y : z; }
    vec2 xy() const { return vec2(x, y); }
    vec2 rg() const { return vec2(x, y); }
    vec3 rgb() const { return *this; }
};
struct vec4 {
    union { struct { float x, y, z, w; }; struct { float r, g, b, a; }; };
    vec4() : x(undef_f()), y(undef_f()), z(undef_f()), w(undef_f()) {}
    vec4(float a_, float b_, float c_, float d_) : x(a_), y(b_), z(c_), w(d_) {}
    vec4(vec3 v, float d_) : x(v.x), y(v.y), z(v.z), w(d_) {}
    vec3 rgb() const { return vec3(x, y, z); }
    vec2 rg() const { return vec2(x, y); }
    vec2 xy() const { return vec2(x, y); }
};
struct ivec2 {
    int x, y;
    ivec2() : x(undef_i()), y(undef_i()) {}
    ivec2(int a, int b) : x(a), y(b) {}
    ivec2 xy() const { return *this; }
};
struct ivec3 {
    int x, y, z;
    ivec3() : x(undef_i()), y(undef_i()), z(undef_i()) {}
    ivec3(int a, int b, int c) : x(a), y(b), z(c) {}
    explicit ivec3(vec3 v) : x(int(v.x)), y(int(v.y)), z(int(v.z)) {}   // int(float): truncation
    int& operator[](int i) { return i == 0 ? x : i == 1 ? y : z; }
    int operator[](int i) const { return i == 0 ? x : i == 1 ? y : z; }
    ivec2 xy() const { return ivec2(x, y); }
};
struct mat4 { float m[16]; };

static inline bool operator==(ivec2 a, ivec2 b) { return a.x == b.x && a.y == b.y; }
static inline bool operator==(vec3 a, vec3 b) { return a.x == b.x && a.y == b.y && a.z == b.z; }

// component-wise arithmetic (GLSL 4.50 5.9)
static inline vec2 operator+(vec2 a, vec2 b) { return vec2(a.x + b.x, a.y + b.y); }
static inline vec2 operator*(vec2 a, float s) { return vec2(a.x * s, a.y * s); }
static inline vec2 operator*(float s, vec2 a) { return vec2(s * a.x, s * a.y); }
static inline vec2& operator*=(vec2& a, vec2 b) { a.x = a.x * b.x; a.y = a.y * b.y; return a; }
static inline vec2& operator+=(vec2& a, float s) { a.x = a.x + s; a.y = a.y + s; return a; }

static inline vec3 operator+(vec3 a, vec3 b) { return vec3(a.x + b.x, a.y + b.y, a.z + b.z); }
static inline vec3 operator-(vec3 a, vec3 b) { return vec3(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline vec3 operator*(vec3 a, vec3 b) { return vec3(a.x * b.x, a.y * b.y, a.z * b.z); }
static inline vec3 operator*(vec3 a, float s) { return vec3(a.x * s, a.y * s, a.z * s); }
static inline vec3 operator*(float s, vec3 a) { return vec3(s * a.x, s * a.y, s * a.z); }
static inline vec3 operator/(vec3 a, float s) { return vec3(a.x / s, a.y / s, a.z / s); }
static inline vec3 operator/(float s, vec3 a) { return vec3(s / a.x, s / a.y, s / a.z); }
static inline vec3 operator-(vec3 a) { return vec3(-a.x, -a.y, -a.z); }
static inline vec3& operator+=(vec3& a, vec3 b) { a = a + b; return a; }
static inline vec3& operator*=(vec3& a, vec3 b) { a = a * b; return a; }

// ---- built-ins: scalar forms are plain functions, so GLSL's int -> float conversions resolve
static inline float sqrt(float x) { return ::sqrtf(x); }
static inline float abs(float x) { return pnl_fabs(x); }
static inline float sin(float x) { return pnl_sin(x); }
static inline float cos(float x) { return pnl_cos(x); }
static inline float asin(float x) { return pnl_asin(x); }
static inline float atan(float y, float x) { return pnl_atan2(y, x); }
static inline float log(float x) { return pnl_log(x); }
static inline float pow(float x, float y) { return pnl_pow(x, y); }
static inline float min(float a, float b) { return (b < a || a != a) ? b : a; }
static inline float max(float a, float b) { return (b > a || a != a) ? b : a; }
static inline float clamp(float x, float lo, float hi) { return min(max(x, lo), hi); }
static inline float mix(float x, float y, float a) { return x * (1.0f - a) + y * a; }
static inline vec3 min(vec3 a, vec3 b) { return vec3(min(a.x, b.x), min(a.y, b.y), min(a.z, b.z)); }
static inline vec3 max(vec3 a, vec3 b) { return vec3(max(a.x, b.x), max(a.y, b.y), max(a.z, b.z)); }
static inline vec3 clamp(vec3 v, vec3 lo, vec3 hi) {
    return vec3(clamp(v.x, lo.x, hi.x), clamp(v.y, lo.y, hi.y), clamp(v.z, lo.z, hi.z));
}
static inline vec3 mix(vec3 x, vec3 y, float a) { return vec3(mix(x.x, y.x, a), mix(x.y, y.y, a), mix(x.z, y.z, a)); }
static inline float dot(vec3 a, vec3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
static inline vec3 cross(vec3 a, vec3 b) {
    return vec3(a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y);
}
static inline float length(vec3 a) { return ::sqrtf(dot(a, a)); }
static inline vec3 normalize(vec3 a) { return a / length(a); }

// ---- resources ---------------------------------------------------------------
struct samplerBuffer { const float* p = nullptr; int n = 0; };      // n RGB32F texels
struct sampler1D { const float* p = nullptr; int n = 0; };
struct sampler2D {
    int kind = 0;                    // 0 unbound, 1 RGB32F clamp-to-edge, 2 UNORM8 repeat
    const float* f = nullptr;
    const uint8_t* u8 = nullptr;     // rows of align4(w * ch) bytes
    int w = 0, h = 0, ch = 0;
};
struct image2D { float* p = nullptr; int w = 0, h = 0; };

extern uint64_t fetches_out_of_range;          // counted for the driver's report

static inline vec4 texel_rgb32f(const float* p, int n, int i) {
    if (i < 0 || i >= n) { ++fetches_out_of_range; return vec4(0.0f, 0.0f, 0.0f, 1.0f); }
    return vec4(p[3 * i], p[3 * i + 1], p[3 * i + 2], 1.0f);
}
static inline vec4 texelFetch(const samplerBuffer& s, int i) { return texel_rgb32f(s.p, s.n, i); }
static inline vec4 texelFetch(const sampler1D& s, int i, int) { return texel_rgb32f(s.p, s.n, i); }

static inline int wrap_clamp(float fl, int n) {
    if (fl != fl) return 0;
    fl = min(max(fl, -1.0f), (float)n);
    int i = (int)fl;
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}
static inline int wrap_repeat(float fl, int n) {
    if (fl != fl) return 0;
    float q = ::floorf(fl / (float)n);
    float m = fl - (float)n * q;
    m = min(max(m, 0.0f), (float)n);
    int i = (int)m;
    if (i >= n) i -= n;
    if (i < 0) i += n;
    return i;
}
static inline float unorm8(uint8_t c) { return (float)c / 255.0f; }
static inline vec3 fetch2d(const sampler2D& s, int i, int j) {
    if (s.kind == 1) {
        const float* t = s.f + 3 * ((size_t)j * s.w + i);
        return vec3(t[0], t[1], t[2]);
    }
    size_t stride = (size_t)((s.w * s.ch + 3) & ~3);
    const uint8_t* p = s.u8 + (size_t)j * stride + (size_t)i * s.ch;
    if (s.ch == 1) return vec3(unorm8(p[0]), 0.0f, 0.0f);
    if (s.ch == 2) return vec3(unorm8(p[0]), unorm8(p[1]), 0.0f);
    return vec3(unorm8(p[0]), unorm8(p[1]), unorm8(p[2]));
}
// GL 4.5 8.14.2 LINEAR at level 0: u' = s*W - 0.5, i0 = floor(u'), a = frac(u'),
// tau = (1-a)(1-b) T00 + a(1-b) T10 + (1-a)b T01 + ab T11, summed left to right.
static inline vec4 texture(const sampler2D& s, vec2 uv) {
    if (s.kind == 0) return vec4(0.0f, 0.0f, 0.0f, 1.0f);
    float fu = uv.x * (float)s.w - 0.5f, fv = uv.y * (float)s.h - 0.5f;
    float flu = ::floorf(fu), flv = ::floorf(fv);
    float a = fu - flu, b = fv - flv;
    int i0, i1, j0, j1;
    if (s.kind == 1) {
        i0 = wrap_clamp(flu, s.w); i1 = wrap_clamp(flu + 1.0f, s.w);
        j0 = wrap_clamp(flv, s.h); j1 = wrap_clamp(flv + 1.0f, s.h);
    } else {
        i0 = wrap_repeat(flu, s.w); i1 = wrap_repeat(flu + 1.0f, s.w);
        j0 = wrap_repeat(flv, s.h); j1 = wrap_repeat(flv + 1.0f, s.h);
    }
    vec3 t00 = fetch2d(s, i0, j0), t10 = fetch2d(s, i1, j0), t01 = fetch2d(s, i0, j1), t11 = fetch2d(s, i1, j1);
    float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
    return vec4(((w00 * t00.x + w10 * t10.x) + w01 * t01.x) + w11 * t11.x,
                ((w00 * t00.y + w10 * t10.y) + w01 * t01.y) + w11 * t11.y,
                ((w00 * t00.z + w10 * t10.z) + w01 * t01.z) + w11 * t11.z, 1.0f);
}
static inline vec4 texture2D(const sampler2D& s, vec2 uv) { return texture(s, uv); }

static inline vec4 imageLoad(const image2D& im, ivec2 p) {
    const float* q = im.p + 4 * ((size_t)p.y * im.w + p.x);
    return vec4(q[0], q[1], q[2], q[3]);
}
static inline void imageStore(const image2D& im, ivec2 p, vec4 v) {
    float* q = im.p + 4 * ((size_t)p.y * im.w + p.x);
    q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
}

extern ivec3 gl_GlobalInvocationID;

}  // namespace glsl
