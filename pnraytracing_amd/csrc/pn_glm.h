// pnraytracing_amd/csrc/pn_glm.h -- glm-equivalent float vectors and matrices, host code.
//
// The one copy of the glm 0.9.9.8 operation orders both libraries need: libpnrt_host.so
// places models with them (ModelOutput, model.hpp:101-135), libpnrt.so computes a
// placement's normal matrix and the light areas with them (pnrt_place_models).  Every
// product and sum is rounded on its own: compile with -ffp-contract=off.
#pragma once
#include <cmath>

namespace pnglm {

struct vec3 {
    float x = 0.f, y = 0.f, z = 0.f;
    vec3() = default;
    vec3(float a, float b, float c) : x(a), y(b), z(c) {}
    float& operator[](int i) { return i == 0 ? x : (i == 1 ? y : z); }
    float operator[](int i) const { return i == 0 ? x : (i == 1 ? y : z); }
};
inline vec3 operator+(vec3 a, vec3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline vec3 operator-(vec3 a, vec3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline vec3 operator*(vec3 a, vec3 b) { return {a.x * b.x, a.y * b.y, a.z * b.z}; }
inline vec3 operator*(vec3 v, float s) { return {v.x * s, v.y * s, v.z * s}; }
inline vec3 operator*(float s, vec3 v) { return {s * v.x, s * v.y, s * v.z}; }
inline bool operator==(vec3 a, vec3 b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
// glm compute_dot<vec3>: tmp = a*b; (tmp.x + tmp.y) + tmp.z
inline float dot(vec3 a, vec3 b) { vec3 t = a * b; return t.x + t.y + t.z; }
// glm compute_cross (func_geometric.inl)
inline vec3 cross(vec3 x, vec3 y) {
    return {x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y};
}
inline float length(vec3 v) { return std::sqrt(dot(v, v)); }
// ModelOutput's triangle area (model.hpp:101-135): |e1 x e2| * 0.5, the product in double
inline float tri_area(vec3 p0, vec3 p1, vec3 p2) { return (float)((double)length(cross(p1 - p0, p2 - p0)) * 0.5); }

struct vec4 {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    float& operator[](int i) { return v[i]; }
    float operator[](int i) const { return v[i]; }
};
inline vec4 V4(float a, float b, float c, float d) { vec4 r; r.v[0] = a; r.v[1] = b; r.v[2] = c; r.v[3] = d; return r; }
inline vec4 operator+(const vec4& a, const vec4& b) { return V4(a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + b[3]); }
inline vec4 operator-(const vec4& a, const vec4& b) { return V4(a[0] - b[0], a[1] - b[1], a[2] - b[2], a[3] - b[3]); }
inline vec4 operator*(const vec4& a, const vec4& b) { return V4(a[0] * b[0], a[1] * b[1], a[2] * b[2], a[3] * b[3]); }
inline vec4 operator*(const vec4& a, float s) { return V4(a[0] * s, a[1] * s, a[2] * s, a[3] * s); }

struct mat4 {  // column major, c[col][row]
    vec4 c[4];
    static mat4 identity() { mat4 m; for (int i = 0; i < 4; ++i) m.c[i][i] = 1.f; return m; }
    // 16 floats, column major, as pnrt_model_matrix writes them
    static mat4 load(const float* f) { mat4 m; for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) m.c[i][j] = f[4 * i + j]; return m; }
    void store(float* f) const { for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) f[4 * i + j] = c[i][j]; }
};
// glm type_mat4x4.inl operator*(mat4, mat4): Result[i] = A0*B[i][0] + A1*B[i][1] + A2*B[i][2] + A3*B[i][3]
inline mat4 operator*(const mat4& a, const mat4& b) {
    mat4 r;
    for (int i = 0; i < 4; ++i)
        r.c[i] = ((a.c[0] * b.c[i][0] + a.c[1] * b.c[i][1]) + a.c[2] * b.c[i][2]) + a.c[3] * b.c[i][3];
    return r;
}
// glm operator*(mat4, vec4): (m0*v0 + m1*v1) + (m2*v2 + m3*v3)
inline vec4 operator*(const mat4& m, const vec4& v) {
    vec4 add0 = m.c[0] * v[0] + m.c[1] * v[1];
    vec4 add1 = m.c[2] * v[2] + m.c[3] * v[3];
    return add0 + add1;
}
inline mat4 transpose(const mat4& m) {
    mat4 r;
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) r.c[i][j] = m.c[j][i];
    return r;
}
// glm compute_inverse<4,4> (func_matrix.inl), same expression order
inline mat4 inverse(const mat4& M) {
    auto m = [&](int i, int j) { return M.c[i][j]; };
    float Coef00 = m(2,2) * m(3,3) - m(3,2) * m(2,3);
    float Coef02 = m(1,2) * m(3,3) - m(3,2) * m(1,3);
    float Coef03 = m(1,2) * m(2,3) - m(2,2) * m(1,3);
    float Coef04 = m(2,1) * m(3,3) - m(3,1) * m(2,3);
    float Coef06 = m(1,1) * m(3,3) - m(3,1) * m(1,3);
    float Coef07 = m(1,1) * m(2,3) - m(2,1) * m(1,3);
    float Coef08 = m(2,1) * m(3,2) - m(3,1) * m(2,2);
    float Coef10 = m(1,1) * m(3,2) - m(3,1) * m(1,2);
    float Coef11 = m(1,1) * m(2,2) - m(2,1) * m(1,2);
    float Coef12 = m(2,0) * m(3,3) - m(3,0) * m(2,3);
    float Coef14 = m(1,0) * m(3,3) - m(3,0) * m(1,3);
    float Coef15 = m(1,0) * m(2,3) - m(2,0) * m(1,3);
    float Coef16 = m(2,0) * m(3,2) - m(3,0) * m(2,2);
    float Coef18 = m(1,0) * m(3,2) - m(3,0) * m(1,2);
    float Coef19 = m(1,0) * m(2,2) - m(2,0) * m(1,2);
    float Coef20 = m(2,0) * m(3,1) - m(3,0) * m(2,1);
    float Coef22 = m(1,0) * m(3,1) - m(3,0) * m(1,1);
    float Coef23 = m(1,0) * m(2,1) - m(2,0) * m(1,1);
    vec4 Fac0 = V4(Coef00, Coef00, Coef02, Coef03);
    vec4 Fac1 = V4(Coef04, Coef04, Coef06, Coef07);
    vec4 Fac2 = V4(Coef08, Coef08, Coef10, Coef11);
    vec4 Fac3 = V4(Coef12, Coef12, Coef14, Coef15);
    vec4 Fac4 = V4(Coef16, Coef16, Coef18, Coef19);
    vec4 Fac5 = V4(Coef20, Coef20, Coef22, Coef23);
    vec4 Vec0 = V4(m(1,0), m(0,0), m(0,0), m(0,0));
    vec4 Vec1 = V4(m(1,1), m(0,1), m(0,1), m(0,1));
    vec4 Vec2 = V4(m(1,2), m(0,2), m(0,2), m(0,2));
    vec4 Vec3 = V4(m(1,3), m(0,3), m(0,3), m(0,3));
    vec4 Inv0 = (Vec1 * Fac0 - Vec2 * Fac1) + Vec3 * Fac2;
    vec4 Inv1 = (Vec0 * Fac0 - Vec2 * Fac3) + Vec3 * Fac4;
    vec4 Inv2 = (Vec0 * Fac1 - Vec1 * Fac3) + Vec3 * Fac5;
    vec4 Inv3 = (Vec0 * Fac2 - Vec1 * Fac4) + Vec2 * Fac5;
    vec4 SignA = V4(+1.f, -1.f, +1.f, -1.f);
    vec4 SignB = V4(-1.f, +1.f, -1.f, +1.f);
    mat4 Inv;
    Inv.c[0] = Inv0 * SignA; Inv.c[1] = Inv1 * SignB; Inv.c[2] = Inv2 * SignA; Inv.c[3] = Inv3 * SignB;
    vec4 Row0 = V4(Inv.c[0][0], Inv.c[1][0], Inv.c[2][0], Inv.c[3][0]);
    vec4 Dot0 = M.c[0] * Row0;
    float Dot1 = (Dot0[0] + Dot0[1]) + (Dot0[2] + Dot0[3]);
    float One = 1.0f / Dot1;
    mat4 r;
    for (int i = 0; i < 4; ++i) r.c[i] = Inv.c[i] * One;
    return r;
}
// ModelOutput's matrix for normals
inline mat4 normal_matrix(const mat4& M) { return transpose(inverse(M)); }

}  // namespace pnglm
