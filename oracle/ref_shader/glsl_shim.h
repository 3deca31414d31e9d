// glsl_shim.h -- ORACLE-side vector header (test infrastructure, NOT product code).
//
// Lets a C++ compiler read the reference's fragment shaders after the textual rewrite of glsl2cpp.py.  The shaders' text supplies
// structure, operand order and indices; this header supplies what GLSL leaves open, each entry as DESIGN.md section 3 resolves it:
//   normalize(v) = v / sqrt((x*x + y*y) + z*z), normalize(0) = 0;  min / max = fminf / fmaxf;  atan / asin / exp = the oracle's
//   exported vo_atan2f / vo_asinf / vo_expf;  nearest + repeat texel = floor(fract(u) * n) clamped;  linear + clamp-to-edge =
//   the spec's bilinear, a coordinate within `snap` of a texel centre point-samples (rule K: integral tap offsets);  texture() of the
//   volume = texel rint(uvw * size), the inverse of vec3(pos) / vec3(bounds);  float -> int conversion saturates, NaN -> 0.
// Everything else is literal: component-wise operators are plain fp32 operations in the order written (0 * inf is NaN), every
// vector type value-initialises to zero, and uniform-block arrays read a byte buffer with a stride and yield 0 past its end.
// Compile with -O2 -ffp-contract=off -fno-fast-math, as the oracle.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

extern "C" {
float vo_atan2f(float y, float x);
float vo_asinf(float x);
float vo_expf(float x);
}

namespace glsl {

typedef unsigned int uint;

struct vec2; struct vec3; struct vec4;

// Swizzles live in a union with the components (GNU anonymous structs); reading converts, assigning writes through the named
// components only (also from a swizzle of the same type: `outColor.rgb = skyColor(d).rgb` must leave outColor.a alone, so the copy
// assignment is spelled out, and with it the vector types' own copies).
template <int N, int A, int B> struct swz2 {
    float v[N];
    operator vec2() const;
    swz2& operator=(const vec2& o);
    swz2& operator=(const swz2& o);
};
template <int N, int A, int B, int C> struct swz3 {
    float v[N];
    operator vec3() const;
    swz3& operator=(const vec3& o);
    swz3& operator=(const swz3& o);
};

struct ivec2 { int x, y; ivec2() : x(0), y(0) {} ivec2(int a, int b) : x(a), y(b) {} };
struct uvec2 { uint x, y; uvec2() : x(0), y(0) {} uvec2(uint a, uint b) : x(a), y(b) {} };
struct uvec3 { uint x, y, z; uvec3() : x(0), y(0), z(0) {} uvec3(uint a, uint b, uint c) : x(a), y(b), z(c) {} };
struct bvec3 { bool x, y, z; bvec3() : x(false), y(false), z(false) {} bvec3(bool a, bool b, bool c) : x(a), y(b), z(c) {} };
struct uvec4 {
    union { struct { uint x, y, z, w; }; struct { uint r, g, b, a; }; };
    uvec4() { x = y = z = w = 0; }
    uvec4(uint a_, uint b_, uint c_, uint d_) { x = a_; y = b_; z = c_; w = d_; }
};

struct vec2 {
    union { struct { float x, y; }; struct { float r, g; }; swz2<2, 0, 1> xy; };
    vec2() { x = y = 0.0f; }
    explicit vec2(float s) { x = y = s; }
    vec2(float a, float b) { x = a; y = b; }
    vec2(const ivec2& v) { x = (float)v.x; y = (float)v.y; }      // GLSL's implicit int -> float vector conversions
    vec2(const uvec2& v) { x = (float)v.x; y = (float)v.y; }
    vec2(const vec2& o) { x = o.x; y = o.y; }
    vec2& operator=(const vec2& o) { x = o.x; y = o.y; return *this; }
    vec2& operator+=(const vec2& o) { x = x + o.x; y = y + o.y; return *this; }
    vec2& operator*=(const vec2& o) { x = x * o.x; y = y * o.y; return *this; }
    vec2& operator+=(float s) { x = x + s; y = y + s; return *this; }
};

struct ivec3;

struct vec3 {
    union {
        struct { float x, y, z; }; struct { float r, g, b; };
        swz3<3, 0, 1, 2> xyz; swz3<3, 1, 2, 0> yzx; swz3<3, 2, 0, 1> zxy; swz3<3, 0, 1, 2> rgb; swz2<3, 0, 1> xy;
    };
    vec3() { x = y = z = 0.0f; }
    explicit vec3(float s) { x = y = z = s; }
    vec3(float a, float b, float c) { x = a; y = b; z = c; }
    vec3(const vec2& v, float c) { x = v.x; y = v.y; z = c; }
    vec3(const ivec3& v);
    vec3(const uvec3& v) { x = (float)v.x; y = (float)v.y; z = (float)v.z; }
    explicit vec3(const bvec3& v) { x = v.x ? 1.0f : 0.0f; y = v.y ? 1.0f : 0.0f; z = v.z ? 1.0f : 0.0f; }
    vec3(const vec3& o) { x = o.x; y = o.y; z = o.z; }
    vec3& operator=(const vec3& o) { x = o.x; y = o.y; z = o.z; return *this; }
    vec3& operator+=(const vec3& o) { x = x + o.x; y = y + o.y; z = z + o.z; return *this; }
};

struct vec4 {
    union {
        struct { float x, y, z, w; }; struct { float r, g, b, a; };
        swz3<4, 0, 1, 2> xyz; swz3<4, 0, 1, 2> rgb; swz2<4, 0, 1> xy;
    };
    vec4() { x = y = z = w = 0.0f; }
    explicit vec4(float s) { x = y = z = w = s; }
    vec4(float a_, float b_, float c_, float d_) { x = a_; y = b_; z = c_; w = d_; }
    vec4(const vec4& o) { x = o.x; y = o.y; z = o.z; w = o.w; }
    vec4& operator=(const vec4& o) { x = o.x; y = o.y; z = o.z; w = o.w; return *this; }
    vec4& operator+=(const vec4& o) { x = x + o.x; y = y + o.y; z = z + o.z; w = w + o.w; return *this; }
};

// float -> int as the GPU's conversion instruction does it: towards zero, saturating, NaN -> 0 (in C++ out of range is undefined)
inline int f2i(float f)
{
    if (f != f) return 0;
    if (f >= 2147483648.0f) return 2147483647;
    if (f <= -2147483648.0f) return -2147483647 - 1;
    return (int)f;
}

struct ivec3 {
    int x, y, z;
    ivec3() : x(0), y(0), z(0) {}
    ivec3(int a, int b, int c) : x(a), y(b), z(c) {}
    explicit ivec3(const vec3& v) : x(f2i(v.x)), y(f2i(v.y)), z(f2i(v.z)) {}
    ivec3& operator+=(const ivec3& o) { x += o.x; y += o.y; z += o.z; return *this; }
};
inline ivec3 operator*(const ivec3& a, const ivec3& b) { return ivec3(a.x * b.x, a.y * b.y, a.z * b.z); }

inline vec3::vec3(const ivec3& v) { x = (float)v.x; y = (float)v.y; z = (float)v.z; }

template <int N, int A, int B> swz2<N, A, B>::operator vec2() const { return vec2(v[A], v[B]); }
template <int N, int A, int B> swz2<N, A, B>& swz2<N, A, B>::operator=(const vec2& o) { v[A] = o.x; v[B] = o.y; return *this; }
template <int N, int A, int B> swz2<N, A, B>& swz2<N, A, B>::operator=(const swz2& o) { return *this = (vec2)o; }
template <int N, int A, int B, int C> swz3<N, A, B, C>& swz3<N, A, B, C>::operator=(const swz3& o) { return *this = (vec3)o; }
template <int N, int A, int B, int C> swz3<N, A, B, C>::operator vec3() const { return vec3(v[A], v[B], v[C]); }
template <int N, int A, int B, int C> swz3<N, A, B, C>& swz3<N, A, B, C>::operator=(const vec3& o)
{
    float a = o.x, b = o.y, c = o.z;
    v[A] = a; v[B] = b; v[C] = c;
    return *this;
}

// ---- component-wise operators, literal ---------------------------------------------------------------------------------------------
#define GLSL_OPS2(OP) \
    inline vec2 operator OP(const vec2& a, const vec2& b) { return vec2(a.x OP b.x, a.y OP b.y); } \
    inline vec2 operator OP(const vec2& a, float b) { return vec2(a.x OP b, a.y OP b); } \
    inline vec2 operator OP(float a, const vec2& b) { return vec2(a OP b.x, a OP b.y); }
#define GLSL_OPS3(OP) \
    inline vec3 operator OP(const vec3& a, const vec3& b) { return vec3(a.x OP b.x, a.y OP b.y, a.z OP b.z); } \
    inline vec3 operator OP(const vec3& a, float b) { return vec3(a.x OP b, a.y OP b, a.z OP b); } \
    inline vec3 operator OP(float a, const vec3& b) { return vec3(a OP b.x, a OP b.y, a OP b.z); }
#define GLSL_OPS4(OP) \
    inline vec4 operator OP(const vec4& a, const vec4& b) { return vec4(a.x OP b.x, a.y OP b.y, a.z OP b.z, a.w OP b.w); } \
    inline vec4 operator OP(const vec4& a, float b) { return vec4(a.x OP b, a.y OP b, a.z OP b, a.w OP b); } \
    inline vec4 operator OP(float a, const vec4& b) { return vec4(a OP b.x, a OP b.y, a OP b.z, a OP b.w); }
GLSL_OPS2(+) GLSL_OPS2(-) GLSL_OPS2(*) GLSL_OPS2(/)
GLSL_OPS3(+) GLSL_OPS3(-) GLSL_OPS3(*) GLSL_OPS3(/)
GLSL_OPS4(+) GLSL_OPS4(-) GLSL_OPS4(*) GLSL_OPS4(/)
#undef GLSL_OPS2
#undef GLSL_OPS3
#undef GLSL_OPS4
inline vec2 operator-(const vec2& a) { return vec2(-a.x, -a.y); }
inline vec3 operator-(const vec3& a) { return vec3(-a.x, -a.y, -a.z); }
inline vec4 operator-(const vec4& a) { return vec4(-a.x, -a.y, -a.z, -a.w); }

// ---- built-in functions -----------------------------------------------------------------------------------------------------------
inline float floor(float x) { return ::floorf(x); }
inline vec3 floor(const vec3& v) { return vec3(::floorf(v.x), ::floorf(v.y), ::floorf(v.z)); }
inline float abs(float x) { return ::fabsf(x); }
inline vec3 abs(const vec3& v) { return vec3(::fabsf(v.x), ::fabsf(v.y), ::fabsf(v.z)); }
inline float sign(float x) { return (float)((x > 0.0f) - (x < 0.0f)); }
inline vec3 sign(const vec3& v) { return vec3(sign(v.x), sign(v.y), sign(v.z)); }
inline float min(float a, float b) { return ::fminf(a, b); }
inline float max(float a, float b) { return ::fmaxf(a, b); }
inline vec3 min(const vec3& a, const vec3& b) { return vec3(::fminf(a.x, b.x), ::fminf(a.y, b.y), ::fminf(a.z, b.z)); }
inline vec3 max(const vec3& a, const vec3& b) { return vec3(::fmaxf(a.x, b.x), ::fmaxf(a.y, b.y), ::fmaxf(a.z, b.z)); }
inline float mod(float x, float y) { return x - y * ::floorf(x / y); }
inline vec3 mod(const vec3& v, float y) { return vec3(mod(v.x, y), mod(v.y, y), mod(v.z, y)); }
inline float dot(const vec3& a, const vec3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
inline float dot(const vec4& a, const vec4& b) { return ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w; }
inline float length(const vec3& v) { return ::sqrtf(dot(v, v)); }
inline vec3 normalize(const vec3& v)
{
    float l = length(v);
    if (l == 0.0f) return vec3();
    return vec3(v.x / l, v.y / l, v.z / l);
}
inline vec3 reflect(const vec3& I, const vec3& N) { return I - 2.0f * dot(N, I) * N; }
inline bvec3 lessThanEqual(const vec3& a, const vec3& b) { return bvec3(a.x <= b.x, a.y <= b.y, a.z <= b.z); }
inline float atan(float y, float x) { return vo_atan2f(y, x); }
inline float asin(float x) { return vo_asinf(x); }
inline float exp(float x) { return vo_expf(x); }

// ---- textures -----------------------------------------------------------------------------------------------------------------------
struct usampler3D { const uint8_t* data = nullptr; uint w = 0, h = 0, d = 0; };

inline uint texel3(float u, uint n)
{
    float t = ::rintf(u * (float)n);
    if (!(t >= 0.0f)) return 0;
    uint i = (uint)t;
    return i >= n ? n - 1 : i;
}
inline uvec4 texture(const usampler3D& s, const vec3& uvw)
{
    size_t x = texel3(uvw.x, s.w), y = texel3(uvw.y, s.h), z = texel3(uvw.z, s.d);
    return uvec4(s.data[x + (y + z * (size_t)s.h) * (size_t)s.w], 0, 0, 1);
}

enum { FMT_UNORM8 = 0, FMT_SNORM8 = 1, FMT_F32 = 2 };
enum { FILTER_NEAREST_REPEAT = 0, FILTER_LINEAR_CLAMP = 1 };
struct sampler2D {
    const void* data = nullptr; int w = 0, h = 0; int format = FMT_UNORM8; int filter = FILTER_NEAREST_REPEAT;
    float snap = 0.0f;                         // linear filter: |coordinate - texel centre| <= snap on both axes point-samples
};

inline vec4 texel2(const sampler2D& s, int x, int y)
{
    x = x < 0 ? 0 : (x > s.w - 1 ? s.w - 1 : x);
    y = y < 0 ? 0 : (y > s.h - 1 ? s.h - 1 : y);
    size_t i = ((size_t)y * (size_t)s.w + (size_t)x) * 4;
    vec4 r;
    if (s.format == FMT_F32) {
        const float* p = (const float*)s.data + i;
        r = vec4(p[0], p[1], p[2], p[3]);
    } else if (s.format == FMT_SNORM8) {
        const int8_t* p = (const int8_t*)s.data + i;
        r = vec4(::fmaxf((float)p[0] / 127.0f, -1.0f), ::fmaxf((float)p[1] / 127.0f, -1.0f),
                 ::fmaxf((float)p[2] / 127.0f, -1.0f), ::fmaxf((float)p[3] / 127.0f, -1.0f));
    } else {
        const uint8_t* p = (const uint8_t*)s.data + i;
        r = vec4((float)p[0] / 255.0f, (float)p[1] / 255.0f, (float)p[2] / 255.0f, (float)p[3] / 255.0f);
    }
    return r;
}
inline int wrap_texel(float u, int n)
{
    float fr = u - ::floorf(u);
    if (!(fr >= 0.0f)) return 0;
    int i = (int)::floorf(fr * (float)n);
    return i >= n ? n - 1 : i;
}
inline vec4 texture(const sampler2D& s, const vec2& uv)
{
    if (s.filter == FILTER_NEAREST_REPEAT) return texel2(s, wrap_texel(uv.x, s.w), wrap_texel(uv.y, s.h));
    float fx = uv.x * (float)s.w - 0.5f, fy = uv.y * (float)s.h - 0.5f;
    float rx = ::rintf(fx), ry = ::rintf(fy);
    if (::fabsf(fx - rx) <= s.snap && ::fabsf(fy - ry) <= s.snap) return texel2(s, f2i(rx), f2i(ry));
    float x0f = ::floorf(fx), y0f = ::floorf(fy);
    float tx = fx - x0f, ty = fy - y0f;
    int x0 = f2i(x0f), y0 = f2i(y0f);
    vec4 c00 = texel2(s, x0, y0), c10 = texel2(s, x0 + 1, y0), c01 = texel2(s, x0, y0 + 1), c11 = texel2(s, x0 + 1, y0 + 1);
    vec4 a = c00 + tx * (c10 - c00), b = c01 + tx * (c11 - c01);
    return a + ty * (b - a);
}

// ---- uniform-block arrays: a byte buffer read with a stride, 0 past its end --------------------------------------------------------
template <class T, int N> struct ubo_array {
    const unsigned char* data = nullptr; size_t size = 0, stride = sizeof(T);
    T operator[](unsigned long i) const
    {
        T v{};
        size_t o = (size_t)i * stride;
        if (data && o + sizeof(T) <= size) std::memcpy((void*)&v, data + o, sizeof(T));
        return v;
    }
};

static vec4 gl_FragCoord;

}  // namespace glsl
