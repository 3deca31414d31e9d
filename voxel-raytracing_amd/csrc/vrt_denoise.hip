// vrt_denoise.hip -- K3 for gfx950: the a-trous denoiser kernels and launch_denoise_pass.
#include "vrt_device_common.h"
#include <type_traits>

namespace vrt {

// ---------------------------------------------------------------------------------------------
// K3: a-trous denoiser pass
// ---------------------------------------------------------------------------------------------
//
// Same arithmetic as denoiser.frag:38-73 / the oracle, bit for bit, but with the work the values make
// unnecessary left out:
//   * UNORM8 / SNORM8 decode c/255, c/127: q0 = c*r, q = fma(fma(-D, q0, c), r, q0) with r = RN(1/D) equals the
//     IEEE quotient for every one of the 256 codes (checked exhaustively in tests/test_denoise_decode.py);
//     3 instructions instead of a ~12-instruction division sequence, 8 decodes per tap;
//   * pass 0 has phi = 1/0 * phi0 = +inf, so every edge-stopping weight is min(exp(-0), 1) = 1 exactly
//     (NaN / inf distances included: fminf ignores the NaN): the pass is specialised to a plain weighted blur;
//   * a distance of exactly 0 gives exp(-0) = 1 and a quotient below -87 gives exp = 0 (vrt_spec.h exp_spec):
//     neither needs the division + exponential; a zero weight makes the whole tap contribute +0.
// One wave = 64 consecutive pixels of a row (coalesced 256 B / 1 KiB accesses).

struct Guides { float c[4], n[4], p[4]; };


__device__ __forceinline__ void texel_guides(const DenoiseParams& P, int x, int y, Guides& g)
{
    x = x < 0 ? 0 : (x > P.W - 1 ? P.W - 1 : x);
    y = y < 0 ? 0 : (y > P.H - 1 ? P.H - 1 : y);
    size_t i = (size_t)y * (size_t)P.W + (size_t)x;
    uchar4 c = reinterpret_cast<const uchar4*>(P.color_in)[i];
    char4 n = reinterpret_cast<const char4*>(P.normal)[i];
    float4 p = reinterpret_cast<const float4*>(P.position)[i];
    g.c[0] = decode_unorm8(c.x); g.c[1] = decode_unorm8(c.y); g.c[2] = decode_unorm8(c.z); g.c[3] = decode_unorm8(c.w);
    g.n[0] = decode_snorm8(n.x); g.n[1] = decode_snorm8(n.y); g.n[2] = decode_snorm8(n.z); g.n[3] = decode_snorm8(n.w);
    g.p[0] = p.x; g.p[1] = p.y; g.p[2] = p.z; g.p[3] = p.w;
}

__device__ __forceinline__ void sample_guides(const DenoiseParams& P, int px, int py, float ox, float oy, Guides& g)
{
    if (ox == floorf(ox) && oy == floorf(oy)) { texel_guides(P, px + (int)ox, py + (int)oy, g); return; }
    float fx = ((float)px + 0.5f + ox) - 0.5f, fy = ((float)py + 0.5f + oy) - 0.5f;
    float x0f = floorf(fx), y0f = floorf(fy);
    float tx = fx - x0f, ty = fy - y0f;
    int x0 = (int)x0f, y0 = (int)y0f;
    Guides g00, g10, g01, g11;
    texel_guides(P, x0, y0, g00); texel_guides(P, x0 + 1, y0, g10);
    texel_guides(P, x0, y0 + 1, g01); texel_guides(P, x0 + 1, y0 + 1, g11);
    for (int k = 0; k < 4; k++) {
        float a, b;
        a = g00.c[k] + tx * (g10.c[k] - g00.c[k]); b = g01.c[k] + tx * (g11.c[k] - g01.c[k]); g.c[k] = a + ty * (b - a);
        a = g00.n[k] + tx * (g10.n[k] - g00.n[k]); b = g01.n[k] + tx * (g11.n[k] - g01.n[k]); g.n[k] = a + ty * (b - a);
        a = g00.p[k] + tx * (g10.p[k] - g00.p[k]); b = g01.p[k] + tx * (g11.p[k] - g01.p[k]); g.p[k] = a + ty * (b - a);
    }
}

__device__ __forceinline__ float dist2_4(const float* a, const float* b)
{
    float t0 = a[0] - b[0], t1 = a[1] - b[1], t2 = a[2] - b[2], t3 = a[3] - b[3];
    return ((t0 * t0 + t1 * t1) + t2 * t2) + t3 * t3;
}

// min(exp(-(d2)/phi), 1) (denoiser.frag:55,60,65) for a finite phi > 0, skipping the division and the exponential
// when the value of d2 already decides the result.
__device__ __forceinline__ float edge_weight(float d2, float phi)
{
    if (d2 == 0.0f) return 1.0f;                      // (-0)/phi = -0, exp(-0) = 1
    float x = (-d2) / phi;
    if (x < -87.0f) return 0.0f;                      // exp_spec's own cut-off
    return fminf(exp_spec(x), 1.0f);
}

// One pixel of a pass, the shader's own way (denoiser.frag:38-73 tap by tap): the body of k_denoise.
template <bool PHI_INF>
__device__ __forceinline__ uchar4 denoise_pixel(const DenoiseParams& P, int px, int py)
{
    const bool shipped = (P.mode & 1) == VRT_DENOISE_AS_SHIPPED;
    const int ntaps = shipped ? 3 : 9;
    float sw = P.step_width;
    float sw2 = sw * sw;
    Guides s, o;
    texel_guides(P, px, py, s);
    float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float total = 0.0f;
    for (int i = 0; i < ntaps; i++) {
        int tx, ty; float kern;
        if (shipped) {        // std140 aliasing: taps (-1,-1)*G2, (1,-1)*G0, (0,0)*G2
            tx = i == 0 ? -1 : (i == 1 ? 1 : 0); ty = i == 2 ? 0 : -1;
            kern = i == 1 ? kGauss0 : kGauss2;
        } else {
            tx = i % 3 - 1; ty = i / 3 - 1;
            int r2 = tx * tx + ty * ty;
            kern = r2 == 0 ? kGauss0 : (r2 == 1 ? kGauss1 : kGauss2);
        }
        sample_guides(P, px, py, (float)tx * sw, (float)ty * sw, o);
        float w = 1.0f;
        if (!PHI_INF) {
            float pw = edge_weight(dist2_4(s.p, o.p), P.phi_pos);
            float cw = 1.0f, nw = 1.0f;
            if (pw != 0.0f) {                         // a zero factor makes w = +0 whatever the other two are (all finite)
                cw = edge_weight(dist2_4(s.c, o.c), P.phi_color);
                float dn = dist2_4(s.n, o.n);
                nw = dn == 0.0f ? 1.0f : edge_weight(fmaxf(dn / sw2, 0.0f), P.phi_normal);
            }
            w = (cw * nw) * pw;
        }
        for (int k = 0; k < 4; k++) sum[k] += (o.c[k] * w) * kern;
        total += w * kern;
    }
    uchar4 out;
    out.x = unorm8(sum[0] / total); out.y = unorm8(sum[1] / total);
    out.z = unorm8(sum[2] / total); out.w = unorm8(sum[3] / total);
    return out;
}

// One TAP of a weighted pass with an integral tap offset R, the shader's own way: the tap's weight (cw * nw) * pw and its
// colour texel (k_denoise_ver's redone pixels: nine lanes share a pixel, one tap each, so that a pixel costs one tap's
// chain of dependent instructions instead of nine; the sums are then taken by one lane in the shader's order).  The
// arithmetic is denoise_pixel<false>'s, operation for operation.
__device__ __forceinline__ float guides_tap_weight(float phi_color, float phi_normal, float phi_pos, float sw, const Guides& s, const Guides& o)
{
    const float sw2 = sw * sw;
    float pw = edge_weight(dist2_4(s.p, o.p), phi_pos);
    float cw = 1.0f, nw = 1.0f;
    if (pw != 0.0f) {
        cw = edge_weight(dist2_4(s.c, o.c), phi_color);
        float dn = dist2_4(s.n, o.n);
        nw = dn == 0.0f ? 1.0f : edge_weight(fmaxf(dn / sw2, 0.0f), phi_normal);
    }
    return (cw * nw) * pw;
}
__device__ __forceinline__ float denoise_tap_weight(const DenoiseParams& P, int px, int py, int tx, int ty, int R, uint32_t& color)
{
    Guides s, o;
    texel_guides(P, px + tx * R, py + ty * R, o);         // (both texels requested before either is used)
    texel_guides(P, px, py, s);
    {
        int x = px + tx * R, y = py + ty * R;
        x = x < 0 ? 0 : (x > P.W - 1 ? P.W - 1 : x);
        y = y < 0 ? 0 : (y > P.H - 1 ? P.H - 1 : y);
        color = reinterpret_cast<const uint32_t*>(P.color_in)[(size_t)y * (size_t)P.W + (size_t)x];
    }
    return guides_tap_weight(P.phi_color, P.phi_normal, P.phi_pos, P.step_width, s, o);
}

template <bool PHI_INF>
__global__ __launch_bounds__(256) void k_denoise(const DenoiseParams P)
{
    int px = blockIdx.x * 64 + (threadIdx.x & 63);
    int r = blockIdx.y * 4 + (threadIdx.x >> 6);
    // (the launch rounds the rows up to blocks of 4: a row past the last local strip's is no row of this rank, though strip_row, which
    // does not know the strip count, may find the extension of the next strip of its stride inside the frame)
    if (r >= P.sh.n_local_strips * (P.sh.strip_rows + 2 * P.extend)) return;
    int py = strip_row(P.sh, P.extend, r, P.H);
    if (py < 0 || px >= P.W) return;
    reinterpret_cast<uchar4*>(P.color_out)[(size_t)py * (size_t)P.W + (size_t)px] = denoise_pixel<PHI_INF>(P, px, py);
}

typedef float v2f __attribute__((ext_vector_type(2)));

// ---- the exact weights of TWO taps at a time, without branches -------------------------------------------------------------
// The weighted pass is bound by instruction issue (two Cephes exponentials and two correctly rounded divisions per channel
// and tap, behind data-dependent shortcuts whose short EXEC-masked blocks cost as much as they save).  Every shortcut of
// edge_weight() is the value the long way round gives anyway -- exp_spec(-0) = 1 exactly, a factor 0 makes the product +0 --
// so the long way round, for two taps at once in the two halves of packed fp32 instructions (v_pk_mul / v_pk_add / v_pk_fma:
// the same IEEE operations element-wise, never contracted), is the same arithmetic: 12 packed exponentials per pixel
// instead of 27 scalar ones.

// RN(a / b) element-wise for a pass-uniform b with r = RN(1 / b): q0 = a r and two residual corrections -- the core of the
// compiler's own IEEE division sequence (which refines an approximate reciprocal to within an ulp, multiplies, and corrects
// twice), without its range scaling: exact while no intermediate leaves the normal range, i.e. for b in [2^-20, 2^20] (the
// host checks) and a = 0 or a in [2^-90, 2^90] (the caller checks; decoded 8-bit guides cannot leave it).
__device__ __forceinline__ v2f div_uniform2(v2f a, float b, float r)
{
    const v2f nb = {-b, -b}, rr = {r, r};
    v2f q = a * rr;
    q = __builtin_elementwise_fma(__builtin_elementwise_fma(nb, q, a), rr, q);
    q = __builtin_elementwise_fma(__builtin_elementwise_fma(nb, q, a), rr, q);
    return q;
}

// min(exp_spec(-q), 1) element-wise for q >= 0 (vrt_spec.h exp_spec, operation for operation)
__device__ __forceinline__ v2f edge_weight2(v2f q)
{
    const v2f x0 = -q;
    const v2f fx = __builtin_elementwise_floor(x0 * 1.44269504088896341f + 0.5f);
    v2f x = x0 - fx * 0.693359375f;
    x = x - fx * -2.12194440e-4f;
    const v2f z = x * x;
    const v2f p = (((((1.9875691500e-4f * x + 1.3981999507e-3f) * x + 8.3334519073e-3f) * x
                     + 4.1665795894e-2f) * x + 1.6666665459e-1f) * x + 5.0000001201e-1f) * z + x + 1.0f;
    const int n0 = (int)fx.x, n1 = (int)fx.y;
    const v2f sc = {__uint_as_float(((uint32_t)n0 + 127u) << 23), __uint_as_float(((uint32_t)n1 + 127u) << 23)};
    const v2f e = p * sc;
    v2f w;
    w.x = x0.x < -87.0f ? 0.0f : fminf(e.x, 1.0f);
    w.y = x0.y < -87.0f ? 0.0f : fminf(e.y, 1.0f);
    return w;
}

// |a - b|^2 in the order of dist2_4, the two halves of each float4 in one packed instruction
__device__ __forceinline__ float dist2_4pk(const float4& a, const float4& b)
{
    const v2f t01 = (v2f){a.x, a.y} - (v2f){b.x, b.y}, t23 = (v2f){a.z, a.w} - (v2f){b.z, b.w};
    const v2f q01 = t01 * t01, q23 = t23 * t23;
    return ((q01.x + q01.y) + q23.x) + q23.y;
}

// LDS-tiled form for integral stepWidth: a workgroup owns 64x4 pixels; the guides of that tile plus a halo of
// R = stepWidth pixels are fetched, decoded ONCE and parked in LDS as three float4 planes (48 B per pixel), so each
// pixel's guides are read from HBM/L2 once per pass instead of once per tap that lands on it (9x), and the 8-bit
// decodes are not repeated per tap.  Same arithmetic on the same decoded values as k_denoise.
template <bool PHI_INF, bool SHIPPED, bool FAST = false, bool PACKED = false>
__global__ __launch_bounds__(256) void k_denoise_lds(const DenoiseParams P, int R)
{
    extern __shared__ __attribute__((aligned(16))) float4 lds_g[];
    const int RW = 64 + 2 * R, RH = 4 + 2 * R, NP = RW * RH;
    float4* lc = lds_g; float4* ln = lds_g + NP; float4* lp = lds_g + 2 * NP;
    const int x0 = blockIdx.x * 64, r0 = blockIdx.y * 4;
    // rows of one block are consecutive frame rows (checked by the launcher); a single rank owns every row in order
    const bool whole = P.sh.nranks == 1 && P.extend == 0;
    // Sharded: the four rows of a block lie in one extended strip (per % 4 == 0), but the strip's first `extend` rows
    // do not exist above the top of the frame (and its last ones may not below the bottom), so the block's frame row
    // is taken from its first row that exists -- not from row r0, which for extend % 4 == 2 is missing while r0 + 2
    // and r0 + 3 are frame rows 0 and 1.  y0 may be negative; the staging clamps and the row test below masks.
    int y0 = -1;
    bool any_row = false;
    if (whole) { y0 = r0; any_row = r0 < P.H; }
    else {
#pragma unroll
        for (int k = 3; k >= 0; k--) {
            const int yk = strip_row(P.sh, P.extend, r0 + k, P.H);
            if (yk >= 0) { y0 = yk - k; any_row = true; }
        }
    }
    if (!any_row) return;
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    // staging: texel t = threadIdx.x + 256 k of the haloed tile, k = 0, 1, ... -- every thread gets the same number of
    // texels (+-1); (cx, cy) = (t % RW, t / RW) is kept without divisions: RW is 66..74, so threadIdx.x / RW is 0..3
    {
        const int t0 = (int)threadIdx.x;
        int cy = (t0 >= RW ? 1 : 0) + (t0 >= 2 * RW ? 1 : 0) + (t0 >= 3 * RW ? 1 : 0);
        int cx = t0 - cy * RW;
        const int dy = 256 >= 3 * RW + RW ? 4 : 3;             // 256 / RW (RW <= 64: 4 never happens; RW in 66..74: 3)
        const int dx = 256 - dy * RW;
        for (int t = t0; t < NP; t += 256) {
            int x = x0 - R + cx, y = y0 - R + cy;
            x = x < 0 ? 0 : (x > P.W - 1 ? P.W - 1 : x);
            y = y < 0 ? 0 : (y > P.H - 1 ? P.H - 1 : y);
            const size_t i = (size_t)y * (size_t)P.W + (size_t)x;
            const uchar4 c = reinterpret_cast<const uchar4*>(P.color_in)[i];
            lc[t] = make_float4(decode_unorm8(c.x), decode_unorm8(c.y), decode_unorm8(c.z), decode_unorm8(c.w));
            if (!PHI_INF) {                                   // pass 0 weighs every tap 1: only the colour is ever read
                const char4 n = reinterpret_cast<const char4*>(P.normal)[i];
                ln[t] = make_float4(decode_snorm8(n.x), decode_snorm8(n.y), decode_snorm8(n.z), decode_snorm8(n.w));
                lp[t] = reinterpret_cast<const float4*>(P.position)[i];
            }
            cx += dx; cy += dy;
            if (cx >= RW) { cx -= RW; cy++; }
        }
    }
    __syncthreads();
    const int px = x0 + lx, py = y0 + ly;
    if (px >= P.W || py < 0 || py >= P.H) return;
    if (!whole && strip_row(P.sh, P.extend, r0 + ly, P.H) != py) return;   // above / past the end of the strip or frame

    constexpr int ntaps = SHIPPED ? 3 : 9;
    const float sw = P.step_width, sw2 = sw * sw;
    const int c0 = (ly + R) * RW + (lx + R);
    const float4 sc = lc[c0], sn = PHI_INF ? sc : ln[c0], sp = PHI_INF ? sc : lp[c0];
    const float s_c[4] = {sc.x, sc.y, sc.z, sc.w}, s_n[4] = {sn.x, sn.y, sn.z, sn.w}, s_p[4] = {sp.x, sp.y, sp.z, sp.w};
    float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float total = 0.0f;
    const int rowoff = R * RW;
    if constexpr (PACKED && !PHI_INF && !FAST) {
        // taps in the shader's order, two at a time; the centre tap (all three distances are 0 or NaN: every weight is 1)
        // between them where the order has it
        v2f s01 = {0.0f, 0.0f}, s23 = {0.0f, 0.0f};
        constexpr int npairs = SHIPPED ? 1 : 4;
#pragma unroll 1
        for (int j = 0; j < npairs; j++) {
            int ta, tb; float ka, kb;                          // tap offsets (in units of R, relative to c0) and kernel weights
            if (SHIPPED) { ta = -rowoff - R; tb = -rowoff + R; ka = kGauss2; kb = kGauss0; }
            else if (j == 0) { ta = -rowoff - R; tb = -rowoff; ka = kGauss2; kb = kGauss1; }
            else if (j == 1) { ta = -rowoff + R; tb = -R; ka = kGauss2; kb = kGauss1; }
            else if (j == 2) { ta = R; tb = rowoff - R; ka = kGauss1; kb = kGauss2; }
            else { ta = rowoff; tb = rowoff + R; ka = kGauss1; kb = kGauss2; }
            if (!SHIPPED && j == 2) {                          // tap 4, the centre: w = 1, kern = 1
                s01 += (v2f){sc.x, sc.y}; s23 += (v2f){sc.z, sc.w};
                total += 1.0f;
            }
            const float4 oca = lc[c0 + ta], ocb = lc[c0 + tb], opa = lp[c0 + ta], opb = lp[c0 + tb], ona = ln[c0 + ta], onb = ln[c0 + tb];
            const v2f dp = {dist2_4pk(sp, opa), dist2_4pk(sp, opb)};
            const v2f dc = {dist2_4pk(sc, oca), dist2_4pk(sc, ocb)};
            const v2f dn = {dist2_4pk(sn, ona), dist2_4pk(sn, onb)};
            // positions are the caller's floats: a distance outside the range the short division is exact for (tiny, huge,
            // inf, NaN) sends the wave through edge_weight() for this pair
            const uint32_t ua = __float_as_uint(dp.x), ub = __float_as_uint(dp.y);
            const bool odd = (ua != 0u && ua - 0x12800000u > 0x6C800000u - 0x12800000u) || (ub != 0u && ub - 0x12800000u > 0x6C800000u - 0x12800000u);
            v2f w;
            if (__builtin_expect(__ballot(odd) != 0ull, 0)) {
                const float pa = edge_weight(dp.x, P.phi_pos), pb = edge_weight(dp.y, P.phi_pos);
                float ca = 1.0f, na = 1.0f, cb = 1.0f, nb = 1.0f;
                if (pa != 0.0f) { ca = edge_weight(dc.x, P.phi_color); na = dn.x == 0.0f ? 1.0f : edge_weight(fmaxf(dn.x / sw2, 0.0f), P.phi_normal); }
                if (pb != 0.0f) { cb = edge_weight(dc.y, P.phi_color); nb = dn.y == 0.0f ? 1.0f : edge_weight(fmaxf(dn.y / sw2, 0.0f), P.phi_normal); }
                w = (v2f){(ca * na) * pa, (cb * nb) * pb};
            } else {
                // a channel in which all 64 pixels agree with both their taps (sky: every position is 0; a flat wall: one
                // normal) has weight exp(-0) = 1 throughout: one compare and a branch the whole wave takes or not
                const v2f one = {1.0f, 1.0f};
                v2f pw = one, cw = one, nw = one;
                if (__ballot((ua | ub) != 0u) != 0ull) pw = edge_weight2(div_uniform2(dp, P.phi_pos, P.rp));
                if (__ballot((__float_as_uint(dc.x) | __float_as_uint(dc.y)) != 0u) != 0ull) cw = edge_weight2(div_uniform2(dc, P.phi_color, P.rc));
                if (__ballot((__float_as_uint(dn.x) | __float_as_uint(dn.y)) != 0u) != 0ull)
                    nw = edge_weight2(div_uniform2(div_uniform2(dn, sw2, P.rs), P.phi_normal, P.rn));
                w = (cw * nw) * pw;
            }
            s01 += ((v2f){oca.x, oca.y} * w.x) * ka; s23 += ((v2f){oca.z, oca.w} * w.x) * ka; total += w.x * ka;
            s01 += ((v2f){ocb.x, ocb.y} * w.y) * kb; s23 += ((v2f){ocb.z, ocb.w} * w.y) * kb; total += w.y * kb;
        }
        if (SHIPPED) {                                         // tap 2, the centre: w = 1, kern = G2
            s01 += (v2f){sc.x, sc.y} * kGauss2; s23 += (v2f){sc.z, sc.w} * kGauss2;
            total += kGauss2;
        }
        sum[0] = s01.x; sum[1] = s01.y; sum[2] = s23.x; sum[3] = s23.y;
    } else {
    // pass 0 unrolls into nine LDS reads and 72 multiply-adds; the weighted taps stay a loop (unrolled they need 72
    // VGPRs and 14 KB of code, and measured 7 % slower)
    constexpr int kUnroll = PHI_INF ? 9 : 1;
#pragma unroll kUnroll
    for (int i = 0; i < ntaps; i++) {
        int tx, ty; float kern;
        if (SHIPPED) {
            tx = i == 0 ? -1 : (i == 1 ? 1 : 0); ty = i == 2 ? 0 : -1;
            kern = i == 1 ? kGauss0 : kGauss2;
        } else {
            tx = i % 3 - 1; ty = i / 3 - 1;
            int r2 = tx * tx + ty * ty;
            kern = r2 == 0 ? kGauss0 : (r2 == 1 ? kGauss1 : kGauss2);
        }
        const int ci = c0 + ty * rowoff + tx * R;
        const float4 oc = lc[ci];
        const float o_c[4] = {oc.x, oc.y, oc.z, oc.w};
        float w = 1.0f;
        if (!PHI_INF && FAST) {
            // the product of the three weights as one exponential (each argument is <= 0, so no factor exceeds 1 and the
            // shader's min(., 1) has nothing to do): three multiply-adds and one v_exp_f32 instead of three divisions and
            // three polynomial exponentials
            const float4 op = lp[ci], on = ln[ci];
            const float o_p[4] = {op.x, op.y, op.z, op.w}, o_n[4] = {on.x, on.y, on.z, on.w};
            // (a NaN position distance -- NaN or inf - inf -- weighs 1 in the shader, fminf(exp(NaN), 1): its term of the one exponent is 0)
            const float e = __builtin_fmaf(fmaxf(dist2_4(s_p, o_p), 0.0f), P.kp, __builtin_fmaf(dist2_4(s_c, o_c), P.kc, fmaxf(dist2_4(s_n, o_n), 0.0f) * P.kn));
            w = __builtin_amdgcn_exp2f(-e);
        } else if (!PHI_INF) {
            const float4 op = lp[ci];
            const float o_p[4] = {op.x, op.y, op.z, op.w};
            float pw = edge_weight(dist2_4(s_p, o_p), P.phi_pos);
            float cw = 1.0f, nw = 1.0f;
            if (pw != 0.0f) {
                const float4 on = ln[ci];
                const float o_n[4] = {on.x, on.y, on.z, on.w};
                cw = edge_weight(dist2_4(s_c, o_c), P.phi_color);
                float dn = dist2_4(s_n, o_n);
                nw = dn == 0.0f ? 1.0f : edge_weight(fmaxf(dn / sw2, 0.0f), P.phi_normal);
            }
            w = (cw * nw) * pw;
        }
        for (int k = 0; k < 4; k++) sum[k] += (o_c[k] * w) * kern;
        total += w * kern;
    }
    }
    uchar4 out;
    if (PHI_INF) {
        // sums are 0 or >= 1/255 * 0.77 and total is the fixed sum of the tap weights (3.3 .. 7.7): no operand or
        // quotient of these four divisions is anywhere near the range where the IEEE sequence rescales, so its core --
        // reciprocal refined once, then two residual corrections per quotient -- can share the reciprocal (23 VALU
        // ops instead of 40) and still round every quotient correctly
        const float r0 = __builtin_amdgcn_rcpf(total);
        const float r = __builtin_fmaf(__builtin_fmaf(-total, r0, 1.0f), r0, r0);
        float q[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float q0 = sum[k] * r;
            float q1 = __builtin_fmaf(__builtin_fmaf(-total, q0, sum[k]), r, q0);
            q[k] = __builtin_fmaf(__builtin_fmaf(-total, q1, sum[k]), r, q1);
        }
        out.x = unorm8(q[0]); out.y = unorm8(q[1]); out.z = unorm8(q[2]); out.w = unorm8(q[3]);
    } else if (FAST) {
        const float r = __builtin_amdgcn_rcpf(total);
        out.x = unorm8(sum[0] * r); out.y = unorm8(sum[1] * r); out.z = unorm8(sum[2] * r); out.w = unorm8(sum[3] * r);
    } else {
        out.x = unorm8(sum[0] / total); out.y = unorm8(sum[1] / total);
        out.z = unorm8(sum[2] / total); out.w = unorm8(sum[3] / total);
    }
    reinterpret_cast<uchar4*>(P.color_out)[(size_t)py * (size_t)P.W + (size_t)px] = out;
}

// VRT_DENOISE_FAST on a whole frame (one rank, integral stepWidth, a weighted pass): a workgroup owns 64 x TH pixels, four rows
// at a time per wave, so that the guides of the tile + halo are fetched and decoded once for TH rows instead of four (a
// halo of R = 3 rows above and below makes a 4-row tile read 2.5x its own rows, a 16-row tile 1.4x); the weights are one
// hardware exponential per tap (see VRT_DENOISE_FAST in vrt.h).
// |a - b|^2 of two float4 in packed fp32 operations (v_pk_add / v_pk_mul / v_pk_fma: two lanes' worth per instruction);
// fused and re-associated -- the fast mode states a tolerance, not a rounding
__device__ __forceinline__ float dist2_pk(const float4& a, const float4& b)
{
    const v2f d0 = (v2f){a.x, a.y} - (v2f){b.x, b.y}, d1 = (v2f){a.z, a.w} - (v2f){b.z, b.w};
    const v2f q = __builtin_elementwise_fma(d1, d1, d0 * d0);
    return q.x + q.y;
}

__device__ __forceinline__ constexpr int r2_of(int tx, int ty) { return tx * tx + ty * ty; }
// as-shipped taps: (-1,-1) * G2, (1,-1) * G0, (0,0) * G2
__device__ __forceinline__ constexpr float shipped_lk(int i) { return i == 1 ? 0.0f : 0.36067376022224085f; }

template <bool SHIPPED, int TH>
__global__ __launch_bounds__(256) void k_denoise_fast(const DenoiseParams P, int R)
{
    extern __shared__ __attribute__((aligned(16))) float4 lds_g[];
    const int RW = 64 + 2 * R, RH = TH + 2 * R, NP = RW * RH;
    float4* lc = lds_g; float4* ln = lds_g + NP; float4* lp = lds_g + 2 * NP;
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * TH;
    {
        int cy = (int)threadIdx.x / RW, cx = (int)threadIdx.x - cy * RW;       // (RW >= 66: cy is 0..3)
        const int dy = 256 / RW, dx = 256 - dy * RW;
        for (int t = (int)threadIdx.x; t < NP; t += 256) {
            int x = x0 - R + cx, y = y0 - R + cy;
            x = x < 0 ? 0 : (x > P.W - 1 ? P.W - 1 : x);
            y = y < 0 ? 0 : (y > P.H - 1 ? P.H - 1 : y);
            const size_t i = (size_t)y * (size_t)P.W + (size_t)x;
            const uchar4 c = reinterpret_cast<const uchar4*>(P.color_in)[i];
            const char4 n = reinterpret_cast<const char4*>(P.normal)[i];
            // the CODES as floats (SNORM -128 = -127): 1/255 and 1/127 ride in the distances' scale factors, and the output is a
            // mean of codes already
            lc[t] = make_float4((float)c.x, (float)c.y, (float)c.z, (float)c.w);
            ln[t] = make_float4(fmaxf((float)n.x, -127.0f), fmaxf((float)n.y, -127.0f), fmaxf((float)n.z, -127.0f), fmaxf((float)n.w, -127.0f));
            lp[t] = reinterpret_cast<const float4*>(P.position)[i];
            cx += dx; cy += dy;
            if (cx >= RW) { cx -= RW; cy++; }
        }
    }
    __syncthreads();
    const int lx = threadIdx.x & 63, px = x0 + lx;
    if (px >= P.W) return;
    constexpr int ntaps = SHIPPED ? 3 : 9;
    const int rowoff = R * RW;
    const float kc = P.kc * (1.0f / (255.0f * 255.0f)), kn = P.kn * (1.0f / (127.0f * 127.0f));
    for (int ly = (int)(threadIdx.x >> 6); ly < TH; ly += 4) {
        const int py = y0 + ly;
        if (py >= P.H) break;
        const int c0 = (ly + R) * RW + (lx + R);
        const float4 sc = lc[c0], sn = ln[c0], sp = lp[c0];
        v2f s01 = {0.0f, 0.0f}, s23 = {0.0f, 0.0f};
        float total = 0.0f;
#pragma unroll
        for (int i = 0; i < ntaps; i++) {
            int tx, ty; float kern;
            if (SHIPPED) {
                tx = i == 0 ? -1 : (i == 1 ? 1 : 0); ty = i == 2 ? 0 : -1;
                kern = i == 1 ? kGauss0 : kGauss2;
            } else {
                tx = i % 3 - 1; ty = i / 3 - 1;
                const int r2 = tx * tx + ty * ty;
                kern = r2 == 0 ? kGauss0 : (r2 == 1 ? kGauss1 : kGauss2);
            }
            if (tx == 0 && ty == 0) {                            // the centre tap: every distance is 0, its weight is the kernel's
                s01 += (v2f){sc.x, sc.y} * kern; s23 += (v2f){sc.z, sc.w} * kern; total += kern;
                continue;
            }
            const int ci = c0 + ty * rowoff + tx * R;
            const float4 oc = lc[ci], op = lp[ci], on = ln[ci];
            // the kernel weight rides in the exponent: w * kern = exp2(-(e - log2 kern))
            const float lk = r2_of(tx, ty) == 0 ? 0.0f : (r2_of(tx, ty) == 1 ? 0.18033688011112042f : 0.36067376022224085f);   // -log2(G1), -log2(G2)
            // (a NaN position distance -- NaN or inf - inf -- weighs 1 in the shader, fminf(exp(NaN), 1): its term of the one exponent is 0)
            const float e = __builtin_fmaf(fmaxf(dist2_pk(sp, op), 0.0f), P.kp, __builtin_fmaf(dist2_pk(sc, oc), kc, __builtin_fmaf(dist2_pk(sn, on), kn, SHIPPED ? shipped_lk(i) : lk)));
            const float wk = __builtin_amdgcn_exp2f(-e);
            const v2f w2 = {wk, wk};
            s01 = __builtin_elementwise_fma((v2f){oc.x, oc.y}, w2, s01);
            s23 = __builtin_elementwise_fma((v2f){oc.z, oc.w}, w2, s23);
            total += wk;
        }
        const float r = __builtin_amdgcn_rcpf(total);
        // a weighted mean of codes: round half up, clamp (the weights are positive, the mean cannot leave 0..255 by more than rounding)
        uchar4 out;
        out.x = (uint8_t)fminf(floorf(fmaf(s01.x, r, 0.5f)), 255.0f); out.y = (uint8_t)fminf(floorf(fmaf(s01.y, r, 0.5f)), 255.0f);
        out.z = (uint8_t)fminf(floorf(fmaf(s23.x, r, 0.5f)), 255.0f); out.w = (uint8_t)fminf(floorf(fmaf(s23.y, r, 0.5f)), 255.0f);
        reinterpret_cast<uchar4*>(P.color_out)[(size_t)py * (size_t)P.W + (size_t)px] = out;
    }
}

#define VRT_DEN_FIXCAP 1024
// The listed pixels of a workgroup, the shader's own way (k_denoise_ver, k_denoise_pair): nine lanes per listed pixel, a tap
// each (denoise_tap_weight); then four of them a channel each, the sums in the shader's order.  More flagged than the list holds -- hostile
// input -- or `all`: every pixel of the segment instead (columns xo .. xo + ow - 1, rows ys .. ye - 1; pixels that were sure get
// the value they already have).  Called by every thread of the workgroup, behind the barrier that made n and the list final.
template <bool SHIPPED, bool PASS0>
__device__ __forceinline__ void denoise_redo(const DenoiseParams& P, int R, uint32_t n, bool all, int xo, int ow, int ys, int ye,
                                             const uint32_t* fl_px, float (*fx_w)[9], uint32_t (*fx_c)[9], uint32_t first = 0u)
{
    constexpr int ntaps = SHIPPED ? 3 : 9;
    const bool overflow = all || n > VRT_DEN_FIXCAP;
    const uint32_t entries = overflow ? 64u * (uint32_t)(ye - ys) : n;
    const bool shipped = SHIPPED;
    // nine lanes per listed pixel: a tap each (denoise_tap_weight), then four of them a channel each -- the sums in the shader's order
    const uint32_t per = blockDim.x / 9u, grp = threadIdx.x / 9u;          // pixels per round (fx_w, fx_c hold that many)
    const int tap = (int)(threadIdx.x - grp * 9u);
    int tx, ty;
    if (shipped) { tx = tap == 0 ? -1 : (tap == 1 ? 1 : 0); ty = tap == 2 ? 0 : -1; }
    else { tx = tap % 3 - 1; ty = tap / 3 - 1; }
    for (uint32_t base = overflow ? 0u : first; base < entries; base += per) {        // (`first`: entries below it have been done)
        const uint32_t e = base + grp;
        bool live = grp < per && e < entries;
        uint32_t idx = 0u;
        if (live) {
            if (overflow) { const uint32_t qx = (uint32_t)xo + (e & 63u); live = (int)(e & 63u) < ow && qx < (uint32_t)P.W; idx = (uint32_t)(ys + (int)(e >> 6)) * (uint32_t)P.W + qx; }
            else idx = fl_px[e];
        }
        const int py = (int)(idx / (uint32_t)P.W), qx = (int)(idx - (uint32_t)py * (uint32_t)P.W);
        if (live && tap < ntaps) {
            uint32_t col;
            float w = 1.0f;
            if (PASS0) {
                int x = qx + tx * R, y = py + ty * R;
                x = x < 0 ? 0 : (x > P.W - 1 ? P.W - 1 : x);
                y = y < 0 ? 0 : (y > P.H - 1 ? P.H - 1 : y);
                col = reinterpret_cast<const uint32_t*>(P.color_in)[(size_t)y * (size_t)P.W + (size_t)x];
            } else w = denoise_tap_weight(P, qx, py, tx, ty, R, col);
            fx_w[grp][tap] = w; fx_c[grp][tap] = col;
        }
        __syncthreads();
        if (live && tap < 4) {                                   // channel `tap` of the pixel
            float sum = 0.0f, total = 0.0f;
#pragma unroll
            for (int i = 0; i < ntaps; i++) {
                float kern;
                if (shipped) kern = i == 1 ? kGauss0 : kGauss2;
                else { const int ux = i % 3 - 1, uy = i / 3 - 1, r2 = ux * ux + uy * uy; kern = r2 == 0 ? kGauss0 : (r2 == 1 ? kGauss1 : kGauss2); }
                const float w = fx_w[grp][i];
                const float oc = decode_unorm8((fx_c[grp][i] >> (8 * tap)) & 0xFFu);
                sum += (oc * w) * kern;
                total += w * kern;
            }
            P.color_out[(size_t)idx * 4u + (size_t)tap] = unorm8(sum / total);
        }
        __syncthreads();
    }
}

// ---- the verified pass -----------------------------------------------------------------------------------------------------
// vrt_denoise_bound.h: of a weighted pass only floor(mean * 255 + 0.5) is ever seen.  This kernel computes the mean cheaply --
// code distances as exact integers (three v_dot4_u32_u8: |a - b|^2 = a.a + b.b - 2 a.b over the four bytes of a texel; normals
// biased by 128, which differences do not see), the three edge-stopping weights and the kernel weight as ONE hardware
// exponential, fused accumulation, a reciprocal -- and every pixel one of whose channels lies within P.guard codes of a
// rounding boundary (NaN included: the comparison fails) is evaluated once more at the end, the shader's own way
// (denoise_pixel), by the workgroup that found it.  What the kernel leaves in color_out is the exact kernels' output bit for
// bit (tests/test_gpu_denoise.py).  FLAG = false is VRT_DENOISE_FAST: the same arithmetic, nothing redone (<= 1 code away).
//
// A workgroup owns a column strip of 64 pixels and `seg_rows` rows of it and walks DOWN the strip four rows at a time (one row
// per wave) through a ring of rows in LDS -- position 16 B, colour and (biased) normal codes 8 B per texel --: while a group
// of rows is being filtered the four rows the next group adds are already on their way from memory into registers, and go
// into the ring slots of the four rows the group no longer needs.  A texel is fetched once per strip and segment (1.1 - 1.3x
// the planes, against 1.9x for 64 x 8 tiles with their halo), the fetch latency hides under the arithmetic, and the launch is
// ONE round of workgroups that all end together.  RT: the tap offset at compile time (LDS offsets become immediates), 0: any.
// u - 2 v (a shift and a subtraction).  Not as v_mad_i32_i24 through inline assembly: the result of a v_dot4 may not be read by
// another vector instruction for three wait states on gfx950, and only instructions the compiler knows get their s_nops -- an
// asm block here read stale registers; the compiler's own 24-bit multiply-add sign-extends first and is three instructions.
__device__ __forceinline__ int mad24_minus2(uint32_t v, uint32_t u) { return (int)(u - 2u * v); }
template <bool SHIPPED, bool FLAG, int RT, bool PASS0 = false>
__global__ __launch_bounds__(256) void k_denoise_ver(const DenoiseParams P, int Rrt, int seg_rows, int segs_per_strip)
{
    extern __shared__ __attribute__((aligned(16))) float4 lds_g[];
    __shared__ uint32_t fl_n, fl_w4;
    __shared__ uint32_t fl_px[FLAG ? VRT_DEN_FIXCAP : 1];
    __shared__ float fx_w[FLAG ? 28 : 1][9];
    __shared__ uint32_t fx_c[FLAG ? 28 : 1][9];
#ifdef VRT_K3_STAMPS
    // (development build, tools/exp_k3_timeline.py: a workgroup's start / ring filled / rows done / end on the 100 MHz clock, written
    // over the first words of color_out when it ends -- the image is garbage)
    uint32_t k3_t[4] = {(uint32_t)wall_clock64(), 0u, 0u, 0u};
    auto k3_stamp = [&]() {
        if (threadIdx.x == 0) {
            uint32_t* o = reinterpret_cast<uint32_t*>(P.color_out) + 4u * (blockIdx.y * gridDim.x + blockIdx.x);
            o[0] = k3_t[0]; o[1] = k3_t[1]; o[2] = k3_t[2]; o[3] = (uint32_t)wall_clock64();
        }
    };
#endif
    const int R = RT ? RT : Rrt;
    const int RW = 64 + 2 * R;
    const int U = (4 + 2 * R + 3) / 4;                    // units of four rows a group of four output rows reads
    const int NR = 4 * (U + 1);                           // ring: those + the unit on its way in
    float4* lp = lds_g; uint2* lq = reinterpret_cast<uint2*>(lds_g + NR * RW);
    uint32_t* lc = reinterpret_cast<uint32_t*>(lds_g);      // PASS0 (phi = +inf, every weight exactly 1): the ring holds the colour codes only
    // the rows of this workgroup: segment j of the rank's local strip k, the strip taken with the `extend` rows either side that
    // this pass must also produce (strip_row's rows; one rank: the one strip is the frame)
    const int x0 = blockIdx.x * 64;
    int ys, ye;
    {
        const int k = (int)blockIdx.y / segs_per_strip, j = (int)blockIdx.y - k * segs_per_strip;
        const int g = k * P.sh.nranks + P.sh.rank;
        int r0 = g * P.sh.strip_rows - P.extend, r1 = (g + 1) * P.sh.strip_rows;
        r1 = (r1 < P.H ? r1 : P.H) + P.extend;
        r0 = r0 < 0 ? 0 : r0; r1 = r1 < P.H ? r1 : P.H;
        ys = r0 + j * seg_rows;
        ye = ys + seg_rows < r1 ? ys + seg_rows : r1;
    }
    if (ys >= ye) return;                                 // uniform per workgroup (a strip's last segment may be empty)
    const int groups = (ye - ys + 3) >> 2;
    if (threadIdx.x == 0) { fl_n = 0u; fl_w4 = 0u; }
    __syncthreads();
    // a thread's two texels of a unit (4 * RW <= 512 of them): row in the unit, clamped frame column
    const int tA = (int)threadIdx.x, tB = tA + 256;
    const int rA = tA / RW, cA = tA - rA * RW, rB = tB / RW, cB = tB - rB * RW;
    const bool hasB = tB < 4 * RW;
    int xA = x0 - R + cA, xB = x0 - R + cB;
    xA = xA < 0 ? 0 : (xA > P.W - 1 ? P.W - 1 : xA);
    xB = xB < 0 ? 0 : (xB > P.W - 1 ? P.W - 1 : xB);
    const uint32_t* const gc = reinterpret_cast<const uint32_t*>(P.color_in);
    const uint32_t* const gn = reinterpret_cast<const uint32_t*>(P.normal);
    const float4* const gp = reinterpret_cast<const float4*>(P.position);
    float4 pA = make_float4(0.0f, 0.0f, 0.0f, 0.0f), pB = pA;
    uint32_t colA, nrmA = 0u, colB = 0u, nrmB = 0u;
    auto fetch = [&](int unit) {                           // unit u = relative rows 4u .. 4u + 3 = frame rows ys - R + 4u ...
        int yA = ys - R + 4 * unit + rA, yB = ys - R + 4 * unit + rB;
        yA = yA < 0 ? 0 : (yA > P.H - 1 ? P.H - 1 : yA);
        yB = yB < 0 ? 0 : (yB > P.H - 1 ? P.H - 1 : yB);
        const uint32_t iA = (uint32_t)yA * (uint32_t)P.W + (uint32_t)xA, iB = (uint32_t)yB * (uint32_t)P.W + (uint32_t)xB;
        if (PASS0) { colA = gc[iA]; if (hasB) colB = gc[iB]; return; }
        pA = gp[iA]; colA = gc[iA]; nrmA = gn[iA];
        if (hasB) { pB = gp[iB]; colB = gc[iB]; nrmB = gn[iB]; }
    };
    auto bias = [](uint32_t n) {
        // SNORM code -128 decodes like -127 (max(c / 127, -1)): bytes 0x80 become 0x81; then every byte biased by 128
        uint32_t z = n ^ 0x80808080u;                                                   // bytes that were 0x80 are 0 now
        z = ~(((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z | 0x7F7F7F7Fu);                     // 0x80 exactly in those bytes
        return (n | (z >> 7)) ^ 0x80808080u;
    };
    auto stash = [&](int unit) {
        const int slot = (unit % (U + 1)) * 4;
        // (a colour alpha or a position w other than +-0: the rows take their general form from the next barrier on)
        if (((colA | colB) >> 24) != 0u || ((__float_as_uint(pA.w) | __float_as_uint(pB.w)) << 1) != 0u) fl_w4 = 1u;
        if (PASS0) { lc[(slot + rA) * RW + cA] = colA; if (hasB) lc[(slot + rB) * RW + cB] = colB; return; }
        lp[(slot + rA) * RW + cA] = pA; lq[(slot + rA) * RW + cA] = make_uint2(colA, bias(nrmA));
        if (hasB) { lp[(slot + rB) * RW + cB] = pB; lq[(slot + rB) * RW + cB] = make_uint2(colB, bias(nrmB)); }
    };
    {
        // the first U units (U <= 4), all requested before the first is stored: one round trip to memory, not U (every workgroup
        // of the launch stands here at the same time: nothing else hides them)
        float4 qpA[4], qpB[4]; uint32_t qcA[4], qnA[4], qcB[4], qnB[4];
#pragma unroll
        for (int u = 0; u < 4; u++) if (u < U) { fetch(u); qpA[u] = pA; qpB[u] = pB; qcA[u] = colA; qnA[u] = nrmA; qcB[u] = colB; qnB[u] = nrmB; }
#pragma unroll
        for (int u = 0; u < 4; u++) if (u < U) { pA = qpA[u]; pB = qpB[u]; colA = qcA[u]; nrmA = qnA[u]; colB = qcB[u]; nrmB = qnB[u]; stash(u); }
    }
    __syncthreads();

#ifdef VRT_K3_STAMPS
    k3_t[1] = (uint32_t)wall_clock64();
#endif
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lx = threadIdx.x & 63, px = x0 + lx;
    constexpr int ntaps = SHIPPED ? 3 : 9;
    const float kc = P.vkc, kn = P.vkn, kp = P.vkp;
    const float half_guard = 0.5f - P.guard;
    // One output row of a wave.  W4 = false: no texel in the ring has a colour alpha or a position w other than 0 (what K1 writes,
    // SURVEY 9.4-F): the fourth channel's sums and the fourth difference are +0 whatever the weights are -- the same values
    // without the instructions (a texel that has one raises fl_w4 when it is stored into the ring, before its first use).
    auto row = [&](auto w4_tag, int yr, int py, uint32_t& out_codes, uint32_t& out_idx, bool& out_sure) {
        constexpr bool W4 = decltype(w4_tag)::value;
        const int b0 = (yr % NR) * RW + lx, b1 = ((yr + R) % NR) * RW + lx, b2 = ((yr + 2 * R) % NR) * RW + lx;   // column of tap tx = -1
        uint2 sq; float4 sp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (PASS0) sq = make_uint2(lc[b1 + R], 0u); else { sq = lq[b1 + R]; sp = lp[b1 + R]; }
        const uint32_t scc = PASS0 ? 0u : __builtin_amdgcn_udot4(sq.x, sq.x, 0u, false), snn = PASS0 ? 0u : __builtin_amdgcn_udot4(sq.y, sq.y, 0u, false);
        constexpr float kcen = SHIPPED ? kGauss2 : kGauss0;
        float a0 = (float)(sq.x & 0xFFu) * kcen, a1 = (float)((sq.x >> 8) & 0xFFu) * kcen, a2 = (float)((sq.x >> 16) & 0xFFu) * kcen, a3 = W4 ? (float)(sq.x >> 24) * kcen : 0.0f;
        float total = kcen;
#pragma unroll
        for (int i = 0; i < ntaps; i++) {
            int tx, ty;
            if (SHIPPED) { tx = i == 0 ? -1 : (i == 1 ? 1 : 0); ty = i == 2 ? 0 : -1; }
            else { tx = i % 3 - 1; ty = i / 3 - 1; }
            if (tx == 0 && ty == 0) continue;                // the centre tap: every distance is 0, its weight is the kernel's (above)
            const int ci = (ty < 0 ? b0 : (ty == 0 ? b1 : b2)) + (tx + 1) * R;
            if (PASS0) {                                     // every edge-stopping weight is exactly 1: the tap's weight is the kernel's
                const uint32_t oc = lc[ci];
                const float kk = SHIPPED ? (i == 1 ? kGauss0 : kGauss2) : (r2_of(tx, ty) == 1 ? kGauss1 : kGauss2);
                a0 = __builtin_fmaf((float)(oc & 0xFFu), kk, a0);
                a1 = __builtin_fmaf((float)((oc >> 8) & 0xFFu), kk, a1);
                a2 = __builtin_fmaf((float)((oc >> 16) & 0xFFu), kk, a2);
                if (W4) a3 = __builtin_fmaf((float)(oc >> 24), kk, a3);
                continue;
            }
            const uint2 oq = lq[ci];
            const float4 op = lp[ci];
            const int dc = mad24_minus2(__builtin_amdgcn_udot4(sq.x, oq.x, 0u, false), __builtin_amdgcn_udot4(oq.x, oq.x, scc, false));
            const int dn = mad24_minus2(__builtin_amdgcn_udot4(sq.y, oq.y, 0u, false), __builtin_amdgcn_udot4(oq.y, oq.y, snn, false));
            const float dx = sp.x - op.x, dy = sp.y - op.y, dz = sp.z - op.z;
            float dp = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
            if (W4) { const float dw = sp.w - op.w; dp = __builtin_fmaf(dw, dw, dp); }
            if (!FLAG) dp = fmaxf(dp, 0.0f);                 // VRT_DENOISE_FAST, nothing redone: a NaN distance weighs 1, as in the shader's fminf(exp(NaN), 1)
            // the kernel weight rides in the exponent: w * kern = exp2(-(e + -log2 kern))
            const float lk = SHIPPED ? shipped_lk(i) : (r2_of(tx, ty) == 1 ? 0.18033688011112042f : 0.36067376022224085f);
            const float e = __builtin_fmaf(dp, kp, __builtin_fmaf((float)dc, kc, __builtin_fmaf((float)dn, kn, lk)));
            const float wk = __builtin_amdgcn_exp2f(-e);
            a0 = __builtin_fmaf((float)(oq.x & 0xFFu), wk, a0);
            a1 = __builtin_fmaf((float)((oq.x >> 8) & 0xFFu), wk, a1);
            a2 = __builtin_fmaf((float)((oq.x >> 16) & 0xFFu), wk, a2);
            if (W4) a3 = __builtin_fmaf((float)(oq.x >> 24), wk, a3);
            total += wk;
        }
        // (PASS0: the weights' sum is a constant; its reciprocal rounded once from double)
        const float r = PASS0 ? (SHIPPED ? (float)(1.0 / (2.0 * 0.7788007830714049 + 1.0)) : (float)(1.0 / (1.0 + 4.0 * 0.8824969025845955 + 4.0 * 0.7788007830714049))) : __builtin_amdgcn_rcpf(total);
        // a weighted mean of codes, + 0.5: its floor is the output, its fraction says how far the nearest rounding boundary is
        const float y0f = __builtin_fmaf(a0, r, 0.5f), y1f = __builtin_fmaf(a1, r, 0.5f), y2f = __builtin_fmaf(a2, r, 0.5f);
        const float f0 = __builtin_amdgcn_fractf(y0f), f1 = __builtin_amdgcn_fractf(y1f), f2 = __builtin_amdgcn_fractf(y2f);
        // (the truncation is the floor -- the means are positive -- and cannot pass 255: a mean of codes with positive weights is at most
        // 255 (1 + 20 eps), + 0.5; a NaN converts to 0 and is redone anyway)
        const uint32_t o0 = (uint32_t)y0f, o1 = (uint32_t)y1f, o2 = (uint32_t)y2f;
        // sure <=> every channel's fraction lies further than the guard from 0 and from 1 (a NaN mean compares false)
        bool sure = !FLAG || (__builtin_fabsf(f0 - 0.5f) < half_guard && __builtin_fabsf(f1 - 0.5f) < half_guard && __builtin_fabsf(f2 - 0.5f) < half_guard);
        uint32_t o3 = 0u;                                        // (W4 = false: the mean of zeros is 0, half a code from either boundary)
        if (W4) {
            const float y3f = __builtin_fmaf(a3, r, 0.5f), f3 = __builtin_amdgcn_fractf(y3f);
            o3 = (uint32_t)y3f;
            if (FLAG) sure = sure && __builtin_fabsf(f3 - 0.5f) < half_guard;
        }
        out_codes = o0 | (o1 << 8) | (o2 << 16) | (o3 << 24); out_idx = (uint32_t)py * (uint32_t)P.W + (uint32_t)px; out_sure = sure;
    };
    for (int g = 0; g < groups; g++) {
        const bool more = g + 1 < groups;
#ifdef VRT_VER_PRIO
        // (a wave's priority falls as it gets on: see k_denoise_pair)
        if (4 * g < groups) __builtin_amdgcn_s_setprio(3); else if (2 * g < groups) __builtin_amdgcn_s_setprio(2);
        else if (4 * g < 3 * groups) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0);
#endif
        if (more) fetch(g + U);                                  // the unit group g + 1 adds: in flight while group g is filtered
        const int yr = 4 * g + wave, py = ys + yr;               // relative row of the output; its taps' rows are yr, yr + R, yr + 2R in ring terms
        const bool have = py < ye && px < P.W;
        uint32_t out_codes = 0u, out_idx = 0u;
        bool out_sure = true;
        const bool w4 = fl_w4 != 0u;                             // (uniform: read after the barrier that follows every store into the ring)
        if (have) {
            if (w4) row(std::true_type{}, yr, py, out_codes, out_idx, out_sure);
            else    row(std::false_type{}, yr, py, out_codes, out_idx, out_sure);
        }
        // (the ring first, the output after it: the wait for the fetched unit would otherwise also wait for this group's store
        // -- on gfx950 one counter covers both -- once per group, with nothing left to hide it)
        if (more) stash(g + U);                                  // into the slots of the unit group g no longer reads
        if (have) {
            if (out_sure) reinterpret_cast<uint32_t*>(P.color_out)[out_idx] = out_codes;
            else if (FLAG) { const uint32_t slot = atomicAdd(&fl_n, 1u); if (slot < VRT_DEN_FIXCAP) fl_px[slot] = out_idx; }
        }
        __syncthreads();
    }
#ifdef VRT_K3_STAMPS
    k3_t[2] = (uint32_t)wall_clock64();
#endif
    if (FLAG) {
        // (the loop's last barrier is behind us: fl_n and fl_px are final)
        const uint32_t n = fl_n;
#ifdef VRT_K3_STAMPS
        if (n == 0u) { __syncthreads(); k3_stamp(); return; }
#endif
        if (n == 0u) return;                                     // uniform per workgroup
        if (P.fix_counts && threadIdx.x == 0) atomicAdd(&P.fix_counts[(blockIdx.y * gridDim.x + blockIdx.x) & (VRT_DENOISE_SEGS - 1u)], n);
        denoise_redo<SHIPPED, PASS0>(P, R, n, false, x0, 64, ys, ye, fl_px, fx_w, fx_c);
    }
#ifdef VRT_K3_STAMPS
    __syncthreads(); k3_stamp();
#endif
}

// ---- the verified pass, every weight computed once (round 4) ---------------------------------------------------------------
// The weight of a tap is symmetric: w(p, q) = w(q, p) -- integer code distances, squares of differences, the same kernel weight
// for d and -d -- bit for bit in the arithmetic above.  Of the eight taps of a pixel p the four "forward" ones (1, 0), (-1, 1),
// (0, 1), (1, 1) are computed by p's lane; the four "backward" ones are forward weights of the pixels R to the left / R rows
// above.  A workgroup is R waves and a group of rows is R rows, one per wave, so that the row R above a wave's row is the row
// the SAME wave did one group earlier: its three downward weights are still in registers (the one straight above stays in its
// lane, the diagonal ones come through the crossbar, ds_bpermute), and the weight of the tap to the left is this row's own
// (1, 0) of the lane R to the left.  Four exponentials per pixel instead of eight, no weight ever in memory; in exchange R rows
// above every segment only compute downward weights and a wave's 64 lanes are 64 columns of which the inner 64 - 2 R produce
// output.  The ring holds a texel as position x, y, z + the biased normal codes (16 B) and the four colour codes as halves
// (8 B): exact in fp16, so the colour distance is four v_dot2_f32_f16 (integers below 2^24: exact in fp32 in any order) and a
// tap's colour goes into the sums by v_fma_mix_f32 without a conversion.  The sums are taken in the order of k_denoise_ver
// (centre, then taps 0 .. 8): the output is that kernel's bit for bit, redone pixels and all.  The position's w has a plane of its
// own in the ring, read only once a texel with a w other than +-0 or a colour alpha has been met (K1 writes neither).
typedef _Float16 v2h __attribute__((ext_vector_type(2)));
#ifndef VRT_PAIR_FIXCAP
#define VRT_PAIR_FIXCAP 256     // listed pixels of a workgroup (of <= 58 x ~30): a few are listed, 2 % of a hostile frame; more: all of them redone
#endif
template <bool FLAG, int R>
__global__ __launch_bounds__(64 * R) void k_denoise_pair(const DenoiseParams P, int seg_rows, int segs_per_strip)
{
    extern __shared__ __attribute__((aligned(16))) float4 lds_g[];
    __shared__ uint32_t fl_n, fl_w4;
    __shared__ uint32_t fl_px[VRT_PAIR_FIXCAP];
    __shared__ float fx_w[(64 * R) / 9][9];
    __shared__ uint32_t fx_c[(64 * R) / 9][9];
#ifdef VRT_K3_STAMPS
    uint32_t k3_t[4] = {(uint32_t)wall_clock64(), 0u, 0u, 0u};
    uint32_t k3_redo = 0u;                                // (time inside the in-loop redo rounds; the stamp "ring filled" is moved back by it)
    auto k3_stamp = [&]() {
        if (threadIdx.x == 0) {
            uint32_t* o = reinterpret_cast<uint32_t*>(P.color_out) + 4u * (blockIdx.y * gridDim.x + blockIdx.x);
            o[0] = k3_t[0]; o[1] = k3_t[1] + k3_redo; o[2] = k3_t[2]; o[3] = (uint32_t)wall_clock64();
        }
    };
#endif
    constexpr int OW = 64 - 2 * R;                        // output columns of a strip
    constexpr int UT = R * 64;                            // texels of a unit of R rows
    constexpr int NT = 4 * UT;                            // ring: four units (three that a group reads + the one on its way in)
    float4* lp = lds_g;                                   // x, y, z, biased normal codes
    uint2* lh = reinterpret_cast<uint2*>(lds_g + NT);     // colour codes as four halves
    float* lw = reinterpret_cast<float*>(lh + NT);        // position w (read by the general form of a row only)
    const int x0 = blockIdx.x * OW;                       // first output column; lane l is column x0 - R + l
    int ys, ye;
    {
        const int k = (int)blockIdx.y / segs_per_strip, j = (int)blockIdx.y - k * segs_per_strip;
        const int g = k * P.sh.nranks + P.sh.rank;
        int r0 = g * P.sh.strip_rows - P.extend, r1 = (g + 1) * P.sh.strip_rows;
        r1 = (r1 < P.H ? r1 : P.H) + P.extend;
        r0 = r0 < 0 ? 0 : r0; r1 = r1 < P.H ? r1 : P.H;
        ys = r0 + j * seg_rows;
        ye = ys + seg_rows < r1 ? ys + seg_rows : r1;
    }
    if (ys >= ye) return;                                 // uniform per workgroup
    const int nrows = ye - ys;
    const int groups = (nrows + 2 * R - 1) / R;           // centre rows f = 0 .. nrows + R - 1 in ring terms (ring row 0 = frame row ys - R)
    if (threadIdx.x == 0) { fl_n = 0u; fl_w4 = 0u; }
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int l = threadIdx.x & 63, px = x0 - R + l;
    // a lane's texel, the texel R to its left, the texel R to its right within this wave's row of a unit (the ends are never used)
    const int tl = wave * 64 + l, tL = wave * 64 + (l - R < 0 ? 0 : l - R), tR = wave * 64 + (l + R > 63 ? 63 : l + R);
    const int bL = (l - R < 0 ? 0 : l - R) << 2, bR = (l + R > 63 ? 63 : l + R) << 2;      // the same lanes for ds_bpermute
    // a thread's texel of a unit: row `wave` of the unit, its own column (clamped to the frame: the ring holds copies of the border)
    const uint32_t xA = (uint32_t)(px < 0 ? 0 : (px > P.W - 1 ? P.W - 1 : px));
    const uint32_t* const gc = reinterpret_cast<const uint32_t*>(P.color_in);
    const uint32_t* const gn = reinterpret_cast<const uint32_t*>(P.normal);
    const float4* const gp = reinterpret_cast<const float4*>(P.position);
    float4 pA = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint32_t colA = 0u, nrmA = 0u;
    auto fetch = [&](int unit) {                           // (the row is the wave's: a scalar base and the lane's column)
        int yA = ys - R + R * unit + wave;
        yA = yA < 0 ? 0 : (yA > P.H - 1 ? P.H - 1 : yA);
        const size_t ro = (size_t)yA * (size_t)P.W;
        pA = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(gp + ro) + xA * 16u);
        colA = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(gc + ro) + xA * 4u);
        nrmA = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(gn + ro) + xA * 4u);
    };
    auto bias = [](uint32_t n) {                          // (k_denoise_ver's: SNORM -128 reads as -127, then every byte + 128)
        uint32_t z = n ^ 0x80808080u;
        z = ~(((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z | 0x7F7F7F7Fu);
        return (n | (z >> 7)) ^ 0x80808080u;
    };
    auto stash = [&](int slot) {
        const int i = slot * UT + tl;
        // (a colour alpha or a position w other than +-0: the rows take their general form from the next barrier on)
        if ((colA >> 24) != 0u || (__float_as_uint(pA.w) << 1) != 0u) fl_w4 = 1u;
        // codes as halves: 1024 + c is 0x6400 | c in fp16, exactly; minus 1024
        const v2h k1024 = {(_Float16)1024.0f, (_Float16)1024.0f};
        const v2h c01 = __builtin_bit_cast(v2h, __builtin_amdgcn_perm(colA, 0x64646464u, 0x00050004u)) - k1024;
        const v2h c23 = __builtin_bit_cast(v2h, __builtin_amdgcn_perm(colA, 0x64646464u, 0x00070006u)) - k1024;
        lp[i] = make_float4(pA.x, pA.y, pA.z, __uint_as_float(bias(nrmA)));
        lh[i] = make_uint2(__builtin_bit_cast(uint32_t, c01), __builtin_bit_cast(uint32_t, c23));
#ifndef VRT_PAIR_NOLW
        lw[i] = pA.w;
#endif
    };
    {
        fetch(0);                                          // (both requested before the first is stored: one round trip)
        const float4 qp = pA; const uint32_t qc = colA, qn = nrmA;
        fetch(1);
        const float4 rp = pA; const uint32_t rcol = colA, rn = nrmA;
        pA = qp; colA = qc; nrmA = qn; stash(0);
        pA = rp; colA = rcol; nrmA = rn; stash(1);
    }
    __syncthreads();
#ifdef VRT_K3_STAMPS
    k3_t[1] = (uint32_t)wall_clock64();
#endif
    const float kc = P.vkc, kn = P.vkn, kp = P.vkp;
    const float half_guard = 0.5f - P.guard;
    float pf1 = 0.0f, pf2 = 0.0f, pf3 = 0.0f;             // the downward weights (-1, 1), (0, 1), (1, 1) of this wave's row of the group before
    // One centre row of a wave -- in ring slot S, the row below it in slot S + 1, the row above in slot S - 1 --: the forward
    // weights of its 64 texels, and (`outrow`: it is a row of the segment) the pixel.
    auto row = [&](auto w4_tag, auto s_tag, bool outrow, int py, uint32_t& out_codes, uint32_t& out_idx, bool& out_sure) {
        constexpr bool W4 = decltype(w4_tag)::value;
        constexpr int rc = decltype(s_tag)::value * UT, rf = ((decltype(s_tag)::value + 1) & 3) * UT, rb = ((decltype(s_tag)::value + 3) & 3) * UT;
        const float4 s4 = lp[rc + tl];
        const uint2 sh = lh[rc + tl];
        const v2h s01 = __builtin_bit_cast(v2h, sh.x), s23 = __builtin_bit_cast(v2h, sh.y);
        const v2h m01 = s01 * (_Float16)(-2.0f), m23 = s23 * (_Float16)(-2.0f);            // -2 s: |s - o|^2 = |s|^2 + |o|^2 + (-2 s) . o
        const uint32_t sn = __float_as_uint(s4.w);
        const float sw = W4 ? lw[rc + tl] : 0.0f;
        const float scc = __builtin_amdgcn_fdot2(s01, s01, __builtin_amdgcn_fdot2(s23, s23, 0.0f, false), false);
        const uint32_t snn = __builtin_amdgcn_udot4(sn, sn, 0u, false);
        float wf[4]; uint2 hf[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int ci = k == 0 ? rc + tR : (k == 1 ? rf + tL : (k == 2 ? rf + tl : rf + tR));
            const float4 o4 = lp[ci];
            const uint2 oh = lh[ci];
            hf[k] = oh;
            const v2h o01 = __builtin_bit_cast(v2h, oh.x), o23 = __builtin_bit_cast(v2h, oh.y);
            const uint32_t on = __float_as_uint(o4.w);
            // integers below 2^24 at every step: exact
            const float dc = __builtin_amdgcn_fdot2(m23, o23, __builtin_amdgcn_fdot2(m01, o01, __builtin_amdgcn_fdot2(o23, o23, __builtin_amdgcn_fdot2(o01, o01, scc, false), false), false), false);
            const int dn = mad24_minus2(__builtin_amdgcn_udot4(sn, on, 0u, false), __builtin_amdgcn_udot4(on, on, snn, false));
            const float dx = s4.x - o4.x, dy = s4.y - o4.y, dz = s4.z - o4.z;
            float dp = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
            if (W4) { const float dw = sw - lw[ci]; dp = __builtin_fmaf(dw, dw, dp); }
            if (!FLAG) dp = fmaxf(dp, 0.0f);                 // VRT_DENOISE_FAST, nothing redone: a NaN distance weighs 1, as in the shader's fminf(exp(NaN), 1)
            const float lk = (k == 0 || k == 2) ? 0.18033688011112042f : 0.36067376022224085f;      // -log2(G1), -log2(G2)
            const float e = __builtin_fmaf(dp, kp, __builtin_fmaf(dc, kc, __builtin_fmaf((float)dn, kn, lk)));
            wf[k] = __builtin_amdgcn_exp2f(-e);
        }
        // the backward taps: (-1, -1) is the (1, 1) of the texel R left and R up, (0, -1) the (0, 1) of the texel R up, (1, -1) the
        // (-1, 1) of the texel R right and R up, (-1, 0) the (1, 0) of the texel R to the left
        const float w0 = __int_as_float(__builtin_amdgcn_ds_bpermute(bL, __float_as_int(pf3)));
        const float w1 = pf2;
        const float w2 = __int_as_float(__builtin_amdgcn_ds_bpermute(bR, __float_as_int(pf1)));
        const float w3 = __int_as_float(__builtin_amdgcn_ds_bpermute(bL, __float_as_int(wf[0])));
        pf1 = wf[1]; pf2 = wf[2]; pf3 = wf[3];
        if (!outrow) return;
        const uint2 h0 = lh[rb + tL], h1 = lh[rb + tl], h2 = lh[rb + tR], h3 = lh[rc + tL];
        constexpr float kcen = kGauss0;
        float a0 = (float)s01.x * kcen, a1 = (float)s01.y * kcen, a2 = (float)s23.x * kcen, a3 = W4 ? (float)s23.y * kcen : 0.0f;
        float total = kcen;
        auto acc = [&](const uint2& h, float wk) {
            const v2h c01 = __builtin_bit_cast(v2h, h.x), c23 = __builtin_bit_cast(v2h, h.y);
            a0 = __builtin_fmaf((float)c01.x, wk, a0);
            a1 = __builtin_fmaf((float)c01.y, wk, a1);
            a2 = __builtin_fmaf((float)c23.x, wk, a2);
            if (W4) a3 = __builtin_fmaf((float)c23.y, wk, a3);
            total += wk;
        };
        acc(h0, w0); acc(h1, w1); acc(h2, w2); acc(h3, w3);              // taps 0 .. 3
        acc(hf[0], wf[0]); acc(hf[1], wf[1]); acc(hf[2], wf[2]); acc(hf[3], wf[3]);   // taps 5 .. 8
        const float r = __builtin_amdgcn_rcpf(total);
        const float y0f = __builtin_fmaf(a0, r, 0.5f), y1f = __builtin_fmaf(a1, r, 0.5f), y2f = __builtin_fmaf(a2, r, 0.5f);
        const float f0 = __builtin_amdgcn_fractf(y0f), f1 = __builtin_amdgcn_fractf(y1f), f2 = __builtin_amdgcn_fractf(y2f);
        const uint32_t o0 = (uint32_t)y0f, o1 = (uint32_t)y1f, o2 = (uint32_t)y2f;
        bool sure = !FLAG || (__builtin_fabsf(f0 - 0.5f) < half_guard && __builtin_fabsf(f1 - 0.5f) < half_guard && __builtin_fabsf(f2 - 0.5f) < half_guard);
        uint32_t o3 = 0u;
        if (W4) {
            const float y3f = __builtin_fmaf(a3, r, 0.5f), f3 = __builtin_amdgcn_fractf(y3f);
            o3 = (uint32_t)y3f;
            if (FLAG) sure = sure && __builtin_fabsf(f3 - 0.5f) < half_guard;
        }
        out_codes = o0 | (o1 << 8) | (o2 << 16) | (o3 << 24); out_idx = (uint32_t)py * (uint32_t)P.W + (uint32_t)px; out_sure = sure;
    };
    // Group g: the centre rows R g .. R g + R - 1, one per wave, in ring slot g & 3.  They read units g - 1, g, g + 1; unit g + 2
    // arrives meanwhile and goes into the slot of unit g - 2.  (Four groups per turn of the loop: the slots are constants and every
    // LDS address is a lane's base + an immediate.)
    auto step = [&](auto s_tag, int g) {
        constexpr int S = decltype(s_tag)::value;
        const bool more = g + 1 < groups;
#ifndef VRT_PAIR_NOPRIO
        // The scheduler serves the oldest wave first: of the workgroups of a compute unit the youngest would be left to finish alone,
        // one wave per SIMD.  A wave's priority falls as it gets on, so that whoever is behind goes first and all end together.
        {
            if (4 * g < groups) __builtin_amdgcn_s_setprio(3); else if (2 * g < groups) __builtin_amdgcn_s_setprio(2);
            else if (4 * g < 3 * groups) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0);
        }
#endif
        if (more) fetch(g + 2);
        const int f = R * g + wave, py = ys + f - R;
        const bool outrow = g >= 1 && py < ye;
        const bool have = outrow && l >= R && l < 64 - R && px < P.W;
        uint32_t out_codes = 0u, out_idx = 0u;
        bool out_sure = true;
        const bool w4 = fl_w4 != 0u;
        if (f < nrows + R) {                                         // (uniform per wave; every lane computes its texel's weights)
            if (w4) row(std::true_type{}, s_tag, outrow, py, out_codes, out_idx, out_sure);
            else    row(std::false_type{}, s_tag, outrow, py, out_codes, out_idx, out_sure);
        }
        if (more) stash((S + 2) & 3);
        if (have) {
            if (out_sure) reinterpret_cast<uint32_t*>(P.color_out)[out_idx] = out_codes;
            else if (FLAG) { const uint32_t slot = atomicAdd(&fl_n, 1u); if (slot < VRT_PAIR_FIXCAP) fl_px[slot] = out_idx; }
        }
        __syncthreads();
    };
    uint32_t done = 0u;                                               // listed pixels already evaluated the shader's own way
    for (int g = 0; g < groups; g += 4) {
        if (FLAG && g > 0) {
            // The pixels listed so far, now -- under the other workgroups' rows -- rather than all at the end of the launch, where every
            // workgroup would stand in this chain of dependent instructions at once with nothing to hide it.  (The barrier: nobody
            // lists a pixel of the next group before everybody has read the count.)
            const uint32_t n = fl_n < VRT_PAIR_FIXCAP ? fl_n : VRT_PAIR_FIXCAP;
            __syncthreads();
#ifdef VRT_K3_STAMPS
            const uint32_t k3_r0 = (uint32_t)wall_clock64();
#endif
#ifndef VRT_PAIR_EXP_NOREDO
            if (n > done) { denoise_redo<false, false>(P, R, n, false, x0, OW, ys, ye, fl_px, fx_w, fx_c, done); done = n; }
#endif
#ifdef VRT_K3_STAMPS
            k3_redo += (uint32_t)wall_clock64() - k3_r0;
#endif
        }
        step(std::integral_constant<int, 0>{}, g);
        if (g + 1 >= groups) break;
        step(std::integral_constant<int, 1>{}, g + 1);
        if (g + 2 >= groups) break;
        step(std::integral_constant<int, 2>{}, g + 2);
        if (g + 3 >= groups) break;
        step(std::integral_constant<int, 3>{}, g + 3);
    }
#ifdef VRT_K3_STAMPS
    k3_t[2] = (uint32_t)wall_clock64();
#endif
    if (FLAG) {
        // (the loop's last barrier is behind us: fl_n and fl_px are final)
        const uint32_t n = fl_n;
        if (n > done) {                                              // uniform per workgroup
#ifndef VRT_PAIR_NOPRIO
            __builtin_amdgcn_s_setprio(3);
#endif
#ifndef VRT_PAIR_EXP_NOREDO
            denoise_redo<false, false>(P, R, n, n > VRT_PAIR_FIXCAP, x0, OW, ys, ye, fl_px, fx_w, fx_c, done);
#endif
        }
        if (n != 0u && P.fix_counts && threadIdx.x == 0) atomicAdd(&P.fix_counts[(blockIdx.y * gridDim.x + blockIdx.x) & (VRT_DENOISE_SEGS - 1u)], n);
    }
#ifdef VRT_K3_STAMPS
    __syncthreads(); k3_stamp();
#endif
}

// ---- pass 0, a wave to itself (round 4) --------------------------------------------------------------------------------------
// phi = +inf: every edge-stopping weight is exactly 1 and the pass is a 3 x 3 blur of the colour plane with the tap offset 1.  A
// wave owns 62 output columns (its 64 lanes are the columns x0 - 1 .. x0 + 62) and SEG rows: it requests the SEG + 2 rows of its
// column once, all before the first is used, and walks down them with the three rows it needs as floats in registers -- a lane's
// left and right neighbours come through the data-parallel shifts (wave_shr / wave_shl), no LDS, no barrier, nothing shared with
// another wave.  The kernel is separable -- (g, 1, g) x (g, 1, g) with g = G1 = exp(-1/8), G2 = G1^2 --, so a row's horizontal sums
// fma(l, g, fma(r, g, c)) are taken once, when the row arrives, and an output row is fma(h_up, g, fma(h_down, g, h)): four fused
// multiply-adds per channel instead of eight.  That is another cheap form than k_denoise_ver<.., PASS0>'s, under the same guard
// (vrt_denoise_bound.h, denoise_guard_pass0, derives both); the pixels within the guard -- a dozen to a hundred per frame -- go
// through denoise_redo at the end.
#ifndef VRT_P0_SEG
#define VRT_P0_SEG 8
#endif
template <bool FLAG>
__global__ __launch_bounds__(64) void k_denoise_p0(const DenoiseParams P, int segs_per_strip)
{
    __shared__ uint32_t fl_px[64];
    __shared__ float fx_w[7][9];
    __shared__ uint32_t fx_c[7][9];
    constexpr int OW = 62, SEG = VRT_P0_SEG;
    const int x0 = blockIdx.x * OW;
    int ys, ye;
    {
        const int k = (int)blockIdx.y / segs_per_strip, j = (int)blockIdx.y - k * segs_per_strip;
        const int g = k * P.sh.nranks + P.sh.rank;
        int r0 = g * P.sh.strip_rows - P.extend, r1 = (g + 1) * P.sh.strip_rows;
        r1 = (r1 < P.H ? r1 : P.H) + P.extend;
        r0 = r0 < 0 ? 0 : r0; r1 = r1 < P.H ? r1 : P.H;
        ys = r0 + j * SEG;
        ye = ys + SEG < r1 ? ys + SEG : r1;
    }
    if (ys >= ye) return;                                 // uniform
    const int l = threadIdx.x, px = x0 - 1 + l;
    const uint32_t xA = (uint32_t)(px < 0 ? 0 : (px > P.W - 1 ? P.W - 1 : px));
    const uint32_t* const gc = reinterpret_cast<const uint32_t*>(P.color_in);
    uint32_t code[SEG + 2];
#pragma unroll
    for (int q = 0; q < SEG + 2; q++) {                   // rows ys - 1 .. ys + SEG, clamped to the frame (rows beyond ye + 1 are never used)
        int y = ys - 1 + q;
        y = y < 0 ? 0 : (y > P.H - 1 ? P.H - 1 : y);
        code[q] = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(gc + (size_t)y * (size_t)P.W) + xA * 4u);
    }
    const float half_guard = 0.5f - P.guard;
    constexpr float rsum = (float)(1.0 / (1.0 + 4.0 * 0.8824969025845955 + 4.0 * 0.7788007830714049));
    // a row as its horizontal sums, three (four) channels
    struct Row { float h[4]; };
    bool w4 = false;                                      // (uniform) a colour alpha has been met: the fourth channel's sums from here on
    auto load_row = [&](uint32_t cc, Row& o) {
        const uint32_t cl = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)cc, 0x138, 0xf, 0xf, false);     // wave_shr:1 -- lane l gets lane l - 1's
        const uint32_t cr = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)cc, 0x130, 0xf, 0xf, false);     // wave_shl:1 -- lane l gets lane l + 1's
        if (__ballot((cc >> 24) != 0u) != 0ull) w4 = true;
        o.h[0] = __builtin_fmaf((float)(cl & 0xFFu), kGauss1, __builtin_fmaf((float)(cr & 0xFFu), kGauss1, (float)(cc & 0xFFu)));
        o.h[1] = __builtin_fmaf((float)((cl >> 8) & 0xFFu), kGauss1, __builtin_fmaf((float)((cr >> 8) & 0xFFu), kGauss1, (float)((cc >> 8) & 0xFFu)));
        o.h[2] = __builtin_fmaf((float)((cl >> 16) & 0xFFu), kGauss1, __builtin_fmaf((float)((cr >> 16) & 0xFFu), kGauss1, (float)((cc >> 16) & 0xFFu)));
        o.h[3] = w4 ? __builtin_fmaf((float)(cl >> 24), kGauss1, __builtin_fmaf((float)(cr >> 24), kGauss1, (float)(cc >> 24))) : 0.0f;
    };
    Row rows[3];
    load_row(code[0], rows[0]);
    load_row(code[1], rows[1]);
    uint32_t n = 0u;                                      // (uniform) pixels listed so far
    const bool col_ok = l >= 1 && l <= OW && px < P.W;
#pragma unroll
    for (int q = 0; q < SEG; q++) {
        load_row(code[q + 2], rows[(q + 2) % 3]);
        const int py = ys + q;
        if (py < ye) {                                    // uniform
            const Row& up = rows[q % 3]; const Row& me = rows[(q + 1) % 3]; const Row& dn = rows[(q + 2) % 3];
            float a[4];
#pragma unroll
            for (int ch = 0; ch < 4; ch++) a[ch] = (ch == 3 && !w4) ? 0.0f : __builtin_fmaf(up.h[ch], kGauss1, __builtin_fmaf(dn.h[ch], kGauss1, me.h[ch]));
            const float y0f = __builtin_fmaf(a[0], rsum, 0.5f), y1f = __builtin_fmaf(a[1], rsum, 0.5f), y2f = __builtin_fmaf(a[2], rsum, 0.5f);
            const float f0 = __builtin_amdgcn_fractf(y0f), f1 = __builtin_amdgcn_fractf(y1f), f2 = __builtin_amdgcn_fractf(y2f);
            const uint32_t o0 = (uint32_t)y0f, o1 = (uint32_t)y1f, o2 = (uint32_t)y2f;
            bool sure = !FLAG || (__builtin_fabsf(f0 - 0.5f) < half_guard && __builtin_fabsf(f1 - 0.5f) < half_guard && __builtin_fabsf(f2 - 0.5f) < half_guard);
            uint32_t o3 = 0u;
            if (w4) {
                const float y3f = __builtin_fmaf(a[3], rsum, 0.5f), f3 = __builtin_amdgcn_fractf(y3f);
                o3 = (uint32_t)y3f;
                if (FLAG) sure = sure && __builtin_fabsf(f3 - 0.5f) < half_guard;
            }
            const uint32_t idx = (uint32_t)py * (uint32_t)P.W + (uint32_t)px;
            if (col_ok) {
                if (sure) reinterpret_cast<uint32_t*>(P.color_out)[idx] = o0 | (o1 << 8) | (o2 << 16) | (o3 << 24);
            }
            if (FLAG) {
                const uint64_t m = __ballot(col_ok && !sure);
                if (m != 0ull) {                              // (uniform; rare) the listed pixels: the wave's own count, a lane's rank among the listers
                    if (col_ok && !sure) {
                        const uint32_t slot = n + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                        if (slot < 64u) fl_px[slot] = idx;
                    }
                    n += (uint32_t)__builtin_popcountll(m);
                }
            }
        }
    }
    if (FLAG && n != 0u) {
        __syncthreads();
        if (P.fix_counts && threadIdx.x == 0) atomicAdd(&P.fix_counts[(blockIdx.y * gridDim.x + blockIdx.x) & (VRT_DENOISE_SEGS - 1u)], n);
        denoise_redo<false, true>(P, 1, n, n > 64u, x0, OW, ys, ye, fl_px, fx_w, fx_c);
    }
}

// a run-time bool as a template argument: f(std::true_type()) or f(std::false_type()); inside f, decltype(b)::value
template <class F> static void dispatch_bool(bool b, F&& f)
{
    if (b) f(std::true_type()); else f(std::false_type());
}

hipError_t launch_denoise_pass(const DenoiseParams& p, hipStream_t s)
{
    int per = p.sh.strip_rows + 2 * p.extend;
    int rows = p.sh.n_local_strips * per;
    dim3 grid((unsigned)((p.W + 63) / 64), (unsigned)((rows + 3) / 4)), block(256);
    // phi = +inf in all three channels <=> pass 0 (denoiser_stage.cpp:148-150)
    bool inf = __builtin_isinf(p.phi_color) && __builtin_isinf(p.phi_normal) && __builtin_isinf(p.phi_pos);
    // LDS tiling needs an integral tap offset, a halo that fits (<= 5 px: 74 x 14 px x 48 B = 48.6 KiB) and blocks of
    // 4 consecutive frame rows (single strip, or strips whose extended height is a multiple of 4)
    float sw = p.step_width;
    int R = (int)sw;
    bool tiled = (float)R == sw && R >= 1 && R <= 5 && (p.sh.nranks == 1 || per % 4 == 0);
    const bool shipped = (p.mode & 1) == VRT_DENOISE_AS_SHIPPED;
    if ((float)R == sw && R == 1 && inf && p.verified && !shipped && !p.no_p0) {
        // pass 0 of the canonical taps, a wave to itself (k_denoise_p0): strips of 62 output columns x VRT_P0_SEG rows.  (VRT_DENOISE_FAST too:
        // its pass 0 has always been exact, and this is 8 us against the literal kernel's 11.7.)
        const int strips = (p.W + 61) / 62;
        const int strip_ext = p.sh.nranks == 1 ? p.H : per;
        const int segs = (strip_ext + VRT_P0_SEG - 1) / VRT_P0_SEG;
        dim3 g2((unsigned)strips, (unsigned)(segs * p.sh.n_local_strips));
        hipLaunchKernelGGL((k_denoise_p0<true>), g2, dim3(64), 0, s, p, segs);
    }
    else
    // (a rank's 16-row strips are too short for it -- R rows above every segment only compute weights --: two passes over rank 0's strips of
    // 2 / 4 / 8 ranks 29.8 / 18.5 / 14.2 us against k_denoise_ver's 27.0 / 19.5 / 13.9, tools/exp_r4_k3_shard.py; bands of 64 rows and more take it)
    if ((float)R == sw && R >= 2 && R <= 5 && p.verified && !inf && !shipped && !p.no_pair && (p.sh.nranks == 1 || per >= 64)) {
        // the verified pass with every weight computed once (k_denoise_pair): strips of 64 - 2 R output columns x seg_rows rows, R waves
        // per workgroup, as many waves in the launch as k_denoise_ver's (p.pair_wgs > 0: that many workgroups instead)
        const int ow = 64 - 2 * R;
        const int strips = (p.W + ow - 1) / ow;
        const int strip_ext = p.sh.nranks == 1 ? p.H : per;
        const int total = p.sh.nranks == 1 ? p.H : rows;
        // (as many waves as k_denoise_ver's launch, and no segment much longer than 48 rows: 4K measured 105 against 109 us for two passes)
        int wgs = (p.pair_wgs > 0 ? p.pair_wgs : 4096 / R) / strips; if (wgs < 1) wgs = 1;
        if (p.pair_wgs <= 0 && wgs < (total + 47) / 48) wgs = (total + 47) / 48;
        int seg_rows = ((total + wgs - 1) / wgs + R - 1) / R * R; if (seg_rows < 2 * R) seg_rows = 2 * R;
        const int segs = (strip_ext + seg_rows - 1) / seg_rows;
        dim3 g2((unsigned)strips, (unsigned)(segs * p.sh.n_local_strips));
#ifdef VRT_PAIR_NOLW
        const size_t l2 = (size_t)(4 * R) * 64 * 24;
#else
        const size_t l2 = (size_t)(4 * R) * 64 * 28;
#endif
        const bool flag = !(p.mode & VRT_DENOISE_FAST);
        dispatch_bool(flag, [&](auto fl) {
            constexpr bool FL = decltype(fl)::value;
            switch (R) {
            case 2:  hipLaunchKernelGGL((k_denoise_pair<FL, 2>), g2, dim3(64 * 2), l2, s, p, seg_rows, segs); break;
            case 3:  hipLaunchKernelGGL((k_denoise_pair<FL, 3>), g2, dim3(64 * 3), l2, s, p, seg_rows, segs); break;
            case 4:  hipLaunchKernelGGL((k_denoise_pair<FL, 4>), g2, dim3(64 * 4), l2, s, p, seg_rows, segs); break;
            default: hipLaunchKernelGGL((k_denoise_pair<FL, 5>), g2, dim3(64 * 5), l2, s, p, seg_rows, segs); break;
            }
        });
    }
    else if ((float)R == sw && R >= 1 && R <= 5 && p.verified && !(inf && (p.mode & VRT_DENOISE_FAST))) {
        // the verified pass (exact output) or, with VRT_DENOISE_FAST, its cheap half alone: 64-pixel column strips x seg_rows rows of
        // the rank's strips (with the rows either side this pass must also produce), about four workgroups per compute unit
        // (768 ... 2048 measured the same); pass 0: the ring holds the colour plane only -- 34 VGPRs, 9 KB of LDS: eight
        const int strips = (p.W + 63) / 64;
        const int strip_ext = p.sh.nranks == 1 ? p.H : per;                 // rows of a local strip with its extension
        const int total = p.sh.nranks == 1 ? p.H : rows;
        int wgs = (inf ? 2048 : 1024) / strips; if (wgs < 1) wgs = 1;
        int seg_rows = ((total + wgs - 1) / wgs + 3) & ~3; if (seg_rows < 8) seg_rows = 8;
        const int segs = (strip_ext + seg_rows - 1) / seg_rows;
        dim3 g2((unsigned)strips, (unsigned)(segs * p.sh.n_local_strips));
        const int U = (4 + 2 * R + 3) / 4;
        const size_t l2 = (size_t)(64 + 2 * R) * (size_t)(4 * (U + 1)) * (inf ? 4 : 24);
        if (inf) dispatch_bool(shipped, [&](auto sh) {
            constexpr bool SH = decltype(sh)::value;
            if (R == 1) hipLaunchKernelGGL((k_denoise_ver<SH, true, 1, true>), g2, block, l2, s, p, R, seg_rows, segs);
            else        hipLaunchKernelGGL((k_denoise_ver<SH, true, 0, true>), g2, block, l2, s, p, R, seg_rows, segs);
        });
        else {
            const bool flag = !(p.mode & VRT_DENOISE_FAST);
            dispatch_bool(flag, [&](auto fl) { dispatch_bool(shipped, [&](auto sh) {
                constexpr bool FL = decltype(fl)::value, SH = decltype(sh)::value;
                switch (R) {
                case 2:  hipLaunchKernelGGL((k_denoise_ver<SH, FL, 2>), g2, block, l2, s, p, R, seg_rows, segs); break;
                case 3:  hipLaunchKernelGGL((k_denoise_ver<SH, FL, 3>), g2, block, l2, s, p, R, seg_rows, segs); break;
                case 5:  hipLaunchKernelGGL((k_denoise_ver<SH, FL, 5>), g2, block, l2, s, p, R, seg_rows, segs); break;
                default: hipLaunchKernelGGL((k_denoise_ver<SH, FL, 0>), g2, block, l2, s, p, R, seg_rows, segs); break;
                }
            }); });
        }
    }
    else if (tiled) {
        size_t lds = (size_t)(64 + 2 * R) * (size_t)(4 + 2 * R) * (inf ? 16 : 48);   // pass 0 stages the colour plane only
        if (false) {}
        else if (!inf && (p.mode & VRT_DENOISE_FAST) && p.sh.nranks == 1 && p.extend == 0) {
            const int th = p.tile16 ? 16 : 8;                                // development switch: tile height 8 / 16
            dim3 g2((unsigned)((p.W + 63) / 64), (unsigned)((p.H + th - 1) / th));
            const size_t l2 = (size_t)(64 + 2 * R) * (size_t)(th + 2 * R) * 48;
            dispatch_bool(shipped, [&](auto sh) {
                if (th == 8) hipLaunchKernelGGL((k_denoise_fast<decltype(sh)::value, 8>), g2, block, l2, s, p, R);
                else         hipLaunchKernelGGL((k_denoise_fast<decltype(sh)::value, 16>), g2, block, l2, s, p, R);
            });
        }
        else dispatch_bool(shipped, [&](auto sh) {
            constexpr bool SH = decltype(sh)::value;
            if (!inf && (p.mode & VRT_DENOISE_FAST)) hipLaunchKernelGGL((k_denoise_lds<false, SH, true>), grid, block, lds, s, p, R);
            else if (inf) hipLaunchKernelGGL((k_denoise_lds<true, SH>), grid, block, lds, s, p, R);
            else if (p.packed_ok && !p.no_packed)                            // (development switch: the tap-by-tap form)
                hipLaunchKernelGGL((k_denoise_lds<false, SH, false, true>), grid, block, lds, s, p, R);
            else hipLaunchKernelGGL((k_denoise_lds<false, SH>), grid, block, lds, s, p, R);
        });
    } else {
        if (inf) hipLaunchKernelGGL(k_denoise<true>, grid, block, 0, s, p);
        else     hipLaunchKernelGGL(k_denoise<false>, grid, block, 0, s, p);
    }
    return hipGetLastError();
}

} // namespace vrt
