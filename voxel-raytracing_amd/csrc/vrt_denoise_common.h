// vrt_denoise_common.h -- K3, what the denoiser kernels share: the guides of a texel, the shader's own weights and pixel (vrt_denoise.hip includes it first).
#pragma once

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

} // namespace vrt
