// vrt_denoise_literal.h -- K3, the kernels that compute every pixel themselves: k_denoise (any tap offset, bilinear), k_denoise_lds (tiled) and
// k_denoise_fast (VRT_DENOISE_FAST on a whole frame).  Included by vrt_denoise.hip behind vrt_denoise_common.h.
#pragma once

namespace vrt {

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

} // namespace vrt
