// vrt_denoise_ver.h -- K3, the verified pass: k_denoise_ver, and denoise_redo, by which it, k_denoise_pair and k_denoise_p0 evaluate the pixels
// they list once more.  Included by vrt_denoise.hip behind vrt_denoise_literal.h (r2_of).
#pragma once

namespace vrt {

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

} // namespace vrt
