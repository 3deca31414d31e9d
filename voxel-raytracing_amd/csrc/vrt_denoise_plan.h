// vrt_denoise_plan.h -- which kernel a denoiser pass takes and the shape of its launch, decided on the host alone: no HIP type, so
// plain g++ compiles it and tests/test_launch_shapes_cpu.py asks it what the case tables of the GPU tests really exercise
// (tests/native/denoise_plan_host.cpp).  launch_denoise_pass (vrt_denoise.hip) fills a DenoisePlanIn from the DenoiseParams of the
// pass, calls denoise_plan and launches what the DenoisePlan names, with the geometry it states.
#pragma once
#include <cstdint>

#include "../../include/vrt.h"

#ifndef VRT_P0_SEG
#define VRT_P0_SEG 8            // rows of a k_denoise_p0 segment (vrt_denoise_p0.h: the kernel's SEG)
#endif

namespace vrt {

enum DenoiseFamily : int32_t {
    DENOISE_K_DENOISE = 0,     // k_denoise<PHI_INF>
    DENOISE_K_LDS     = 1,     // k_denoise_lds<PHI_INF, SHIPPED, FAST, PACKED>
    DENOISE_K_FAST    = 2,     // k_denoise_fast<SHIPPED, TH>
    DENOISE_K_VER     = 3,     // k_denoise_ver<SHIPPED, FLAG, RT, PASS0>
    DENOISE_K_PAIR    = 4,     // k_denoise_pair<FLAG, R>
    DENOISE_K_P0      = 5      // k_denoise_p0<FLAG>
};

// what launch_denoise_pass reads of a pass (DenoiseParams and its ShardMap)
struct DenoisePlanIn {
    int32_t W, H;
    float   step_width;
    int32_t phi_inf;           // all three phis are +inf <=> pass 0 (denoiser_stage.cpp:148-150)
    int32_t mode, verified, packed_ok, extend;
    int32_t tile16, no_packed, no_pair, no_p0, pair_wgs;      // the development switches
    int32_t nranks, strip_rows, n_local_strips;               // of the shard
};

// One number per instantiation: the family and its template arguments in the template's own order (the comments above).  The arms
// of launch_denoise_pass' switch are these; tests/test_launch_shapes_cpu.py lists them once more and shows that the case tables of
// the GPU tests reach each.
constexpr uint32_t denoise_key(int32_t family, int32_t a = 0, int32_t b = 0, int32_t c = 0, int32_t d = 0)
{
    return (uint32_t)family << 24 | (uint32_t)a << 18 | (uint32_t)b << 12 | (uint32_t)c << 6 | (uint32_t)d;
}

struct DenoisePlan {
    int32_t  family;           // DenoiseFamily
    uint32_t key;              // denoise_key of the instantiation
    // the template arguments of the instantiation; those the family does not have are 0
    int32_t  PHI_INF, SHIPPED, FAST, PACKED, FLAG, RT, PASS0, TH;
    int32_t  pair_R;           // k_denoise_pair's R
    uint32_t grid_x, grid_y, block;
    uint64_t lds_bytes;        // dynamic LDS
    // the integer arguments behind the DenoiseParams, where the family takes them (else 0)
    int32_t  R, seg_rows, segs;
};

inline DenoisePlan denoise_plan(const DenoisePlanIn& p)
{
    DenoisePlan q = {};
    int per = p.strip_rows + 2 * p.extend;
    // (int is enough: vrt_denoise refuses more than 10 passes and a tap reaches ceil(i * stepWidth + 1) rows, so with the steps of a few
    // pixels the filter is for, extend is some tens of rows and rows stays near H + 2 * extend * strips: 9.7e8 at the tallest verified
    // frame, H = 2^28 - 1 in 16-row strips over 2 ranks with extend = 50 (tests/native/denoise_plan_host.cpp).  A step width in the thousands on such a
    // frame would overflow it, here as in every version before.)
    int rows = p.n_local_strips * per;
    // the literal kernels' launch: 64 columns x 4 rows of the rank's rows per workgroup
    q.grid_x = (unsigned)((p.W + 63) / 64); q.grid_y = (unsigned)((rows + 3) / 4); q.block = 256;
    bool inf = p.phi_inf != 0;
    // LDS tiling needs an integral tap offset, a halo that fits (<= 5 px: 74 x 14 px x 48 B = 48.6 KiB) and blocks of
    // 4 consecutive frame rows (single strip, or strips whose extended height is a multiple of 4)
    float sw = p.step_width;
    int R = (int)sw;
    bool tiled = (float)R == sw && R >= 1 && R <= 5 && (p.nranks == 1 || per % 4 == 0);
    const bool shipped = (p.mode & 1) == VRT_DENOISE_AS_SHIPPED;
    if ((float)R == sw && R == 1 && inf && p.verified && !shipped && !p.no_p0) {
        // pass 0 of the canonical taps, a wave to itself (k_denoise_p0): strips of 62 output columns x VRT_P0_SEG rows.  (VRT_DENOISE_FAST too:
        // its pass 0 has always been exact, and this is 8 us against the literal kernel's 11.7.)
        const int strips = (p.W + 61) / 62;
        const int strip_ext = p.nranks == 1 ? p.H : per;
        const int segs = (strip_ext + VRT_P0_SEG - 1) / VRT_P0_SEG;
        q.family = DENOISE_K_P0; q.FLAG = 1;
        q.grid_x = (unsigned)strips; q.grid_y = (unsigned)(segs * p.n_local_strips); q.block = 64;
        q.segs = segs;
    }
    else
    // (a rank's 16-row strips are too short for it -- R rows above every segment only compute weights --: two passes over rank 0's strips of
    // 2 / 4 / 8 ranks 29.8 / 18.5 / 14.2 us against k_denoise_ver's 27.0 / 19.5 / 13.9, tools/exp_r4_k3_shard.py; bands of 64 rows and more take it)
    if ((float)R == sw && R >= 2 && R <= 5 && p.verified && !inf && !shipped && !p.no_pair && (p.nranks == 1 || per >= 64)) {
        // the verified pass with every weight computed once (k_denoise_pair): strips of 64 - 2 R output columns x seg_rows rows, R waves
        // per workgroup, as many waves in the launch as k_denoise_ver's (p.pair_wgs > 0: that many workgroups instead)
        const int ow = 64 - 2 * R;
        const int strips = (p.W + ow - 1) / ow;
        const int strip_ext = p.nranks == 1 ? p.H : per;
        const int total = p.nranks == 1 ? p.H : rows;
        // (as many waves as k_denoise_ver's launch, and no segment much longer than 48 rows: 4K measured 105 against 109 us for two passes)
        int wgs = (p.pair_wgs > 0 ? p.pair_wgs : 4096 / R) / strips; if (wgs < 1) wgs = 1;
        if (p.pair_wgs <= 0 && wgs < (total + 47) / 48) wgs = (total + 47) / 48;
        int seg_rows = ((total + wgs - 1) / wgs + R - 1) / R * R; if (seg_rows < 2 * R) seg_rows = 2 * R;
        const int segs = (strip_ext + seg_rows - 1) / seg_rows;
        q.family = DENOISE_K_PAIR; q.FLAG = !(p.mode & VRT_DENOISE_FAST); q.pair_R = R;
        q.grid_x = (unsigned)strips; q.grid_y = (unsigned)(segs * p.n_local_strips); q.block = (unsigned)(64 * R);
#ifdef VRT_PAIR_NOLW
        q.lds_bytes = (uint64_t)(4 * R) * 64 * 24;
#else
        q.lds_bytes = (uint64_t)(4 * R) * 64 * 28;
#endif
        q.seg_rows = seg_rows; q.segs = segs;
    }
    else if ((float)R == sw && R >= 1 && R <= 5 && p.verified && !(inf && (p.mode & VRT_DENOISE_FAST))) {
        // the verified pass (exact output) or, with VRT_DENOISE_FAST, its cheap half alone: 64-pixel column strips x seg_rows rows of
        // the rank's strips (with the rows either side this pass must also produce), about four workgroups per compute unit
        // (768 ... 2048 measured the same); pass 0: the ring holds the colour plane only -- 34 VGPRs, 9 KB of LDS: eight
        const int strips = (p.W + 63) / 64;
        const int strip_ext = p.nranks == 1 ? p.H : per;                 // rows of a local strip with its extension
        const int total = p.nranks == 1 ? p.H : rows;
        int wgs = (inf ? 2048 : 1024) / strips; if (wgs < 1) wgs = 1;
        int seg_rows = ((total + wgs - 1) / wgs + 3) & ~3; if (seg_rows < 8) seg_rows = 8;
        const int segs = (strip_ext + seg_rows - 1) / seg_rows;
        const int U = (4 + 2 * R + 3) / 4;
        q.family = DENOISE_K_VER; q.SHIPPED = shipped;
        // pass 0 is always exact (FLAG); the tap offsets 1 (pass 0 only), 2, 3 and 5 at compile time, any other at run time (RT = 0)
        if (inf) { q.FLAG = 1; q.RT = R == 1 ? 1 : 0; q.PASS0 = 1; }
        else { q.FLAG = !(p.mode & VRT_DENOISE_FAST); q.RT = (R == 2 || R == 3 || R == 5) ? R : 0; }
        q.grid_x = (unsigned)strips; q.grid_y = (unsigned)(segs * p.n_local_strips);
        q.lds_bytes = (uint64_t)(64 + 2 * R) * (uint64_t)(4 * (U + 1)) * (inf ? 4 : 24);
        q.R = R; q.seg_rows = seg_rows; q.segs = segs;
    }
    else if (tiled) {
        if (!inf && (p.mode & VRT_DENOISE_FAST) && p.nranks == 1 && p.extend == 0) {
            const int th = p.tile16 ? 16 : 8;                                // development switch: tile height 8 / 16
            q.family = DENOISE_K_FAST; q.SHIPPED = shipped; q.TH = th;
            q.grid_y = (unsigned)((p.H + th - 1) / th);
            q.lds_bytes = (uint64_t)(64 + 2 * R) * (uint64_t)(th + 2 * R) * 48;
        }
        else {
            q.family = DENOISE_K_LDS; q.SHIPPED = shipped;
            if (!inf && (p.mode & VRT_DENOISE_FAST)) q.FAST = 1;
            else if (inf) q.PHI_INF = 1;
            else if (p.packed_ok && !p.no_packed) q.PACKED = 1;              // (development switch: the tap-by-tap form)
            q.lds_bytes = (uint64_t)(64 + 2 * R) * (uint64_t)(4 + 2 * R) * (inf ? 16 : 48);   // pass 0 stages the colour plane only
        }
        q.R = R;
    } else {
        q.family = DENOISE_K_DENOISE; q.PHI_INF = inf;
    }
    switch (q.family) {
    case DENOISE_K_DENOISE: q.key = denoise_key(q.family, q.PHI_INF); break;
    case DENOISE_K_LDS:     q.key = denoise_key(q.family, q.PHI_INF, q.SHIPPED, q.FAST, q.PACKED); break;
    case DENOISE_K_FAST:    q.key = denoise_key(q.family, q.SHIPPED, q.TH); break;
    case DENOISE_K_VER:     q.key = denoise_key(q.family, q.SHIPPED, q.FLAG, q.RT, q.PASS0); break;
    case DENOISE_K_PAIR:    q.key = denoise_key(q.family, q.FLAG, q.pair_R); break;
    default:                q.key = denoise_key(q.family, q.FLAG); break;
    }
    return q;
}

} // namespace vrt
