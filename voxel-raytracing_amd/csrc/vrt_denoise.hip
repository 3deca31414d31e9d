// vrt_denoise.hip -- K3 for gfx950: the a-trous denoiser.  The kernels, one header per family, in the order they build on each other, and
// launch_denoise_pass; which kernel a pass takes is decided in vrt_denoise_plan.h.
#include "vrt_device_common.h"
#include "vrt_denoise_plan.h"
#include <type_traits>

#include "vrt_denoise_common.h"
#include "vrt_denoise_literal.h"
#include "vrt_denoise_ver.h"
#include "vrt_denoise_pair.h"
#include "vrt_denoise_p0.h"

namespace vrt {

// Which kernel a pass takes and the shape of its launch: denoise_plan (vrt_denoise_plan.h).  Here, the launch of what it names.
hipError_t launch_denoise_pass(const DenoiseParams& p, hipStream_t s)
{
    DenoisePlanIn in;
    in.W = p.W; in.H = p.H; in.step_width = p.step_width;
    // phi = +inf in all three channels <=> pass 0 (denoiser_stage.cpp:148-150)
    in.phi_inf = __builtin_isinf(p.phi_color) && __builtin_isinf(p.phi_normal) && __builtin_isinf(p.phi_pos);
    in.mode = p.mode; in.verified = p.verified; in.packed_ok = p.packed_ok; in.extend = p.extend;
    in.tile16 = p.tile16; in.no_packed = p.no_packed; in.no_pair = p.no_pair; in.no_p0 = p.no_p0; in.pair_wgs = p.pair_wgs;
    in.nranks = p.sh.nranks; in.strip_rows = p.sh.strip_rows; in.n_local_strips = p.sh.n_local_strips;
    const DenoisePlan q = denoise_plan(in);
    const dim3 g(q.grid_x, q.grid_y), b(q.block);
    const size_t l = (size_t)q.lds_bytes;
    constexpr int32_t KD = DENOISE_K_DENOISE, KL = DENOISE_K_LDS, KF = DENOISE_K_FAST, KV = DENOISE_K_VER, KP = DENOISE_K_PAIR, K0 = DENOISE_K_P0;
    // The compiler emits an instantiation where it is first named, so the order of the arms is the order of the kernels in the code
    // object.  It is the order they have had so far, which keeps every kernel at its address; what another order costs or gains has
    // not been measured.  Add new arms at the end.
    switch (q.key) {
    // <FLAG>
    case denoise_key(K0, 1): hipLaunchKernelGGL((k_denoise_p0<true>), g, b, 0, s, p, q.segs); break;
    // <FLAG, R>
    case denoise_key(KP, 1, 2): hipLaunchKernelGGL((k_denoise_pair<true, 2>), g, b, l, s, p, q.seg_rows, q.segs); break;
    case denoise_key(KP, 1, 3): hipLaunchKernelGGL((k_denoise_pair<true, 3>), g, b, l, s, p, q.seg_rows, q.segs); break;
    case denoise_key(KP, 1, 4): hipLaunchKernelGGL((k_denoise_pair<true, 4>), g, b, l, s, p, q.seg_rows, q.segs); break;
    case denoise_key(KP, 1, 5): hipLaunchKernelGGL((k_denoise_pair<true, 5>), g, b, l, s, p, q.seg_rows, q.segs); break;
    case denoise_key(KP, 0, 2): hipLaunchKernelGGL((k_denoise_pair<false, 2>), g, b, l, s, p, q.seg_rows, q.segs); break;
    case denoise_key(KP, 0, 3): hipLaunchKernelGGL((k_denoise_pair<false, 3>), g, b, l, s, p, q.seg_rows, q.segs); break;
    case denoise_key(KP, 0, 4): hipLaunchKernelGGL((k_denoise_pair<false, 4>), g, b, l, s, p, q.seg_rows, q.segs); break;
    case denoise_key(KP, 0, 5): hipLaunchKernelGGL((k_denoise_pair<false, 5>), g, b, l, s, p, q.seg_rows, q.segs); break;
    // <SHIPPED, FLAG, RT, PASS0>: pass 0
    case denoise_key(KV, 1, 1, 1, 1): hipLaunchKernelGGL((k_denoise_ver<true, true, 1, true>), g, b, l, s, p, q.R, q.seg_rows, q.segs); break;
    case denoise_key(KV, 1, 1, 0, 1): hipLaunchKernelGGL((k_denoise_ver<true, true, 0, true>), g, b, l, s, p, q.R, q.seg_rows, q.segs); break;
    case denoise_key(KV, 0, 1, 1, 1): hipLaunchKernelGGL((k_denoise_ver<false, true, 1, true>), g, b, l, s, p, q.R, q.seg_rows, q.segs); break;
    case denoise_key(KV, 0, 1, 0, 1): hipLaunchKernelGGL((k_denoise_ver<false, true, 0, true>), g, b, l, s, p, q.R, q.seg_rows, q.segs); break;
    // ... the weighted passes
    case denoise_key(KV, 1, 1, 2, 0): hipLaunchKernelGGL((k_denoise_ver<true, true, 2>), g, b, l, s, p, q.R, q.seg_rows, q.segs); break;
    case denoise_key(KV, 1, 1, 3, 0): hipLaunchKernelGGL((k_denoise_ver<true, true, 3>), g, b, l, s, p, q.R, q.seg_rows, q.segs); break;
    case denoise_key(KV, 1, 1, 5, 0): hipLaunchKernelGGL((k_denoise_ver<true, true, 5>), g, b, l, s, p, q.R, q.seg_rows, q.segs); break;
    case denoise_key(KV, 1, 1, 0, 0): hipLaunchKernelGGL((k_denoise_ver<true, true, 0>), g, b, l, s, p, q.R, q.seg_rows, q.segs); break;
    case denoise_key(KV, 0, 1, 2, 0): hipLaunchKernelGGL((k_denoise_ver<false, true, 2>), g, b, l, s, p, q.R, q.seg_rows, q.segs); break;
    case denoise_key(KV, 0, 1, 3, 0): hipLaunchKernelGGL((k_denoise_ver<false, true, 3>), g, b, l, s, p, q.R, q.seg_rows, q.segs); break;
    case denoise_key(KV, 0, 1, 5, 0): hipLaunchKernelGGL((k_denoise_ver<false, true, 5>), g, b, l, s, p, q.R, q.seg_rows, q.segs); break;
    case denoise_key(KV, 0, 1, 0, 0): hipLaunchKernelGGL((k_denoise_ver<false, true, 0>), g, b, l, s, p, q.R, q.seg_rows, q.segs); break;
    case denoise_key(KV, 1, 0, 2, 0): hipLaunchKernelGGL((k_denoise_ver<true, false, 2>), g, b, l, s, p, q.R, q.seg_rows, q.segs); break;
    case denoise_key(KV, 1, 0, 3, 0): hipLaunchKernelGGL((k_denoise_ver<true, false, 3>), g, b, l, s, p, q.R, q.seg_rows, q.segs); break;
    case denoise_key(KV, 1, 0, 5, 0): hipLaunchKernelGGL((k_denoise_ver<true, false, 5>), g, b, l, s, p, q.R, q.seg_rows, q.segs); break;
    case denoise_key(KV, 1, 0, 0, 0): hipLaunchKernelGGL((k_denoise_ver<true, false, 0>), g, b, l, s, p, q.R, q.seg_rows, q.segs); break;
    case denoise_key(KV, 0, 0, 2, 0): hipLaunchKernelGGL((k_denoise_ver<false, false, 2>), g, b, l, s, p, q.R, q.seg_rows, q.segs); break;
    case denoise_key(KV, 0, 0, 3, 0): hipLaunchKernelGGL((k_denoise_ver<false, false, 3>), g, b, l, s, p, q.R, q.seg_rows, q.segs); break;
    case denoise_key(KV, 0, 0, 5, 0): hipLaunchKernelGGL((k_denoise_ver<false, false, 5>), g, b, l, s, p, q.R, q.seg_rows, q.segs); break;
    case denoise_key(KV, 0, 0, 0, 0): hipLaunchKernelGGL((k_denoise_ver<false, false, 0>), g, b, l, s, p, q.R, q.seg_rows, q.segs); break;
    // <SHIPPED, TH>
    case denoise_key(KF, 1, 8): hipLaunchKernelGGL((k_denoise_fast<true, 8>), g, b, l, s, p, q.R); break;
    case denoise_key(KF, 1, 16): hipLaunchKernelGGL((k_denoise_fast<true, 16>), g, b, l, s, p, q.R); break;
    case denoise_key(KF, 0, 8): hipLaunchKernelGGL((k_denoise_fast<false, 8>), g, b, l, s, p, q.R); break;
    case denoise_key(KF, 0, 16): hipLaunchKernelGGL((k_denoise_fast<false, 16>), g, b, l, s, p, q.R); break;
    // <PHI_INF, SHIPPED, FAST, PACKED>
    case denoise_key(KL, 0, 1, 1, 0): hipLaunchKernelGGL((k_denoise_lds<false, true, true>), g, b, l, s, p, q.R); break;
    case denoise_key(KL, 1, 1, 0, 0): hipLaunchKernelGGL((k_denoise_lds<true, true>), g, b, l, s, p, q.R); break;
    case denoise_key(KL, 0, 1, 0, 1): hipLaunchKernelGGL((k_denoise_lds<false, true, false, true>), g, b, l, s, p, q.R); break;
    case denoise_key(KL, 0, 1, 0, 0): hipLaunchKernelGGL((k_denoise_lds<false, true>), g, b, l, s, p, q.R); break;
    case denoise_key(KL, 0, 0, 1, 0): hipLaunchKernelGGL((k_denoise_lds<false, false, true>), g, b, l, s, p, q.R); break;
    case denoise_key(KL, 1, 0, 0, 0): hipLaunchKernelGGL((k_denoise_lds<true, false>), g, b, l, s, p, q.R); break;
    case denoise_key(KL, 0, 0, 0, 1): hipLaunchKernelGGL((k_denoise_lds<false, false, false, true>), g, b, l, s, p, q.R); break;
    case denoise_key(KL, 0, 0, 0, 0): hipLaunchKernelGGL((k_denoise_lds<false, false>), g, b, l, s, p, q.R); break;
    // <PHI_INF>
    case denoise_key(KD, 1): hipLaunchKernelGGL((k_denoise<true>), g, b, 0, s, p); break;
    case denoise_key(KD, 0): hipLaunchKernelGGL((k_denoise<false>), g, b, 0, s, p); break;
    default: return hipErrorInvalidValue;                      // (the plan names no other instantiation)
    }
    return hipGetLastError();
}

} // namespace vrt
