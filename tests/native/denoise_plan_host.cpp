// denoise_plan_host.cpp -- csrc/vrt_denoise_plan.h built for the host: the kernel and launch shape of a denoiser pass, as
// launch_denoise_pass takes them, for tests/test_launch_shapes_cpu.py to hold the case tables of the GPU tests to.  With
// -DDENOISE_PLAN_MAIN it is a program of its own (built with the sanitizers by the tests): the plan over a sweep of small frames and
// at the largest ones, one checksum line per block.
#include <cstdio>
#include <initializer_list>

#include "../../voxel-raytracing_amd/csrc/vrt_denoise_plan.h"

using namespace vrt;

namespace {

struct Sum {
    uint64_t h = 1469598103934665603ull, n = 0;
    void word(uint64_t v) { h = (h ^ v) * 1099511628211ull; }
    void plan(const DenoisePlanIn& in)
    {
        const DenoisePlan q = denoise_plan(in);
        word((uint64_t)q.family); word(q.key); word(q.grid_x); word(q.grid_y); word(q.block); word(q.lds_bytes);
        word((uint64_t)q.R); word((uint64_t)q.seg_rows); word((uint64_t)q.segs);
        n++;
    }
};

// every route of a frame: pass 0 and a weighted pass, the four modes, verified or not, each switch alone
void routes(Sum& s, DenoisePlanIn in)
{
    for (int inf = 0; inf < 2; inf++)
        for (int mode = 0; mode < 4; mode++)
            for (int verified = 0; verified < 2; verified++)
                for (int sw = 0; sw < 6; sw++) {
                    DenoisePlanIn p = in;
                    p.phi_inf = inf; p.mode = mode; p.verified = verified;
                    p.tile16 = sw == 1; p.no_packed = sw == 2; p.no_pair = sw == 3; p.no_p0 = sw == 4; p.packed_ok = sw != 5;
                    s.plan(p);
                }
}

const float kSteps[] = {1.0f, 2.0f, 3.0f, 4.0f, 5.0f, 6.0f, 1.5f, 0.75f};
const int kPairWgs[] = {0, 1, 3, 21, 60, 4096};

} // namespace

extern "C" {

void denoise_plan_c(const DenoisePlanIn* in, DenoisePlan* out) { *out = denoise_plan(*in); }
uint32_t denoise_key_c(int32_t family, int32_t a, int32_t b, int32_t c, int32_t d) { return denoise_key(family, a, b, c, d); }
uint32_t denoise_plan_sizes_c() { return (uint32_t)sizeof(DenoisePlanIn) << 16 | (uint32_t)sizeof(DenoisePlan); }

// block 0: whole frames; 1: a rank's strips; 2: the largest frames.  -> the checksum; *plans: how many plans went into it
uint64_t denoise_plan_block_c(int32_t block, uint64_t* plans)
{
    Sum s;
    if (block == 0) {
        // W = 1, one below / at / one above a multiple of every strip width (64 - 2 R: 54 .. 62, and 64), many strips; heights below 2 R and up
        const int Ws[] = {1, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63, 64, 65, 107, 108, 109, 123, 124, 125, 127, 128, 129, 130, 4097, 16384};
        const int Hs[] = {1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 37, 47, 48, 49, 65, 117, 361, 925, 2160};
        for (int W : Ws) for (int H : Hs) for (float sw : kSteps) for (int pw : kPairWgs) {
            DenoisePlanIn in = {};
            in.W = W; in.H = H; in.step_width = sw; in.pair_wgs = pw;
            in.nranks = 1; in.strip_rows = (H + 15) / 16 * 16; in.n_local_strips = 1;        // (make_shard: one rank)
            routes(s, in);
        }
    } else if (block == 1) {
        const int Ws[] = {1, 58, 59, 64, 117, 130};
        for (int W : Ws) for (int nranks = 2; nranks <= 4; nranks++) for (int strip : {16, 32, 48, 64, 80}) for (int ext : {0, 1, 3, 5, 8, 25})
            for (int local = 1; local <= 3; local++) for (float sw : kSteps) for (int pw : kPairWgs) {
                DenoisePlanIn in = {};
                in.W = W; in.H = strip * nranks * local - 7; in.step_width = sw; in.pair_wgs = pw; in.extend = ext;
                in.nranks = nranks; in.strip_rows = strip; in.n_local_strips = local;
                routes(s, in);
            }
    } else {
        // include/vrt.h states no size limit of its own for vrt_denoise (it refuses W or H < 1 only); the frames it is given are
        // vrt_render_geometry's, whose limits that header does state ("Limits: screen_size up to 32768 per side and below 2^28 pixels per
        // frame"): so up to 32768 a side, and the verified form up to W * H < 2^28, the bound vrt_denoise applies itself (vrt_api_post.hip),
        // a side of which no part of the plan limits; sharded: strips of 16 rows over 2 ranks, extended by 50 rows, more than ten passes
        // of the default step reach -- rows = 9.7e8 at H = 2^28 - 1, the margin vrt_denoise_plan.h states beside `rows`
        const int big[][2] = {{32768, 32768}, {32768, 1}, {1, 32768}, {32767, 32767}, {32768, 8191}, {8191, 32768}, {16384, 16383}, {16383, 16384},
                              {(1 << 28) - 1, 1}, {1, (1 << 28) - 1}};
        for (const auto& wh : big) for (float sw : kSteps) for (int pw : kPairWgs) {
            DenoisePlanIn in = {};
            in.W = wh[0]; in.H = wh[1]; in.step_width = sw; in.pair_wgs = pw;
            in.nranks = 1; in.strip_rows = (wh[1] + 15) / 16 * 16; in.n_local_strips = 1;
            routes(s, in);
            if (wh[1] >= 32) {
                in.nranks = 2; in.strip_rows = 16; in.n_local_strips = (wh[1] + 31) / 32; in.extend = 50;
                routes(s, in);
            }
        }
    }
    if (plans) *plans = s.n;
    return s.h;
}

} // extern "C"

#if defined(DENOISE_PLAN_MAIN)
int main()
{
    for (int block = 0; block < 3; block++) {
        uint64_t n = 0;
        const uint64_t h = denoise_plan_block_c(block, &n);
        printf("%d %llu %llu\n", block, (unsigned long long)n, (unsigned long long)h);
    }
    return 0;
}
#endif
