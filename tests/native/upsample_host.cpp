// upsample_host.cpp -- TEST HELPER: the per-pixel function of temporal upsampling (csrc/vrt_upsample.h) compiled for the host
// and run over dumped planes, so that the definition the kernel runs can be compared with its numpy restatement
// (tests/upsample_reference.py) without a GPU.  A program of its own (tests/test_upsample_cpu.py builds it with
// g++ -ffp-contract=off, and once more with -fsanitize=address,undefined):
//     upsample_host IN OUT
// IN:  int32 w, h, TW, TH, frames, max_history, has_history, planes (bit 0: resolved8, bit 1: motion); float32 tol_abs, tol_rel
//      (tol_rel < 0: the default of each frame's current camera); if has_history the history before frame 0 (color16, surface);
//      then per frame: vrt_push cur, vrt_push prev, color8, position, normal8 (w x h).
// OUT: per frame int32 rc (0, or 1 / 2 where vrt_upsample answers VRT_ERR_INVALID for the current / previous camera's basis; the
//      run ends there), color16, surface and the planes asked for (TW x TH).  Frame k's history feeds frame k + 1.
//     upsample_host --alpha IN OUT     IN: float32 (ux, uy, X, Y) each; OUT: uint32 upsample_alpha of each
//     upsample_host --blend IN OUT     IN: uint32 (h, c, a, n) each;    OUT: uint32 upsample_blend of each
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/vrt.h"
#include "../../voxel-raytracing_amd/csrc/vrt_upsample.h"

using namespace vrt;

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool put(FILE* f, const void* p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }

// the two small functions of the definition over a list of arguments
static int functions(const char* mode, const char* inp, const char* outp)
{
    FILE* in = fopen(inp, "rb");
    FILE* out = fopen(outp, "wb");
    if (!in || !out) { fprintf(stderr, "upsample_host: cannot open a file\n"); return 2; }
    uint32_t q[4];
    while (get(in, q, sizeof q)) {
        uint32_t r;
        if (!strcmp(mode, "--alpha")) r = upsample_alpha(rp_u2f(q[0]), rp_u2f(q[1]), rp_u2f(q[2]), rp_u2f(q[3]));
        else r = upsample_blend(q[0], q[1], q[2], q[3]);
        if (!put(out, &r, 4)) return 2;
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}

int main(int argc, char** argv)
{
    if (argc == 4 && (!strcmp(argv[1], "--alpha") || !strcmp(argv[1], "--blend"))) return functions(argv[1], argv[2], argv[3]);
    if (argc != 3) { fprintf(stderr, "usage: upsample_host IN OUT\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "upsample_host: cannot open a file\n"); return 2; }
    int32_t hd[8]; float tl[2];
    if (!get(in, hd, sizeof hd) || !get(in, tl, sizeof tl)) { fprintf(stderr, "upsample_host: short header\n"); return 2; }
    const int w = hd[0], h = hd[1], TW = hd[2], TH = hd[3], frames = hd[4];
    const uint32_t max_history = (uint32_t)hd[5];
    if (w <= 0 || h <= 0 || TW < w || TH < h || TW > 32768 || TH > 32768 || frames < 0) { fprintf(stderr, "upsample_host: bad sizes\n"); return 2; }
    const size_t n = (size_t)w * h, tn = (size_t)TW * TH;
    std::vector<rp_u2> hc[2] = {std::vector<rp_u2>(tn), std::vector<rp_u2>(tn)};
    std::vector<rp_u4> hs[2] = {std::vector<rp_u4>(tn), std::vector<rp_u4>(tn)};
    int cur_hist = -1;
    if (hd[6]) {
        if (!get(in, hc[0].data(), tn * 8) || !get(in, hs[0].data(), tn * 16)) { fprintf(stderr, "upsample_host: short history\n"); return 2; }
        cur_hist = 0;
    }
    std::vector<uint32_t> color(n), normal(n), resolved(tn);
    std::vector<rp_u4> position(n);
    std::vector<float> motion(2 * tn);
    for (int f = 0; f < frames; f++) {
        vrt_push cur, prev;
        if (!get(in, &cur, sizeof cur) || !get(in, &prev, sizeof prev) || !get(in, color.data(), n * 4) || !get(in, position.data(), n * 16) ||
            !get(in, normal.data(), n * 4)) { fprintf(stderr, "upsample_host: short frame %d\n", f); return 2; }
        const float tol_rel = tl[1] < 0.0f ? reproject_default_tol_rel(cur.cam_right, w) : tl[1];
        UpsampleConsts k;
        const int32_t rc = upsample_consts(w, h, TW, TH, cur.cam_pos, cur.cam_dir, cur.cam_right, cur.cam_up, prev.cam_pos, prev.cam_dir,
                                           prev.cam_right, prev.cam_up, tl[0], tol_rel, max_history, k);
        if (!put(out, &rc, 4)) return 2;
        if (rc != 0) break;
        const int nxt = cur_hist >= 0 ? 1 - cur_hist : 0;
        const rp_u4* hin_s = cur_hist >= 0 ? hs[cur_hist].data() : nullptr;
        const rp_u2* hin_c = cur_hist >= 0 ? hc[cur_hist].data() : nullptr;
        for (int Y = 0; Y < TH; Y++)
            for (int X = 0; X < TW; X++) {
                int rx, ry;
                upsample_source(k, X, Y, rx, ry);
                const size_t j = (size_t)ry * w + rx, i = (size_t)Y * TW + X;
                ReprojectPixel o;
                upsample_pixel(k, X, Y, position[j], normal[j], color[j], hin_s, hin_c, o);
                hc[nxt][i] = o.color16; hs[nxt][i] = o.surface; resolved[i] = o.resolved;
                motion[2 * i] = o.mvx; motion[2 * i + 1] = o.mvy;
            }
        cur_hist = nxt;
        if (!put(out, hc[nxt].data(), tn * 8) || !put(out, hs[nxt].data(), tn * 16) || ((hd[7] & 1) && !put(out, resolved.data(), tn * 4)) ||
            ((hd[7] & 2) && !put(out, motion.data(), tn * 8))) return 2;
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
