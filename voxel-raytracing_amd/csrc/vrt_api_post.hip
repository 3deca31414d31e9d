// vrt_api_post.hip -- what the C-ABI does with rendered images: the denoiser stage, strip packing, presentation (blit, accumulate,
// resolve), temporal reprojection and temporal upsampling (push blocks and ray cameras each).  Host code only; the kernels are
// vrt_denoise.hip, vrt_post.hip, vrt_reproject.hip, vrt_reproject_cam.hip, vrt_upsample.hip and vrt_upsample_cam.hip.
//
// vrt_reproject, vrt_reproject_camera, vrt_upsample and vrt_upsample_camera state their common argument rules once, in file-local helpers: temporal_null,
// temporal_defaults / temporal_settings, temporal_planes (overlap, then alignment) and temporal_fill (the parameter block's pointers).
//
// Call surface mirrored from the reference (paths relative to its root):
//   DenoiserStage::record      source/voxels/stages/denoiser_stage.cpp:143-154,156-258
#include <cmath>
#include <cstring>

#include "vrt_host.h"
#include "vrt_denoise_bound.h"
#include "vrt_reproject_cam.h"
#include "vrt_upsample_cam.h"

using namespace vrt;

// ---- denoiser stage --------------------------------------------------------------------------------

static int tap_reach(const vrt_denoiser_settings* ds, int pass)
{
    float sw = (float)pass * ds->step_width + 1.0f;         // denoiser_stage.cpp:151
    int r = (int)sw; if ((float)r < sw) r++;
    return r;
}

// The guard of pass `pass` (vrt_denoise_bound.h), from the pass' parameters as vrt_denoise makes them
static double pass_guard(const vrt_denoiser_settings* ds, int pass)
{
    if (pass == 0) return denoise_guard_pass0();               // pass 0: a plain blur, tap offset 1
    const float inv = 1.0f / (float)pass;
    return denoise_guard((double)(inv * ds->phi_color0), (double)(inv * ds->phi_normal0), (double)(inv * ds->phi_pos0),
                         (double)((float)pass * ds->step_width + 1.0f), (ds->mode & 1) == VRT_DENOISE_AS_SHIPPED);
}

extern "C" {

int vrt_denoise_halo_rows(const vrt_denoiser_settings* ds)
{
    if (!ds) return 0;
    int h = 0;
    for (int i = 0; i < ds->iterations; i++) h += tap_reach(ds, i);
    return h;
}

int vrt_denoise(vrt_ctx* c, int32_t W, int32_t H, const vrt_denoiser_settings* ds,
                const uint8_t* color_in, const int8_t* normal8, const float* position,
                uint8_t* target0, uint8_t* target1, const vrt_shard* shard, const uint8_t** result)
{
    if (!c || !ds || !color_in || !normal8 || !position || !result) return fail(VRT_ERR_INVALID, "vrt_denoise: NULL argument");
    if (ds->iterations < 0 || ds->iterations > 10) return fail(VRT_ERR_INVALID, "vrt_denoise: iterations must be in 0..10 (MAX_DENOISER_PASSES)");
    if (ds->mode < 0 || ds->mode > 3) return fail(VRT_ERR_INVALID, "vrt_denoise: mode must be VRT_DENOISE_CANONICAL or _AS_SHIPPED, optionally | VRT_DENOISE_FAST");
    if (ds->iterations > 0 && !target0) return fail(VRT_ERR_INVALID, "vrt_denoise: target0 is NULL");
    if (ds->iterations > 1 && !target1) return fail(VRT_ERR_INVALID, "vrt_denoise: target1 is NULL");
    if (!(ds->phi_color0 > 0.0f) || !(ds->phi_normal0 > 0.0f) || !(ds->phi_pos0 > 0.0f))
        return fail(VRT_ERR_INVALID, "vrt_denoise: phi parameters must be > 0 (SURVEY 9.4-E)");
    if (!(ds->step_width >= 0.0f)) return fail(VRT_ERR_INVALID, "vrt_denoise: step_width must be >= 0");
    if (W <= 0 || H <= 0) return fail(VRT_ERR_INVALID, "vrt_denoise: bad size");
    HIPCHK(hipSetDevice(c->device));
    {
        const void* ptrs[5] = {color_in, normal8, position, target0, target1};
        int prc = check_device_ptrs(c, 1, ptrs, 5, "vrt_denoise");
        if (prc != VRT_OK) return prc;
    }
    DenoiseParams p;
    memset(&p, 0, sizeof p);
    int rc = make_shard(shard, H, p.sh, nullptr);
    if (rc != VRT_OK) return rc;
    p.normal = normal8; p.position = position; p.W = W; p.H = H; p.mode = ds->mode;
    p.tile16 = c->opt.denoise_th16; p.no_packed = c->opt.denoise_packed ? 0 : 1;
    p.no_pair = c->opt.denoise_pair ? 0 : 1; p.no_p0 = c->opt.denoise_p0 ? 0 : 1; p.pair_wgs = c->opt.denoise_pair_wgs;
    uint8_t* targets[2] = {target0, target1};
    const uint8_t* last = color_in;
    // which passes take the verified form (an integral tap offset, a guard worth having)
    double guards[10];
    bool any_verified = false;
    c->den_last_passes = 0;
    for (int i = 0; i < ds->iterations; i++) {
        guards[i] = INFINITY;
        if (!c->opt.denoise_verified || (size_t)W * (size_t)H >= (1u << 28)) continue;
        guards[i] = pass_guard(ds, i);
        if (i == 0 || guards[i] <= kDenGuardMax) any_verified = true;
    }
    const bool counting = any_verified && !(ds->mode & VRT_DENOISE_FAST) && c->opt.denoise_count;
    if (counting) {
        if (!c->den_counts) HIPCHK(c->den_counts.alloc(10 * VRT_DENOISE_SEGS * sizeof(uint32_t)));
        HIPCHK(hipMemsetAsync(c->den_counts.get(), 0, (size_t)ds->iterations * VRT_DENOISE_SEGS * sizeof(uint32_t), c->stream));
    }
    if (c->timing) HIPCHK(hipEventRecord(c->ev_den0, c->stream));
    for (int i = 0; i < ds->iterations; i++) {                 // denoiser_stage.cpp:204-255
        int ping = i % 2;
        float inv = 1.0f / (float)i;                           // pass 0: +inf (denoiser_stage.cpp:148-150)
        p.phi_color = inv * ds->phi_color0;
        p.phi_normal = inv * ds->phi_normal0;
        p.phi_pos = inv * ds->phi_pos0;
        p.step_width = (float)i * ds->step_width + 1.0f;
        {
            const float log2e = 1.44269504088896341f;
            p.kc = log2e / p.phi_color; p.kp = log2e / p.phi_pos; p.kn = log2e / (p.phi_normal * (p.step_width * p.step_width));   // pass 0: all 0
            {
                const float sw2 = p.step_width * p.step_width;
                auto ok = [](float v) { return v >= 0x1p-20f && v <= 0x1p20f; };
                p.packed_ok = (ok(p.phi_color) && ok(p.phi_normal) && ok(p.phi_pos) && ok(sw2)) ? 1 : 0;
                p.rc = 1.0f / p.phi_color; p.rn = 1.0f / p.phi_normal; p.rp = 1.0f / p.phi_pos; p.rs = 1.0f / sw2;
            }
        }
        p.verified = 0;
        if (guards[i] <= kDenGuardMax) {
            const double log2e = 1.4426950408889634;
            const double sw = (double)p.step_width;
            p.vkc = (float)(log2e / ((double)p.phi_color * 255.0 * 255.0));
            p.vkn = (float)(log2e / ((double)p.phi_normal * sw * sw * 127.0 * 127.0));
            p.vkp = (float)(log2e / (double)p.phi_pos);
            const double g = c->opt.denoise_guard_div8 ? guards[i] * 0.125 : guards[i];
            p.guard = std::nextafterf((float)g, 1.0f);
            p.fix_counts = counting ? c->den_counts.get() + (size_t)i * VRT_DENOISE_SEGS : nullptr;
            p.verified = 1;
            if (counting) c->den_last_passes |= 1 << i;
        }
        p.color_in = last; p.color_out = targets[ping];
        int ext = 0;
        if (p.sh.nranks > 1) for (int j = i + 1; j < ds->iterations; j++) ext += tap_reach(ds, j);
        p.extend = ext;
        if (p.sh.n_local_strips > 0) HIPCHK(launch_denoise_pass(p, c->stream));
        last = targets[ping];
    }
    if (c->timing) { HIPCHK(hipEventRecord(c->ev_den1, c->stream)); c->have_den = true; }
    *result = last;
    return VRT_OK;
}

int vrt_denoise_guard(const vrt_denoiser_settings* ds, int32_t pass, float* guard)
{
    if (!ds || !guard) return fail(VRT_ERR_INVALID, "vrt_denoise_guard: NULL argument");
    if (pass < 0 || pass > 9) return fail(VRT_ERR_INVALID, "vrt_denoise_guard: pass must be 0..9");
    *guard = (float)pass_guard(ds, pass);
    return VRT_OK;
}

int vrt_debug_denoise_redone(vrt_ctx* c, int32_t pass, uint32_t* pixels)
{
    if (!c || !pixels) return fail(VRT_ERR_INVALID, "vrt_debug_denoise_redone: NULL argument");
    if (pass < 0 || pass > 9) return fail(VRT_ERR_INVALID, "vrt_debug_denoise_redone: pass must be 0..9");
    *pixels = 0;
    if (!(c->den_last_passes & (1 << pass)) || !c->den_counts) return VRT_OK;      // the pass did not take the verified form
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    uint32_t counts[VRT_DENOISE_SEGS];
    HIPCHK(hipMemcpy(counts, c->den_counts.get() + (size_t)pass * VRT_DENOISE_SEGS, sizeof counts, hipMemcpyDeviceToHost));
    uint64_t n = 0;
    for (uint32_t v : counts) n += v;
    *pixels = (uint32_t)n;
    return VRT_OK;
}

// ---- strip packing ---------------------------------------------------------------------------------

static int rows_call(vrt_ctx* c, const void* src, void* dst, int W, int H, int bpp, const vrt_shard* sh,
                     int halo, int dir, int unpack)
{
    if (!c || !src || !dst) return fail(VRT_ERR_INVALID, "strip copy: NULL argument");
    if (W <= 0 || H <= 0 || bpp <= 0 || halo < 0) return fail(VRT_ERR_INVALID, "strip copy: bad size");
    HIPCHK(hipSetDevice(c->device));
    RowsParams p;
    memset(&p, 0, sizeof p);
    int mx = 1;
    int rc = make_shard(sh, H, p.sh, &mx);
    if (rc != VRT_OK) return rc;
    if (halo > p.sh.strip_rows) return fail(VRT_ERR_INVALID, "strip copy: halo larger than strip_rows");
    p.src = (const uint8_t*)src; p.dst = (uint8_t*)dst; p.W = W; p.H = H; p.bpp = bpp;
    p.halo = halo; p.dir = dir; p.unpack = unpack;
    int rows = halo ? mx * halo : (p.sh.nranks == 1 ? H : mx * p.sh.strip_rows);
    HIPCHK(launch_rows(p, rows, c->stream));
    return VRT_OK;
}

int vrt_pack_rows(vrt_ctx* c, const void* full, void* packed, int32_t W, int32_t H, int32_t bpp, const vrt_shard* sh)
{ return rows_call(c, full, packed, W, H, bpp, sh, 0, 0, 0); }

int vrt_unpack_rows(vrt_ctx* c, const void* packed, void* full, int32_t W, int32_t H, int32_t bpp, const vrt_shard* sh)
{ return rows_call(c, packed, full, W, H, bpp, sh, 0, 0, 1); }

int vrt_pack_halo(vrt_ctx* c, const void* full, void* packed, int32_t W, int32_t H, int32_t bpp,
                  const vrt_shard* sh, int32_t halo, int32_t dir)
{
    if (halo <= 0 || (dir != -1 && dir != 1)) return fail(VRT_ERR_INVALID, "vrt_pack_halo: halo > 0 and dir = +-1 required");
    return rows_call(c, full, packed, W, H, bpp, sh, halo, dir, 0);
}

int vrt_unpack_halo(vrt_ctx* c, const void* packed, void* full, int32_t W, int32_t H, int32_t bpp,
                    const vrt_shard* sh, int32_t halo, int32_t dir)
{
    if (halo <= 0 || (dir != -1 && dir != 1)) return fail(VRT_ERR_INVALID, "vrt_unpack_halo: halo > 0 and dir = +-1 required");
    return rows_call(c, packed, full, W, H, bpp, sh, halo, dir, 1);
}

// n images per launch (chunks of VRT_ROWS_BATCH).  shards: one map for all images (per_image == 0) or one per image.
static int rows_batch_call(vrt_ctx* c, int n, const void* const* src, void* const* dst, int W, int H, int bpp,
                           const vrt_shard* shards, int per_image, int unpack, int halo = 0, int dir = 0)
{
    if (!c || !src || !dst) return fail(VRT_ERR_INVALID, "strip copy (batch): NULL argument");
    if (n < 0 || W <= 0 || H <= 0 || bpp <= 0) return fail(VRT_ERR_INVALID, "strip copy (batch): bad size");
    // every argument of every image before the first launch: a refused call has copied nothing
    for (int i = 0; i < n; i++) {
        if (!src[i] || !dst[i]) return fail(VRT_ERR_INVALID, "strip copy (batch): NULL image pointer");
        ShardMap sm;
        int rc = make_shard(per_image ? &shards[i] : shards, H, sm, nullptr);
        if (rc != VRT_OK) return rc;
        if (halo > sm.strip_rows) return fail(VRT_ERR_INVALID, "strip copy (batch): halo larger than strip_rows");
    }
    HIPCHK(hipSetDevice(c->device));
    for (int i0 = 0; i0 < n;) {
        RowsBatchParams p;
        memset(&p, 0, sizeof p);
        p.W = W; p.H = H; p.bpp = bpp; p.unpack = unpack; p.halo = halo; p.dir = dir;
        // A launch has one grid height, and a packing launch zero-fills the rows of an image that its strips do not reach: images
        // whose packed buffers differ in rows (another nranks or strip_rows) go into launches of their own, or the shorter
        // buffer would be written past its end.
        int rows = 0, m = 0;
        for (; m < VRT_ROWS_BATCH && i0 + m < n; m++) {
            ShardMap sm;
            int mx = 1;
            int rc = make_shard(per_image ? &shards[i0 + m] : shards, H, sm, &mx);
            if (rc != VRT_OK) return rc;
            const int r = halo ? mx * halo : (sm.nranks == 1 ? H : mx * sm.strip_rows);
            if (m > 0 && r != rows) break;
            rows = r;
            p.sh[m] = sm; p.src[m] = (const uint8_t*)src[i0 + m]; p.dst[m] = (uint8_t*)dst[i0 + m];
        }
        HIPCHK(launch_rows_batch(p, rows, m, c->stream));
        i0 += m;
    }
    return VRT_OK;
}

int vrt_pack_rows_batch(vrt_ctx* c, int32_t n, const void* const* full, void* const* packed, int32_t W, int32_t H, int32_t bpp,
                        const vrt_shard* shard)
{ return rows_batch_call(c, n, full, packed, W, H, bpp, shard, 0, 0); }

int vrt_unpack_rows_batch(vrt_ctx* c, int32_t n, const void* const* packed, void* const* full, int32_t W, int32_t H, int32_t bpp,
                          const vrt_shard* shards)
{
    if (!shards) return fail(VRT_ERR_INVALID, "vrt_unpack_rows_batch: one vrt_shard per image is required");
    return rows_batch_call(c, n, packed, full, W, H, bpp, shards, 1, 1);
}

int vrt_pack_halo_batch(vrt_ctx* c, int32_t n, const void* const* full, void* const* packed, int32_t W, int32_t H, int32_t bpp,
                        const vrt_shard* shards, int32_t halo, int32_t dir)
{
    if (!shards) return fail(VRT_ERR_INVALID, "vrt_pack_halo_batch: one vrt_shard per image is required");
    if (halo <= 0 || (dir != -1 && dir != 1)) return fail(VRT_ERR_INVALID, "vrt_pack_halo_batch: halo > 0 and dir = +-1 required");
    return rows_batch_call(c, n, full, packed, W, H, bpp, shards, 1, 0, halo, dir);
}

int vrt_unpack_halo_batch(vrt_ctx* c, int32_t n, const void* const* packed, void* const* full, int32_t W, int32_t H, int32_t bpp,
                          const vrt_shard* shards, int32_t halo, int32_t dir)
{
    if (!shards) return fail(VRT_ERR_INVALID, "vrt_unpack_halo_batch: one vrt_shard per image is required");
    if (halo <= 0 || (dir != -1 && dir != 1)) return fail(VRT_ERR_INVALID, "vrt_unpack_halo_batch: halo > 0 and dir = +-1 required");
    return rows_batch_call(c, n, packed, full, W, H, bpp, shards, 1, 1, halo, dir);
}

size_t vrt_halo_bytes(int32_t W, int32_t H, int32_t bpp, const vrt_shard* sh, int32_t halo)
{
    ShardMap m; int mx = 1;
    if (make_shard(sh, H, m, &mx) != VRT_OK) return 0;
    return (size_t)mx * (size_t)halo * (size_t)W * (size_t)bpp;
}

// ---- presentation / temporal helpers ---------------------------------------------------------------

int vrt_blit(vrt_ctx* c, const void* src_rgba8, int32_t sw, int32_t sh, void* dst_rgba8, int32_t tw, int32_t th)
{
    if (!c || !src_rgba8 || !dst_rgba8) return fail(VRT_ERR_INVALID, "vrt_blit: NULL argument");
    if (sw <= 0 || sh <= 0 || tw <= 0 || th <= 0) return fail(VRT_ERR_INVALID, "vrt_blit: bad size");
    if (src_rgba8 == dst_rgba8) return fail(VRT_ERR_INVALID, "vrt_blit: source and target must differ");
    HIPCHK(hipSetDevice(c->device));
    BlitParams p;
    p.src = (const uint8_t*)src_rgba8; p.dst = (uint8_t*)dst_rgba8; p.sw = sw; p.sh = sh; p.tw = tw; p.th = th;
    HIPCHK(launch_blit(p, c->stream));
    return VRT_OK;
}

int vrt_accumulate(vrt_ctx* c, const void* color_rgba8, void* accum_u32, int32_t W, int32_t H, int32_t reset)
{
    if (!c || !color_rgba8 || !accum_u32) return fail(VRT_ERR_INVALID, "vrt_accumulate: NULL argument");
    if (W <= 0 || H <= 0) return fail(VRT_ERR_INVALID, "vrt_accumulate: bad size");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(launch_accumulate(color_rgba8, accum_u32, (size_t)W * (size_t)H, reset != 0, c->stream));
    return VRT_OK;
}

int vrt_resolve(vrt_ctx* c, const void* accum_u32, void* out_rgba8, int32_t W, int32_t H, uint32_t frames)
{
    if (!c || !accum_u32 || !out_rgba8) return fail(VRT_ERR_INVALID, "vrt_resolve: NULL argument");
    if (W <= 0 || H <= 0) return fail(VRT_ERR_INVALID, "vrt_resolve: bad size");
    if (frames == 0 || frames > (1u << 22)) return fail(VRT_ERR_INVALID, "vrt_resolve: frames must be in 1..2^22");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(launch_resolve(accum_u32, out_rgba8, (size_t)W * (size_t)H, frames, c->stream));
    return VRT_OK;
}

} // extern "C"

// ---- the temporal passes: what vrt_reproject, vrt_reproject_camera, vrt_upsample and vrt_upsample_camera share ----
// Each check takes the entry point's name for its message and returns VRT_OK or what fail() returned.  An entry point applies them
// in this order, between its own rules: temporal_null, (its size rules), temporal_settings, (its constants), temporal_planes --
// and only then looks at the context.

// The seven plane arguments of a temporal pass.  The three current planes hold one texel per pixel of the frame; the histories,
// resolved8 and motion one per texel of the history (the same count, but for the two upsampling passes)
struct TemporalPlanes {
    const uint8_t* color8; const float* position; const int8_t* normal8;
    const vrt_history* history_in; const vrt_history* history_out; uint8_t* resolved8; float* motion;
};

static int temporal_null(const char* fn, const vrt_ctx* c, const void* cur, const void* prev, const TemporalPlanes& pl)
{
    if (!c || !cur || !prev || !pl.color8 || !pl.position || !pl.normal8 || !pl.history_out || !pl.history_out->color16 ||
        !pl.history_out->surface || (pl.history_in && (!pl.history_in->color16 || !pl.history_in->surface)))
        return fail(VRT_ERR_INVALID, std::string(fn) + ": NULL argument");
    return VRT_OK;
}

// the default settings, given the default tol_rel of the camera they are for
static void temporal_defaults(float tol_rel, vrt_reproject_settings* s) { s->max_history = 32; s->tol_abs = 0.5f; s->tol_rel = tol_rel; }

// st: the caller's settings, or the defaults; then the rules for either
static int temporal_settings(const char* fn, const vrt_reproject_settings* settings, float default_tol_rel, vrt_reproject_settings& st)
{
    if (settings) st = *settings;
    else temporal_defaults(default_tol_rel, &st);
    if (st.max_history < 1u || st.max_history > 255u) return fail(VRT_ERR_INVALID, std::string(fn) + ": max_history must be in 1..255");
    if (!(st.tol_abs >= 0.0f) || !(st.tol_rel >= 0.0f) || !rp_finite(st.tol_abs) || !rp_finite(st.tol_rel))
        return fail(VRT_ERR_INVALID, std::string(fn) + ": a tolerance is negative or not finite");
    return VRT_OK;
}

// No output overlaps another plane, then every plane is aligned to its texel: over a frame of n texels and a history of tn
static int temporal_planes(const char* fn, const TemporalPlanes& pl, size_t n, size_t tn)
{
    const vrt_history* hin = pl.history_in;
    const vrt_history* hout = pl.history_out;
    struct Range { const char* lo; size_t bytes; bool out; };
    const Range rg[9] = {
        {(const char*)pl.color8, n * 4, false}, {(const char*)pl.position, n * 16, false}, {(const char*)pl.normal8, n * 4, false},
        {hin ? (const char*)hin->color16 : nullptr, tn * 8, false}, {hin ? (const char*)hin->surface : nullptr, tn * 16, false},
        {(const char*)hout->color16, tn * 8, true}, {(const char*)hout->surface, tn * 16, true},
        {(const char*)pl.resolved8, tn * 4, true}, {(const char*)pl.motion, tn * 8, true}};
    for (int a = 0; a < 9; a++)
        for (int b = a + 1; b < 9; b++) {
            if (!rg[a].lo || !rg[b].lo || (!rg[a].out && !rg[b].out)) continue;
            if ((uintptr_t)rg[a].lo < (uintptr_t)rg[b].lo + rg[b].bytes && (uintptr_t)rg[b].lo < (uintptr_t)rg[a].lo + rg[a].bytes)
                return fail(VRT_ERR_INVALID, std::string(fn) + ": an output overlaps another buffer (the history is gathered: in and out must differ)");
        }
    if ((((uintptr_t)pl.position | (uintptr_t)hout->surface | (uintptr_t)(hin ? hin->surface : nullptr)) & 15u) != 0u ||
        (((uintptr_t)hout->color16 | (uintptr_t)(hin ? hin->color16 : nullptr) | (uintptr_t)pl.motion) & 7u) != 0u ||
        (((uintptr_t)pl.color8 | (uintptr_t)pl.normal8 | (uintptr_t)pl.resolved8) & 3u) != 0u)
        return fail(VRT_ERR_INVALID, std::string(fn) + ": a plane is not aligned to its texel size");
    return VRT_OK;
}

// the nine pointer members of ReprojectParams / UpsampleParams
template <class Params>
static void temporal_fill(Params& p, const TemporalPlanes& pl)
{
    p.color8 = (const uint32_t*)pl.color8; p.position = (const rp_u4*)pl.position; p.normal8 = (const uint32_t*)pl.normal8;
    p.hist_color = pl.history_in ? (const rp_u2*)pl.history_in->color16 : nullptr;
    p.hist_surface = pl.history_in ? (const rp_u4*)pl.history_in->surface : nullptr;
    p.out_color = (rp_u2*)pl.history_out->color16; p.out_surface = (rp_u4*)pl.history_out->surface;
    p.resolved8 = (uint32_t*)pl.resolved8; p.motion = pl.motion;
}

extern "C" {

// ---- temporal reprojection (csrc/vrt_reproject.h is the definition, vrt_reproject.hip the kernel) ----

void vrt_reproject_settings_default(const vrt_push* cur, vrt_reproject_settings* s)
{
    if (s) temporal_defaults((cur && cur->screen_size[0] > 0) ? reproject_default_tol_rel(cur->cam_right, cur->screen_size[0]) : 0.0f, s);
}

int vrt_history_bytes(int32_t W, int32_t H, size_t* color16, size_t* surface)
{
    if (W <= 0 || H <= 0 || W > 32768 || H > 32768) return fail(VRT_ERR_INVALID, "vrt_history_bytes: bad size");
    const size_t n = (size_t)W * (size_t)H;
    if (color16) *color16 = n * 8;
    if (surface) *surface = n * 16;
    return VRT_OK;
}

int vrt_reproject(vrt_ctx* c, int32_t W, int32_t H, const vrt_push* cur, const vrt_push* prev, const vrt_reproject_settings* settings,
                  const uint8_t* color8, const float* position, const int8_t* normal8, const vrt_history* history_in,
                  const vrt_history* history_out, uint8_t* resolved8, float* motion)
{
    // every argument error is reported before the context or a device is looked at
    static const char fn[] = "vrt_reproject";
    const TemporalPlanes pl{color8, position, normal8, history_in, history_out, resolved8, motion};
    if (int rc = temporal_null(fn, c, cur, prev, pl)) return rc;
    if (W <= 0 || H <= 0 || W > 32768 || H > 32768) return fail(VRT_ERR_INVALID, "vrt_reproject: bad frame size");
    if ((int64_t)W * (int64_t)H >= ((int64_t)1 << 28))
        return fail(VRT_ERR_UNSUPPORTED, "vrt_reproject: 2^28 pixels or more per frame (the limit of vrt_render_geometry)");
    vrt_reproject_settings st;
    if (int rc = temporal_settings(fn, settings, reproject_default_tol_rel(cur->cam_right, W), st)) return rc;
    ReprojectParams p;
    if (!reproject_consts(W, H, prev->cam_pos, prev->cam_dir, prev->cam_right, prev->cam_up, prev->camera_jitter, cur->cam_pos,
                          st.tol_abs, st.tol_rel, st.max_history, p.k))
        return fail(VRT_ERR_INVALID, "vrt_reproject: the previous camera's basis is degenerate (zero or non-finite determinant)");
    const size_t n = (size_t)W * (size_t)H;
    if (int rc = temporal_planes(fn, pl, n, n)) return rc;
    temporal_fill(p, pl);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(launch_reproject(p, c->stream));
    return VRT_OK;
}

// ---- temporal reprojection for ray cameras (csrc/vrt_reproject_cam.h is the definition, vrt_reproject_cam.hip the kernel) ----

void vrt_reproject_camera_settings_default(const vrt_ray_camera* cur, int32_t W, vrt_reproject_settings* s)
{
    if (s) temporal_defaults(cur ? reproject_cam_default_tol_rel(*cur, W) : 0.0f, s);
}

int vrt_reproject_camera(vrt_ctx* c, int32_t W, int32_t H, const vrt_ray_camera* cur, const vrt_ray_camera* prev,
                         const vrt_reproject_settings* settings, const uint8_t* color8, const float* position,
                         const int8_t* normal8, const vrt_history* history_in, const vrt_history* history_out, uint8_t* resolved8,
                         float* motion)
{
    // every argument error is reported before the context or a device is looked at
    static const char fn[] = "vrt_reproject_camera";
    const TemporalPlanes pl{color8, position, normal8, history_in, history_out, resolved8, motion};
    if (int rc = temporal_null(fn, c, cur, prev, pl)) return rc;
    if (W <= 0 || H <= 0 || W > 32768 || H > 32768) return fail(VRT_ERR_INVALID, "vrt_reproject_camera: bad frame size");
    if ((int64_t)W * (int64_t)H >= ((int64_t)1 << 28))
        return fail(VRT_ERR_UNSUPPORTED, "vrt_reproject_camera: 2^28 pixels or more per frame (the limit of vrt_render_geometry)");
    vrt_reproject_settings st;
    if (int rc = temporal_settings(fn, settings, reproject_cam_default_tol_rel(*cur, W), st)) return rc;
    ReprojectCamConsts ck;
    switch (reproject_cam_consts(W, H, *cur, *prev, st.tol_abs, st.tol_rel, st.max_history, ck)) {
    case 0: break;
    case 1: return fail(VRT_ERR_INVALID, "vrt_reproject_camera: the current and the previous camera are of different models");
    case 2: return fail(VRT_ERR_INVALID, "vrt_reproject_camera: the current camera is not one vrt_camera_rays accepts (unknown model, bad tan_half / half_width, degenerate basis, non-finite position or jitter)");
    case 3: return fail(VRT_ERR_INVALID, "vrt_reproject_camera: the previous camera is not one vrt_camera_rays accepts (unknown model, bad tan_half / half_width, degenerate basis, non-finite position or jitter)");
    default: return fail(VRT_ERR_INVALID, "vrt_reproject_camera: the previous camera's basis is degenerate (zero or non-finite determinant)");
    }
    const size_t n = (size_t)W * (size_t)H;
    if (int rc = temporal_planes(fn, pl, n, n)) return rc;
    ReprojectParams p; p.k = ck.k;
    temporal_fill(p, pl);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(launch_reproject_cam(ck.model, p, c->stream));
    return VRT_OK;
}

// ---- temporal upsampling (csrc/vrt_upsample.h is the definition, vrt_upsample.hip the kernel) ----

int vrt_upsample(vrt_ctx* c, int32_t w, int32_t h, int32_t TW, int32_t TH, const vrt_push* cur, const vrt_push* prev,
                 const vrt_reproject_settings* settings, const uint8_t* color8, const float* position, const int8_t* normal8,
                 const vrt_history* history_in, const vrt_history* history_out, uint8_t* resolved8, float* motion)
{
    // every argument error is reported before the context or a device is looked at
    static const char fn[] = "vrt_upsample";
    const TemporalPlanes pl{color8, position, normal8, history_in, history_out, resolved8, motion};
    if (int rc = temporal_null(fn, c, cur, prev, pl)) return rc;
    if (w <= 0 || h <= 0 || TW <= 0 || TH <= 0 || TW > 32768 || TH > 32768) return fail(VRT_ERR_INVALID, "vrt_upsample: bad frame size");
    if (TW < w || TH < h) return fail(VRT_ERR_INVALID, "vrt_upsample: the display size is smaller than the render size");
    if ((int64_t)TW * (int64_t)TH >= ((int64_t)1 << 28))
        return fail(VRT_ERR_UNSUPPORTED, "vrt_upsample: 2^28 pixels or more per frame (the limit of vrt_render_geometry)");
    if (cur->screen_size[0] != w || cur->screen_size[1] != h || prev->screen_size[0] != w || prev->screen_size[1] != h)
        return fail(VRT_ERR_INVALID, "vrt_upsample: screen_size of a push block is not the render size (w, h)");
    vrt_reproject_settings st;
    if (int rc = temporal_settings(fn, settings, reproject_default_tol_rel(cur->cam_right, w), st)) return rc;
    UpsampleParams p;
    const int bad = upsample_consts(w, h, TW, TH, cur->cam_pos, cur->cam_dir, cur->cam_right, cur->cam_up, prev->cam_pos, prev->cam_dir,
                                    prev->cam_right, prev->cam_up, st.tol_abs, st.tol_rel, st.max_history, p.k);
    if (bad) return fail(VRT_ERR_INVALID, bad == 1 ? "vrt_upsample: the current camera's basis is degenerate (zero or non-finite determinant)"
                                                   : "vrt_upsample: the previous camera's basis is degenerate (zero or non-finite determinant)");
    if (int rc = temporal_planes(fn, pl, (size_t)w * (size_t)h, (size_t)TW * (size_t)TH)) return rc;
    temporal_fill(p, pl);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(launch_upsample(p, c->stream));
    return VRT_OK;
}

// ---- temporal upsampling for ray cameras (csrc/vrt_upsample_cam.h is the definition, vrt_upsample_cam.hip the kernel) ----

void vrt_upsample_camera_settings_default(const vrt_ray_camera* cur, int32_t w, vrt_reproject_settings* s)
{
    if (s) temporal_defaults(cur ? reproject_cam_default_tol_rel(*cur, w) : 0.0f, s);
}

int vrt_upsample_camera(vrt_ctx* c, int32_t w, int32_t h, int32_t TW, int32_t TH, const vrt_ray_camera* cur, const vrt_ray_camera* prev,
                        const vrt_reproject_settings* settings, const uint8_t* color8, const float* position, const int8_t* normal8,
                        const vrt_history* history_in, const vrt_history* history_out, uint8_t* resolved8, float* motion)
{
    // every argument error is reported before the context or a device is looked at
    static const char fn[] = "vrt_upsample_camera";
    const TemporalPlanes pl{color8, position, normal8, history_in, history_out, resolved8, motion};
    if (int rc = temporal_null(fn, c, cur, prev, pl)) return rc;
    if (w <= 0 || h <= 0 || TW <= 0 || TH <= 0 || TW > 32768 || TH > 32768) return fail(VRT_ERR_INVALID, "vrt_upsample_camera: bad frame size");
    if (TW < w || TH < h) return fail(VRT_ERR_INVALID, "vrt_upsample_camera: the display size is smaller than the render size");
    if ((int64_t)TW * (int64_t)TH >= ((int64_t)1 << 28))
        return fail(VRT_ERR_UNSUPPORTED, "vrt_upsample_camera: 2^28 pixels or more per frame (the limit of vrt_render_geometry)");
    vrt_reproject_settings st;
    if (int rc = temporal_settings(fn, settings, reproject_cam_default_tol_rel(*cur, w), st)) return rc;
    UpsampleCamConsts ck;
    switch (upsample_cam_consts(w, h, TW, TH, *cur, *prev, st.tol_abs, st.tol_rel, st.max_history, ck)) {
    case 0: break;
    case 1: return fail(VRT_ERR_INVALID, "vrt_upsample_camera: the current and the previous camera are of different models");
    case 2: return fail(VRT_ERR_INVALID, "vrt_upsample_camera: the current camera is not one vrt_camera_rays accepts (unknown model, bad tan_half / half_width, degenerate basis, non-finite position or jitter)");
    case 3: return fail(VRT_ERR_INVALID, "vrt_upsample_camera: the previous camera is not one vrt_camera_rays accepts (unknown model, bad tan_half / half_width, degenerate basis, non-finite position or jitter)");
    case 4: return fail(VRT_ERR_INVALID, "vrt_upsample_camera: the current camera's basis is degenerate (zero or non-finite determinant)");
    default: return fail(VRT_ERR_INVALID, "vrt_upsample_camera: the previous camera's basis is degenerate (zero or non-finite determinant)");
    }
    if (int rc = temporal_planes(fn, pl, (size_t)w * (size_t)h, (size_t)TW * (size_t)TH)) return rc;
    UpsampleParams p; p.k = ck.k;
    temporal_fill(p, pl);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(launch_upsample_cam(ck.model, p, c->stream));
    return VRT_OK;
}

} // extern "C"
