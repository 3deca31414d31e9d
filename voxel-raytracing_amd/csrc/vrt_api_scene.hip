// vrt_api_scene.hip -- the scenes of the C-ABI, made, described and read: construction (dense and bricks), sky and noise, trim,
// memory, info, download, the loaders, read-back (a box, a box's non-empty voxels, the scene as a .vox file).  Host code only; the
// kernels are vrt_scene_build.hip and vrt_scene_read.hip.  What rewrites a scene is vrt_api_edit.hip.
//
// Call surface mirrored from the reference (paths relative to its root):
//   VoxelScene ctor            source/voxels/resource/voxel_scene.cpp:33-133
//   Engine::upload_submit      source/engine/engine.cpp:349-375 (blocking uploads)
#include <atomic>
#include <cstdio>
#include <cstring>
#include <memory>

#include "image_io.h"
#include "vox_reader.h"
#include "vox_writer.h"
#include "vrt_host.h"
#define VRT_SCENE_READ_LAUNCHERS
#include "vrt_scene_read.h"

using namespace vrt;

static std::atomic<uint64_t> g_shade_gen{0};

extern "C" {

void vrt_scene_free(vrt_ctx* c, vrt_scene* s)
{
    if (!s) return;
    if (c) { hipSetDevice(c->device); hipStreamSynchronize(c->stream); }
    delete s;                                                  // (frees the device buffers)
}

int vrt_scene_set_sky(vrt_ctx* c, vrt_scene* s, const float* rgba, uint32_t w, uint32_t h)
{
    if (!c || !s || !rgba || !w || !h) return fail(VRT_ERR_INVALID, "vrt_scene_set_sky: bad argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    DevBuf<float> d;
    size_t bytes = (size_t)w * h * 16;
    HIPCHK(d.alloc(bytes));
    HIPCHK(hipMemcpy(d.get(), rgba, bytes, hipMemcpyHostToDevice));
    DevBuf<uint32_t> d8;
    { hipError_t e8 = d8.alloc((size_t)w * h * 4); if (e8 != hipSuccess) return fail(VRT_ERR_HIP, std::string("hipMalloc (sky RGBA8): ") + hipGetErrorString(e8)); }
    s->sky = std::move(d); s->d.sky = s->sky.get(); s->d.sky_w = w; s->d.sky_h = h;
    // the sky as the colour target stores a miss, and the constants of the texel fast path (vrt_sky.h)
    s->sky8 = std::move(d8); s->d.sky8 = s->sky8.get(); s->d.skyk = sky_fast_consts(w, h);
    s->shade_gen = ++g_shade_gen;
    HIPCHK(launch_sky_rgba8(s->sky.get(), s->sky8.get(), (size_t)w * h, c->stream));
    // skyColor of the normals a hit can have (calcAmbient's sky tint, frag:224): 64 x float4, by the shading code itself
    if (!s->sky_normals) HIPCHK(s->sky_normals.alloc(64 * 4 * sizeof(float)));
    s->d.sky_normals = s->sky_normals.get();
    HIPCHK(launch_sky_normals(s->d, s->sky_normals.get(), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return VRT_OK;
}

int vrt_scene_set_blue_noise(vrt_ctx* c, vrt_scene* s, const uint8_t* rgba8, uint32_t w, uint32_t h)
{
    if (!c || !s || !rgba8 || !w || !h) return fail(VRT_ERR_INVALID, "vrt_scene_set_blue_noise: bad argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    DevBuf<uint8_t> d;
    size_t bytes = (size_t)w * h * 4;
    HIPCHK(d.alloc(bytes));
    HIPCHK(hipMemcpy(d.get(), rgba8, bytes, hipMemcpyHostToDevice));
    s->noise = std::move(d); s->d.noise = s->noise.get(); s->d.noise_w = w; s->d.noise_h = h;
    return VRT_OK;
}

} // extern "C"

// does any of the n voxel ids have a metallic material?  (decides whether the megakernel needs its bounce stack)
static bool any_metallic(const uint8_t* ids, size_t n, const vrt_material palette[256])
{
    bool metal[256], any = false;
    for (int i = 0; i < 256; i++) { metal[i] = palette[i].metallic > 0.0f; any = any || (i != 0 && metal[i]); }
    if (!any) return false;
    for (size_t i = 0; i < n; i++)
        if (ids[i] != 0 && metal[ids[i]]) return true;
    return false;
}

// A scene under construction: an early return frees it as vrt_scene_free does; release() hands it to the caller
struct SceneFree { vrt_ctx* c; void operator()(vrt_scene* s) const { vrt_scene_free(c, s); } };
typedef std::unique_ptr<vrt_scene, SceneFree> NewScene;

// The textures of a new scene: a white 1x1 sky and grey 1x1 noise
static int default_textures(vrt_ctx* c, vrt_scene* s)
{
    const float white[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    const uint8_t grey[4] = {128, 128, 128, 255};
    const int rc = vrt_scene_set_sky(c, s, white, 1, 1);
    return rc == VRT_OK ? vrt_scene_set_blue_noise(c, s, grey, 1, 1) : rc;
}

// The count planes' fields go; the next launch that asks for them builds them again
void vrt::drop_count_fields(vrt_scene* s)
{
    if (!s->df_counts) return;
    s->df_counts_raw.reset(); s->df_counts = nullptr;
    s->bytes -= s->df_bytes;
}

// The clearance fields of a dense scene into dst (df_bytes: eight fields, or nine and the 0xFF byte in trace_df_fast's layout),
// from the voxels already on the device; open: with the open cells coded 0 (launch_open_cells).  Returns when they are built.
hipError_t vrt::build_fields(vrt_ctx* c, const vrt_scene* s, uint8_t* dst, bool open)
{
    const VolumeView& d = s->d.vol;
    const size_t nvox = (size_t)d.W * (size_t)d.H * (size_t)d.D, ndf = df_field_bytes(d.W, d.H, d.D);
    hipError_t e = hipMemsetAsync(dst, 0, s->df_bytes, c->stream);
    if (e != hipSuccess) return e;
    if (d.df_fast) {
        if ((e = hipMemsetAsync(dst + 9 * ndf, 0xFF, 1, c->stream)) != hipSuccess) return e;
        if ((e = launch_pad_vox(s->vox.get(), d.W, d.H, d.D, dst + 8 * ndf, c->stream)) != hipSuccess) return e;
    }
    DevBuf<uint8_t> tmp0, tmp1;                                 // ping-pong buffers of the 3-pass transforms
    if ((e = tmp0.alloc(nvox)) != hipSuccess) return e;
    e = tmp1.alloc(nvox);
    if (e == hipSuccess) e = launch_build_df(s->vox.get(), d.W, d.H, d.D, dst, ndf, tmp0.get(), tmp1.get(), c->stream);
    if (e == hipSuccess && open) e = launch_open_cells(s->vox.get(), d.W, d.H, d.D, dst, ndf, tmp0.get(), tmp1.get(), c->stream);
    const hipError_t sync = hipStreamSynchronize(c->stream);
    return e != hipSuccess ? e : sync;
}

// The occupied 4^3 cells of a dense scene as a list (from the 16^3 summaries: one bit per cell), for the tile tags of a launch.
// Replaces the list the scene holds; above 4 << 20 cells the scene goes without (the tags then cost more than they save).
hipError_t vrt::build_cell_list(vrt_ctx* c, vrt_scene* s)
{
    const VolumeView& d = s->d.vol;
    if (s->cells) { s->cells.reset(); s->bytes -= (uint64_t)s->n_cells * 4; }
    s->n_cells = 0; s->cells_ok = false;
    if (d.n1x > 1024 || d.n1y > 1024 || d.n1z > 1024) return hipSuccess;
    const size_t n2 = (size_t)d.n2x * d.n2y * d.n2z;
    std::vector<uint64_t> h2(n2);
    hipError_t e = hipMemcpyAsync(h2.data(), s->occ2.get(), n2 * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return e;
    std::vector<uint32_t> cells;
    for (size_t w = 0; w < n2; w++) {
        uint64_t bits = h2[w];
        if (!bits) continue;
        const uint32_t wx = (uint32_t)(w % (size_t)d.n2x), wy = (uint32_t)((w / (size_t)d.n2x) % (size_t)d.n2y), wz = (uint32_t)(w / ((size_t)d.n2x * d.n2y));
        for (uint32_t b = 0; b < 64; b++)
            if ((bits >> b) & 1ull) cells.push_back((wx * 4u + (b & 3u)) | ((wy * 4u + ((b >> 2) & 3u)) << 10) | ((wz * 4u + (b >> 4)) << 20));
    }
    if (cells.size() > kMaxCells) return hipSuccess;
    if (!cells.empty()) {
        if ((e = s->cells.alloc(cells.size() * 4)) != hipSuccess) return e;
        if ((e = hipMemcpy(s->cells.get(), cells.data(), cells.size() * 4, hipMemcpyHostToDevice)) != hipSuccess) return e;
        s->bytes += cells.size() * 4;
    }
    s->n_cells = (uint32_t)cells.size();
    s->cells_ok = true;
    return hipSuccess;
}

// The fields a launch that writes count planes marches through (no open cells: the iterations of the reference's loop, to the
// wall), built on first use.
int vrt::fields_for_counts(vrt_ctx* c, const vrt_scene* cs, const uint8_t** out)
{
    vrt_scene* s = const_cast<vrt_scene*>(cs);
    std::lock_guard<std::mutex> lock(s->lazy);
    if (!s->open_cells) { *out = s->df; return VRT_OK; }
    if (!s->df_counts) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (uint64_t)s->df_bytes + 2ull * (uint64_t)s->d.vol.W * s->d.vol.H * s->d.vol.D > (uint64_t)free_b)
            return fail(VRT_ERR_UNSUPPORTED, "vrt_render_geometry: the count planes (steps_primary, steps_total) need a second set of clearance fields (" +
                        std::to_string((uint64_t)s->df_bytes) + " bytes), which does not fit the device memory that is free");
        DevBuf<uint8_t> p;
        HIPCHK(p.alloc(s->df_bytes + 2 * s->df_guard));
        hipError_t e = hipMemsetAsync(p.get(), 0, s->df_bytes + 2 * s->df_guard, c->stream);
        if (e == hipSuccess) e = build_fields(c, s, p.get() + s->df_guard, false);
        if (e != hipSuccess) return fail(VRT_ERR_HIP, std::string("building the count planes' clearance fields: ") + hipGetErrorString(e));
        s->df_counts_raw = std::move(p); s->df_counts = s->df_counts_raw.get() + s->df_guard;
        s->bytes += s->df_bytes;
    }
    *out = s->df_counts;
    return VRT_OK;
}

// a brick's entry in the cell list (its 8^3 cell) from its index in the padded grid
uint32_t vrt::brick_cell_code(uint32_t pc, int pbx, int pby)
{
    return (uint32_t)(pc % (uint32_t)pbx - 1u) | ((uint32_t)((pc / (uint32_t)pbx) % (uint32_t)pby - 1u) << 10) | ((uint32_t)(pc / ((uint32_t)pbx * (uint32_t)pby) - 1u) << 20);
}

extern "C" {

int vrt_scene_from_dense(vrt_ctx* c, const uint8_t* voxels, uint32_t W, uint32_t H, uint32_t D,
                         const vrt_material palette[256], vrt_scene** out)
{
    if (!c || !voxels || !palette || !out) return fail(VRT_ERR_INVALID, "vrt_scene_from_dense: NULL argument");
    if (!W || !H || !D || W > 4096 || H > 4096 || D > 4096)
        return fail(VRT_ERR_UNSUPPORTED, "vrt_scene_from_dense: each dimension must be in 1..4096");
    HIPCHK(hipSetDevice(c->device));
    NewScene hold(new vrt_scene(), SceneFree{c});
    vrt_scene* s = hold.get();
    s->shade_gen = ++g_shade_gen;
    VolumeView& d = s->d.vol;
    d.W = (int)W; d.H = (int)H; d.D = (int)D;
    d.n1x = ceil_div(d.W, 4); d.n1y = ceil_div(d.H, 4); d.n1z = ceil_div(d.D, 4);
    d.n2x = ceil_div(d.n1x, 4); d.n2y = ceil_div(d.n1y, 4); d.n2z = ceil_div(d.n1z, 4);
    d.n3x = ceil_div(d.n2x, 4); d.n3y = ceil_div(d.n2y, 4); d.n3z = ceil_div(d.n2z, 4);
    size_t nvox = (size_t)W * H * D;
    size_t n1 = (size_t)d.n1x * d.n1y * d.n1z, n2 = (size_t)d.n2x * d.n2y * d.n2z, n3 = (size_t)d.n3x * d.n3y * d.n3z;
    size_t n2pad = (n2 + 1) & ~(size_t)1;          // 16-byte multiples for the uint4 LDS staging loop
    size_t n3pad = (n3 + 1) & ~(size_t)1;
    size_t ndf = df_field_bytes(d.W, d.H, d.D);    // one clearance field: x-fastest with a one-voxel border of zeros
    {
        // the dense scene holds about 10x the voxel bytes (eight or nine clearance fields) and two more volumes while it is
        // built: say so up front instead of failing half way through the allocations
        const uint64_t need = (uint64_t)nvox * 3u + 9ull * ndf + (n1 + n2pad + n3pad) * 8ull + (64ull << 20);
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > (uint64_t)free_b)
            return fail(VRT_ERR_UNSUPPORTED, "vrt_scene_from_dense: a " + std::to_string(W) + "x" + std::to_string(H) + "x" + std::to_string(D) +
                        " dense scene needs " + std::to_string(need) + " bytes of device memory (" + std::to_string((uint64_t)free_b) +
                        " free); hand the volume over in bricks (vrt_scene_from_bricks)");
    }
    s->metallic_voxels = any_metallic(voxels, nvox, palette);
    for (int i = 1; i < 256; i++) s->metal[i] = palette[i].metallic > 0.0f;
    HIPCHK(s->vox.alloc(nvox));
    HIPCHK(s->occ1.alloc(n1 * 8));
    HIPCHK(s->occ2.alloc(n2pad * 8));
    HIPCHK(s->occ3.alloc(n3pad * 8));
    HIPCHK(s->palette.alloc(256 * sizeof(vrt_material)));
    // eight clearance fields, and -- while 32-bit offsets reach all of it -- a ninth field with the voxel ids in the same
    // layout plus one byte 0xFF behind it (trace_df_fast)
    {
        const bool fast = df_fast_layout_ok(d.W, d.H, d.D);
        const size_t bytes = fast ? 9 * ndf + 256 : 8 * ndf;
        s->df_guard = ((((size_t)W + 2u) * ((size_t)H + 2u)) * 2u + 511u) & ~(size_t)255u;
        HIPCHK(s->df_raw.alloc(bytes + 2 * s->df_guard));
        s->df = s->df_raw.get() + s->df_guard;
        HIPCHK(hipMemsetAsync(s->df_raw.get(), 0, bytes + 2 * s->df_guard, c->stream));
        s->df_bytes = bytes;
        s->bytes = (uint64_t)nvox + bytes + (n1 + n2pad + n3pad) * 8ull + 256 * sizeof(vrt_material);
        d.df_fast = fast ? 1u : 0u;
    }
    HIPCHK(hipMemsetAsync(s->occ2.get(), 0, n2pad * 8, c->stream));
    HIPCHK(hipMemsetAsync(s->occ3.get(), 0, n3pad * 8, c->stream));
    HIPCHK(hipMemcpyAsync(s->vox.get(), voxels, nvox, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->palette.get(), palette, 256 * sizeof(vrt_material), hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_build_pyramid(s->vox.get(), d.W, d.H, d.D, s->occ1.get(), s->occ2.get(), s->occ3.get(), c->stream));
    // the occupied 4^3 cells as a list, for the tile tags of a launch
    HIPCHK(build_cell_list(c, s));
    {
        s->open_cells = c->opt.open_cells != 0;                           // development switch: 0 = fields without open cells
        HIPCHK(build_fields(c, s, s->df, s->open_cells));
    }
    d.vox = s->vox.get(); d.occ1 = s->occ1.get(); d.occ2 = s->occ2.get(); d.occ3 = s->occ3.get(); d.df = s->df; d.df_stride = ndf; s->d.palette = s->palette.get();
    {
        d.df_prefetch = (d.df_fast && c->opt.df_prefetch) ? 1u : 0u;       // development switch: 0 = no neighbour-row prefetch in the secondary rays' look-ups
        d.df_own = (d.df_fast && c->opt.df_own) ? 1u : 0u;                 // development switch: 0 = the AO rays through the wave-minimum loop too
    }
    s->occ2_bytes = (uint32_t)(n2pad * 8); s->occ3_bytes = (uint32_t)(n3pad * 8);
    const int rc = default_textures(c, s);
    if (rc != VRT_OK) return rc;
    *out = hold.release();
    return VRT_OK;
}

int vrt_scene_from_bricks(vrt_ctx* c, const uint32_t* grid, uint32_t nbx, uint32_t nby, uint32_t nbz,
                          const uint8_t* pool, uint32_t n_bricks, const vrt_material palette[256], vrt_scene** out)
{
    if (!c || !grid || !palette || !out || (n_bricks && !pool)) return fail(VRT_ERR_INVALID, "vrt_scene_from_bricks: NULL argument");
    if (!nbx || !nby || !nbz || nbx > 512 || nby > 512 || nbz > 512)
        return fail(VRT_ERR_UNSUPPORTED, "vrt_scene_from_bricks: each dimension must be 1..512 bricks (8..4096 voxels)");
    if (n_bricks >= 0xFFFFFEu) return fail(VRT_ERR_UNSUPPORTED, "vrt_scene_from_bricks: at most 2^24 - 2 occupied bricks (the march's 24-bit brick pointer)");
    const size_t nb = (size_t)nbx * nby * nbz;
    // the brick a pool entry belongs to, as an index into the padded grid; every entry must be referenced exactly once
    std::vector<uint32_t> coord(n_bricks, 0xFFFFFFFFu);
    const size_t pbx = (size_t)nbx + 2, pby = (size_t)nby + 2, pbz = (size_t)nbz + 2, npad = pbx * pby * pbz;
    for (size_t i = 0; i < nb; i++) {
        const uint32_t g = grid[i];
        if (g == 0u) continue;
        if (g > n_bricks) return fail(VRT_ERR_INVALID, "vrt_scene_from_bricks: a grid entry points past the pool");
        if (coord[g - 1u] != 0xFFFFFFFFu) return fail(VRT_ERR_INVALID, "vrt_scene_from_bricks: two grid entries share a pool brick");
        const size_t x = i % nbx, y = (i / nbx) % nby, z = i / ((size_t)nbx * nby);
        coord[g - 1u] = (uint32_t)((x + 1) + ((y + 1) + (z + 1) * pby) * pbx);
    }
    for (uint32_t i = 0; i < n_bricks; i++)
        if (coord[i] == 0xFFFFFFFFu) return fail(VRT_ERR_INVALID, "vrt_scene_from_bricks: a pool brick is not referenced by the grid");
    HIPCHK(hipSetDevice(c->device));
    NewScene hold(new vrt_scene(), SceneFree{c});
    vrt_scene* s = hold.get();
    s->shade_gen = ++g_shade_gen;
    s->bricks = true;
    VolumeView& d = s->d.vol;
    d.W = (int)(nbx * 8u); d.H = (int)(nby * 8u); d.D = (int)(nbz * 8u);
    d.pbx = (int)pbx; d.pby = (int)pby;
    const size_t cstride = df_field_bytes((int)nbx, (int)nby, (int)nbz);          // one padded coarse field (= npad rounded up to 256 B)
    const size_t pool_bytes = (size_t)n_bricks * 512u, fine_bytes = pool_bytes * 8u;
    s->metallic_voxels = any_metallic(pool, pool_bytes, palette);
    for (int i = 1; i < 256; i++) s->metal[i] = palette[i].metallic > 0.0f;
    {
        DevBuf<uint32_t> grid_dev, coord_dev;                      // the build's temporaries: gone when the build is done
        DevBuf<uint8_t> occ_dev, tmp0_dev, tmp1_dev;
        HIPCHK(s->bgrid.alloc(npad * 4));
        HIPCHK(s->bcoarse.alloc(8 * cstride));
        HIPCHK(s->bpool.alloc(pool_bytes ? pool_bytes : 1));
        HIPCHK(s->bfine.alloc(fine_bytes ? fine_bytes : 1));
        HIPCHK(s->palette.alloc(256 * sizeof(vrt_material)));
        HIPCHK(grid_dev.alloc(nb * 4));
        HIPCHK(coord_dev.alloc((size_t)(n_bricks ? n_bricks : 1) * 4));
        HIPCHK(occ_dev.alloc(nb));
        HIPCHK(tmp0_dev.alloc(nb));
        HIPCHK(tmp1_dev.alloc(nb));
        uint8_t *occ = occ_dev.get(), *tmp0 = tmp0_dev.get(), *tmp1 = tmp1_dev.get();
        s->bytes = npad * 4ull + 8ull * cstride + pool_bytes + fine_bytes + 256 * sizeof(vrt_material);
        HIPCHK(hipMemsetAsync(s->bgrid.get(), 0xFF, npad * 4, c->stream));            // border: 0xFFFFFFFF = outside the volume
        HIPCHK(hipMemsetAsync(s->bcoarse.get(), 0, 8 * cstride, c->stream));
        HIPCHK(hipMemcpyAsync(grid_dev.get(), grid, nb * 4, hipMemcpyHostToDevice, c->stream));
        if (n_bricks) {
            HIPCHK(hipMemcpyAsync(coord_dev.get(), coord.data(), (size_t)n_bricks * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(s->bpool.get(), pool, pool_bytes, hipMemcpyHostToDevice, c->stream));
        }
        HIPCHK(hipMemcpyAsync(s->palette.get(), palette, 256 * sizeof(vrt_material), hipMemcpyHostToDevice, c->stream));
        HIPCHK(launch_brick_grid(grid_dev.get(), (int)nbx, (int)nby, (int)nbz, s->bgrid.get(), occ, c->stream));
        // brick-level clearance: the dense scene's transform over the occupancy of the bricks, capped at VRT_BRICK_EDIT_CAP bricks
        HIPCHK(launch_build_df(occ, (int)nbx, (int)nby, (int)nbz, s->bcoarse.get(), cstride, tmp0, tmp1, c->stream, VRT_BRICK_EDIT_CAP));
        // open bricks (bit 7): no occupied brick left between here and the volume's corner in the octant's direction
        {
            s->open_cells = c->opt.open_cells != 0;                           // development switch: 0 = no open bricks
            if (s->open_cells) HIPCHK(launch_open_cells(occ, (int)nbx, (int)nby, (int)nbz, s->bcoarse.get(), cstride, tmp0, tmp1, c->stream, 0x80));
            d.brick_open = s->open_cells ? 1u : 0u;
            d.df_own = c->opt.df_own ? 1u : 0u;                                // development switch: 0 = the AO rays through the wave-minimum loop too
        }
        // the occupied bricks as a list of 8^3 cells, for the tile tags of a launch
        if (n_bricks <= kMaxCells) {
            std::vector<uint32_t> cells(n_bricks);
            for (uint32_t i = 0; i < n_bricks; i++) cells[i] = brick_cell_code(coord[i], d.pbx, d.pby);
            if (n_bricks) {
                HIPCHK(s->cells.alloc((size_t)n_bricks * 4));
                HIPCHK(hipMemcpy(s->cells.get(), cells.data(), (size_t)n_bricks * 4, hipMemcpyHostToDevice));
                s->bytes += (uint64_t)n_bricks * 4;
            }
            s->n_cells = n_bricks; s->cells_ok = true;
        }
        HIPCHK(launch_brick_fine(s->bgrid.get(), (int)pbx, (int)pby, coord_dev.get(), n_bricks, s->bpool.get(), s->bfine.get(), c->stream));
        // what the march reads: pointer, open bits and the eight coarse clearances of a brick in ONE 8-byte word; the pointer grid and
        // the coarse fields were only needed to build it (and the fine bytes)
        HIPCHK(s->bentry.alloc(npad * 8));
        HIPCHK(launch_brick_pack(s->bgrid.get(), s->bcoarse.get(), cstride, npad, s->bentry.get(), c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        s->bgrid.reset(); s->bcoarse.reset();
        s->bytes = npad * 8ull + pool_bytes + fine_bytes + 256 * sizeof(vrt_material) + (uint64_t)n_bricks * 4;
        s->bcap = n_bricks;
    }
    d.bgrid = nullptr; d.bcoarse = nullptr; d.bcoarse_stride = cstride; d.bpool = s->bpool.get(); d.bfine = s->bfine.get(); d.bentry = s->bentry.get();
    s->d.palette = s->palette.get();
    const int rc = default_textures(c, s);
    if (rc != VRT_OK) return rc;
    *out = hold.release();
    return VRT_OK;
}

int vrt_scene_trim(vrt_ctx* c, vrt_scene* s)
{
    if (!c || !s) return fail(VRT_ERR_INVALID, "vrt_scene_trim: NULL argument");
    HIPCHK(hipSetDevice(c->device));
    // a scene may be shared by several contexts (frames in flight: one stream each); a count-plane launch enqueued on ANY of them
    // may still be reading the fields freed below, so this waits for the whole device, not for the calling context's stream
    HIPCHK(hipDeviceSynchronize());
    std::lock_guard<std::mutex> lock(s->lazy);
    drop_count_fields(s);
    s->drop_scratch();                                           // (an edit, a flood, a voxelization takes its own again)
    // the calling context's miss-colour planes (vrt_miss_plane.h): the next launch that wants one builds it again
    c->sky_planes.clear();
    for (int q = 0; q < VRT_SKY_PLANES; q++) { c->sky_plane_buf[q].reset(); c->sky_plane_px[q] = 0; }
    return VRT_OK;
}

int vrt_debug_scene_state(vrt_ctx* c, const vrt_scene* s, int what, void* host, size_t capacity, size_t* bytes)
{
    if (!c || !s || !bytes) return fail(VRT_ERR_INVALID, "vrt_debug_scene_state: NULL argument");
    const VolumeView& d = s->d.vol;
    const bool brick_state = what == VRT_STATE_BENTRY || what == VRT_STATE_BPOOL || what == VRT_STATE_BFINE;
    if (s->bricks ? !(brick_state || what == VRT_STATE_CELLS) : brick_state)
        return fail(VRT_ERR_UNSUPPORTED, s->bricks ? "vrt_debug_scene_state: a brick scene has the structures VRT_STATE_CELLS, _BENTRY, _BPOOL and _BFINE only"
                                                   : "vrt_debug_scene_state: VRT_STATE_BENTRY, _BPOOL and _BFINE are a brick scene's");
    const void* src = nullptr;
    size_t n = 0;
    switch (what) {
    case VRT_STATE_BENTRY: src = s->bentry.get(); n = ((size_t)d.W / 8 + 2u) * ((size_t)d.H / 8 + 2u) * ((size_t)d.D / 8 + 2u) * 8u; break;
    case VRT_STATE_BPOOL:  src = s->bpool.get();  n = (size_t)s->bcap * 512u; break;
    case VRT_STATE_BFINE:  src = s->bfine.get();  n = (size_t)s->bcap * 4096u; break;
    case VRT_STATE_VOX:   src = s->vox.get();  n = (size_t)d.W * d.H * d.D; break;
    case VRT_STATE_DF:    src = s->df;   n = s->df_bytes; break;
    case VRT_STATE_OCC1:  src = s->occ1.get(); n = (size_t)d.n1x * d.n1y * d.n1z * 8; break;
    case VRT_STATE_OCC2:  src = s->occ2.get(); n = s->occ2_bytes; break;      // with the zero word that pads it to 16-byte multiples
    case VRT_STATE_OCC3:  src = s->occ3.get(); n = s->occ3_bytes; break;
    case VRT_STATE_CELLS: src = s->cells.get(); n = (size_t)s->n_cells * 4; break;
    default: return fail(VRT_ERR_INVALID, "vrt_debug_scene_state: unknown structure");
    }
    *bytes = n;
    if (!host) return VRT_OK;
    if (capacity < n) return fail(VRT_ERR_INVALID, "vrt_debug_scene_state: the host buffer is too small");
    HIPCHK(hipSetDevice(c->device));
    if (n) HIPCHK(hipMemcpyAsync(host, src, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return VRT_OK;
}

int vrt_scene_memory(const vrt_scene* s, uint64_t* bytes)
{
    if (!s || !bytes) return fail(VRT_ERR_INVALID, "vrt_scene_memory: NULL argument");
    *bytes = s->bytes + (uint64_t)s->d.sky_w * s->d.sky_h * 20u + (uint64_t)s->d.noise_w * s->d.noise_h * 4u + 64u * 16u;
    return VRT_OK;
}

int vrt_scene_load_vox_mem(vrt_ctx* c, const void* buf, size_t n, vrt_scene** out)
{
    if (!c || !buf || !out) return fail(VRT_ERR_INVALID, "vrt_scene_load_vox_mem: NULL argument");
    FlatScene fs; std::string err;
    int rc = vox_flatten((const uint8_t*)buf, n, fs, err);
    if (rc != VRT_OK) return fail(rc, err);
    return vrt_scene_from_dense(c, fs.voxels.data(), fs.dims[0], fs.dims[1], fs.dims[2], fs.palette, out);
}

int vrt_scene_load_vox_file(vrt_ctx* c, const char* path, vrt_scene** out)
{
    if (!c || !path || !out) return fail(VRT_ERR_INVALID, "vrt_scene_load_vox_file: NULL argument");
    FILE* f = fopen(path, "rb");
    if (!f) return fail(VRT_ERR_IO, "Failed to read voxel scene");
    std::vector<uint8_t> buf;
    if (fseek(f, 0, SEEK_END) == 0) {
        long sz = ftell(f);
        if (sz > 0) { buf.resize((size_t)sz); rewind(f); if (fread(buf.data(), 1, buf.size(), f) != buf.size()) buf.clear(); }
    }
    fclose(f);
    if (buf.empty()) return fail(VRT_ERR_IO, "Failed to read voxel scene");
    return vrt_scene_load_vox_mem(c, buf.data(), buf.size(), out);
}

int vrt_scene_set_sky_file(vrt_ctx* c, vrt_scene* s, const char* path)
{
    if (!c || !s || !path) return fail(VRT_ERR_INVALID, "vrt_scene_set_sky_file: NULL argument");
    LoadedImage img; std::string err;
    int rc = image_load(path, img, err);
    if (rc != VRT_OK) return fail(rc, err);
    if (!img.is_hdr) {                                        // 8-bit image as sky: c/255 per channel
        img.f32.resize(img.u8.size());
        for (size_t i = 0; i < img.u8.size(); i++) img.f32[i] = (float)img.u8[i] / 255.0f;
    }
    return vrt_scene_set_sky(c, s, img.f32.data(), img.w, img.h);
}

int vrt_scene_set_blue_noise_file(vrt_ctx* c, vrt_scene* s, const char* path)
{
    if (!c || !s || !path) return fail(VRT_ERR_INVALID, "vrt_scene_set_blue_noise_file: NULL argument");
    LoadedImage img; std::string err;
    int rc = image_load(path, img, err);
    if (rc != VRT_OK) return fail(rc, err);
    if (img.is_hdr) return fail(VRT_ERR_UNSUPPORTED, "vrt_scene_set_blue_noise_file: the noise texture is RGBA8_UNORM, got a float image");
    return vrt_scene_set_blue_noise(c, s, img.u8.data(), img.w, img.h);
}

int vrt_scene_info(const vrt_scene* s, uint32_t dims[3])
{
    if (!s || !dims) return fail(VRT_ERR_INVALID, "vrt_scene_info: NULL argument");
    dims[0] = (uint32_t)s->d.vol.W; dims[1] = (uint32_t)s->d.vol.H; dims[2] = (uint32_t)s->d.vol.D;
    return VRT_OK;
}

int vrt_scene_download(vrt_ctx* c, const vrt_scene* s, uint8_t* voxels, vrt_material palette[256])
{
    if (!c || !s) return fail(VRT_ERR_INVALID, "vrt_scene_download: NULL argument");
    if (s->bricks && voxels) return fail(VRT_ERR_UNSUPPORTED, "vrt_scene_download: a brick scene has no dense volume to copy back");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (voxels) HIPCHK(hipMemcpy(voxels, s->vox.get(), (size_t)s->d.vol.W * s->d.vol.H * s->d.vol.D, hipMemcpyDeviceToHost));
    if (palette) HIPCHK(hipMemcpy(palette, s->palette.get(), 256 * sizeof(vrt_material), hipMemcpyDeviceToHost));
    return VRT_OK;
}

} // extern "C"

// ---- scene read-back (vrt_scene_read_box, vrt_scene_list_box, vrt_scene_save_vox_*; csrc/vrt_scene_read.h) -------------------

namespace vrt {

// the box's checks, before any device work; *count: its voxels (vrt_host.h: vrt_api_faces.hip makes them too)
int read_box_checked(const vrt_scene* s, const int32_t lo[3], const uint32_t size[3], uint32_t max_side, const std::string& name, size_t* count)
{
    const int32_t dim[3] = {s->d.vol.W, s->d.vol.H, s->d.vol.D};
    switch (read_box_check(dim, lo, size, max_side, count)) {
    case READ_BOX_OK:       return VRT_OK;
    case READ_BOX_EMPTY:    return fail(VRT_ERR_INVALID, name + ": the box is empty");
    case READ_BOX_OVERFLOW: return fail(VRT_ERR_INVALID, name + ": the box's voxel count overflows size_t");
    case READ_BOX_SIDE:     return fail(VRT_ERR_INVALID, name + ": a listed box has no side above " + std::to_string(max_side) + " (a record holds a coordinate in one byte)");
    default:                return fail(VRT_ERR_INVALID, name + ": the box leaves the volume");
    }
}

ReadBox read_box_of(const vrt_scene* s, const int32_t lo[3], const uint32_t size[3])
{
    const VolumeView& d = s->d.vol;
    ReadBox b{};
    b.vox = s->bricks ? nullptr : s->vox.get();
    b.bentry = s->bentry.get(); b.bpool = s->bpool.get(); b.bcap = s->bcap;
    b.W = d.W; b.H = d.H; b.pbx = d.pbx; b.pby = d.pby;
    for (int a = 0; a < 3; a++) { b.lo[a] = lo[a]; b.size[a] = size[a]; }
    return b;
}

} // namespace vrt

namespace {

// How many non-empty voxels the (checked) box has -> *total, and in `work` every segment's first record.  A box over empty
// bricks only ends behind the bricks' entries.  Returns when the stream is done.
int list_count(vrt_ctx* c, const ReadBox& b, DevBuf<uint32_t>& work, uint32_t* total)
{
    const uint32_t nseg = list_segments(b);
    if (work.bytes() < ((size_t)nseg + 2u) * 4u) HIPCHK(work.alloc(((size_t)nseg + 2u) * 4u));
    *total = 0;
    if (!b.vox) {
        uint32_t occupied = 0;
        HIPCHK(launch_list_bricks(b, work.get() + nseg + 1u, c->stream));
        HIPCHK(hipMemcpyAsync(&occupied, work.get() + nseg + 1u, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (!occupied) return VRT_OK;
    }
    HIPCHK(launch_list_count(b, work.get(), c->stream));
    HIPCHK(hipMemcpyAsync(total, work.get() + nseg, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return VRT_OK;
}

// ... and its `total` (> 0) records to the host
int list_fetch(vrt_ctx* c, const ReadBox& b, const DevBuf<uint32_t>& work, uint32_t total, DevBuf<uint32_t>& dev, uint32_t* records)
{
    if (dev.bytes() < (size_t)total * 4u) HIPCHK(dev.alloc((size_t)total * 4u));
    HIPCHK(launch_list_scatter(b, work.get(), total, dev.get(), c->stream));
    HIPCHK(hipMemcpyAsync(records, dev.get(), (size_t)total * 4u, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return VRT_OK;
}

// the scene as a .vox file: per tile one listing, then vox_writer.cpp's serialiser -- the dense volume is never held
int scene_save_vox(vrt_ctx* c, const vrt_scene* s, std::vector<uint8_t>& file)
{
    HIPCHK(hipSetDevice(c->device));
    const uint32_t dims[3] = {(uint32_t)s->d.vol.W, (uint32_t)s->d.vol.H, (uint32_t)s->d.vol.D};
    std::vector<vrt_material> palette(256);
    HIPCHK(hipMemcpyAsync(palette.data(), s->palette.get(), 256 * sizeof(vrt_material), hipMemcpyDeviceToHost, c->stream));
    VoxWriter w;
    w.begin(dims);
    DevBuf<uint32_t> work, dev;
    std::vector<uint32_t> rec;
    for (uint32_t t = 0; t < w.tiles() && !w.too_big(); t++) {
        int32_t lo[3]; uint32_t size[3], total = 0;
        w.tile_box(t, lo, size);
        const ReadBox b = read_box_of(s, lo, size);
        int rc = list_count(c, b, work, &total);
        if (rc != VRT_OK) return rc;
        rec.resize(total);
        if (total && (rc = list_fetch(c, b, work, total, dev, rec.data())) != VRT_OK) return rc;
        w.tile(rec.data(), total);
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    std::string err;
    const int rc = w.finish(palette.data(), err);
    if (rc != VRT_OK) return fail(rc, "vrt_scene_save_vox: " + err);
    file.swap(w.out);
    return VRT_OK;
}

// a file's image handed to the caller as a malloc'ed buffer
int hand_over(const std::vector<uint8_t>& file, void** buf, size_t* n)
{
    void* p = malloc(file.size());
    if (!p) return fail(VRT_ERR_INVALID, "out of host memory");
    memcpy(p, file.data(), file.size());
    *buf = p; *n = file.size();
    return VRT_OK;
}

} // namespace

extern "C" {

int vrt_scene_read_box(struct vrt_ctx* c, const vrt_scene* s, const int32_t lo[3], const uint32_t size[3], uint8_t* ids)
{
    if (!c || !s || !lo || !size || !ids) return fail(VRT_ERR_INVALID, "vrt_scene_read_box: NULL argument");
    size_t n = 0;
    const int rc = read_box_checked(s, lo, size, 0, "vrt_scene_read_box", &n);
    if (rc != VRT_OK) return rc;
    HIPCHK(hipSetDevice(c->device));
    DevBuf<uint8_t> stage;
    if (stage.alloc(n) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VRT_ERR_UNSUPPORTED, "vrt_scene_read_box: no device memory for a staging buffer of " + std::to_string(n) + " bytes; read the box in parts");
    }
    HIPCHK(launch_read_box(read_box_of(s, lo, size), stage.get(), c->stream));
    HIPCHK(hipMemcpyAsync(ids, stage.get(), n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return VRT_OK;
}

int vrt_scene_list_box(struct vrt_ctx* c, const vrt_scene* s, const int32_t lo[3], const uint32_t size[3], uint32_t* records, uint64_t capacity,
                       uint64_t* count)
{
    if (!c || !s || !lo || !size || !count) return fail(VRT_ERR_INVALID, "vrt_scene_list_box: NULL argument");
    size_t n = 0;
    int rc = read_box_checked(s, lo, size, VRT_LIST_MAX_SIDE, "vrt_scene_list_box", &n);
    if (rc != VRT_OK) return rc;
    HIPCHK(hipSetDevice(c->device));
    const ReadBox b = read_box_of(s, lo, size);
    DevBuf<uint32_t> work, dev;
    uint32_t total = 0;
    if ((rc = list_count(c, b, work, &total)) != VRT_OK) return rc;
    *count = total;
    if (!records || !total) return VRT_OK;
    if (capacity < (uint64_t)total)
        return fail(VRT_ERR_INVALID, "vrt_scene_list_box: the box has " + std::to_string(total) + " non-empty voxels and `records` room for " + std::to_string(capacity));
    return list_fetch(c, b, work, total, dev, records);
}

int vrt_vox_encode_host(const uint8_t* voxels, const uint32_t dims[3], const vrt_material palette[256], void** buf, size_t* n)
{
    if (!voxels || !dims || !palette || !buf || !n) return fail(VRT_ERR_INVALID, "vrt_vox_encode_host: NULL argument");
    for (int a = 0; a < 3; a++)
        if (!dims[a] || dims[a] > 4096) return fail(VRT_ERR_INVALID, "vrt_vox_encode_host: each dimension must be in 1..4096");
    std::vector<uint8_t> file; std::string err;
    const int rc = vox_encode(voxels, dims, palette, file, err);
    if (rc != VRT_OK) return fail(rc, "vrt_vox_encode_host: " + err);
    return hand_over(file, buf, n);
}

int vrt_scene_save_vox_mem(struct vrt_ctx* c, const vrt_scene* s, void** buf, size_t* n)
{
    if (!c || !s || !buf || !n) return fail(VRT_ERR_INVALID, "vrt_scene_save_vox_mem: NULL argument");
    std::vector<uint8_t> file;
    const int rc = scene_save_vox(c, s, file);
    return rc == VRT_OK ? hand_over(file, buf, n) : rc;
}

int vrt_scene_save_vox_file(struct vrt_ctx* c, const vrt_scene* s, const char* path)
{
    if (!c || !s || !path) return fail(VRT_ERR_INVALID, "vrt_scene_save_vox_file: NULL argument");
    std::vector<uint8_t> file;
    const int rc = scene_save_vox(c, s, file);
    if (rc != VRT_OK) return rc;
    FILE* f = fopen(path, "wb");
    if (!f) return fail(VRT_ERR_IO, std::string("Could not write voxel scene ") + path);
    const bool ok = fwrite(file.data(), 1, file.size(), f) == file.size();
    if (fclose(f) != 0 || !ok) return fail(VRT_ERR_IO, std::string("Could not write voxel scene ") + path);
    return VRT_OK;
}

} // extern "C"
