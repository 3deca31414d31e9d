// vrt_api_scene.hip -- the scenes of the C-ABI: construction (dense and bricks), sky and noise, memory, download, edits of dense
// scenes and of reserved brick scenes, read-back (a box, a box's non-empty voxels, the scene as a .vox file), brushes and stamps
// (an edit whose ids a kernel composes).  Host code only; the kernels are vrt_scene_build.hip, vrt_scene_edit.hip,
// vrt_scene_read.hip, vrt_brush.hip, vrt_flood.hip (flood fills: vrt_scene_flood, whose loop over rounds lives here) and
// vrt_voxelize.hip (mesh voxelization: vrt_scene_voxelize, whose cut of the triangles into work items lives here).
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
#include "vrt_brush_launch.h"          // (brings vrt_scene_read.h and its launchers)
#include "vrt_flood_launch.h"
#include "vrt_voxelize_launch.h"

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

// Did the edit bring a metallic voxel?  (ids == NULL: the box was filled with `id`.)  From then on the scene's rays may bounce.
static void note_metallic(vrt_scene* s, const uint8_t* ids, size_t nbox, uint8_t id)
{
    if (s->metallic_voxels) return;
    if (ids) { for (size_t i = 0; i < nbox && !s->metallic_voxels; i++) s->metallic_voxels = ids[i] != 0 && s->metal[ids[i]]; }
    else s->metallic_voxels = id != 0 && s->metal[id];
}

// Where the ids of an edited box come from: the host (uploaded), one id for the whole box, or -- a brush, a stamp, a flood -- a
// kernel that composes them in the scratch memory, where the upload would have put them
struct EditIds {
    const uint8_t*  host = nullptr;       // the box's ids in box-index order, or
    uint8_t         id = 0;               // (host, compose and flood all NULL) one id for the whole box, or
    const BrushJob* compose = nullptr;    // launch_brush_compose's job, whose box is the edit's, or
    const FloodJob* flood = nullptr;      // launch_flood_compose's, likewise, or
    const VoxJob*   voxelize = nullptr;   // launch_vox_compose's, likewise, and
    const uint32_t* written = nullptr;    // the set of ids the kernel writes (BrushRecord::ids)
    bool boxed() const { return host != nullptr || compose != nullptr || flood != nullptr || voxelize != nullptr; }
};

static void note_metallic(vrt_scene* s, const EditIds& src, size_t nbox)
{
    if (!src.compose && !src.flood && !src.voxelize) { note_metallic(s, src.host, nbox, src.id); return; }
    for (int i = 1; i < 256 && !s->metallic_voxels; i++) s->metallic_voxels = ((src.written[i >> 5] >> (i & 31)) & 1u) != 0u && s->metal[i];
}

// the box's ids into the scratch memory (src.boxed())
static hipError_t edit_ids_to_scratch(vrt_ctx* c, const EditIds& src, uint8_t* dev, size_t nbox)
{
    if (src.compose) return launch_brush_compose(*src.compose, dev, c->stream);
    if (src.flood) return launch_flood_compose(*src.flood, dev, c->stream);
    if (src.voxelize) return launch_vox_compose(*src.voxelize, dev, c->stream);
    return hipMemcpyAsync(dev, src.host, nbox, hipMemcpyHostToDevice, c->stream);
}

// The edits' scratch memory, grown to `need` bytes (contents are not kept)
static hipError_t edit_scratch_room(vrt_scene* s, size_t need)
{
    if (need <= s->edit_scratch_bytes) return hipSuccess;
    if (s->edit_scratch) { s->edit_scratch.reset(); s->bytes -= s->edit_scratch_bytes; }
    s->edit_scratch_bytes = 0;
    const hipError_t e = s->edit_scratch.alloc(need);
    if (e != hipSuccess) return e;
    s->edit_scratch_bytes = need; s->bytes += need;
    return hipSuccess;
}

// The count planes' fields go; the next launch that asks for them builds them again
static void drop_count_fields(vrt_scene* s)
{
    if (!s->df_counts) return;
    s->df_counts_raw.reset(); s->df_counts = nullptr;
    s->bytes -= s->df_bytes;
}

// The clearance fields of a dense scene into dst (df_bytes: eight fields, or nine and the 0xFF byte in trace_df_fast's layout),
// from the voxels already on the device; open: with the open cells coded 0 (launch_open_cells).  Returns when they are built.
static hipError_t build_fields(vrt_ctx* c, const vrt_scene* s, uint8_t* dst, bool open)
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
static hipError_t build_cell_list(vrt_ctx* c, vrt_scene* s)
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
    if (cells.size() > (4u << 20)) return hipSuccess;
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

// ---- editable brick scenes (vrt_scene_reserve_bricks; csrc/vrt_brick_edit.h) ------------------------------------------------

namespace {

const uint32_t kNoBrick = 0xFFFFFFFFu;
const size_t kMaxCells = (size_t)4u << 20;      // above it a scene goes without a cell list (as vrt_scene_from_bricks)

inline size_t round256(size_t n) { return (n + 255u) & ~(size_t)255u; }

struct BrickDims { int nb[3]; size_t n, npad, cstride; };
BrickDims brick_dims(const vrt_scene* s)
{
    const VolumeView& d = s->d.vol;
    BrickDims b;
    b.nb[0] = d.W / 8; b.nb[1] = d.H / 8; b.nb[2] = d.D / 8;
    b.n = (size_t)b.nb[0] * b.nb[1] * b.nb[2];
    b.npad = ((size_t)b.nb[0] + 2u) * ((size_t)b.nb[1] + 2u) * ((size_t)b.nb[2] + 2u);
    b.cstride = (size_t)d.bcoarse_stride;
    return b;
}

// device bytes of a reserved brick scene
uint64_t brick_scene_bytes(const vrt_scene* s)
{
    const BrickDims b = brick_dims(s);
    return b.npad * 8ull + (uint64_t)s->bcap * 512ull * 9ull + 256 * sizeof(vrt_material) + (uint64_t)s->cells_room * 4ull +
           b.npad * 4ull + b.n + 8ull * b.cstride + s->edit_scratch_bytes + s->flood_scratch_bytes + s->voxelize_scratch_bytes;
}

uint32_t brick_cell_code(uint32_t pc, int pbx, int pby)
{
    return (uint32_t)(pc % (uint32_t)pbx - 1u) | ((uint32_t)((pc / (uint32_t)pbx) % (uint32_t)pby - 1u) << 10) | ((uint32_t)(pc / ((uint32_t)pbx * (uint32_t)pby) - 1u) << 20);
}

void brick_cell_add(vrt_scene* s, uint32_t slot, uint32_t pc)
{
    s->cell_pos[slot] = (uint32_t)s->hcells.size();
    s->hcells.push_back(brick_cell_code(pc, s->d.vol.pbx, s->d.vol.pby));
    s->cell_slot.push_back(slot);
}

void brick_cell_remove(vrt_scene* s, uint32_t slot)
{
    const uint32_t pos = s->cell_pos[slot], last = (uint32_t)s->hcells.size() - 1u;
    s->hcells[pos] = s->hcells[last]; s->cell_slot[pos] = s->cell_slot[last];
    s->cell_pos[s->cell_slot[pos]] = pos;
    s->hcells.pop_back(); s->cell_slot.pop_back();
    s->cell_pos[slot] = kNoBrick;
}

// the host's cell list to the device; a scene with more than kMaxCells occupied bricks goes without until it has fewer again
hipError_t brick_upload_cells(vrt_scene* s)
{
    const size_t n = s->hcells.size();
    s->n_cells = 0; s->cells_ok = false;
    if (n > kMaxCells || n > s->cells_room) return hipSuccess;
    if (n) { const hipError_t e = hipMemcpy(s->cells.get(), s->hcells.data(), n * 4, hipMemcpyHostToDevice); if (e != hipSuccess) return e; }
    s->n_cells = (uint32_t)n; s->cells_ok = true;
    return hipSuccess;
}

// the full build of the coarse fields, as vrt_scene_from_bricks does it, from the occupancy bytes; tmp0 / tmp1: one byte per brick
hipError_t brick_build_coarse(vrt_ctx* c, vrt_scene* s, uint8_t* tmp0, uint8_t* tmp1, bool pack)
{
    const BrickDims b = brick_dims(s);
    hipError_t e = launch_build_df(s->bocc.get(), b.nb[0], b.nb[1], b.nb[2], s->bcoarse.get(), b.cstride, tmp0, tmp1, c->stream, VRT_BRICK_EDIT_CAP);
    if (e == hipSuccess && s->open_cells) e = launch_open_cells(s->bocc.get(), b.nb[0], b.nb[1], b.nb[2], s->bcoarse.get(), b.cstride, tmp0, tmp1, c->stream, 0x80);
    if (e == hipSuccess && pack) e = launch_brick_pack(s->bgrid.get(), s->bcoarse.get(), b.cstride, b.npad, s->bentry.get(), c->stream);
    return e;
}

// vrt_scene_edit_box / vrt_scene_fill_box on a reserved brick scene; the caller checked the box, waited for the stream and holds the lock
int brick_scene_edit(vrt_ctx* c, vrt_scene* s, const EditBox& box, const EditIds& src, const std::string& name)
{
    const VolumeView& d = s->d.vol;
    const BrickDims bd = brick_dims(s);
    BrickEdit e;
    e.nbx = bd.nb[0]; e.nby = bd.nb[1]; e.nbz = bd.nb[2]; e.pbx = d.pbx; e.pby = d.pby;
    EditSpan f[3];
    size_t nT = 1, nF = 1, nbox = 1;
    for (int a = 0; a < 3; a++) {
        e.lo[a] = box.lo[a]; e.hi[a] = box.hi[a];
        const EditSpan t = brick_span_t(box.lo[a], box.hi[a]);
        e.t_lo[a] = t.lo; e.t_n[a] = t.hi - t.lo;
        f[a] = brick_span_f(t, bd.nb[a]);
        nT *= (size_t)e.t_n[a]; nF *= (size_t)(f[a].hi - f[a].lo); nbox *= (size_t)(box.hi[a] - box.lo[a]);
    }
    const bool rule = brick_edit_in_place(e.nbx, e.nby, e.nbz, box.lo, box.hi);
    // scratch: the ids | a word per brick of T from the classification | one to the write | the fine list | the coarse passes'
    const bool ids = src.boxed();
    const size_t ids_room = ids ? round256(nbox) : 0, t_room = round256(nT * 4);
    const size_t list_max = rule ? nF : ((size_t)s->n_occ + nT < (size_t)s->bcap ? (size_t)s->n_occ + nT : (size_t)s->bcap);
    const size_t list_room = round256(list_max * 8);
    const size_t coarse_room = rule ? bedit_coarse_scratch_bytes(e, bd.cstride, s->open_cells) : 2 * round256(bd.n);
    HIPCHK(edit_scratch_room(s, ids_room + 2 * t_room + list_room + coarse_room));
    uint8_t* ids_dev = s->edit_scratch.get();
    uint32_t* after_dev = (uint32_t*)(ids_dev + ids_room);
    uint32_t* ptr_dev = (uint32_t*)(ids_dev + ids_room + t_room);
    uint2* list_dev = (uint2*)(ids_dev + ids_room + 2 * t_room);
    uint8_t* coarse_scr = ids_dev + ids_room + 2 * t_room + list_room;
    if (ids) HIPCHK(edit_ids_to_scratch(c, src, ids_dev, nbox));
    e.ids = ids ? ids_dev : nullptr; e.id = src.id;
    // 1. classify, before anything is written: a refused edit leaves the scene as it was
    std::vector<uint32_t> after(nT), new_ptr(nT);
    HIPCHK(launch_bedit_classify(e, s->bgrid.get(), s->bpool.get(), after_dev, c->stream));
    HIPCHK(hipMemcpyAsync(after.data(), after_dev, nT * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    auto pc_of = [&](size_t t) {
        const int bx = e.t_lo[0] + (int)(t % (size_t)e.t_n[0]), by = e.t_lo[1] + (int)((t / (size_t)e.t_n[0]) % (size_t)e.t_n[1]);
        const int bz = e.t_lo[2] + (int)(t / ((size_t)e.t_n[0] * e.t_n[1]));
        return (uint32_t)((size_t)(bx + 1) + ((size_t)(by + 1) + (size_t)(bz + 1) * (size_t)e.pby) * (size_t)e.pbx);
    };
    size_t appear = 0, vanish = 0;
    for (size_t t = 0; t < nT; t++) {
        const uint32_t old = s->hgrid[pc_of(t)];
        if (!old && after[t]) appear++;
        if (old && !after[t]) vanish++;
    }
    if (appear > s->free_slots.size() + vanish)
        return fail(VRT_ERR_UNSUPPORTED, name + ": the edit makes " + std::to_string(appear) + " empty bricks occupied and the pool has " +
                    std::to_string(s->free_slots.size() + vanish) + " free slots; reserve more with vrt_scene_reserve_bricks");
    note_metallic(s, src, nbox);
    // slots: the bricks that vanish give theirs back first, so an edit may move as many bricks as it likes within the reservation
    for (size_t t = 0; t < nT; t++) {
        const uint32_t pc = pc_of(t), old = s->hgrid[pc];
        new_ptr[t] = old;
        if (!old || after[t]) continue;
        s->free_slots.push_back(old - 1u); s->slot_pc[old - 1u] = kNoBrick;
        brick_cell_remove(s, old - 1u);
        s->hgrid[pc] = 0u; new_ptr[t] = 0u;
    }
    for (size_t t = 0; t < nT && appear; t++) {
        const uint32_t pc = pc_of(t);
        if (s->hgrid[pc] || !after[t]) continue;
        const uint32_t slot = s->free_slots.back();
        s->free_slots.pop_back(); s->slot_pc[slot] = pc;
        brick_cell_add(s, slot, pc);
        s->hgrid[pc] = slot + 1u; new_ptr[t] = slot + 1u;
    }
    s->n_occ = (uint32_t)((size_t)s->n_occ + appear - vanish);
    // 2. write
    HIPCHK(hipMemcpy(ptr_dev, new_ptr.data(), nT * 4, hipMemcpyHostToDevice));
    HIPCHK(launch_bedit_write(e, s->bgrid.get(), s->bocc.get(), s->bpool.get(), ptr_dev, c->stream));
    // 3. fine bytes: the occupied bricks of F -- or every occupied brick, on the full build path
    const bool changed = appear != 0 || vanish != 0, full = changed && !rule;
    std::vector<uint2> list;
    if (full) {
        for (uint32_t slot = 0; slot < s->bcap; slot++)
            if (s->slot_pc[slot] != kNoBrick) list.push_back(make_uint2(slot, s->slot_pc[slot]));
    } else {
        for (int z = f[2].lo; z < f[2].hi; z++) for (int y = f[1].lo; y < f[1].hi; y++) for (int x = f[0].lo; x < f[0].hi; x++) {
            const uint32_t pc = (uint32_t)((size_t)(x + 1) + ((size_t)(y + 1) + (size_t)(z + 1) * (size_t)e.pby) * (size_t)e.pbx);
            if (s->hgrid[pc]) list.push_back(make_uint2(s->hgrid[pc] - 1u, pc));
        }
    }
    if (list.size() > list_max) return fail(VRT_ERR_HIP, name + ": internal error (fine list)");
    if (!list.empty()) HIPCHK(hipMemcpy(list_dev, list.data(), list.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(launch_brick_fine_list(s->bgrid.get(), e.pbx, e.pby, list_dev, (uint32_t)list.size(), s->bpool.get(), s->bfine.get(), c->stream));
    // 4. coarse fields, open bits, entries, 5. cell list: functions of the occupancy and the slots alone
    if (changed) {
        if (full) HIPCHK(brick_build_coarse(c, s, coarse_scr, coarse_scr + round256(bd.n), true));
        else {
            HIPCHK(launch_bedit_coarse(e, s->bocc.get(), s->bcoarse.get(), bd.cstride, coarse_scr, s->open_cells, c->stream));
            HIPCHK(launch_brick_pack(s->bgrid.get(), s->bcoarse.get(), bd.cstride, bd.npad, s->bentry.get(), c->stream));
        }
        HIPCHK(brick_upload_cells(s));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return VRT_OK;
}

} // namespace

extern "C" {

int vrt_scene_reserve_bricks(vrt_ctx* c, vrt_scene* s, uint32_t capacity)
{
    if (!c || !s) return fail(VRT_ERR_INVALID, "vrt_scene_reserve_bricks: NULL argument");
    if (!s->bricks) return fail(VRT_ERR_UNSUPPORTED, "vrt_scene_reserve_bricks: a dense scene has no brick pool (it is editable as it is)");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::lock_guard<std::mutex> lock(s->lazy);
    const uint32_t n_occ = s->reserved ? s->n_occ : s->bcap;
    if (capacity < n_occ) return fail(VRT_ERR_INVALID, "vrt_scene_reserve_bricks: the scene has " + std::to_string(n_occ) + " occupied bricks");
    if (capacity >= 0xFFFFFEu) return fail(VRT_ERR_INVALID, "vrt_scene_reserve_bricks: at most 2^24 - 3 bricks (the march's 24-bit brick pointer)");
    VolumeView& d = s->d.vol;
    const BrickDims bd = brick_dims(s);
    if (!s->reserved) {
        // the grid and the occupancy back out of the entries; the coarse fields built again (an entry holds them saturated at 15)
        DevBuf<uint8_t> tmp;
        hipError_t e = s->bgrid.alloc(bd.npad * 4);
        if (e == hipSuccess) e = s->bocc.alloc(bd.n);
        if (e == hipSuccess) e = s->bcoarse.alloc(8 * bd.cstride);
        if (e == hipSuccess) e = tmp.alloc(2 * round256(bd.n));
        if (e == hipSuccess) e = hipMemsetAsync(s->bcoarse.get(), 0, 8 * bd.cstride, c->stream);
        if (e == hipSuccess) e = launch_brick_unpack(s->bentry.get(), bd.nb[0], bd.nb[1], bd.nb[2], s->bgrid.get(), s->bocc.get(), c->stream);
        if (e == hipSuccess) e = brick_build_coarse(c, s, tmp.get(), tmp.get() + round256(bd.n), false);
        std::vector<uint32_t> hgrid(bd.npad);
        if (e == hipSuccess) e = hipMemcpyAsync(hgrid.data(), s->bgrid.get(), bd.npad * 4, hipMemcpyDeviceToHost, c->stream);
        const hipError_t sync = hipStreamSynchronize(c->stream);
        tmp.reset();
        if (e == hipSuccess) e = sync;
        if (e != hipSuccess) {
            s->bgrid.reset(); s->bocc.reset(); s->bcoarse.reset();
            return fail(VRT_ERR_HIP, std::string("vrt_scene_reserve_bricks: ") + hipGetErrorString(e));
        }
        s->hgrid.swap(hgrid);
        s->slot_pc.assign(s->bcap, kNoBrick);
        for (size_t i = 0; i < bd.npad; i++) {
            const uint32_t g = s->hgrid[i];
            if (g != 0u && g != 0xFFFFFFFFu) s->slot_pc[g - 1u] = (uint32_t)i;
        }
        s->cell_pos.assign(s->bcap, kNoBrick);
        s->hcells.clear(); s->cell_slot.clear(); s->free_slots.clear();
        for (uint32_t slot = 0; slot < s->bcap; slot++) brick_cell_add(s, slot, s->slot_pc[slot]);     // the build's own order
        s->n_occ = s->bcap;
        s->cells_room = s->cells ? s->bcap : 0;
        s->reserved = true;
        s->bytes = brick_scene_bytes(s);
    }
    if (capacity > s->bcap) {
        DevBuf<uint8_t> pool, fine;
        hipError_t e = pool.alloc((size_t)capacity * 512u);
        if (e == hipSuccess) e = fine.alloc((size_t)capacity * 4096u);
        if (e == hipSuccess && s->bcap) e = hipMemcpy(pool.get(), s->bpool.get(), (size_t)s->bcap * 512u, hipMemcpyDeviceToDevice);
        if (e == hipSuccess && s->bcap) e = hipMemcpy(fine.get(), s->bfine.get(), (size_t)s->bcap * 4096u, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) return fail(VRT_ERR_HIP, std::string("vrt_scene_reserve_bricks: ") + hipGetErrorString(e));
        s->bpool = std::move(pool); s->bfine = std::move(fine); d.bpool = s->bpool.get(); d.bfine = s->bfine.get();
        std::vector<uint32_t> fresh;
        for (uint32_t slot = capacity; slot-- > s->bcap;) fresh.push_back(slot);
        s->free_slots.insert(s->free_slots.begin(), fresh.begin(), fresh.end());    // under the slots already free
        s->slot_pc.resize(capacity, kNoBrick); s->cell_pos.resize(capacity, kNoBrick);
        s->bcap = capacity;
    }
    const size_t room = (size_t)s->bcap < kMaxCells ? (size_t)s->bcap : kMaxCells;
    if (room > s->cells_room) {
        DevBuf<uint32_t> cells;
        HIPCHK(cells.alloc(room * 4));
        s->cells = std::move(cells); s->cells_room = room;
        HIPCHK(brick_upload_cells(s));
    }
    s->bytes = brick_scene_bytes(s);
    return VRT_OK;
}

} // extern "C"

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
    if (s->edit_scratch) {                                       // (an edit takes it again)
        s->edit_scratch.reset();
        s->bytes -= s->edit_scratch_bytes;
        s->edit_scratch_bytes = 0;
    }
    if (s->flood_scratch) {                                      // (a flood takes it again)
        s->flood_scratch.reset();
        s->bytes -= s->flood_scratch_bytes;
        s->flood_scratch_bytes = 0;
    }
    if (s->voxelize_scratch) {                                   // (a voxelization takes it again)
        s->voxelize_scratch.reset();
        s->bytes -= s->voxelize_scratch_bytes;
        s->voxelize_scratch_bytes = 0;
    }
    return VRT_OK;
}

// An edit of the box b, which lies inside the volume, with the ids of src; the caller checked that the scene is editable,
// waited for the stream and holds the lock
static int scene_edit_locked(vrt_ctx* c, vrt_scene* s, const EditBox& b, const EditIds& src, const std::string& name)
{
    if (s->bricks) return brick_scene_edit(c, s, b, src, name);
    const VolumeView& d = s->d.vol;
    const size_t nbox = (size_t)(b.hi[0] - b.lo[0]) * (size_t)(b.hi[1] - b.lo[1]) * (size_t)(b.hi[2] - b.lo[2]);
    const bool ids = src.boxed();
    note_metallic(s, src, nbox);
    drop_count_fields(s);
    const bool in_place = edit_in_place(d.W, d.H, d.D, b.lo, b.hi, VRT_EDIT_CAP);
    size_t need = ids ? ((nbox + 255u) & ~(size_t)255u) : 0;
    const size_t ids_room = need;
    if (in_place) need += edit_scratch_bytes(b, s->open_cells);
    HIPCHK(edit_scratch_room(s, need));
    uint8_t* const scratch = s->edit_scratch.get();
    if (ids) HIPCHK(edit_ids_to_scratch(c, src, scratch, nbox));
    const size_t ndf = (size_t)d.df_stride;
    HIPCHK(launch_edit_write(s->vox.get(), d.df_fast ? s->df + 8 * ndf : nullptr, b, ids ? scratch : nullptr, src.id, c->stream));
    HIPCHK(launch_edit_pyramid(s->vox.get(), b, s->occ1.get(), s->occ2.get(), s->occ3.get(), c->stream));
    if (in_place) HIPCHK(launch_edit_fields(s->vox.get(), b, s->df, ndf, scratch + ids_room, s->open_cells, c->stream));
    else HIPCHK(build_fields(c, s, s->df, s->open_cells));
    HIPCHK(build_cell_list(c, s));
    HIPCHK(hipStreamSynchronize(c->stream));
    return VRT_OK;
}

// vrt_scene_edit_box / vrt_scene_fill_box: ids == NULL fills the box with `id`
static int scene_edit(vrt_ctx* c, vrt_scene* s, const int32_t lo[3], const uint32_t size[3], const uint8_t* ids, uint8_t id, const char* who)
{
    const std::string name(who);
    if (s->bricks && !s->reserved) return fail(VRT_ERR_UNSUPPORTED, name + ": a brick scene cannot be edited before vrt_scene_reserve_bricks");
    const VolumeView& d = s->d.vol;
    const int dim[3] = {d.W, d.H, d.D};
    EditBox b;
    b.W = d.W; b.H = d.H; b.D = d.D;
    for (int a = 0; a < 3; a++) {
        if (size[a] == 0) return fail(VRT_ERR_INVALID, name + ": the box is empty");
        if (lo[a] < 0 || lo[a] >= dim[a] || (uint64_t)size[a] > (uint64_t)(dim[a] - lo[a])) return fail(VRT_ERR_INVALID, name + ": the box leaves the volume");
        b.lo[a] = lo[a]; b.hi[a] = lo[a] + (int)size[a];
    }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::lock_guard<std::mutex> lock(s->lazy);
    EditIds src;
    src.host = ids; src.id = id;
    return scene_edit_locked(c, s, b, src, name);
}

int vrt_scene_edit_box(vrt_ctx* c, vrt_scene* s, const int32_t lo[3], const uint32_t size[3], const uint8_t* ids)
{
    if (!c || !s || !lo || !size || !ids) return fail(VRT_ERR_INVALID, "vrt_scene_edit_box: NULL argument");
    return scene_edit(c, s, lo, size, ids, 0, "vrt_scene_edit_box");
}

int vrt_scene_fill_box(vrt_ctx* c, vrt_scene* s, const int32_t lo[3], const uint32_t size[3], uint8_t id)
{
    if (!c || !s || !lo || !size) return fail(VRT_ERR_INVALID, "vrt_scene_fill_box: NULL argument");
    return scene_edit(c, s, lo, size, nullptr, id, "vrt_scene_fill_box");
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
    void* p = malloc(file.size());
    if (!p) return fail(VRT_ERR_INVALID, "out of host memory");
    memcpy(p, file.data(), file.size());
    *buf = p; *n = file.size();
    return VRT_OK;
}

int vrt_scene_save_vox_mem(struct vrt_ctx* c, const vrt_scene* s, void** buf, size_t* n)
{
    if (!c || !s || !buf || !n) return fail(VRT_ERR_INVALID, "vrt_scene_save_vox_mem: NULL argument");
    std::vector<uint8_t> file;
    const int rc = scene_save_vox(c, s, file);
    if (rc != VRT_OK) return rc;
    void* p = malloc(file.size());
    if (!p) return fail(VRT_ERR_INVALID, "out of host memory");
    memcpy(p, file.data(), file.size());
    *buf = p; *n = file.size();
    return VRT_OK;
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

// ---- brushes and stamps (vrt_scene_brush, vrt_scene_stamp; csrc/vrt_brush.h) ---------------------------------------------------

static_assert(VRT_BRUSH_BOX == VRT_BRUSH_SHAPE_BOX && VRT_BRUSH_ELLIPSOID == VRT_BRUSH_SHAPE_ELLIPSOID && VRT_BRUSH_CAPSULE == VRT_BRUSH_SHAPE_CAPSULE,
              "include/vrt.h and csrc/vrt_brush.h number the shapes differently");
static_assert(VRT_BRUSH_SET == VRT_BRUSH_MODE_SET && VRT_BRUSH_PAINT == VRT_BRUSH_MODE_PAINT && VRT_BRUSH_ADD == VRT_BRUSH_MODE_ADD &&
              VRT_BRUSH_REPLACE == VRT_BRUSH_MODE_REPLACE, "include/vrt.h and csrc/vrt_brush.h number the modes differently");

namespace {

// One brush or stamp over the clipped bounds [clo, clo + csize) of the scene j.box views: the extent kernel says what changes;
// if anything does, the tight box of the changes is edited with the ids the compose kernel writes.  The caller checked the
// arguments, waited for the stream and holds the scene's lock.  *out (may be NULL) holds zeros.
int brush_run(vrt_ctx* c, vrt_scene* s, BrushJob& j, const int32_t clo[3], const uint32_t csize[3], const std::string& name, vrt_brush_result* out)
{
    if (!c->brush_rec) HIPCHK(c->brush_rec.alloc(sizeof(BrushRecord)));
    BrushRecord* const rec_dev = (BrushRecord*)c->brush_rec.get();
    const BrushRecord init = brush_record_init();
    BrushRecord rec = init;
    for (int a = 0; a < 3; a++) { j.box.lo[a] = clo[a]; j.box.size[a] = csize[a]; }
    HIPCHK(hipMemcpyAsync(rec_dev, &init, sizeof init, hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_brush_extent(j, rec_dev, c->stream));
    HIPCHK(hipMemcpyAsync(&rec, rec_dev, sizeof rec, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (rec.changed == 0ull) return VRT_OK;                     // nothing is written, no edit pass runs, the count planes' fields stay
    const VolumeView& d = s->d.vol;
    EditBox b;
    b.W = d.W; b.H = d.H; b.D = d.D;
    for (int a = 0; a < 3; a++) {
        if (rec.mn[a] < clo[a] || rec.mx[a] < rec.mn[a] || (int64_t)rec.mx[a] >= (int64_t)clo[a] + (int64_t)csize[a])
            return fail(VRT_ERR_HIP, name + ": internal error (the changed voxels' bounds leave the brush's)");
        b.lo[a] = rec.mn[a]; b.hi[a] = rec.mx[a] + 1;
        j.box.lo[a] = b.lo[a]; j.box.size[a] = (uint32_t)(b.hi[a] - b.lo[a]);
    }
    EditIds src;
    src.compose = &j; src.written = rec.ids;
    const int rc = scene_edit_locked(c, s, b, src, name);
    if (rc == VRT_OK && out) {
        out->changed = rec.changed;
        for (int a = 0; a < 3; a++) { out->lo[a] = b.lo[a]; out->size[a] = j.box.size[a]; }
    }
    return rc;
}

} // namespace

extern "C" {

int vrt_scene_brush(struct vrt_ctx* c, vrt_scene* s, const vrt_brush* brush, vrt_brush_result* result)
{
    const std::string name("vrt_scene_brush");
    if (!c || !s || !brush) return fail(VRT_ERR_INVALID, name + ": NULL argument");
    if (brush->shape != VRT_BRUSH_BOX && brush->shape != VRT_BRUSH_ELLIPSOID && brush->shape != VRT_BRUSH_CAPSULE) return fail(VRT_ERR_INVALID, name + ": unknown shape");
    if (!brush_shape_ok(brush->shape, brush->p))
        return fail(VRT_ERR_INVALID, name + ": a shape parameter is outside its range (box sizes 1..2^30; semi-axes and radius 1..1024 half voxels; a capsule's end points -4096..12288)");
    if (brush->mode < VRT_BRUSH_SET || brush->mode > VRT_BRUSH_REPLACE) return fail(VRT_ERR_INVALID, name + ": unknown mode");
    if (!brush_mode_ok(brush->mode, brush->id, brush->match))
        return fail(VRT_ERR_INVALID, name + (brush->mode == VRT_BRUSH_REPLACE ? ": REPLACE needs id != match" : ": PAINT and ADD need id != 0 (carve with SET)"));
    if (result) memset(result, 0, sizeof *result);
    if (s->bricks && !s->reserved) return fail(VRT_ERR_UNSUPPORTED, name + ": a brick scene cannot be edited before vrt_scene_reserve_bricks");
    const int32_t dim[3] = {s->d.vol.W, s->d.vol.H, s->d.vol.D};
    int64_t lo[3], hi[3];
    int32_t clo[3];
    uint32_t csize[3];
    brush_bounds(brush->shape, brush->p, lo, hi);
    if (!brush_clip(lo, hi, dim, clo, csize)) return VRT_OK;       // wholly outside the volume: nothing to do
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::lock_guard<std::mutex> lock(s->lazy);
    BrushJob j{};
    j.box = read_box_of(s, clo, csize);
    j.form = brush->shape; j.mode = brush->mode;
    for (int i = 0; i < 9; i++) j.p[i] = brush->p[i];
    j.id = brush->id; j.match = brush->match;
    return brush_run(c, s, j, clo, csize, name, result);
}

int vrt_scene_stamp(struct vrt_ctx* c, vrt_scene* dst, const int32_t dst_lo[3], const vrt_scene* src, const int32_t src_lo[3],
                    const uint32_t size[3], uint32_t orient, uint32_t flags, vrt_brush_result* result)
{
    const std::string name("vrt_scene_stamp");
    if (!c || !dst || !dst_lo || !src || !src_lo || !size) return fail(VRT_ERR_INVALID, name + ": NULL argument");
    if (!stamp_orient_ok(orient)) return fail(VRT_ERR_INVALID, name + ": an orientation is perm | flips << 3 with perm in 0..5 and flips in 0..7");
    if (flags & ~(uint32_t)VRT_STAMP_SKIP_EMPTY) return fail(VRT_ERR_INVALID, name + ": unknown flag");
    size_t n = 0;
    const int rc = read_box_checked(src, src_lo, size, 0, name, &n);
    if (rc != VRT_OK) return rc;
    for (int a = 0; a < 3; a++)
        if (size[a] > VRT_STAMP_MAX_SIDE) return fail(VRT_ERR_INVALID, name + ": a stamp has no side above " + std::to_string(VRT_STAMP_MAX_SIDE) + "; stamp in parts");
    if (result) memset(result, 0, sizeof *result);
    if (dst->bricks && !dst->reserved) return fail(VRT_ERR_UNSUPPORTED, name + ": a brick scene cannot be edited before vrt_scene_reserve_bricks");
    const int32_t dim[3] = {dst->d.vol.W, dst->d.vol.H, dst->d.vol.D};
    uint32_t dsize[3], csize[3];
    int64_t lo[3], hi[3];
    int32_t clo[3];
    stamp_dst_size(orient, size, dsize);
    for (int a = 0; a < 3; a++) { lo[a] = (int64_t)dst_lo[a]; hi[a] = (int64_t)dst_lo[a] + (int64_t)dsize[a]; }
    if (!brush_clip(lo, hi, dim, clo, csize)) return VRT_OK;       // wholly outside the destination
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::lock_guard<std::mutex> lock(dst->lazy);
    // the source box into staging before anything is written: a stamp of a scene onto itself copies the old content
    DevBuf<uint8_t> stage;
    if (stage.alloc(n) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VRT_ERR_UNSUPPORTED, name + ": no device memory for a staging buffer of " + std::to_string(n) + " bytes; stamp in parts");
    }
    HIPCHK(launch_read_box(read_box_of(src, src_lo, size), stage.get(), c->stream));
    BrushJob j{};
    j.box = read_box_of(dst, clo, csize);
    j.form = VRT_BRUSH_FORM_STAMP;
    j.stage = stage.get();
    for (int a = 0; a < 3; a++) { j.dst_lo[a] = dst_lo[a]; j.src_size[a] = size[a]; }
    j.orient = orient; j.skip_empty = (flags & VRT_STAMP_SKIP_EMPTY) ? 1u : 0u;
    const int rcb = brush_run(c, dst, j, clo, csize, name, result);
    HIPCHK(hipStreamSynchronize(c->stream));                       // (the staging buffer goes when this returns)
    return rcb;
}

} // extern "C"

// ---- flood fills (vrt_scene_flood; csrc/vrt_flood.h) ---------------------------------------------------------------------------

static_assert(VRT_FLOOD_SAME == VRT_FLOOD_MATCH_SAME && VRT_FLOOD_SOLID == VRT_FLOOD_MATCH_SOLID && VRT_FLOOD_FACES == VRT_FLOOD_CONN_FACES &&
              VRT_FLOOD_CORNERS == VRT_FLOOD_CONN_CORNERS && VRT_FLOOD_MEASURE == VRT_FLOOD_FLAG_MEASURE,
              "include/vrt.h and csrc/vrt_flood.h number the predicates, connectivities or flags differently");

namespace {

const uint32_t kFloodBatchMax = 32;     // rounds enqueued between two reads of the counters

// The flood's scratch memory: passable mask | reached mask | two sets of activity flags | the rounds' counters | the record
struct FloodScratch { uint8_t *passable, *reached; uint32_t *act[2], *counters; FloodRecord* rec; size_t zero_bytes; };

bool flood_scratch_room(vrt_scene* s, size_t ntiles, FloodScratch* out)
{
    const size_t mask = ntiles * VRT_FLOOD_TILE_BYTES, flags = round256(ntiles * 4), counters = round256(kFloodBatchMax * 4), rec = round256(sizeof(FloodRecord));
    const size_t need = 2 * mask + 2 * flags + counters + rec;
    if (need > s->flood_scratch_bytes) {
        if (s->flood_scratch) { s->flood_scratch.reset(); s->bytes -= s->flood_scratch_bytes; }
        s->flood_scratch_bytes = 0;
        if (s->flood_scratch.alloc(need) != hipSuccess) { (void)hipGetLastError(); return false; }
        s->flood_scratch_bytes = need; s->bytes += need;
    }
    uint8_t* p = s->flood_scratch.get();
    out->passable = p; out->reached = p + mask;
    out->act[0] = (uint32_t*)(p + 2 * mask); out->act[1] = (uint32_t*)(p + 2 * mask + flags);
    out->counters = (uint32_t*)(p + 2 * mask + 2 * flags);
    out->rec = (FloodRecord*)(p + 2 * mask + 2 * flags + counters);
    out->zero_bytes = 2 * mask + 2 * flags;
    return true;
}

} // namespace

extern "C" {

int vrt_scene_flood(struct vrt_ctx* c, vrt_scene* s, const vrt_flood* flood, vrt_flood_result* result)
{
    const std::string name("vrt_scene_flood");
    if (!c || !s || !flood || !result) return fail(VRT_ERR_INVALID, name + ": NULL argument");
    if (flood->match != VRT_FLOOD_SAME && flood->match != VRT_FLOOD_SOLID) return fail(VRT_ERR_INVALID, name + ": unknown match (VRT_FLOOD_SAME or VRT_FLOOD_SOLID)");
    if (flood->connectivity != VRT_FLOOD_FACES && flood->connectivity != VRT_FLOOD_CORNERS)
        return fail(VRT_ERR_INVALID, name + ": connectivity is VRT_FLOOD_FACES (6) or VRT_FLOOD_CORNERS (26)");
    if (flood->flags & ~(uint32_t)VRT_FLOOD_MEASURE) return fail(VRT_ERR_INVALID, name + ": unknown flag");
    if (!flood_args_ok(flood->match, flood->connectivity, flood->flags, flood->size)) return fail(VRT_ERR_INVALID, name + ": each size of the bounds is in 1..2^30");
    const bool measure = (flood->flags & VRT_FLOOD_MEASURE) != 0u;
    const int32_t dim[3] = {s->d.vol.W, s->d.vol.H, s->d.vol.D};
    int64_t lo[3], hi[3];
    int32_t clo[3];
    uint32_t csize[3];
    for (int a = 0; a < 3; a++) { lo[a] = (int64_t)flood->lo[a]; hi[a] = (int64_t)flood->lo[a] + (int64_t)flood->size[a]; }
    const bool any = brush_clip(lo, hi, dim, clo, csize);
    if (any && !flood_sides_ok(csize))
        return fail(VRT_ERR_INVALID, name + ": the bounds inside the volume have no side above " + std::to_string(VRT_FLOOD_MAX_SIDE) + "; flood in parts");
    memset(result, 0, sizeof *result);
    if (!measure && s->bricks && !s->reserved) return fail(VRT_ERR_UNSUPPORTED, name + ": a brick scene cannot be edited before vrt_scene_reserve_bricks");
    if (!any || !flood_seed_inside(flood->seed, clo, csize)) return VRT_OK;      // bounds wholly outside the volume, or the seed outside them: nothing to do
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::lock_guard<std::mutex> lock(s->lazy);
    FloodJob j{};
    j.box = read_box_of(s, clo, csize);
    flood_tiles(csize, j.nt);
    for (int a = 0; a < 3; a++) { j.clo[a] = clo[a]; j.seed[a] = flood->seed[a]; }
    j.match = flood->match; j.connectivity = flood->connectivity; j.id = flood->id;
    const size_t ntiles = flood_tile_count(j.nt);
    FloodScratch scr;
    if (!flood_scratch_room(s, ntiles, &scr))
        return fail(VRT_ERR_UNSUPPORTED, name + ": no device memory for the masks of " + std::to_string(ntiles) + " tiles; flood in parts");
    j.passable = scr.passable; j.reached = scr.reached;
    const FloodRecord init = flood_record_init();
    FloodRecord rec = init;
    HIPCHK(hipMemsetAsync(scr.passable, 0, scr.zero_bytes, c->stream));
    HIPCHK(hipMemcpyAsync(scr.rec, &init, sizeof init, hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_flood_pass(j, scr.act[0], scr.rec, c->stream));
    // the rounds, in batches: one read of the batch's counters each.  Every round that marked a tile gained a bit, so more of them
    // than flood_round_bound cannot be
    const uint64_t bound = flood_round_bound(csize);
    uint64_t round = 0;
    uint32_t batch = 4, marked[kFloodBatchMax];
    for (bool done = false; !done;) {
        HIPCHK(hipMemsetAsync(scr.counters, 0, batch * 4, c->stream));
        for (uint32_t i = 0; i < batch; i++)
            HIPCHK(launch_flood_round(j, scr.act[(round + i) & 1u], scr.act[(round + i + 1u) & 1u], i ? scr.counters + i - 1u : nullptr, scr.counters + i, c->stream));
        HIPCHK(hipMemcpyAsync(marked, scr.counters, batch * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (uint32_t i = 0; i < batch && !done; i++) {
            round++;
            done = marked[i] == 0u;
        }
        if (!done && round > bound) return fail(VRT_ERR_HIP, name + ": internal error (more rounds than the bounds have voxels)");
        batch = batch * 2u < kFloodBatchMax ? batch * 2u : kFloodBatchMax;
    }
    s->flood_rounds = (uint32_t)(round < 0xFFFFFFFFull ? round : 0xFFFFFFFFull);
    HIPCHK(launch_flood_extent(j, scr.rec, c->stream));
    HIPCHK(hipMemcpyAsync(&rec, scr.rec, sizeof rec, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    vrt_flood_result out{};
    out.seed_id = rec.seed_id;
    out.region = rec.region;
    if (rec.region != 0ull) {
        for (int a = 0; a < 3; a++) {
            if (rec.mn[a] < clo[a] || rec.mx[a] < rec.mn[a] || (int64_t)rec.mx[a] >= (int64_t)clo[a] + (int64_t)csize[a])
                return fail(VRT_ERR_HIP, name + ": internal error (the region's bounds leave the flood's)");
            out.region_lo[a] = rec.mn[a]; out.region_size[a] = (uint32_t)(rec.mx[a] - rec.mn[a] + 1);
        }
    }
    if (!measure && rec.edit.changed != 0ull) {                  // (else: nothing is written, no edit pass runs, the count planes' fields stay)
        const VolumeView& d = s->d.vol;
        EditBox b;
        b.W = d.W; b.H = d.H; b.D = d.D;
        for (int a = 0; a < 3; a++) {
            if (rec.edit.mn[a] < clo[a] || rec.edit.mx[a] < rec.edit.mn[a] || (int64_t)rec.edit.mx[a] >= (int64_t)clo[a] + (int64_t)csize[a])
                return fail(VRT_ERR_HIP, name + ": internal error (the changed voxels' bounds leave the flood's)");
            b.lo[a] = rec.edit.mn[a]; b.hi[a] = rec.edit.mx[a] + 1;
            j.box.lo[a] = b.lo[a]; j.box.size[a] = (uint32_t)(b.hi[a] - b.lo[a]);
        }
        EditIds src;
        src.flood = &j; src.written = rec.edit.ids;
        const int rc = scene_edit_locked(c, s, b, src, name);
        if (rc != VRT_OK) return rc;
        out.edit.changed = rec.edit.changed;
        for (int a = 0; a < 3; a++) { out.edit.lo[a] = b.lo[a]; out.edit.size[a] = j.box.size[a]; }
    }
    *result = out;
    return VRT_OK;
}

int vrt_debug_flood_rounds(const vrt_scene* s, uint32_t* rounds)
{
    if (!s || !rounds) return fail(VRT_ERR_INVALID, "vrt_debug_flood_rounds: NULL argument");
    *rounds = s->flood_rounds;
    return VRT_OK;
}

} // extern "C"

// ---- mesh voxelization (vrt_scene_voxelize; csrc/vrt_voxelize.h) -----------------------------------------------------------------

static_assert(VRT_VOXELIZE_SURFACE == VRT_VOXELIZE_FILL_SURFACE && VRT_VOXELIZE_SOLID == VRT_VOXELIZE_FILL_SOLID,
              "include/vrt.h and csrc/vrt_voxelize.h number the fills differently");
static_assert(VRT_BRUSH_SET == 0 && VRT_BRUSH_PAINT == 1 && VRT_BRUSH_ADD == 2 && VRT_BRUSH_REPLACE == 3, "vox_job_ok spells the modes as numbers");

namespace {

// The voxelization's scratch memory: coverage mask | toggle mask | the record
struct VoxScratch { unsigned long long *cover, *toggle; VoxRecord* rec; size_t zero_bytes; };

bool vox_scratch_room(vrt_scene* s, const uint32_t csize[3], bool solid, VoxScratch* out)
{
    const size_t rows = (size_t)csize[1] * csize[2];
    const size_t cover = round256(rows * vox_cover_words(csize[0]) * 8u), toggle = solid ? round256(rows * vox_toggle_words(csize[0]) * 8u) : 0u;
    const size_t need = cover + toggle + round256(sizeof(VoxRecord));
    if (need > s->voxelize_scratch_bytes) {
        if (s->voxelize_scratch) { s->voxelize_scratch.reset(); s->bytes -= s->voxelize_scratch_bytes; }
        s->voxelize_scratch_bytes = 0;
        if (s->voxelize_scratch.alloc(need) != hipSuccess) { (void)hipGetLastError(); return false; }
        s->voxelize_scratch_bytes = need; s->bytes += need;
    }
    uint8_t* p = s->voxelize_scratch.get();
    out->cover = (unsigned long long*)p;
    out->toggle = solid ? (unsigned long long*)(p + cover) : nullptr;
    out->rec = (VoxRecord*)(p + cover + toggle);
    out->zero_bytes = cover + toggle;
    return true;
}

} // namespace

extern "C" {

int vrt_scene_voxelize(struct vrt_ctx* c, vrt_scene* s, const int32_t* vertices, uint32_t nv, const uint32_t* triangles, uint32_t nt,
                       const vrt_voxelize* job, vrt_voxelize_result* result)
{
    const std::string name("vrt_scene_voxelize");
    if (!c || !s || !vertices || !triangles || !job || !result) return fail(VRT_ERR_INVALID, name + ": NULL argument");
    if (nt < 1u || nt > VRT_VOXELIZE_MAX_TRIANGLES) return fail(VRT_ERR_INVALID, name + ": 1..2^20 triangles a call");
    if (nv < 1u || nv > VRT_VOXELIZE_MAX_VERTICES) return fail(VRT_ERR_INVALID, name + ": 1..2^24 vertices a call");
    if (job->mode < VRT_BRUSH_SET || job->mode > VRT_BRUSH_REPLACE) return fail(VRT_ERR_INVALID, name + ": unknown mode");
    if (job->fill == 0u || (job->fill & ~(uint32_t)(VRT_VOXELIZE_SURFACE | VRT_VOXELIZE_SOLID)) != 0u)
        return fail(VRT_ERR_INVALID, name + ": fill is VRT_VOXELIZE_SURFACE, VRT_VOXELIZE_SOLID or both");
    if (!brush_mode_ok(job->mode, job->id, job->match))
        return fail(VRT_ERR_INVALID, name + (job->mode == VRT_BRUSH_REPLACE ? ": REPLACE needs id != match" : ": PAINT and ADD need id != 0 (carve with SET)"));
    if (!vox_job_ok(job->mode, job->id, job->match, job->fill, job->size)) return fail(VRT_ERR_INVALID, name + ": each size of the bounds is in 1..2^30");
    for (size_t i = 0; i < (size_t)nv * 3u; i++)
        if (!vox_coord_ok(vertices[i]))
            return fail(VRT_ERR_INVALID, name + ": coordinate " + std::to_string(vertices[i]) + " of vertex " + std::to_string(i / 3u) + " is outside -65536..131072 (sixteenths of a voxel)");
    for (size_t i = 0; i < (size_t)nt * 3u; i++)
        if (triangles[i] >= nv) return fail(VRT_ERR_INVALID, name + ": triangle " + std::to_string(i / 3u) + " names vertex " + std::to_string(triangles[i]) + " of " + std::to_string(nv));
    const int32_t dim[3] = {s->d.vol.W, s->d.vol.H, s->d.vol.D};
    int64_t lo[3], hi[3];
    int32_t clo[3];
    uint32_t csize[3];
    for (int a = 0; a < 3; a++) { lo[a] = (int64_t)job->lo[a]; hi[a] = (int64_t)job->lo[a] + (int64_t)job->size[a]; }
    const bool any = brush_clip(lo, hi, dim, clo, csize);
    if (any && !vox_sides_ok(csize))
        return fail(VRT_ERR_INVALID, name + ": the bounds inside the volume have no side above " + std::to_string(VRT_VOXELIZE_MAX_SIDE) + "; voxelize in parts");
    memset(result, 0, sizeof *result);
    if (s->bricks && !s->reserved) return fail(VRT_ERR_UNSUPPORTED, name + ": a brick scene cannot be edited before vrt_scene_reserve_bricks");
    if (!any) return VRT_OK;                                     // bounds wholly outside the volume: nothing to do
    // the work items: every triangle's clipped box cut into slabs of rows (SURFACE) and of columns (SOLID)
    const bool surface = (job->fill & VRT_VOXELIZE_SURFACE) != 0u, solid = (job->fill & VRT_VOXELIZE_SOLID) != 0u;
    const uint32_t item_rows = s->voxelize_item_rows ? s->voxelize_item_rows : VRT_VOXELIZE_ITEM_ROWS;
    std::vector<VoxItem> items[2];
    uint64_t candidates = 0;
    for (uint32_t t = 0; t < nt; t++) {
        VoxTri T;
        int32_t blo[3], bhi[3];
        vox_tri_setup(vertices + 3u * (size_t)triangles[3u * (size_t)t], vertices + 3u * (size_t)triangles[3u * (size_t)t + 1u],
                      vertices + 3u * (size_t)triangles[3u * (size_t)t + 2u], T);
        for (int k = 0; k < 2; k++) {
            if (!(k == 0 ? surface : solid) || !vox_tri_box(T, k == 1, clo, csize, blo, bhi)) continue;
            const uint32_t rows = (uint32_t)(bhi[1] - blo[1] + 1) * (uint32_t)(bhi[2] - blo[2] + 1), step = k == 0 ? item_rows : item_rows * 64u;
            candidates += k == 0 ? (uint64_t)rows * (uint64_t)(bhi[0] - blo[0] + 1) : (uint64_t)rows;
            for (uint32_t f = 0; f < rows; f += step) items[k].push_back(VoxItem{t, f, rows - f < step ? rows - f : step});
        }
        if (candidates > VRT_VOXELIZE_MAX_CANDIDATES || items[0].size() + items[1].size() > VRT_VOXELIZE_MAX_ITEMS)
            return fail(VRT_ERR_UNSUPPORTED, name + ": more than 2^31 candidate voxels or 2^24 work items (the triangles' boxes cut to the bounds); voxelize in parts");
    }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::lock_guard<std::mutex> lock(s->lazy);
    VoxJob j{};
    j.box = read_box_of(s, clo, csize);
    for (int a = 0; a < 3; a++) { j.clo[a] = clo[a]; j.csize[a] = csize[a]; }
    j.mode = job->mode; j.id = job->id; j.match = job->match;
    VoxScratch scr;
    if (!vox_scratch_room(s, csize, solid, &scr)) return fail(VRT_ERR_UNSUPPORTED, name + ": no device memory for the masks; voxelize in parts");
    j.cover = scr.cover; j.toggle = scr.toggle;
    // the mesh and the items, uploaded on the context's stream; they go when this returns
    const size_t vbytes = (size_t)nv * 12u, tbytes = (size_t)nt * 12u, ibytes[2] = {items[0].size() * sizeof(VoxItem), items[1].size() * sizeof(VoxItem)};
    const size_t voff = 0, toff = round256(vbytes), ioff0 = toff + round256(tbytes), ioff1 = ioff0 + round256(ibytes[0]);
    DevBuf<uint8_t> mesh;
    if (mesh.alloc(ioff1 + round256(ibytes[1]) + 256u) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VRT_ERR_UNSUPPORTED, name + ": no device memory for the mesh and its work items");
    }
    HIPCHK(hipMemcpyAsync(mesh.get() + voff, vertices, vbytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(mesh.get() + toff, triangles, tbytes, hipMemcpyHostToDevice, c->stream));
    if (ibytes[0]) HIPCHK(hipMemcpyAsync(mesh.get() + ioff0, items[0].data(), ibytes[0], hipMemcpyHostToDevice, c->stream));
    if (ibytes[1]) HIPCHK(hipMemcpyAsync(mesh.get() + ioff1, items[1].data(), ibytes[1], hipMemcpyHostToDevice, c->stream));
    j.vertices = (const int32_t*)(mesh.get() + voff); j.triangles = (const uint32_t*)(mesh.get() + toff);
    const VoxRecord init = vox_record_init();
    VoxRecord rec = init;
    HIPCHK(hipMemsetAsync(scr.cover, 0, scr.zero_bytes, c->stream));
    HIPCHK(hipMemcpyAsync(scr.rec, &init, sizeof init, hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_vox_surface(j, (const VoxItem*)(mesh.get() + ioff0), (uint32_t)items[0].size(), c->stream));
    if (solid) {
        HIPCHK(launch_vox_cross(j, (const VoxItem*)(mesh.get() + ioff1), (uint32_t)items[1].size(), c->stream));
        HIPCHK(launch_vox_scan(j, c->stream));
    }
    s->voxelize_items = (uint32_t)(items[0].size() + items[1].size());
    HIPCHK(launch_vox_extent(j, scr.rec, c->stream));
    HIPCHK(hipMemcpyAsync(&rec, scr.rec, sizeof rec, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                     // (the mesh's device copy is read no more)
    vrt_voxelize_result out{};
    out.covered = rec.covered;
    if (rec.edit.changed != 0ull) {                              // (else: nothing is written, no edit pass runs, the count planes' fields stay)
        const VolumeView& d = s->d.vol;
        EditBox b;
        b.W = d.W; b.H = d.H; b.D = d.D;
        for (int a = 0; a < 3; a++) {
            if (rec.edit.mn[a] < clo[a] || rec.edit.mx[a] < rec.edit.mn[a] || (int64_t)rec.edit.mx[a] >= (int64_t)clo[a] + (int64_t)csize[a])
                return fail(VRT_ERR_HIP, name + ": internal error (the changed voxels' bounds leave the call's)");
            b.lo[a] = rec.edit.mn[a]; b.hi[a] = rec.edit.mx[a] + 1;
            j.box.lo[a] = b.lo[a]; j.box.size[a] = (uint32_t)(b.hi[a] - b.lo[a]);
        }
        EditIds src;
        src.voxelize = &j; src.written = rec.edit.ids;
        const int rc = scene_edit_locked(c, s, b, src, name);
        if (rc != VRT_OK) return rc;
        out.edit.changed = rec.edit.changed;
        for (int a = 0; a < 3; a++) { out.edit.lo[a] = b.lo[a]; out.edit.size[a] = j.box.size[a]; }
    }
    *result = out;
    return VRT_OK;
}

int vrt_debug_voxelize_item_rows(vrt_scene* s, uint32_t rows)
{
    if (!s) return fail(VRT_ERR_INVALID, "vrt_debug_voxelize_item_rows: NULL argument");
    s->voxelize_item_rows = rows;
    return VRT_OK;
}

int vrt_debug_voxelize_items(const vrt_scene* s, uint32_t* items)
{
    if (!s || !items) return fail(VRT_ERR_INVALID, "vrt_debug_voxelize_items: NULL argument");
    *items = s->voxelize_items;
    return VRT_OK;
}

} // extern "C"
