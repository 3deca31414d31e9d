// vrt_api_edit.hip -- what rewrites a scene through the C-ABI: edits of dense scenes and of reserved brick scenes
// (vrt_scene_reserve_bricks, vrt_scene_edit_box, vrt_scene_fill_box), and the edits whose ids a kernel composes: brushes and stamps,
// flood fills (whose loop over rounds lives here), mesh voxelization (whose cut of the triangles into work items lives here)
// and morphology (whose phases are launched here), and the connected components (whose passes are launched here; listing them writes nothing).
// Host code only; the kernels are vrt_scene_edit.hip, vrt_scene_build.hip, vrt_brush.hip, vrt_flood.hip, vrt_voxelize.hip, vrt_morph.hip and vrt_components.hip.
// vrt_api_scene.hip makes, describes and reads the scenes.
#include <cstddef>
#include <cstring>

#include "vrt_host.h"
#include "vrt_brush_launch.h"          // (brings vrt_scene_read.h and its launchers)
#include "vrt_flood_launch.h"
#include "vrt_voxelize_launch.h"
#include "vrt_morph_launch.h"
#include "vrt_components_launch.h"

using namespace vrt;

static_assert(VRT_BRUSH_BOX == VRT_BRUSH_SHAPE_BOX && VRT_BRUSH_ELLIPSOID == VRT_BRUSH_SHAPE_ELLIPSOID && VRT_BRUSH_CAPSULE == VRT_BRUSH_SHAPE_CAPSULE,
              "include/vrt.h and csrc/vrt_brush.h number the shapes differently");
static_assert(VRT_BRUSH_SET == VRT_BRUSH_MODE_SET && VRT_BRUSH_PAINT == VRT_BRUSH_MODE_PAINT && VRT_BRUSH_ADD == VRT_BRUSH_MODE_ADD &&
              VRT_BRUSH_REPLACE == VRT_BRUSH_MODE_REPLACE, "include/vrt.h and csrc/vrt_brush.h number the modes differently");
static_assert(VRT_FLOOD_SAME == VRT_FLOOD_MATCH_SAME && VRT_FLOOD_SOLID == VRT_FLOOD_MATCH_SOLID && VRT_FLOOD_FACES == VRT_FLOOD_CONN_FACES &&
              VRT_FLOOD_CORNERS == VRT_FLOOD_CONN_CORNERS && VRT_FLOOD_MEASURE == VRT_FLOOD_FLAG_MEASURE,
              "include/vrt.h and csrc/vrt_flood.h number the predicates, connectivities or flags differently");
static_assert(VRT_VOXELIZE_SURFACE == VRT_VOXELIZE_FILL_SURFACE && VRT_VOXELIZE_SOLID == VRT_VOXELIZE_FILL_SOLID,
              "include/vrt.h and csrc/vrt_voxelize.h number the fills differently");
static_assert(VRT_MORPH_DILATE == VRT_MORPH_OP_DILATE && VRT_MORPH_ERODE == VRT_MORPH_OP_ERODE && VRT_MORPH_OPEN == VRT_MORPH_OP_OPEN &&
              VRT_MORPH_CLOSE == VRT_MORPH_OP_CLOSE && VRT_MORPH_HOLLOW == VRT_MORPH_OP_HOLLOW && VRT_MORPH_FACES == VRT_MORPH_CONN_FACES &&
              VRT_MORPH_CORNERS == VRT_MORPH_CONN_CORNERS && VRT_MORPH_BORDER_SOLID == VRT_MORPH_FLAG_BORDER_SOLID && VRT_MORPH_MEASURE == VRT_MORPH_FLAG_MEASURE,
              "include/vrt.h and csrc/vrt_morph.h number the operations, connectivities or flags differently");
static_assert(VRT_COMP_SOLID == VRT_COMP_MATCH_SOLID && VRT_COMP_SAME == VRT_COMP_MATCH_SAME && VRT_COMP_EMPTY == VRT_COMP_MATCH_EMPTY &&
              VRT_COMP_FACES == VRT_COMP_CONN_FACES && VRT_COMP_CORNERS == VRT_COMP_CONN_CORNERS && VRT_COMP_KEEP_LARGEST == VRT_COMP_FLAG_KEEP_LARGEST &&
              VRT_COMP_MEASURE == VRT_COMP_FLAG_MEASURE, "include/vrt.h and csrc/vrt_components.h number the predicates, connectivities or flags differently");
static_assert(sizeof(vrt_component) == sizeof(CompRecord) && offsetof(vrt_component, root) == offsetof(CompRecord, root) && offsetof(vrt_component, id) == offsetof(CompRecord, id) &&
              offsetof(vrt_component, voxels) == offsetof(CompRecord, voxels) && offsetof(vrt_component, lo) == offsetof(CompRecord, lo) &&
              offsetof(vrt_component, size) == offsetof(CompRecord, size) && offsetof(vrt_component, faces) == offsetof(CompRecord, faces) &&
              offsetof(vrt_component, reserved) == offsetof(CompRecord, reserved), "include/vrt.h and csrc/vrt_components.h lay the record out differently");
static_assert(VRT_BRUSH_SET == 0 && VRT_BRUSH_PAINT == 1 && VRT_BRUSH_ADD == 2 && VRT_BRUSH_REPLACE == 3, "vox_job_ok spells the modes as numbers");

namespace {

// Where the ids of an edited box come from: the host (uploaded), one id for the whole box, or -- a brush, a stamp, a flood, a
// voxelization -- a kernel that composes them in the scratch memory, where the upload would have put them
typedef hipError_t (*ComposeFn)(const void* job, uint8_t* ids, hipStream_t st);
struct EditIds {
    const uint8_t*  host = nullptr;       // the box's ids in box-index order, or
    uint8_t         id = 0;               // (host and compose both NULL) one id for the whole box, or
    ComposeFn       compose = nullptr;    // the producer: an adapter to a launch_*_compose, with
    const void*     job = nullptr;        // the job it is given, whose box is the edit's, and
    const uint32_t* written = nullptr;    // the set of ids the kernel writes (BrushRecord::ids)
    bool boxed() const { return host != nullptr || compose != nullptr; }
};

// Did the edit bring a metallic voxel?  From then on the scene's rays may bounce.
void note_metallic(vrt_scene* s, const EditIds& src, size_t nbox)
{
    if (s->metallic_voxels) return;
    if (src.compose) { for (int i = 1; i < 256 && !s->metallic_voxels; i++) s->metallic_voxels = ((src.written[i >> 5] >> (i & 31)) & 1u) != 0u && s->metal[i]; }
    else if (src.host) { for (size_t i = 0; i < nbox && !s->metallic_voxels; i++) s->metallic_voxels = src.host[i] != 0 && s->metal[src.host[i]]; }
    else s->metallic_voxels = src.id != 0 && s->metal[src.id];
}

// the box's ids into the scratch memory (src.boxed())
hipError_t edit_ids_to_scratch(vrt_ctx* c, const EditIds& src, uint8_t* dev, size_t nbox)
{
    if (src.compose) return src.compose(src.job, dev, c->stream);
    return hipMemcpyAsync(dev, src.host, nbox, hipMemcpyHostToDevice, c->stream);
}

// VRT_OK, or what every call that rewrites a scene answers for a brick scene without a reserved pool
int editable(const vrt_scene* s, const std::string& name)
{
    if (s->bricks && !s->reserved) return fail(VRT_ERR_UNSUPPORTED, name + ": a brick scene cannot be edited before vrt_scene_reserve_bricks");
    return VRT_OK;
}

// the box [lo, lo + size) cut to the scene's volume -> clo, csize; false: nothing is left
bool clip_box(const vrt_scene* s, const int32_t lo[3], const uint32_t size[3], int32_t clo[3], uint32_t csize[3])
{
    const int32_t dim[3] = {s->d.vol.W, s->d.vol.H, s->d.vol.D};
    int64_t l[3], h[3];
    for (int a = 0; a < 3; a++) { l[a] = (int64_t)lo[a]; h[a] = (int64_t)lo[a] + (int64_t)size[a]; }
    return brush_clip(l, h, dim, clo, csize);
}

// ---- editable brick scenes (vrt_scene_reserve_bricks; csrc/vrt_brick_edit.h) ------------------------------------------------

const uint32_t kNoBrick = 0xFFFFFFFFu;

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
           b.npad * 4ull + b.n + 8ull * b.cstride + s->scratch_bytes();
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
    HIPCHK(s->edit_scratch.room(ids_room + 2 * t_room + list_room + coarse_room, s->bytes));
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

// An edit of the box b, which lies inside the volume, with the ids of src; the caller checked that the scene is editable,
// waited for the stream and holds the lock
int scene_edit_locked(vrt_ctx* c, vrt_scene* s, const EditBox& b, const EditIds& src, const std::string& name)
{
    s->edit_gen++;                                               // whatever was labelled before is stale (vrt_scene_component_labels), even if the edit is refused
    if (s->bricks) return brick_scene_edit(c, s, b, src, name);
    const VolumeView& d = s->d.vol;
    const size_t nbox = (size_t)(b.hi[0] - b.lo[0]) * (size_t)(b.hi[1] - b.lo[1]) * (size_t)(b.hi[2] - b.lo[2]);
    const bool ids = src.boxed();
    note_metallic(s, src, nbox);
    drop_count_fields(s);
    const bool in_place = edit_in_place(d.W, d.H, d.D, b.lo, b.hi, VRT_EDIT_CAP);
    size_t need = ids ? round256(nbox) : 0;
    const size_t ids_room = need;
    if (in_place) need += edit_scratch_bytes(b, s->open_cells);
    HIPCHK(s->edit_scratch.room(need, s->bytes));
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
int scene_edit(vrt_ctx* c, vrt_scene* s, const int32_t lo[3], const uint32_t size[3], const uint8_t* ids, uint8_t id, const char* who)
{
    const std::string name(who);
    if (const int rc = editable(s, name)) return rc;
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

// The tail of an edit whose ids a kernel composes.  rec: what the extent kernel found inside the clipped bounds [clo, clo + csize).
// If anything changes, the tight box of the changes is edited with the ids that `compose` writes for `job`, whose ReadBox `box`
// is narrowed to it first.  whose: the noun of the internal error.  *out (may be NULL) holds zeros.
int composed_edit(vrt_ctx* c, vrt_scene* s, const BrushRecord& rec, const int32_t clo[3], const uint32_t csize[3], ReadBox& box, ComposeFn compose,
                  const void* job, const char* whose, const std::string& name, vrt_brush_result* out)
{
    if (rec.changed == 0ull) return VRT_OK;                     // nothing is written, no edit pass runs, the count planes' fields stay
    if (!brush_extent_ok(rec.mn, rec.mx, clo, csize)) return fail(VRT_ERR_HIP, name + ": internal error (the changed voxels' bounds leave " + whose + ")");
    const VolumeView& d = s->d.vol;
    EditBox b;
    b.W = d.W; b.H = d.H; b.D = d.D;
    for (int a = 0; a < 3; a++) {
        b.lo[a] = rec.mn[a]; b.hi[a] = rec.mx[a] + 1;
        box.lo[a] = b.lo[a]; box.size[a] = (uint32_t)(b.hi[a] - b.lo[a]);
    }
    EditIds src;
    src.compose = compose; src.job = job; src.written = rec.ids;
    const int rc = scene_edit_locked(c, s, b, src, name);
    if (rc == VRT_OK && out) {
        out->changed = rec.changed;
        for (int a = 0; a < 3; a++) { out->lo[a] = b.lo[a]; out->size[a] = box.size[a]; }
    }
    return rc;
}

// ---- brushes and stamps (vrt_scene_brush, vrt_scene_stamp; csrc/vrt_brush.h) ---------------------------------------------------

hipError_t brush_compose(const void* job, uint8_t* ids, hipStream_t st) { return launch_brush_compose(*(const BrushJob*)job, ids, st); }

// One brush or stamp over the clipped bounds [clo, clo + csize) of the scene j.box views: the extent kernel says what changes, the
// tail edits it.  The caller checked the arguments, waited for the stream and holds the scene's lock.  *out (may be NULL) holds zeros.
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
    return composed_edit(c, s, rec, clo, csize, j.box, brush_compose, &j, "the brush's", name, out);
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
    if (const int rc = editable(s, name)) return rc;
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
    if (const int rcd = editable(dst, name)) return rcd;
    uint32_t dsize[3], csize[3];
    int32_t clo[3];
    stamp_dst_size(orient, size, dsize);
    if (!clip_box(dst, dst_lo, dsize, clo, csize)) return VRT_OK;  // wholly outside the destination
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

namespace {

const uint32_t kFloodBatchMax = 32;     // rounds enqueued between two reads of the counters

hipError_t flood_compose(const void* job, uint8_t* ids, hipStream_t st) { return launch_flood_compose(*(const FloodJob*)job, ids, st); }

// The flood's scratch memory: passable mask | reached mask | two sets of activity flags | the rounds' counters | the record
struct FloodScratch { uint8_t *passable, *reached; uint32_t *act[2], *counters; FloodRecord* rec; size_t zero_bytes; };

bool flood_scratch_room(vrt_scene* s, size_t ntiles, FloodScratch* out)
{
    const size_t mask = ntiles * VRT_FLOOD_TILE_BYTES, flags = round256(ntiles * 4), counters = round256(kFloodBatchMax * 4), rec = round256(sizeof(FloodRecord));
    if (s->flood_scratch.room(2 * mask + 2 * flags + counters + rec, s->bytes) != hipSuccess) { (void)hipGetLastError(); return false; }
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
    int32_t clo[3];
    uint32_t csize[3];
    const bool any = clip_box(s, flood->lo, flood->size, clo, csize);
    if (any && !flood_sides_ok(csize))
        return fail(VRT_ERR_INVALID, name + ": the bounds inside the volume have no side above " + std::to_string(VRT_FLOOD_MAX_SIDE) + "; flood in parts");
    memset(result, 0, sizeof *result);
    if (const int rc = measure ? VRT_OK : editable(s, name)) return rc;
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
        if (!brush_extent_ok(rec.mn, rec.mx, clo, csize)) return fail(VRT_ERR_HIP, name + ": internal error (the region's bounds leave the flood's)");
        for (int a = 0; a < 3; a++) { out.region_lo[a] = rec.mn[a]; out.region_size[a] = (uint32_t)(rec.mx[a] - rec.mn[a] + 1); }
    }
    if (!measure) {
        const int rc = composed_edit(c, s, rec.edit, clo, csize, j.box, flood_compose, &j, "the flood's", name, &out.edit);
        if (rc != VRT_OK) return rc;
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

namespace {

hipError_t vox_compose(const void* job, uint8_t* ids, hipStream_t st) { return launch_vox_compose(*(const VoxJob*)job, ids, st); }

// The voxelization's scratch memory: coverage mask | toggle mask | the record
struct VoxScratch { unsigned long long *cover, *toggle; VoxRecord* rec; size_t zero_bytes; };

bool vox_scratch_room(vrt_scene* s, const uint32_t csize[3], bool solid, VoxScratch* out)
{
    const size_t rows = (size_t)csize[1] * csize[2];
    const size_t cover = round256(rows * vox_cover_words(csize[0]) * 8u), toggle = solid ? round256(rows * vox_toggle_words(csize[0]) * 8u) : 0u;
    if (s->voxelize_scratch.room(cover + toggle + round256(sizeof(VoxRecord)), s->bytes) != hipSuccess) { (void)hipGetLastError(); return false; }
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
    int32_t clo[3];
    uint32_t csize[3];
    const bool any = clip_box(s, job->lo, job->size, clo, csize);
    if (any && !vox_sides_ok(csize))
        return fail(VRT_ERR_INVALID, name + ": the bounds inside the volume have no side above " + std::to_string(VRT_VOXELIZE_MAX_SIDE) + "; voxelize in parts");
    memset(result, 0, sizeof *result);
    if (const int rc = editable(s, name)) return rc;
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
    const int rc = composed_edit(c, s, rec.edit, clo, csize, j.box, vox_compose, &j, "the call's", name, &out.edit);
    if (rc != VRT_OK) return rc;
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

// ---- morphology (vrt_scene_morph; csrc/vrt_morph.h) -------------------------------------------------------------------------------

namespace {

hipError_t morph_compose(const void* job, uint8_t* ids, hipStream_t st) { return launch_morph_compose(*(const MorphJob*)job, ids, st); }

} // namespace

extern "C" {

int vrt_scene_morph(struct vrt_ctx* c, vrt_scene* s, const vrt_morph* morph, vrt_morph_result* result)
{
    const std::string name("vrt_scene_morph");
    if (!c || !s || !morph || !result) return fail(VRT_ERR_INVALID, name + ": NULL argument");
    if (morph->op < VRT_MORPH_DILATE || morph->op > VRT_MORPH_HOLLOW) return fail(VRT_ERR_INVALID, name + ": unknown operation (VRT_MORPH_DILATE .. VRT_MORPH_HOLLOW)");
    if (morph->connectivity != VRT_MORPH_FACES && morph->connectivity != VRT_MORPH_CORNERS)
        return fail(VRT_ERR_INVALID, name + ": connectivity is VRT_MORPH_FACES (6) or VRT_MORPH_CORNERS (26)");
    if (morph->radius < 1 || morph->radius > VRT_MORPH_MAX_RADIUS) return fail(VRT_ERR_INVALID, name + ": the radius is in 1.." + std::to_string(VRT_MORPH_MAX_RADIUS));
    if (morph->flags & ~(uint32_t)(VRT_MORPH_BORDER_SOLID | VRT_MORPH_MEASURE)) return fail(VRT_ERR_INVALID, name + ": unknown flag");
    if (morph_adds(morph->op) && morph->id == 0) return fail(VRT_ERR_INVALID, name + ": DILATE and CLOSE need id != 0 (the id of the voxels they add)");
    if (!morph_args_ok(morph->op, morph->connectivity, morph->radius, morph->flags, morph->id, morph->size)) return fail(VRT_ERR_INVALID, name + ": each size of the bounds is in 1..2^30");
    const bool measure = (morph->flags & VRT_MORPH_MEASURE) != 0u;
    int32_t clo[3];
    uint32_t csize[3];
    const bool any = clip_box(s, morph->lo, morph->size, clo, csize);
    if (any && !morph_sides_ok(csize))
        return fail(VRT_ERR_INVALID, name + ": the bounds inside the volume have no side above " + std::to_string(VRT_MORPH_MAX_SIDE) + "; work in parts");
    memset(result, 0, sizeof *result);
    if (const int rc = measure ? VRT_OK : editable(s, name)) return rc;
    if (!any) return VRT_OK;                                     // bounds wholly outside the volume: nothing to do
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::lock_guard<std::mutex> lock(s->lazy);
    MorphJob j{};
    j.box = read_box_of(s, clo, csize);
    j.dim[0] = s->d.vol.W; j.dim[1] = s->d.vol.H; j.dim[2] = s->d.vol.D;
    morph_domain(clo, csize, morph_halo(morph->op, morph->radius), j.mlo, j.msize);
    j.op = morph->op; j.connectivity = morph->connectivity; j.radius = (uint32_t)morph->radius;
    j.border_solid = (morph->flags & VRT_MORPH_BORDER_SOLID) ? 1u : 0u; j.id = morph->id;
    // scratch: mask A | mask B | the record
    const size_t mask = round256(morph_mask_words(j.msize) * 4u);
    if (s->morph_scratch.room(2 * mask + round256(sizeof(MorphRecord)), s->bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VRT_ERR_UNSUPPORTED, name + ": no device memory for two masks of " + std::to_string(mask) + " bytes; work in parts");
    }
    j.mask[0] = (uint32_t*)s->morph_scratch.get(); j.mask[1] = (uint32_t*)(s->morph_scratch.get() + mask);
    MorphRecord* const rec_dev = (MorphRecord*)(s->morph_scratch.get() + 2 * mask);
    const MorphRecord init = morph_record_init();
    MorphRecord rec = init;
    HIPCHK(hipMemcpyAsync(rec_dev, &init, sizeof init, hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_morph_pass(j, c->stream));
    const uint32_t phases = morph_phases(morph->op);
    for (uint32_t p = 0; p < phases; p++) HIPCHK(launch_morph_step(j, j.mask[p & 1u], j.mask[(p + 1u) & 1u], morph_phase_erodes(morph->op, p), c->stream));
    j.result = j.mask[phases & 1u];
    HIPCHK(launch_morph_extent(j, rec_dev, c->stream));
    HIPCHK(hipMemcpyAsync(&rec, rec_dev, sizeof rec, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    vrt_morph_result out{};
    out.added = rec.added; out.removed = rec.removed;
    if (rec.added + rec.removed != rec.edit.changed) return fail(VRT_ERR_HIP, name + ": internal error (added + removed != changed)");
    if (!measure) {
        const int rc = composed_edit(c, s, rec.edit, clo, csize, j.box, morph_compose, &j, "the bounds", name, &out.edit);
        if (rc != VRT_OK) return rc;
    }
    *result = out;
    return VRT_OK;
}

} // extern "C"

// ---- connected components (vrt_scene_components, vrt_scene_component_labels, vrt_scene_filter_components; csrc/vrt_components.h) --

namespace {

hipError_t comp_compose(const void* job, uint8_t* ids, hipStream_t st) { return launch_comp_compose(*(const CompJob*)job, ids, st); }

// One labelling and where its results lie: comp_scratch is label volume | the segments' counts | the summary | the filter's record
struct CompRun { CompJob j; CompSummary sum; CompSummary* sum_dev; BrushRecord* rec_dev; };

void comp_scratch_layout(const vrt_scene* s, const uint32_t csize[3], size_t* labels, size_t* work)
{
    *labels = round256((size_t)csize[0] * csize[1] * csize[2] * 4u);
    *work = round256(((size_t)list_segments_per_row(csize[0]) * csize[1] * csize[2] + 2u) * 4u);
}

// what the checks every entry point makes of a vrt_components leave: VRT_OK and *any (false: the bounds lie outside the volume)
int comp_bounds(const vrt_scene* s, const vrt_components* q, const std::string& name, int32_t clo[3], uint32_t csize[3], bool* any)
{
    if (!comp_match_ok(q->match)) return fail(VRT_ERR_INVALID, name + ": unknown match (VRT_COMP_SOLID, VRT_COMP_SAME or VRT_COMP_EMPTY)");
    if (!comp_conn_ok(q->connectivity)) return fail(VRT_ERR_INVALID, name + ": connectivity is VRT_COMP_FACES (6) or VRT_COMP_CORNERS (26)");
    if (q->flags != 0u) return fail(VRT_ERR_INVALID, name + ": unknown flag");
    if (!comp_args_ok(q->match, q->connectivity, q->flags, q->size)) return fail(VRT_ERR_INVALID, name + ": each size of the bounds is in 1..2^30");
    *any = clip_box(s, q->lo, q->size, clo, csize);
    if (*any && !comp_sides_ok(csize))
        return fail(VRT_ERR_INVALID, name + ": the bounds inside the volume have no side above " + std::to_string(VRT_COMP_MAX_SIDE) + "; work in parts");
    return VRT_OK;
}

// The passes of vrt_components.h over the clipped bounds [clo, clo + csize).  The caller checked the arguments, waited for the stream
// and holds the scene's lock.  Returns when the stream is done: the label volume, the table and run->sum are complete.
int comp_label(vrt_ctx* c, vrt_scene* s, const vrt_components* q, const int32_t clo[3], const uint32_t csize[3], const std::string& name, CompRun* run)
{
    CompJob& j = run->j;
    j = CompJob{};
    j.box = read_box_of(s, clo, csize);
    for (int a = 0; a < 3; a++) { j.clo[a] = clo[a]; j.csize[a] = csize[a]; }
    comp_tiles(csize, j.nt);
    j.match = q->match; j.connectivity = q->connectivity;
    size_t labels, work;
    comp_scratch_layout(s, csize, &labels, &work);
    s->comp_valid = false;
    if (s->comp_scratch.room(labels + work + round256(sizeof(CompSummary)) + round256(sizeof(BrushRecord)), s->bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VRT_ERR_UNSUPPORTED, name + ": no device memory for a label volume of " + std::to_string(labels) + " bytes; work in parts");
    }
    uint8_t* const p = s->comp_scratch.get();
    j.labels = (uint32_t*)p;
    uint32_t* const work_dev = (uint32_t*)(p + labels);
    run->sum_dev = (CompSummary*)(p + labels + work);
    run->rec_dev = (BrushRecord*)(p + labels + work + round256(sizeof(CompSummary)));
    const uint32_t nseg = list_segments_per_row(csize[0]) * csize[1] * csize[2];
    uint32_t total = 0;
    HIPCHK(hipMemsetAsync(run->sum_dev, 0, sizeof(CompSummary), c->stream));
    HIPCHK(launch_comp_tile(j, c->stream));
    HIPCHK(launch_comp_seam(j, c->stream));
    HIPCHK(launch_comp_flatten(j, work_dev, c->stream));
    HIPCHK(launch_list_scan(work_dev, nseg, c->stream));
    HIPCHK(hipMemcpyAsync(&total, work_dev + nseg, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    j.ncomp = total;
    run->sum = CompSummary{};
    if (total != 0u) {
        if (s->comp_table.room((size_t)total * sizeof(CompStat), s->bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(VRT_ERR_UNSUPPORTED, name + ": no device memory for a table of " + std::to_string(total) + " components; work in parts");
        }
        j.table = (CompStat*)s->comp_table.get();
        HIPCHK(launch_comp_number(j, work_dev, c->stream));
        HIPCHK(launch_comp_measure(j, c->stream));
        HIPCHK(launch_comp_summary(j, run->sum_dev, c->stream));
        HIPCHK(hipMemcpyAsync(&run->sum, run->sum_dev, sizeof(CompSummary), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    s->comp_valid = true; s->comp_gen = s->edit_gen;
    for (int a = 0; a < 3; a++) { s->comp_clo[a] = clo[a]; s->comp_csize[a] = csize[a]; }
    return VRT_OK;
}

} // namespace

extern "C" {

int vrt_scene_components(struct vrt_ctx* c, const vrt_scene* scene, const vrt_components* q, vrt_component* records, uint64_t capacity, vrt_components_result* result)
{
    const std::string name("vrt_scene_components");
    if (!c || !scene || !q || !result) return fail(VRT_ERR_INVALID, name + ": NULL argument");
    vrt_scene* const s = const_cast<vrt_scene*>(scene);          // the scene's content is not written: its scratch memory and its lock are
    int32_t clo[3];
    uint32_t csize[3];
    bool any = false;
    if (const int rc = comp_bounds(s, q, name, clo, csize, &any)) return rc;
    memset(result, 0, sizeof *result);
    if (!any) return VRT_OK;                                     // bounds wholly outside the volume: no components
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::lock_guard<std::mutex> lock(s->lazy);
    CompRun run;
    if (const int rc = comp_label(c, s, q, clo, csize, name, &run)) return rc;
    const uint64_t n = run.j.ncomp;
    result->components = n; result->voxels = run.sum.voxels;
    result->largest = n ? (uint64_t)comp_largest_number(run.sum.largest) : 0ull;
    if (!records || !n) return VRT_OK;
    if (capacity < n) return fail(VRT_ERR_INVALID, name + ": the bounds have " + std::to_string(n) + " components and `records` room for " + std::to_string(capacity));
    std::vector<CompStat> table(n);
    HIPCHK(hipMemcpyAsync(table.data(), run.j.table, n * sizeof(CompStat), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (uint64_t k = 0; k < n; k++) {
        const CompRecord r = comp_record_of(table[k], clo, csize);
        memcpy(records + k, &r, sizeof r);
    }
    return VRT_OK;
}

int vrt_scene_component_labels(struct vrt_ctx* c, const vrt_scene* scene, const int32_t lo[3], const uint32_t size[3], uint32_t* labels)
{
    const std::string name("vrt_scene_component_labels");
    if (!c || !scene || !lo || !size || !labels) return fail(VRT_ERR_INVALID, name + ": NULL argument");
    vrt_scene* const s = const_cast<vrt_scene*>(scene);
    for (int a = 0; a < 3; a++)
        if (size[a] == 0u) return fail(VRT_ERR_INVALID, name + ": the box is empty");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::lock_guard<std::mutex> lock(s->lazy);
    if (!s->comp_valid) return fail(VRT_ERR_INVALID, name + ": the scene has no labelling (vrt_scene_components makes one; vrt_scene_trim drops it)");
    if (s->comp_gen != s->edit_gen) return fail(VRT_ERR_INVALID, name + ": the scene was edited after its latest labelling; label it again");
    for (int a = 0; a < 3; a++)
        if (lo[a] < s->comp_clo[a] || (int64_t)lo[a] + (int64_t)size[a] > (int64_t)s->comp_clo[a] + (int64_t)s->comp_csize[a])
            return fail(VRT_ERR_INVALID, name + ": the box leaves the bounds of the latest labelling");
    const size_t n = (size_t)size[0] * size[1] * size[2];
    DevBuf<uint32_t> stage;
    if (stage.alloc(n * 4u) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VRT_ERR_UNSUPPORTED, name + ": no device memory for a staging buffer of " + std::to_string(n * 4u) + " bytes; read the labels in parts");
    }
    CompJob j{};
    for (int a = 0; a < 3; a++) { j.clo[a] = s->comp_clo[a]; j.csize[a] = s->comp_csize[a]; }
    j.labels = (uint32_t*)s->comp_scratch.get();
    HIPCHK(launch_comp_labels(j, lo, size, stage.get(), c->stream));
    HIPCHK(hipMemcpyAsync(labels, stage.get(), n * 4u, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return VRT_OK;
}

int vrt_scene_filter_components(struct vrt_ctx* c, vrt_scene* s, const vrt_components* q, const vrt_component_filter* f, vrt_filter_result* result)
{
    const std::string name("vrt_scene_filter_components");
    if (!c || !s || !q || !f || !result) return fail(VRT_ERR_INVALID, name + ": NULL argument");
    if (f->flags & ~(uint32_t)(VRT_COMP_KEEP_LARGEST | VRT_COMP_MEASURE)) return fail(VRT_ERR_INVALID, name + ": unknown filter flag");
    if (f->min_voxels > f->max_voxels) return fail(VRT_ERR_INVALID, name + ": min_voxels > max_voxels");
    if (!comp_filter_ok(f->min_voxels, f->max_voxels, f->faces_all, f->faces_none, f->flags)) return fail(VRT_ERR_INVALID, name + ": a face mask has the bits 0..5");
    int32_t clo[3];
    uint32_t csize[3];
    bool any = false;
    if (const int rc = comp_bounds(s, q, name, clo, csize, &any)) return rc;
    const bool measure = (f->flags & VRT_COMP_MEASURE) != 0u;
    memset(result, 0, sizeof *result);
    if (const int rc = measure ? VRT_OK : editable(s, name)) return rc;
    if (!any) return VRT_OK;                                     // bounds wholly outside the volume: nothing to do
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::lock_guard<std::mutex> lock(s->lazy);
    CompRun run;
    if (const int rc = comp_label(c, s, q, clo, csize, name, &run)) return rc;
    if (run.j.ncomp == 0u) return VRT_OK;
    CompJob& j = run.j;
    j.id = f->id;
    CompFilter F{};
    F.min_voxels = f->min_voxels; F.max_voxels = f->max_voxels; F.faces_all = f->faces_all; F.faces_none = f->faces_none; F.flags = f->flags;
    F.largest = comp_largest_number(run.sum.largest);
    const BrushRecord init = brush_record_init();
    BrushRecord rec = init;
    HIPCHK(launch_comp_select(j, F, run.sum_dev, c->stream));
    if (!measure) {
        HIPCHK(hipMemcpyAsync(run.rec_dev, &init, sizeof init, hipMemcpyHostToDevice, c->stream));
        HIPCHK(launch_comp_extent(j, run.rec_dev, c->stream));
        HIPCHK(hipMemcpyAsync(&rec, run.rec_dev, sizeof rec, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipMemcpyAsync(&run.sum, run.sum_dev, sizeof(CompSummary), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    vrt_filter_result out{};
    out.components = run.sum.sel_components; out.voxels = run.sum.sel_voxels;
    if (!measure) {
        const int rc = composed_edit(c, s, rec, clo, csize, j.box, comp_compose, &j, "the bounds", name, &out.edit);
        if (rc != VRT_OK) return rc;
    }
    *result = out;
    return VRT_OK;
}

} // extern "C"
