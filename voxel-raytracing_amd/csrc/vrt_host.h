// vrt_host.h -- what the host files of the C-ABI (vrt_api*.hip) share: contexts, scenes, the buffer type that owns their
// device memory, and the few helpers more than one of the files needs.  Host only; no kernel file includes it.
#pragma once
#include <mutex>
#include <string>
#include <vector>

#include "vrt_internal.h"

namespace vrt {

int fail(int code, const std::string& msg);       // sets vrt_last_error's message (vrt_api.hip); returns code

#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return ::vrt::fail(VRT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// One device allocation and its owner: hipFree when it goes out of scope, is reset or is assigned to.
template <class T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; }
        return *this;
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { reset(); }

    hipError_t alloc(size_t bytes)                // frees what it held first
    {
        reset();
        const hipError_t e = hipMalloc((void**)&p_, bytes);
        if (e != hipSuccess) p_ = nullptr; else bytes_ = bytes;
        return e;
    }
    void reset() { if (p_) hipFree(p_); p_ = nullptr; bytes_ = 0; }
    T* get() const { return p_; }
    size_t bytes() const { return bytes_; }
    explicit operator bool() const { return p_ != nullptr; }

private:
    T* p_ = nullptr;
    size_t bytes_ = 0;
};

// Scratch memory a scene keeps from one call to the next and counts in its `bytes` (`total` below)
struct Scratch {
    DevBuf<uint8_t> buf;
    size_t bytes = 0;
    uint8_t* get() const { return buf.get(); }
    void drop(uint64_t& total) { if (buf) { buf.reset(); total -= bytes; } bytes = 0; }
    hipError_t room(size_t need, uint64_t& total)     // grown to `need` bytes (contents are not kept); a failure leaves it empty
    {
        if (need <= bytes) return hipSuccess;
        drop(total);
        const hipError_t e = buf.alloc(need);
        if (e == hipSuccess) { bytes = need; total += need; }
        return e;
    }
};

const size_t kMaxCells = (size_t)4u << 20;        // above it a scene goes without a cell list
inline size_t round256(size_t n) { return (n + 255u) & ~(size_t)255u; }

} // namespace vrt

// Development switches of a context: A/B experiments and the tests' "the same frame without X" runs.  Each changes speed only,
// never a result; the defaults are the initialisers below (include/vrt.h lists them: not every one is on).  Seeded ONCE, at vrt_ctx_create, from the environment (VRT_TILE_TAGS=0 ...); nothing
// on the render path reads the environment.  vrt_ctx_set_option changes them per context.
struct DevOptions {
    int tile_tags = 1;         // k_tile_tags ahead of K1
    int box_rect = 1;          // the frame's box rectangle
    int xcd_regions = 0;       // launches of >= 8 unsharded frames: one screen region per XCD and frame (off: as a three-dimensional
                               // grid the form runs 30 or 33.6 us per bench frame from one process to the next; rows dealt to the XCDs: 30.0)
    int fast_loop = 1;         // AUTO / DF through the hand-written look-up loop
    int no_bounce_kernel = 1;  // the megakernel without its bounce loop when nothing can bounce
    int packed_bounces = 1;    // the megakernel's bounce chain as one word per hit (no stack of hits in scratch)
    int tags_async = 0;        // the tile tags of a launch on a stream of their own while the context's stream is still busy with the launch before (2: always)
                               // (off: measured SLOWER -- one frame per call, 1 / 2 / 3 contexts in flight: 53.8 / 31.0 / 26.9 us per frame with the
                               // tags on the context's stream, 58.5 / 34.1 / 52.2 us on their own; tools/exp_r4_inflight.py)
    int ao_batch = 1;          // the AO rays of a wave from a pool in LDS that every lane draws on (df_ao_pool_loop, brick_ao_pool)
    int sky_fast = 1;          // sky texel of waves that cannot hit anything by vrt_sky.h
    int sky_span = 1;          // the sky waves of an all-sky 32x8 span store whole rows (vrt_span.h); 0: every wave its own 8x8 block
    int sky_plane = 1;         // the sky waves of primary-only table launches load the miss colour from their view's plane (vrt_miss_plane.h); 0: every wave decides its texel
    int thresh_runs = 1;       // primary rays through df_prim_loop (long runs by threshold)
    int segment_budget = 1;    // segment queries march a wave with min(max_steps, what its 64 segments can need) (vrt_query_seg.hip)
    int hit_table = 1;         // launches without secondary rays take a hit's colour from the table of colorHit() over materials x normals
    int denoise_th16 = 0;      // the tolerance denoiser on 64 x 16 tiles
    int denoise_packed = 1;    // the exact weighted pass two taps at a time in packed fp32
    int denoise_pair = 1;      // verified passes of the canonical taps with an offset of 2 .. 5 through k_denoise_pair (every weight computed once)
    int denoise_p0 = 1;        // verified pass 0 of the canonical taps through k_denoise_p0 (a wave to itself: no LDS, no barrier)
    int denoise_pair_wgs = 0;  // (experiments) workgroups of a k_denoise_pair launch; 0: as many waves as k_denoise_ver's 1024 workgroups
    int denoise_verified = 1;  // weighted passes through k_denoise_ver (vrt_denoise_bound.h); 0: the exact kernels compute every pixel
    int denoise_guard_div8 = 0;// (tests) an eighth of the guard: how much room the bound leaves
    int denoise_count = 0;     // (tests) count the pixels a verified pass evaluates twice (vrt_debug_denoise_redone)
    int open_cells = 1;        // (scene build) open cells / open bricks in the clearance fields
    int df_prefetch = 1;       // (scene build) secondary rays' look-ups prefetch the neighbouring rows
    int df_own = 1;            // (scene build) AO rays spend their own clearance
};

struct vrt_ctx {
    int device = 0;
    DevOptions opt;
    hipStream_t stream = nullptr;
    bool own_stream = true;
    bool timing = true;
    hipEvent_t ev_geo0 = nullptr, ev_prim1 = nullptr, ev_geo1 = nullptr, ev_den0 = nullptr, ev_den1 = nullptr;
    bool have_geo = false, have_den = false;
    vrt::DevBuf<uint4> records;
    vrt::DevBuf<uint32_t> hit_list;   // [records_px] + 1 counter word at the end
    size_t records_px = 0;
    int div_w = 0, div_h = 0, div_ok = 0;   // screen size last examined by screen_div_ok, and its verdict
    uint64_t checked_ptrs[5] = {0, 0, 0, 0, 0};   // digests of the image pointers last verified to be device memory (geometry, denoiser, ray queries, vrt_camera_rays, vrt_render_rays)
    // frame-slot tables of launches with more than VRT_MAX_BATCH frames: a ring of device tables, each with a pinned host
    // image that is uploaded on a stream of its own (the copy runs while the previous launch is still tracing)
    static constexpr int kTabRing = 4;
    vrt::DevBuf<vrt::FrameSlot> tab_dev[kTabRing];
    vrt::FrameSlot* tab_host[kTabRing] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t tab_uploaded[kTabRing] = {nullptr, nullptr, nullptr, nullptr};   // on upload_stream: table i is in device memory
    hipEvent_t tab_consumed[kTabRing] = {nullptr, nullptr, nullptr, nullptr};   // on stream: the launch that read table i is done
    bool tab_busy[kTabRing] = {false, false, false, false};
    int tab_next = 0;
    hipStream_t upload_stream = nullptr;
    // tile tags (k_tile_tags): one word per 8x8-pixel block and frame, valid where == tile_gen.  Two buffers taken in turn: the tags
    // of launch N + 1 are made on a stream of their own while launch N still traces (they depend on the camera alone), and must not
    // land in the buffer launch N reads
    vrt::DevBuf<uint32_t> tile_tags[2];
    size_t tile_tags_words[2] = {0, 0};
    // block verdicts (k_block_verdicts: one byte per block and frame, made from the tags behind them on the same stream): buffer b
    // goes with tag buffer b, is filled and read under the same events.  Like the tags: allocated when a table launch first takes
    // buffer b, grown (behind a synchronise of both streams) when a launch needs more, never shrunk, released with the context
    vrt::DevBuf<uint8_t> verdicts[2];
    size_t verdict_bytes[2] = {0, 0};
    // miss-colour planes (k_miss_plane; vrt_miss_plane.h says when a launch uses one): W x H words per slot, built on `stream` ahead
    // of the launch that first uses them and read by K1 on `stream` only -- a slot is rewritten behind every launch that read it.
    // Each slot allocated when first built, grown when a larger frame takes it, released with the context and by vrt_scene_trim
    vrt::SkyPlaneCache sky_planes;
    vrt::DevBuf<uint32_t> sky_plane_buf[VRT_SKY_PLANES];
    size_t sky_plane_px[VRT_SKY_PLANES] = {0, 0, 0, 0};
    uint64_t sky_planes_built = 0;     // k_miss_plane launches so far (vrt_ctx_get_option)
    uint8_t sky_plane_last[VRT_MAX_TABLE] = {};   // which plane each frame of the latest launch loaded from (0: none; vrt_ctx_get_option)
    uint32_t tile_gen = 0;
    int tag_flip = 0;
    hipStream_t tag_stream = nullptr;
    hipEvent_t tag_done[2] = {nullptr, nullptr};      // on tag_stream: the tags in buffer b are complete
    hipEvent_t tag_read[2] = {nullptr, nullptr};      // on stream: the launch that read buffer b is done
    bool tag_read_valid[2] = {false, false};
    // colorHit() over materials x normals for launches without secondary rays (k_hit_colors), and what it was made from
    vrt::DevBuf<uint32_t> hit_colors;
    uint64_t hit_scene_gen = 0;
    // the verified denoiser pass, diagnostics ("denoise_count"): pixels evaluated twice, one set of counters per pass
    vrt::DevBuf<uint32_t> den_counts;  // [10 passes][VRT_DENOISE_SEGS]
    int den_last_passes = 0;           // passes of the latest vrt_denoise call that went through k_denoise_ver (bit i = pass i)
    vrt_settings hit_settings{};
    // vrt_camera_rays, panorama: the column and row tables (vrt_raygen.h) in device memory, their pinned host image, and the
    // event behind the kernel that last read them
    vrt::DevBuf<float> pano_dev;
    float* pano_host = nullptr;
    size_t pano_floats = 0;
    hipEvent_t pano_done = nullptr;
    bool pano_busy = false;
    // vrt_scene_brush / vrt_scene_stamp: the record the extent kernel returns (vrt_brush_launch.h: BrushRecord), allocated by the first brush
    vrt::DevBuf<uint8_t> brush_rec;
};

struct vrt_scene {
    vrt::DevScene d{};
    vrt::DevBuf<uint8_t> vox;
    vrt::DevBuf<uint64_t> occ1, occ2, occ3;
    // the clearance fields: the allocation, and field 0 (df_guard bytes into it), which is what the kernels are handed
    vrt::DevBuf<uint8_t> df_raw;
    uint8_t* df = nullptr;
    // the clearance fields once more without open cells (launch_open_cells): the march the count planes are rendered with,
    // built when a launch first asks for them
    vrt::DevBuf<uint8_t> df_counts_raw;
    uint8_t* df_counts = nullptr;
    bool metallic_voxels = true;       // some voxel of the scene has a material with metallic > 0 (only then can a ray bounce, frag:283)
    vrt::DevBuf<uint32_t> cells;       // occupied 4^3 cells (k_tile_tags), x | y << 10 | z << 20
    uint32_t n_cells = 0;
    bool cells_ok = false;
    bool open_cells = false;
    size_t df_bytes = 0;
    size_t df_guard = 0;               // bytes of room in front of field 0 and behind the last byte of each set of fields: trace_df_fast counts
                                       // its offsets from (W+2)(H+2) bytes in front of field 0, and its prefetches reach one slice past the border
    std::mutex lazy;
    vrt::DevBuf<vrt_material> palette;
    vrt::DevBuf<float> sky;
    vrt::DevBuf<uint8_t> noise;
    vrt::DevBuf<float> sky_normals;
    vrt::DevBuf<uint32_t> sky8;
    uint32_t occ2_bytes = 0, occ3_bytes = 0;
    // brick scenes
    vrt::DevBuf<uint32_t> bgrid; vrt::DevBuf<uint8_t> bcoarse, bpool, bfine;
    vrt::DevBuf<uint64_t> bentry;      // bgrid + bcoarse folded into one word per brick (what the march reads; the two are freed after the build)
    bool bricks = false;
    uint32_t bcap = 0;                 // bricks bpool / bfine have room for
    // editable brick scenes (vrt_scene_reserve_bricks): bgrid, bcoarse (unfolded: cap 16, bit 7 = open) and the occupancy bytes stay
    // on the device; the host keeps the padded grid once more, the brick of every pool slot and the slots that are free
    bool reserved = false;
    vrt::DevBuf<uint8_t> bocc;         // one byte per brick of the (unpadded) lattice
    uint32_t n_occ = 0;                // occupied bricks
    size_t cells_room = 0;             // entries `cells` has room for (reserved scenes)
    std::vector<uint32_t> hgrid;       // bgrid
    std::vector<uint32_t> slot_pc;     // pool slot -> index in the padded grid, 0xFFFFFFFF = free
    std::vector<uint32_t> free_slots;  // a stack: the lowest slot on top
    std::vector<uint32_t> hcells, cell_slot, cell_pos;   // the cell list, the slot behind each entry, and each slot's entry
    uint64_t bytes = 0;                // device memory held (volume structures + textures)
    // scene edits (vrt_scene_edit_box): which materials are metallic, and the passes' scratch memory (kept from edit to edit, counted
    // in `bytes`, dropped by vrt_scene_trim)
    bool metal[256] = {};
    vrt::Scratch edit_scratch;
    // flood fills (vrt_scene_flood): the two masks, the activity flags, the rounds' counters and the record (vrt_flood_launch.h), kept
    // from flood to flood, counted in `bytes`, dropped by vrt_scene_trim; and how many rounds the latest flood ran
    vrt::Scratch flood_scratch;
    uint32_t flood_rounds = 0;
    // mesh voxelization (vrt_scene_voxelize): the coverage and toggle masks and the record (vrt_voxelize_launch.h), kept, counted and
    // dropped as the flood's; rows per work item (0: VRT_VOXELIZE_ITEM_ROWS) and how many items the latest call launched
    vrt::Scratch voxelize_scratch;
    uint32_t voxelize_item_rows = 0, voxelize_items = 0;
    // morphology (vrt_scene_morph): the two masks over the domain and the record (vrt_morph_launch.h), kept, counted and dropped as
    // the flood's
    vrt::Scratch morph_scratch;
    // connected components (vrt_scene_components, vrt_scene_filter_components): the label volume, the segments' counts, the summary
    // and the filter's record in one allocation, the table in another (its size follows from the component count), kept, counted
    // and dropped as the flood's.  edit_gen counts the rewrites of the scene (scene_edit_locked); the latest labelling is valid
    // for vrt_scene_component_labels while comp_valid and comp_gen == edit_gen, over the clipped bounds comp_clo, comp_csize
    vrt::Scratch comp_scratch, comp_table;
    uint64_t edit_gen = 0, comp_gen = 0;
    bool comp_valid = false;
    int32_t comp_clo[3] = {0, 0, 0};
    uint32_t comp_csize[3] = {0, 0, 0};
    // the six together: what brick_scene_bytes counts and vrt_scene_trim drops
    size_t scratch_bytes() const
    {
        return edit_scratch.bytes + flood_scratch.bytes + voxelize_scratch.bytes + morph_scratch.bytes + comp_scratch.bytes + comp_table.bytes;
    }
    void drop_scratch()
    {
        edit_scratch.drop(bytes); flood_scratch.drop(bytes); voxelize_scratch.drop(bytes); morph_scratch.drop(bytes);
        comp_scratch.drop(bytes); comp_table.drop(bytes); comp_valid = false;
    }
    uint64_t shade_gen = 0;           // changes whenever something a hit's colour depends on does (creation, vrt_scene_set_sky)
};

namespace vrt {

// vrt_api.hip
int make_shard(const vrt_shard* sh, int H, ShardMap& m, int* max_local_strips);
int check_device_ptrs(vrt_ctx* c, int slot, const void* const* ptrs, int n, const char* what);

// vrt_api_scene.hip: the fields a launch that writes count planes marches through, built on first use
int fields_for_counts(vrt_ctx* c, const vrt_scene* s, const uint8_t** out);
// vrt_api_scene.hip, for the edits too (vrt_api_edit.hip): a dense scene's clearance fields built into dst from the voxels on the
// device (open: with the open cells coded 0), its cell list made again, the count planes' fields dropped (the next launch that
// asks builds them again), and a brick's entry in the cell list from its index pc in the padded grid.  Hidden: they were one
// file's statics, and the library's dynamic symbols stay what they were
#define VRT_HIDDEN __attribute__((visibility("hidden")))
VRT_HIDDEN hipError_t build_fields(vrt_ctx* c, const vrt_scene* s, uint8_t* dst, bool open);
VRT_HIDDEN hipError_t build_cell_list(vrt_ctx* c, vrt_scene* s);
VRT_HIDDEN void drop_count_fields(vrt_scene* s);
VRT_HIDDEN uint32_t brick_cell_code(uint32_t pc, int pbx, int pby);

// vrt_api_scene.hip: what the read-back calls make of a box before any device work (vrt_scene_read.h: read_box_check; the message
// names `name`; *count: the box's voxels), and the checked box as the kernels take it.  ReadBox is vrt_scene_read.h's, for the
// files that define VRT_SCENE_READ_LAUNCHERS.
int read_box_checked(const vrt_scene* s, const int32_t lo[3], const uint32_t size[3], uint32_t max_side, const std::string& name, size_t* count);
struct ReadBox;
ReadBox read_box_of(const vrt_scene* s, const int32_t lo[3], const uint32_t size[3]);

// May the kernels divide by W and H with a multiplication (screen_div_exact)?  The context remembers the last size examined.
inline int screen_div_ok(vrt_ctx* c, int W, int H)
{
    if (c->div_w != W || c->div_h != H) { c->div_ok = (screen_div_exact(W) && screen_div_exact(H)) ? 1 : 0; c->div_w = W; c->div_h = H; }
    return c->div_ok;
}

} // namespace vrt
