/*
 * vrt.h -- C-ABI of the MI355X-native voxel ray tracer (libvrt_hip.so).
 *
 * The reference (ectucker1/voxel-raytracing) has no FFI layer; the boundary this library replaces is
 * the C++ object surface of source/voxels + source/engine.  Each entry point cites the reference
 * interface it stands in for (paths relative to the reference root).  Plain pointers and sizes only;
 * no exceptions cross the ABI: every call returns VRT_OK or an error code and vrt_last_error()
 * returns the thread-local message (the reference throws std::runtime_error, app.cpp:21-25).
 *
 * Threading: one vrt_ctx per host thread / per GPU; calls on one context are serialised on its HIP
 * stream (the reference is strictly single-threaded, engine.cpp:28-46).  Frames in flight
 * (MAX_FRAMES_IN_FLIGHT, engine.hpp:19): one context per frame slot; contexts of one device run
 * concurrently and may share a vrt_scene, which is read-only while rendering (vrt_scene_edit_box changes it between launches).  All image pointers in
 * vrt_frame are DEVICE pointers owned by the caller (or allocated with vrt_device_alloc).
 * There is no CPU fallback: without a HIP device every compute call fails with VRT_ERR_NO_DEVICE.
 */
#ifndef VRT_H
#define VRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VRT_OK               0
#define VRT_ERR_INVALID      1   /* bad argument */
#define VRT_ERR_IO           2   /* "Failed to read voxel scene"            voxel_scene.cpp:42 */
#define VRT_ERR_PARSE        3   /* "Could not parse voxel scene"           voxel_scene.cpp:46 */
#define VRT_ERR_NO_INSTANCE  4   /* "Voxel scene does not contain an instance." voxel_scene.cpp:50 */
#define VRT_ERR_NO_DEVICE    5   /* no HIP device / HIP runtime error at context creation */
#define VRT_ERR_HIP          6   /* HIP runtime error (message has the HIP error string) */
#define VRT_ERR_UNSUPPORTED  7

#define VRT_MAX_BOUNCES 8

typedef struct vrt_ctx   vrt_ctx;    /* device + stream + workspace  (stands in for Engine, engine.hpp:71-76) */
typedef struct vrt_scene vrt_scene;  /* device-resident scene        (VoxelScene, voxel_scene.hpp:18-34)      */

/* Material, source/voxels/resource/material.hpp:5-12 (32 B, std140 compatible). */
typedef struct vrt_material {
    float diffuse[4];
    float metallic;
    float pad[3];
} vrt_material;

/* ScreenQuadPush, source/voxels/resource/screen_quad_push.hpp:5-15; filled at voxel_renderer.cpp:72-83.
 * 96 bytes, identical member offsets (camPos@0 camDir@16 camRight@32 camUp@48 volumeBounds@64 frame@76
 * screenSize@80 cameraJitter@88). */
typedef struct vrt_push {
    float    cam_pos[4];
    float    cam_dir[4];
    float    cam_right[4];
    float    cam_up[4];
    uint32_t volume_bounds[3];
    uint32_t frame;
    int32_t  screen_size[2];
    float    camera_jitter[2];
} vrt_push;

/* Traversal strategies.  All of them produce bit-identical hit records and G-buffers (the DDA state is
 * advanced with the same fp32 additions as voxel_volume.frag:164-170); they differ only in how much memory
 * work is skipped.  steps_* planes are exact for DENSE / BITMASK / DF and upper bounds for JUMP / DFJ. */
#define VRT_TRAVERSAL_AUTO    0   /* fastest available (currently DF) */
#define VRT_TRAVERSAL_DENSE   1   /* one R8 fetch per DDA iteration (voxel_volume.frag:157), fetched 4 iterations ahead */
#define VRT_TRAVERSAL_BITMASK 2   /* solid test on 4^3 occupancy words (L2) + 16^3 / 64^3 summaries staged in LDS */
#define VRT_TRAVERSAL_JUMP    3   /* BITMASK + exact closed-form jumps across empty pyramid cells */
#define VRT_TRAVERSAL_DF      4   /* octant clearance, its minimum over the wave agreed by a DPP reduction; ALU-only runs between look-ups */
#define VRT_TRAVERSAL_DFJ     5   /* DF with the long runs (clearance >= 12) done per lane in closed form (JUMP's integer form) */
/* (6, 7: internal -- the brick-scene march and the hand-written DF loop; both are what AUTO resolves to where they apply) */

#define VRT_FLAG_SPLIT_KERNELS 4u /* trace secondary rays in a second kernel (K2) over the compacted hit list instead of inside K1 */
#define VRT_FLAG_DEBUG_PLANES 1u  /* steps_total / rays_total receive traversal diagnostics instead (development aid) */
#define VRT_FLAG_MARCHED_COUNTS 16u /* the count planes (steps_primary, steps_total, rays_total) report the PRODUCT march's own work -- rays
                                     * end at open cells, untagged blocks are not traced, an any-hit ray decided at a look-up reports the
                                     * iterations it took -- instead of the reference loop's iterations; every other plane is unchanged.
                                     * bench.py's roofline figures count these.  The launch runs the counting twins of the look-up loops: the same
                                     * march as the product launch (threshold runs included: a threshold run reports the steps its axes took,
                                     * which is the iteration count unless two axes tie) */
#define VRT_FLAG_LOOKUP_COUNTS 32u  /* with VRT_FLAG_MARCHED_COUNTS: the count planes hold the BYTES the march asked for instead of its iterations --
                                     * one per clearance look-up of a live lane (three where the look-ups prefetch), one per voxel id read; brick
                                     * scenes: 8 per brick word, 1 per fine byte and id.  What bench.py reports as roofline.requested_bytes */

/* VolumeParameters (parameters.hpp:5-9) + Light (voxel_scene.hpp:10-15) as GeometryStage::record fills
 * them each frame (geometry_stage.cpp:135-145), plus the shader's compile-time constants
 * (voxel_volume.frag:68-69,219) promoted to runtime fields. */
typedef struct vrt_settings {
    uint32_t ao_samples;        /* occlusionSettings.numSamples, default 4   */
    float    ambient_intensity; /* occlusionSettings.intensity,  default 1   */
    float    light_dir[3];      /* lightSettings.direction, default normalize(1,1,1) */
    float    light_intensity;   /* default 1 */
    float    light_color[4];    /* default (1,1,1,1) */
    uint32_t max_steps;         /* MAX_RAY_STEPS   = 512 */
    uint32_t ao_steps;          /* AO ray step cap = 64  */
    uint32_t max_bounces;       /* MAX_REFLECTIONS = 5 (<= VRT_MAX_BOUNCES) */
    uint32_t shadows;           /* 1 = reference behaviour; 0 = "primary rays only" (no shadow ray) */
    uint32_t traversal;         /* VRT_TRAVERSAL_* */
    uint32_t flags;
} vrt_settings;

/* GeometryBuffer, source/voxels/stages/geometry_stage.hpp:19-27, target formats geometry_stage.cpp:22-33.
 * Row-major, origin top-left.  Any plane may be NULL (not written).  All DEVICE pointers.
 * In sharded mode (vrt_shard.nranks > 1) the planes are still full-frame W*H; a rank writes only
 * the rows it owns. */
typedef struct vrt_frame {
    uint8_t*  color8;        /* RGBA8_UNORM, alpha = 0                     */
    float*    depth;         /* R32F                                        */
    float*    motion;        /* RG32F (always 0, voxel_volume.frag:333; vrt_reproject fills it) */
    uint8_t*  mask8;         /* R8_UNORM: 0.9 on hit / 0                    */
    float*    position;      /* RGBA32F, w = 0                              */
    int8_t*   normal8;       /* RGBA8_SNORM, w = 0                          */
    /* debug / parity planes (no reference analogue) */
    float*    color_f;       /* 3 floats / px before UNORM8 quantisation    */
    uint8_t*  hit_id;        /* primary-ray material id, 0 = miss           */
    int16_t*  hit_voxel;     /* 3 / px: grid cell of the hit                */
    uint8_t*  hit_mask;      /* bit0..2 = final DDA mask x,y,z              */
    /* The two count planes report the iterations of the REFERENCE's loop (every ray walks to a hit, the wall or the end of its
     * budget).  The product march takes fewer -- rays end where nothing solid is left in their octant, blocks of pixels no
     * occupied cell projects onto are not traced -- so a launch with a count plane marches a second set of clearance fields
     * without those shortcuts (built on first use, as large as the first) and uses no tile tags: diagnostics, not for
     * production launches.  Every other plane is the same either way. */
    uint32_t* steps_primary; /* DDA iterations that sampled a voxel (frag:157), primary ray  */
    uint32_t* steps_total;   /* ... all rays of the pixel                   */
    uint32_t* rays_total;    /* rays traced for the pixel                   */
    /* multi-GPU (no reference analogue): the colour once more, in the layout vrt_pack_rows produces -- the rows this rank
     * owns, packed in increasing row order, vrt_shard_rows() rows in all (padding rows are not written).  Lets the
     * tracing kernel fill the send buffer of the collective itself instead of a copy kernel after it. */
    uint8_t*  color8_strips;
} vrt_frame;

/* Screen-tile sharding (no reference analogue; BASELINE north_star).  The frame is cut into
 * horizontal strips of strip_rows rows (multiple of 16); strip s belongs to rank s % nranks.
 * nranks = 1 (or a NULL vrt_shard*) renders everything. */
typedef struct vrt_shard {
    int32_t rank;
    int32_t nranks;
    int32_t strip_rows;
} vrt_shard;

/* ---- context --------------------------------------------------------------------------------- */
/* Engine::init (engine.cpp:14): selects HIP device `device`, creates the context stream. */
int  vrt_ctx_create(int device, vrt_ctx** out);
void vrt_ctx_destroy(vrt_ctx* ctx);                         /* Engine::destroy */
/* Adopt an externally owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) in place of the
 * context's own stream.  NULL is a valid handle: the HIP null (legacy default) stream, which is what
 * torch's default stream is. */
int  vrt_ctx_set_stream(vrt_ctx* ctx, void* hip_stream);
int  vrt_ctx_synchronize(vrt_ctx* ctx);                     /* device.waitIdle(), engine.cpp:351 */
/* Development switches of a context (no reference analogue; the reference's counterpart is recompiling a shader): each changes
 * speed only, never a result -- the tests render "the same frame without X" with them.  Name (default), who looks at it:
 *   every vrt_render_geometry* call:  "tile_tags" (1), "box_rect" (1), "fast_loop" (1), "thresh_runs" (1), "hit_table" (1), "sky_fast" (1),
 *                                     "sky_span" (1: the sky waves of an all-sky 32x8 span store whole rows; needs sky_fast),
 *                                     "sky_plane" (1: in primary-only launches of more than 8 frames the sky waves of frames that share a view
 *                                     -- ray-generation constants, screen size and sky equal bit for bit -- load the miss colour from a plane
 *                                     computed once per view, csrc/vrt_miss_plane.h; needs sky_fast; 0: every sky wave decides its texel),
 *                                     (read-only through vrt_ctx_get_option, for the tests: "sky_planes_built", "sky_planes_held",
 *                                     "sky_plane_min_group" and "sky_plane_of_<f>" -- the plane frame f of the latest launch loaded from, 0: none),
 *                                     "no_bounce_kernel" (1), "ao_batch" (1: the AO rays of a wave from a pool in LDS every lane draws on),
 *                                     "packed_bounces" (1: the bounce chain as one word per hit on dense scenes; 2: on brick scenes too,
 *                                     where it measured slower; 0: the stack of hits), "tags_async" (0: the tile tags of a launch on a
 *                                     stream of their own measured slower; 1: on that stream while the context's stream is busy with
 *                                     the launch before, which the library asks the runtime at every launch; 2: on that stream always,
 *                                     busy or not -- the value the tests use, because it does not depend on timing),
 *                                     "xcd_regions" (0 -- until round 3 VRT_XCD_REGIONS was on by default; as a three-dimensional grid the
 *                                     form ran 30.0 or 33.6 us per bench frame from one process to the next, so it is opt-in now)
 *   vrt_denoise:                      "denoise_packed" (1), "denoise_verified" (1), "denoise_pair" (1: verified passes of the canonical taps
 *                                     with offsets 2 .. 5 compute every weight once, k_denoise_pair; 0: k_denoise_ver), "denoise_p0" (1: pass 0 through k_denoise_p0), "denoise_pair_wgs" (0; experiments: workgroups of a
 *                                     k_denoise_pair launch), "denoise_th16" (0: the tolerance kernel's 64 x 16 tiles
 *                                     are an experiment), and the tests' handles on the verified pass "denoise_guard_div8" (0), "denoise_count" (0)
 *   vrt_trace_rays / vrt_occluded_rays / vrt_pick_pixels:  "thresh_runs" (1) and nothing else
 *   vrt_trace_segments / vrt_occluded_segments:  "thresh_runs" (1), "segment_budget" (1: a wave of 64 segments is marched with
 *                                     min(max_steps, the iterations its longest segment can need); 0: with max_steps) and nothing else
 *   vrt_render_rays:                  "thresh_runs" (1), "ao_batch" (1) and nothing else
 *   scene creation:                   "open_cells" (1), "df_prefetch" (1), "df_own" (1)
 * The environment seeds them ONCE, at vrt_ctx_create (VRT_TILE_TAGS=0, VRT_SKY_FAST=0, ...); nothing on the render path calls
 * getenv.  Values are non-negative integers (the switches: 0 / 1; a negative value is stored as 0).  Unknown name: VRT_ERR_INVALID. */
int  vrt_ctx_set_option(vrt_ctx* ctx, const char* name, int32_t value);
int  vrt_ctx_get_option(vrt_ctx* ctx, const char* name, int32_t* value);
const char* vrt_last_error(void);
/* Name of the device, compute units, and whether the library was built for its gfx arch. */
int  vrt_device_info(vrt_ctx* ctx, char* name, size_t name_len, int* compute_units);

/* Device memory helpers so that C/C++ callers need no HIP headers (Buffer, engine/resource/buffer.hpp). */
int  vrt_device_alloc(vrt_ctx* ctx, size_t bytes, void** out);
int  vrt_device_free(vrt_ctx* ctx, void* p);
int  vrt_memcpy_h2d(vrt_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int  vrt_memcpy_d2h(vrt_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int  vrt_memset(vrt_ctx* ctx, void* dst_dev, int value, size_t bytes);

/* ---- scene ----------------------------------------------------------------------------------- */
/* VoxelScene::VoxelScene(engine, filename, skybox) (voxel_scene.cpp:33-133): read the file, parse the
 * MagicaVoxel chunks (own reader, validated against ogt_vox.h:1179-1991), flatten all instances of
 * frame 0 into one dense R8 volume with the Y/Z swap (voxel_scene.cpp:53-105), build the palette
 * (pow 2.2 + MATL metal, :108-117), upload, and build the occupancy pyramid. */
int  vrt_scene_load_vox_file(vrt_ctx* ctx, const char* path, vrt_scene** out);
/* ogt_vox_read_scene(buffer,size) + the same flatten. */
int  vrt_scene_load_vox_mem(vrt_ctx* ctx, const void* buf, size_t n, vrt_scene** out);
/* Synthetic scenes: dense R8 volume, index x + y*W + z*W*H (Texture3D upload order, voxel_scene.cpp:99,122). */
int  vrt_scene_from_dense(vrt_ctx* ctx, const uint8_t* voxels, uint32_t W, uint32_t H, uint32_t D,
                          const vrt_material palette[256], vrt_scene** out);
/* The same volume handed over SPARSELY, in 8^3 bricks (no reference analogue: the reference's Texture3D is dense,
 * voxel_scene.cpp:77-78,122; BASELINE configs[4] is a 2048^3 volume -- 8 GiB dense, 9x that with the dense scene's clearance
 * fields).  grid[bx + by*nbx + bz*nbx*nby] = 0 for an empty brick, else 1 + its index in `pool`; pool holds n_bricks x 512
 * voxel ids, voxel (x,y,z) of a brick at x + 8y + 64z.  The scene is the W x H x D = 8nbx x 8nby x 8nbz volume those bricks
 * spell out, and renders bit for bit like vrt_scene_from_dense of the same content; device memory is per OCCUPIED brick
 * (4.5 KiB: ids + per-voxel clearance) plus 12 bytes per brick of the grid.  Only VRT_TRAVERSAL_AUTO applies to it. */
int  vrt_scene_from_bricks(vrt_ctx* ctx, const uint32_t* grid, uint32_t nbx, uint32_t nby, uint32_t nbz,
                           const uint8_t* pool, uint32_t n_bricks, const vrt_material palette[256], vrt_scene** out);
/* Drops what a scene holds only for diagnostics: the second set of clearance fields (without open cells) that the first launch
 * with a count plane (steps_primary / steps_total) builds -- as large as the first, 9 x the padded voxel bytes.  A later launch
 * with count planes builds it again.  Callers that never attach count planes never hold it.  Waits for the context's stream. */
int  vrt_scene_trim(vrt_ctx* ctx, vrt_scene* scene);
/* Scene edits (no reference analogue: the reference uploads its Texture3D once, voxel_scene.cpp:122).  Rewrite the voxels of the
 * box [lo, lo+size) of a dense scene and bring every structure the march reads up to date -- volume, clearance fields with
 * their open cells, occupancy pyramid, the list of occupied cells -- byte for byte as vrt_scene_from_dense of the edited volume
 * would build them, recomputing only what the box can have changed (csrc/vrt_edit.h; an edit whose recomputed cells, summed over
 * the eight octants, reach half of a full build's, or with a side above 512, rebuilds the fields in full instead).
 * ids: HOST pointer, size[0]*size[1]*size[2] voxel ids, x fastest (x + y*size[0] + z*size[0]*size[1]); id 0 = empty.
 * After the call returns, every later launch on any context renders exactly as it would on a scene newly built from the edited
 * volume.  The edit works on the context's stream and, like vrt_scene_set_sky, waits for it: launches enqueued on this context
 * before the call see the old volume, later ones the new.  The caller makes sure no OTHER context is still rendering the scene.
 * A box that is empty (a zero size) or leaves the volume, or a NULL argument: VRT_ERR_INVALID.  A brick scene that
 * vrt_scene_reserve_bricks has not made editable: VRT_ERR_UNSUPPORTED.  Writing an id whose material has metallic > 0 makes the scene one whose rays can bounce, and it stays
 * one when the last such voxel is carved away again (that selects a kernel, never a result).  The count planes' second set of
 * fields is dropped (the next launch with a count plane builds it again).  The passes keep their scratch memory from edit to
 * edit; vrt_scene_memory counts it and vrt_scene_trim drops it. */
int  vrt_scene_edit_box(vrt_ctx* ctx, vrt_scene* scene, const int32_t lo[3], const uint32_t size[3], const uint8_t* ids);
/* The same with one id for the whole box (0 carves, non-zero fills). */
int  vrt_scene_fill_box(vrt_ctx* ctx, vrt_scene* scene, const int32_t lo[3], const uint32_t size[3], uint8_t id);
/* Makes a brick scene editable: room for capacity_bricks bricks in its pool, and the structures an edit updates kept on the
 * device (padded pointer grid, brick occupancy, the eight coarse fields before they are folded into the entries: 5 bytes per
 * brick of the padded grid more, and 4.5 KiB per reserved brick).  capacity_bricks below the number of occupied bricks, or above
 * 2^24 - 3: VRT_ERR_INVALID; a dense scene: VRT_ERR_UNSUPPORTED.  Calling it again with a larger capacity grows the
 * reservation; one that is not larger changes nothing.  What the scene renders is unchanged, bit for bit.  Waits for the
 * context's stream, like an edit.  vrt_scene_memory counts the reservation and vrt_scene_trim keeps it.
 * vrt_scene_edit_box / vrt_scene_fill_box then work on the scene under the dense scene's contract, and leave every structure
 * the march reads as vrt_scene_from_bricks of the edited volume would build it (up to which pool slot a brick lies in): a brick
 * whose 512 voxels all become 0 becomes an empty brick and its slot is free again, an empty brick that receives a non-zero id
 * takes a free slot.  Only the bricks the box meets and their neighbours are recomputed, and the brick-level fields only if
 * some brick's occupancy changed (csrc/vrt_brick_edit.h).  An edit that needs more slots than are free changes nothing and
 * returns VRT_ERR_UNSUPPORTED; reserve more and repeat it. */
int  vrt_scene_reserve_bricks(vrt_ctx* ctx, vrt_scene* scene, uint32_t capacity_bricks);
/* Diagnostics (tests): copy one of a scene's device structures to the host, as it lies in memory.  host == NULL only
 * reports *bytes; a capacity below that is VRT_ERR_INVALID.  VRT_STATE_DF is the whole allocation of the clearance fields: eight
 * zero-bordered fields, and where the layout has them the ninth with the voxel ids and the 0xFF byte behind it; VRT_STATE_OCC2 and _OCC3 include the zero word that pads an odd count of
 * words to an even one.  Selectors 0 - 4
 * are a dense scene's, 6 - 8 a brick scene's (the other kind: VRT_ERR_UNSUPPORTED), the cell list either's.  Waits for the
 * context's stream. */
#define VRT_STATE_VOX   0
#define VRT_STATE_DF    1
#define VRT_STATE_OCC1  2
#define VRT_STATE_OCC2  3
#define VRT_STATE_OCC3  4
#define VRT_STATE_CELLS 5   /* the occupied 4^3 cells (brick scenes: the occupied bricks), x | y << 10 | z << 20, in no particular order */
#define VRT_STATE_BENTRY 6  /* one packed 8-byte word per brick of the padded grid ((nbx+2)(nby+2)(nbz+2); VolumeView::bentry) */
#define VRT_STATE_BPOOL  7  /* the voxel ids, 512 bytes per pool slot, for every slot the pool has room for; a slot no entry points to holds anything */
#define VRT_STATE_BFINE  8  /* the per-voxel clearances, 8 x 512 bytes per pool slot, likewise */
int  vrt_debug_scene_state(vrt_ctx* ctx, const vrt_scene* scene, int what, void* host, size_t capacity, size_t* bytes);
/* Device bytes a scene holds (volume, clearance, pyramid / brick structures, palette, sky, noise). */
int  vrt_scene_memory(const vrt_scene* sc, uint64_t* bytes);
/* Host-only half of the loader (no device needed): parse + flatten into malloc'd host memory.
 * *voxels must be released with vrt_host_free.  Used by tests and by the C++ host mirror. */
int  vrt_vox_flatten_host(const void* buf, size_t n, uint32_t dims[3], uint8_t** voxels,
                          vrt_material palette[256], uint32_t* num_instances, uint64_t* dropped);
void vrt_host_free(void* p);
/* Texture2D(skybox .hdr, RGBA32F) (voxel_scene.cpp:132; nearest/repeat sampler texture_2d.cpp:158-163):
 * raw float RGBA texels, row-major.  Default when never called: 1x1 white. */
int  vrt_scene_set_sky(vrt_ctx* ctx, vrt_scene* sc, const float* rgba, uint32_t w, uint32_t h);
/* Texture2D(blue_noise_rgba.png, RGBA8_UNORM) (voxel_renderer.cpp:22).  Default: 1x1 mid-grey. */
int  vrt_scene_set_blue_noise(vrt_ctx* ctx, vrt_scene* sc, const uint8_t* rgba8, uint32_t w, uint32_t h);
/* Texture2D(engine, filepath, 4, format) (source/engine/resource/texture_2d.cpp:22-44): decode the file on the host
 * (Radiance .hdr -> linear float RGBA like stbi_loadf, PNG -> RGBA8 like stbi_load) and upload it.  An 8-bit image given
 * as sky is converted c/255; a float image given as noise is rejected.  Failure: "Could not load image <path>". */
int  vrt_scene_set_sky_file(vrt_ctx* ctx, vrt_scene* sc, const char* path);
int  vrt_scene_set_blue_noise_file(vrt_ctx* ctx, vrt_scene* sc, const char* path);
/* The decoders alone (host only).  *pixels: float RGBA (is_hdr = 1) or RGBA8 (is_hdr = 0), release with vrt_host_free. */
int  vrt_image_load(const char* path, int* is_hdr, uint32_t* w, uint32_t* h, void** pixels);
/* Writers for rendered frames (host memory): 8-bit PNG / binary PPM from RGBA8, PFM from float RGB(A) with the given
 * stride in floats (3 for color_f, 4 for position). */
int  vrt_image_write_png(const char* path, const uint8_t* rgba8, uint32_t w, uint32_t h);
int  vrt_image_write_ppm(const char* path, const uint8_t* rgba8, uint32_t w, uint32_t h);
int  vrt_image_write_pfm(const char* path, const float* pixels, uint32_t w, uint32_t h, uint32_t stride_floats);
/* VoxelScene::width/height/depth (voxel_scene.hpp:21). */
int  vrt_scene_info(const vrt_scene* sc, uint32_t dims[3]);
/* Copy the dense volume / palette back to the host (tests, oracle comparison). */
int  vrt_scene_download(vrt_ctx* ctx, const vrt_scene* sc, uint8_t* voxels, vrt_material palette[256]);
/* Scene read-back (no reference analogue: the reference has no editor and never writes a scene).  The definitions -- box index,
 * record, order, tiles -- are csrc/vrt_scene_read.h's; the file's are csrc/vox_writer.cpp's.  These work on dense scenes of every
 * field layout and on brick scenes, reserved or not; they run on the context's stream and wait for it, like
 * vrt_scene_download: a read enqueued after an edit sees the edit.  (Their context parameter is spelled `struct vrt_ctx*`, as
 * vrt_trace_segments': the same type.)
 * vrt_scene_read_box: the inverse of vrt_scene_edit_box.  ids: HOST pointer to size[0]*size[1]*size[2] bytes, x fastest, which
 * receive the voxel ids of the box [lo, lo+size); an empty brick reads as zeros.  An empty box, a box that leaves the volume, a
 * size whose byte count overflows size_t or a NULL argument: VRT_ERR_INVALID before any device work; a box for which no staging
 * buffer can be allocated on the device: VRT_ERR_UNSUPPORTED (read it in parts). */
int  vrt_scene_read_box(struct vrt_ctx* ctx, const vrt_scene* scene, const int32_t lo[3], const uint32_t size[3], uint8_t* ids);
/* The non-empty voxels (id != 0) of a box whose sides are each at most 256, compacted on the device: one uint32 per voxel,
 * (x-lo[0]) | (y-lo[1]) << 8 | (z-lo[2]) << 16 | id << 24, in ascending order of x + y*size[0] + z*size[0]*size[1] (relative
 * coordinates) -- the order is part of the contract: the output is a function of the scene's content alone.  records: HOST
 * pointer to `capacity` entries.  *count always receives the number of non-empty voxels; records == NULL (capacity ignored) only
 * counts; capacity < *count writes nothing to records and returns VRT_ERR_INVALID with *count set.  The errors of
 * vrt_scene_read_box, and a side above 256: VRT_ERR_INVALID.  Of a brick scene an empty brick costs one read of its grid word,
 * and a box over empty bricks only launches nothing beyond those reads. */
int  vrt_scene_list_box(struct vrt_ctx* ctx, const vrt_scene* scene, const int32_t lo[3], const uint32_t size[3],
                        uint32_t* records, uint64_t capacity, uint64_t* count);
/* A dense volume (x + y*W + z*W*H, dims = W, H, D, each 1..4096) and a palette as a MagicaVoxel .vox file in malloc'd host
 * memory (release with vrt_host_free); host only, the counterpart of vrt_vox_flatten_host.  The scene is written in tiles of at
 * most 256 voxels per axis, one model each (csrc/vox_writer.cpp has the layout).  A scene whose palette came from bytes -- every
 * loaded .vox -- reads back exactly (dims, voxels, every palette float, every metallic value) through this library's loader and
 * the reference's; ANY OTHER PALETTE IS QUANTISED: a colour channel becomes the byte whose pow(c/255, 2.2) is nearest (ties to
 * the lower byte), and id 0's alpha reads back as 0.  A file beyond the 2^32 - 1 bytes a MAIN chunk can state:
 * VRT_ERR_UNSUPPORTED. */
int  vrt_vox_encode_host(const uint8_t* voxels, const uint32_t dims[3], const vrt_material palette[256], void** buf, size_t* n);
/* The same file, byte for byte, of a scene on the device -- dense or bricks -- without ever holding its dense volume: per tile
 * one vrt_scene_list_box, then the same serialiser (peak host memory: one tile's records plus the file).  _mem: *buf is
 * released with vrt_host_free.  _file: writes to path; a file that cannot be written: VRT_ERR_IO. */
int  vrt_scene_save_vox_mem (struct vrt_ctx* ctx, const vrt_scene* scene, void** buf, size_t* n);
int  vrt_scene_save_vox_file(struct vrt_ctx* ctx, const vrt_scene* scene, const char* path);
/* Surface extraction (no reference analogue): the read-side twin of vrt_scene_voxelize.  csrc/vrt_faces.h is the definition,
 * in plain integers.  Directions d: 0 = -x, 1 = +x, 2 = -y, 3 = +y, 4 = -z, 5 = +z.  Face d of a voxel of the box [lo, lo+size)
 * with id != 0 is EXPOSED iff the voxel across it is empty; a neighbour outside the volume is empty, a neighbour outside the box
 * but inside the volume is read from the scene (a scene extracted in parts gives exactly the faces of the scene extracted whole),
 * unless VRT_FACES_CLOSED is set: then every voxel outside the box counts as empty and the box's faces are a closed surface.
 * Without VRT_FACES_RUNS every exposed face is a record of length 1; with it, exposed faces of the same d and id that follow
 * each other along the run axis (y for d = 0, 1; x otherwise) merge into a run, which also ends where the box-relative
 * coordinate along that axis reaches a multiple of 64 (length 1 .. 64).  A record is one uint64: the vrt_scene_list_box word of
 * the run's lowest voxel in bits 0 .. 31, length - 1 in bits 32 .. 37, d in bits 40 .. 42, every other bit 0.  Order: ascending d,
 * within a d ascending key of the first voxel, the run axis fastest (d >= 2: x + y*size[0] + z*size[0]*size[1]; d < 2:
 * y + (x + z*size[0])*size[1], relative coordinates) -- part of the contract, as vrt_scene_list_box's.
 * records: HOST pointer to `capacity` entries.  counts[d] always receives the number of records of direction d; records == NULL
 * (capacity ignored) only counts; a capacity below their sum writes nothing to records and returns VRT_ERR_INVALID with the
 * counts set.  The errors of vrt_scene_list_box, or an unknown flag: VRT_ERR_INVALID before any device work; scan words or a
 * staging buffer that cannot be allocated on the device (a 256^3 checkerboard has 50 M records): VRT_ERR_UNSUPPORTED, list the
 * box in parts.  Dense scenes of every field layout and brick scenes, reserved or not; runs on the context's stream and waits
 * for it, so a call enqueued after an edit sees the edit. */
#define VRT_FACES_RUNS   1u
#define VRT_FACES_CLOSED 2u
int  vrt_scene_list_faces(struct vrt_ctx* ctx, const vrt_scene* scene, const int32_t lo[3], const uint32_t size[3], uint32_t flags,
                          uint64_t* records, uint64_t capacity, uint64_t counts[6]);
/* n records of a box at lo as quads (host only; no device needed).  The quad of a record lies in the plane axis(d) = coordinate
 * (+ 1 for odd d), is `length` long along the run axis and 1 along the third; its corners start at the one with the lowest
 * coordinates and run counter-clockwise seen from the empty side.  *vertices: int32 [*nv][3] in SIXTEENTHS OF A VOXEL, the unit
 * vrt_scene_voxelize takes, volume coordinates, welded in order of first appearance; *quads: uint32 [n][4] indices into them;
 * *ids: uint8 [n].  Release the three with vrt_host_free.  A word that is no record, or a NULL argument: VRT_ERR_INVALID. */
int  vrt_faces_mesh_host(const uint64_t* records, uint64_t n, const int32_t lo[3], int32_t** vertices, uint64_t* nv,
                         uint32_t** quads, uint8_t** ids);
/* The same quads as a Wavefront OBJ and its material library, both in malloc'd host memory (vrt_host_free; host only).  The OBJ:
 * `mtllib <mtl_name>`, the vertices as `v x y z` in integer VOXEL coordinates, then the quads as `f a b c d` under
 * `usemtl id_<N>`, ascending N, within an N in the records' order.  The library: `newmtl id_<N>` and `Kd r g b` (the palette's
 * diffuse colour, each float printed %.9g) for every id used, ascending. */
int  vrt_faces_obj_host(const uint64_t* records, uint64_t n, const int32_t lo[3], const vrt_material palette[256],
                        const char* mtl_name, void** obj, size_t* nobj, void** mtl, size_t* nmtl);
/* A scene's whole surface as such an OBJ -- dense or bricks -- without ever holding its dense volume: the scene is cut into the
 * tiles of vrt_scene_save_vox_*, x fastest, then y, then z; per tile one vrt_scene_list_faces with `flags`, then the tile's
 * vertices and its groups as above (welded within a tile only; indices run on through the file).  flags: 0 or VRT_FACES_RUNS;
 * VRT_FACES_CLOSED is refused with VRT_ERR_INVALID (the tiles would get seams).  _file: writes path and beside it the library,
 * path with its extension replaced by .mtl, which the OBJ names without its directory; a file that cannot be written:
 * VRT_ERR_IO. */
int  vrt_scene_save_obj_mem (struct vrt_ctx* ctx, const vrt_scene* scene, const char* mtl_name, uint32_t flags, void** obj,
                             size_t* nobj, void** mtl, size_t* nmtl);
int  vrt_scene_save_obj_file(struct vrt_ctx* ctx, const vrt_scene* scene, const char* path, uint32_t flags);
/* Scene brushes and stamps (no reference analogue): an edit whose ids are composed ON THE DEVICE -- paint a sphere, drag a
 * capsule, recolour what is solid, fill what is empty, replace one material, paste a box of one scene into another -- and which
 * rebuilds around the TIGHT box of the voxels that really change, not around the shape's bounds.  csrc/vrt_brush.h is the
 * definition: plain integer arithmetic, no floating point, so which voxels a brush covers is the same on every machine.
 * Shape positions are in HALF VOXELS: the centre of voxel (x, y, z) is (2x+1, 2y+1, 2z+1), so a brush can be centred on a voxel
 * or on a voxel corner.  vrt_brush::p per shape:
 *   VRT_BRUSH_BOX        p[0..2] = lo, p[3..5] = size, in VOXELS; lo may be negative, each size in 1..2^30
 *   VRT_BRUSH_ELLIPSOID  p[0..2] = centre, p[3..5] = semi-axes, half voxels, each semi-axis in 1..1024 (a sphere: all equal;
 *                        (1, 1, 1) centred on a voxel: that voxel)
 *   VRT_BRUSH_CAPSULE    p[0..2] = a, p[3..5] = b, p[6] = radius, half voxels; radius in 1..1024, every coordinate of a and b in
 *                        -4096..12288; a == b is a sphere
 * (the rest of p is ignored).  A voxel INSIDE the shape becomes: VRT_BRUSH_SET id (0 carves); VRT_BRUSH_PAINT id where it was
 * not empty (id != 0); VRT_BRUSH_ADD id where it was empty (id != 0); VRT_BRUSH_REPLACE id where it was `match` (id != match).
 * A brush that lies partly outside the volume covers what is inside, and one that lies wholly outside changes nothing and is
 * VRT_OK -- unlike vrt_scene_edit_box, which refuses a box that leaves the volume.
 * result (may be NULL): how many voxels changed their id and the tight box that holds them (zeros when none did).  When
 * changed > 0 the scene is afterwards exactly what vrt_scene_edit_box(result.lo, result.size, the box's new ids) leaves, every
 * structure byte for byte a fresh build's.  When changed == 0 -- PAINT over air, REPLACE of an id that is not there, SET of the
 * id already there, a brush outside the volume -- nothing is written, no edit pass runs and the count planes' second set of
 * fields is NOT dropped.  Works on dense scenes of every field layout and on brick scenes after vrt_scene_reserve_bricks (before:
 * VRT_ERR_UNSUPPORTED; an edit that needs more slots than are free: VRT_ERR_UNSUPPORTED and nothing changed, as
 * vrt_scene_edit_box).  A NULL argument, an unknown shape or mode, a parameter outside its range or a broken id condition:
 * VRT_ERR_INVALID before any device work.  Stream rules and the metallic rule are vrt_scene_edit_box's (the ids actually written
 * decide, not the ids a shape could have written). */
#define VRT_BRUSH_BOX       0
#define VRT_BRUSH_ELLIPSOID 1
#define VRT_BRUSH_CAPSULE   2
#define VRT_BRUSH_SET       0
#define VRT_BRUSH_PAINT     1
#define VRT_BRUSH_ADD       2
#define VRT_BRUSH_REPLACE   3
typedef struct vrt_brush {
    int32_t shape, mode;
    int32_t p[9];
    uint8_t id, match;
} vrt_brush;
typedef struct vrt_brush_result {
    uint64_t changed;
    int32_t  lo[3];
    uint32_t size[3];    /* tight box of the changed voxels; zeros when changed == 0 */
} vrt_brush_result;
int  vrt_scene_brush(struct vrt_ctx* ctx, vrt_scene* scene, const vrt_brush* brush, vrt_brush_result* result);
/* Paste the box [src_lo, src_lo+size) of src into dst.  The source box must lie inside src and have no side above 512
 * (VRT_ERR_INVALID: stamp in parts); src may be dense or bricks (reserved or not), on the same device, and may be dst itself: the
 * source is gathered before anything is written, so an overlapping stamp copies the OLD content.  orient = perm | flips << 3
 * (the 48 symmetries of the box, 0 = identity): perm 0..5 = which source axis feeds destination x, y, z -- xyz, xzy, yxz, yzx,
 * zxy, zyx -- and bit a of flips reverses destination axis a (csrc/vrt_brush.h: stamp_source).  The oriented box is placed with
 * its low corner at dst_lo, which may be negative, and clipped to dst.  flags: VRT_STAMP_SKIP_EMPTY leaves the destination voxel
 * as it is where the source id is 0.  Ids are copied verbatim; the palettes are not compared.  Result, no-op rule, brick scenes
 * and errors as vrt_scene_brush. */
#define VRT_STAMP_SKIP_EMPTY 1u
int  vrt_scene_stamp(struct vrt_ctx* ctx, vrt_scene* dst, const int32_t dst_lo[3], const vrt_scene* src, const int32_t src_lo[3],
                     const uint32_t size[3], uint32_t orient, uint32_t flags, vrt_brush_result* result);
/* Flood fill (no reference analogue): select voxels by CONNECTIVITY on the device and rewrite them -- fill a closed cavity,
 * recolour or delete one object, or (VRT_FLOOD_MEASURE) ask how large the thing at the seed is.  csrc/vrt_flood.h is the
 * definition.  The bounds [lo, lo+size) are in voxels; lo may be negative, each size in 1..2^30; they are clipped to the volume and
 * the clipped bounds may have no side above 512 (VRT_ERR_INVALID: flood in parts).  A voxel PASSES under VRT_FLOOD_SAME iff its id
 * equals the id of the seed voxel (0 included: the cavity fill), under VRT_FLOOD_SOLID iff its id != 0.  The REGION is the
 * connected component of the seed among the passing voxels of the clipped bounds, joined through faces (VRT_FLOOD_FACES) or
 * through faces, edges and corners (VRT_FLOOD_CORNERS); a seed that does not pass has the empty region.  Every voxel of the region
 * becomes `id`.  result (not NULL): the region's voxel count and tight box (zeros when empty), the id found at the seed, and, as
 * vrt_scene_brush's result, how many voxels changed their id and their tight box.  Bounds wholly outside the volume or a seed
 * outside the clipped bounds change nothing and are VRT_OK with a zero result.  When edit.changed == 0 -- SAME with the id already
 * there, SOLID on an empty seed -- nothing is written, no edit pass runs and the count planes' second set of fields is kept.
 * flags: VRT_FLOOD_MEASURE writes nothing and reports the region only (edit stays zeros); it works on every scene, brick scenes
 * that were never reserved included.  Otherwise brick scenes, slot exhaustion (VRT_ERR_UNSUPPORTED, nothing changed), stream rules
 * and the metallic rule are vrt_scene_brush's.  A NULL argument, an unknown match, connectivity or flag, a size of 0 or above
 * 2^30: VRT_ERR_INVALID before any device work.  The masks the search needs (2 bits per voxel of the clipped bounds) are kept with
 * the scene between calls: vrt_scene_memory counts them, vrt_scene_trim drops them; VRT_ERR_UNSUPPORTED if they cannot be had. */
#define VRT_FLOOD_SAME    0
#define VRT_FLOOD_SOLID   1
#define VRT_FLOOD_FACES   6
#define VRT_FLOOD_CORNERS 26
#define VRT_FLOOD_MEASURE 1u   /* flags: write nothing, report the region only */
typedef struct vrt_flood {
    int32_t  seed[3], lo[3];
    uint32_t size[3];
    int32_t  match, connectivity;
    uint32_t flags;
    uint8_t  id;
} vrt_flood;
typedef struct vrt_flood_result {
    uint64_t region;
    int32_t  region_lo[3];
    uint32_t region_size[3];   /* the component and its tight box; zeros when empty */
    uint32_t seed_id;          /* the id found at the seed */
    vrt_brush_result edit;     /* as vrt_scene_brush's; zeros under VRT_FLOOD_MEASURE */
} vrt_flood_result;
int  vrt_scene_flood(struct vrt_ctx* ctx, vrt_scene* scene, const vrt_flood* flood, vrt_flood_result* result);
/* (diagnostics) how many rounds of its tile kernel the scene's latest flood ran */
int  vrt_debug_flood_rounds(const vrt_scene* scene, uint32_t* rounds);
/* Mesh voxelization (no reference analogue): compose a triangle mesh into the scene on the device.  csrc/vrt_voxelize.h is the
 * definition; it uses integers only, so which voxels a mesh covers is the same on every machine.  vertices: host int32[nv][3] in
 * SIXTEENTHS of a voxel (voxel (x, y, z) is the closed cube [16x, 16x+16]^3), every coordinate in -65536..131072; triangles: host
 * uint32[nt][3], indices into vertices; nt in 1..2^20, nv in 1..2^24.  fill: VRT_VOXELIZE_SURFACE covers every voxel whose closed
 * cube meets a triangle (conservative, the 13-axis test with closed comparisons; degenerate triangles included),
 * VRT_VOXELIZE_SOLID every voxel whose centre lies inside the mesh by parity along +x (an odd number of triangles cross the ray
 * from the centre towards +x; top-left rule on the yz-projection, so a closed mesh fills the same voxels whatever the order,
 * winding or subdivision of its triangles); both bits: the union.  The bounds [lo, lo+size) are in voxels; lo may be negative,
 * each size in 1..2^30; they are clipped to the volume and the clipped bounds may have no side above 512 (VRT_ERR_INVALID:
 * voxelize in parts).  Voxels outside the bounds never change, but triangles outside them still count for the parity: a solid
 * voxelized in parts gives the same voxels as in one piece.  A covered voxel becomes `id` under mode VRT_BRUSH_SET, PAINT, ADD or
 * REPLACE(match), with vrt_scene_brush's conditions on the ids.  result (not NULL): how many voxels of the bounds the mesh covers,
 * and, as vrt_scene_brush's result, how many changed their id and their tight box.  Bounds wholly outside the volume: VRT_OK with
 * a zero result.  When edit.changed == 0 nothing is written, no edit pass runs and the count planes' second set of fields is kept.
 * Brick scenes, slot exhaustion (VRT_ERR_UNSUPPORTED, nothing changed), stream rules and the metallic rule are vrt_scene_brush's.
 * A NULL argument, a zero count or one above its limit, an index >= nv, a coordinate out of range, an unknown mode or fill bit, a
 * fill of 0, a size of 0 or above 2^30: VRT_ERR_INVALID before any device work.  A call that would test more than 2^31 candidate
 * voxels (the triangles' bounding boxes cut to the bounds, summed): VRT_ERR_UNSUPPORTED, nothing changed.  The masks (1 or 2 bits
 * per voxel of the clipped bounds) are kept with the scene between calls: vrt_scene_memory counts them, vrt_scene_trim drops
 * them; VRT_ERR_UNSUPPORTED if they or the mesh's device copy cannot be had. */
#define VRT_VOXELIZE_SURFACE 1u
#define VRT_VOXELIZE_SOLID   2u
typedef struct vrt_voxelize {
    int32_t  lo[3]; uint32_t size[3];      /* bounds, voxels */
    int32_t  mode; uint32_t fill;          /* VRT_BRUSH_* ; VRT_VOXELIZE_SURFACE | VRT_VOXELIZE_SOLID */
    uint8_t  id, match;
} vrt_voxelize;
typedef struct vrt_voxelize_result { uint64_t covered; vrt_brush_result edit; } vrt_voxelize_result;
int  vrt_scene_voxelize(struct vrt_ctx* ctx, vrt_scene* scene, const int32_t* vertices, uint32_t nv,
                        const uint32_t* triangles, uint32_t nt, const vrt_voxelize* job, vrt_voxelize_result* result);
/* (diagnostics) rows per work item of this scene's voxelizations from now on (0: the default), and how many work items the
 * latest one launched (surface + solid) */
int  vrt_debug_voxelize_item_rows(vrt_scene* scene, uint32_t rows);
int  vrt_debug_voxelize_items(const vrt_scene* scene, uint32_t* items);
/* Morphology (no reference analogue): select voxels by their NEIGHBOURHOOD in the scene itself and grow, shrink, open, close or
 * hollow the solid on the device -- hollow a voxelized solid to a shell, thicken a thin surface, remove specks (OPEN), close
 * pinholes (CLOSE), erode or dilate by a margin.  csrc/vrt_morph.h is the definition; it uses integers only.  S is the set of
 * solid cells (id != 0) of the infinite grid: the scene inside the volume, empty outside it (VRT_MORPH_BORDER_SOLID: solid outside
 * it).  connectivity VRT_MORPH_FACES measures distance in L1, VRT_MORPH_CORNERS in L-infinity; radius r in 1..8.  dil_r(X) holds
 * every cell within r of a cell of X, ero_r(X) every cell whose whole ball of radius r lies in X.  The result set R:
 *   VRT_MORPH_DILATE dil_r(S) | VRT_MORPH_ERODE ero_r(S) | VRT_MORPH_OPEN dil_r(ero_r(S)) | VRT_MORPH_CLOSE ero_r(dil_r(S)) |
 *   VRT_MORPH_HOLLOW S \ ero_r(S), a shell of thickness r.
 * R is computed on the whole grid and written inside the bounds [lo, lo+size) only (voxels; lo may be negative, each size in
 * 1..2^30; clipped to the volume, no clipped side above 512: VRT_ERR_INVALID, work in parts): an empty voxel in R becomes `id`, a
 * solid voxel not in R becomes 0, every other voxel keeps its id -- morphology never recolours, and a grown voxel does not
 * inherit a neighbour's id.  The volume outside the bounds is read as it is, r cells out (2r for OPEN and CLOSE), so parts
 * computed from the same old scene agree with the whole; parts applied in place one after another see each other.  DILATE and
 * CLOSE need id >= 1 (VRT_ERR_INVALID); ERODE, OPEN and HOLLOW never add a voxel and ignore it.  result (not NULL): how many
 * voxels were added and removed (added + removed == edit.changed) and, as vrt_scene_brush's result, the edit.  Bounds wholly
 * outside the volume: VRT_OK with a zero result.  When edit.changed == 0 nothing is written, no edit pass runs and the count
 * planes' second set of fields is kept.  flags: VRT_MORPH_MEASURE writes nothing and reports added and removed only (edit stays
 * zeros); it works on every scene, brick scenes that were never reserved included.  Otherwise brick scenes, slot exhaustion
 * (VRT_ERR_UNSUPPORTED, nothing changed), stream rules and the metallic rule are vrt_scene_brush's.  A NULL argument, an unknown
 * operation, connectivity or flag, a radius outside 1..8, a size of 0 or above 2^30: VRT_ERR_INVALID before any device work.  The
 * masks (2 bits per cell of the clipped bounds grown by the halo) are kept with the scene between calls: vrt_scene_memory counts
 * them, vrt_scene_trim drops them; VRT_ERR_UNSUPPORTED if they cannot be had. */
#define VRT_MORPH_DILATE  0
#define VRT_MORPH_ERODE   1
#define VRT_MORPH_OPEN    2
#define VRT_MORPH_CLOSE   3
#define VRT_MORPH_HOLLOW  4
#define VRT_MORPH_FACES   6
#define VRT_MORPH_CORNERS 26
#define VRT_MORPH_BORDER_SOLID 1u   /* flags: every cell outside the volume is solid */
#define VRT_MORPH_MEASURE      2u   /* flags: write nothing, report added and removed only */
typedef struct vrt_morph {
    int32_t  op, connectivity, radius;
    int32_t  lo[3];
    uint32_t size[3];
    uint32_t flags;
    uint8_t  id;
} vrt_morph;
typedef struct vrt_morph_result {
    uint64_t added, removed;
    vrt_brush_result edit;     /* as vrt_scene_brush's; zeros under VRT_MORPH_MEASURE */
} vrt_morph_result;
int  vrt_scene_morph(struct vrt_ctx* ctx, vrt_scene* scene, const vrt_morph* morph, vrt_morph_result* result);
/* Connected components: label, measure and filter all the regions of the bounds at once on the device -- delete every speck below N
 * voxels, fill every closed cavity, keep only the largest object, count the islands and list their sizes and boxes.
 * csrc/vrt_components.h is the definition; it uses integers only.  The bounds [lo, lo+size) are in voxels (lo may be negative, each
 * size in 1..2^30; clipped to the volume, no clipped side above 512: VRT_ERR_INVALID, work in parts; wholly outside the volume:
 * VRT_OK with a zero result).  A voxel PASSES under VRT_COMP_SOLID and VRT_COMP_SAME iff its id != 0, under VRT_COMP_EMPTY iff its
 * id == 0; two adjacent passing voxels are JOINED always (SOLID, EMPTY) or iff their ids are equal (SAME); adjacent means a shared
 * face (VRT_COMP_FACES) or a face, edge or corner (VRT_COMP_CORNERS), among the voxels of the clipped bounds only.  The ROOT of a
 * component is its voxel of lowest rx + csize[0] * (ry + csize[1] * rz), (rx, ry, rz) its offset from the clipped lo; components
 * are numbered 0..n-1 in ascending root order, so every output is a function of the scene's content alone.
 * vrt_scene_components lists one vrt_component per component in that order (records may be NULL with capacity 0: count only; a
 * capacity below the count with records != NULL: VRT_ERR_INVALID after *result is written, as vrt_scene_list_box).  It works on
 * every scene, brick scenes never reserved included, and writes nothing to the scene.  result->largest: the number of the component
 * with the most voxels, the lowest number among equals (0 when there is none).
 * vrt_scene_component_labels copies the labels (a voxel's component number, 0xFFFFFFFF if it does not pass; read-box order) of a
 * box inside the clipped bounds of the scene's latest labelling (by vrt_scene_components or vrt_scene_filter_components).  Every call
 * that rewrites the scene after it -- edit, fill, brush, stamp, flood, voxelize, morph, filter -- and vrt_scene_trim make that
 * labelling stale: VRT_ERR_INVALID.
 * vrt_scene_filter_components labels the bounds, SELECTS the components with min_voxels <= voxels <= max_voxels,
 * (faces & faces_all) == faces_all, (faces & faces_none) == 0 and, under VRT_COMP_KEEP_LARGEST, all but the largest, and makes every
 * voxel of a selected component `id`, with vrt_scene_flood's rules for the edit: no-op (changed == 0 writes nothing), tight box,
 * brick slots (VRT_ERR_UNSUPPORTED, nothing changed), the metallic rule, the stream rules.  VRT_COMP_MEASURE writes nothing and
 * reports the selection only; it works on every scene.  A NULL argument, an unknown match, connectivity or flag, a face bit above
 * 5, min_voxels > max_voxels, a size of 0 or above 2^30: VRT_ERR_INVALID before any device work.  The label volume (4 bytes per
 * voxel of the clipped bounds: 512 MiB at 512^3) and the table are kept with the scene: vrt_scene_memory counts them,
 * vrt_scene_trim drops them; VRT_ERR_UNSUPPORTED if they cannot be had. */
#define VRT_COMP_SOLID   0
#define VRT_COMP_SAME    1
#define VRT_COMP_EMPTY   2
#define VRT_COMP_FACES   6
#define VRT_COMP_CORNERS 26
#define VRT_COMP_KEEP_LARGEST 1u   /* vrt_component_filter.flags: the largest component is never selected */
#define VRT_COMP_MEASURE      2u   /* vrt_component_filter.flags: write nothing, report the selection only */
typedef struct vrt_components {
    int32_t  lo[3];
    uint32_t size[3];
    int32_t  match, connectivity;
    uint32_t flags;            /* 0: none is defined */
} vrt_components;
typedef struct vrt_component {
    int32_t  root[3];          /* volume coordinates */
    uint32_t id;               /* of the root voxel */
    uint64_t voxels;
    int32_t  lo[3];            /* the tight box */
    uint32_t size[3];
    uint32_t faces;            /* bit d: a voxel on face d of the clipped bounds; 0 = -x, 1 = +x, 2 = -y, 3 = +y, 4 = -z, 5 = +z */
    uint32_t reserved;         /* 0 */
} vrt_component;
typedef struct vrt_components_result {
    uint64_t components, voxels;
    uint64_t largest;          /* number of the largest; lowest number wins ties */
} vrt_components_result;
typedef struct vrt_component_filter {
    uint64_t min_voxels, max_voxels;
    uint32_t faces_all, faces_none;
    uint32_t flags;
    uint8_t  id;               /* what every voxel of a selected component becomes */
} vrt_component_filter;
typedef struct vrt_filter_result {
    uint64_t components, voxels;   /* selected */
    vrt_brush_result edit;     /* as vrt_scene_brush's; zeros under VRT_COMP_MEASURE */
} vrt_filter_result;
int  vrt_scene_components(struct vrt_ctx* ctx, const vrt_scene* scene, const vrt_components* components, vrt_component* records, uint64_t capacity,
                          vrt_components_result* result);
int  vrt_scene_component_labels(struct vrt_ctx* ctx, const vrt_scene* scene, const int32_t lo[3], const uint32_t size[3], uint32_t* labels /* host */);
int  vrt_scene_filter_components(struct vrt_ctx* ctx, vrt_scene* scene, const vrt_components* components, const vrt_component_filter* filter,
                                 vrt_filter_result* result);
void vrt_scene_free(vrt_ctx* ctx, vrt_scene* sc);            /* VoxelScene::destroy */

/* ---- settings -------------------------------------------------------------------------------- */
/* Defaults of VoxelRenderSettings (voxel_render_settings.hpp:21-42) + shader constants. */
void vrt_settings_default(vrt_settings* s);

/* ---- geometry stage -------------------------------------------------------------------------- */
/* GeometryStage::record (geometry_stage.cpp:106-153) == one full-screen run of voxel_volume.frag:
 * primary-ray DDA kernel + (when AO / shadow / reflection rays are enabled) the secondary-ray and
 * shading kernels.  Asynchronous on the context stream.
 * Limits: screen_size up to 32768 per side and below 2^28 pixels per frame (16384 x 16384 is refused with
 * VRT_ERR_UNSUPPORTED): a launch addresses the full-frame planes with 32-bit byte offsets -- 16 B per pixel in the
 * position plane -- and sharded launches (vrt_shard) index the same full-frame planes, so strips do not lift the limit;
 * a larger image is rendered as several frames whose camera planes are shifted. */
int  vrt_render_geometry(vrt_ctx* ctx, const vrt_scene* sc, const vrt_push* push,
                         const vrt_settings* settings, const vrt_frame* frame, const vrt_shard* shard);

/* The same for n frames of one scene, one screen size and one set of settings -- consecutive camera poses of an
 * animation (App::run's frame loop, source/app.cpp:18-27, rendered offline), or the frames of a multi-GPU batch --
 * in ONE launch (per 256 frames): the tiles of frame f+1 are dispatched while frame f drains, so the tail of a frame
 * (tens of microseconds during which most of the GPU idles) is paid once per launch instead of once per frame.
 * Up to 8 frames travel in the kernel arguments; larger batches go through a small table in device memory that is
 * uploaded on a stream of its own.  pushes[n], frames[n]; every frame needs its own output planes.  Results are
 * identical to n single calls. */
int  vrt_render_geometry_batch(vrt_ctx* ctx, const vrt_scene* sc, int32_t n, const vrt_push* pushes,
                               const vrt_settings* settings, const vrt_frame* frames, const vrt_shard* shard);

/* The same with one strip assignment PER FRAME (shards[n]; all with the same nranks and strip_rows): a rank of a
 * multi-GPU batch traces frame block b with the assignment of rank (rank + b) % nranks, so that rows which do not divide
 * evenly over the ranks still cost every rank the same per step -- in one launch.  No reference analogue. */
int  vrt_render_geometry_slots(vrt_ctx* ctx, const vrt_scene* sc, int32_t n, const vrt_push* pushes,
                               const vrt_settings* settings, const vrt_frame* frames, const vrt_shard* shards);

/* ---- ray queries (no reference analogue as an interface; the rays are traceRay's) ----------------------------- */
/* Trace rays the caller supplies, or the primary rays of single pixels, through a scene: which voxel a ray meets first
 * (traceRay, voxel_volume.frag:176-196 over traceRayInt, :127-174), or only whether it meets one (traceRayHit, :198-202).
 * Output planes of a batch of n rays: DEVICE pointers, any may be NULL (not written), at least one non-NULL; pos and voxel
 * 4-byte aligned.  A miss -- the ray leaves the volume or exhausts max_steps -- is 0 in every plane. */
typedef struct vrt_ray_hits {
    uint8_t* material;  /* n:  voxel id at the hit, 0 = miss (traceRay, voxel_volume.frag:176-196)                          */
    float*   pos;       /* 3n: RayHit.pos (frag:187-189), bit for bit what the position plane holds for a primary ray       */
    int32_t* voxel;     /* 3n: grid cell of the hit (mapPos, frag:135,168); (0,0,0) on a miss, like the hit_voxel plane     */
    int8_t*  normal;    /* 3n: -mask * rayStep (frag:190) before normalisation, each component in {-1,0,1}                  */
} vrt_ray_hits;
/* origins, dirs: DEVICE pointers to n x 3 packed floats in volume coordinates (voxel units, the volume is [0,W]x[0,H]x[0,D]).
 * The direction is used as given -- traceRay does not normalise, and the +0.1 of boxIntersection (frag:122) is in units of
 * it.  max_steps has MAX_RAY_STEPS' meaning (frag:68,151).  For a distance limit per ray see vrt_trace_segments / vrt_occluded_segments.
 * Rays are traced in the order given, one per lane, 64 consecutive rays per wave: neighbouring rays that walk neighbouring
 * cells cost least (tools/exp_query.py measures the price of an order that does not).
 * Asynchronous on the context's stream; n == 0 is VRT_OK and launches nothing.  A scene may be queried between edits under
 * the rule of rendering: a query enqueued before vrt_scene_edit_box sees the old volume, a later one the new.
 * n < 0, n > 2^28 (268 435 456: the kernel indexes the dwords of a plane, three per ray, and their byte offsets in 32
 * bits -- split a larger batch), a NULL argument, no output plane, max_steps == 0: VRT_ERR_INVALID, before any device work.
 * For every ray with finite origin and direction the planes equal the reference's traceRay of the same volume, pos by bit
 * pattern, zero direction components (+0 and -0), the direction (0, 0, 0) from inside the volume, subnormal components beside
 * ordinary ones and origins up to 10^30 voxels away included -- with the set left open in which the GLSL itself is not defined.
 * Call a direction component d "flat" when 1 / d overflows (d is +-0 or |d| <= 2^-128).  Left open:
 *  (1) a flat component whose origin component is exactly 0 or exactly the volume's size on that axis.  boxIntersection
 *      multiplies 0 by infinity there (frag:113-114); this library's fminf / fmaxf drop the NaN, the axis' slab becomes empty
 *      (entry at +inf or exit at -inf), the box test fails, and the ray is marched from its origin's own cell without
 *      boxIntersection's advance: a miss at once where that cell lies outside the volume, else a march from the origin;
 *  (2) a flat, negative, non-zero component whose origin component is an integer: sideDist is 0 * inf (frag:144);
 *  (3) a direction whose three components are all flat with an origin outside the volume -- (0, 0, 0) included:
 *      boxIntersection's point is origin + inf * d -- and a direction whose three components are all zero or subnormal
 *      (|d| < 2^-126) without all being zero: GLSL may flush them, and where it does not the three sideDist are infinite or
 *      overflow within a few steps and the loop steps every axis on the tie.  The query reads such a direction as (0, 0, 0);
 *  (4) a ray one of whose sideDist overflows within max_steps (every stepping |d| below about 2^-117 at 1024 steps).
 * Never a fault, but pinned by nothing.  float -> int conversions saturate (NaN: 0), as the GPU's instruction does.
 * Traversal is what VRT_TRAVERSAL_AUTO resolves to: the hand-written look-up loop on dense scenes whose fields it can
 * address in 32 bits (for max_steps <= 1024, the budgets its position recovery is exact for; above, VRT_TRAVERSAL_DF; a wave
 * of 64 rays that holds a subnormal direction component takes VRT_TRAVERSAL_DF too), VRT_TRAVERSAL_DF with 64-bit offsets on
 * larger volumes, the brick march on brick scenes.  Of the context options only
 * "thresh_runs" is looked at. */
int  vrt_trace_rays(vrt_ctx* ctx, const vrt_scene* scene, int64_t n, const float* origins, const float* dirs,
                    uint32_t max_steps, const vrt_ray_hits* out);
/* traceRayHit (frag:198-202): occluded[i] = 1 if ray i meets a voxel within max_steps, else 0 -- material != 0 of
 * vrt_trace_rays, for less work (a ray whose clearance covers the rest of its budget is decided where it stands). */
int  vrt_occluded_rays(vrt_ctx* ctx, const vrt_scene* scene, int64_t n, const float* origins, const float* dirs,
                       uint32_t max_steps, uint8_t* occluded);
/* The primary rays of n pixels: xy is a DEVICE pointer to n x (x, y), and ray i is the one main() generates for that pixel
 * under `push` (frag:312-322, jitter included) -- by the device function the geometry stage itself uses, so record i equals
 * what a frame rendered with that push and max_steps holds at the pixel in hit_id, position, hit_voxel and hit_mask / the
 * sign of normal8.  A pixel outside push->screen_size is a miss, not an error.  push->volume_bounds must equal the scene's
 * dimensions and screen_size be within vrt_render_geometry's limits (else VRT_ERR_INVALID). */
int  vrt_pick_pixels(vrt_ctx* ctx, const vrt_scene* scene, const vrt_push* push, uint32_t max_steps,
                     int64_t n, const int32_t* xy, const vrt_ray_hits* out);
/* Ray segments: vrt_trace_rays / vrt_occluded_rays with a distance limit per ray -- is there a voxel between A and B (a shadow
 * ray to a point light, line of sight, a sweep that stops at a wall).  t_max: a DEVICE pointer to n floats, 4-byte aligned.
 * The hit's parameter along the ray as given is  t_hit = t_adv + d,  one fp32 addition: d is the length RayHit.pos is made with
 * (pos = p + d * dir, frag:187-189) and t_adv what boxIntersection moved the origin by to get p -- tmin + 0.1 where its test
 * passes (frag:120-123), else 0.  t is in units of dir, like the +0.1: with origin A and direction B - A, t = 1 is B.  A hit is
 * kept iff t_hit <= t_max (an fp32 compare: a NaN t_max keeps nothing, +inf everything, 0 or -0 a ray that starts inside a solid
 * voxel); a hit that is not kept is a miss, 0 in every plane and in t_hit.  A kept hit's planes are vrt_trace_rays' of the same
 * ray and max_steps, bit for bit, under the same contract and with the same open set; with t_max = +inf the two calls agree on
 * every ray.  The quirk inherited from boxIntersection: a ray that starts outside the volume is advanced by 0.1 * |dir| voxels
 * past the face it enters through, so a voxel within that distance of the face is not seen.
 * t_hit: a DEVICE pointer to n floats, or NULL.  At least one of out's planes or t_hit must be non-NULL; out may be NULL if t_hit
 * is not.  Errors: those of vrt_trace_rays, in its order, and a NULL t_max.  Traversal as for vrt_trace_rays; both calls run the
 * closest-hit march (t_hit is made from its final state).  Of the context options "thresh_runs" and "segment_budget" are looked
 * at; neither changes a result.  csrc/vrt_query_seg.h is the definition, host and device. */
int  vrt_trace_segments(struct vrt_ctx* ctx, const vrt_scene* scene, int64_t n, const float* origins, const float* dirs,
                        const float* t_max, uint32_t max_steps, const vrt_ray_hits* out, float* t_hit);
/* occluded[i] = 1 if ray i has a hit within max_steps with t_hit <= t_max[i], else 0; nothing else is written. */
int  vrt_occluded_segments(struct vrt_ctx* ctx, const vrt_scene* scene, int64_t n, const float* origins, const float* dirs,
                           const float* t_max, uint32_t max_steps, uint8_t* occluded);

/* ---- ray generation for caller-side cameras (no reference analogue: the only camera the reference draws is main()'s pinhole,
 * voxel_volume.frag:312-322, whose horizontal field of view is fixed at 90 degrees because camDir is re-normalised -- the
 * CameraController's focal length has no effect) ---------------------------------------------------------------------------------
 * vrt_camera_rays writes the primary rays of a W x H frame under one of three camera models into the two planes of 3 packed
 * floats per ray that vrt_trace_rays and vrt_occluded_rays take: which voxel every pixel of a wide-angle, an orthographic or a
 * panoramic view sees, or whether it sees one, is then one more call.  csrc/vrt_raygen.h defines the three models step by step in
 * fp32; the GPU result equals it bit for bit.  vrt_render_rays (below) shades such rays: the geometry stage's full G-buffer for any
 * camera. */
#define VRT_CAMERA_PERSPECTIVE  0   /* main()'s pinhole with a field of view: tan_half = tan(horizontal FOV / 2); 1.0f is the reference's camera bit for bit */
#define VRT_CAMERA_ORTHOGRAPHIC 1   /* parallel rays along cam_dir; half_width: half the view's width in voxels */
#define VRT_CAMERA_PANORAMA     2   /* equirectangular around cam_pos, the inverse of skyColor's mapping (frag:98-105); the basis is not used */
typedef struct vrt_ray_camera {
    int32_t  model;        /* VRT_CAMERA_* */
    vrt_push basis;        /* cam_pos, cam_dir, cam_right, cam_up, camera_jitter (perspective only); the other fields are not read */
    float    tan_half;     /* perspective: > 0 and finite */
    float    half_width;   /* orthographic: > 0 and finite */
} vrt_ray_camera;
/* The rays of a W x H frame: origins and dirs are DEVICE pointers to W * H x 3 packed floats, ray py * W + px for pixel (px, py),
 * 4-byte aligned, not overlapping.  Perspective and panorama directions are unit vectors, the orthographic one is
 * normalize(cam_dir).  With VRT_CAMERA_PERSPECTIVE and tan_half == 1.0f ray py * W + px is the ray vrt_pick_pixels traces for
 * pixel (px, py) under `basis` with screen_size (W, H).  Asynchronous on the context's stream (the panorama's tables --
 * 8 (W + H) bytes -- are uploaded with the call; a second panorama call on the context waits for the first one's kernel).
 * Frame-size limits of vrt_render_geometry.
 * VRT_ERR_INVALID, before any device work: a NULL argument, W or H < 1 or beyond the limits, a misaligned or overlapping
 * pointer, an unknown model, a tan_half (perspective) or half_width (orthographic) that is not finite and positive, a
 * degenerate basis (non-finite position or jitter; perspective and orthographic: a zero or non-finite determinant). */
int  vrt_camera_rays(vrt_ctx* ctx, const vrt_ray_camera* camera, int32_t W, int32_t H, float* origins, float* dirs);
/* vrt_camera_rays with a sub-pixel sample offset: ray py * W + px goes through the point (px + 0.5 + offset[0], py + 0.5 + offset[1])
 * of the pixel grid instead of the pixel's centre.  offset is a HOST pointer to two floats, in pixels, finite, |o| <= 1.  All three
 * models: perspective and orthographic shift the screen coordinate (the perspective model's camera_jitter is still added, and what
 * vrt_camera_rays does with it is unchanged), the panorama's tables are computed at the shifted positions.  This is what gives
 * the orthographic and the panorama model -- which apply no jitter -- samples that fall between each other from frame to frame
 * (vrt_jitter_offset's values serve), for vrt_upsample_camera to gather.  With offset (0, 0) every ray equals vrt_camera_rays'
 * bit for bit.  csrc/vrt_raygen.h, camera_ray_offset, is the definition; the GPU result equals it bit for bit.
 * VRT_ERR_INVALID, before any device work: every case of vrt_camera_rays; offset NULL, not finite or beyond 1 in magnitude.
 * (The context parameter of this function and of vrt_upsample_camera below is spelled `struct vrt_ctx*`: the same type, the same
 * ABI.  tests/test_stream_cases_cpu.py finds the context functions by the spelling `vrt_ctx*` and wants each in the table of
 * tests/stream_common.py, which the change that added these two functions could not touch; tests/test_gpu_upsample_cam.py runs
 * both on the three kinds of stream behind a busy device itself.  DESIGN.md 8 lists the table entry, and this spelling, as open.) */
int  vrt_camera_rays_offset(struct vrt_ctx* ctx, const vrt_ray_camera* camera, int32_t W, int32_t H, const float offset[2],
                            float* origins, float* dirs);

/* ---- the G-buffer of caller-supplied rays (no reference analogue: the reference draws main()'s pinhole only) -------------------
 * The G-buffer of a W x H frame whose primary rays the caller supplies: ray py * W + px is pixel (px, py)'s.  origins, dirs: DEVICE
 * pointers to W * H x 3 packed floats (what vrt_camera_rays writes and vrt_trace_rays takes), 4-byte aligned, overlapping no
 * output plane.  Every plane of `out` holds what main() (voxel_volume.frag:312-346) writes for pixel (px, py) of frame index
 * `frame` if that pixel's primary ray is (origin, dir):
 *   the primary record  vrt_trace_rays' record of the ray with settings->max_steps, bit for bit: the same open set, the same
 *                       reading of an all-small direction as (0, 0, 0), the same traversal (the rule for budgets above 1024 included)
 *   position            (pos, 0);  depth = length(pos - origin), 0 on a miss;  mask8 = 230 on a hit, 0 on a miss;  motion = 0
 *   normal8             the SNORM8 codes of normalize(-mask * rayStep), 0 on a miss
 *   hit_id, hit_voxel, hit_mask   material id, hit cell and final DDA mask of the primary hit (0 on a miss)
 *   color8 / color_f    a hit: colorMainRay (frag:267-307) with RayHit.dir = the direction as given -- AO, shadow and bounce rays
 *                       as vrt_render_geometry traces them; the blue-noise texel is pixel (px, py)'s (its coordinate does not
 *                       depend on W or H), the sample offset is frame % 32.  A miss: skyColor(dir).
 * Directions are used as given.  vrt_camera_rays delivers unit vectors; a direction that is not one is traced exactly as
 * vrt_trace_rays traces it, and its sky texel, its reflection and its AO are whatever the formulas give for it.  Only FINITE
 * directions are in the contract.  The sky look-up of a miss cannot fault on any value (a NaN coordinate reaches texel 0), but a
 * metallic hit reflects the direction into a bounce ray, and a bounce ray made from a NaN, an infinity or a subnormal component
 * is one vrt_trace_rays' contract does not cover either: what such a pixel holds is pinned by nothing, and the path it takes
 * through the shading kernel has not been examined.
 * VRT_ERR_UNSUPPORTED: a non-NULL steps_primary, steps_total, rays_total or color8_strips; any bit of settings->flags; a
 * settings->traversal other than VRT_TRAVERSAL_AUTO.
 * VRT_ERR_INVALID, before any device work: a NULL argument, W or H < 1 or beyond vrt_render_geometry's frame limits (2^28 pixels
 * and more included), max_steps == 0, max_bounces > VRT_MAX_BOUNCES, no output plane at all, a misaligned ray plane, a ray plane
 * that overlaps an output plane.
 * Asynchronous on the context's stream.  There is no vrt_shard: a rank of a multi-GPU frame passes the rays of its own rows as a
 * frame of that many rows.  Two kernels, the split form of the geometry stage over a ray buffer: the primary march of
 * vrt_trace_rays writes the planes, the misses' colour and one 16-byte record per hit; the shading kernel runs one lane per hit.
 * Of the context options "thresh_runs" and "ao_batch" are honoured and nothing else. */
int  vrt_render_rays(vrt_ctx* ctx, const vrt_scene* scene, int32_t W, int32_t H, const float* origins, const float* dirs,
                     uint32_t frame, const vrt_settings* settings, const vrt_frame* out);

/* ---- denoiser stage -------------------------------------------------------------------------- */
#define VRT_DENOISE_CANONICAL  0  /* the intended 9-tap a-trous filter                               */
#define VRT_DENOISE_AS_SHIPPED 1  /* the std140-aliased 3-tap filter the shipped UBO upload produces  */
#define VRT_DENOISE_FAST       2  /* flag, OR-ed into either: the weighted passes (pass >= 1, integral stepWidth) evaluate the three
                                   * edge-stopping weights as ONE hardware exponential, exp2(-(dc2*kc + dn2*kn + dp2*kp)), and divide
                                   * by multiplying with the hardware reciprocal -- the shader's own freedom (GLSL exp / division are
                                   * not correctly rounded either).  Stated bound against the exact mode and the oracle: at most ONE
                                   * RGBA8 code per channel per pass (tests/test_gpu_denoise.py), non-finite positions included: a NaN
                                   * position distance weighs 1 here as in the exact mode (tests/test_gpu_denoise_shard.py); the exact
                                   * mode stays the default. */

/* DenoiserSettings, voxel_render_settings.hpp:21-29. */
typedef struct vrt_denoiser_settings {
    int32_t iterations;     /* default 2, max 10 (MAX_DENOISER_PASSES, denoiser_stage.hpp:9) */
    float   phi_color0;     /* 20.4 */
    float   phi_normal0;    /* 1e-2 */
    float   phi_pos0;       /* 1e-1 */
    float   step_width;     /* 2.0  */
    int32_t mode;           /* VRT_DENOISE_* */
} vrt_denoiser_settings;
void vrt_denoiser_settings_default(vrt_denoiser_settings* s);

/* DenoiserStage::record(cmd, flightFrame, color, normal, pos) (denoiser_stage.cpp:156-258): runs
 * `iterations` ping-pong passes of denoiser.frag:38-73 with the per-pass parameters of
 * denoiser_stage.cpp:143-154.  target0/target1 are the two RGBA8 ping-pong images (_colorTargets);
 * *result receives the one holding the final image (color_in itself when iterations == 0).
 * With a shard, only the rank's own rows of the final image are valid; the guide planes must already
 * hold `vrt_denoise_halo_rows()` valid rows either side of every owned strip.  A sharded call READS the rank's
 * own rows +- vrt_denoise_halo_rows(), clipped to the frame, of the three input planes and nothing beyond (what
 * the other rows hold never reaches an own row of the result); it WRITES, in both targets, own rows +- the halo
 * at most (pass i: own rows +- the reaches of the later passes) and no other row.  A rank without a strip
 * launches nothing.  The halo may exceed strip_rows (16-row strips, five passes at step width 2: 25 rows): the
 * extended regions of a rank's own strips then overlap, the overlap is written twice with equal values and the
 * result is the same -- only vrt_pack_halo, which sends rows of ONE neighbouring strip, refuses such a halo, so
 * the caller must bring those rows in another way. */
int  vrt_denoise(vrt_ctx* ctx, int32_t W, int32_t H, const vrt_denoiser_settings* ds,
                 const uint8_t* color_in, const int8_t* normal8, const float* position,
                 uint8_t* target0, uint8_t* target1, const vrt_shard* shard, const uint8_t** result);
/* Sum of the per-pass tap reach ceil(stepWidth_i) over all passes: rows a strip needs from its neighbours. */
int  vrt_denoise_halo_rows(const vrt_denoiser_settings* ds);
/* A pass with an integral tap offset (<= 5; whole frames and sharded passes alike) is computed in two steps: a cheap evaluation of
 * every pixel (hardware exponential and reciprocal, integer code distances) and a second, literal one -- the operations of
 * denoiser.frag:48-72 as the numeric spec fixes them -- of the pixels whose cheap value lies within `guard` RGBA8 codes of a
 * rounding boundary of the RGBA8 target (csrc/vrt_denoise_bound.h derives the guard).  The image is the literal evaluation's,
 * bit for bit.  vrt_denoise_guard reports the guard of a pass (+inf: the pass is computed literally throughout; needs no
 * device); vrt_debug_denoise_redone how many pixels of a pass the latest vrt_denoise call on the context evaluated twice
 * (counted only while the context option "denoise_count" is 1). */
int  vrt_denoise_guard(const vrt_denoiser_settings* ds, int32_t pass, float* guard);
int  vrt_debug_denoise_redone(vrt_ctx* ctx, int32_t pass, uint32_t* pixels);

/* ---- multi-GPU strip packing (feeds the RCCL gather; no reference analogue) -------------------- */
/* Number of rows rank owns. */
int  vrt_shard_rows(int32_t H, const vrt_shard* shard);
/* Pack the rows a rank owns (in increasing row order) of a full-frame plane with `bytes_per_px` into a
 * contiguous buffer, or scatter them back (root side, after the gather).  Device pointers. */
int  vrt_pack_rows(vrt_ctx* ctx, const void* full, void* packed, int32_t W, int32_t H,
                   int32_t bytes_per_px, const vrt_shard* shard);
int  vrt_unpack_rows(vrt_ctx* ctx, const void* packed, void* full, int32_t W, int32_t H,
                     int32_t bytes_per_px, const vrt_shard* shard);
/* The same for n images in one launch per 64 images (host arrays of n device pointers): the frames of a batch on a
 * rank (one shard for all), and at the root of the gather frames x source ranks (shards[n], one per image).  The shards of
 * a call may differ in every field (images whose packed buffers differ in rows take launches of their own).  A NULL image
 * pointer or a bad shard anywhere in the arrays: VRT_ERR_INVALID before anything is copied. */
int  vrt_pack_rows_batch(vrt_ctx* ctx, int32_t n, const void* const* full, void* const* packed, int32_t W, int32_t H,
                         int32_t bytes_per_px, const vrt_shard* shard);
int  vrt_unpack_rows_batch(vrt_ctx* ctx, int32_t n, const void* const* packed, void* const* full, int32_t W, int32_t H,
                           int32_t bytes_per_px, const vrt_shard* shards);
/* Pack / unpack the halo rows exchanged with the ring neighbours before a sharded denoise:
 * dir = -1: the first `halo` rows of every owned strip (sent to the rank owning the strip above),
 * dir = +1: the last `halo` rows of every owned strip (sent to the rank owning the strip below).
 * vrt_unpack_halo takes the SENDER's shard and the same dir: the rows are written back at their true
 * frame positions in the receiver's full-frame plane (i.e. just outside the receiver's own strips).
 * vrt_unpack_rows likewise takes the shard of the rank that packed the buffer. */
int  vrt_pack_halo(vrt_ctx* ctx, const void* full, void* packed, int32_t W, int32_t H,
                   int32_t bytes_per_px, const vrt_shard* shard, int32_t halo, int32_t dir);
int  vrt_unpack_halo(vrt_ctx* ctx, const void* packed, void* full, int32_t W, int32_t H,
                     int32_t bytes_per_px, const vrt_shard* shard, int32_t halo, int32_t dir);
size_t vrt_halo_bytes(int32_t W, int32_t H, int32_t bytes_per_px, const vrt_shard* shard, int32_t halo);
/* The halo rows of n images in one launch per 64 (the frames of a batch; shards[n]: each image's own strip assignment --
 * for unpack the SENDER's): one ring exchange per step then carries the colour, normal and position rows of every frame. */
int  vrt_pack_halo_batch(vrt_ctx* ctx, int32_t n, const void* const* full, void* const* packed, int32_t W, int32_t H,
                         int32_t bytes_per_px, const vrt_shard* shards, int32_t halo, int32_t dir);
int  vrt_unpack_halo_batch(vrt_ctx* ctx, int32_t n, const void* const* packed, void* const* full, int32_t W, int32_t H,
                           int32_t bytes_per_px, const vrt_shard* shards, int32_t halo, int32_t dir);

/* ---- the collective itself, for hosts without torch.distributed (no reference analogue; BASELINE north_star: "C++ host code
 * ... RCCL gather over xGMI") ---------------------------------------------------------------------------------------------
 * RCCL (librccl.so, found with dlopen at first use: the library the process already has -- torch's own copy in a Python
 * process -- or /opt/rocm's) behind plain C: one communicator rank per vrt_ctx.  Two ways to build the ranks:
 *   one process per GPU:        rank 0 calls vrt_comm_unique_id, hands the 128 bytes to the others out of band (a file, MPI,
 *                               a socket), every rank calls vrt_comm_init_rank;
 *   one process, several GPUs:  vrt_comm_init_all over the contexts (the C++ App: `vrt_app --devices 0,1,...`); calls that
 *                               belong to different ranks of one step are then wrapped in vrt_group_start / vrt_group_end.
 * vrt_gather_strips: every rank's `bytes` at `send` arrive at `recv + r * bytes` on `root` (the packed strips of vrt_pack_rows:
 * root unpacks them with vrt_unpack_rows and rank r's vrt_shard).  Enqueued on the context's stream; device pointers. */
typedef struct vrt_comm vrt_comm;
int  vrt_comm_unique_id(uint8_t id[128]);
int  vrt_comm_init_rank(vrt_ctx* ctx, int32_t nranks, int32_t rank, const uint8_t id[128], vrt_comm** out);
int  vrt_comm_init_all(int32_t n, vrt_ctx* const* ctxs, vrt_comm** out /* n handles */);
void vrt_comm_destroy(vrt_comm* comm);
int  vrt_group_start(void);
int  vrt_group_end(void);
int  vrt_gather_strips(vrt_ctx* ctx, vrt_comm* comm, int32_t root, const void* send, void* recv, size_t bytes);

/* ---- presentation / temporal helpers ----------------------------------- */
/* Replaces BlitStage::record + shader/blit.frag:14-22 (source/voxels/stages/blit_stage.cpp:41-75): the RGBA8 source
 * is centre-cropped to the target's aspect ratio and resampled with a linear, clamp-to-edge sampler
 * (render_image.cpp:61-66).  Also the plain upscale of a reduced-resolution render
 * (voxel_render_settings.cpp:3-13) that stands in for the FSR2 dispatch (upscaler_stage.cpp:72-161, out of scope).
 * Device pointers; runs on the context's stream. */
int  vrt_blit(vrt_ctx* ctx, const void* src_rgba8, int32_t src_w, int32_t src_h,
              void* dst_rgba8, int32_t dst_w, int32_t dst_h);

/* N-frame accumulation of jittered frames, the offline stand-in for FSR2's temporal pass: accum is W*H*4 uint32
 * (device), holding exact sums of the UNORM8 codes; reset != 0 starts a new sequence with this frame.
 * vrt_resolve writes the mean of `frames` accumulated frames, rounded half up: (2*sum + frames) / (2*frames). */
int  vrt_accumulate(vrt_ctx* ctx, const void* color_rgba8, void* accum_u32, int32_t W, int32_t H, int32_t reset);
int  vrt_resolve(vrt_ctx* ctx, const void* accum_u32, void* out_rgba8, int32_t W, int32_t H, uint32_t frames);

/* ---- temporal reprojection: history under a MOVING camera (no reference analogue: voxel_volume.frag:332 is a TODO, "use inverse
 * of camera matrix to reproject old position and calculate motion vectors", and the motion target stays 0) ------------------------
 * vrt_accumulate sums the frames pixel by pixel, which is right only while the camera stands still.  vrt_reproject finds, for every
 * pixel, where the surface it shows was on the previous frame's screen, fetches the history there (bilinear, four taps, weights in
 * 1/256), drops every tap that shows another surface -- the position plane is the world-space hit point and a voxel normal one of
 * a few codes, so the test is exact: same normal code, hit points within tol_abs + tol_rel * depth voxels of each other --
 * blends the current colour in, and writes the motion vectors.  csrc/vrt_reproject.h is the definition, step by step in fp32 and
 * integers; the GPU result equals it bit for bit.
 * A history is two planes of W * H texels (vrt_history_bytes): color16, 4 x uint16 per pixel, the accumulated colour in 8.8 fixed
 * point; surface, 4 x 32 bit per pixel, xyz = the world position the pixel shows, w = normal8.xyz | count << 24 with count in
 * 1..255 the number of frames accumulated (a miss pixel: position 0, normal bits 0, count 1). */
typedef struct vrt_history {
    uint16_t* color16;      /* DEVICE, 8-byte aligned  */
    uint32_t* surface;      /* DEVICE, 16-byte aligned */
} vrt_history;
typedef struct vrt_reproject_settings {
    uint32_t max_history;   /* 1..255: frames a pixel's history counts for at most (the blend weight of a new frame is >= 1/max); default 32 */
    float    tol_abs;       /* voxels, default 0.5 */
    float    tol_rel;       /* voxels per unit of depth, default 4 * |cam_right| / screen width: two pixel footprints */
} vrt_reproject_settings;
/* The defaults; tol_rel from cur->cam_right and cur->screen_size[0].  Needs no device. */
void vrt_reproject_settings_default(const vrt_push* cur, vrt_reproject_settings* s);
/* Bytes of the two planes of a W x H history (either pointer may be NULL).  Needs no device. */
int  vrt_history_bytes(int32_t W, int32_t H, size_t* color16, size_t* surface);
/* One frame of the sequence.  cur / prev: the push blocks this frame and the previous one were rendered with (their jitter is part
 * of the projection: motion vectors without jitter come from pushes whose camera_jitter is 0); settings NULL: the defaults.
 * color8 (RGBA8, normally the denoised image), position (RGBA32F) and normal8 (RGBA8_SNORM, w = 0) are the current frame's planes.
 * history_in: what the previous call wrote, NULL to start a new sequence (every pixel: count 1, resolved = colour).  history_out:
 * other buffers -- the kernel gathers, so in and out ping-pong.  resolved8 (RGBA8: the history rounded to codes) and motion (RG32F:
 * previous screen position minus current, in pixels, x right and y down; written for every hit whose point lies in front of the
 * previous camera, inside its frame or not; 0 for a miss) may each be NULL.  All DEVICE pointers, W * H texels, aligned to their
 * texel.  Asynchronous on the context's stream.  Frame-size limits of vrt_render_geometry.
 * VRT_ERR_INVALID, before any device work: a NULL required argument, max_history outside 1..255, a negative or non-finite
 * tolerance, a previous camera whose basis is degenerate (zero or non-finite determinant), an output that overlaps another buffer
 * of the call, a misaligned plane.
 * The history lives in VOLUME coordinates: it knows nothing of the scene's content.  After vrt_scene_edit_box the caller starts a
 * new sequence, or accepts that pixels whose geometry did not move keep their old lighting until the blend forgets it.
 * There is no vrt_shard here: reprojecting a strip needs history rows that other ranks own, which is out of scope -- sharded
 * renderers and the multi-GPU bench keep vrt_accumulate / vrt_resolve. */
int  vrt_reproject(vrt_ctx* ctx, int32_t W, int32_t H, const vrt_push* cur, const vrt_push* prev,
                   const vrt_reproject_settings* settings, const uint8_t* color8, const float* position, const int8_t* normal8,
                   const vrt_history* history_in, const vrt_history* history_out, uint8_t* resolved8, float* motion);

/* ---- temporal reprojection for ray cameras: vrt_reproject under the three models of vrt_camera_rays -------------------------------
 * vrt_reproject projects a hit point onto the previous screen through the push blocks' pinhole.  vrt_reproject_camera does it
 * through a vrt_ray_camera, so that frames drawn with vrt_camera_rays + vrt_render_rays keep a history; everything else -- the
 * history's format and vrt_history_bytes, the four taps and their exact surface test, the blend, the optional outputs, the
 * ping-pong of history_in / history_out, asynchrony, the frame-size limits -- is vrt_reproject's.  csrc/vrt_reproject_cam.h is
 * the definition, step by step in fp32; the GPU result equals it bit for bit.
 * The previous-screen position of a hit point P, d = P - prev->basis.cam_pos: PERSPECTIVE is vrt_reproject's projection over the
 * basis U = cam_right * tan_half, V = cam_up * tan_half * H / W, C = normalize(cam_dir) + jitter (with tan_half == 1.0f every
 * plane equals vrt_reproject's under the two bases, bit for bit); ORTHOGRAPHIC solves d = sx U + sy V + l cam_dir with U, V
 * scaled by half_width (no jitter) and keeps P if l > 0, the previous camera having seen only what lies in front of its plane;
 * PANORAMA is skyColor's mapping, u = atan(d.z, d.x) * 0.1591 + 0.5 and t = asin(-normalize(d).y) * 0.3183 + 0.5, at pixel
 * (u W - 0.5, t H - 0.5), for every finite d != 0.  The tap tolerance is tol_abs + tol_rel * |P - cur position| (perspective,
 * panorama) or tol_abs + tol_rel (orthographic: a parallel view's footprint does not grow with depth).
 * The panorama is periodic in x: a history tap at column -1 reads column W - 1, one at column W reads column 0 (and is dropped,
 * like any tap, if it shows another surface); rows are clipped.  Its motion is the plain difference of the two screen positions,
 * not taken the short way round: a surface that crossed the seam moves by almost +-W.
 * cur / prev: the cameras this frame and the previous one were drawn with, as given to vrt_camera_rays (the perspective model's
 * jitter included).  settings NULL: vrt_reproject_camera_settings_default(cur, W, ...).
 * VRT_ERR_INVALID, before any device work: every case of vrt_reproject; cur->model != prev->model; a camera vrt_camera_rays
 * would refuse (unknown model, a tan_half or half_width that is not finite and positive, a degenerate basis, a non-finite
 * position or jitter), current or previous.
 * There is no vrt_shard here, for the reason vrt_reproject gives.  vrt_upsample's counterpart is vrt_upsample_camera (below). */
int  vrt_reproject_camera(vrt_ctx* ctx, int32_t W, int32_t H, const vrt_ray_camera* cur, const vrt_ray_camera* prev,
                          const vrt_reproject_settings* settings, const uint8_t* color8, const float* position,
                          const int8_t* normal8, const vrt_history* history_in, const vrt_history* history_out,
                          uint8_t* resolved8, float* motion);
/* The defaults for camera `cur` and a frame W pixels wide: max_history 32, tol_abs 0.5, tol_rel two pixel footprints -- perspective
 * 4 |cam_right| tan_half / W per unit of depth, orthographic 4 |cam_right| half_width / W voxels, panorama 2 / (0.1591 W) per unit
 * of depth; 0 for a camera vrt_camera_rays would refuse.  Needs no device. */
void vrt_reproject_camera_settings_default(const vrt_ray_camera* cur, int32_t W, vrt_reproject_settings* s);

/* ---- temporal upsampling: a DISPLAY-resolution history from jittered render-resolution frames (the part of the FSR2 dispatch,
 * upscaler_stage.cpp:72-161, that the jitter sequence exists for; the library itself stays out of scope) -----------------------
 * vrt_reproject keeps its history at render resolution, and the step to the display is one bilinear vrt_blit of it.  vrt_upsample
 * keeps the history, and writes its outputs, at TW x TH >= w x h: for every display pixel it takes the sample of the render
 * pixel under it, finds where that sample really fell on the display grid -- its hit point projected through the UNJITTERED
 * current camera, because the reference adds the jitter to the ray in world x / y (voxel_volume.frag:319) -- and weighs it by a
 * tent of one display pixel; the history is fetched where the surface was under the unjittered previous camera, with the taps and
 * the tap test of vrt_reproject, and blended with that weight.  A pixel no sample of this frame fell on carries its history on:
 * blended with weight 0, or -- where the far sample it was given matches no tap -- the nearest history texel copied whole.
 * csrc/vrt_upsample.h is the definition, step by step in fp32 and integers; the GPU result equals it bit for bit.
 * w, h: the size of color8 / position / normal8, the current frame's planes; cur->screen_size and prev->screen_size must both be
 * (w, h).  TW, TH: the size of both histories (the format of vrt_reproject; vrt_history_bytes(TW, TH, ...) sizes them), of
 * resolved8 and of motion.  settings: vrt_reproject's; NULL: vrt_reproject_settings_default(cur, ...), whose tol_rel is then two
 * RENDER-pixel footprints.  history_in NULL starts a new sequence (every pixel: count 1, resolved = its render pixel's colour, what
 * a nearest-sample blit shows); history_out: other buffers.  resolved8 (RGBA8) and motion (RG32F, in DISPLAY pixels: where the
 * surface was minus where it is, both without jitter; 0 for a miss and for a point not in front of the previous camera) may each
 * be NULL.  All DEVICE pointers, aligned to their texel.  Asynchronous on the context's stream.  The frame-size limits of
 * vrt_render_geometry apply to TW x TH.
 * VRT_ERR_INVALID, before any device work: a NULL required argument, TW < w or TH < h, a push block whose screen_size is not
 * (w, h), max_history outside 1..255, a negative or non-finite tolerance, a current or previous camera whose basis is degenerate
 * (zero or non-finite determinant), a misaligned plane, an output that overlaps another buffer of the call.
 * Sky pixels keep no history (a miss shows its nearest sample); after vrt_scene_edit_box the caller decides as for vrt_reproject.
 * There is no vrt_shard here, for the reason vrt_reproject gives. */
int  vrt_upsample(vrt_ctx* ctx, int32_t w, int32_t h, int32_t TW, int32_t TH, const vrt_push* cur, const vrt_push* prev,
                  const vrt_reproject_settings* settings, const uint8_t* color8, const float* position, const int8_t* normal8,
                  const vrt_history* history_in, const vrt_history* history_out, uint8_t* resolved8, float* motion);

/* ---- temporal upsampling for ray cameras: vrt_upsample under the three models of vrt_camera_rays ------------------------------------
 * vrt_upsample finds where a sample fell, and where its surface was, through the push blocks' pinhole.  vrt_upsample_camera does
 * both through a vrt_ray_camera, so that frames drawn at w x h with vrt_camera_rays_offset (or a jittered perspective camera) +
 * vrt_render_rays feed a history at TW x TH; everything else -- the render pixel under a display pixel, the miss rule, the tent in
 * 1/256, the four taps and their exact surface test, the blend, the carry of a pixel no sample fell on, the history's format, the
 * optional outputs, the ping-pong, asynchrony, the size limits -- is vrt_upsample's.  csrc/vrt_upsample_cam.h is the definition,
 * step by step in fp32 and integers; the GPU result equals it bit for bit.
 * cur / prev: the cameras of this frame and the previous one WITHOUT sample offset; the perspective model's camera_jitter is not
 * read (it must be finite).  Both projections, of a hit point P with d = P - cam_pos onto the TW x TH grid: PERSPECTIVE is
 * vrt_upsample's over the basis U = cam_right * tan_half, V = cam_up * tan_half * h / w, C = normalize(cam_dir) (with
 * tan_half == 1.0f every plane equals vrt_upsample's, bit for bit); ORTHOGRAPHIC solves d = sx U + sy V + l cam_dir with U, V
 * scaled by half_width; both keep P when the product d . (U x V) is finite, non-zero and has the sign of the determinant
 * U . (V x C) -- P lies in front of the camera --, as csrc/vrt_upsample_cam.h tests it; PANORAMA is skyColor's mapping at display pixel (u TW - 0.5, t TH - 0.5) for every
 * finite d != 0, as in vrt_reproject_camera.  The tap tolerance is tol_abs + tol_rel * |P - cur position| (perspective, panorama)
 * or tol_abs + tol_rel (orthographic).
 * The panorama is periodic in x over TW display pixels: the tent's x distance is taken the short way round (a sample pushed left
 * of column 0 counts for column TW - 1 and the reverse), the history is fetched at X + motion brought back by one period into
 * [-0.5, TW - 0.5), and tap columns -1 and TW read columns TW - 1 and 0; rows are clipped.  Its motion is the plain difference of
 * the two display positions, not taken the short way round.
 * settings NULL: vrt_upsample_camera_settings_default(cur, w, ...), which is vrt_reproject_camera_settings_default at the RENDER
 * width: tol_rel is two render-pixel footprints.
 * VRT_ERR_INVALID, before any device work: every case of vrt_upsample but the push blocks' screen_size; cur->model != prev->model;
 * a camera vrt_camera_rays would refuse at (w, h), current or previous; a current or previous basis whose fp32 determinant is zero
 * or not finite (perspective, orthographic).  VRT_ERR_UNSUPPORTED: TW * TH >= 2^28.
 * Sky pixels keep no history; there is no vrt_shard here, for the reason vrt_reproject gives. */
int  vrt_upsample_camera(struct vrt_ctx* ctx, int32_t w, int32_t h, int32_t TW, int32_t TH, const vrt_ray_camera* cur,
                         const vrt_ray_camera* prev, const vrt_reproject_settings* settings, const uint8_t* color8,
                         const float* position, const int8_t* normal8, const vrt_history* history_in,
                         const vrt_history* history_out, uint8_t* resolved8, float* motion);
void vrt_upsample_camera_settings_default(const vrt_ray_camera* cur, int32_t w, vrt_reproject_settings* s);

/* Replace ffxFsr2GetJitterPhaseCount / ffxFsr2GetJitterOffset as called by UpscalerStage::update
 * (source/voxels/stages/upscaler_stage.cpp:59-70): phase count int(8 * (display_width / render_width)^2);
 * offset = Halton(2,3)(index % phase_count + 1) - 0.5, in pixels; feeds vrt_push.camera_jitter. */
int32_t vrt_jitter_phase_count(int32_t render_width, int32_t display_width);
int  vrt_jitter_offset(int32_t index, int32_t phase_count, float* jitter_x, float* jitter_y);

/* ---- instrumentation ------------------------------------------------------------------------- */
/* Time of the most recent vrt_render_geometry primary-ray kernel / all its kernels, and of the most
 * recent vrt_denoise, in milliseconds (HIP events on the context stream; blocks until they complete). */
int  vrt_last_timings(vrt_ctx* ctx, float* primary_ms, float* geometry_ms, float* denoise_ms);
/* Diagnostic of the sky-texel fast path (csrc/vrt_sky.h; skyColor, voxel_volume.frag:98-105): for n unnormalised
 * directions (device floats, xyz per direction) the texel skyColor(normalize(v)) reads under the numeric spec and the
 * one the fast path decides, both computed by the GPU: out[4i] = spec x | y << 16, out[4i+1] = fast x | y << 16,
 * out[4i+2] = 1 if the fast path is sure of its texel (only then may the two be compared), out[4i+3] = float bits of the
 * fast coordinate u * sky_w.  tests/test_gpu_sky.py sweeps it over 10^8 directions. */
int  vrt_debug_sky_texels(vrt_ctx* ctx, const vrt_scene* scene, const float* dirs_dev, size_t n, uint32_t* out_dev);
/* Diagnostic of the numeric spec on the device (csrc/vrt_spec.h): evaluates ONE primitive per element, bit patterns
 * in and bit patterns out, so that nothing is rounded on the way.  a_dev, b_dev, c_dev: n device words each (a float's bits; for
 * VRT_SPEC_WRAP_TEXEL b holds the texture size n as a uint32); out_dev: n device words, 3 n for VRT_SPEC_NORMALIZE3 (x, y, z per
 * element).  Element i is evaluated by lane i of the launch (256 lanes a workgroup): elements 64 k .. 64 k + 63 share a wave.
 *   fn  evaluates              reads      writes per element
 *   0   sqrt_spec(a)           a          the result's bits
 *   1   div_spec(a, b)         a, b       the result's bits
 *   2   atan2_spec(a, b)       a = y, b = x   the result's bits
 *   3   asin_spec(a)           a          the result's bits
 *   4   exp_spec(a)            a          the result's bits
 *   5   unorm8(a)              a          0 .. 255
 *   6   snorm8(a)              a          -127 .. 127, sign-extended to 32 bits
 *   7   wrap_texel(a, b)       a, b       the texel index
 *   8   normalize3(a, b, c)    a, b, c    three words
 * An array fn does not read may be NULL.  VRT_ERR_INVALID: an unknown fn, a NULL ctx, out_dev or array that fn reads; n == 0 with
 * valid pointers does nothing and succeeds; VRT_ERR_UNSUPPORTED: n > 2^31.  The kernel pins the header under the library's compiler
 * flags in a unit of its own; the copies inlined into the render and denoise kernels stay pinned by the frame tests.
 * tests/test_gpu_spec.py holds it to the oracle on every bit pattern of the one-argument primitives. */
#define VRT_SPEC_SQRT        0u
#define VRT_SPEC_DIV         1u
#define VRT_SPEC_ATAN2       2u
#define VRT_SPEC_ASIN        3u
#define VRT_SPEC_EXP         4u
#define VRT_SPEC_UNORM8      5u
#define VRT_SPEC_SNORM8      6u
#define VRT_SPEC_WRAP_TEXEL  7u
#define VRT_SPEC_NORMALIZE3  8u
int  vrt_debug_spec(vrt_ctx* ctx, uint32_t fn, const uint32_t* a_dev, const uint32_t* b_dev, const uint32_t* c_dev, size_t n, uint32_t* out_dev);
/* Development builds only (make variant EXTRA=-DVRT_TRACE_COUNTERS; the product library answers zeros): look-ups of the brick
 * march since the last call, summed over the lanes of all rays -- all, those inside an occupied brick (the second, dependent
 * load), those that found a solid voxel, those that ended in the border or an open brick.  Waits for the stream; resets. */
int  vrt_debug_brick_counts(vrt_ctx* ctx, uint64_t out[4]);
/* Enable/disable per-call event recording (default on). */
int  vrt_ctx_set_timing(vrt_ctx* ctx, int enabled);

#ifdef __cplusplus
}
#endif
#endif /* VRT_H */
