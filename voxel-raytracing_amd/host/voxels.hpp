// voxels.hpp -- C++17 host side above the C-ABI (include/vrt.h), mirroring the reference's object surface for
// the hot path: same class names, member names, argument meaning and error behaviour (std::runtime_error with
// the reference's messages).  Header-only; link with libvrt_hip.so.  No Vulkan, no HIP headers needed.
//
//   VoxelRenderSettings (+Fsr/Denoiser/AmbientOcclusion/LightSettings)  source/voxels/voxel_render_settings.hpp:6-59
//   CameraController                                                   source/voxels/resource/camera_controller.cpp:15-44
//   VoxelScene                                                         source/voxels/resource/voxel_scene.hpp:18-34
//   GeometryBuffer / GeometryStage                                     source/voxels/stages/geometry_stage.hpp:19-53
//   DenoiserStage                                                      source/voxels/stages/denoiser_stage.hpp:22-47
//   VoxelRenderer                                                      source/voxels/voxel_renderer.hpp:17-38
//   Engine                                                             source/engine/engine.hpp:71-76 (device + stream only)
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/vrt.h"

namespace vrt_host {

inline void check(int rc)
{
    if (rc != VRT_OK) throw std::runtime_error(vrt_last_error());
}

struct vec3 { float x = 0, y = 0, z = 0; };
inline vec3 operator+(vec3 a, vec3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline vec3 operator*(vec3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
inline vec3 cross(vec3 a, vec3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline vec3 normalize(vec3 a) { float l = std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z); return {a.x / l, a.y / l, a.z / l}; }

// ---- settings (voxel_render_settings.hpp) -------------------------------------------------------------
enum class FsrScaling : uint32_t { NONE = 10, QUALITY = 15, BALANCED = 17, PERFORMANCE = 20, ULTRA_PERFORMANCE = 30 };
struct FsrSettings { bool enable = true; FsrScaling scaling = FsrScaling::BALANCED; };
struct DenoiserSettings {
    bool enable = true; int iterations = 2; float phiColor0 = 20.4f; float phiNormal0 = 1E-2f; float phiPos0 = 1E-1f;
    float stepWidth = 2.0f; int mode = VRT_DENOISE_CANONICAL;
};
struct AmbientOcclusionSettings { int numSamples = 4; float intensity = 1.0f; };
struct LightSettings { vec3 direction = normalize({1.0f, 1.0f, 1.0f}); std::array<float, 4> color{1, 1, 1, 1}; float intensity = 1.0f; };
struct TraceSettings {   // voxel_volume.frag:68-69,219 promoted to runtime knobs
    uint32_t maxRaySteps = 512, aoSteps = 64, maxReflections = 5; bool shadows = true; uint32_t traversal = VRT_TRAVERSAL_AUTO;
};

class VoxelRenderSettings {
public:
    std::array<uint32_t, 2> targetResolution{1920, 1080};
    FsrSettings fsrSetttings{};            // (sic)
    DenoiserSettings denoiserSettings{};
    AmbientOcclusionSettings occlusionSettings{};
    LightSettings lightSettings{};
    TraceSettings traceSettings{};
    std::string voxPath = "../resource/treehouse.vox";
    std::string skyboxPath = "../resource/rustig_koppie.hdr";

    std::array<uint32_t, 2> renderResolution() const     // voxel_render_settings.cpp:3-13
    {
        if (!fsrSetttings.enable) return targetResolution;
        auto scale = [&](uint32_t dim) { return static_cast<uint32_t>((10.0f / static_cast<uint32_t>(fsrSetttings.scaling)) * dim); };
        return {scale(targetResolution[0]), scale(targetResolution[1])};
    }
    vrt_settings toC() const                             // geometry_stage.cpp:135-145
    {
        vrt_settings s{};
        s.ao_samples = (uint32_t)occlusionSettings.numSamples; s.ambient_intensity = occlusionSettings.intensity;
        s.light_dir[0] = lightSettings.direction.x; s.light_dir[1] = lightSettings.direction.y; s.light_dir[2] = lightSettings.direction.z;
        s.light_intensity = lightSettings.intensity;
        for (int i = 0; i < 4; i++) s.light_color[i] = lightSettings.color[i];
        s.max_steps = traceSettings.maxRaySteps; s.ao_steps = traceSettings.aoSteps; s.max_bounces = traceSettings.maxReflections;
        s.shadows = traceSettings.shadows ? 1u : 0u; s.traversal = traceSettings.traversal; s.flags = 0;
        return s;
    }
    vrt_denoiser_settings denoiserToC() const
    {
        return {denoiserSettings.iterations, denoiserSettings.phiColor0, denoiserSettings.phiNormal0, denoiserSettings.phiPos0,
                denoiserSettings.stepWidth, denoiserSettings.mode};
    }
};

// ---- camera (camera_controller.cpp) -------------------------------------------------------------------
class CameraController {
public:
    vec3 position, direction, right, up, normalDir;
    float yaw, pitch, focalLength;
    explicit CameraController(vec3 position = {8, 8, -50}, float yaw = 90.0f, float pitch = 0.0f,
                              float focalLength = static_cast<float>(1 / std::tan((55.0 / 2) * 3.14159265358979323846 / 180)))
        : position(position), yaw(yaw), pitch(pitch), focalLength(focalLength) { updateDirectionVectors(); }
    void updateDirectionVectors()                         // :15-28
    {
        const vec3 worldUp{0.0f, -1.0f, 0.0f};
        const float ry = yaw * 0.01745329251994329576923690768489f, rp = pitch * 0.01745329251994329576923690768489f;
        normalDir = normalize({std::cos(ry) * std::cos(rp), std::sin(rp), std::sin(ry) * std::cos(rp)});
        right = normalize(cross(normalDir, worldUp));
        up = normalize(cross(right, normalDir));
        direction = normalDir * focalLength;
    }
    void update(float delta, float forward = 0.0f, float strafe = 0.0f)   // :30-44, keys replaced by scripted axes
    {
        const float cameraSpeed = 50.0f;
        position = position + normalDir * (cameraSpeed * delta * forward) + right * (cameraSpeed * delta * strafe);
        updateDirectionVectors();
    }
    void mouse(float offsetX, float offsetY)                              // :46-68 with the right button held
    {
        yaw -= offsetX;
        pitch = std::min(std::max(pitch - offsetY, -90.0f), 90.0f);
        updateDirectionVectors();
    }
};

// ---- engine -------------------------------------------------------------------------------------------
class Engine {
public:
    explicit Engine(int device = 0) { check(vrt_ctx_create(device, &ctx)); }
    ~Engine() { vrt_ctx_destroy(ctx); }
    Engine(const Engine&) = delete; Engine& operator=(const Engine&) = delete;
    void waitIdle() { check(vrt_ctx_synchronize(ctx)); }
    vrt_ctx* ctx = nullptr;
};

template <class T> class DeviceBuffer {                   // Buffer / RenderImage storage (engine/resource/buffer.hpp)
public:
    DeviceBuffer(const std::shared_ptr<Engine>& e, size_t count) : engine(e), count(count)
    {
        void* p = nullptr; check(vrt_device_alloc(e->ctx, count * sizeof(T), &p)); ptr = static_cast<T*>(p);
        check(vrt_memset(e->ctx, ptr, 0, count * sizeof(T)));
    }
    ~DeviceBuffer() { vrt_device_free(engine->ctx, ptr); }
    DeviceBuffer(const DeviceBuffer&) = delete; DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    std::vector<T> download() const { std::vector<T> h(count); check(vrt_memcpy_d2h(engine->ctx, h.data(), ptr, count * sizeof(T))); return h; }
private:
    std::shared_ptr<Engine> engine;
public:
    size_t count;
    T* ptr = nullptr;
};

// ---- scene --------------------------------------------------------------------------------------------
class VoxelScene {
public:
    uint32_t width = 0, height = 0, depth = 0;
    VoxelScene(const std::shared_ptr<Engine>& engine, const std::string& filename, const std::string& skyboxFilename = "")
        : engine(engine)                                                                              // voxel_scene.cpp:33
    {
        check(vrt_scene_load_vox_file(engine->ctx, filename.c_str(), &handle)); dims();
        if (!skyboxFilename.empty()) setSkybox(skyboxFilename);                                       // :132
    }
    VoxelScene(const std::shared_ptr<Engine>& engine, const uint8_t* voxels, uint32_t W, uint32_t H, uint32_t D, const vrt_material* palette)
        : engine(engine) { check(vrt_scene_from_dense(engine->ctx, voxels, W, H, D, palette, &handle)); dims(); }
    ~VoxelScene() { vrt_scene_free(engine->ctx, handle); }
    VoxelScene(const VoxelScene&) = delete; VoxelScene& operator=(const VoxelScene&) = delete;
    // Rewrite the box [lo, lo + size) (no reference analogue; vrt_scene_edit_box / vrt_scene_fill_box): ids x-fastest, 0 = empty
    void edit(const std::array<int32_t, 3>& lo, const std::array<uint32_t, 3>& size, const uint8_t* ids) { check(vrt_scene_edit_box(engine->ctx, handle, lo.data(), size.data(), ids)); }
    void fill(const std::array<int32_t, 3>& lo, const std::array<uint32_t, 3>& size, uint8_t id) { check(vrt_scene_fill_box(engine->ctx, handle, lo.data(), size.data(), id)); }
    // Brushes and stamps (no reference analogue; vrt_scene_brush / vrt_scene_stamp): an edit composed on the device, rebuilt around
    // the tight box of what changed, which is what they return (changed == 0: nothing was written).  brush takes the C structure;
    // the helpers take voxel units that are multiples of 0.5 -- voxel (x, y, z) has its centre at (x + .5, y + .5, z + .5) -- and
    // refuse anything else.  mode: VRT_BRUSH_SET, _PAINT, _ADD, _REPLACE.  A shape partly outside the volume is clipped.
    vrt_brush_result brush(const vrt_brush& b) { vrt_brush_result r{}; check(vrt_scene_brush(engine->ctx, handle, &b, &r)); return r; }
    static int32_t halfVoxels(double v)
    {
        const double h = 2.0 * v;
        if (!(h >= -2147483648.0 && h <= 2147483647.0) || h != (double)(int64_t)h) throw std::runtime_error("a brush position must be a multiple of 0.5 voxels");
        return (int32_t)h;
    }
    vrt_brush_result box(const std::array<int32_t, 3>& lo, const std::array<int32_t, 3>& size, uint8_t id, int32_t mode = VRT_BRUSH_SET, uint8_t match = 0)
    {
        vrt_brush b{}; b.shape = VRT_BRUSH_BOX; b.mode = mode; b.id = id; b.match = match;
        for (size_t a = 0; a < 3; a++) { b.p[a] = lo[a]; b.p[3 + a] = size[a]; }
        return brush(b);
    }
    vrt_brush_result ellipsoid(const std::array<double, 3>& center, const std::array<double, 3>& radii, uint8_t id, int32_t mode = VRT_BRUSH_SET, uint8_t match = 0)
    {
        vrt_brush b{}; b.shape = VRT_BRUSH_ELLIPSOID; b.mode = mode; b.id = id; b.match = match;
        for (size_t a = 0; a < 3; a++) { b.p[a] = halfVoxels(center[a]); b.p[3 + a] = halfVoxels(radii[a]); }
        return brush(b);
    }
    vrt_brush_result sphere(const std::array<double, 3>& center, double radius, uint8_t id, int32_t mode = VRT_BRUSH_SET, uint8_t match = 0)
    {
        return ellipsoid(center, {radius, radius, radius}, id, mode, match);
    }
    vrt_brush_result capsule(const std::array<double, 3>& a0, const std::array<double, 3>& b0, double radius, uint8_t id, int32_t mode = VRT_BRUSH_SET, uint8_t match = 0)
    {
        vrt_brush b{}; b.shape = VRT_BRUSH_CAPSULE; b.mode = mode; b.id = id; b.match = match;
        for (size_t a = 0; a < 3; a++) { b.p[a] = halfVoxels(a0[a]); b.p[3 + a] = halfVoxels(b0[a]); }
        b.p[6] = halfVoxels(radius);
        return brush(b);
    }
    // the box [srcLo, srcLo + size) of src (which may be this scene) pasted at dstLo under orient = perm | flips << 3
    vrt_brush_result stamp(const std::array<int32_t, 3>& dstLo, const VoxelScene& src, const std::array<int32_t, 3>& srcLo, const std::array<uint32_t, 3>& size,
                           uint32_t orient = 0, bool skipEmpty = false)
    {
        vrt_brush_result r{};
        check(vrt_scene_stamp(engine->ctx, handle, dstLo.data(), src.handle, srcLo.data(), size.data(), orient, skipEmpty ? VRT_STAMP_SKIP_EMPTY : 0u, &r));
        return r;
    }
    // Flood fills (no reference analogue; vrt_scene_flood): every voxel connected to `seed` becomes `id`.  match VRT_FLOOD_SAME (the
    // seed's id, 0 included) | VRT_FLOOD_SOLID; connectivity VRT_FLOOD_FACES | VRT_FLOOD_CORNERS; the search stays in [lo, lo + size),
    // without bounds in the whole volume.  flood takes the C structure; region measures and writes nothing (VRT_FLOOD_MEASURE).
    vrt_flood_result flood(const vrt_flood& f) { vrt_flood_result r{}; check(vrt_scene_flood(engine->ctx, handle, &f, &r)); return r; }
    vrt_flood floodOf(const std::array<int32_t, 3>& seed, uint8_t id, int32_t match, int32_t connectivity, uint32_t flags) const
    {
        vrt_flood f{};
        for (size_t a = 0; a < 3; a++) f.seed[a] = seed[a];
        f.size[0] = width; f.size[1] = height; f.size[2] = depth;
        f.match = match; f.connectivity = connectivity; f.flags = flags; f.id = id;
        return f;
    }
    vrt_flood_result flood(const std::array<int32_t, 3>& seed, uint8_t id, int32_t match = VRT_FLOOD_SAME, int32_t connectivity = VRT_FLOOD_FACES)
    {
        return flood(floodOf(seed, id, match, connectivity, 0u));
    }
    vrt_flood_result flood(const std::array<int32_t, 3>& seed, uint8_t id, int32_t match, int32_t connectivity, const std::array<int32_t, 3>& lo,
                           const std::array<uint32_t, 3>& size)
    {
        vrt_flood f = floodOf(seed, id, match, connectivity, 0u);
        for (size_t a = 0; a < 3; a++) { f.lo[a] = lo[a]; f.size[a] = size[a]; }
        return flood(f);
    }
    vrt_flood_result region(const std::array<int32_t, 3>& seed, int32_t match = VRT_FLOOD_SAME, int32_t connectivity = VRT_FLOOD_FACES)
    {
        return flood(floodOf(seed, 0, match, connectivity, VRT_FLOOD_MEASURE));
    }
    vrt_flood_result region(const std::array<int32_t, 3>& seed, int32_t match, int32_t connectivity, const std::array<int32_t, 3>& lo, const std::array<uint32_t, 3>& size)
    {
        vrt_flood f = floodOf(seed, 0, match, connectivity, VRT_FLOOD_MEASURE);
        for (size_t a = 0; a < 3; a++) { f.lo[a] = lo[a]; f.size[a] = size[a]; }
        return flood(f);
    }
    // Mesh voxelization (no reference analogue; vrt_scene_voxelize): a triangle mesh composed into the scene.  vertices: three int32
    // per vertex in SIXTEENTHS of a voxel (meshUnits converts a position in voxels: nearest, ties to even, of float(v) * 16);
    // triangles: three indices each.  fill VRT_VOXELIZE_SURFACE | VRT_VOXELIZE_SOLID, mode VRT_BRUSH_*; without bounds the mesh's own.
    static int32_t meshUnits(float voxels) { return (int32_t)std::nearbyintf(voxels * 16.0f); }
    vrt_voxelize_result voxelize(const std::vector<int32_t>& vertices, const std::vector<uint32_t>& triangles, const vrt_voxelize& job)
    {
        vrt_voxelize_result r{};
        check(vrt_scene_voxelize(engine->ctx, handle, vertices.data(), (uint32_t)(vertices.size() / 3), triangles.data(), (uint32_t)(triangles.size() / 3), &job, &r));
        return r;
    }
    vrt_voxelize_result voxelize(const std::vector<int32_t>& vertices, const std::vector<uint32_t>& triangles, uint8_t id, uint32_t fill = VRT_VOXELIZE_SURFACE,
                                 int32_t mode = VRT_BRUSH_SET, uint8_t match = 0)
    {
        vrt_voxelize job{};
        job.mode = mode; job.fill = fill; job.id = id; job.match = match;
        for (size_t a = 0; a < 3 && vertices.size() >= 3; a++) {      // the voxels whose closed cube [16x, 16x+16] the vertices can touch
            int32_t m = vertices[a], M = vertices[a];
            for (size_t i = a; i < vertices.size(); i += 3) { m = std::min(m, vertices[i]); M = std::max(M, vertices[i]); }
            const int32_t lo = (m + 15 >= 0 ? (m + 15) / 16 : -((-m) / 16)) - 1, hi = M >= 0 ? M / 16 : -((15 - M) / 16);
            job.lo[a] = lo; job.size[a] = (uint32_t)(hi - lo + 1);
        }
        return voxelize(vertices, triangles, job);
    }
    // Morphology (no reference analogue; vrt_scene_morph): grow, shrink, open, close or hollow the scene's solid by the ball of `radius`
    // (1..8) of connectivity VRT_MORPH_FACES | VRT_MORPH_CORNERS; an added voxel becomes `id` (DILATE and CLOSE need one), none is
    // recoloured; flags VRT_MORPH_BORDER_SOLID | VRT_MORPH_MEASURE; without bounds the whole volume.
    vrt_morph_result morph(const vrt_morph& m) { vrt_morph_result r{}; check(vrt_scene_morph(engine->ctx, handle, &m, &r)); return r; }
    vrt_morph_result morph(int32_t op, int32_t radius, int32_t connectivity = VRT_MORPH_FACES, uint8_t id = 0, uint32_t flags = 0u)
    {
        vrt_morph m{};
        m.op = op; m.connectivity = connectivity; m.radius = radius; m.flags = flags; m.id = id;
        m.size[0] = width; m.size[1] = height; m.size[2] = depth;
        return morph(m);
    }
    vrt_morph_result morph(int32_t op, int32_t radius, int32_t connectivity, uint8_t id, uint32_t flags, const std::array<int32_t, 3>& lo, const std::array<uint32_t, 3>& size)
    {
        vrt_morph m{};
        m.op = op; m.connectivity = connectivity; m.radius = radius; m.flags = flags; m.id = id;
        for (size_t a = 0; a < 3; a++) { m.lo[a] = lo[a]; m.size[a] = size[a]; }
        return morph(m);
    }
    // Connected components (no reference analogue; vrt_scene_components, vrt_scene_component_labels, vrt_scene_filter_components): every
    // component of the bounds at once -- match VRT_COMP_SOLID | VRT_COMP_SAME | VRT_COMP_EMPTY, connectivity VRT_COMP_FACES |
    // VRT_COMP_CORNERS -- as records in ascending order of their roots; labels: the component number of every voxel of a box inside the
    // latest labelling's bounds (0xFFFFFFFF: does not pass), x fastest; filter: every voxel of a selected component becomes f.id.
    std::vector<vrt_component> components(const vrt_components& q, vrt_components_result* result = nullptr)
    {
        vrt_components_result r{};
        check(vrt_scene_components(engine->ctx, handle, &q, nullptr, 0, &r));
        std::vector<vrt_component> rec((size_t)r.components);
        if (!rec.empty()) check(vrt_scene_components(engine->ctx, handle, &q, rec.data(), rec.size(), &r));
        if (result) *result = r;
        return rec;
    }
    std::vector<vrt_component> components(int32_t match = VRT_COMP_SOLID, int32_t connectivity = VRT_COMP_FACES, vrt_components_result* result = nullptr)
    {
        return components(wholeVolume(match, connectivity), result);
    }
    std::vector<uint32_t> labels(const std::array<int32_t, 3>& lo, const std::array<uint32_t, 3>& size)
    {
        std::vector<uint32_t> out((size_t)size[0] * size[1] * size[2]);
        check(vrt_scene_component_labels(engine->ctx, handle, lo.data(), size.data(), out.data()));
        return out;
    }
    vrt_filter_result filterComponents(const vrt_components& q, const vrt_component_filter& f)
    {
        vrt_filter_result r{};
        check(vrt_scene_filter_components(engine->ctx, handle, &q, &f, &r));
        return r;
    }
    // delete every solid component below minVoxels voxels | every region of air that touches no face of the volume becomes id | delete
    // every solid component but the largest
    vrt_filter_result despeckle(uint64_t minVoxels, int32_t connectivity = VRT_COMP_FACES)
    {
        vrt_component_filter f{};
        f.max_voxels = minVoxels ? minVoxels - 1u : 0u;
        return filterComponents(wholeVolume(VRT_COMP_SOLID, connectivity), f);
    }
    vrt_filter_result fillCavities(uint8_t id, int32_t connectivity = VRT_COMP_FACES)
    {
        vrt_component_filter f{};
        f.max_voxels = ~0ull; f.faces_none = 63u; f.id = id;
        return filterComponents(wholeVolume(VRT_COMP_EMPTY, connectivity), f);
    }
    vrt_filter_result keepLargest(int32_t connectivity = VRT_COMP_FACES)
    {
        vrt_component_filter f{};
        f.max_voxels = ~0ull; f.flags = VRT_COMP_KEEP_LARGEST;
        return filterComponents(wholeVolume(VRT_COMP_SOLID, connectivity), f);
    }
    vrt_components wholeVolume(int32_t match, int32_t connectivity) const
    {
        vrt_components q{};
        q.match = match; q.connectivity = connectivity;
        q.size[0] = width; q.size[1] = height; q.size[2] = depth;
        return q;
    }
    // A brick scene becomes editable, with room for `capacity` bricks in its pool (vrt_scene_reserve_bricks); edit / fill then work on it
    // Read-back (no reference analogue; vrt_scene_read_box / vrt_scene_list_box / vrt_scene_save_vox_file).  read: the ids of the
    // box [lo, lo + size), x fastest -- what edit takes.  voxels: the box's non-empty voxels (no side above 256), one word each,
    // x | y << 8 | z << 16 | id << 24 relative to lo, in ascending order of x + y * size[0] + z * size[0] * size[1].  save: the scene
    // as it stands as a MagicaVoxel file (a palette that did not come from bytes is quantised).
    std::vector<uint8_t> read(const std::array<int32_t, 3>& lo, const std::array<uint32_t, 3>& size) const
    {
        std::vector<uint8_t> ids((size_t)size[0] * size[1] * size[2]);
        check(vrt_scene_read_box(engine->ctx, handle, lo.data(), size.data(), ids.data()));
        return ids;
    }
    std::vector<uint32_t> voxels(const std::array<int32_t, 3>& lo, const std::array<uint32_t, 3>& size) const
    {
        uint64_t n = 0;
        check(vrt_scene_list_box(engine->ctx, handle, lo.data(), size.data(), nullptr, 0, &n));
        std::vector<uint32_t> rec((size_t)n);
        if (n) check(vrt_scene_list_box(engine->ctx, handle, lo.data(), size.data(), rec.data(), n, &n));
        return rec;
    }
    void save(const std::string& path) const { check(vrt_scene_save_vox_file(engine->ctx, handle, path.c_str())); }
    // Surface extraction (vrt_scene_list_faces / vrt_scene_save_obj_file; include/vrt.h has the record and the order).  faces: the
    // exposed faces of a box (no side above 256) as records, flags = VRT_FACES_RUNS | VRT_FACES_CLOSED; counts (if given): records
    // per direction.  saveObj: the whole surface as a Wavefront OBJ of quads and, beside it, its .mtl.
    std::vector<uint64_t> faces(const std::array<int32_t, 3>& lo, const std::array<uint32_t, 3>& size, uint32_t flags = VRT_FACES_RUNS,
                                std::array<uint64_t, 6>* counts = nullptr) const
    {
        std::array<uint64_t, 6> c{};
        check(vrt_scene_list_faces(engine->ctx, handle, lo.data(), size.data(), flags, nullptr, 0, c.data()));
        uint64_t n = 0;
        for (const uint64_t k : c) n += k;
        std::vector<uint64_t> rec((size_t)n);
        if (n) check(vrt_scene_list_faces(engine->ctx, handle, lo.data(), size.data(), flags, rec.data(), n, c.data()));
        if (counts) *counts = c;
        return rec;
    }
    void saveObj(const std::string& path, bool runs = true) const { check(vrt_scene_save_obj_file(engine->ctx, handle, path.c_str(), runs ? VRT_FACES_RUNS : 0u)); }
    void reserveBricks(uint32_t capacity) { check(vrt_scene_reserve_bricks(engine->ctx, handle, capacity)); }
    void setSkybox(const float* rgba, uint32_t w, uint32_t h) { check(vrt_scene_set_sky(engine->ctx, handle, rgba, w, h)); }
    void setSkybox(const std::string& path) { check(vrt_scene_set_sky_file(engine->ctx, handle, path.c_str())); }          // Texture2D(.hdr)
    void setBlueNoise(const std::string& path) { check(vrt_scene_set_blue_noise_file(engine->ctx, handle, path.c_str())); }   // Texture2D(.png)
    void setBlueNoise(const uint8_t* rgba8, uint32_t w, uint32_t h) { check(vrt_scene_set_blue_noise(engine->ctx, handle, rgba8, w, h)); }
    // Ray queries (no reference analogue as an interface; vrt_trace_rays / vrt_occluded_rays / vrt_pick_pixels): host vectors in, host
    // vectors out.  origins, dirs: 3 floats per ray in volume coordinates, the direction used as given; a miss is 0 in every plane.
    struct RayHits { std::vector<uint8_t> material; std::vector<float> pos; std::vector<int32_t> voxel; std::vector<int8_t> normal; };
    RayHits traceRays(const std::vector<float>& origins, const std::vector<float>& dirs, uint32_t maxSteps = 512)
    {
        if (origins.size() != dirs.size() || origins.size() % 3) throw std::runtime_error("traceRays: origins and dirs hold 3 floats per ray");
        const size_t n = origins.size() / 3;
        if (n == 0) return RayHits{};
        DeviceBuffer<float> o(engine, 3 * n), d(engine, 3 * n);
        check(vrt_memcpy_h2d(engine->ctx, o.ptr, origins.data(), 12 * n)); check(vrt_memcpy_h2d(engine->ctx, d.ptr, dirs.data(), 12 * n));
        HitPlanes h(engine, n);
        check(vrt_trace_rays(engine->ctx, handle, (int64_t)n, o.ptr, d.ptr, maxSteps, &h.c));
        return h.download();
    }
    std::vector<uint8_t> occluded(const std::vector<float>& origins, const std::vector<float>& dirs, uint32_t maxSteps = 512)
    {
        if (origins.size() != dirs.size() || origins.size() % 3) throw std::runtime_error("occluded: origins and dirs hold 3 floats per ray");
        const size_t n = origins.size() / 3;
        if (n == 0) return {};
        DeviceBuffer<float> o(engine, 3 * n), d(engine, 3 * n);
        check(vrt_memcpy_h2d(engine->ctx, o.ptr, origins.data(), 12 * n)); check(vrt_memcpy_h2d(engine->ctx, d.ptr, dirs.data(), 12 * n));
        DeviceBuffer<uint8_t> occ(engine, n);
        check(vrt_occluded_rays(engine->ctx, handle, (int64_t)n, o.ptr, d.ptr, maxSteps, occ.ptr));
        return occ.download();
    }
    // Ray segments (vrt_trace_segments / vrt_occluded_segments): the same with a distance limit per ray, tMax[i] in units of ray i's
    // direction; a hit is kept iff its parameter t <= tMax[i], one that is not is a miss (0 in every plane and in t).
    struct SegmentHits { RayHits hits; std::vector<float> t; };
    SegmentHits traceSegments(const std::vector<float>& origins, const std::vector<float>& dirs, const std::vector<float>& tMax, uint32_t maxSteps = 512)
    {
        if (origins.size() != dirs.size() || origins.size() % 3 || tMax.size() * 3 != origins.size())
            throw std::runtime_error("traceSegments: origins and dirs hold 3 floats per ray, tMax one");
        const size_t n = tMax.size();
        if (n == 0) return SegmentHits{};
        DeviceBuffer<float> o(engine, 3 * n), d(engine, 3 * n), tm(engine, n), t(engine, n);
        check(vrt_memcpy_h2d(engine->ctx, o.ptr, origins.data(), 12 * n)); check(vrt_memcpy_h2d(engine->ctx, d.ptr, dirs.data(), 12 * n));
        check(vrt_memcpy_h2d(engine->ctx, tm.ptr, tMax.data(), 4 * n));
        HitPlanes h(engine, n);
        check(vrt_trace_segments(engine->ctx, handle, (int64_t)n, o.ptr, d.ptr, tm.ptr, maxSteps, &h.c, t.ptr));
        return SegmentHits{h.download(), t.download()};
    }
    std::vector<uint8_t> occluded(const std::vector<float>& origins, const std::vector<float>& dirs, const std::vector<float>& tMax, uint32_t maxSteps = 512)
    {
        if (origins.size() != dirs.size() || origins.size() % 3 || tMax.size() * 3 != origins.size())
            throw std::runtime_error("occluded: origins and dirs hold 3 floats per ray, tMax one");
        const size_t n = tMax.size();
        if (n == 0) return {};
        DeviceBuffer<float> o(engine, 3 * n), d(engine, 3 * n), tm(engine, n);
        check(vrt_memcpy_h2d(engine->ctx, o.ptr, origins.data(), 12 * n)); check(vrt_memcpy_h2d(engine->ctx, d.ptr, dirs.data(), 12 * n));
        check(vrt_memcpy_h2d(engine->ctx, tm.ptr, tMax.data(), 4 * n));
        DeviceBuffer<uint8_t> occ(engine, n);
        check(vrt_occluded_segments(engine->ctx, handle, (int64_t)n, o.ptr, d.ptr, tm.ptr, maxSteps, occ.ptr));
        return occ.download();
    }
    // Line of sight for point pairs: 1 where no voxel lies between a[i] and b[i] -- origin a, direction b - a (fp32), tMax = 1.  Inherited
    // from boxIntersection: for a outside the volume the ray is advanced 0.1 * |b - a| voxels past the face it enters through.
    std::vector<uint8_t> visible(const std::vector<float>& a, const std::vector<float>& b, uint32_t maxSteps = 512)
    {
        if (a.size() != b.size() || a.size() % 3) throw std::runtime_error("visible: a and b hold 3 floats per point");
        std::vector<float> d(a.size());
        for (size_t i = 0; i < a.size(); i++) d[i] = b[i] - a[i];
        std::vector<uint8_t> v = occluded(a, d, std::vector<float>(a.size() / 3, 1.0f), maxSteps);
        for (uint8_t& x : v) x = x ? 0 : 1;
        return v;
    }
    // xy: (x, y) per pixel; record i is what a frame rendered with `push` holds at pixel i
    RayHits pick(const vrt_push& push, const std::vector<int32_t>& xy, uint32_t maxSteps = 512)
    {
        if (xy.size() % 2) throw std::runtime_error("pick: xy holds 2 coordinates per pixel");
        const size_t n = xy.size() / 2;
        if (n == 0) return RayHits{};
        DeviceBuffer<int32_t> p(engine, 2 * n);
        check(vrt_memcpy_h2d(engine->ctx, p.ptr, xy.data(), 8 * n));
        HitPlanes h(engine, n);
        check(vrt_pick_pixels(engine->ctx, handle, &push, maxSteps, (int64_t)n, p.ptr, &h.c));
        return h.download();
    }
    vrt_scene* handle = nullptr;
private:
    struct HitPlanes {
        DeviceBuffer<uint8_t> material; DeviceBuffer<float> pos; DeviceBuffer<int32_t> voxel; DeviceBuffer<int8_t> normal; vrt_ray_hits c{};
        HitPlanes(const std::shared_ptr<Engine>& e, size_t n) : material(e, n), pos(e, 3 * n), voxel(e, 3 * n), normal(e, 3 * n)
        { c.material = material.ptr; c.pos = pos.ptr; c.voxel = voxel.ptr; c.normal = normal.ptr; }
        RayHits download() const { return RayHits{material.download(), pos.download(), voxel.download(), normal.download()}; }   // (vrt_memcpy_d2h waits for the stream)
    };
    void dims() { uint32_t d[3]; check(vrt_scene_info(handle, d)); width = d[0]; height = d[1]; depth = d[2]; }
    std::shared_ptr<Engine> engine;
};

// ---- stages -------------------------------------------------------------------------------------------
struct GeometryBuffer {                                   // geometry_stage.hpp:19-27
    std::shared_ptr<DeviceBuffer<uint8_t>> color, mask; std::shared_ptr<DeviceBuffer<float>> depth, motion, position;
    std::shared_ptr<DeviceBuffer<int8_t>> normal; uint32_t width = 0, height = 0;
};

class GeometryStage {
public:
    GeometryStage(const std::shared_ptr<Engine>& engine, const std::shared_ptr<VoxelRenderSettings>& settings, const std::shared_ptr<VoxelScene>& scene)
        : engine(engine), settings(settings), scene(scene) {}
    GeometryBuffer record(const vrt_push& push, const vrt_shard* shard = nullptr)     // geometry_stage.cpp:106
    {
        vrt_frame f = targets();
        vrt_settings st = settings->toC();
        check(vrt_render_geometry(engine->ctx, scene->handle, &push, &st, &f, shard));
        return gb;
    }
    // The G-buffer of a frame whose primary rays the caller supplies (no reference analogue; vrt_render_rays): origins, dirs are DEVICE
    // pointers to renderResolution() rays of 3 packed floats, ray py * W + px for pixel (px, py) -- what vrt_camera_rays writes
    GeometryBuffer recordRays(const float* origins, const float* dirs, uint32_t frame = 0)
    {
        vrt_frame f = targets();
        vrt_settings st = settings->toC();
        check(vrt_render_rays(engine->ctx, scene->handle, (int32_t)gb.width, (int32_t)gb.height, origins, dirs, frame, &st, &f));
        return gb;
    }
    // n camera poses in one launch per 8 frames (vrt_render_geometry_batch); every frame gets its own planes, kept in `batch`
    const std::vector<GeometryBuffer>& recordBatch(const std::vector<vrt_push>& pushes, const vrt_shard* shard = nullptr)
    {
        auto res = settings->renderResolution();
        size_t n = (size_t)res[0] * res[1];
        while (batch.size() < pushes.size()) {
            GeometryBuffer g;
            g.color = std::make_shared<DeviceBuffer<uint8_t>>(engine, n * 4); g.mask = std::make_shared<DeviceBuffer<uint8_t>>(engine, n);
            g.depth = std::make_shared<DeviceBuffer<float>>(engine, n); g.motion = std::make_shared<DeviceBuffer<float>>(engine, n * 2);
            g.position = std::make_shared<DeviceBuffer<float>>(engine, n * 4); g.normal = std::make_shared<DeviceBuffer<int8_t>>(engine, n * 4);
            g.width = res[0]; g.height = res[1];
            batch.push_back(g);
        }
        std::vector<vrt_frame> frames(pushes.size());
        for (size_t k = 0; k < pushes.size(); k++) {
            vrt_frame f{}; const GeometryBuffer& g = batch[k];
            f.color8 = g.color->ptr; f.depth = g.depth->ptr; f.motion = g.motion->ptr; f.mask8 = g.mask->ptr; f.position = g.position->ptr; f.normal8 = g.normal->ptr;
            frames[k] = f;
        }
        vrt_settings st = settings->toC();
        check(vrt_render_geometry_batch(engine->ctx, scene->handle, (int32_t)pushes.size(), pushes.data(), &st, frames.data(), shard));
        return batch;
    }
private:
    vrt_frame targets()
    {
        auto res = settings->renderResolution();
        if (gb.width != res[0] || gb.height != res[1]) {                              // RENDER_RESIZE recreation (:19-45)
            size_t n = (size_t)res[0] * res[1];
            gb.color = std::make_shared<DeviceBuffer<uint8_t>>(engine, n * 4); gb.mask = std::make_shared<DeviceBuffer<uint8_t>>(engine, n);
            gb.depth = std::make_shared<DeviceBuffer<float>>(engine, n); gb.motion = std::make_shared<DeviceBuffer<float>>(engine, n * 2);
            gb.position = std::make_shared<DeviceBuffer<float>>(engine, n * 4); gb.normal = std::make_shared<DeviceBuffer<int8_t>>(engine, n * 4);
            gb.width = res[0]; gb.height = res[1];
        }
        vrt_frame f{}; f.color8 = gb.color->ptr; f.depth = gb.depth->ptr; f.motion = gb.motion->ptr; f.mask8 = gb.mask->ptr;
        f.position = gb.position->ptr; f.normal8 = gb.normal->ptr;
        return f;
    }
    std::shared_ptr<Engine> engine; std::shared_ptr<VoxelRenderSettings> settings; std::shared_ptr<VoxelScene> scene; GeometryBuffer gb;
    std::vector<GeometryBuffer> batch;
};

class DenoiserStage {
public:
    DenoiserStage(const std::shared_ptr<Engine>& engine, const std::shared_ptr<VoxelRenderSettings>& settings) : engine(engine), settings(settings) {}
    // returns the device pointer of the image holding the result (one of the ping-pong targets, or colorInput)
    const uint8_t* record(const GeometryBuffer& g, const vrt_shard* shard = nullptr)  // denoiser_stage.cpp:156
    {
        size_t n = (size_t)g.width * g.height * 4;
        if (!targets[0] || targets[0]->count != n) { targets[0] = std::make_shared<DeviceBuffer<uint8_t>>(engine, n); targets[1] = std::make_shared<DeviceBuffer<uint8_t>>(engine, n); }
        vrt_denoiser_settings ds = settings->denoiserToC();
        const uint8_t* result = nullptr;
        check(vrt_denoise(engine->ctx, (int32_t)g.width, (int32_t)g.height, &ds, g.color->ptr, g.normal->ptr, g.position->ptr,
                          targets[0]->ptr, targets[1]->ptr, shard, &result));
        return result;
    }
private:
    std::shared_ptr<Engine> engine; std::shared_ptr<VoxelRenderSettings> settings; std::shared_ptr<DeviceBuffer<uint8_t>> targets[2];
};

// UpscalerStage (upscaler_stage.cpp): update() is the reference's jitter / frame sequence (:59-70); record() replaces the
// FSR2 dispatch (:72-161, prebuilt third party, out of scope) by exact N-frame accumulation + bilinear upscale (a camera at
// rest), recordReprojected() by temporal reprojection (a moving one), recordUpsampled() by temporal upsampling (the history at
// targetResolution, no blit).
class UpscalerStage {
public:
    float jitterX = 0, jitterY = 0; int frameCount = 0; uint32_t accumulated = 0;
    UpscalerStage(const std::shared_ptr<Engine>& engine, const std::shared_ptr<VoxelRenderSettings>& settings) : engine(engine), settings(settings) {}
    int32_t phaseCount() const { return vrt_jitter_phase_count((int32_t)settings->renderResolution()[0], (int32_t)settings->targetResolution[0]); }
    void update(float delta)                                                           // :59-70
    {
        _deltaMsec = delta * 1000;
        const int32_t jitterPhaseCount = phaseCount();
        check(vrt_jitter_offset(frameCount % jitterPhaseCount, jitterPhaseCount, &jitterX, &jitterY));
        frameCount++;
        if (frameCount > jitterPhaseCount) frameCount = 0;
    }
    void reset() { accumulated = 0; histCur = -1; }
    // The temporal pass under a moving camera (vrt_reproject): `color` is blended into the history fetched where each pixel's
    // surface was on the previous frame's screen, and the motion vectors are written into g.motion.  Two histories are written in
    // turn; reset() starts a new sequence.
    vrt_reproject_settings reprojectSettings{0, 0.5f, -1.0f};                          // max_history 0 / tol_rel < 0: the default
    const uint8_t* recordReprojected(const uint8_t* color, const GeometryBuffer& g, const vrt_push& push)
    {
        ensureReprojected(g);
        vrt_reproject_settings st; vrt_reproject_settings_default(&push, &st); overrideSettings(st);
        vrt_history in{}, out{}; const bool running = nextHistories(in, out);
        check(vrt_reproject(engine->ctx, (int32_t)g.width, (int32_t)g.height, &push, running ? &prevPush : &push, &st, color, g.position->ptr, g.normal->ptr,
                            running ? &in : nullptr, &out, resolved->ptr, g.motion->ptr));
        commit(); prevPush = push;
        return upscaled(g.width, g.height);
    }
    // recordReprojected() for a frame drawn through a vrt_ray_camera (vrt_reproject_camera): cam is the block the frame's rays were
    // made with; the previous frame's is kept here.  The histories are recordReprojected()'s buffers.
    const uint8_t* recordReprojectedCamera(const uint8_t* color, const GeometryBuffer& g, const vrt_ray_camera& cam)
    {
        ensureReprojected(g);
        if (histCur >= 0 && prevCamera.model != cam.model) histCur = -1;               // another camera model: a new sequence
        vrt_reproject_settings st; vrt_reproject_camera_settings_default(&cam, (int32_t)g.width, &st); overrideSettings(st);
        vrt_history in{}, out{}; const bool running = nextHistories(in, out);
        check(vrt_reproject_camera(engine->ctx, (int32_t)g.width, (int32_t)g.height, &cam, running ? &prevCamera : &cam, &st, color, g.position->ptr, g.normal->ptr,
                                   running ? &in : nullptr, &out, resolved->ptr, g.motion->ptr));
        commit(); prevCamera = cam;
        return upscaled(g.width, g.height);
    }
    // The temporal pass at display resolution (vrt_upsample): the history pair, the resolved image and the motion vectors
    // (motion(), in display pixels; g.motion is not touched) live at targetResolution, every sample where it fell on the display grid.
    const uint8_t* recordUpsampled(const uint8_t* color, const GeometryBuffer& g, const vrt_push& push)
    {
        const uint32_t tw = settings->targetResolution[0], th = settings->targetResolution[1];
        const size_t tn = (size_t)tw * th;
        ensureHistories(tn);
        ensureTarget();
        if (!displayMotion || displayMotion->count != tn * 2) displayMotion = std::make_shared<DeviceBuffer<float>>(engine, tn * 2);
        vrt_reproject_settings st; vrt_reproject_settings_default(&push, &st); overrideSettings(st);
        vrt_history in{}, out{}; const bool running = nextHistories(in, out);
        check(vrt_upsample(engine->ctx, (int32_t)g.width, (int32_t)g.height, (int32_t)tw, (int32_t)th, &push, running ? &prevPush : &push, &st, color,
                           g.position->ptr, g.normal->ptr, running ? &in : nullptr, &out, target->ptr, displayMotion->ptr));
        commit(); prevPush = push;
        return target->ptr;
    }
    // recordUpsampled() for a frame drawn through a vrt_ray_camera (vrt_upsample_camera): cam is the frame's camera WITHOUT sample
    // offset and without jitter (the offsets went into the rays); the previous frame's is kept here.  The histories, the target
    // and motion() are recordUpsampled()'s buffers.
    const uint8_t* recordUpsampledCamera(const uint8_t* color, const GeometryBuffer& g, const vrt_ray_camera& cam)
    {
        const uint32_t tw = settings->targetResolution[0], th = settings->targetResolution[1];
        const size_t tn = (size_t)tw * th;
        ensureHistories(tn);
        ensureTarget();
        if (!displayMotion || displayMotion->count != tn * 2) displayMotion = std::make_shared<DeviceBuffer<float>>(engine, tn * 2);
        if (histCur >= 0 && prevCamera.model != cam.model) histCur = -1;               // another camera model: a new sequence
        vrt_reproject_settings st; vrt_upsample_camera_settings_default(&cam, (int32_t)g.width, &st); overrideSettings(st);
        vrt_history in{}, out{}; const bool running = nextHistories(in, out);
        check(vrt_upsample_camera(engine->ctx, (int32_t)g.width, (int32_t)g.height, (int32_t)tw, (int32_t)th, &cam, running ? &prevCamera : &cam, &st, color,
                                  g.position->ptr, g.normal->ptr, running ? &in : nullptr, &out, target->ptr, displayMotion->ptr));
        commit(); prevCamera = cam;
        return target->ptr;
    }
    const float* motion() const { return displayMotion ? displayMotion->ptr : nullptr; }
    const uint8_t* record(const uint8_t* color, uint32_t w, uint32_t h)
    {
        size_t n = (size_t)w * h * 4;
        if (!accum || accum->count != n || !resolved || resolved->count != n) { accum = std::make_shared<DeviceBuffer<uint32_t>>(engine, n); resolved = std::make_shared<DeviceBuffer<uint8_t>>(engine, n); accumulated = 0; }
        ensureTarget();
        check(vrt_accumulate(engine->ctx, color, accum->ptr, (int32_t)w, (int32_t)h, accumulated == 0));
        accumulated++;
        check(vrt_resolve(engine->ctx, accum->ptr, resolved->ptr, (int32_t)w, (int32_t)h, accumulated));
        return upscaled(w, h);
    }
private:
    // -- what the temporal passes share: the ring of two histories written in turn, the settings, the images
    void ensureHistories(size_t n)                                                      // n texels each; another size starts a new sequence
    {
        if (histColor[0] && histColor[0]->count == n * 4) return;
        for (int k = 0; k < 2; k++) { histColor[k] = std::make_shared<DeviceBuffer<uint16_t>>(engine, n * 4); histSurface[k] = std::make_shared<DeviceBuffer<uint32_t>>(engine, n * 4); }
        histCur = -1;
    }
    bool nextHistories(vrt_history& in, vrt_history& out) const                         // what the next call reads and writes; false: no history in
    {
        const int nxt = histCur >= 0 ? 1 - histCur : 0;
        out = {histColor[nxt]->ptr, histSurface[nxt]->ptr};
        if (histCur >= 0) in = {histColor[histCur]->ptr, histSurface[histCur]->ptr};
        return histCur >= 0;
    }
    void commit() { histCur = histCur >= 0 ? 1 - histCur : 0; accumulated++; }         // the call wrote `out`
    void overrideSettings(vrt_reproject_settings& st) const                            // a camera's defaults under reprojectSettings
    {
        if (reprojectSettings.max_history != 0) st.max_history = reprojectSettings.max_history;
        st.tol_abs = reprojectSettings.tol_abs;
        if (reprojectSettings.tol_rel >= 0) st.tol_rel = reprojectSettings.tol_rel;
    }
    void ensureTarget() { size_t tn = (size_t)settings->targetResolution[0] * settings->targetResolution[1] * 4; if (!target || target->count != tn) target = std::make_shared<DeviceBuffer<uint8_t>>(engine, tn); }
    void ensureReprojected(const GeometryBuffer& g)                                     // histories and the resolved image at render size
    {
        const size_t n = (size_t)g.width * g.height;
        ensureHistories(n);
        if (!resolved || resolved->count != n * 4) { resolved = std::make_shared<DeviceBuffer<uint8_t>>(engine, n * 4); accum.reset(); }
        ensureTarget();
    }
    const uint8_t* upscaled(uint32_t w, uint32_t h)                                     // the resolved image through the bilinear blit
    {
        check(vrt_blit(engine->ctx, resolved->ptr, (int32_t)w, (int32_t)h, target->ptr, (int32_t)settings->targetResolution[0], (int32_t)settings->targetResolution[1]));
        return target->ptr;
    }
    std::shared_ptr<Engine> engine; std::shared_ptr<VoxelRenderSettings> settings; float _deltaMsec = 0;
    std::shared_ptr<DeviceBuffer<uint32_t>> accum; std::shared_ptr<DeviceBuffer<uint8_t>> resolved, target;
    std::shared_ptr<DeviceBuffer<uint16_t>> histColor[2]; std::shared_ptr<DeviceBuffer<uint32_t>> histSurface[2]; int histCur = -1; vrt_push prevPush{}; vrt_ray_camera prevCamera{};
    std::shared_ptr<DeviceBuffer<float>> displayMotion;
};

// BlitStage::record + shader/blit.frag (blit_stage.cpp:41-75): centre-cropped bilinear copy to a window-sized target.
class BlitStage {
public:
    BlitStage(const std::shared_ptr<Engine>& engine, const std::shared_ptr<VoxelRenderSettings>& settings) : engine(engine), settings(settings) {}
    const uint8_t* record(const uint8_t* source, uint32_t sw, uint32_t sh, uint32_t tw, uint32_t th)
    {
        size_t n = (size_t)tw * th * 4;
        if (!target || target->count != n) target = std::make_shared<DeviceBuffer<uint8_t>>(engine, n);
        check(vrt_blit(engine->ctx, source, (int32_t)sw, (int32_t)sh, target->ptr, (int32_t)tw, (int32_t)th));
        return target->ptr;
    }
private:
    std::shared_ptr<Engine> engine; std::shared_ptr<VoxelRenderSettings> settings; std::shared_ptr<DeviceBuffer<uint8_t>> target;
};

// ---- renderer (voxel_renderer.cpp) ----------------------------------------------------------------------
class VoxelRenderer {
public:
    VoxelRenderer(const std::shared_ptr<Engine>& engine, const std::shared_ptr<VoxelRenderSettings>& settings, const std::shared_ptr<VoxelScene>& scene)
        : engine(engine), _settings(settings), _scene(scene), _camera(std::make_unique<CameraController>()),
          _geometryStage(std::make_unique<GeometryStage>(engine, settings, scene)), _denoiserStage(std::make_unique<DenoiserStage>(engine, settings)),
          _upscalerStage(std::make_unique<UpscalerStage>(engine, settings)), _blitStage(std::make_unique<BlitStage>(engine, settings)) {}
    CameraController& camera() { return *_camera; }
    UpscalerStage& upscaler() { return *_upscalerStage; }
    void update(float delta, float forward = 0.0f, float strafe = 0.0f)               // :33-39
    { _time += delta; _camera->update(delta, forward, strafe); _upscalerStage->update(delta); }
    vrt_push pushConstants() const                                                     // :72-83
    {
        vrt_push p{}; auto res = _settings->renderResolution();
        p.screen_size[0] = (int32_t)res[0]; p.screen_size[1] = (int32_t)res[1];
        p.volume_bounds[0] = _scene->width; p.volume_bounds[1] = _scene->height; p.volume_bounds[2] = _scene->depth;
        const CameraController& c = *_camera;
        p.cam_pos[0] = c.position.x; p.cam_pos[1] = c.position.y; p.cam_pos[2] = c.position.z; p.cam_pos[3] = 1;
        p.cam_dir[0] = c.direction.x; p.cam_dir[1] = c.direction.y; p.cam_dir[2] = c.direction.z;
        p.cam_up[0] = c.up.x; p.cam_up[1] = c.up.y; p.cam_up[2] = c.up.z;
        p.cam_right[0] = c.right.x; p.cam_right[1] = c.right.y; p.cam_right[2] = c.right.z;
        p.frame = (uint32_t)_upscalerStage->frameCount;                                // :80-82
        p.camera_jitter[0] = _upscalerStage->jitterX; p.camera_jitter[1] = _upscalerStage->jitterY;
        return p;
    }
    // recordCommands (:55-94); returns the RGBA8 image (host copy) and its size in outW / outH.
    // temporal: take the FSR branch (:86-87) through the accumulation stand-in -- or, with reproject, through temporal reprojection,
    // which keeps the history under a moving camera and fills gBuffer.motion -- with upsample too, at targetResolution (temporal
    // upsampling: no blit, motion in upscaler().motion()); windowW/H != 0: append the blit (:89).  With a projection the temporal
    // pass is vrt_reproject_camera (reproject is required), with upsample vrt_upsample_camera.
    std::vector<uint8_t> render(uint32_t* outW = nullptr, uint32_t* outH = nullptr)
    {
        vrt_push push = pushConstants();
        GeometryBuffer g;
        vrt_ray_camera cam{};
        if (projection >= 0) {
            // another camera model: its rays (vrt_camera_rays over this renderer's camera basis and jitter), then their G-buffer
            if (temporal && !reproject) throw std::runtime_error("VoxelRenderer: temporal with a projection needs reproject (the pixel-by-pixel accumulation is wrong for a moving ray camera)");
            cam.model = projection; cam.basis = push; cam.tan_half = tanHalf; cam.half_width = halfWidth;
            const size_t n = (size_t)push.screen_size[0] * (size_t)push.screen_size[1];
            if (!_rayOrigins || _rayOrigins->count != 3 * n) { _rayOrigins = std::make_unique<DeviceBuffer<float>>(engine, 3 * n); _rayDirs = std::make_unique<DeviceBuffer<float>>(engine, 3 * n); }
            // upsample: the orthographic and the panorama model, which apply no jitter, take the jitter sequence as sample offsets
            const float offset[2] = {push.camera_jitter[0], push.camera_jitter[1]};
            if (upsample && projection != VRT_CAMERA_PERSPECTIVE && (offset[0] != 0.0f || offset[1] != 0.0f))
                check(vrt_camera_rays_offset(engine->ctx, &cam, push.screen_size[0], push.screen_size[1], offset, _rayOrigins->ptr, _rayDirs->ptr));
            else check(vrt_camera_rays(engine->ctx, &cam, push.screen_size[0], push.screen_size[1], _rayOrigins->ptr, _rayDirs->ptr));
            g = _geometryStage->recordRays(_rayOrigins->ptr, _rayDirs->ptr, push.frame);
            // (the display-resolution pass projects through the camera without offset and without jitter)
            if (upsample) cam.basis.camera_jitter[0] = cam.basis.camera_jitter[1] = 0.0f;
        } else g = _geometryStage->record(push);
        const uint8_t* img = _settings->denoiserSettings.enable ? _denoiserStage->record(g) : g.color->ptr;
        uint32_t w = g.width, h = g.height;
        if (temporal && _settings->fsrSetttings.enable) { if (upsample && !reproject) throw std::runtime_error("VoxelRenderer: upsample needs reproject"); img = !reproject ? _upscalerStage->record(img, w, h) : projection >= 0 ? (upsample ? _upscalerStage->recordUpsampledCamera(img, g, cam) : _upscalerStage->recordReprojectedCamera(img, g, cam)) : upsample ? _upscalerStage->recordUpsampled(img, g, push) : _upscalerStage->recordReprojected(img, g, push); w = _settings->targetResolution[0]; h = _settings->targetResolution[1]; }
        if (windowW && windowH) { img = _blitStage->record(img, w, h, windowW, windowH); w = windowW; h = windowH; }
        std::vector<uint8_t> host((size_t)w * h * 4);
        check(vrt_memcpy_d2h(engine->ctx, host.data(), img, host.size()));
        gBuffer = g;
        if (outW) *outW = w;
        if (outH) *outH = h;
        return host;
    }
    bool temporal = false, reproject = false, upsample = false; uint32_t windowW = 0, windowH = 0; GeometryBuffer gBuffer;
    // projection >= 0: a VRT_CAMERA_* model drawn through vrt_camera_rays + vrt_render_rays instead of the built-in 90-degree pinhole
    int projection = -1; float tanHalf = 1.0f, halfWidth = 1.0f;
private:
    std::unique_ptr<DeviceBuffer<float>> _rayOrigins, _rayDirs;
    std::shared_ptr<Engine> engine; std::shared_ptr<VoxelRenderSettings> _settings; std::shared_ptr<VoxelScene> _scene;
    std::unique_ptr<CameraController> _camera; std::unique_ptr<GeometryStage> _geometryStage; std::unique_ptr<DenoiserStage> _denoiserStage;
    std::unique_ptr<UpscalerStage> _upscalerStage; std::unique_ptr<BlitStage> _blitStage;
    float _time = 0;
};

// ---- one process, several GPUs (no reference analogue; BASELINE north_star) -----------------------------------------------
// The frame cut into 16-row strips, strip s traced by device s % N (every device holds the whole scene), the three planes the
// rest of the frame graph reads -- colour, normal, position -- gathered to device 0 through RCCL (vrt_gather_strips, one
// grouped gather per plane), assembled there, and the denoiser run on the assembled frame.  (The Python host also shards
// the denoiser, with a ring exchange of halo rows: voxel-raytracing_amd/distributed.py.)
class ShardedRenderer {
public:
    ShardedRenderer(const std::vector<std::shared_ptr<Engine>>& engines, const std::shared_ptr<VoxelRenderSettings>& settings,
                    const std::vector<std::shared_ptr<VoxelScene>>& scenes, int stripRows = 16)
        : engines(engines), settings(settings), scenes(scenes), stripRows(stripRows), comms(engines.size(), nullptr)
    {
        if (engines.empty() || engines.size() != scenes.size()) throw std::runtime_error("ShardedRenderer: one scene per engine");
        std::vector<vrt_ctx*> ctxs;
        for (auto& e : engines) ctxs.push_back(e->ctx);
        check(vrt_comm_init_all((int32_t)ctxs.size(), ctxs.data(), comms.data()));
        for (size_t i = 0; i < engines.size(); i++) stages.push_back(std::make_unique<GeometryStage>(engines[i], settings, scenes[i]));
        denoiser = std::make_unique<DenoiserStage>(engines[0], settings);
    }
    ~ShardedRenderer() { for (vrt_comm* c : comms) vrt_comm_destroy(c); }
    ShardedRenderer(const ShardedRenderer&) = delete; ShardedRenderer& operator=(const ShardedRenderer&) = delete;

    std::vector<uint8_t> render(const vrt_push& push, uint32_t* outW = nullptr, uint32_t* outH = nullptr)
    {
        const int n = (int)engines.size();
        auto res = settings->renderResolution();
        const int32_t W = (int32_t)res[0], H = (int32_t)res[1];
        std::vector<GeometryBuffer> gbs;
        std::vector<vrt_shard> shards((size_t)n);
        for (int r = 0; r < n; r++) {                                   // every device traces its strips (asynchronously)
            shards[(size_t)r] = vrt_shard{r, n, stripRows};
            gbs.push_back(stages[(size_t)r]->record(push, n > 1 ? &shards[(size_t)r] : nullptr));
        }
        {                                                               // (one device: a one-rank communicator, the same path)
            const size_t rows = (size_t)vrt_shard_rows(H, &shards[0]);
            if (!full.color || full.width != res[0] || full.height != res[1]) {
                size_t px = (size_t)W * H;
                full.color = std::make_shared<DeviceBuffer<uint8_t>>(engines[0], px * 4); full.normal = std::make_shared<DeviceBuffer<int8_t>>(engines[0], px * 4);
                full.position = std::make_shared<DeviceBuffer<float>>(engines[0], px * 4);
                full.width = res[0]; full.height = res[1];
                packed.clear(); gathered.reset();
                for (int r = 0; r < n; r++) packed.push_back(std::make_shared<DeviceBuffer<uint8_t>>(engines[(size_t)r], rows * (size_t)W * 16));
                gathered = std::make_shared<DeviceBuffer<uint8_t>>(engines[0], (size_t)n * rows * (size_t)W * 16);
            }
            for (int plane = 0; plane < 3; plane++) {
                const int bpp = plane == 2 ? 16 : 4;
                const size_t bytes = rows * (size_t)W * (size_t)bpp;
                for (int r = 0; r < n; r++) {
                    const void* src = plane == 0 ? (const void*)gbs[(size_t)r].color->ptr : (plane == 1 ? (const void*)gbs[(size_t)r].normal->ptr : (const void*)gbs[(size_t)r].position->ptr);
                    check(vrt_pack_rows(engines[(size_t)r]->ctx, src, packed[(size_t)r]->ptr, W, H, bpp, &shards[(size_t)r]));
                }
                check(vrt_group_start());                               // the n ranks of this process: one grouped gather
                for (int r = 0; r < n; r++)
                    check(vrt_gather_strips(engines[(size_t)r]->ctx, comms[(size_t)r], 0, packed[(size_t)r]->ptr, r == 0 ? gathered->ptr : nullptr, bytes));
                check(vrt_group_end());
                void* dst = plane == 0 ? (void*)full.color->ptr : (plane == 1 ? (void*)full.normal->ptr : (void*)full.position->ptr);
                for (int r = 0; r < n; r++)
                    check(vrt_unpack_rows(engines[0]->ctx, gathered->ptr + (size_t)r * bytes, dst, W, H, bpp, &shards[(size_t)r]));
                for (int r = 1; r < n; r++) engines[(size_t)r]->waitIdle();   // the send buffers are reused by the next plane
                engines[0]->waitIdle();
            }
        }
        const uint8_t* img = settings->denoiserSettings.enable ? denoiser->record(full) : full.color->ptr;
        std::vector<uint8_t> host((size_t)W * H * 4);
        check(vrt_memcpy_d2h(engines[0]->ctx, host.data(), img, host.size()));
        if (outW) *outW = res[0];
        if (outH) *outH = res[1];
        return host;
    }
private:
    std::vector<std::shared_ptr<Engine>> engines; std::shared_ptr<VoxelRenderSettings> settings; std::vector<std::shared_ptr<VoxelScene>> scenes;
    int stripRows; std::vector<vrt_comm*> comms; std::vector<std::unique_ptr<GeometryStage>> stages; std::unique_ptr<DenoiserStage> denoiser;
    GeometryBuffer full; std::vector<std::shared_ptr<DeviceBuffer<uint8_t>>> packed; std::shared_ptr<DeviceBuffer<uint8_t>> gathered;
};

} // namespace vrt_host
