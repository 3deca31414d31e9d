// vrt_api_faces.hip -- surface extraction in the C-ABI: vrt_scene_list_faces (the exposed faces of a box, compacted on the device),
// vrt_faces_mesh_host (records -> welded quads), the Wavefront OBJ writer (vrt_faces_obj_host, vrt_scene_save_obj_*).  Host code
// only; the kernels are vrt_faces.hip, the definitions csrc/vrt_faces.h.
#include <cstdio>
#include <cstring>
#include <map>
#include <unordered_map>

#include "vrt_host.h"
#define VRT_SCENE_READ_LAUNCHERS
#include "vrt_faces_launch.h"

using namespace vrt;

static_assert(VRT_FACES_RUNS == VRT_FACES_FLAG_RUNS && VRT_FACES_CLOSED == VRT_FACES_FLAG_CLOSED, "include/vrt.h and csrc/vrt_faces.h number the flags differently");

namespace {

FacesJob faces_job(const vrt_scene* s, const int32_t lo[3], const uint32_t size[3], uint32_t flags)
{
    FacesJob j{};
    j.box = read_box_of(s, lo, size);
    j.dim[0] = s->d.vol.W; j.dim[1] = s->d.vol.H; j.dim[2] = s->d.vol.D;
    j.flags = flags;
    return j;
}

// How many records the (checked) box has: first[d] = the first record of direction d, first[6] = their number, and in `work`
// every segment's first record.  A box over empty bricks only ends behind the bricks' entries.  Returns when the stream is done.
int faces_count(vrt_ctx* c, const FacesJob& j, DevBuf<uint32_t>& work, uint32_t first[VRT_FACES_DIRECTIONS + 1u])
{
    const uint32_t words = faces_work_words(j);
    for (uint32_t d = 0; d <= VRT_FACES_DIRECTIONS; d++) first[d] = 0;
    if (work.bytes() < ((size_t)words + 1u + 7u) * 4u && work.alloc(((size_t)words + 1u + 7u) * 4u) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VRT_ERR_UNSUPPORTED, "vrt_scene_list_faces: no device memory for " + std::to_string(words) + " scan words; list the box in parts");
    }
    if (!j.box.vox) {
        uint32_t occupied = 0;
        HIPCHK(launch_list_bricks(j.box, work.get(), c->stream));
        HIPCHK(hipMemcpyAsync(&occupied, work.get(), 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (!occupied) return VRT_OK;
    }
    HIPCHK(launch_faces_count(j, work.get(), c->stream));
    HIPCHK(hipMemcpyAsync(first, work.get() + words + 1u, (VRT_FACES_DIRECTIONS + 1u) * 4u, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return VRT_OK;
}

// ... and its `total` (> 0) records to the host
int faces_fetch(vrt_ctx* c, const FacesJob& j, const DevBuf<uint32_t>& work, uint32_t total, DevBuf<uint64_t>& dev, uint64_t* records)
{
    if (dev.bytes() < (size_t)total * 8u && dev.alloc((size_t)total * 8u) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VRT_ERR_UNSUPPORTED, "vrt_scene_list_faces: no device memory for a staging buffer of " + std::to_string(total) + " records; list the box in parts");
    }
    HIPCHK(launch_faces_scatter(j, work.get(), total, dev.get(), c->stream));
    HIPCHK(hipMemcpyAsync(records, dev.get(), (size_t)total * 8u, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return VRT_OK;
}

// n records -> their quads over vertices welded in order of first appearance.  A vertex is its corner in voxels relative to the
// box's lo (0 .. 256 per axis); quads and ids are appended to.
struct FaceMesh {
    std::vector<uint32_t> corners;                                  // nv * 3
    std::vector<uint32_t> quads;                                    // n * 4
    std::vector<uint8_t>  ids;                                      // n
};

bool faces_mesh(const uint64_t* records, uint64_t n, FaceMesh& m)
{
    std::unordered_map<uint32_t, uint32_t> seen;
    seen.reserve((size_t)n * 2u);
    m.quads.reserve((size_t)n * 4u);
    m.ids.reserve((size_t)n);
    for (uint64_t i = 0; i < n; i++) {
        if (!face_record_valid(records[i])) return false;
        for (uint32_t k = 0; k < 4u; k++) {
            uint32_t c[3];
            face_quad_corner(records[i], k, c);
            const uint32_t key = c[0] | (c[1] << 10) | (c[2] << 20);
            const auto at = seen.emplace(key, (uint32_t)(m.corners.size() / 3u));
            if (at.second) m.corners.insert(m.corners.end(), c, c + 3);
            m.quads.push_back(at.first->second);
        }
        m.ids.push_back((uint8_t)face_record_id(records[i]));
    }
    return true;
}

void* host_copy(const void* p, size_t bytes)
{
    void* out = malloc(bytes ? bytes : 1u);
    if (out && bytes) memcpy(out, p, bytes);
    return out;
}

// An OBJ file made tile by tile: a tile's vertices (integer voxel coordinates), then its quads under `usemtl id_<N>` in
// ascending id, within an id in the records' order.  Vertices are welded within a tile only.
struct ObjWriter {
    std::string out;
    bool used[256] = {};
    uint64_t nv = 0;

    void begin(const char* mtl_name) { out = std::string("mtllib ") + mtl_name + "\n"; }
    bool tile(const uint64_t* records, uint64_t n, const int32_t lo[3])
    {
        FaceMesh m;
        if (!faces_mesh(records, n, m)) return false;
        char line[96];
        for (size_t v = 0; v < m.corners.size(); v += 3) {
            snprintf(line, sizeof line, "v %lld %lld %lld\n", (long long)lo[0] + m.corners[v], (long long)lo[1] + m.corners[v + 1], (long long)lo[2] + m.corners[v + 2]);
            out += line;
        }
        std::map<uint32_t, std::vector<uint64_t>> by_id;
        for (uint64_t i = 0; i < n; i++) by_id[m.ids[i]].push_back(i);
        for (const auto& g : by_id) {
            used[g.first] = true;
            snprintf(line, sizeof line, "usemtl id_%u\n", g.first);
            out += line;
            for (const uint64_t i : g.second) {
                const uint32_t* q = &m.quads[i * 4u];
                snprintf(line, sizeof line, "f %llu %llu %llu %llu\n", (unsigned long long)(nv + q[0] + 1u), (unsigned long long)(nv + q[1] + 1u),
                         (unsigned long long)(nv + q[2] + 1u), (unsigned long long)(nv + q[3] + 1u));
                out += line;
            }
        }
        nv += m.corners.size() / 3u;
        return true;
    }
    std::string mtl(const vrt_material palette[256]) const
    {
        std::string t;
        char line[128];
        for (uint32_t id = 1; id < 256u; id++) {
            if (!used[id]) continue;
            snprintf(line, sizeof line, "newmtl id_%u\nKd %.9g %.9g %.9g\n", id, palette[id].diffuse[0], palette[id].diffuse[1], palette[id].diffuse[2]);
            t += line;
        }
        return t;
    }
};

int obj_out(const ObjWriter& w, const vrt_material palette[256], void** obj, size_t* nobj, void** mtl, size_t* nmtl)
{
    const std::string t = w.mtl(palette);
    void* a = host_copy(w.out.data(), w.out.size());
    void* b = host_copy(t.data(), t.size());
    if (!a || !b) { free(a); free(b); return fail(VRT_ERR_INVALID, "out of host memory"); }
    *obj = a; *nobj = w.out.size(); *mtl = b; *nmtl = t.size();
    return VRT_OK;
}

// the scene's surface as an OBJ: per tile of vox_writer's tiling one vrt_scene_list_faces, then the writer
int scene_save_obj(vrt_ctx* c, const vrt_scene* s, const char* mtl_name, uint32_t flags, ObjWriter& w, std::vector<vrt_material>& palette)
{
    if (flags & ~VRT_FACES_FLAG_RUNS)
        return fail(VRT_ERR_INVALID, flags & VRT_FACES_FLAG_CLOSED ? "vrt_scene_save_obj: VRT_FACES_CLOSED would put seams between the tiles" : "vrt_scene_save_obj: unknown flag");
    HIPCHK(hipSetDevice(c->device));
    palette.resize(256);
    HIPCHK(hipMemcpyAsync(palette.data(), s->palette.get(), 256 * sizeof(vrt_material), hipMemcpyDeviceToHost, c->stream));
    const uint32_t dims[3] = {(uint32_t)s->d.vol.W, (uint32_t)s->d.vol.H, (uint32_t)s->d.vol.D};
    uint32_t nt[3];
    for (int a = 0; a < 3; a++) nt[a] = save_tiles(dims[a]);
    w.begin(mtl_name);
    DevBuf<uint32_t> work;
    DevBuf<uint64_t> dev;
    std::vector<uint64_t> rec;
    for (uint32_t tz = 0; tz < nt[2]; tz++)
        for (uint32_t ty = 0; ty < nt[1]; ty++)
            for (uint32_t tx = 0; tx < nt[0]; tx++) {
                const uint32_t t[3] = {tx, ty, tz};
                int32_t lo[3]; uint32_t size[3], first[VRT_FACES_DIRECTIONS + 1u];
                for (int a = 0; a < 3; a++) { uint32_t l; save_tile_span(dims[a], t[a], &l, &size[a]); lo[a] = (int32_t)l; }
                const FacesJob j = faces_job(s, lo, size, flags);
                int rc = faces_count(c, j, work, first);
                if (rc != VRT_OK) return rc;
                const uint32_t total = first[VRT_FACES_DIRECTIONS];
                rec.resize(total);
                if (total && (rc = faces_fetch(c, j, work, total, dev, rec.data())) != VRT_OK) return rc;
                if (!w.tile(rec.data(), total, lo)) return fail(VRT_ERR_HIP, "vrt_scene_save_obj: a record the kernels cannot have written");
            }
    HIPCHK(hipStreamSynchronize(c->stream));
    return VRT_OK;
}

} // namespace

extern "C" {

int vrt_scene_list_faces(struct vrt_ctx* c, const vrt_scene* s, const int32_t lo[3], const uint32_t size[3], uint32_t flags, uint64_t* records,
                         uint64_t capacity, uint64_t counts[6])
{
    if (!c || !s || !lo || !size || !counts) return fail(VRT_ERR_INVALID, "vrt_scene_list_faces: NULL argument");
    for (uint32_t d = 0; d < VRT_FACES_DIRECTIONS; d++) counts[d] = 0;
    if (flags & ~(VRT_FACES_FLAG_RUNS | VRT_FACES_FLAG_CLOSED)) return fail(VRT_ERR_INVALID, "vrt_scene_list_faces: unknown flag");
    size_t n = 0;
    int rc = read_box_checked(s, lo, size, VRT_LIST_MAX_SIDE, "vrt_scene_list_faces", &n);
    if (rc != VRT_OK) return rc;
    HIPCHK(hipSetDevice(c->device));
    const FacesJob j = faces_job(s, lo, size, flags);
    DevBuf<uint32_t> work;
    DevBuf<uint64_t> dev;
    uint32_t first[VRT_FACES_DIRECTIONS + 1u];
    if ((rc = faces_count(c, j, work, first)) != VRT_OK) return rc;
    for (uint32_t d = 0; d < VRT_FACES_DIRECTIONS; d++) counts[d] = first[d + 1u] - first[d];
    const uint32_t total = first[VRT_FACES_DIRECTIONS];
    if (!records || !total) return VRT_OK;
    if (capacity < (uint64_t)total)
        return fail(VRT_ERR_INVALID, "vrt_scene_list_faces: the box has " + std::to_string(total) + " records and `records` room for " + std::to_string(capacity));
    return faces_fetch(c, j, work, total, dev, records);
}

int vrt_faces_mesh_host(const uint64_t* records, uint64_t n, const int32_t lo[3], int32_t** vertices, uint64_t* nv, uint32_t** quads, uint8_t** ids)
{
    if ((!records && n) || !lo || !vertices || !nv || !quads || !ids) return fail(VRT_ERR_INVALID, "vrt_faces_mesh_host: NULL argument");
    if (n > (1ull << 28)) return fail(VRT_ERR_INVALID, "vrt_faces_mesh_host: more records than a box has");
    FaceMesh m;
    if (!faces_mesh(records, n, m)) return fail(VRT_ERR_INVALID, "vrt_faces_mesh_host: a word that is no record (csrc/vrt_faces.h: face_record)");
    std::vector<int32_t> v(m.corners.size());
    for (size_t i = 0; i < v.size(); i++) {
        const int64_t p = ((int64_t)lo[i % 3u] + (int64_t)m.corners[i]) * 16;
        if (p < INT32_MIN || p > INT32_MAX) return fail(VRT_ERR_INVALID, "vrt_faces_mesh_host: lo puts a vertex beyond int32 sixteenths of a voxel");
        v[i] = (int32_t)p;
    }
    void* a = host_copy(v.data(), v.size() * 4u);
    void* b = host_copy(m.quads.data(), m.quads.size() * 4u);
    void* d = host_copy(m.ids.data(), m.ids.size());
    if (!a || !b || !d) { free(a); free(b); free(d); return fail(VRT_ERR_INVALID, "out of host memory"); }
    *vertices = (int32_t*)a; *nv = v.size() / 3u; *quads = (uint32_t*)b; *ids = (uint8_t*)d;
    return VRT_OK;
}

int vrt_faces_obj_host(const uint64_t* records, uint64_t n, const int32_t lo[3], const vrt_material palette[256], const char* mtl_name, void** obj,
                       size_t* nobj, void** mtl, size_t* nmtl)
{
    if ((!records && n) || !lo || !palette || !mtl_name || !obj || !nobj || !mtl || !nmtl) return fail(VRT_ERR_INVALID, "vrt_faces_obj_host: NULL argument");
    if (n > (1ull << 28)) return fail(VRT_ERR_INVALID, "vrt_faces_obj_host: more records than a box has");
    ObjWriter w;
    w.begin(mtl_name);
    if (!w.tile(records, n, lo)) return fail(VRT_ERR_INVALID, "vrt_faces_obj_host: a word that is no record (csrc/vrt_faces.h: face_record)");
    return obj_out(w, palette, obj, nobj, mtl, nmtl);
}

int vrt_scene_save_obj_mem(struct vrt_ctx* c, const vrt_scene* s, const char* mtl_name, uint32_t flags, void** obj, size_t* nobj, void** mtl, size_t* nmtl)
{
    if (!c || !s || !mtl_name || !obj || !nobj || !mtl || !nmtl) return fail(VRT_ERR_INVALID, "vrt_scene_save_obj_mem: NULL argument");
    ObjWriter w;
    std::vector<vrt_material> palette;
    const int rc = scene_save_obj(c, s, mtl_name, flags, w, palette);
    return rc != VRT_OK ? rc : obj_out(w, palette.data(), obj, nobj, mtl, nmtl);
}

int vrt_scene_save_obj_file(struct vrt_ctx* c, const vrt_scene* s, const char* path, uint32_t flags)
{
    if (!c || !s || !path || !*path) return fail(VRT_ERR_INVALID, "vrt_scene_save_obj_file: NULL argument");
    // the sibling .mtl: the path with its extension replaced (none: appended); the OBJ names it without its directory
    std::string mtl_path(path);
    const size_t slash = mtl_path.find_last_of('/'), dot = mtl_path.find_last_of('.');
    if (dot != std::string::npos && (slash == std::string::npos || dot > slash + 1u)) mtl_path.erase(dot);
    mtl_path += ".mtl";
    if (mtl_path == path) return fail(VRT_ERR_INVALID, "vrt_scene_save_obj_file: the path is that of its own .mtl");
    const std::string mtl_name = slash == std::string::npos ? mtl_path : mtl_path.substr(slash + 1u);
    ObjWriter w;
    std::vector<vrt_material> palette;
    const int rc = scene_save_obj(c, s, mtl_name.c_str(), flags, w, palette);
    if (rc != VRT_OK) return rc;
    const std::string files[2] = {path, mtl_path}, text[2] = {w.out, w.mtl(palette.data())};
    for (int k = 0; k < 2; k++) {
        FILE* f = fopen(files[k].c_str(), "wb");
        if (!f) return fail(VRT_ERR_IO, "Could not write mesh " + files[k]);
        const bool ok = fwrite(text[k].data(), 1, text[k].size(), f) == text[k].size();
        if (fclose(f) != 0 || !ok) return fail(VRT_ERR_IO, "Could not write mesh " + files[k]);
    }
    return VRT_OK;
}

} // extern "C"
