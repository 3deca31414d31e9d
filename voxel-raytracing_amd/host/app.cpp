// app.cpp -- offline counterpart of the reference's App (source/app.cpp:8-27, run/main.cpp:3): load a scene,
// set camera + settings, render through the C++ host mirror (voxels.hpp) and write the RGBA image.
// --rays IN --hits OUT [--ray-steps N]: no frame; the rays of IN (raw little-endian float32, n x 6: origin then direction) are
// traced through the loaded scene (VoxelScene::traceRays) and OUT receives per ray material (u8), pos (3 x f32), voxel (3 x i32),
// normal (3 x i8), packed in that order: 28 bytes.  With --segments a ray of IN has a seventh float, its distance limit t_max
// (VoxelScene::traceSegments), and a record of OUT ends with the hit's parameter t (f32): 32 bytes.
// --projection perspective:FOV | ortho:HALFWIDTH | panorama: the frame is drawn under that camera model (vrt_camera_rays over the
// --pos / --yaw / --pitch basis, then vrt_render_rays) instead of the built-in 90-degree pinhole; with --temporal it needs --reproject
// (the history is then kept by vrt_reproject_camera, with --upsample too at display resolution by vrt_upsample_camera); not with
// --devices.
// --fill X Y Z SX SY SZ ID (repeatable): the box is filled with ID (0 carves) before anything else looks at the scene
// (VoxelScene::fill).  --brush SHAPE:MODE:PARAMS:ID[:MATCH] (repeatable; applied in command-line order together with --fill):
// SHAPE box | sphere | ellipsoid | capsule, MODE set | paint | add | replace, PARAMS comma-separated in VOXEL units -- box
// x,y,z,sx,sy,sz (whole voxels); sphere cx,cy,cz,r; ellipsoid cx,cy,cz,rx,ry,rz; capsule ax,ay,az,bx,by,bz,r (multiples of 0.5;
// voxel (x, y, z) has its centre at x+.5, y+.5, z+.5) -- e.g. --brush sphere:paint:16,16,16,5.5:9 (VoxelScene::brush).  --save-vox OUT: the scene as it stands after that is written as a MagicaVoxel file (VoxelScene::save).
// --flood X,Y,Z:MATCH:CONN:ID[:LOX,LOY,LOZ:SX,SY,SZ] (repeatable, in command-line order with --fill and --brush): every voxel connected
// to the seed X,Y,Z becomes ID -- MATCH same | solid, CONN 6 | 26, inside the bounds if given, else in the whole volume
// (VoxelScene::flood); e.g. --flood 16,16,16:same:6:9 fills the cavity around (16, 16, 16).
// --voxelize FILE.obj:ID[:FILL[:MODE]] (repeatable, in command-line order with the others): the triangle mesh of a Wavefront OBJ file
// becomes ID -- FILL surface (default) | solid | both, MODE set (default) | paint | add -- inside the mesh's own bounds
// (VoxelScene::voxelize).  The reader is minimal: `v` and `f` lines, polygons as fans, negative indices, everything after a `/`
// ignored; coordinates are voxels.
// --morph OP:CONN:R[:ID[:solid][:LOX,LOY,LOZ:SX,SY,SZ]] (repeatable, in command-line order with the others): OP dilate | erode | open |
// close | hollow of the scene's solid by the ball of radius R (1..8) of CONN 6 | 26; added voxels become ID (dilate and close need
// one); `solid`: the cells outside the volume count as solid; inside the bounds if given, else in the whole volume
// (VoxelScene::morph); e.g. --morph hollow:6:1 leaves a shell one voxel thick of a voxelized solid.
// --components MATCH:CONN[:LOX,LOY,LOZ:SX,SY,SZ] (repeatable, in command-line order with the others): one line per connected component
// of the bounds (else the whole volume) -- MATCH solid | same | empty, CONN 6 | 26 -- in ascending order of its root
// (VoxelScene::components).  --despeckle N deletes every solid component below N voxels, --fill-cavities ID makes every region of air
// that touches no face of the volume ID, --keep-largest deletes every solid component but the largest (6-connectivity, the whole
// volume; VoxelScene::despeckle, fillCavities, keepLargest); they compose with --save-vox like the other edits.
// --save-obj OUT.obj: the surface of the scene as it stands after the edits as a Wavefront OBJ of quads in voxel coordinates, grouped
// by id, with its .mtl beside it (VoxelScene::saveObj).
// --read-box X Y Z SX SY SZ OUT: the ids of the box, x fastest, raw bytes (VoxelScene::read).  With any of these and no image output
// (--out, --raw, --png) no frame is rendered.
// Errors propagate as exceptions to run(), are printed, and the process exits with EXIT_FAILURE.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

#include "voxels.hpp"

using namespace vrt_host;

namespace {

std::vector<uint8_t> readFile(const std::string& path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("cannot open " + path);
    std::streamsize n = f.tellg(); f.seekg(0);
    std::vector<uint8_t> b((size_t)n);
    if (!f.read((char*)b.data(), n)) throw std::runtime_error("cannot read " + path);
    return b;
}

// "VRTD" dense-scene container written by the Python harness: dims, voxels, palette, sky, noise
std::shared_ptr<VoxelScene> loadDense(const std::shared_ptr<Engine>& engine, const std::string& path)
{
    std::vector<uint8_t> b = readFile(path);
    size_t o = 0;
    auto u32 = [&]() { uint32_t v; if (o + 4 > b.size()) throw std::runtime_error("truncated dense scene"); memcpy(&v, &b[o], 4); o += 4; return v; };
    if (b.size() < 4 || memcmp(b.data(), "VRTD", 4) != 0) throw std::runtime_error("not a VRTD file");
    o = 4;
    uint32_t W = u32(), H = u32(), D = u32();
    size_t nv = (size_t)W * H * D;
    if (o + nv + 256 * sizeof(vrt_material) > b.size()) throw std::runtime_error("truncated dense scene");
    const uint8_t* vox = &b[o]; o += nv;
    std::vector<vrt_material> pal(256); memcpy(pal.data(), &b[o], 256 * sizeof(vrt_material)); o += 256 * sizeof(vrt_material);
    auto scene = std::make_shared<VoxelScene>(engine, vox, W, H, D, pal.data());
    if (o < b.size()) { uint32_t w = u32(), h = u32(); std::vector<float> sky((size_t)w * h * 4); memcpy(sky.data(), &b[o], sky.size() * 4); o += sky.size() * 4; scene->setSkybox(sky.data(), w, h); }
    if (o < b.size()) { uint32_t w = u32(), h = u32(); scene->setBlueNoise(&b[o], w, h); o += (size_t)w * h * 4; }
    return scene;
}

// --brush SHAPE:MODE:PARAMS:ID[:MATCH]
vrt_brush parseBrush(const std::string& spec)
{
    auto split = [](const std::string& t, char sep) {
        std::vector<std::string> out; size_t at = 0;
        for (;;) { const size_t e = t.find(sep, at); out.push_back(t.substr(at, e == std::string::npos ? e : e - at)); if (e == std::string::npos) break; at = e + 1; }
        return out;
    };
    const std::vector<std::string> f = split(spec, ':');
    if (f.size() != 4 && f.size() != 5) throw std::runtime_error("--brush wants SHAPE:MODE:PARAMS:ID[:MATCH], got " + spec);
    vrt_brush b{};
    std::vector<double> v;
    for (const std::string& t : split(f[2], ',')) v.push_back(std::stod(t));
    auto want = [&](size_t n) { if (v.size() != n) throw std::runtime_error("--brush " + f[0] + " takes " + std::to_string(n) + " parameters"); };
    if (f[0] == "box") {
        want(6); b.shape = VRT_BRUSH_BOX;
        for (size_t a = 0; a < 6; a++) { if (v[a] != (double)(int32_t)v[a]) throw std::runtime_error("--brush box takes whole voxels"); b.p[a] = (int32_t)v[a]; }
    } else if (f[0] == "sphere") {
        want(4); b.shape = VRT_BRUSH_ELLIPSOID;
        for (size_t a = 0; a < 3; a++) { b.p[a] = VoxelScene::halfVoxels(v[a]); b.p[3 + a] = VoxelScene::halfVoxels(v[3]); }
    } else if (f[0] == "ellipsoid") {
        want(6); b.shape = VRT_BRUSH_ELLIPSOID;
        for (size_t a = 0; a < 6; a++) b.p[a] = VoxelScene::halfVoxels(v[a]);
    } else if (f[0] == "capsule") {
        want(7); b.shape = VRT_BRUSH_CAPSULE;
        for (size_t a = 0; a < 7; a++) b.p[a] = VoxelScene::halfVoxels(v[a]);
    } else throw std::runtime_error("--brush: unknown shape " + f[0]);
    if (f[1] == "set") b.mode = VRT_BRUSH_SET; else if (f[1] == "paint") b.mode = VRT_BRUSH_PAINT; else if (f[1] == "add") b.mode = VRT_BRUSH_ADD;
    else if (f[1] == "replace") b.mode = VRT_BRUSH_REPLACE; else throw std::runtime_error("--brush: unknown mode " + f[1]);
    const unsigned long id = std::stoul(f[3]), match = f.size() == 5 ? std::stoul(f[4]) : 0ul;
    if (id > 255 || match > 255) throw std::runtime_error("--brush: ids are 0..255");
    b.id = (uint8_t)id; b.match = (uint8_t)match;
    return b;
}

// --flood X,Y,Z:MATCH:CONN:ID[:LOX,LOY,LOZ:SX,SY,SZ]; without bounds size[0] stays 0 and the scene's dimensions are taken
vrt_flood parseFlood(const std::string& spec)
{
    auto split = [](const std::string& t, char sep) {
        std::vector<std::string> out; size_t at = 0;
        for (;;) { const size_t e = t.find(sep, at); out.push_back(t.substr(at, e == std::string::npos ? e : e - at)); if (e == std::string::npos) break; at = e + 1; }
        return out;
    };
    const std::vector<std::string> f = split(spec, ':');
    if (f.size() != 4 && f.size() != 6) throw std::runtime_error("--flood wants X,Y,Z:MATCH:CONN:ID[:LOX,LOY,LOZ:SX,SY,SZ], got " + spec);
    auto three = [&](const std::string& t) {
        const std::vector<std::string> v = split(t, ',');
        if (v.size() != 3) throw std::runtime_error("--flood: three comma-separated whole voxels, got " + t);
        return std::array<long long, 3>{std::stoll(v[0]), std::stoll(v[1]), std::stoll(v[2])};
    };
    vrt_flood fl{};
    const std::array<long long, 3> seed = three(f[0]);
    for (size_t a = 0; a < 3; a++) fl.seed[a] = (int32_t)seed[a];
    if (f[1] == "same") fl.match = VRT_FLOOD_SAME; else if (f[1] == "solid") fl.match = VRT_FLOOD_SOLID; else throw std::runtime_error("--flood: unknown match " + f[1]);
    fl.connectivity = std::stoi(f[2]);
    const unsigned long id = std::stoul(f[3]);
    if (id > 255) throw std::runtime_error("--flood: ids are 0..255");
    fl.id = (uint8_t)id;
    if (f.size() == 6) {
        const std::array<long long, 3> lo = three(f[4]), size = three(f[5]);
        for (size_t a = 0; a < 3; a++) {
            if (size[a] < 1 || size[a] > 0xFFFFFFFFll) throw std::runtime_error("--flood: a size of the bounds is outside 1..2^32-1");
            fl.lo[a] = (int32_t)lo[a]; fl.size[a] = (uint32_t)size[a];
        }
    }
    return fl;
}

// --morph OP:CONN:R[:ID[:solid][:LOX,LOY,LOZ:SX,SY,SZ]]; without bounds size[0] stays 0 and the scene's dimensions are taken
vrt_morph parseMorph(const std::string& spec)
{
    auto split = [](const std::string& t, char sep) {
        std::vector<std::string> out; size_t at = 0;
        for (;;) { const size_t e = t.find(sep, at); out.push_back(t.substr(at, e == std::string::npos ? e : e - at)); if (e == std::string::npos) break; at = e + 1; }
        return out;
    };
    const std::vector<std::string> f = split(spec, ':');
    const std::string want = "--morph wants OP:CONN:R[:ID[:solid][:LOX,LOY,LOZ:SX,SY,SZ]], got " + spec;
    if (f.size() < 3) throw std::runtime_error(want);
    vrt_morph m{};
    if (f[0] == "dilate") m.op = VRT_MORPH_DILATE; else if (f[0] == "erode") m.op = VRT_MORPH_ERODE; else if (f[0] == "open") m.op = VRT_MORPH_OPEN;
    else if (f[0] == "close") m.op = VRT_MORPH_CLOSE; else if (f[0] == "hollow") m.op = VRT_MORPH_HOLLOW; else throw std::runtime_error("--morph: unknown operation " + f[0]);
    m.connectivity = std::stoi(f[1]);
    m.radius = std::stoi(f[2]);
    size_t at = 3;
    if (at < f.size() && f[at] != "solid" && f[at].find(',') == std::string::npos) {
        const unsigned long id = std::stoul(f[at++]);
        if (id > 255) throw std::runtime_error("--morph: ids are 0..255");
        m.id = (uint8_t)id;
    }
    if (at < f.size() && f[at] == "solid") { m.flags |= VRT_MORPH_BORDER_SOLID; at++; }
    if (at == f.size()) return m;
    if (at + 2 != f.size()) throw std::runtime_error(want);
    for (size_t k = 0; k < 2; k++) {
        const std::vector<std::string> v = split(f[at + k], ',');
        if (v.size() != 3) throw std::runtime_error("--morph: three comma-separated whole voxels, got " + f[at + k]);
        for (size_t a = 0; a < 3; a++) {
            const long long t = std::stoll(v[a]);
            if (k == 1 && (t < 1 || t > 0xFFFFFFFFll)) throw std::runtime_error("--morph: a size of the bounds is outside 1..2^32-1");
            if (k == 0) m.lo[a] = (int32_t)t; else m.size[a] = (uint32_t)t;
        }
    }
    return m;
}

// --components MATCH:CONN[:LOX,LOY,LOZ:SX,SY,SZ]; without bounds size[0] stays 0 and the scene's dimensions are taken
vrt_components parseComponents(const std::string& spec)
{
    auto split = [](const std::string& t, char sep) {
        std::vector<std::string> out; size_t at = 0;
        for (;;) { const size_t e = t.find(sep, at); out.push_back(t.substr(at, e == std::string::npos ? e : e - at)); if (e == std::string::npos) break; at = e + 1; }
        return out;
    };
    const std::vector<std::string> f = split(spec, ':');
    if (f.size() != 2 && f.size() != 4) throw std::runtime_error("--components wants MATCH:CONN[:LOX,LOY,LOZ:SX,SY,SZ], got " + spec);
    vrt_components q{};
    if (f[0] == "solid") q.match = VRT_COMP_SOLID; else if (f[0] == "same") q.match = VRT_COMP_SAME; else if (f[0] == "empty") q.match = VRT_COMP_EMPTY;
    else throw std::runtime_error("--components: unknown match " + f[0]);
    q.connectivity = std::stoi(f[1]);
    for (size_t k = 0; k + 2 < f.size(); k++) {
        const std::vector<std::string> v = split(f[2 + k], ',');
        if (v.size() != 3) throw std::runtime_error("--components: three comma-separated whole voxels, got " + f[2 + k]);
        for (size_t a = 0; a < 3; a++) {
            const long long t = std::stoll(v[a]);
            if (k == 1 && (t < 1 || t > 0xFFFFFFFFll)) throw std::runtime_error("--components: a size of the bounds is outside 1..2^32-1");
            if (k == 0) q.lo[a] = (int32_t)t; else q.size[a] = (uint32_t)t;
        }
    }
    return q;
}

// --voxelize FILE.obj:ID[:FILL[:MODE]]
struct VoxelizeOp { std::vector<int32_t> vertices; std::vector<uint32_t> triangles; uint8_t id = 0; uint32_t fill = VRT_VOXELIZE_SURFACE; int32_t mode = VRT_BRUSH_SET; };

VoxelizeOp parseVoxelize(const std::string& spec)
{
    std::vector<std::string> f; size_t at = 0;
    for (;;) { const size_t e = spec.find(':', at); f.push_back(spec.substr(at, e == std::string::npos ? e : e - at)); if (e == std::string::npos) break; at = e + 1; }
    if (f.size() < 2 || f.size() > 4) throw std::runtime_error("--voxelize wants FILE.obj:ID[:FILL[:MODE]], got " + spec);
    VoxelizeOp op;
    const unsigned long id = std::stoul(f[1]);
    if (id > 255) throw std::runtime_error("--voxelize: ids are 0..255");
    op.id = (uint8_t)id;
    if (f.size() > 2) { if (f[2] == "surface") op.fill = VRT_VOXELIZE_SURFACE; else if (f[2] == "solid") op.fill = VRT_VOXELIZE_SOLID; else if (f[2] == "both") op.fill = VRT_VOXELIZE_SURFACE | VRT_VOXELIZE_SOLID; else throw std::runtime_error("--voxelize: unknown fill " + f[2]); }
    if (f.size() > 3) { if (f[3] == "set") op.mode = VRT_BRUSH_SET; else if (f[3] == "paint") op.mode = VRT_BRUSH_PAINT; else if (f[3] == "add") op.mode = VRT_BRUSH_ADD; else throw std::runtime_error("--voxelize: unknown mode " + f[3]); }
    std::ifstream in(f[0]);
    if (!in) throw std::runtime_error("--voxelize: cannot open " + f[0]);
    std::string line;
    while (std::getline(in, line)) {
        const size_t hash = line.find('#');
        if (hash != std::string::npos) line.resize(hash);
        std::istringstream ls(line);
        std::string key, w;
        if (!(ls >> key)) continue;
        if (key == "v") {
            for (int a = 0; a < 3; a++) { if (!(ls >> w)) throw std::runtime_error("--voxelize: a vertex needs three coordinates: " + line); op.vertices.push_back(VoxelScene::meshUnits((float)std::stod(w))); }
        } else if (key == "f") {
            std::vector<uint32_t> idx;
            const long long nv = (long long)(op.vertices.size() / 3);
            while (ls >> w) {
                const long long i = std::stoll(w.substr(0, w.find('/')));
                const long long k = i > 0 ? i - 1 : nv + i;
                if (k < 0 || k >= nv) throw std::runtime_error("--voxelize: face corner " + w + " names no vertex read so far");
                idx.push_back((uint32_t)k);
            }
            for (size_t k = 1; k + 1 < idx.size(); k++) { op.triangles.push_back(idx[0]); op.triangles.push_back(idx[k]); op.triangles.push_back(idx[k + 1]); }
        }
    }
    return op;
}

int run(int argc, char** argv)
{
    try {
        std::string vox, dense, out, raw, dumpPush, sky, noise, png, rays, hits; uint32_t raySteps = 512; bool segments = false;
        auto settings = std::make_shared<VoxelRenderSettings>();
        vec3 pos{8, 8, -50}; float yaw = 90, pitch = 0; bool havePos = false; int device = 0;
        std::vector<int> devices;                                          // --devices a,b,...: one process drives several GPUs
        int frames = 1; uint32_t windowW = 0, windowH = 0; float flyForward = 0, flyStrafe = 0, flyMouseX = 0; bool temporal = false, reproject = false, upsample = false;
        std::string dumpPushes, projection; std::vector<vrt_push> allPushes;
        struct Box { std::array<int32_t, 3> lo; std::array<uint32_t, 3> size; uint8_t id; };
        struct SceneOp { bool isBrush; Box box; vrt_brush brush; bool isFlood = false; vrt_flood flood{}; bool isVoxelize = false; VoxelizeOp voxelize{}; bool isMorph = false; vrt_morph morph{};
                         int comp = 0; vrt_components components{}; unsigned long compValue = 0; };   // --fill, --brush, --flood, --voxelize, --morph, --components, --despeckle, --fill-cavities and --keep-largest, in the order given (comp: 1 list, 2 despeckle, 3 fill cavities, 4 keep largest)
        std::vector<SceneOp> sceneOps; Box readBox{}; std::string saveVox, saveObj, readBoxOut;
        for (int i = 1; i < argc; i++) {
            std::string a = argv[i];
            auto next = [&]() { if (i + 1 >= argc) throw std::runtime_error("missing value for " + a); return std::string(argv[++i]); };
            if (a == "--vox") vox = next(); else if (a == "--dense") dense = next(); else if (a == "--out") out = next();
            else if (a == "--raw") raw = next(); else if (a == "--dump-push") dumpPush = next();
            else if (a == "--sky") sky = next(); else if (a == "--noise") noise = next(); else if (a == "--png") png = next();
            else if (a == "--rays") rays = next(); else if (a == "--hits") hits = next(); else if (a == "--ray-steps") raySteps = (uint32_t)std::stoul(next());
            else if (a == "--segments") segments = true;
            else if (a == "--fill" || a == "--read-box") {
                Box b{};
                for (int k = 0; k < 3; k++) b.lo[(size_t)k] = std::stoi(next());
                for (int k = 0; k < 3; k++) b.size[(size_t)k] = (uint32_t)std::stoul(next());
                if (a == "--fill") { b.id = (uint8_t)std::stoul(next()); sceneOps.push_back(SceneOp{false, b, vrt_brush{}}); } else { readBox = b; readBoxOut = next(); }
            }
            else if (a == "--brush") sceneOps.push_back(SceneOp{true, Box{}, parseBrush(next())});
            else if (a == "--flood") { SceneOp op{false, Box{}, vrt_brush{}}; op.isFlood = true; op.flood = parseFlood(next()); sceneOps.push_back(op); }
            else if (a == "--voxelize") { SceneOp op{false, Box{}, vrt_brush{}}; op.isVoxelize = true; op.voxelize = parseVoxelize(next()); sceneOps.push_back(op); }
            else if (a == "--morph") { SceneOp op{false, Box{}, vrt_brush{}}; op.isMorph = true; op.morph = parseMorph(next()); sceneOps.push_back(op); }
            else if (a == "--components") { SceneOp op{false, Box{}, vrt_brush{}}; op.comp = 1; op.components = parseComponents(next()); sceneOps.push_back(op); }
            else if (a == "--despeckle" || a == "--fill-cavities" || a == "--keep-largest") {
                SceneOp op{false, Box{}, vrt_brush{}};
                op.comp = a == "--despeckle" ? 2 : a == "--fill-cavities" ? 3 : 4;
                if (op.comp != 4) op.compValue = std::stoul(next());
                if (op.comp == 2 && op.compValue < 1) throw std::runtime_error("--despeckle wants N >= 1");
                if (op.comp == 3 && op.compValue > 255) throw std::runtime_error("--fill-cavities: ids are 0..255");
                sceneOps.push_back(op);
            }
            else if (a == "--save-vox") saveVox = next();
            else if (a == "--save-obj") saveObj = next();
            else if (a == "--width") settings->targetResolution[0] = (uint32_t)std::stoul(next());
            else if (a == "--height") settings->targetResolution[1] = (uint32_t)std::stoul(next());
            else if (a == "--pos") { pos.x = std::stof(next()); pos.y = std::stof(next()); pos.z = std::stof(next()); havePos = true; }
            else if (a == "--yaw") yaw = std::stof(next()); else if (a == "--pitch") pitch = std::stof(next());
            else if (a == "--no-fsr") settings->fsrSetttings.enable = false;
            else if (a == "--no-denoise") settings->denoiserSettings.enable = false;
            else if (a == "--iterations") settings->denoiserSettings.iterations = std::stoi(next());
            else if (a == "--ao") settings->occlusionSettings.numSamples = std::stoi(next());
            else if (a == "--bounces") settings->traceSettings.maxReflections = (uint32_t)std::stoul(next());
            else if (a == "--no-shadows") settings->traceSettings.shadows = false;
            else if (a == "--primary-only") { settings->occlusionSettings.numSamples = 0; settings->traceSettings.shadows = false; settings->traceSettings.maxReflections = 0; }
            else if (a == "--device") device = std::stoi(next());
            else if (a == "--devices") { std::string l = next(); size_t p0 = 0; while (p0 <= l.size()) { size_t c = l.find(',', p0); if (c == std::string::npos) c = l.size(); if (c > p0) devices.push_back(std::stoi(l.substr(p0, c - p0))); p0 = c + 1; } }
            else if (a == "--frames") frames = std::max(1, std::stoi(next()));                 // frames to run (update + render each)
            else if (a == "--temporal") temporal = true;                                       // accumulate jittered frames + upscale
            else if (a == "--reproject") reproject = true;                                     // with --temporal: keep the history under --fly (vrt_reproject)
            else if (a == "--upsample") upsample = true;                                       // with --temporal --reproject: the history at display resolution (vrt_upsample)
            else if (a == "--dump-pushes") dumpPushes = next();                                // every frame's push block, 96 bytes each
            else if (a == "--window") { windowW = (uint32_t)std::stoul(next()); windowH = (uint32_t)std::stoul(next()); }
            else if (a == "--projection") projection = next();
            else if (a == "--fly") { flyForward = std::stof(next()); flyStrafe = std::stof(next()); flyMouseX = std::stof(next()); }
            else throw std::runtime_error("unknown argument " + a);
        }
        if (segments && (rays.empty() || hits.empty())) throw std::runtime_error("--segments goes with --rays and --hits");
        if (!devices.empty() && !projection.empty()) throw std::runtime_error("--projection renders on one device (vrt_render_rays has no strips)");
        if (!devices.empty()) {
            // screen strips over the listed GPUs, RCCL gather to the first one (ShardedRenderer); the scene is loaded on each
            std::vector<std::shared_ptr<Engine>> engines; std::vector<std::shared_ptr<VoxelScene>> scenes;
            for (int d : devices) {
                auto e = std::make_shared<Engine>(d);
                std::shared_ptr<VoxelScene> sc = !dense.empty() ? loadDense(e, dense) : std::make_shared<VoxelScene>(e, vox.empty() ? settings->voxPath : vox);
                if (!sky.empty()) sc->setSkybox(sky);
                if (!noise.empty()) sc->setBlueNoise(noise);
                engines.push_back(e); scenes.push_back(sc);
            }
            VoxelRenderer cameraOnly(engines[0], settings, scenes[0]);                         // push constants as the single-GPU path builds them
            if (!havePos) pos = {scenes[0]->width / 2.0f, scenes[0]->height / 2.0f, -0.8f * scenes[0]->depth};
            cameraOnly.camera().position = pos; cameraOnly.camera().yaw = yaw; cameraOnly.camera().pitch = pitch;
            cameraOnly.camera().updateDirectionVectors();
            ShardedRenderer sharded(engines, settings, scenes);
            uint32_t res[2] = {0, 0};
            std::vector<uint8_t> img = sharded.render(cameraOnly.pushConstants(), &res[0], &res[1]);
            if (!raw.empty()) std::ofstream(raw, std::ios::binary).write((const char*)img.data(), (std::streamsize)img.size());
            if (!png.empty()) check(vrt_image_write_png(png.c_str(), img.data(), res[0], res[1]));
            std::printf("rendered %ux%u on %zu device(s), RCCL gather\n", res[0], res[1], devices.size());
            return EXIT_SUCCESS;
        }
        if (upsample && !(temporal && reproject)) throw std::runtime_error("--upsample needs --temporal --reproject");
        auto engine = std::make_shared<Engine>(device);
        std::shared_ptr<VoxelScene> scene;
        if (!dense.empty()) scene = loadDense(engine, dense);
        else scene = std::make_shared<VoxelScene>(engine, vox.empty() ? settings->voxPath : vox);
        if (!sky.empty()) scene->setSkybox(sky);
        if (!noise.empty()) scene->setBlueNoise(noise);
        for (const SceneOp& op : sceneOps) {
            if (op.isVoxelize) {
                const vrt_voxelize_result r = scene->voxelize(op.voxelize.vertices, op.voxelize.triangles, op.voxelize.id, op.voxelize.fill, op.voxelize.mode);
                std::printf("voxelize: %llu voxels covered, %llu changed, box %d %d %d + %u %u %u\n", (unsigned long long)r.covered, (unsigned long long)r.edit.changed,
                            r.edit.lo[0], r.edit.lo[1], r.edit.lo[2], r.edit.size[0], r.edit.size[1], r.edit.size[2]);
                continue;
            }
            if (op.comp == 1) {
                vrt_components q = op.components;
                if (q.size[0] == 0u) { q.size[0] = scene->width; q.size[1] = scene->height; q.size[2] = scene->depth; }
                vrt_components_result r{};
                const std::vector<vrt_component> rec = scene->components(q, &r);
                std::printf("components: %llu, %llu voxels, largest %llu\n", (unsigned long long)r.components, (unsigned long long)r.voxels, (unsigned long long)r.largest);
                for (size_t k = 0; k < rec.size(); k++)
                    std::printf("component %zu: root %d %d %d id %u voxels %llu box %d %d %d + %u %u %u faces %u\n", k, rec[k].root[0], rec[k].root[1], rec[k].root[2], rec[k].id,
                                (unsigned long long)rec[k].voxels, rec[k].lo[0], rec[k].lo[1], rec[k].lo[2], rec[k].size[0], rec[k].size[1], rec[k].size[2], rec[k].faces);
                continue;
            }
            if (op.comp != 0) {
                const vrt_filter_result r = op.comp == 2 ? scene->despeckle(op.compValue) : op.comp == 3 ? scene->fillCavities((uint8_t)op.compValue) : scene->keepLargest();
                std::printf("%s: %llu components of %llu voxels selected, %llu changed, box %d %d %d + %u %u %u\n",
                            op.comp == 2 ? "despeckle" : op.comp == 3 ? "fill-cavities" : "keep-largest", (unsigned long long)r.components, (unsigned long long)r.voxels,
                            (unsigned long long)r.edit.changed, r.edit.lo[0], r.edit.lo[1], r.edit.lo[2], r.edit.size[0], r.edit.size[1], r.edit.size[2]);
                continue;
            }
            if (op.isMorph) {
                vrt_morph m = op.morph;
                if (m.size[0] == 0u) { m.size[0] = scene->width; m.size[1] = scene->height; m.size[2] = scene->depth; }
                const vrt_morph_result r = scene->morph(m);
                std::printf("morph: %llu voxels added, %llu removed, box %d %d %d + %u %u %u\n", (unsigned long long)r.added, (unsigned long long)r.removed,
                            r.edit.lo[0], r.edit.lo[1], r.edit.lo[2], r.edit.size[0], r.edit.size[1], r.edit.size[2]);
                continue;
            }
            if (op.isFlood) {
                vrt_flood fl = op.flood;
                if (fl.size[0] == 0u) { fl.size[0] = scene->width; fl.size[1] = scene->height; fl.size[2] = scene->depth; }
                const vrt_flood_result r = scene->flood(fl);
                std::printf("flood: region of %llu voxels (id %u at the seed), %llu changed, box %d %d %d + %u %u %u\n", (unsigned long long)r.region, r.seed_id,
                            (unsigned long long)r.edit.changed, r.edit.lo[0], r.edit.lo[1], r.edit.lo[2], r.edit.size[0], r.edit.size[1], r.edit.size[2]);
                continue;
            }
            if (!op.isBrush) { scene->fill(op.box.lo, op.box.size, op.box.id); continue; }
            const vrt_brush_result r = scene->brush(op.brush);
            std::printf("brush: %llu voxels changed, box %d %d %d + %u %u %u\n", (unsigned long long)r.changed, r.lo[0], r.lo[1], r.lo[2], r.size[0], r.size[1], r.size[2]);
        }
        if (!saveVox.empty()) scene->save(saveVox);
        if (!saveObj.empty()) scene->saveObj(saveObj);
        if (!readBoxOut.empty()) {
            const std::vector<uint8_t> ids = scene->read(readBox.lo, readBox.size);
            std::ofstream f(readBoxOut, std::ios::binary);
            if (!f.write((const char*)ids.data(), (std::streamsize)ids.size())) throw std::runtime_error("cannot write " + readBoxOut);
        }
        if ((!saveVox.empty() || !saveObj.empty() || !readBoxOut.empty()) && out.empty() && raw.empty() && png.empty() && rays.empty() && hits.empty()) {
            std::printf("scene %ux%ux%u written\n", scene->width, scene->height, scene->depth);
            return EXIT_SUCCESS;
        }
        if (!rays.empty() || !hits.empty()) {
            if (rays.empty() || hits.empty()) throw std::runtime_error("--rays and --hits go together");
            const std::vector<uint8_t> in = readFile(rays);
            const size_t inRec = segments ? 28 : 24, outRec = segments ? 32 : 28;
            if (in.size() % inRec) throw std::runtime_error(rays + ": not a whole number of rays (" + std::to_string(inRec / 4) + " float32 each)");
            const size_t n = in.size() / inRec;
            std::vector<float> o(3 * n), d(3 * n), tMax(segments ? n : 0);
            for (size_t i = 0; i < n; i++) {
                memcpy(&o[3 * i], &in[inRec * i], 12); memcpy(&d[3 * i], &in[inRec * i + 12], 12);
                if (segments) memcpy(&tMax[i], &in[inRec * i + 24], 4);
            }
            VoxelScene::SegmentHits sh;
            if (segments) sh = scene->traceSegments(o, d, tMax, raySteps); else sh.hits = scene->traceRays(o, d, raySteps);
            const VoxelScene::RayHits& h = sh.hits;
            std::vector<uint8_t> rec(outRec * n);
            for (size_t i = 0; i < n; i++) {
                uint8_t* r = &rec[outRec * i];
                r[0] = h.material[i]; memcpy(r + 1, &h.pos[3 * i], 12); memcpy(r + 13, &h.voxel[3 * i], 12); memcpy(r + 25, &h.normal[3 * i], 3);
                if (segments) memcpy(r + 28, &sh.t[i], 4);
            }
            std::ofstream f(hits, std::ios::binary);
            if (!f.write((const char*)rec.data(), (std::streamsize)rec.size())) throw std::runtime_error("cannot write " + hits);
            std::printf("traced %zu rays scene %ux%ux%u\n", n, scene->width, scene->height, scene->depth);
            return EXIT_SUCCESS;
        }
        VoxelRenderer renderer(engine, settings, scene);
        if (!havePos) pos = {scene->width / 2.0f, scene->height / 2.0f, -0.8f * scene->depth};
        renderer.camera().position = pos; renderer.camera().yaw = yaw; renderer.camera().pitch = pitch;
        renderer.camera().updateDirectionVectors();
        if (!projection.empty()) {
            if (temporal && !reproject) throw std::runtime_error("--projection with --temporal needs --reproject (the pixel-by-pixel accumulation is wrong for a moving ray camera)");
            const size_t c = projection.find(':');
            const std::string kind = projection.substr(0, c), value = c == std::string::npos ? "" : projection.substr(c + 1);
            if (kind == "perspective" && !value.empty()) { renderer.projection = VRT_CAMERA_PERSPECTIVE; renderer.tanHalf = std::tan(std::stof(value) * 3.14159265358979323846f / 360.0f); }
            else if (kind == "ortho" && !value.empty()) { renderer.projection = VRT_CAMERA_ORTHOGRAPHIC; renderer.halfWidth = std::stof(value); }
            else if (kind == "panorama" && value.empty()) renderer.projection = VRT_CAMERA_PANORAMA;
            else throw std::runtime_error("--projection perspective:FOV | ortho:HALFWIDTH | panorama");
        }
        renderer.temporal = temporal; renderer.reproject = reproject; renderer.upsample = upsample; renderer.windowW = windowW; renderer.windowH = windowH;
        std::vector<uint8_t> img; uint32_t res[2] = {0, 0};
        const bool moving = flyForward != 0 || flyStrafe != 0 || flyMouseX != 0;
        for (int f = 0; f < frames; f++) {                                                     // App::run loop (source/app.cpp:18-27)
            if (frames > 1 || temporal) {
                if (flyMouseX != 0) renderer.camera().mouse(flyMouseX, 0.0f);
                renderer.update(1.0f / 60.0f, flyForward, flyStrafe);
                if (moving && !reproject) renderer.upscaler().reset();                         // no reprojection: history is per pose
            }
            allPushes.push_back(renderer.pushConstants());
            img = renderer.render(&res[0], &res[1]);
        }
        if (!dumpPush.empty()) { vrt_push p = renderer.pushConstants(); std::ofstream(dumpPush, std::ios::binary).write((const char*)&p, sizeof p); }
        if (!dumpPushes.empty()) std::ofstream(dumpPushes, std::ios::binary).write((const char*)allPushes.data(), (std::streamsize)(allPushes.size() * sizeof(vrt_push)));
        if (!raw.empty()) std::ofstream(raw, std::ios::binary).write((const char*)img.data(), (std::streamsize)img.size());
        if (!png.empty()) check(vrt_image_write_png(png.c_str(), img.data(), res[0], res[1]));
        if (!out.empty()) {
            std::ofstream f(out, std::ios::binary);
            f << "P6\n" << res[0] << " " << res[1] << "\n255\n";
            for (size_t i = 0; i < img.size(); i += 4) f.write((const char*)&img[i], 3);
        }
        std::printf("rendered %ux%u scene %ux%ux%u\n", res[0], res[1], scene->width, scene->height, scene->depth);
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return EXIT_FAILURE;
    }
    return EXIT_SUCCESS;
}

} // namespace

int main(int argc, char** argv) { return run(argc, argv); }
