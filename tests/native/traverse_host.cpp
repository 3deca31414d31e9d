// traverse_host.cpp -- TEST HELPER: compiles the product's traversal header (csrc/vrt_traverse.h over csrc/vrt_march_*.h) for the
// host so that its three strategies can be compared with the oracle on millions of rays without a GPU.
// Built on demand by tests/test_traverse_host.py with g++; never linked into libvrt_hip.so.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../voxel-raytracing_amd/csrc/vrt_traverse.h"

using namespace vrt;

struct HostVolume {
    VolumeView v;
    std::vector<uint8_t> vox;
    std::vector<uint64_t> o1, o2, o3;
    std::vector<uint8_t> df;
};

static void build_up(const std::vector<uint64_t>& lo, int lx, int ly, int lz, std::vector<uint64_t>& hi, int hx, int hy, int hz)
{
    hi.assign((size_t)hx * hy * hz, 0);
    for (int z = 0; z < lz; z++) for (int y = 0; y < ly; y++) for (int x = 0; x < lx; x++)
        if (lo[(size_t)x + ((size_t)y + (size_t)z * ly) * lx])
            hi[(size_t)(x >> 2) + ((size_t)(y >> 2) + (size_t)(z >> 2) * hy) * hx] |= 1ull << cell_bit(x, y, z);
}

extern "C" {

void* th_create(const uint8_t* vox, int W, int H, int D)
{
    HostVolume* h = new HostVolume();
    h->vox.assign(vox, vox + (size_t)W * H * D);
    VolumeView& v = h->v;
    v.W = W; v.H = H; v.D = D;
    v.n1x = (W + 3) / 4; v.n1y = (H + 3) / 4; v.n1z = (D + 3) / 4;
    v.n2x = (v.n1x + 3) / 4; v.n2y = (v.n1y + 3) / 4; v.n2z = (v.n1z + 3) / 4;
    v.n3x = (v.n2x + 3) / 4; v.n3y = (v.n2y + 3) / 4; v.n3z = (v.n2z + 3) / 4;
    h->o1.assign((size_t)v.n1x * v.n1y * v.n1z, 0);
    for (int z = 0; z < D; z++) for (int y = 0; y < H; y++) for (int x = 0; x < W; x++)
        if (h->vox[(size_t)x + ((size_t)y + (size_t)z * H) * W])
            h->o1[(size_t)(x >> 2) + ((size_t)(y >> 2) + (size_t)(z >> 2) * v.n1y) * v.n1x] |= 1ull << cell_bit(x, y, z);
    build_up(h->o1, v.n1x, v.n1y, v.n1z, h->o2, v.n2x, v.n2y, v.n2z);
    build_up(h->o2, v.n2x, v.n2y, v.n2z, h->o3, v.n3x, v.n3y, v.n3z);
    // clearance fields: per octant three one-sided 1-D min-max passes (same definition as k_df_pass, written independently)
    {
        const int CAP = 127;
        size_t stride = df_field_bytes(W, H, D);                 // padded x-fastest fields (vrt_volume.h df_index)
        h->df.assign(8 * stride, 0);
        std::vector<uint8_t> a((size_t)W * H * D), b((size_t)W * H * D);
        for (int o = 0; o < 8; o++) {
            int sg[3] = {(o & 1) ? 1 : -1, (o & 2) ? 1 : -1, (o & 4) ? 1 : -1};
            for (size_t i = 0; i < a.size(); i++) a[i] = h->vox[i] ? 0 : CAP + 1;
            for (int axis = 0; axis < 3; axis++) {
                for (int z = 0; z < D; z++) for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
                    size_t i = (size_t)x + ((size_t)y + (size_t)z * H) * W;
                    int pos = axis == 0 ? x : (axis == 1 ? y : z), dim = axis == 0 ? W : (axis == 1 ? H : D);
                    long long st = (axis == 0 ? 1 : (axis == 1 ? (long long)W : (long long)W * H)) * sg[axis];
                    int best = a[i];
                    for (int t = 1; t < best; t++) {
                        int q = pos + t * sg[axis];
                        int val = (q < 0 || q >= dim) ? 0 : a[(long long)i + t * st];
                        int m = val > t ? val : t;
                        if (m < best) best = m;
                    }
                    b[i] = (uint8_t)best;
                }
                a.swap(b);
            }
            for (int z = 0; z < D; z++) for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
                size_t i = (size_t)x + ((size_t)y + (size_t)z * H) * W;
                h->df[(size_t)o * stride + df_index(v, x, y, z)] = a[i] > CAP ? CAP : a[i];
            }
        }
        v.df_stride = stride;
    }
    v.df = h->df.data();
    v.vox = h->vox.data(); v.occ1 = h->o1.data(); v.occ2 = h->o2.data(); v.occ3 = h->o3.data();
    return h;
}

void th_destroy(void* p) { delete (HostVolume*)p; }

// the host's eligibility test for trace_df_fast's 32-bit layout, and the largest byte offset the loop can form for a volume
// (64-bit arithmetic; the test compares the two either side of 2^32)
int th_df_fast_layout_ok(int W, int H, int D) { return df_fast_layout_ok(W, H, D) ? 1 : 0; }
uint64_t th_df_fast_reach(int W, int H, int D)
{
    const uint64_t pwh = ((uint64_t)W + 2u) * ((uint64_t)H + 2u), stride = df_field_bytes(W, H, D);
    const uint64_t bias = pwh, sentinel = bias + 9u * stride;                    // trace_df_fast: bias, octoff + index, sentinel
    const uint64_t last_index = ((uint64_t)W + 2u) * ((uint64_t)H + 2u) * ((uint64_t)D + 2u) - 1u;
    const uint64_t id_read = bias + 8u * stride + last_index;                    // octoff + idx + voxoff
    const uint64_t prefetch = bias + 7u * stride + last_index + pwh;             // a live lane's index + one slice
    uint64_t m = sentinel;
    if (id_read > m) m = id_read;
    if (prefetch > m) m = prefetch;
    return m;
}

} // extern "C"

// ---- brick scenes: the two-level clearance of vrt_scene_from_bricks, built here by plain definitions -----------------------
// (an independent builder: the traversal only needs SOME lower bound of the true clearance, so the fields need not equal the
// device builder's -- the coarse field is the largest cube of empty bricks, the fine field the true clearance capped at 16)
struct HostBricks {
    VolumeView v;
    std::vector<uint32_t> grid;
    std::vector<uint8_t> coarse, pool, fine;
    std::vector<uint64_t> entry;
};

// clearance of every cell of a W x H x D occupancy (outside = solid) towards octant o, capped: three one-sided min-max passes
static std::vector<uint8_t> octant_clearance(const std::vector<uint8_t>& solid, int W, int H, int D, int o, int cap)
{
    std::vector<uint8_t> a((size_t)W * H * D), b((size_t)W * H * D);
    const int sg[3] = {(o & 1) ? 1 : -1, (o & 2) ? 1 : -1, (o & 4) ? 1 : -1};
    for (size_t i = 0; i < a.size(); i++) a[i] = solid[i] ? 0 : (uint8_t)(cap + 1);
    for (int axis = 0; axis < 3; axis++) {
        for (int z = 0; z < D; z++) for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
            const size_t i = (size_t)x + ((size_t)y + (size_t)z * H) * W;
            const int pos = axis == 0 ? x : (axis == 1 ? y : z), dim = axis == 0 ? W : (axis == 1 ? H : D);
            const long long st = (axis == 0 ? 1 : (axis == 1 ? (long long)W : (long long)W * H)) * sg[axis];
            int best = a[i];
            for (int t = 1; t < best; t++) {
                const int q = pos + t * sg[axis];
                const int val = (q < 0 || q >= dim) ? 0 : a[(long long)i + t * st];
                const int m = val > t ? val : t;
                if (m < best) best = m;
            }
            b[i] = (uint8_t)best;
        }
        a.swap(b);
    }
    for (auto& c : a) if (c > cap) c = (uint8_t)cap;
    return a;
}

extern "C" {

void* thb_create(const uint8_t* vox, int W, int H, int D)                // dimensions: multiples of 8
{
    HostBricks* h = new HostBricks();
    VolumeView& v = h->v;
    memset(&v, 0, sizeof v);
    v.W = W; v.H = H; v.D = D;
    const int nbx = W / 8, nby = H / 8, nbz = D / 8, pbx = nbx + 2, pby = nby + 2, pbz = nbz + 2;
    v.pbx = pbx; v.pby = pby;
    h->grid.assign((size_t)pbx * pby * pbz, 0xFFFFFFFFu);
    std::vector<uint8_t> occ((size_t)nbx * nby * nbz, 0), solid((size_t)W * H * D);
    for (size_t i = 0; i < solid.size(); i++) solid[i] = vox[i] != 0;
    std::vector<std::vector<uint8_t>> dense(8);
    for (int o = 0; o < 8; o++) dense[o] = octant_clearance(solid, W, H, D, o, 16);
    uint32_t n = 0;
    for (int bz = 0; bz < nbz; bz++) for (int by = 0; by < nby; by++) for (int bx = 0; bx < nbx; bx++) {
        bool any = false;
        for (int z = 0; z < 8 && !any; z++) for (int y = 0; y < 8 && !any; y++) for (int x = 0; x < 8; x++)
            if (vox[(size_t)(bx * 8 + x) + ((size_t)(by * 8 + y) + (size_t)(bz * 8 + z) * H) * W]) { any = true; break; }
        const size_t pi = (size_t)(bx + 1) + ((size_t)(by + 1) + (size_t)(bz + 1) * pby) * pbx;
        h->grid[pi] = any ? ++n : 0u;
        occ[(size_t)bx + ((size_t)by + (size_t)bz * nby) * nbx] = any;
        if (!any) continue;
        for (int z = 0; z < 8; z++) for (int y = 0; y < 8; y++) for (int x = 0; x < 8; x++)
            h->pool.push_back(vox[(size_t)(bx * 8 + x) + ((size_t)(by * 8 + y) + (size_t)(bz * 8 + z) * H) * W]);
        for (int o = 0; o < 8; o++)
            for (int z = 0; z < 8; z++) for (int y = 0; y < 8; y++) for (int x = 0; x < 8; x++)
                h->fine.push_back(dense[o][(size_t)(bx * 8 + x) + ((size_t)(by * 8 + y) + (size_t)(bz * 8 + z) * H) * W]);
    }
    const size_t cstride = (size_t)pbx * pby * pbz;
    h->coarse.assign(8 * cstride, 0);
    for (int o = 0; o < 8; o++) {
        std::vector<uint8_t> c = octant_clearance(occ, nbx, nby, nbz, o, 16);
        for (int bz = 0; bz < nbz; bz++) for (int by = 0; by < nby; by++) for (int bx = 0; bx < nbx; bx++)
            h->coarse[(size_t)o * cstride + (size_t)(bx + 1) + ((size_t)(by + 1) + (size_t)(bz + 1) * pby) * pbx] = c[(size_t)bx + ((size_t)by + (size_t)bz * nby) * nbx];
    }
    if (h->pool.empty()) { h->pool.push_back(0); h->fine.push_back(0); }
    h->entry.resize(cstride);
    for (size_t i = 0; i < cstride; i++) {
        uint8_t c8[8];
        for (int o = 0; o < 8; o++) c8[o] = h->coarse[(size_t)o * cstride + i];
        h->entry[i] = brick_entry_pack(h->grid[i], c8);
    }
    v.bentry = h->entry.data();
    v.bgrid = h->grid.data(); v.bcoarse = h->coarse.data(); v.bcoarse_stride = cstride; v.bpool = h->pool.data(); v.bfine = h->fine.data();
    return h;
}

void thb_destroy(void* p) { delete (HostBricks*)p; }

// the builder's clearance on its own (tests/test_scene_reference_cpu.py holds it against the definition in numpy)
void thb_octant_clearance(const uint8_t* solid, int W, int H, int D, int o, int cap, uint8_t* out)
{
    const std::vector<uint8_t> c = octant_clearance(std::vector<uint8_t>(solid, solid + (size_t)W * H * D), W, H, D, o, cap);
    memcpy(out, c.data(), c.size());
}

// same output record as th_trace; anyhit != 0: the any-hit form (only material and fetches are defined)
void thb_trace(void* p, int n, const float* starts, const float* dirs, uint32_t maxSteps, int anyhit, uint32_t* out, uint64_t* lookups)
{
    HostBricks* h = (HostBricks*)p;
    TraceStats total;
    for (int i = 0; i < n; i++) {
        f3 s = mk3(starts[i * 3], starts[i * 3 + 1], starts[i * 3 + 2]);
        f3 d = mk3(dirs[i * 3], dirs[i * 3 + 1], dirs[i * 3 + 2]);
        RayInt r;
        TraceStats st;
        if (anyhit) trace_brick<TraceStats, true>(h->v, s, d, maxSteps, r, st);
        else        trace_brick<TraceStats, false>(h->v, s, d, maxSteps, r, st);
        total.lookups += st.lookups;
        uint32_t* o = out + (size_t)i * 12;
        o[0] = r.material; o[1] = r.material ? r.mask : 0; o[2] = r.material ? (uint32_t)r.mx : 0; o[3] = r.material ? (uint32_t)r.my : 0;
        o[4] = r.material ? (uint32_t)r.mz : 0;
        o[5] = r.material ? f2u(r.side.x) : 0; o[6] = r.material ? f2u(r.side.y) : 0; o[7] = r.material ? f2u(r.side.z) : 0;
        o[8] = f2u(r.pos.x); o[9] = f2u(r.pos.y); o[10] = f2u(r.pos.z); o[11] = r.fetches;
    }
    if (lookups) *lookups = total.lookups;
}

// out per ray: 12 uint32: material, mask, mx,my,mz, side bits x3, p bits x3, fetches ; stats: 6 uint32 summed
void th_trace(void* p, int trav, int n, const float* starts, const float* dirs, uint32_t maxSteps, uint32_t* out, uint64_t* stats)
{
    HostVolume* h = (HostVolume*)p;
    TraceStats total;
    for (int i = 0; i < n; i++) {
        f3 s = mk3(starts[i * 3], starts[i * 3 + 1], starts[i * 3 + 2]);
        f3 d = mk3(dirs[i * 3], dirs[i * 3 + 1], dirs[i * 3 + 2]);
        RayInt r;
        if (trav == VRT_TRAVERSAL_JUMP) {
            TraceStats st;
            trace_jump(h->v, h->v.occ2, h->v.occ3, s, d, maxSteps, r, st);
            total.literal += st.literal; total.jumps1 += st.jumps1; total.jumps2 += st.jumps2; total.jumps3 += st.jumps3;
            total.retrace += st.retrace; total.lookups += st.lookups;
        } else if (trav == VRT_TRAVERSAL_BITMASK) {
            trace_literal<VRT_TRAVERSAL_BITMASK>(h->v, h->v.occ2, s, d, maxSteps, r);
        } else if (trav == VRT_TRAVERSAL_DFJ) {
            TraceStats st;
            trace_dfj(h->v, s, d, maxSteps, r, st);
            total.jumps1 += st.jumps1; total.jumps3 += st.jumps3; total.lookups += st.lookups; total.retrace += st.retrace;
        } else if (trav == VRT_TRAVERSAL_DF) {
            TraceStats st;
            trace_df(h->v, s, d, maxSteps, r, st);
            total.jumps1 += st.jumps1; total.jumps2 += st.jumps2; total.lookups += st.lookups;
        } else {
            trace_literal<VRT_TRAVERSAL_DENSE>(h->v, h->v.occ2, s, d, maxSteps, r);
        }
        uint32_t* o = out + (size_t)i * 12;
        o[0] = r.material; o[1] = r.material ? r.mask : 0; o[2] = r.material ? (uint32_t)r.mx : 0; o[3] = r.material ? (uint32_t)r.my : 0;
        o[4] = r.material ? (uint32_t)r.mz : 0;
        o[5] = r.material ? f2u(r.side.x) : 0; o[6] = r.material ? f2u(r.side.y) : 0; o[7] = r.material ? f2u(r.side.z) : 0;
        o[8] = f2u(r.pos.x); o[9] = f2u(r.pos.y); o[10] = f2u(r.pos.z); o[11] = r.fetches;
    }
    if (stats) { stats[0] = total.literal; stats[1] = total.jumps1; stats[2] = total.jumps2; stats[3] = total.jumps3; stats[4] = total.retrace; stats[5] = total.lookups; }
}

} // extern "C"
