// vrt_scene_edit.hip -- scene edit kernels for gfx950 (vrt_scene_edit_box) and the host-side plan of their launches.
#include "vrt_device_common.h"

namespace vrt {

// ---------------------------------------------------------------------------------------------
// scene edits (vrt_scene_edit_box): a box of voxels is rewritten and only the bytes it can have changed are recomputed.
// vrt_edit.h has the regions (R_o, E, Q_o) and why nothing else changes; the results equal a fresh build byte for byte.
//   k_edit_write      the box's ids into the volume (and into field 8 where the layout has it)
//   k_edit_occ1/_up   the pyramid words the box overlaps
//   k_edit_pass_x     clearance pass x over R_x(sx) x E_y x E_z for both signs of x: one wave per line, the distance to the next
//                     solid from a ballot of 64 voxels and a carry from the chunk beyond (no look-up loop at all)
//   k_edit_pass_lds   clearance passes y (4 sign pairs) and z (8 octants): 64 lines along x side by side with their whole scanned
//                     extent in LDS (64 B rows: a wave's look-up is one conflict-free row), the min-max loop of k_df_pass on LDS,
//                     stores of whole 64 B rows -- pass z straight into the octant's zero-bordered field
//   k_edit_open_scan/_x   the open cells of Q_o: the three AND scans of launch_open_cells restricted to Q_o, each seeded with the
//                     (unchanged) open state of the cells just beyond Q_o's far faces, which stands for everything further out
// Every intermediate is clamped to cap (min and max commute with the clamp), so a look-up never reaches beyond cap - 1.
// ---------------------------------------------------------------------------------------------

static_assert(VRT_EDIT_CAP == VRT_DF_CAP, "vrt_edit.h states the regions for the dense scene's cap");

__device__ __forceinline__ size_t edit_pidx(int x, int y, int z, int W, int H)     // index into a zero-bordered field
{
    return (size_t)(x + 1) + ((size_t)(y + 1) + (size_t)(z + 1) * ((size_t)H + 2u)) * ((size_t)W + 2u);
}

// blockIdx.y / .z: y and z within the box.  ids == nullptr: every voxel gets `id`
__global__ __launch_bounds__(256) void k_edit_write(uint8_t* __restrict__ vox, uint8_t* __restrict__ field8, const EditBox B,
                                                    const uint8_t* __restrict__ ids, int id)
{
    const int nx = B.hi[0] - B.lo[0], ny = B.hi[1] - B.lo[1];
    const int bx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (bx >= nx) return;
    const int x = B.lo[0] + bx, y = B.lo[1] + (int)blockIdx.y, z = B.lo[2] + (int)blockIdx.z;
    const uint8_t v = ids ? ids[(size_t)bx + ((size_t)blockIdx.y + (size_t)blockIdx.z * (size_t)ny) * (size_t)nx] : (uint8_t)id;
    vox[(size_t)x + ((size_t)y + (size_t)z * (size_t)B.H) * (size_t)B.W] = v;
    if (field8) field8[edit_pidx(x, y, z, B.W, B.H)] = v;
}

// k_build_occ1 / k_build_occ_up for the words [c0, c0 + n) of each axis
__global__ void k_edit_occ1(const uint8_t* __restrict__ vox, int W, int H, int D, uint64_t* __restrict__ occ1, int n1x, int n1y,
                            int c0x, int c0y, int c0z, int ncx)
{
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= ncx) return;
    const int cx = c0x + t, cy = c0y + (int)blockIdx.y, cz = c0z + (int)blockIdx.z;
    uint64_t w = 0;
    for (int z = 0; z < 4; z++) {
        const int vz = cz * 4 + z;
        if (vz >= D) break;
        for (int y = 0; y < 4; y++) {
            const int vy = cy * 4 + y;
            if (vy >= H) break;
            const size_t base = (size_t)cx * 4 + ((size_t)vy + (size_t)vz * H) * W;
            for (int x = 0; x < 4; x++)
                if (cx * 4 + x < W && vox[base + x] != 0) w |= 1ull << (x | (y << 2) | (z << 4));
        }
    }
    occ1[(size_t)cx + ((size_t)cy + (size_t)cz * n1y) * n1x] = w;
}

__global__ void k_edit_occ_up(const uint64_t* __restrict__ lo, int lx, int ly, int lz, uint64_t* __restrict__ hi, int hx, int hy,
                              int c0x, int c0y, int c0z, int ncx)
{
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= ncx) return;
    const int cx = c0x + t, cy = c0y + (int)blockIdx.y, cz = c0z + (int)blockIdx.z;
    uint64_t w = 0;
    for (int z = 0; z < 4; z++) {
        const int vz = cz * 4 + z;
        if (vz >= lz) break;
        for (int y = 0; y < 4; y++) {
            const int vy = cy * 4 + y;
            if (vy >= ly) break;
            for (int x = 0; x < 4; x++) {
                const int vx = cx * 4 + x;
                if (vx < lx && lo[(size_t)vx + ((size_t)vy + (size_t)vz * ly) * lx] != 0) w |= 1ull << (x | (y << 2) | (z << 4));
            }
        }
    }
    hi[(size_t)cx + ((size_t)cy + (size_t)cz * hy) * hx] = w;
}

hipError_t launch_edit_write(uint8_t* vox, uint8_t* field8, const EditBox& b, const uint8_t* ids_dev, int id, hipStream_t s)
{
    const int nx = b.hi[0] - b.lo[0], ny = b.hi[1] - b.lo[1], nz = b.hi[2] - b.lo[2];
    hipLaunchKernelGGL(k_edit_write, dim3((unsigned)((nx + 255) / 256), (unsigned)ny, (unsigned)nz), dim3(256), 0, s, vox, field8, b, ids_dev, id);
    return hipGetLastError();
}

hipError_t launch_edit_pyramid(const uint8_t* vox, const EditBox& b, uint64_t* occ1, uint64_t* occ2, uint64_t* occ3, hipStream_t s)
{
    const int n1x = (b.W + 3) / 4, n1y = (b.H + 3) / 4, n1z = (b.D + 3) / 4;
    const int n2x = (n1x + 3) / 4, n2y = (n1y + 3) / 4, n2z = (n1z + 3) / 4;
    const int n3x = (n2x + 3) / 4, n3y = (n2y + 3) / 4;
    int c0[3], n[3];
    for (int a = 0; a < 3; a++) { c0[a] = b.lo[a] >> 2; n[a] = ((b.hi[a] - 1) >> 2) - c0[a] + 1; }
    hipLaunchKernelGGL(k_edit_occ1, dim3((unsigned)((n[0] + 63) / 64), (unsigned)n[1], (unsigned)n[2]), dim3(64), 0, s, vox, b.W, b.H, b.D, occ1, n1x, n1y,
                       c0[0], c0[1], c0[2], n[0]);
    for (int a = 0; a < 3; a++) { c0[a] = b.lo[a] >> 4; n[a] = ((b.hi[a] - 1) >> 4) - c0[a] + 1; }
    hipLaunchKernelGGL(k_edit_occ_up, dim3((unsigned)((n[0] + 63) / 64), (unsigned)n[1], (unsigned)n[2]), dim3(64), 0, s, (const uint64_t*)occ1, n1x, n1y, n1z,
                       occ2, n2x, n2y, c0[0], c0[1], c0[2], n[0]);
    for (int a = 0; a < 3; a++) { c0[a] = b.lo[a] >> 6; n[a] = ((b.hi[a] - 1) >> 6) - c0[a] + 1; }
    hipLaunchKernelGGL(k_edit_occ_up, dim3((unsigned)((n[0] + 63) / 64), (unsigned)n[1], (unsigned)n[2]), dim3(64), 0, s, (const uint64_t*)occ2, n2x, n2y, n2z,
                       occ3, n3x, n3y, c0[0], c0[1], c0[2], n[0]);
    return hipGetLastError();
}

// pass x for both signs (blockIdx.y: 0 = -x, 1 = +x): lines E_y x E_z, results for x in R_x(sign), x-fastest and compact
struct EditPassX {
    const uint8_t* vox;
    uint8_t* dst[2];
    int W, H;
    int xr_lo[2], xr_hi[2];
    int ey_lo, ny, ez_lo, nz;
    int cap;
};

__global__ __launch_bounds__(256) void k_edit_pass_x(const EditPassX P)
{
    const int lane = (int)(threadIdx.x & 63u);
    const size_t line = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (line >= (size_t)P.ny * (size_t)P.nz) return;           // wave-uniform
    const int si = (int)blockIdx.y, cap = P.cap;
    const int ly = (int)(line % (size_t)P.ny), lz = (int)(line / (size_t)P.ny);
    const uint8_t* row = P.vox + ((size_t)(P.ey_lo + ly) + (size_t)(P.ez_lo + lz) * (size_t)P.H) * (size_t)P.W;
    const int xa = P.xr_lo[si], xb = P.xr_hi[si];
    uint8_t* out = P.dst[si] + line * (size_t)(xb - xa);
    // the scanned span: R_x and cap - 1 voxels beyond it towards the sign; what lies beyond the span is at least cap away from
    // every cell of R_x, which is all the carry has to say
    const int s0 = si ? xa : xa - (cap - 1), s1 = si ? xb + (cap - 1) : xb;
    const int chunks = (s1 - s0 + 63) / 64;
    int carry = cap;                                           // distance from the first voxel beyond the chunk to the next solid, clamped
    for (int c = 0; c < chunks; c++) {
        const int x = s0 + (si ? chunks - 1 - c : c) * 64 + lane;
        const bool solid = (x < 0 || x >= P.W) ? true : row[x] != 0;       // outside the volume counts as solid
        const uint64_t mask = __ballot(solid);
        int d;
        if (si) {
            const uint64_t m = mask >> lane;
            d = m ? __ffsll((long long)m) - 1 : (64 - lane) + carry;
            carry = mask ? __ffsll((long long)mask) - 1 : 64 + carry;
        } else {
            const uint64_t m = mask << (63 - lane);
            d = m ? __clzll((long long)m) : (lane + 1) + carry;
            carry = mask ? __clzll((long long)mask) : 64 + carry;
        }
        carry = carry < cap ? carry : cap;
        if (x >= xa && x < xb) out[x - xa] = (uint8_t)(d < cap ? d : cap);
    }
}

// passes y and z: workgroup = 64 lines along x (lane = x) x the whole scanned extent of the source, staged in LDS; out of the
// source's extent is out of the volume (E is clipped by nothing else), i.e. solid
#define VRT_EDIT_LDS_ROWS (VRT_EDIT_MAX_SIDE + 2 * (VRT_EDIT_CAP - 1))
struct EditPassL {
    const uint8_t* src;
    uint8_t* dst;
    int nx, n_scan;                   // lanes in all; the source's extent along the scanned axis
    size_t src_scan, src_other;       // source strides along the scanned axis and across the lines (blockIdx.y)
    int out_lo, n_out;                // scanned positions [out_lo, out_lo + n_out) are written
    size_t dst_scan, dst_other;
    int dir, cap;
};

__global__ __launch_bounds__(256) void k_edit_pass_lds(const EditPassL P)
{
    __shared__ uint8_t L[VRT_EDIT_LDS_ROWS * 64];
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    const int x = (int)blockIdx.x * 64 + lane;
    const bool live = x < P.nx;
    const uint8_t* s = P.src + (size_t)blockIdx.y * P.src_other + (size_t)x;
    for (int t = w; t < P.n_scan; t += 4) L[t * 64 + lane] = live ? s[(size_t)t * P.src_scan] : (uint8_t)0;
    __syncthreads();
    uint8_t* d = P.dst + (size_t)blockIdx.y * P.dst_other + (size_t)x;
    for (int k = w; k < P.n_out; k += 4) {
        const int p = P.out_lo + k;
        int best = L[p * 64 + lane];
        for (int t = 1; t < best; t++) {
            const int q = p + t * P.dir;
            const int val = (q < 0 || q >= P.n_scan) ? 0 : (int)L[q * 64 + lane];
            const int m = val > t ? val : t;
            best = best < m ? best : m;
        }
        if (live) d[(size_t)k * P.dst_scan] = (uint8_t)best;
    }
}

// open cells of Q_o.  Scans along y (axis 1; blockIdx.y = z within Q) and z (axis 2; blockIdx.y = y within Q), one thread per
// x of Q; the flag starts as the open state -- in the field as it stands: those cells are outside Q_o -- of the cell just beyond
// Q_o's far face on that axis (true where that is outside the volume), which speaks for the whole corner box beyond it.
struct EditOpen {
    const uint8_t* vox;
    uint8_t* field;                   // the octant's zero-bordered field
    uint8_t *tmp0, *tmp1;             // |Q_o| bytes each, x-fastest
    int W, H, D;
    int q_lo[3], q_n[3];              // Q_o
    int r_lo[3], r_hi[3];             // R_o
    int sgn[3];
    int cap;
    int mark;                         // 0: open = the code 0 (dense scenes); else the bit beside the clearance that says open (brick lattice: 0x80)
};

__device__ __forceinline__ bool edit_open_before(const EditOpen& P, int x, int y, int z)
{
    if (x < 0 || y < 0 || z < 0 || x >= P.W || y >= P.H || z >= P.D) return true;
    if (P.mark) return (P.field[edit_pidx(x, y, z, P.W, P.H)] & (uint8_t)P.mark) != 0;
    return P.field[edit_pidx(x, y, z, P.W, P.H)] == 0 && P.vox[(size_t)x + ((size_t)y + (size_t)z * (size_t)P.H) * (size_t)P.W] == 0;
}

__global__ __launch_bounds__(256) void k_edit_open_scan(const EditOpen P, int axis)
{
    const int qx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (qx >= P.q_n[0]) return;
    const int len = P.q_n[axis], dir = P.sgn[axis], o = (int)blockIdx.y;
    const size_t nx = (size_t)P.q_n[0], nxy = nx * (size_t)P.q_n[1];
    const size_t step = axis == 1 ? nx : nxy;
    const size_t base = (size_t)qx + (axis == 1 ? (size_t)o * nxy : (size_t)o * nx);
    const int x = P.q_lo[0] + qx;
    const int beyond = dir > 0 ? P.q_lo[axis] + len : P.q_lo[axis] - 1;
    uint8_t flag = axis == 1 ? (uint8_t)edit_open_before(P, x, beyond, P.q_lo[2] + o) : (uint8_t)edit_open_before(P, x, P.q_lo[1] + o, beyond);
    for (int t = 0; t < len; t++) {                            // from the far end of the line towards the near one
        const int k = dir > 0 ? len - 1 - t : t;
        const size_t i = base + (size_t)k * step;
        if (axis == 1) flag &= (uint8_t)(P.vox[(size_t)x + ((size_t)(P.q_lo[1] + k) + (size_t)(P.q_lo[2] + o) * (size_t)P.H) * (size_t)P.W] == 0);
        else           flag &= P.tmp0[i];
        (axis == 1 ? P.tmp0 : P.tmp1)[i] = flag;
    }
}

// the scan along x, one wave per line of Q_o, and the bytes that follow from it (vrt_edit.h): 0 where the cell is open now; the
// wall clearance where a cell outside R_o was open and is not any more; R_o otherwise holds what pass z has just written
__global__ __launch_bounds__(256) void k_edit_open_x(const EditOpen P)
{
    const int lane = (int)(threadIdx.x & 63u);
    const size_t line = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (line >= (size_t)P.q_n[1] * (size_t)P.q_n[2]) return;   // wave-uniform
    const int y = P.q_lo[1] + (int)(line % (size_t)P.q_n[1]), z = P.q_lo[2] + (int)(line / (size_t)P.q_n[1]);
    const int dir = P.sgn[0], nx = P.q_n[0];
    const uint8_t* row = P.tmp1 + line * (size_t)nx;
    const bool yz_in_r = y >= P.r_lo[1] && y < P.r_hi[1] && z >= P.r_lo[2] && z < P.r_hi[2];
    bool carry = edit_open_before(P, dir > 0 ? P.q_lo[0] + nx : P.q_lo[0] - 1, y, z);
    const int chunks = (nx + 63) / 64;
    for (int c = 0; c < chunks; c++) {
        const int qx = (dir > 0 ? chunks - 1 - c : c) * 64 + lane;
        const bool f = qx < nx ? row[qx] != 0 : true;
        const uint64_t blocked = ~__ballot(f);
        const bool open = carry && f && (dir > 0 ? (blocked >> lane) == 0ull : (blocked << (63 - lane)) == 0ull);
        carry = carry && blocked == 0ull;
        if (qx >= nx) continue;
        const int x = P.q_lo[0] + qx;
        uint8_t* cell = P.field + edit_pidx(x, y, z, P.W, P.H);
        if (P.mark) { *cell = open ? (uint8_t)(*cell | (uint8_t)P.mark) : (uint8_t)(*cell & (uint8_t)~P.mark); continue; }
        if (open) { *cell = 0; continue; }
        if (yz_in_r && x >= P.r_lo[0] && x < P.r_hi[0]) continue;
        if (*cell == 0 && P.vox[(size_t)x + ((size_t)y + (size_t)z * (size_t)P.H) * (size_t)P.W] == 0)
            *cell = (uint8_t)edit_wall_clearance(x, y, z, P.W, P.H, P.D, P.sgn[0], P.sgn[1], P.sgn[2], P.cap);
    }
}

namespace {
struct EditPlan {
    EditSpan e[3], r[3][2];           // E; R per axis and sign (0: -, 1: +)
    size_t x_bytes[2], y_bytes[2][2];
    size_t clear_bytes, open_bytes;   // open_bytes: one of the two buffers of the open scans (the largest Q_o)
};
EditPlan edit_plan(const EditBox& b)
{
    EditPlan p;
    const int dim[3] = {b.W, b.H, b.D};
    for (int a = 0; a < 3; a++) {
        p.e[a] = edit_span_e(b.lo[a], b.hi[a], dim[a], VRT_EDIT_CAP);
        for (int si = 0; si < 2; si++) p.r[a][si] = edit_span_r(b.lo[a], b.hi[a], dim[a], si ? 1 : -1, VRT_EDIT_CAP);
    }
    const size_t ney = (size_t)(p.e[1].hi - p.e[1].lo), nez = (size_t)(p.e[2].hi - p.e[2].lo);
    p.clear_bytes = 0; p.open_bytes = 0;
    for (int sx = 0; sx < 2; sx++) {
        const size_t nx = (size_t)(p.r[0][sx].hi - p.r[0][sx].lo);
        p.x_bytes[sx] = (nx * ney * nez + 255u) & ~(size_t)255u;
        p.clear_bytes += p.x_bytes[sx];
        for (int sy = 0; sy < 2; sy++) {
            p.y_bytes[sx][sy] = (nx * (size_t)(p.r[1][sy].hi - p.r[1][sy].lo) * nez + 255u) & ~(size_t)255u;
            p.clear_bytes += p.y_bytes[sx][sy];
        }
    }
    for (int o = 0; o < 8; o++) {
        size_t n = 1;
        for (int a = 0; a < 3; a++) { const EditSpan q = edit_span_q(b.lo[a], b.hi[a], dim[a], ((o >> a) & 1) ? 1 : -1); n *= (size_t)(q.hi - q.lo); }
        n = (n + 255u) & ~(size_t)255u;
        p.open_bytes = n > p.open_bytes ? n : p.open_bytes;
    }
    return p;
}
} // namespace

size_t edit_scratch_bytes(const EditBox& b, bool open)
{
    const EditPlan p = edit_plan(b);
    const size_t ob = open ? 2 * p.open_bytes : 0;
    return p.clear_bytes > ob ? p.clear_bytes : ob;
}

// df: the scene's fields as they were before the edit; vox: the volume AFTER it (launch_edit_write); scratch: edit_scratch_bytes
hipError_t launch_edit_fields(const uint8_t* vox, const EditBox& b, uint8_t* df, size_t stride, uint8_t* scratch, bool open, hipStream_t s)
{
    const EditPlan p = edit_plan(b);
    const int cap = VRT_EDIT_CAP;
    const int ney = p.e[1].hi - p.e[1].lo, nez = p.e[2].hi - p.e[2].lo;
    uint8_t *tx[2], *ty[2][2];
    {
        uint8_t* q = scratch;
        for (int sx = 0; sx < 2; sx++) { tx[sx] = q; q += p.x_bytes[sx]; }
        for (int sx = 0; sx < 2; sx++) for (int sy = 0; sy < 2; sy++) { ty[sx][sy] = q; q += p.y_bytes[sx][sy]; }
    }
    {
        EditPassX P;
        P.vox = vox; P.W = b.W; P.H = b.H; P.cap = cap;
        for (int sx = 0; sx < 2; sx++) { P.dst[sx] = tx[sx]; P.xr_lo[sx] = p.r[0][sx].lo; P.xr_hi[sx] = p.r[0][sx].hi; }
        P.ey_lo = p.e[1].lo; P.ny = ney; P.ez_lo = p.e[2].lo; P.nz = nez;
        const size_t lines = (size_t)ney * (size_t)nez;
        hipLaunchKernelGGL(k_edit_pass_x, dim3((unsigned)((lines + 3) / 4), 2), dim3(256), 0, s, P);
    }
    for (int sx = 0; sx < 2; sx++) {
        const int nx = p.r[0][sx].hi - p.r[0][sx].lo;
        for (int sy = 0; sy < 2; sy++) {
            const EditSpan ry = p.r[1][sy];
            EditPassL P;
            P.src = tx[sx]; P.dst = ty[sx][sy]; P.nx = nx; P.n_scan = ney;
            P.src_scan = (size_t)nx; P.src_other = (size_t)nx * (size_t)ney;
            P.out_lo = ry.lo - p.e[1].lo; P.n_out = ry.hi - ry.lo;
            P.dst_scan = (size_t)nx; P.dst_other = (size_t)nx * (size_t)P.n_out;
            P.dir = sy ? 1 : -1; P.cap = cap;
            hipLaunchKernelGGL(k_edit_pass_lds, dim3((unsigned)((nx + 63) / 64), (unsigned)nez), dim3(256), 0, s, P);
        }
    }
    for (int o = 0; o < 8; o++) {
        const int sx = o & 1, sy = (o >> 1) & 1, sz = (o >> 2) & 1;
        const EditSpan rx = p.r[0][sx], ry = p.r[1][sy], rz = p.r[2][sz];
        const int nx = rx.hi - rx.lo, ny = ry.hi - ry.lo;
        EditPassL P;
        P.src = ty[sx][sy]; P.nx = nx; P.n_scan = nez;
        P.src_scan = (size_t)nx * (size_t)ny; P.src_other = (size_t)nx;
        P.out_lo = rz.lo - p.e[2].lo; P.n_out = rz.hi - rz.lo;
        P.dst = df + (size_t)o * stride + (size_t)(rx.lo + 1) + ((size_t)(ry.lo + 1) + (size_t)(rz.lo + 1) * ((size_t)b.H + 2u)) * ((size_t)b.W + 2u);
        P.dst_scan = ((size_t)b.W + 2u) * ((size_t)b.H + 2u); P.dst_other = (size_t)b.W + 2u;
        P.dir = sz ? 1 : -1; P.cap = cap;
        hipLaunchKernelGGL(k_edit_pass_lds, dim3((unsigned)((nx + 63) / 64), (unsigned)ny), dim3(256), 0, s, P);
    }
    if (open) {
        const int dim[3] = {b.W, b.H, b.D};
        for (int o = 0; o < 8; o++) {
            EditOpen P;
            P.vox = vox; P.field = df + (size_t)o * stride; P.tmp0 = scratch; P.tmp1 = scratch + p.open_bytes;
            P.W = b.W; P.H = b.H; P.D = b.D; P.cap = cap; P.mark = 0;
            for (int a = 0; a < 3; a++) {
                const int si = (o >> a) & 1;
                const EditSpan q = edit_span_q(b.lo[a], b.hi[a], dim[a], si ? 1 : -1);
                P.q_lo[a] = q.lo; P.q_n[a] = q.hi - q.lo; P.r_lo[a] = p.r[a][si].lo; P.r_hi[a] = p.r[a][si].hi; P.sgn[a] = si ? 1 : -1;
            }
            const unsigned bx = (unsigned)((P.q_n[0] + 255) / 256);
            hipLaunchKernelGGL(k_edit_open_scan, dim3(bx, (unsigned)P.q_n[2]), dim3(256), 0, s, P, 1);
            hipLaunchKernelGGL(k_edit_open_scan, dim3(bx, (unsigned)P.q_n[1]), dim3(256), 0, s, P, 2);
            const size_t lines = (size_t)P.q_n[1] * (size_t)P.q_n[2];
            hipLaunchKernelGGL(k_edit_open_x, dim3((unsigned)((lines + 3) / 4)), dim3(256), 0, s, P);
        }
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// edits of brick scenes (vrt_scene_reserve_bricks, then vrt_scene_edit_box).  vrt_brick_edit.h has the regions (T, F, R_o, E, Q_o).
//   k_bedit_classify  per brick of T: is it occupied once the box's part is laid over its old content?  (the host assigns slots)
//   k_bedit_write     the box's ids into the pool bricks of T (a brick that appears starts from zeros), the padded grid and the
//                     occupancy bytes
//   k_brick_fine_list (vrt_scene_build.hip) the fine bytes of the occupied bricks of F
//   only when a brick's occupancy changed:
//   k_bedit_extract   the occupancy of E as a lattice of its own, through the build's own transform (launch_build_df, cap 16)
//   k_bedit_copy      R_o of each octant from there into the scene's coarse fields
//   k_edit_open_scan/_x   with mark = 0x80: the open bits of Q_o; then the entries are packed again (launch_brick_pack)
// ---------------------------------------------------------------------------------------------

static_assert(VRT_BRICK_EDIT_CAP == 16, "vrt_scene_from_bricks builds the coarse fields with cap 16");

// the voxel of the box at (x, y, z), which the caller knows to be inside it
__device__ __forceinline__ uint8_t bedit_box_id(const BrickEdit& P, int x, int y, int z)
{
    if (!P.ids) return (uint8_t)P.id;
    const size_t nx = (size_t)(P.hi[0] - P.lo[0]), ny = (size_t)(P.hi[1] - P.lo[1]);
    return P.ids[(size_t)(x - P.lo[0]) + ((size_t)(y - P.lo[1]) + (size_t)(z - P.lo[2]) * ny) * nx];
}

// one wave per brick of T; lane = (x, y) within the brick, z in a loop
__global__ __launch_bounds__(64) void k_bedit_classify(const BrickEdit P, const uint32_t* __restrict__ padded, const uint8_t* __restrict__ pool,
                                                       uint32_t* __restrict__ after)
{
    const uint32_t t = blockIdx.x;
    const int bx = P.t_lo[0] + (int)(t % (uint32_t)P.t_n[0]), by = P.t_lo[1] + (int)((t / (uint32_t)P.t_n[0]) % (uint32_t)P.t_n[1]);
    const int bz = P.t_lo[2] + (int)(t / ((uint32_t)P.t_n[0] * (uint32_t)P.t_n[1]));
    const uint32_t ptr = padded[(size_t)(bx + 1) + ((size_t)(by + 1) + (size_t)(bz + 1) * (size_t)P.pby) * (size_t)P.pbx];
    const int lx = (int)(threadIdx.x & 7u), ly = (int)(threadIdx.x >> 3);
    const int x = bx * 8 + lx, y = by * 8 + ly;
    const bool xy_in = x >= P.lo[0] && x < P.hi[0] && y >= P.lo[1] && y < P.hi[1];
    bool any = false;
    for (int lz = 0; lz < 8; lz++) {
        const int z = bz * 8 + lz;
        uint8_t v;
        if (xy_in && z >= P.lo[2] && z < P.hi[2]) v = bedit_box_id(P, x, y, z);     // a brick the box covers is decided by the ids alone
        else v = ptr ? pool[(size_t)(ptr - 1u) * 512u + (size_t)(lx + ly * 8 + lz * 64)] : (uint8_t)0;
        any = any || v != 0;
    }
    const uint64_t m = __ballot(any);
    if (threadIdx.x == 0) after[t] = m ? 1u : 0u;
}

// new_ptr[t]: the brick's grid entry after the edit (0: empty; the old entry where it stays occupied; a fresh slot + 1 where it appears)
__global__ __launch_bounds__(64) void k_bedit_write(const BrickEdit P, uint32_t* __restrict__ padded, uint8_t* __restrict__ occ,
                                                    uint8_t* __restrict__ pool, const uint32_t* __restrict__ new_ptr)
{
    const uint32_t t = blockIdx.x;
    const int bx = P.t_lo[0] + (int)(t % (uint32_t)P.t_n[0]), by = P.t_lo[1] + (int)((t / (uint32_t)P.t_n[0]) % (uint32_t)P.t_n[1]);
    const int bz = P.t_lo[2] + (int)(t / ((uint32_t)P.t_n[0] * (uint32_t)P.t_n[1]));
    const size_t pc = (size_t)(bx + 1) + ((size_t)(by + 1) + (size_t)(bz + 1) * (size_t)P.pby) * (size_t)P.pbx;
    const uint32_t old = padded[pc], np = new_ptr[t];
    __syncthreads();
    if (threadIdx.x == 0) {
        padded[pc] = np;
        occ[(size_t)bx + ((size_t)by + (size_t)bz * (size_t)P.nby) * (size_t)P.nbx] = np ? 1 : 0;
    }
    if (np == 0u) return;                                      // the slot of a brick that vanished keeps what it held: nothing points to it
    const int lx = (int)(threadIdx.x & 7u), ly = (int)(threadIdx.x >> 3);
    const int x = bx * 8 + lx, y = by * 8 + ly;
    const bool xy_in = x >= P.lo[0] && x < P.hi[0] && y >= P.lo[1] && y < P.hi[1];
    uint8_t* brick = pool + (size_t)(np - 1u) * 512u;
    for (int lz = 0; lz < 8; lz++) {
        const int z = bz * 8 + lz;
        if (xy_in && z >= P.lo[2] && z < P.hi[2]) brick[lx + ly * 8 + lz * 64] = bedit_box_id(P, x, y, z);
        else if (old == 0u) brick[lx + ly * 8 + lz * 64] = 0;
    }
}

hipError_t launch_bedit_classify(const BrickEdit& p, const uint32_t* padded, const uint8_t* pool, uint32_t* after, hipStream_t s)
{
    const unsigned n = (unsigned)p.t_n[0] * (unsigned)p.t_n[1] * (unsigned)p.t_n[2];
    hipLaunchKernelGGL(k_bedit_classify, dim3(n), dim3(64), 0, s, p, padded, pool, after);
    return hipGetLastError();
}

hipError_t launch_bedit_write(const BrickEdit& p, uint32_t* padded, uint8_t* occ, uint8_t* pool, const uint32_t* new_ptr, hipStream_t s)
{
    const unsigned n = (unsigned)p.t_n[0] * (unsigned)p.t_n[1] * (unsigned)p.t_n[2];
    hipLaunchKernelGGL(k_bedit_write, dim3(n), dim3(64), 0, s, p, padded, occ, pool, new_ptr);
    return hipGetLastError();
}

// the coarse fields after a change of occupancy
struct BrickCoarse {
    int nbx, nby;
    int e_lo[3], e_n[3];              // E
    int r_lo[8][3], r_n[8][3];        // R_o
    size_t cstride, sstride;          // bytes between the scene's fields / the sub-lattice's
};

__global__ __launch_bounds__(256) void k_bedit_extract(const BrickCoarse P, const uint8_t* __restrict__ occ, uint8_t* __restrict__ sub)
{
    const size_t n = (size_t)P.e_n[0] * P.e_n[1] * P.e_n[2], i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int x = P.e_lo[0] + (int)(i % (size_t)P.e_n[0]), y = P.e_lo[1] + (int)((i / (size_t)P.e_n[0]) % (size_t)P.e_n[1]);
    const int z = P.e_lo[2] + (int)(i / ((size_t)P.e_n[0] * P.e_n[1]));
    sub[i] = occ[(size_t)x + ((size_t)y + (size_t)z * (size_t)P.nby) * (size_t)P.nbx];
}

// blockIdx.y: the octant.  The open bit of the bricks written is cleared; the scans of Q_o (which holds R_o) set it again
__global__ __launch_bounds__(256) void k_bedit_copy(const BrickCoarse P, const uint8_t* __restrict__ subdf, uint8_t* __restrict__ coarse)
{
    const int o = (int)blockIdx.y;
    const size_t n = (size_t)P.r_n[o][0] * P.r_n[o][1] * P.r_n[o][2], i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int x = P.r_lo[o][0] + (int)(i % (size_t)P.r_n[o][0]), y = P.r_lo[o][1] + (int)((i / (size_t)P.r_n[o][0]) % (size_t)P.r_n[o][1]);
    const int z = P.r_lo[o][2] + (int)(i / ((size_t)P.r_n[o][0] * P.r_n[o][1]));
    coarse[(size_t)o * P.cstride + edit_pidx(x, y, z, P.nbx, P.nby)] =
        subdf[(size_t)o * P.sstride + edit_pidx(x - P.e_lo[0], y - P.e_lo[1], z - P.e_lo[2], P.e_n[0], P.e_n[1])];
}

namespace {
struct BrickCoarsePlan {
    BrickCoarse k;
    size_t sub_bytes, tmp_bytes;      // the sub-lattice; one of the two ping-pong buffers (the transform's, then the open scans')
    unsigned copy_blocks;
};
BrickCoarsePlan bedit_coarse_plan(const BrickEdit& b, size_t cstride, bool open)
{
    BrickCoarsePlan p;
    const int nb[3] = {b.nbx, b.nby, b.nbz};
    p.k.nbx = b.nbx; p.k.nby = b.nby; p.k.cstride = cstride;
    EditSpan t[3];
    for (int a = 0; a < 3; a++) {
        t[a].lo = b.t_lo[a]; t[a].hi = b.t_lo[a] + b.t_n[a];
        const EditSpan e = brick_span_e(t[a], nb[a]);
        p.k.e_lo[a] = e.lo; p.k.e_n[a] = e.hi - e.lo;
    }
    size_t rmax = 0, qmax = 0;
    for (int o = 0; o < 8; o++) {
        size_t rn = 1, qn = 1;
        for (int a = 0; a < 3; a++) {
            const int sign = ((o >> a) & 1) ? 1 : -1;
            const EditSpan r = brick_span_r(t[a], nb[a], sign), q = brick_span_q(t[a], nb[a], sign);
            p.k.r_lo[o][a] = r.lo; p.k.r_n[o][a] = r.hi - r.lo;
            rn *= (size_t)(r.hi - r.lo); qn *= (size_t)(q.hi - q.lo);
        }
        rmax = rn > rmax ? rn : rmax; qmax = qn > qmax ? qn : qmax;
    }
    const size_t ne = (size_t)p.k.e_n[0] * p.k.e_n[1] * p.k.e_n[2];
    p.k.sstride = df_field_bytes(p.k.e_n[0], p.k.e_n[1], p.k.e_n[2]);
    p.sub_bytes = (ne + 255u) & ~(size_t)255u;
    p.tmp_bytes = ((open && qmax > ne ? qmax : ne) + 255u) & ~(size_t)255u;
    p.copy_blocks = (unsigned)((rmax + 255) / 256);
    return p;
}
} // namespace

size_t bedit_coarse_scratch_bytes(const BrickEdit& b, size_t cstride, bool open)
{
    const BrickCoarsePlan p = bedit_coarse_plan(b, cstride, open);
    return p.sub_bytes + 8 * p.k.sstride + 2 * p.tmp_bytes;
}

// occ: the occupancy bytes AFTER the edit; coarse: the scene's eight unfolded fields as they were before it
hipError_t launch_bedit_coarse(const BrickEdit& b, const uint8_t* occ, uint8_t* coarse, size_t cstride, uint8_t* scratch, bool open, hipStream_t s)
{
    const BrickCoarsePlan p = bedit_coarse_plan(b, cstride, open);
    uint8_t *sub = scratch, *subdf = sub + p.sub_bytes, *tmp0 = subdf + 8 * p.k.sstride, *tmp1 = tmp0 + p.tmp_bytes;
    const size_t ne = (size_t)p.k.e_n[0] * p.k.e_n[1] * p.k.e_n[2];
    hipLaunchKernelGGL(k_bedit_extract, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, s, p.k, occ, sub);
    hipError_t e = launch_build_df(sub, p.k.e_n[0], p.k.e_n[1], p.k.e_n[2], subdf, p.k.sstride, tmp0, tmp1, s, VRT_BRICK_EDIT_CAP);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_bedit_copy, dim3(p.copy_blocks, 8), dim3(256), 0, s, p.k, (const uint8_t*)subdf, coarse);
    if (open) {
        const int nb[3] = {b.nbx, b.nby, b.nbz};
        for (int o = 0; o < 8; o++) {
            EditOpen P;
            P.vox = occ; P.field = coarse + (size_t)o * cstride; P.tmp0 = tmp0; P.tmp1 = tmp1;
            P.W = b.nbx; P.H = b.nby; P.D = b.nbz; P.cap = VRT_BRICK_EDIT_CAP; P.mark = 0x80;
            for (int a = 0; a < 3; a++) {
                const int si = (o >> a) & 1;
                EditSpan t; t.lo = b.t_lo[a]; t.hi = b.t_lo[a] + b.t_n[a];
                const EditSpan q = brick_span_q(t, nb[a], si ? 1 : -1);
                P.q_lo[a] = q.lo; P.q_n[a] = q.hi - q.lo; P.r_lo[a] = p.k.r_lo[o][a]; P.r_hi[a] = p.k.r_lo[o][a] + p.k.r_n[o][a]; P.sgn[a] = si ? 1 : -1;
            }
            const unsigned bx = (unsigned)((P.q_n[0] + 255) / 256);
            hipLaunchKernelGGL(k_edit_open_scan, dim3(bx, (unsigned)P.q_n[2]), dim3(256), 0, s, P, 1);
            hipLaunchKernelGGL(k_edit_open_scan, dim3(bx, (unsigned)P.q_n[1]), dim3(256), 0, s, P, 2);
            const size_t lines = (size_t)P.q_n[1] * (size_t)P.q_n[2];
            hipLaunchKernelGGL(k_edit_open_x, dim3((unsigned)((lines + 3) / 4)), dim3(256), 0, s, P);
        }
    }
    return hipGetLastError();
}

} // namespace vrt
