// A program of its own over csrc/vrt_brush.h, built by tests/test_brush_cpu.py with -fsanitize=address,undefined
// -fno-sanitize-recover=undefined and run as a child process: random and extreme shapes, the predicate at the corners, face
// centres and random voxels of the bounds (and well outside them), every mode, every orientation.  Signed overflow in the
// header's int64 arithmetic ends the program; so does a disagreement with the same predicate in 128-bit integers (host only).
//   brush_fuzz [seed] [rounds]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../voxel-raytracing_amd/csrc/vrt_brush.h"

using namespace vrt;
typedef __int128 wide;

static uint64_t g_state = 1;
static uint64_t rnd()
{
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return g_state;
}
static int32_t rnd_in(int32_t lo, int32_t hi) { return (int32_t)((int64_t)lo + (int64_t)(rnd() % (uint64_t)((int64_t)hi - lo + 1))); }
// mostly the ends of a range, sometimes anything in it
static int32_t pick(int32_t lo, int32_t hi)
{
    switch (rnd() % 6) {
    case 0: return lo;
    case 1: return hi;
    case 2: return lo + (hi > lo ? 1 : 0);
    case 3: return hi - (hi > lo ? 1 : 0);
    default: return rnd_in(lo, hi);
    }
}

static bool inside_wide(int32_t shape, const int32_t p[9], int32_t x, int32_t y, int32_t z)
{
    const wide v[3] = {x, y, z};
    if (shape == VRT_BRUSH_SHAPE_BOX) {
        for (int a = 0; a < 3; a++)
            if (v[a] < p[a] || v[a] >= (wide)p[a] + p[3 + a]) return false;
        return true;
    }
    const wide P[3] = {2 * v[0] + 1, 2 * v[1] + 1, 2 * v[2] + 1};
    if (shape == VRT_BRUSH_SHAPE_ELLIPSOID) {
        const wide dx = P[0] - p[0], dy = P[1] - p[1], dz = P[2] - p[2];
        const wide rx2 = (wide)p[3] * p[3], ry2 = (wide)p[4] * p[4], rz2 = (wide)p[5] * p[5];
        return dx * dx * ry2 * rz2 + dy * dy * rx2 * rz2 + dz * dz * rx2 * ry2 <= rx2 * ry2 * rz2;
    }
    wide L2 = 0, q = 0, da2 = 0, db2 = 0;
    for (int a = 0; a < 3; a++) {
        const wide e = (wide)p[3 + a] - p[a], da = P[a] - p[a], db = P[a] - p[3 + a];
        L2 += e * e; q += da * e; da2 += da * da; db2 += db * db;
    }
    const wide r2 = (wide)p[6] * p[6];
    if (q <= 0 || L2 == 0) return da2 <= r2;
    if (q >= L2) return db2 <= r2;
    return da2 * L2 - q * q <= r2 * L2;
}

static long g_checked = 0, g_inside = 0;

static int check(int32_t shape, const int32_t p[9], int64_t x, int64_t y, int64_t z)
{
    if (x < INT32_MIN || x > INT32_MAX || y < INT32_MIN || y > INT32_MAX || z < INT32_MIN || z > INT32_MAX) return 0;
    const bool got = brush_inside(shape, p, (int32_t)x, (int32_t)y, (int32_t)z), exp = inside_wide(shape, p, (int32_t)x, (int32_t)y, (int32_t)z);
    g_checked++; g_inside += got ? 1 : 0;
    if (got == exp) return 0;
    fprintf(stderr, "shape %d p %d %d %d %d %d %d %d voxel %lld %lld %lld: header %d, 128-bit %d\n", shape, p[0], p[1], p[2], p[3], p[4], p[5], p[6],
            (long long)x, (long long)y, (long long)z, (int)got, (int)exp);
    return 1;
}

static int one_shape(int32_t shape, const int32_t p[9])
{
    if (!brush_shape_ok(shape, p)) { fprintf(stderr, "a shape inside its ranges was refused\n"); return 1; }
    int64_t lo[3], hi[3];
    brush_bounds(shape, p, lo, hi);
    int bad = 0;
    // corners, edge and face centres of the bounds and of the bounds grown by one; the middle
    for (int g = 0; g < 2; g++)
        for (int k = 0; k < 27; k++) {
            int64_t v[3];
            for (int a = 0; a < 3; a++) {
                const int s = (k / (a == 0 ? 1 : a == 1 ? 3 : 9)) % 3;
                v[a] = s == 0 ? lo[a] - g : s == 1 ? lo[a] + (hi[a] - lo[a]) / 2 : hi[a] - 1 + g;
            }
            bad += check(shape, p, v[0], v[1], v[2]);
        }
    for (int i = 0; i < 48; i++) {                 // random voxels of the bounds
        int64_t v[3];
        for (int a = 0; a < 3; a++) v[a] = lo[a] + (int64_t)(rnd() % (uint64_t)(hi[a] - lo[a]));
        bad += check(shape, p, v[0], v[1], v[2]);
    }
    if (shape == VRT_BRUSH_SHAPE_CAPSULE)
        for (int i = 0; i < 48; i++) {             // voxels within about r of a point of the segment
            const int64_t t = (int64_t)(rnd() % 1025);
            int64_t v[3];
            for (int a = 0; a < 3; a++) {
                const int64_t at = p[a] + ((int64_t)p[3 + a] - p[a]) * t / 1024 + rnd_in(-p[6] - 2, p[6] + 2);
                v[a] = brush_floor_half(at);
            }
            bad += check(shape, p, v[0], v[1], v[2]);
        }
    for (int i = 0; i < 8; i++)                    // anywhere at all: the predicate answers without evaluating a product
        bad += check(shape, p, (int32_t)rnd(), (int32_t)rnd(), (int32_t)rnd());
    bad += check(shape, p, INT32_MIN, INT32_MAX, 0) + check(shape, p, INT32_MAX, INT32_MAX, INT32_MAX) + check(shape, p, INT32_MIN, INT32_MIN, INT32_MIN);
    // the clip never reports a box outside the volume
    const int32_t dim[3] = {pick(1, 4096), pick(1, 4096), pick(1, 4096)};
    int32_t clo[3];
    uint32_t cs[3];
    if (brush_clip(lo, hi, dim, clo, cs))
        for (int a = 0; a < 3; a++)
            if (clo[a] < 0 || cs[a] == 0u || (int64_t)clo[a] + cs[a] > dim[a] || clo[a] < lo[a] || (int64_t)clo[a] + cs[a] > hi[a]) { fprintf(stderr, "clip leaves the volume or the bounds\n"); bad++; }
    // the extent check: any int32 bounds against any clipped bounds up to the largest size, without overflow; the extremes both ways
    const int32_t mn[3] = {(int32_t)rnd(), (int32_t)rnd(), (int32_t)rnd()}, mx[3] = {(int32_t)rnd(), (int32_t)rnd(), (int32_t)rnd()};
    const int32_t top[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, bot[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    const uint32_t one[3] = {1u, 1u, 1u}, big[3] = {1u << 30, 1u << 30, 1u << 30};
    (void)brush_extent_ok(mn, mx, mn, big);
    (void)brush_extent_ok(mn, mx, top, big);
    if (!brush_extent_ok(top, top, top, one) || !brush_extent_ok(bot, bot, bot, big) || brush_extent_ok(top, bot, bot, big)) { fprintf(stderr, "extent check at the extremes\n"); bad++; }
    return bad;
}

int main(int argc, char** argv)
{
    g_state = argc > 1 ? strtoull(argv[1], nullptr, 10) * 2654435761u + 88172645463325252ull : 88172645463325252ull;
    const long rounds = argc > 2 ? atol(argv[2]) : 20000;
    int bad = 0;
    for (long r = 0; r < rounds && !bad; r++) {
        int32_t p[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        // ellipsoids: the semi-axes at their ends (1024, 1023 / 1024 / 1 mixes), the centre anywhere an int32 can be
        for (int a = 0; a < 3; a++) { p[a] = (r % 4 == 0) ? pick(INT32_MIN, INT32_MAX) : pick(-4096, 12288); p[3 + a] = pick(1, VRT_BRUSH_MAX_RADIUS); }
        bad += one_shape(VRT_BRUSH_SHAPE_ELLIPSOID, p);
        // capsules: the end points at -4096 and 12288, the radius at 1024
        for (int a = 0; a < 6; a++) p[a] = pick(VRT_BRUSH_CAPSULE_MIN, VRT_BRUSH_CAPSULE_MAX);
        if (r % 5 == 0) for (int a = 0; a < 3; a++) p[3 + a] = p[a];                               // a == b
        p[6] = pick(1, VRT_BRUSH_MAX_RADIUS);
        bad += one_shape(VRT_BRUSH_SHAPE_CAPSULE, p);
        // boxes: lo anywhere, the size at its ends
        for (int a = 0; a < 3; a++) { p[a] = pick(INT32_MIN, INT32_MAX); p[3 + a] = pick(1, VRT_BRUSH_BOX_MAX_SIZE); }
        bad += one_shape(VRT_BRUSH_SHAPE_BOX, p);
        // modes and stamps
        const uint32_t old = (uint32_t)(rnd() & 255u), id = (uint32_t)(rnd() & 255u), match = (uint32_t)(rnd() & 255u);
        for (int32_t mode = 0; mode < 4; mode++) {
            const uint32_t v = brush_value(mode, old, id, match);
            if (v != old && v != id) { fprintf(stderr, "mode %d made %u of %u with id %u\n", mode, v, old, id); bad++; }
        }
        const uint32_t size[3] = {(uint32_t)pick(1, (int32_t)VRT_STAMP_MAX_SIDE), (uint32_t)pick(1, (int32_t)VRT_STAMP_MAX_SIDE), (uint32_t)pick(1, (int32_t)VRT_STAMP_MAX_SIDE)};
        for (uint32_t orient = 0; orient < 64u; orient++) {
            if (!stamp_orient_ok(orient)) continue;
            uint32_t ds[3], s[3];
            stamp_dst_size(orient, size, ds);
            const uint32_t d[3] = {(uint32_t)pick(0, (int32_t)ds[0] - 1), (uint32_t)pick(0, (int32_t)ds[1] - 1), (uint32_t)pick(0, (int32_t)ds[2] - 1)};
            stamp_source(orient, size, d[0], d[1], d[2], s);
            if (s[0] >= size[0] || s[1] >= size[1] || s[2] >= size[2]) { fprintf(stderr, "orientation %u leaves the source box\n", orient); bad++; }
        }
    }
    // refused: every parameter one step outside its range
    {
        int32_t p[9] = {0, 0, 0, 1, 1, 1, 1, 0, 0};
        int32_t q[9];
        for (int a = 3; a < 6; a++) for (int32_t v : {0, -1, VRT_BRUSH_MAX_RADIUS + 1, INT32_MIN, INT32_MAX}) { for (int i = 0; i < 9; i++) q[i] = p[i]; q[a] = v; if (brush_shape_ok(VRT_BRUSH_SHAPE_ELLIPSOID, q)) bad++; }
        for (int a = 0; a < 6; a++) for (int32_t v : {VRT_BRUSH_CAPSULE_MIN - 1, VRT_BRUSH_CAPSULE_MAX + 1, INT32_MIN, INT32_MAX}) { for (int i = 0; i < 9; i++) q[i] = p[i]; q[a] = v; if (brush_shape_ok(VRT_BRUSH_SHAPE_CAPSULE, q)) bad++; }
        for (int32_t v : {0, -1, VRT_BRUSH_MAX_RADIUS + 1, INT32_MIN}) { for (int i = 0; i < 9; i++) q[i] = p[i]; q[6] = v; if (brush_shape_ok(VRT_BRUSH_SHAPE_CAPSULE, q)) bad++; }
        for (int a = 3; a < 6; a++) for (int32_t v : {0, -1, VRT_BRUSH_BOX_MAX_SIZE + 1, INT32_MIN}) { for (int i = 0; i < 9; i++) q[i] = p[i]; q[a] = v; if (brush_shape_ok(VRT_BRUSH_SHAPE_BOX, q)) bad++; }
        if (brush_shape_ok(3, p) || brush_shape_ok(-1, p) || brush_mode_ok(4, 1, 0) || brush_mode_ok(-1, 1, 0)) bad++;
        if (bad) fprintf(stderr, "a parameter outside its range was accepted\n");
    }
    printf("%ld predicates, %ld inside\n", g_checked, g_inside);
    return bad ? 1 : 0;
}
