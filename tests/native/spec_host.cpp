// spec_host.cpp -- TEST HELPER: the product's numeric spec (csrc/vrt_spec.h) compiled for the host, one primitive per element over
// arrays of 32-bit patterns, with the fn numbers of vrt_debug_spec (include/vrt.h).  It calls the header's functions and restates
// nothing.  Built on demand by tests/test_spec_cpu.py with g++ -ffp-contract=off; never linked into libvrt_hip.so.
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../voxel-raytracing_amd/csrc/vrt_spec.h"

using namespace vrt;

static inline float f_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline uint32_t u_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static void spec_range(int fn, const uint32_t* a, const uint32_t* b, const uint32_t* c, size_t i0, size_t i1, uint32_t* out)
{
    for (size_t i = i0; i < i1; i++) {
        switch (fn) {
        case 0: out[i] = u_of(sqrt_spec(f_of(a[i]))); break;
        case 1: out[i] = u_of(div_spec(f_of(a[i]), f_of(b[i]))); break;
        case 2: out[i] = u_of(atan2_spec(f_of(a[i]), f_of(b[i]))); break;
        case 3: out[i] = u_of(asin_spec(f_of(a[i]))); break;
        case 4: out[i] = u_of(exp_spec(f_of(a[i]))); break;
        case 5: out[i] = (uint32_t)unorm8(f_of(a[i])); break;
        case 6: out[i] = (uint32_t)(int32_t)snorm8(f_of(a[i])); break;
        case 7: out[i] = wrap_texel(f_of(a[i]), b[i]); break;
        case 8: {
            const f3 d = normalize3(mk3(f_of(a[i]), f_of(b[i]), f_of(c[i])));
            out[3 * i] = u_of(d.x); out[3 * i + 1] = u_of(d.y); out[3 * i + 2] = u_of(d.z);
            break;
        }
        default: break;
        }
    }
}

extern "C" {

// returns 0, or -1 for an unknown fn or a NULL array that fn reads
int spec_host_batch(int fn, const uint32_t* a, const uint32_t* b, const uint32_t* c, size_t n, uint32_t* out, int nthreads)
{
    const bool two = fn == 1 || fn == 2 || fn == 7 || fn == 8;
    if (fn < 0 || fn > 8 || !a || !out || (two && !b) || (fn == 8 && !c)) return -1;
    if (nthreads < 1) nthreads = 1;
    const size_t per = (n + (size_t)nthreads - 1) / (size_t)nthreads;
    std::vector<std::thread> ts;
    for (int t = 0; t < nthreads; t++) {
        size_t i0 = per * (size_t)t, i1 = i0 + per;
        if (i0 > n) i0 = n;
        if (i1 > n) i1 = n;
        ts.emplace_back(spec_range, fn, a, b, c, i0, i1, out);
    }
    for (auto& t : ts) t.join();
    return 0;
}

} // extern "C"
