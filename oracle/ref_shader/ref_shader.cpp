// ref_shader.cpp -- ORACLE-side driver (test infrastructure, NOT product code).
//
// Runs the reference's own fragment shaders on the CPU: oracle/Makefile rewrites shader/voxel_volume.frag, denoiser.frag and
// blit.frag from where they lie in the reference tree (glsl2cpp.py, rules listed there) into oracle/_ref/*.inc, and this file
// includes those behind glsl_shim.h.  Neither the rewritten text nor the library is committed.  The driver only feeds uniforms,
// textures and the per-fragment inputs (vScreenPos = ((px+.5)/W, (py+.5)/H), gl_FragCoord = (px+.5, py+.5), as the full-screen
// triangle of screen_quad.vert interpolates them) and copies out what main() wrote, as raw floats: no quantisation here.
// Every output is reset to zero before each invocation (unwritten outColor.a etc. read 0).
// Not thread-safe: the shaders' uniforms are globals, as in GLSL.
//
// Output: oracle/_ref/libvrt_refshader.so, linked against oracle/libvrt_oracle.so (run path $ORIGIN/..) for vo_atan2f / vo_asinf /
// vo_expf, so that the elementary functions are the oracle's, bit for bit.
#include "glsl_shim.h"

namespace glsl {
namespace voxel_volume {
#include "voxel_volume.frag.inc"
}
namespace denoiser {
#include "denoiser.frag.inc"
}
namespace blit {
#include "blit.frag.inc"
}
}  // namespace glsl

using namespace glsl;
namespace vv = glsl::voxel_volume;
namespace dn = glsl::denoiser;
namespace bl = glsl::blit;

static_assert(sizeof(vv::pushConstants) == 96, "push block layout");
static_assert(sizeof(dn::pushConstants) == 96, "push block layout");
static_assert(sizeof(vv::Material) == 32, "palette entry layout");

extern "C" {

void rs_set_push(const void* push96) { std::memcpy((void*)&vv::pushConstants, push96, 96); }

// palette: `bytes` of Material entries 32 bytes apart (entries past the end read 0)
void rs_set_palette(const void* data, size_t bytes)
{
    vv::materials.data = (const unsigned char*)data; vv::materials.size = bytes; vv::materials.stride = 32;
}

void rs_set_params(uint32_t ao_samples, float ambient_intensity)
{
    vv::aoSamples = ao_samples; vv::ambientIntensity = ambient_intensity;
}

void rs_set_light(const float* dir3, float intensity, const float* color4)
{
    vv::lightDir = vec3(dir3[0], dir3[1], dir3[2]);
    vv::lightIntensity = intensity;
    vv::lightColor = vec4(color4[0], color4[1], color4[2], color4[3]);
}

void rs_set_volume(const uint8_t* voxels, uint32_t w, uint32_t h, uint32_t d)
{
    vv::scene.data = voxels; vv::scene.w = w; vv::scene.h = h; vv::scene.d = d;
}

void rs_set_sky(const float* rgba, int w, int h)
{
    vv::skybox.data = rgba; vv::skybox.w = w; vv::skybox.h = h; vv::skybox.format = FMT_F32; vv::skybox.filter = FILTER_NEAREST_REPEAT;
}

void rs_set_noise(const uint8_t* rgba, int w, int h)
{
    vv::blueNoise.data = rgba; vv::blueNoise.w = w; vv::blueNoise.h = h; vv::blueNoise.format = FMT_UNORM8;
    vv::blueNoise.filter = FILTER_NEAREST_REPEAT;
}

// main() of voxel_volume.frag for the pixels [x0, x1) x [y0, y1) of the push block's screen; planes are whole frames, row-major:
// color 4, depth 1, motion 2, mask 1, pos 3, normal 3 floats per pixel.
void rs_render(int x0, int y0, int x1, int y1, float* color, float* depth, float* motion, float* mask, float* pos, float* normal)
{
    int W = vv::pushConstants.screenSize.x, H = vv::pushConstants.screenSize.y;
    for (int py = y0; py < y1; py++)
        for (int px = x0; px < x1; px++) {
            vv::vScreenPos = vec2(((float)px + 0.5f) / (float)W, ((float)py + 0.5f) / (float)H);
            gl_FragCoord = vec4((float)px + 0.5f, (float)py + 0.5f, 0.0f, 1.0f);
            vv::outColor = vec4(); vv::outDepth = 0.0f; vv::outMotion = vec2(); vv::outMask = 0.0f;
            vv::outPos = vec3(); vv::outNormal = vec3();
            vv::main();
            size_t i = (size_t)py * (size_t)W + (size_t)px;
            color[i * 4 + 0] = vv::outColor.x; color[i * 4 + 1] = vv::outColor.y;
            color[i * 4 + 2] = vv::outColor.z; color[i * 4 + 3] = vv::outColor.w;
            depth[i] = vv::outDepth;
            motion[i * 2 + 0] = vv::outMotion.x; motion[i * 2 + 1] = vv::outMotion.y;
            mask[i] = vv::outMask;
            pos[i * 3 + 0] = vv::outPos.x; pos[i * 3 + 1] = vv::outPos.y; pos[i * 3 + 2] = vv::outPos.z;
            normal[i * 3 + 0] = vv::outNormal.x; normal[i * 3 + 1] = vv::outNormal.y; normal[i * 3 + 2] = vv::outNormal.z;
        }
}

// One pass of denoiser.frag over a W x H frame: colour RGBA8_UNORM, normal RGBA8_SNORM, position RGBA32F, all through a linear
// clamp-to-edge sampler whose coordinates within 1/512 texel of a texel centre point-sample (8 bits of sub-texel precision; the
// integral step widths of the default schedule land there, rule K).  params4 = phiColor, phiNormal, phiPos, stepWidth.  The kernel
// and offset uniform buffers are byte ranges read with the given strides: (4, 8) is the intended tight layout, (16, 16) is std140
// over the reference's tight upload (as shipped).
void rs_denoise_pass(const uint8_t* color, const int8_t* normal, const float* position, int W, int H, const float* params4,
                     const void* kernel, size_t kernel_bytes, size_t kernel_stride,
                     const void* offsets, size_t offset_bytes, size_t offset_stride, float* out)
{
    const float snap = 1.0f / 512.0f;
    dn::inputColor.data = color; dn::inputColor.w = W; dn::inputColor.h = H; dn::inputColor.format = FMT_UNORM8;
    dn::inputNormal.data = normal; dn::inputNormal.w = W; dn::inputNormal.h = H; dn::inputNormal.format = FMT_SNORM8;
    dn::inputPos.data = position; dn::inputPos.w = W; dn::inputPos.h = H; dn::inputPos.format = FMT_F32;
    dn::inputColor.filter = dn::inputNormal.filter = dn::inputPos.filter = FILTER_LINEAR_CLAMP;
    dn::inputColor.snap = dn::inputNormal.snap = dn::inputPos.snap = snap;
    dn::params.phiColor = params4[0]; dn::params.phiNormal = params4[1]; dn::params.phiPos = params4[2]; dn::params.stepWidth = params4[3];
    dn::kernel.data = (const unsigned char*)kernel; dn::kernel.size = kernel_bytes; dn::kernel.stride = kernel_stride;
    dn::offset.data = (const unsigned char*)offsets; dn::offset.size = offset_bytes; dn::offset.stride = offset_stride;
    dn::pushConstants.screenSize = ivec2(W, H);
    for (int py = 0; py < H; py++)
        for (int px = 0; px < W; px++) {
            dn::vScreenPos = vec2(((float)px + 0.5f) / (float)W, ((float)py + 0.5f) / (float)H);
            gl_FragCoord = vec4((float)px + 0.5f, (float)py + 0.5f, 0.0f, 1.0f);
            dn::outColor = vec4();
            dn::main();
            size_t i = ((size_t)py * (size_t)W + (size_t)px) * 4;
            out[i + 0] = dn::outColor.x; out[i + 1] = dn::outColor.y; out[i + 2] = dn::outColor.z; out[i + 3] = dn::outColor.w;
        }
}

// blit.frag: an RGBA8_UNORM source through a linear clamp-to-edge sampler (plain bilinear) into a tw x th target.
void rs_blit(const uint8_t* src, int sw, int sh, int tw, int th, float* out)
{
    bl::inputImage.data = src; bl::inputImage.w = sw; bl::inputImage.h = sh; bl::inputImage.format = FMT_UNORM8;
    bl::inputImage.filter = FILTER_LINEAR_CLAMP; bl::inputImage.snap = 0.0f;
    bl::offsets.sourceSize = uvec2((uint)sw, (uint)sh);
    bl::offsets.targetSize = uvec2((uint)tw, (uint)th);
    for (int py = 0; py < th; py++)
        for (int px = 0; px < tw; px++) {
            bl::vScreenPos = vec2(((float)px + 0.5f) / (float)tw, ((float)py + 0.5f) / (float)th);
            gl_FragCoord = vec4((float)px + 0.5f, (float)py + 0.5f, 0.0f, 1.0f);
            bl::outColor = vec4();
            bl::main();
            size_t i = ((size_t)py * (size_t)tw + (size_t)px) * 4;
            out[i + 0] = bl::outColor.x; out[i + 1] = bl::outColor.y; out[i + 2] = bl::outColor.z; out[i + 3] = bl::outColor.w;
        }
}

}  // extern "C"
