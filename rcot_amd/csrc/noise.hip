// Whole-image noise on the device (rcot_amd/chain.py: the noise_<model> stages of a degradation chain): one streaming pass over a
// uint8 HWC image that adds a counter-based normal deviate to every byte.  It sits between the other whole-image degradations
// (csrc/blur.hip, csrc/resize.hip, csrc/jpeg.hip), where the noise of rcot_patch_prep — made on the clean PATCH of a denoise_* sample
// (csrc/dataprep.hip) — cannot: a JPEG round trip after the noise has to see the whole noisy image.
//
// THE RULE (the only place it is defined).  For byte c of pixel (y, x), value v:
//     out = (uint8) clip(v + s z, 0, 255)          the product and the sum rounded separately in fp32 (no contraction), clip, then
//                                                  truncation: numpy's clip(...).astype(uint8), what dataprep.hip does per patch
//     z   = counter_randn(seed, idx)               common.h: splitmix64 finaliser, Box-Muller on two 24-bit uniforms
//   model 0  "g"     s = p0                         idx = (y W + x) 3 + c     white Gaussian noise, channels independent
//   model 1  "gray"  s = p0                         idx = y W + x             one deviate shared by R, G and B of a pixel
//   model 2  "pg"    s = sqrtf(p0 v + p1 p1)        idx = (y W + x) 3 + c     heteroscedastic Gaussian, the Poisson-Gaussian model:
//                                                                             variance p0 v + p1^2 in 8-bit units
//   s = 0 gives out = v: with p0 = 0 (and p1 = 0 for pg) the image is copied byte for byte, and no kernel runs.
//
// THE KERNEL.  The image is one array of n = 3 H W bytes.  A thread owns a RUN of 48 consecutive bytes — 16 whole pixels, three
// 16-byte words: it loads the three words, makes the 48 (gray: 16) deviates in registers and writes three 16-byte words, so dst == src
// is safe (a run is read whole before it is written, and runs are disjoint).  The n mod 48 bytes behind the last whole run, at most 15
// pixels, go pixel by pixel through the byte path; so does the whole image when src or dst is not 16-byte aligned.  Runs and the tail
// are walked grid-stride with 64-bit indices: an image of 2^31 bytes or more is legal.  No LDS, no atomics, no workspace.
// dst must be src itself or not overlap it.
#include "../../include/rcot_hip.h"
#include "common.h"

#include <cmath>

using namespace rcot;

namespace {

constexpr int RUN = 48;                                  // bytes of a thread's run: lcm(3 bytes of a pixel, 16 bytes of a store)
constexpr int RUN_PIXELS = RUN / 3;
constexpr int RUN_WORDS = RUN / 4;
constexpr int NT = 256;
constexpr int MAX_BLOCKS = 4096;                         // 16 workgroups per CU; larger images stride

template <int MODEL>
__device__ __forceinline__ uint32_t noised(uint32_t v, float p0, float p1, float z) {
    const float fv = (float)v;
    const float s = MODEL == 2 ? sqrtf(p0 * fv + p1 * p1) : p0;
    const float t = fv + s * z;
    return (uint32_t)fminf(fmaxf(t, 0.f), 255.f);        // clip, then the truncation of astype(uint8)
}

template <int MODEL>
__global__ __launch_bounds__(NT) void noise_kernel(const unsigned char* src, unsigned char* dst, uint64_t nruns, uint64_t npix,
                                                   float p0, float p1, uint64_t seed) {
    const uint64_t tid = (uint64_t)blockIdx.x * NT + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * NT;
    for (uint64_t r = tid; r < nruns; r += stride) {
        const uint4* s4 = reinterpret_cast<const uint4*>(src + r * RUN);
        const uint4 a = s4[0], b = s4[1], c = s4[2];
        const uint32_t in[RUN_WORDS] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
        uint32_t out[RUN_WORDS] = {};
#pragma unroll
        for (int p = 0; p < RUN_PIXELS; ++p) {
            float z = 0.f;
            if (MODEL == 1) z = counter_randn(seed, r * RUN_PIXELS + p);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int k = 3 * p + ch;                                            // byte of the run: word k / 4, byte k % 4
                if (MODEL != 1) z = counter_randn(seed, r * RUN + k);
                out[k >> 2] |= noised<MODEL>((in[k >> 2] >> (8 * (k & 3))) & 0xffu, p0, p1, z) << (8 * (k & 3));
            }
        }
        uint4* d4 = reinterpret_cast<uint4*>(dst + r * RUN);
        d4[0] = make_uint4(out[0], out[1], out[2], out[3]);
        d4[1] = make_uint4(out[4], out[5], out[6], out[7]);
        d4[2] = make_uint4(out[8], out[9], out[10], out[11]);
    }
    // the pixels behind the last whole run (all of them when nruns is 0), one per thread and step
    for (uint64_t px = nruns * RUN_PIXELS + tid; px < npix; px += stride) {
        float z = 0.f;
        if (MODEL == 1) z = counter_randn(seed, px);
        uint32_t o[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            if (MODEL != 1) z = counter_randn(seed, px * 3 + ch);
            o[ch] = noised<MODEL>(src[px * 3 + ch], p0, p1, z);
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) dst[px * 3 + ch] = (unsigned char)o[ch];
    }
}

}  // namespace

extern "C" int rcot_noise_u8(const unsigned char* src, unsigned char* dst, int h, int w, int model, float p0, float p1,
                             unsigned long long seed, void* stream) {
    if (!src || !dst || h < 1 || w < 1 || model < 0 || model > 2) return RCOT_EINVAL;
    if (!std::isfinite(p0) || !std::isfinite(p1) || p0 < 0.f || p1 < 0.f) return RCOT_EINVAL;
    if (model != 2 && p0 > 255.f) return RCOT_EINVAL;
    const uint64_t npix = (uint64_t)h * (uint64_t)w, n = 3 * npix;
    hipStream_t st = (hipStream_t)stream;
    if (p0 == 0.f && (model != 2 || p1 == 0.f)) {                                    // s = 0 everywhere: the copy
        if (dst != src) {
            hipError_t e = hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) return (int)e;
        }
        return RCOT_OK;
    }
    const uint64_t nruns = al16(src) && al16(dst) ? n / RUN : 0;
    const uint64_t tail = npix - nruns * RUN_PIXELS;
    const uint64_t items = nruns > tail ? nruns : tail;
    const dim3 grid((unsigned)((items + NT - 1) / NT < MAX_BLOCKS ? (items + NT - 1) / NT : MAX_BLOCKS)), block(NT);
    switch (model) {
        case 0: RCOT_LAUNCH(noise_kernel<0>, grid, block, 0, st, src, dst, nruns, npix, p0, p1, (uint64_t)seed); break;
        case 1: RCOT_LAUNCH(noise_kernel<1>, grid, block, 0, st, src, dst, nruns, npix, p0, p1, (uint64_t)seed); break;
        default: RCOT_LAUNCH(noise_kernel<2>, grid, block, 0, st, src, dst, nruns, npix, p0, p1, (uint64_t)seed); break;
    }
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}
