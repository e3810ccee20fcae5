// Shared helpers for the rcot_hip kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#define RCOT_OK 0
#define RCOT_EINVAL (-1)      // bad shape / alignment / null pointer
#define RCOT_EWORKSPACE (-2)  // caller-provided workspace too small
#define RCOT_EUNSUPPORTED (-3) // no kernel of this entry point takes the shape

#define RCOT_LAUNCH_CHECK()                          \
    do {                                             \
        hipError_t e__ = hipGetLastError();          \
        if (e__ != hipSuccess) return (int)e__;      \
    } while (0)

namespace rcot {
// Per-launch device time stamps (rcot_profile_begin / rcot_profile_end, api.hip): while the calling thread collects, every launch of the
// library goes through hipExtLaunchKernelGGL with a start and a stop event of its own — the dispatch packet's own begin / end times,
// what rocprofv3 --kernel-trace lists, with nothing added between the kernels.
bool prof_on();
void prof_slot(const void* fn, hipEvent_t* e0, hipEvent_t* e1);
template <typename F> inline const void* prof_fn(F f) { return reinterpret_cast<const void*>(f); }
}  // namespace rcot

#define RCOT_LAUNCH(kernel, grid, block, smem, stream, ...)                                              \
    do {                                                                                                  \
        if (rcot::prof_on()) {                                                                            \
            hipEvent_t e0__, e1__;                                                                        \
            rcot::prof_slot(rcot::prof_fn(kernel), &e0__, &e1__);                                         \
            hipExtLaunchKernelGGL(kernel, grid, block, smem, stream, e0__, e1__, 0, __VA_ARGS__);         \
        } else {                                                                                          \
            hipLaunchKernelGGL(kernel, grid, block, smem, stream, __VA_ARGS__);                           \
        }                                                                                                 \
    } while (0)

namespace rcot {

// Launch of a kernel whose dynamic LDS may pass the 64 KiB a kernel gets by default: the limit is raised to the CU's 160 KiB once per
// kernel (one instantiation of this template, and so one `once`, per kernel), then RCOT_LAUNCH.  The caller checks with
// RCOT_LAUNCH_CHECK() as after any launch.
template <auto Kernel, class... A>
inline void launch_lds(dim3 grid, dim3 block, size_t smem, hipStream_t st, const A&... a) {
    static bool once = (hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess);
    (void)once;
    RCOT_LAUNCH(Kernel, grid, block, smem, st, a...);
}

constexpr int WAVE = 64;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// Block-wide sum for blockDim.x == NT (multiple of 64). `red` must hold NT/64 floats.
template <int NT>
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __syncthreads();
    if (l == 0) red[w] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) t += red[i];
    return t;
}

// F.normalize (MDTA's q and k rows): |x| from the row's sum of squares, clamped as torch does.
__device__ __forceinline__ float clamp_norm(float sumsq) { return fmaxf(sqrtf(sumsq), 1e-12f); }

// Its backward's diagonal term, dx += D x with D = -tau s / |x|^2 (s: the row's sum of dS.Gn); zero where the forward clamped.
__device__ __forceinline__ float norm_bwd_scale(float tau, float s, float sumsq) { return sumsq >= 1e-24f ? -tau * s / sumsq : 0.f; }

// Fixed-order totals of per-workgroup partials, for ONE workgroup of 256 threads: ND streams of nb fp64 values (stream d at
// part_d[d * nb ..)) and one stream of nb int64 values.  Strided per-thread sums (the loads of eight steps in flight, the sums in
// order), then a tree over the 256 threads; every thread returns with the totals.
template <int ND>
__device__ __forceinline__ void final_sums(const double* __restrict__ part_d, const long long* __restrict__ part_i, long nb,
                                           double (&tot_d)[ND], long long& tot_i) {
    __shared__ double sd[ND][256];
    __shared__ long long si[256];
    const int t = threadIdx.x;
    double s[ND] = {};
    long long n = 0;
#pragma unroll 8
    for (long b = t; b < nb; b += 256) {
#pragma unroll
        for (int d = 0; d < ND; ++d) s[d] += part_d[d * nb + b];
        n += part_i[b];
    }
#pragma unroll
    for (int d = 0; d < ND; ++d) sd[d][t] = s[d];
    si[t] = n;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int d = 0; d < ND; ++d) sd[d][t] += sd[d][t + o];
            si[t] += si[t + o];
        }
        __syncthreads();
    }
#pragma unroll
    for (int d = 0; d < ND; ++d) tot_d[d] = sd[d][0];
    tot_i = si[0];
}

// Unsigned division by a runtime-invariant divisor (host precomputes magic/shift).
struct FastDiv {
    uint32_t d, magic, shift;
    __host__ void init(uint32_t div) {
        d = div ? div : 1;
        shift = 0;
        while ((1ull << shift) < d) ++shift;
        magic = (uint32_t)(((1ull << 32) * ((1ull << shift) - d)) / d + 1);
    }
    __device__ __forceinline__ uint32_t div(uint32_t n) const {
        return (uint32_t)(((uint64_t)__umulhi(n, magic) + n) >> shift);
    }
    __device__ __forceinline__ void divmod(uint32_t n, uint32_t& q, uint32_t& r) const {
        q = div(n);
        r = n - q * d;
    }
};

__device__ __forceinline__ float gelu_erf(float a) {
    return 0.5f * a * (1.0f + erff(a * 0.70710678118654752440f));
}
// d/da [a * Phi(a)] = Phi(a) + a * phi(a)
__device__ __forceinline__ float gelu_erf_grad(float a) {
    const float cdf = 0.5f * (1.0f + erff(a * 0.70710678118654752440f));
    const float pdf = 0.39894228040143267794f * __expf(-0.5f * a * a);
    return cdf + a * pdf;
}

// gelu(a) and gelu'(a) from ONE exponential: Phi via erf(x) = 1 - (a1 t + ... + a5 t^5) exp(-x^2), t = 1/(1 + p x)
// (Abramowitz & Stegun 7.1.26, |error| <= 1.5e-7, i.e. ~2 ulp of Phi), and phi(a) = exp(-a^2/2)/sqrt(2 pi) is the same
// exponential.  Used by the backward gate, which is VALU-bound with erff + expf per pixel.
__device__ __forceinline__ void gelu_and_grad(float a, float& g, float& dg) {
    const float e = __expf(-0.5f * a * a);
    const float x = fabsf(a) * 0.70710678118654752440f;
    const float t = __frcp_rn(fmaf(0.3275911f, x, 1.0f));
    float q = fmaf(1.061405429f, t, -1.453152027f);
    q = fmaf(q, t, 1.421413741f);
    q = fmaf(q, t, -0.284496736f);
    q = fmaf(q, t, 0.254829592f);
    const float erfv = copysignf(fmaf(-q * t, e, 1.0f), a);
    const float cdf = fmaf(0.5f, erfv, 0.5f);
    g = a * cdf;
    dg = fmaf(a * 0.39894228040143267794f, e, cdf);
}

__device__ __forceinline__ uint64_t mix64(uint64_t z) {          // splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// standard normal from a counter (Box-Muller on two 24-bit uniforms): the one noise source of the library — the patch noise of the
// denoise_* tasks (dataprep.hip) and the whole-image noise of a degradation chain (noise.hip)
__device__ __forceinline__ float counter_randn(uint64_t seed, uint64_t idx) {
    const uint64_t h = mix64(seed + 0x9e3779b97f4a7c15ull * (idx + 1));
    const float u1 = ((float)((h >> 40) & 0xffffff) + 1.0f) * (1.0f / 16777217.0f);     // (0, 1)
    const float u2 = (float)((h >> 8) & 0xffffff) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * __logf(u1)) * __cosf(6.283185307179586f * u2);
}

// The 8 dihedral maps of numpy's rot90 / flipud composition (the reference's data_augmentation, util/image_utils.py:133-163) on a
// Th x Tw rectangle: source pixel (sy, sx) of the rectangle for pixel (i, j) of the mapped one.  Modes 0, 1, 4, 5 keep the shape
// (i < Th, j < Tw); modes 2, 3, 6, 7 give Tw x Th (i < Tw, j < Th).
__host__ __device__ __forceinline__ void dihedral(int mode, int Th, int Tw, int i, int j, int& sy, int& sx) {
    switch (mode) {
        case 1: sy = Th - 1 - i; sx = j; break;              // flipud
        case 2: sy = j; sx = Tw - 1 - i; break;              // rot90 (counter-clockwise)
        case 3: sy = j; sx = i; break;                       // rot90 + flipud
        case 4: sy = Th - 1 - i; sx = Tw - 1 - j; break;     // rot180
        case 5: sy = i; sx = Tw - 1 - j; break;              // rot180 + flipud
        case 6: sy = Th - 1 - j; sx = i; break;              // rot270
        case 7: sy = Th - 1 - j; sx = Tw - 1 - i; break;     // rot270 + flipud
        default: sy = i; sx = j; break;                      // 0: identity
    }
}
// the mode that undoes `mode` (rot90 and rot270 undo each other; the flips, rot180 and the two transposes undo themselves)
__host__ __device__ __forceinline__ int dihedral_inverse(int mode) { return mode == 2 ? 6 : mode == 6 ? 2 : mode; }

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// "not one of my shapes": what a dispatcher inside the library (dispatch.h) answers so that its caller tries the next kernel
// family.  Never returned by an entry point.
constexpr int NOT_ELIGIBLE = -100;

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// workgroups of bs threads that cover n elements, between 1 and cap (grid-stride kernels)
inline int grid_for(long n, int bs = 256, int cap = 8192) {
    long g = (n + bs - 1) / bs;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

// Name of the kernel symbol the calling thread's last dispatcher chose (printf-style; api.hip).  bench.py reads it back through
// rcot_last_kernel() to attribute the time of an entry point to the kernel family that ran (several families serve one entry point).
void note_kernel(const char* fmt, ...);
inline const char* tf(bool b) { return b ? "true" : "false"; }

}  // namespace rcot
