// Implicit-GEMM dense convolutions on the MFMA fp32 engine: forward (bias + LeakyReLU, residual,
// PixelShuffle/PixelUnshuffle folded into the store), data gradient, weight gradient.
// Serves the critic's k5s1 / k4s2 / k3s1 stack and the transport map's patch-embed / Downsample /
// Upsample / output 3x3 convolutions.
//
// GEMM view: M = output channels, N = (image, output pixel) — the batch is FOLDED into N so that the deep
// critic layers (4x4 .. 16x16 pixels per image) still fill 64/128-wide tiles — and K = (ci, ky, kx); when
// M*N gives too few workgroups the K loop is split into slabs (deterministic reduce).  The stride-2 data
// gradient is decomposed by OUTPUT PARITY: each of the 4 parity classes of dX only ever sees 2x2 of the
// 4x4 taps, so it is run as 4 dense sub-problems with K = Co*4 instead of one with K = Co*16 of which 3/4
// would multiply zeros.
#include <cstdlib>
#include "gemm_core.h"
#include "dispatch.h"
#include "../../include/rcot_hip.h"

using namespace rcot;

namespace {

using CfgL = TileCfg<128, 128>;
using CfgS = TileCfg<64, 64>;

struct ConvGeom {
    const float* src;      // tensor the gather reads
    int B, Ci, Co, H, W, OH, OW, KH, KW, stride, pad;
    FastDiv dKHW, dKW, dOW, dW, dP, dHW, dW2, dHW2;
};

// Every functor splits its gather into px() (x index: once per thread), pk() (k index: once per slab or element)
// and idx() (element offset + inside-the-tensor flag; the loader loads UNCONDITIONALLY — from offset 0 when outside — and zeroes
// the value on its way to LDS: a load under a branch makes the compiler drain every outstanding load before the next use) — see FunctorLoader.  Offsets are ints: every tensor has < 2^31 elements (checked).
struct TapK { int off, ky, kx; };        // channel offset + filter tap
struct PixX { int off, y, x; };          // image offset + (pre-shifted) pixel coordinates
struct OffS { int off; };

// forward: B(k=(ci,ky,kx), n=(b,oy,ox)) = X[b][ci][oy*s+ky-p][ox*s+kx-p]
struct FwdB {
    typedef ConvGeom P;
    [[maybe_unused]] static constexpr bool TABLE = true;     // KS = TapK: eligible for the per-slab LDS table
    typedef TapK KS;
    typedef PixX XS;
    __device__ static __forceinline__ int extent(const P& g) { return g.B * (int)g.dP.d; }
    __device__ static __forceinline__ KS pk(const P& g, int, int k) {
        uint32_t ci, r, ky, kx;
        g.dKHW.divmod(k, ci, r);
        g.dKW.divmod(r, ky, kx);
        return KS{(int)ci * g.H * g.W, (int)ky, (int)kx};
    }
    __device__ static __forceinline__ XS px(const P& g, int, int n) {
        uint32_t b, pix, oy, ox;
        g.dP.divmod(n, b, pix);
        g.dOW.divmod(pix, oy, ox);
        return XS{(int)b * g.Ci * g.H * g.W, (int)(oy * g.stride) - g.pad, (int)(ox * g.stride) - g.pad};
    }
    __device__ static __forceinline__ int idx(const P& g, const KS& k, const XS& x, bool& ok) {
        const int iy = x.y + k.ky, ix = x.x + k.kx;
        ok = (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
        return x.off + k.off + iy * g.W + ix;
    }
};

// stride-1 data gradient: A(m=ci, k=(co,ky,kx)) = Wt[co][ci][ky][kx]
struct DgradA {
    typedef ConvGeom P;
    [[maybe_unused]] static constexpr bool TABLE = false;
    typedef OffS KS;
    typedef OffS XS;
    __device__ static __forceinline__ int extent(const P& g) { return g.Ci; }
    __device__ static __forceinline__ KS pk(const P& g, int, int k) {
        uint32_t co, r;
        g.dKHW.divmod(k, co, r);
        return KS{(int)co * g.Ci * (int)g.dKHW.d + (int)r};
    }
    __device__ static __forceinline__ XS px(const P& g, int, int m) { return XS{m * (int)g.dKHW.d}; }
    __device__ static __forceinline__ int idx(const P&, const KS& k, const XS& x, bool& ok) { ok = true; return k.off + x.off; }
};
// stride-1 data gradient: B(k=(co,ky,kx), n=(b,y,x)) = dY[b][co][y+p-ky][x+p-kx]
struct DgradB {
    typedef ConvGeom P;
    [[maybe_unused]] static constexpr bool TABLE = true;     // KS = TapK: eligible for the per-slab LDS table
    typedef TapK KS;
    typedef PixX XS;
    __device__ static __forceinline__ int extent(const P& g) { return g.B * (int)g.dHW.d; }
    __device__ static __forceinline__ KS pk(const P& g, int, int k) {
        uint32_t co, r, ky, kx;
        g.dKHW.divmod(k, co, r);
        g.dKW.divmod(r, ky, kx);
        return KS{(int)co * g.OH * g.OW, (int)ky, (int)kx};
    }
    __device__ static __forceinline__ XS px(const P& g, int, int n) {
        uint32_t b, pix, y, x;
        g.dHW.divmod(n, b, pix);
        g.dW.divmod(pix, y, x);
        return XS{(int)b * g.Co * g.OH * g.OW, (int)y + g.pad, (int)x + g.pad};
    }
    __device__ static __forceinline__ int idx(const P& g, const KS& k, const XS& x, bool& ok) {
        const int oy = x.y - k.ky, ox = x.x - k.kx;
        ok = (unsigned)oy < (unsigned)g.OH && (unsigned)ox < (unsigned)g.OW;
        return x.off + k.off + oy * g.OW + ox;
    }
};

// stride-2 (k4) data gradient, parity class cls = 2*py + px:  taps ky = ky0 + 2*jy, ky0 = (py + pad) & 1
// A(m=ci, k=(co,jy,jx)) = Wt[co][ci][ky][kx]
struct Dgrad2A {
    typedef ConvGeom P;
    [[maybe_unused]] static constexpr bool TABLE = false;
    typedef OffS KS;
    typedef OffS XS;
    __device__ static __forceinline__ int extent(const P& g) { return g.Ci; }
    __device__ static __forceinline__ KS pk(const P& g, int cls, int k) {
        const int co = k >> 2, jy = (k >> 1) & 1, jx = k & 1;
        const int ky = (((cls >> 1) + g.pad) & 1) + 2 * jy, kx = (((cls & 1) + g.pad) & 1) + 2 * jx;
        return KS{co * g.Ci * 16 + ky * 4 + kx};
    }
    __device__ static __forceinline__ XS px(const P&, int, int m) { return XS{m * 16}; }
    __device__ static __forceinline__ int idx(const P&, const KS& k, const XS& x, bool& ok) { ok = true; return k.off + x.off; }
};
// B(k=(co,jy,jx), n=(b,y',x')) = dY[b][co][(2y'+py+p-ky)/2][(2x'+px+p-kx)/2]
struct Dgrad2B {
    typedef ConvGeom P;
    [[maybe_unused]] static constexpr bool TABLE = true;     // KS = TapK: eligible for the per-slab LDS table
    typedef TapK KS;
    typedef PixX XS;
    __device__ static __forceinline__ int extent(const P& g) { return g.B * (int)g.dHW2.d; }
    __device__ static __forceinline__ KS pk(const P& g, int cls, int k) {
        const int co = k >> 2, jy = (k >> 1) & 1, jx = k & 1;
        const int ky = (((cls >> 1) + g.pad) & 1) + 2 * jy, kx = (((cls & 1) + g.pad) & 1) + 2 * jx;
        return KS{co * g.OH * g.OW, ky, kx};
    }
    __device__ static __forceinline__ XS px(const P& g, int cls, int n) {
        uint32_t b, pix, y2, x2;
        g.dHW2.divmod(n, b, pix);
        g.dW2.divmod(pix, y2, x2);
        return XS{(int)b * g.Co * g.OH * g.OW, 2 * (int)y2 + (cls >> 1) + g.pad, 2 * (int)x2 + (cls & 1) + g.pad};
    }
    __device__ static __forceinline__ int idx(const P& g, const KS& k, const XS& x, bool& ok) {
        const int ty = x.y - k.ky, tx = x.x - k.kx;                 // even by construction
        const int oy = ty >> 1, ox = tx >> 1;
        ok = ty >= 0 && tx >= 0 && oy < g.OH && ox < g.OW;
        return x.off + k.off + oy * g.OW + ox;
    }
};

// weight gradient: A(m=co, k=(b,pix)) = dY[b][co][pix]
struct WgradA {
    typedef ConvGeom P;
    [[maybe_unused]] static constexpr bool TABLE = false;
    typedef OffS KS;
    typedef OffS XS;
    __device__ static __forceinline__ int extent(const P& g) { return g.Co; }
    __device__ static __forceinline__ KS pk(const P& g, int, int k) {
        uint32_t b, pix;
        g.dP.divmod(k, b, pix);
        return KS{(int)b * g.Co * (int)g.dP.d + (int)pix};
    }
    __device__ static __forceinline__ XS px(const P& g, int, int m) { return XS{m * (int)g.dP.d}; }
    __device__ static __forceinline__ int idx(const P&, const KS& k, const XS& x, bool& ok) { ok = true; return k.off + x.off; }
};
// weight gradient: B(k=(b,oy,ox), n=(ci,ky,kx)) = X[b][ci][oy*s+ky-p][ox*s+kx-p]
struct WgradB {
    typedef ConvGeom P;
    [[maybe_unused]] static constexpr bool TABLE = false;
    typedef PixX KS;
    typedef TapK XS;
    __device__ static __forceinline__ int extent(const P& g) { return g.Ci * (int)g.dKHW.d; }
    __device__ static __forceinline__ KS pk(const P& g, int, int k) {
        uint32_t b, pix, oy, ox;
        g.dP.divmod(k, b, pix);
        g.dOW.divmod(pix, oy, ox);
        return KS{(int)b * g.Ci * g.H * g.W, (int)(oy * g.stride) - g.pad, (int)(ox * g.stride) - g.pad};
    }
    __device__ static __forceinline__ XS px(const P& g, int, int n) {
        uint32_t ci, r, ky, kx;
        g.dKHW.divmod(n, ci, r);
        g.dKW.divmod(r, ky, kx);
        return XS{(int)ci * g.H * g.W, (int)ky, (int)kx};
    }
    __device__ static __forceinline__ int idx(const P& g, const KS& k, const XS& x, bool& ok) {
        const int iy = k.y + x.ky, ix = k.x + x.kx;
        ok = (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
        return k.off + x.off + iy * g.W + ix;
    }
};

ConvGeom make_geom(const float* src, int B, int Ci, int Co, int H, int W, int KH, int KW, int stride, int pad) {
    ConvGeom g{};
    g.src = src;
    g.B = B; g.Ci = Ci; g.Co = Co; g.H = H; g.W = W; g.KH = KH; g.KW = KW; g.stride = stride; g.pad = pad;
    g.OH = (H + 2 * pad - KH) / stride + 1;
    g.OW = (W + 2 * pad - KW) / stride + 1;
    g.dKHW.init(KH * KW); g.dKW.init(KW); g.dOW.init(g.OW); g.dW.init(W);
    g.dP.init(g.OH * g.OW); g.dHW.init(H * W);
    g.dW2.init(W >> 1 ? W >> 1 : 1); g.dHW2.init((H >> 1) * (W >> 1) ? (H >> 1) * (W >> 1) : 1);
    return g;
}

template <class Cfg> using AStrK = StridedLoader<Cfg::BM, Cfg::SA, true>;
template <class Cfg> using BFwd = FunctorLoader<Cfg::BN, Cfg::SB, FwdB, false>;
template <class Cfg> using ADg = FunctorLoader<Cfg::BM, Cfg::SA, DgradA, true>;
template <class Cfg> using BDg = FunctorLoader<Cfg::BN, Cfg::SB, DgradB, false>;
template <class Cfg> using ADg2 = FunctorLoader<Cfg::BM, Cfg::SA, Dgrad2A, true>;
template <class Cfg> using BDg2 = FunctorLoader<Cfg::BN, Cfg::SB, Dgrad2B, false>;
template <class Cfg> using AWg = FunctorLoader<Cfg::BM, Cfg::SA, WgradA, true>;
template <class Cfg> using BWg = FunctorLoader<Cfg::BN, Cfg::SB, WgradB, true>;

bool valid(int B, int Ci, int H, int W, int Co, int KH, int KW, int stride, int pad) {
    if (!(B > 0 && Ci > 0 && Co > 0 && H > 0 && W > 0 && KH > 0 && KW > 0 && (stride == 1 || stride == 2) && pad >= 0 &&
          H + 2 * pad >= KH && W + 2 * pad >= KW))
        return false;
    const long OH = (H + 2 * pad - KH) / stride + 1, OW = (W + 2 * pad - KW) / stride + 1;
    const long lim = (1L << 31) - 1;                          // the gathers index with 32-bit offsets
    return (long)B * Ci * H * W <= lim && (long)B * Co * OH * OW <= lim && (long)Co * Ci * KH * KW <= lim;
}

// ------------------------------------------------------------------ forward product with a lean slab loop (round 4)
// On this part the VALU instructions of a SIMD do not overlap its MFMAs (scripts/micro/lds_mfma_loop.hip: 128 VALU instructions
// beside the 8 MFMAs of a 64x64-tile slab halve the rate, exactly 4 cycles each), and the generic engine above spends ~110
// VALU instructions per slab on 64-bit address arithmetic, per-element tap decomposition and LDS addresses.  This kernel is
// the same algorithm (64x64 tile, two register sets, two LDS stages, one barrier per slab, the same (k, k+1) MFMA pairing: with the
// same split factor the results are bit-identical) written so that nothing but the per-element bounds test is left to the VALU:
//   * A (weights, k contiguous): ONE 16-byte load per thread and slab at  uniform base (Wt + k0, SALU)  +  a 32-bit offset fixed
//     for the tile;
//   * B (im2col gather): a thread's four elements of a slab share its pixel and differ in k = k0 + wave + 4 i, which is
//     WAVE-UNIFORM — tap decomposition and tap offset are scalar; per element: two adds + two compares for the bounds, one add for
//     the 32-bit offset, two selects;
//   * every LDS address is a per-thread constant plus an immediate.
struct LeanB { float v[4]; };
typedef unsigned lean_u4 __attribute__((ext_vector_type(4)));
// TM: 64-row tiles per workgroup (wavefront tile 32 TM x 32): with TM = 2 every per-slab cost but the MFMAs is shared by twice the work
// R16 > 0 (TM = 2 staging; round 6, the 80-channel convolutions of the MPRNet transport map): output rows in units of SIXTEEN.  A
// product with 64 < M <= 16 R16 rows rode in two 64-row tiles, the second mostly empty (M = 80: 128 rows of MFMA work for 80; 154 us
// where 64 rows take 57).  Here one workgroup holds all 16 R16 rows of its 64 pixels: the four wavefronts side by side (16 pixels
// each), R16 accumulators of v_mfma_f32_16x16x4_f32 per wavefront — the same MACs per cycle as the 32x32x2 form, and per MFMA cycle
// the same number of LDS reads ((R16 + 1) per 32 R16 cycles against 2 per 64).  Staging, fetches and the slab loop are the TM = 2
// kernel's; the sum over k runs four at a time instead of two (another rounding order than the 64-row tiles: only shapes that take
// this form see it).
typedef float f32x4v __attribute__((ext_vector_type(4)));
template <int TM, int R16 = 0>
__global__ __launch_bounds__(256) void conv_fwd_lean_kernel(GemmDims d, const float* __restrict__ Wt, ConvGeom g, EpiP ep) {
    static_assert(R16 == 0 || (TM == 2 && R16 >= 5 && R16 <= 8) || (TM == 1 && R16 >= 1 && R16 <= 3), "the 16-row form stages a whole A tile");
    constexpr int LD = 68, LDA = 64 * TM + 4, STAGE = BK * (LDA + LD);
    __shared__ __attribute__((aligned(16))) float lds[2 * STAGE > 4096 ? 2 * STAGE : 4096];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int nblk = d.tilesM * d.tilesN;
    const int bid = xcd_remap(blockIdx.x, nblk);
    const int tm = bid % d.tilesM, tn = bid / d.tilesM;
    const int zs = blockIdx.z;
    const int m0 = tm * 64 * TM, n0 = tn * 64;
    const int kbeg = zs * d.kchunk;
    const int kend = min(d.K, kbeg + d.kchunk);
    const int nk = (kend - kbeg + BK - 1) / BK;
    // buffer resources (raw, byte addressed; out-of-range reads return 0): 32-bit per-thread offsets + scalar offsets, no 64-bit VALU
    const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc((void*)Wt, 0, (int)((unsigned)d.M * (unsigned)d.K * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t rB =
        __builtin_amdgcn_make_buffer_rsrc((void*)g.src, 0, (int)((unsigned)g.B * (unsigned)g.Ci * (unsigned)(g.H * g.W) * 4u), 0x00020000);

    // ---- A: row xx of the tile, k chunk kc.  Chunks past kend of a last partial slab read the row's next weights (or 0 past the
    // tensor): their B rows are zero, and x * 0 leaves the fmaf chain as the engine's 0 * 0 does.
    const int xx = tid >> 2, kc = (tid & 3) * 4;
    unsigned a_off[TM];
#pragma unroll
    for (int h = 0; h < TM; ++h) a_off[h] = ((unsigned)min(m0 + xx + 64 * h, d.M - 1) * (unsigned)d.K + (unsigned)kc) * 4u;
    // ---- B: pixel n0 + lane; rows wave + 4 i of every slab.  tapmask bit (ky * KW + kx) SET: that tap of this pixel lies OUTSIDE the
    // image (bit 31: always set, the "tap" of k >= kend).  An invalid element reads at offset | 0x80000000: past every tensor this
    // kernel takes (< 2 GiB, checked by the launcher), where a raw buffer returns 0.
    const int n = n0 + lane;
    unsigned pixb, tapmask = 0xffffffffu;
    {
        uint32_t b, pix, oy, ox;
        const bool xok = n < d.N;
        g.dP.divmod(xok ? n : 0, b, pix);
        g.dOW.divmod(pix, oy, ox);
        const int y0 = (int)(oy * g.stride) - g.pad, x0 = (int)(ox * g.stride) - g.pad;
        pixb = (unsigned)((int)b * g.Ci * g.H * g.W + y0 * g.W + x0) * 4u;      // (wraps for y0 / x0 < 0; the sum with a valid tap does not)
        for (int ky = 0; ky < g.KH; ++ky)
            for (int kx = 0; kx < g.KW; ++kx)
                if (xok && (unsigned)(y0 + ky) < (unsigned)g.H && (unsigned)(x0 + kx) < (unsigned)g.W) tapmask &= ~(1u << (ky * g.KW + kx));
    }
    const unsigned HWb = (unsigned)(g.H * g.W) * 4u, Wb = (unsigned)g.W * 4u;

    struct LeanA { lean_u4 q[TM]; };
    auto fetchA = [&](int kt, LeanA& qa) {
#pragma unroll
        for (int h = 0; h < TM; ++h) {
            const auto raw = __builtin_amdgcn_raw_buffer_load_b128(rA, a_off[h], (kbeg + kt * BK) * 4, 0);
            static_assert(sizeof(raw) == 16, "b128");
            qa.q[h] = __builtin_bit_cast(lean_u4, raw);   // (the builtin's own type is not an ext vector: a plain assignment splats element 0)
        }
    };
    // tap state of this wave's four rows, for the NEXT slab to fetch (slabs are fetched in order): channel offset, tap index.
    // Advanced by 16 k per slab without divisions (scalar unit: one per CU, shared by the four SIMDs)
    const int KHW = (int)g.dKHW.d, KW = (int)g.dKW.d;
    const int q16 = BK / KHW, r16 = BK - q16 * KHW;
    const unsigned kyM = 256u / (unsigned)KW + 1u;                 // ky = (rr * kyM) >> 8 for rr < KH * KW <= 31, KW <= 5
    unsigned cib[4];
    int rr_[4], kk_[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t ci, rr;
        kk_[i] = kbeg + wave + 4 * i;
        g.dKHW.divmod((uint32_t)kk_[i], ci, rr);
        cib[i] = ci * HWb;
        rr_[i] = (int)rr;
    }
    auto fetchB = [&](LeanB& r) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {                                  // wave-uniform: everything up to `voff` is scalar
            const unsigned rr = (unsigned)rr_[i];
            const unsigned ky = (rr * kyM) >> 8, kx = rr - ky * (unsigned)KW;
            const unsigned tapb = cib[i] + ky * Wb + kx * 4u;
            const unsigned bit = kk_[i] < kend ? rr : 31u;
            const unsigned bad = __builtin_amdgcn_ubfe(tapmask, bit, 1u);
            const unsigned voff = (pixb + tapb) | (bad << 31);         // outside the image / past kend: beyond the buffer -> reads 0
            r.v[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rB, voff, 0, 0));
            kk_[i] += BK;
            rr_[i] += r16;
            cib[i] += (unsigned)q16 * HWb;
            if (rr_[i] >= KHW) { rr_[i] -= KHW; cib[i] += HWb; }
        }
    };
    float* const As0 = lds + kc * LDA + xx;
    float* const Bs0 = lds + BK * LDA + wave * LD + lane;
    auto commit = [&](int stage, const LeanA& qa, const LeanB& r) {
        float* As = As0 + stage * STAGE;
#pragma unroll
        for (int h = 0; h < TM; ++h) {
            const unsigned q0 = qa.q[h][0], q1 = qa.q[h][1], q2 = qa.q[h][2], q3 = qa.q[h][3];      // (bit_cast of a vector ELEMENT expression reads element 0)
            As[64 * h] = __uint_as_float(q0); As[64 * h + LDA] = __uint_as_float(q1);
            As[64 * h + 2 * LDA] = __uint_as_float(q2); As[64 * h + 3 * LDA] = __uint_as_float(q3);
        }
        float* Bs = Bs0 + stage * STAGE;
#pragma unroll
        for (int i = 0; i < 4; ++i) Bs[4 * i * LD] = r.v[i];
    };

    f32x16 acc[TM][1];
    f32x4v acc16[R16 > 0 ? R16 : 1];
    if (R16 == 0) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][0][r] = 0.f;
    } else {
#pragma unroll
        for (int i = 0; i < (R16 > 0 ? R16 : 1); ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc16[i][r] = 0.f;
    }
    const int lm = lane & 31, lk = lane >> 5;
    const int l16 = lane & 15, lq = lane >> 4;                     // 16x16x4 operands: A[row l16][k lq], B[k lq][column l16]
    const float* const Fa0 = R16 == 0 ? lds + lk * LDA + wm * 32 * TM + lm : lds + lq * LDA + l16;
    const float* const Fb0 = R16 == 0 ? lds + BK * LDA + lk * LD + wn * 32 + lm : lds + BK * LDA + lq * LD + wave * 16 + l16;
    auto mma = [&](int stage) {
        const float* Fa = Fa0 + stage * STAGE;
        const float* Fb = Fb0 + stage * STAGE;
        if (R16 == 0) {
#pragma unroll
            for (int ks = 0; ks < BK / 2; ++ks) {
                const float bv = Fb[2 * ks * LD];
#pragma unroll
                for (int i = 0; i < TM; ++i) acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(Fa[2 * ks * LDA + 32 * i], bv, acc[i][0], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int ks = 0; ks < BK / 4; ++ks) {
                const float bv = Fb[4 * ks * LD];
#pragma unroll
                for (int i = 0; i < (R16 > 0 ? R16 : 1); ++i)
                    acc16[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(Fa[4 * ks * LDA + 16 * i], bv, acc16[i], 0, 0, 0);
            }
        }
    };

    // The slab loop has NO conditional fetch / commit: with a fetch under `if (kt + 2 < nk)` the compiler cannot count the younger
    // loads at the commit of the other register set and waits for ALL outstanding loads there (s_waitcnt vmcnt(0): the full memory
    // latency exposed every slab, lookahead zero — which is what held every form of this engine at ~60 TF/s).  Slabs past the
    // range are fetched as zeros (k >= kend) and, when the slab count is odd, one of them is multiplied: acc + x * 0.
    LeanA qa0, qa1;
    LeanB rb0, rb1;
    fetchA(0, qa0); fetchB(rb0);
    fetchA(1, qa1); fetchB(rb1);
    commit(0, qa0, rb0);
    __syncthreads();
    for (int kt = 0; kt < nk; kt += 2) {          // (three register sets / stages measured the same: 983 vs 977 us per forward sweep)
        fetchA(kt + 2, qa0); fetchB(rb0);
        mma(0);
        commit(1, qa1, rb1);
        __syncthreads();
        fetchA(kt + 3, qa1); fetchB(rb1);
        mma(1);
        commit(0, qa0, rb0);
        __syncthreads();
    }

    if (R16 > 0) {                                                  // lane: rows 16 i + 4 lq + r, column 16 wave + l16 of the tile
        const int nc = n0 + wave * 16 + l16;
        if (nc >= d.N) return;
        float* wsb = d.S > 1 ? d.ws + (long)zs * d.M * d.N : nullptr;
#pragma unroll
        for (int i = 0; i < (R16 > 0 ? R16 : 1); ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + 16 * i + 4 * lq + r;
                if (m >= d.M) continue;
                if (wsb) wsb[(long)m * d.N + nc] = acc16[i][r];
                else epi_store(ep, 0, 0, m, nc, acc16[i][r]);
            }
        return;
    }
    const int mrow0 = m0 + wm * 32 * TM + 4 * lk;
    const int ncol = n0 + wn * 32 + lm;
    if (d.S > 1) {
        float* wsb = d.ws + (long)zs * d.M * d.N;
        if ((d.N & 3) == 0) {
            epilogue_vec<TM, 1>(acc, lds + wave * 1024, wsb, d.N, nullptr, 0, nullptr, 1.f, 0.f, m0 + wm * 32 * TM, n0 + wn * 32, d.M, d.N, lane);
            return;
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mrow0 + 32 * i + (r & 3) + 8 * (r >> 2);
                if (m < d.M && ncol < d.N) wsb[(long)m * d.N + ncol] = acc[i][0][r];
            }
        return;
    }
    if (ncol < d.N) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mrow0 + 32 * i + (r & 3) + 8 * (r >> 2);
                if (m < d.M) epi_store(ep, 0, 0, m, ncol, acc[i][0][r]);
            }
    }
}

// The data gradients in the same form.  S2 = false: stride 1,  dX[b][ci][y][x] = sum_(co,ky,kx) Wt[co][ci][ky][kx] dY[b][co][y+p-ky][x+p-kx];
// S2 = true: the k4 s2 p1 gradient by output parity class cls = 2 py + px (grid z = 4 classes x S splits): taps ky = ky0 + 2 jy,
// ky0 = (py + p) & 1, over the half-resolution grid (y', x'), dY row y' + (py + p - ky0) / 2 - jy.  Both operands are "one row of 64 per
// instruction": A(m = ci, k) = Wt[...] at  ci * KH*KW * 4 (per thread)  +  a scalar,  B as in the forward kernel with the tap offsets
// NEGATIVE (scalar) and the validity mask over the taps per thread.
template <bool S2>
__global__ __launch_bounds__(256) void conv_dgrad_lean_kernel(GemmDims d, const float* __restrict__ Wt, ConvGeom g, EpiP ep) {
    constexpr int LD = 68, STAGE = 2 * BK * LD;
    __shared__ __attribute__((aligned(16))) float lds[2 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int nblk = d.tilesM * d.tilesN;
    const int bid = xcd_remap(blockIdx.x, nblk);
    const int tm = bid % d.tilesM, tn = bid / d.tilesM;
    const int zs = blockIdx.z;
    const int cls = S2 ? zs / d.S : 0, sp = S2 ? zs - cls * d.S : zs;
    const int m0 = tm * 64, n0 = tn * 64;
    const int kbeg = sp * d.kchunk;
    const int kend = min(d.K, kbeg + d.kchunk);
    const int nk = (kend - kbeg + BK - 1) / BK;
    const int KHW = (int)g.dKHW.d, KW = (int)g.dKW.d;             // (16, 4 for S2)
    const int TAPS = S2 ? 4 : KHW, TW = S2 ? 2 : KW;              // taps per output channel in k, taps per tap row
    const int OHW = g.OH * g.OW;
    const __amdgpu_buffer_rsrc_t rA =
        __builtin_amdgcn_make_buffer_rsrc((void*)Wt, 0, (int)((unsigned)g.Co * (unsigned)g.Ci * (unsigned)KHW * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t rB =
        __builtin_amdgcn_make_buffer_rsrc((void*)g.src, 0, (int)((unsigned)g.B * (unsigned)g.Co * (unsigned)OHW * 4u), 0x00020000);
    const int py = cls >> 1, px = cls & 1;
    const int ky0 = S2 ? ((py + g.pad) & 1) : 0, kx0 = S2 ? ((px + g.pad) & 1) : 0;

    // ---- A: lanes along k (16 consecutive k = consecutive taps of one or two output channels: a few cache lines per instruction; with a
    // lane per input channel every lane sat in its own line): thread (ka = tid & 15, rows xa + 16 i), its tap state advanced per slab
    const int ka = tid & 15, xa = tid >> 4;
    unsigned a_row[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a_row[i] = (unsigned)min(m0 + xa + 16 * i, d.M - 1) * (unsigned)KHW * 4u;
    // ---- B: pixel n0 + lane of the (class) grid; tapmask bit (ty * TW + tx) SET: that tap reads outside dY
    const int n = n0 + lane;
    unsigned pixb, tapmask = 0xffffffffu;
    {
        uint32_t b, pix, y, x;
        const bool xok = n < d.N;
        int by, bx;                                               // dY row / column of tap (0, 0)
        if (S2) {
            g.dHW2.divmod(xok ? n : 0, b, pix);
            g.dW2.divmod(pix, y, x);
            by = (int)y + ((py + g.pad - ky0) >> 1);
            bx = (int)x + ((px + g.pad - kx0) >> 1);
        } else {
            g.dHW.divmod(xok ? n : 0, b, pix);
            g.dW.divmod(pix, y, x);
            by = (int)y + g.pad;
            bx = (int)x + g.pad;
        }
        pixb = (unsigned)((int)b * g.Co * OHW + by * g.OW + bx) * 4u;
        const int TH = S2 ? 2 : g.KH;
        for (int ty = 0; ty < TH; ++ty)
            for (int tx = 0; tx < TW; ++tx)
                if (xok && (unsigned)(by - ty) < (unsigned)g.OH && (unsigned)(bx - tx) < (unsigned)g.OW) tapmask &= ~(1u << (ty * TW + tx));
    }
    const unsigned OHWb = (unsigned)OHW * 4u, OWb = (unsigned)g.OW * 4u, AOb = (unsigned)g.Ci * (unsigned)KHW * 4u;
    const int q16 = BK / TAPS, r16 = BK - q16 * TAPS;
    const unsigned tyM = 256u / (unsigned)TW + 1u;
    unsigned coB[4];                                              // byte offset of the output channel in dY (rows wave + 4 i: scalar)
    int rr_[4], kk_[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        kk_[i] = kbeg + wave + 4 * i;
        const unsigned co = (unsigned)kk_[i] / (unsigned)TAPS;
        rr_[i] = kk_[i] - (int)co * TAPS;
        coB[i] = co * OHWb;
    }
    unsigned coA;                                                 // this thread's k = kbeg + ka (+ 16 per slab): channel offset in Wt, tap
    int rrA;
    {
        const unsigned co = (unsigned)(kbeg + ka) / (unsigned)TAPS;
        rrA = kbeg + ka - (int)co * TAPS;
        coA = co * AOb;
    }
    auto fetch = [&](LeanB& ra, LeanB& rb) {
        {
            const unsigned rr = (unsigned)rrA;
            const unsigned tapA = S2 ? ((unsigned)(ky0 + 2 * (int)(rr >> 1)) * 4u + (unsigned)(kx0 + 2 * (int)(rr & 1))) * 4u : rr * 4u;
            const unsigned ko = coA + tapA;                        // (k >= kend: the B rows are zero; past the tensor a raw buffer reads 0)
#pragma unroll
            for (int i = 0; i < 4; ++i) ra.v[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rA, a_row[i] + ko, 0, 0));
            rrA += r16;
            coA += (unsigned)q16 * AOb;
            if (rrA >= TAPS) { rrA -= TAPS; coA += AOb; }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {                              // wave-uniform up to the per-lane offsets
            const unsigned rr = (unsigned)rr_[i];
            const unsigned ty = (rr * tyM) >> 8, tx = rr - ty * (unsigned)TW;
            const unsigned tapb = coB[i] - ty * OWb - tx * 4u;
            const unsigned bit = kk_[i] < kend ? rr : 31u;
            const unsigned bad = __builtin_amdgcn_ubfe(tapmask, bit, 1u);
            const unsigned voff = (pixb + tapb) | (bad << 31);
            rb.v[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rB, voff, 0, 0));
            kk_[i] += BK;
            rr_[i] += r16;
            coB[i] += (unsigned)q16 * OHWb;
            if (rr_[i] >= TAPS) { rr_[i] -= TAPS; coB[i] += OHWb; }
        }
    };
    float* const As0 = lds + ka * LD + xa;
    float* const Bs0 = lds + BK * LD + wave * LD + lane;
    auto commit = [&](int stage, const LeanB& ra, const LeanB& rb) {
        float* As = As0 + stage * STAGE;
        float* Bs = Bs0 + stage * STAGE;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            As[16 * i] = ra.v[i];
            Bs[4 * i * LD] = rb.v[i];
        }
    };

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int lm = lane & 31, lk = lane >> 5;
    const float* const Fa0 = lds + lk * LD + wm * 32 + lm;
    const float* const Fb0 = lds + BK * LD + lk * LD + wn * 32 + lm;
    auto mma = [&](int stage) {
        const float* Fa = Fa0 + stage * STAGE;
        const float* Fb = Fb0 + stage * STAGE;
#pragma unroll
        for (int ks = 0; ks < BK / 2; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Fa[2 * ks * LD], Fb[2 * ks * LD], acc, 0, 0, 0);
    };

    LeanB ra0, ra1, rb0, rb1;
    fetch(ra0, rb0);
    fetch(ra1, rb1);
    commit(0, ra0, rb0);
    __syncthreads();
    for (int kt = 0; kt < nk; kt += 2) {
        fetch(ra0, rb0);
        mma(0);
        commit(1, ra1, rb1);
        __syncthreads();
        fetch(ra1, rb1);
        mma(1);
        commit(0, ra0, rb0);
        __syncthreads();
    }

    const int mrow0 = m0 + wm * 32 + 4 * lk;
    const int ncol = n0 + wn * 32 + lm;
    if (d.S > 1) {
        float* wsb = d.ws + (long)zs * d.M * d.N;
        if ((d.N & 3) == 0) {
            f32x16 a1[1][1];
            a1[0][0] = acc;
            epilogue_vec<1, 1>(a1, lds + wave * 1024, wsb, d.N, nullptr, 0, nullptr, 1.f, 0.f, m0 + wm * 32, n0 + wn * 32, d.M, d.N, lane);
            return;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = mrow0 + (r & 3) + 8 * (r >> 2);
            if (m < d.M && ncol < d.N) wsb[(long)m * d.N + ncol] = acc[r];
        }
        return;
    }
    if (ncol < d.N) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = mrow0 + (r & 3) + 8 * (r >> 2);
            if (m < d.M) epi_store(ep, cls, 0, m, ncol, acc[r]);
        }
    }
}

template <bool S2>
int launch_conv_dgrad_lean(GemmDims d, const float* Wt, const ConvGeom& g, const EpiP& ep, hipStream_t st) {
    const int Z = S2 ? 4 : 1;
    d.tilesM = cdiv(d.M, 64);
    d.tilesN = cdiv(d.N, 64);
    EpiP epv = ep;
    epv.vec = 0;
    note_kernel(S2 ? "conv_dgrad_lean_kernel<true>" : "conv_dgrad_lean_kernel<false>");
    RCOT_LAUNCH((conv_dgrad_lean_kernel<S2>), dim3(d.tilesM * d.tilesN, 1, Z * d.S), dim3(256), 0, st, d, Wt, g, epv);
    RCOT_LAUNCH_CHECK();
    if (d.S > 1) {
        launch_splitk_reduce(d, ep, Z, st);
        RCOT_LAUNCH_CHECK();
    }
    return RCOT_OK;
}

// The weight gradient in the same form:  dWt[co][(ci, ky, kx)] = sum_(b, oy, ox) dY[b][co][oy][ox] X[b][ci][oy s + ky - p][ox s + kx - p].
// k = (b, pixel) is the contiguous axis of BOTH operands, so lanes run along k (thread (kq = tid & 15, rows / columns xq + 16 i)): the
// pixel state (image, row, column, the two base offsets) is advanced once per slab and thread, an element adds its constant row /
// tap offset and tests its two bounds.
// R16 > 0 (round 6): 16 R16 output rows per workgroup on v_mfma_f32_16x16x4_f32, the four wavefronts side by side — the form of
// conv_fwd_lean_kernel<2, R16> for 64 < Co <= 16 R16 (the 80-channel level of the MPRNet transport map)
template <int R16>
__global__ __launch_bounds__(256) void conv_wgrad_lean_kernel(GemmDims d, const float* __restrict__ dY, ConvGeom g, EpiP ep) {
    constexpr int NA = R16 > 0 ? R16 : 4, TMR = 16 * NA;          // 16-row groups of the A tile a thread fetches; rows per tile
    constexpr int LD = 68, LDA = R16 > 0 ? TMR + 4 : LD, STAGE = BK * (LDA + LD);
    __shared__ __attribute__((aligned(16))) float lds[2 * STAGE > 4096 ? 2 * STAGE : 4096];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int nblk = d.tilesM * d.tilesN;
    const int bid = xcd_remap(blockIdx.x, nblk);
    const int tm = bid % d.tilesM, tn = bid / d.tilesM;
    const int zs = blockIdx.z;
    const int m0 = tm * TMR, n0 = tn * 64;
    const int kbeg = zs * d.kchunk;
    const int kend = min(d.K, kbeg + d.kchunk);
    const int nk = (kend - kbeg + BK - 1) / BK;
    const int P = (int)g.dP.d, HW = g.H * g.W;
    const __amdgpu_buffer_rsrc_t rA =
        __builtin_amdgcn_make_buffer_rsrc((void*)dY, 0, (int)((unsigned)g.B * (unsigned)g.Co * (unsigned)P * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t rB =
        __builtin_amdgcn_make_buffer_rsrc((void*)g.src, 0, (int)((unsigned)g.B * (unsigned)g.Ci * (unsigned)HW * 4u), 0x00020000);
    const int kq = tid & 15, xq = tid >> 4;
    unsigned a_row[NA], b_row[4];
    int kyi[4], kxi[4];
#pragma unroll
    for (int i = 0; i < NA; ++i) a_row[i] = (unsigned)min(m0 + xq + 16 * i, d.M - 1) * (unsigned)P * 4u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = n0 + xq + 16 * i;
        uint32_t ci, r, ky, kx;
        g.dKHW.divmod((uint32_t)min(n, d.N - 1), ci, r);
        g.dKW.divmod(r, ky, kx);
        b_row[i] = (ci * (unsigned)HW + ky * (unsigned)g.W + kx) * 4u;
        kyi[i] = n < d.N ? (int)ky : (1 << 20);                   // (a column past N fails its row test)
        kxi[i] = (int)kx;
    }
    // pixel state of k = kbeg + kq (+ 16 per slab)
    int kk = kbeg + kq, pix;
    unsigned koA, bB;
    {
        uint32_t b, px_;
        g.dP.divmod((uint32_t)min(kk, d.K - 1), b, px_);
        pix = (int)px_;
        koA = (b * (unsigned)g.Co * (unsigned)P + px_) * 4u;
        bB = b * (unsigned)g.Ci * (unsigned)HW * 4u;
    }
    const unsigned wrapA = ((unsigned)g.Co * (unsigned)P - (unsigned)P) * 4u, wrapB = (unsigned)g.Ci * (unsigned)HW * 4u;

    struct LeanAr { float v[NA]; };
    auto fetch = [&](LeanAr& ra, LeanB& rb) {
        uint32_t oy, ox;
        g.dOW.divmod((uint32_t)pix, oy, ox);
        const int iy0 = (int)oy * g.stride - g.pad, ix0 = (int)ox * g.stride - g.pad;
        const unsigned koB = bB + (unsigned)(iy0 * g.W + ix0) * 4u;
        const unsigned kbad = kk < kend ? 0u : 0x80000000u;
#pragma unroll
        for (int i = 0; i < NA; ++i) ra.v[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rA, (a_row[i] + koA) | kbad, 0, 0));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool ok = (unsigned)(iy0 + kyi[i]) < (unsigned)g.H && (unsigned)(ix0 + kxi[i]) < (unsigned)g.W;
            const unsigned voff = (b_row[i] + koB) | (ok ? kbad : 0x80000000u);
            rb.v[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rB, voff, 0, 0));
        }
        kk += BK;
        pix += BK;
        koA += BK * 4u;
        if (pix >= P) { pix -= P; koA += wrapA; bB += wrapB; }      // (P >= 16: at most one image boundary per slab)
    };
    float* const As0 = lds + kq * LDA + xq;
    float* const Bs0 = lds + BK * LDA + kq * LD + xq;
    auto commit = [&](int stage, const LeanAr& ra, const LeanB& rb) {
        float* As = As0 + stage * STAGE;
        float* Bs = Bs0 + stage * STAGE;
#pragma unroll
        for (int i = 0; i < NA; ++i) As[16 * i] = ra.v[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) Bs[16 * i] = rb.v[i];
    };

    f32x16 acc;
    f32x4v acc16[NA];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc16[i][r] = 0.f;
    const int lm = lane & 31, lk = lane >> 5;
    const int l16 = lane & 15, lq = lane >> 4;
    const float* const Fa0 = R16 == 0 ? lds + lk * LDA + wm * 32 + lm : lds + lq * LDA + l16;
    const float* const Fb0 = R16 == 0 ? lds + BK * LDA + lk * LD + wn * 32 + lm : lds + BK * LDA + lq * LD + wave * 16 + l16;
    auto mma = [&](int stage) {
        const float* Fa = Fa0 + stage * STAGE;
        const float* Fb = Fb0 + stage * STAGE;
        if (R16 == 0) {
#pragma unroll
            for (int ks = 0; ks < BK / 2; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Fa[2 * ks * LDA], Fb[2 * ks * LD], acc, 0, 0, 0);
        } else {
#pragma unroll
            for (int ks = 0; ks < BK / 4; ++ks) {
                const float bv = Fb[4 * ks * LD];
#pragma unroll
                for (int i = 0; i < NA; ++i) acc16[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(Fa[4 * ks * LDA + 16 * i], bv, acc16[i], 0, 0, 0);
            }
        }
    };

    LeanAr ra0, ra1;
    LeanB rb0, rb1;
    fetch(ra0, rb0);
    fetch(ra1, rb1);
    commit(0, ra0, rb0);
    __syncthreads();
    for (int kt = 0; kt < nk; kt += 2) {
        fetch(ra0, rb0);
        mma(0);
        commit(1, ra1, rb1);
        __syncthreads();
        fetch(ra1, rb1);
        mma(1);
        commit(0, ra0, rb0);
        __syncthreads();
    }

    if (R16 > 0) {                                                  // lane: rows 16 i + 4 lq + r, column 16 wave + l16 of the tile
        const int nc = n0 + wave * 16 + l16;
        if (nc >= d.N) return;
        float* wsb = d.S > 1 ? d.ws + (long)zs * d.M * d.N : nullptr;
#pragma unroll
        for (int i = 0; i < NA; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + 16 * i + 4 * lq + r;
                if (m >= d.M) continue;
                if (wsb) wsb[(long)m * d.N + nc] = acc16[i][r];
                else epi_store(ep, 0, 0, m, nc, acc16[i][r]);
            }
        return;
    }
    const int mrow0 = m0 + wm * 32 + 4 * lk;
    const int ncol = n0 + wn * 32 + lm;
    if (d.S > 1) {
        float* wsb = d.ws + (long)zs * d.M * d.N;
        if ((d.N & 3) == 0) {
            f32x16 a1[1][1];
            a1[0][0] = acc;
            epilogue_vec<1, 1>(a1, lds + wave * 1024, wsb, d.N, nullptr, 0, nullptr, 1.f, 0.f, m0 + wm * 32, n0 + wn * 32, d.M, d.N, lane);
            return;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = mrow0 + (r & 3) + 8 * (r >> 2);
            if (m < d.M && ncol < d.N) wsb[(long)m * d.N + ncol] = acc[r];
        }
        return;
    }
    if (ncol < d.N) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = mrow0 + (r & 3) + 8 * (r >> 2);
            if (m < d.M) epi_store(ep, 0, 0, m, ncol, acc[r]);
        }
    }
}

// rows of the forward product and the weight gradient in one workgroup, sixteen at a time: 65..80 rows as five groups of sixteen;
// 17..32 / 33..48 rows as two / three groups (the 24- and 48-channel resampling convolutions of the Restormer map, which would
// otherwise ride in a 64-row tile; NOTES round 6)
int conv_r16(int M) {
    if (M > 64 && M <= 80) return 5;
    if (M > 16 && M <= 32) return 2;
    if (M > 32 && M <= 48) return 3;
    return 0;
}
bool conv_rows80(int M) { return conv_r16(M) == 5; }

int launch_conv_wgrad_lean(GemmDims d, const float* dY, const ConvGeom& g, const EpiP& ep, hipStream_t st) {
    const int r16 = conv_r16(d.M);
    d.tilesM = r16 ? 1 : cdiv(d.M, 64);
    d.tilesN = cdiv(d.N, 64);
    EpiP epv = ep;
    epv.vec = 0;
    note_kernel(r16 == 5 ? "conv_wgrad_lean_kernel<5>" : r16 == 3 ? "conv_wgrad_lean_kernel<3>" : r16 == 2 ? "conv_wgrad_lean_kernel<2>" : "conv_wgrad_lean_kernel");
    const dim3 grid(d.tilesM * d.tilesN, 1, d.S);
    if (r16 == 5) RCOT_LAUNCH((conv_wgrad_lean_kernel<5>), grid, dim3(256), 0, st, d, dY, g, epv);
    else if (r16 == 3) RCOT_LAUNCH((conv_wgrad_lean_kernel<3>), grid, dim3(256), 0, st, d, dY, g, epv);
    else if (r16 == 2) RCOT_LAUNCH((conv_wgrad_lean_kernel<2>), grid, dim3(256), 0, st, d, dY, g, epv);
    else RCOT_LAUNCH((conv_wgrad_lean_kernel<0>), grid, dim3(256), 0, st, d, dY, g, epv);
    RCOT_LAUNCH_CHECK();
    if (d.S > 1) {
        launch_splitk_reduce(d, ep, 1, st);
        RCOT_LAUNCH_CHECK();
    }
    return RCOT_OK;
}

int launch_conv_fwd_lean(GemmDims d, const float* Wt, const ConvGeom& g, const EpiP& ep, hipStream_t st) {
    // 128-row tiles where the 64-row plan has >= 1024 workgroups (measured per layer at B = 16: +3..9 % there, -7..-12 % below)
    const bool two = (d.M % 128) == 0 && (long)cdiv(d.M, 64) * cdiv(d.N, 64) * d.S >= 1024;
    // 64 < M <= 80 (the 80-channel level of the MPRNet transport map): all rows in one workgroup, sixteen at a time
    const int r16 = conv_r16(d.M);
    const bool rows80 = r16 == 5;
    d.tilesM = r16 ? 1 : cdiv(d.M, two ? 128 : 64);
    d.tilesN = cdiv(d.N, 64);
    EpiP epv = ep;
    epv.vec = 0;
    note_kernel(rows80 ? "conv_fwd_lean_kernel<2, 5>" : r16 == 3 ? "conv_fwd_lean_kernel<1, 3>" : r16 == 2 ? "conv_fwd_lean_kernel<1, 2>" : two ? "conv_fwd_lean_kernel<2>" : "conv_fwd_lean_kernel<1>");
    if (rows80) RCOT_LAUNCH((conv_fwd_lean_kernel<2, 5>), dim3(d.tilesM * d.tilesN, 1, d.S), dim3(256), 0, st, d, Wt, g, epv);
    else if (r16 == 3) RCOT_LAUNCH((conv_fwd_lean_kernel<1, 3>), dim3(d.tilesM * d.tilesN, 1, d.S), dim3(256), 0, st, d, Wt, g, epv);
    else if (r16 == 2) RCOT_LAUNCH((conv_fwd_lean_kernel<1, 2>), dim3(d.tilesM * d.tilesN, 1, d.S), dim3(256), 0, st, d, Wt, g, epv);
    else if (two) RCOT_LAUNCH((conv_fwd_lean_kernel<2>), dim3(d.tilesM * d.tilesN, 1, d.S), dim3(256), 0, st, d, Wt, g, epv);
    else RCOT_LAUNCH((conv_fwd_lean_kernel<1>), dim3(d.tilesM * d.tilesN, 1, d.S), dim3(256), 0, st, d, Wt, g, epv);
    RCOT_LAUNCH_CHECK();
    if (d.S > 1) {
        launch_splitk_reduce(d, ep, 1, st);
        RCOT_LAUNCH_CHECK();
    }
    return RCOT_OK;
}

bool dgrad_lean() {
    static const int on = getenv("RCOT_CONV_LEAN") ? atoi(getenv("RCOT_CONV_LEAN")) : 1;
    return on != 0 && on != 2;          // (2: forward only, for A/B runs)
}

}  // namespace

extern "C" {

int rcot_conv2d_fwd(const float* X, const float* Wt, const float* bias, float* Y, int B, int Ci, int H, int W,
                    int Co, int KH, int KW, int stride, int pad, float lrelu, int cmap, const float* R, const float* mask,
                    float mslope, float* ws, size_t ws_bytes, void* stream) {
    if (!X || !Wt || !Y || !valid(B, Ci, H, W, Co, KH, KW, stride, pad) || cmap < 0 || cmap > 2) return RCOT_EINVAL;
    if (mask && cmap != 0) return RCOT_EINVAL;
    ConvGeom g = make_geom(X, B, Ci, Co, H, W, KH, KW, stride, pad);
    if (cmap == 1 && ((g.OH | g.OW) & 1)) return RCOT_EINVAL;
    if (cmap == 2 && (Co & 3)) return RCOT_EINVAL;
    if (cmap != 0 && R) return RCOT_EINVAL;
    if (stride == 1 && KH == KW && cmap == 0 && !mask) {     // RGB output: direct kernel
        const int rc = try_conv_few_out(X, Wt, 0, (long)Ci * KH * KW, KH * KW, KW, 1, bias, R, Y, B, Ci, H, W, Co, KH, pad, lrelu,
                                        0.f, (hipStream_t)stream);
        if (rc != NOT_ELIGIBLE) return rc;
    }
    const int P = g.OH * g.OW;
    if ((long)B * P > 0x7fffffffL) return RCOT_EINVAL;
    GemmDims d{};
    d.M = Co; d.N = B * P; d.K = Ci * KH * KW; d.Zi = 1;
    StridedP ap{Wt, (long)d.K, 1, 0, 0, Co, d.K};
    EpiP ep{};
    ep.C = Y; ep.ldc = P; ep.sCo = (long)Co * P;            // shuffles permute within the same per-image volume
    ep.R = R; ep.ldr = P; ep.sRo = (long)Co * P;
    ep.bias = bias;
    ep.alpha = 1.f; ep.beta = 0.f; ep.lrelu = lrelu;
    ep.cmap = cmap; ep.mapW = g.OW; ep.mapH = g.OH;
    ep.fold = 1; ep.foldP.init(P);
    ep.mask = mask; ep.mslope = mslope;
    bool big;
    static const int lean = getenv("RCOT_CONV_LEAN") ? atoi(getenv("RCOT_CONV_LEAN")) : 1;
    const bool lean_f = lean && (d.K & 3) == 0 && (reinterpret_cast<uintptr_t>(Wt) & 15) == 0 && (long)B * Ci * H * W < (1L << 29) &&
                        (long)Co * d.K < (1L << 29) && KH * KW <= 31 && KW <= 7;
    if (lean_f && conv_rows80(Co)) {          // ONE row tile per 64 pixels (the 16-row form): the split factor is planned for that grid —
        d.M = 64;                             // planned as two tiles of 128 pixels, the 80-channel level at 4 x 128 x 128 split in two
        big = plan_splitk(d, 1, ws, ws_bytes);   // for nothing (94 -> 85 us, and no reduce launch behind it)
        d.M = Co;
        while (d.S > 1 && (size_t)d.M * d.N * d.S * sizeof(float) > ws_bytes) {
            --d.S;
            cut_k(d);
        }
    } else {
        big = plan_splitk(d, 1, ws, ws_bytes);
    }
    if (d.S > 1 && (size_t)d.M * d.N * d.S * sizeof(float) > ws_bytes) return RCOT_EWORKSPACE;
    // the lean 64x64 kernel takes every shape it can (same split plan, so results do not depend on which kernel ran); RCOT_CONV_LEAN=0:
    // the generic engine
    if (lean_f) return launch_conv_fwd_lean(d, Wt, g, ep, (hipStream_t)stream);
    if (big) return launch_gemm_cfg<CfgL, AStrK<CfgL>, StridedP, BFwd<CfgL>, ConvGeom, true>(d, ap, g, ep, 1, (hipStream_t)stream);
    return launch_gemm_cfg<CfgS, AStrK<CfgS>, StridedP, BFwd<CfgS>, ConvGeom, true>(d, ap, g, ep, 1, (hipStream_t)stream);
}

int rcot_conv2d_dgrad(const float* dY, const float* Wt, float* dX, int B, int Ci, int H, int W, int Co, int KH,
                      int KW, int stride, int pad, float beta, const float* mask, float mslope, float* ws, size_t ws_bytes,
                      void* stream) {
    if (!dY || !Wt || !dX || !valid(B, Ci, H, W, Co, KH, KW, stride, pad)) return RCOT_EINVAL;
    if (stride == 1 && KH == KW && !mask) {                   // gradient w.r.t. an RGB image: the transposed, rotated filter
        const int rc = try_conv_few_out(dY, Wt, (long)KH * KW - 1, KH * KW, (long)Ci * KH * KW, -KW, -1, nullptr, nullptr, dX, B, Co,
                                        H, W, Ci, KH, pad, 1.f, beta, (hipStream_t)stream);
        if (rc != NOT_ELIGIBLE) return rc;
    }
    ConvGeom gb = make_geom(dY, B, Ci, Co, H, W, KH, KW, stride, pad);
    ConvGeom ga = gb;
    ga.src = Wt;
    if ((long)B * H * W > 0x7fffffffL) return RCOT_EINVAL;
    EpiP ep{};
    ep.C = dX; ep.sCo = (long)Ci * H * W;
    ep.alpha = 1.f; ep.beta = beta; ep.lrelu = 1.f;
    ep.fold = 1;
    ep.mask = mask; ep.mslope = mslope;
    GemmDims d{};
    d.M = Ci; d.Zi = 1;
    bool big;
    if (stride == 2) {
        if (KH != 4 || KW != 4 || (H & 1) || (W & 1)) return RCOT_EINVAL;   // the critic's k4s2p1 only
        const int P2 = (H >> 1) * (W >> 1);
        d.N = B * P2; d.K = Co * 4;
        ep.cmap = 3; ep.mapH = H >> 1; ep.mapW = W >> 1; ep.foldP.init(P2);
        big = plan_splitk(d, 4, ws, ws_bytes);
        if (d.S > 1 && (size_t)d.M * d.N * 4 * d.S * sizeof(float) > ws_bytes) return RCOT_EWORKSPACE;
        if (dgrad_lean() && (long)B * Co * gb.OH * gb.OW < (1L << 29) && (long)Co * Ci * 16 < (1L << 29))
            return launch_conv_dgrad_lean<true>(d, Wt, gb, ep, (hipStream_t)stream);
        if (big) return launch_gemm_cfg<CfgL, ADg2<CfgL>, ConvGeom, BDg2<CfgL>, ConvGeom, true>(d, ga, gb, ep, 4, (hipStream_t)stream);
        return launch_gemm_cfg<CfgS, ADg2<CfgS>, ConvGeom, BDg2<CfgS>, ConvGeom, true>(d, ga, gb, ep, 4, (hipStream_t)stream);
    }
    d.N = B * H * W; d.K = Co * KH * KW;
    ep.ldc = (long)H * W; ep.foldP.init(H * W);
    big = plan_splitk(d, 1, ws, ws_bytes);
    if (d.S > 1 && (size_t)d.M * d.N * d.S * sizeof(float) > ws_bytes) return RCOT_EWORKSPACE;
    if (dgrad_lean() && (long)B * Co * gb.OH * gb.OW < (1L << 29) && (long)Co * Ci * KH * KW < (1L << 29) && KH * KW <= 31 && KW <= 7)
        return launch_conv_dgrad_lean<false>(d, Wt, gb, ep, (hipStream_t)stream);
    if (big) return launch_gemm_cfg<CfgL, ADg<CfgL>, ConvGeom, BDg<CfgL>, ConvGeom, true>(d, ga, gb, ep, 1, (hipStream_t)stream);
    return launch_gemm_cfg<CfgS, ADg<CfgS>, ConvGeom, BDg<CfgS>, ConvGeom, true>(d, ga, gb, ep, 1, (hipStream_t)stream);
}

int rcot_conv2d_wgrad(const float* dY, const float* X, float* dWt, int B, int Ci, int H, int W, int Co, int KH,
                      int KW, int stride, int pad, float beta, float* ws, size_t ws_bytes, void* stream) {
    if (!dY || !X || !dWt || !valid(B, Ci, H, W, Co, KH, KW, stride, pad)) return RCOT_EINVAL;
    if (stride == 1 && KH == KW) {
        const int rc = try_wgrad_few_out(dY, X, dWt, B, Ci, H, W, Co, KH, pad, beta, (hipStream_t)stream);
        if (rc != NOT_ELIGIBLE) return rc;
    }
    ConvGeom gb = make_geom(X, B, Ci, Co, H, W, KH, KW, stride, pad);
    ConvGeom ga = gb;
    ga.src = dY;
    GemmDims d{};
    d.M = Co; d.N = Ci * KH * KW; d.K = B * gb.OH * gb.OW; d.Zi = 1;
    bool big;
    const bool lean_w = dgrad_lean() && gb.OH * gb.OW >= 16 && (long)B * Ci * H * W < (1L << 29) && (long)B * Co * gb.OH * gb.OW < (1L << 29);
    if (lean_w && conv_rows80(Co)) {          // one row tile instead of two: the split factor is planned for that grid
        d.M = 64;
        big = plan_splitk(d, 1, ws, ws_bytes);
        d.M = Co;
        while (d.S > 1 && (size_t)d.M * d.N * d.S * sizeof(float) > ws_bytes) {
            --d.S;
            cut_k(d);
        }
    } else {
        big = plan_splitk(d, 1, ws, ws_bytes);
    }
    if (d.S > 1 && (size_t)d.M * d.N * d.S * sizeof(float) > ws_bytes) return RCOT_EWORKSPACE;
    EpiP ep{};
    ep.C = dWt; ep.ldc = d.N;
    ep.alpha = 1.f; ep.beta = beta; ep.lrelu = 1.f;
    if (lean_w) return launch_conv_wgrad_lean(d, dY, gb, ep, (hipStream_t)stream);
    if (big) return launch_gemm_cfg<CfgL, AWg<CfgL>, ConvGeom, BWg<CfgL>, ConvGeom, true>(d, ga, gb, ep, 1, (hipStream_t)stream);
    return launch_gemm_cfg<CfgS, AWg<CfgS>, ConvGeom, BWg<CfgS>, ConvGeom, true>(d, ga, gb, ep, 1, (hipStream_t)stream);
}

}  // extern "C"
