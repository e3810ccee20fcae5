// Depthwise 3x3 stencils of the transport map (pad 1): plain, GELU-gated, transposed (the data gradient), weight gradient, and the
// one-pass backward kernels that fuse them.  NCHW fp32; pixels are the fastest axis so a wavefront always touches 64 consecutive
// pixels of one channel plane (coalesced 256 B segments).  The family's helpers exist once each, here (dwconv_wgrad_kernel keeps a
// private patch load, see there; conv_thin.hip has rolling-row strips of its own for the dense thin convolutions).
#include <type_traits>
#include "common.h"
#include "../../include/rcot_hip.h"

using namespace rcot;

namespace {

// ------------------------------------------------------------------ rows and patches
// A Row6 is the float4 a thread owns plus one halo pixel per side (columns x0-1 .. x0+4).  The halo pixels come from one of two places:
//  - scalar loads (load_row6), for any W % 4 == 0;
//  - the NEIGHBOURING LANES (land_row6), when consecutive lanes own the adjacent pixel quads of the same row (W/4 divides 64: rows
//    start at lane boundaries of that size, nb_lanes_ok): lanes -1 / +1 hand them over by DPP wave shifts (VALU speed) instead of two
//    more scalar loads per row, and nothing is branched on (every lane executes the shifts; out-of-range rows land as zeros).
struct Row6 { float v[6]; };
struct Patch { Row6 r[6]; };       // rows y0-1..y0+4 of a 4x4 output block

__device__ __forceinline__ float from_lane_below(float v) {      // lane i <- lane i-1   (v_mov_b32_dpp wave_shr:1)
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float from_lane_above(float v) {      // lane i <- lane i+1   (wave_shl:1)
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, true));
}

__device__ __forceinline__ float keep_bits(float v, int mask) {   // v (mask = -1) or +0.0 (mask = 0), bit for bit
    return __builtin_bit_cast(float, __builtin_bit_cast(int, v) & mask);
}

// row y of the plane (zeros outside it) with scalar-load halo pixels
__device__ __forceinline__ void load_row6(const float* __restrict__ plane, int H, int W, int y, int x0, Row6& r) {
    if (y < 0 || y >= H) {
#pragma unroll
        for (int j = 0; j < 6; ++j) r.v[j] = 0.f;
        return;
    }
    const float* q = plane + (long)y * W + x0;
    const float4 c = *reinterpret_cast<const float4*>(q);
    r.v[0] = (x0 > 0) ? q[-1] : 0.f;
    r.v[1] = c.x; r.v[2] = c.y; r.v[3] = c.z; r.v[4] = c.w;
    r.v[5] = (x0 + 4 < W) ? q[4] : 0.f;
}

// Branch-free landing of a quad that is already in registers: zeros unless the row exists (`ok`), halo pixels from lanes -1 / +1
// unless the quad touches the plane's left / right edge.  Every lane that runs the surrounding code must run this too, so a call never
// sits under a condition that differs between the lanes of a row; the kernels REQUEST their rows beforehand (unconditional 16-byte
// loads from clamped row indices): a load inside `if (row exists)` followed by the lane shift costs one full memory round trip per row.
__device__ __forceinline__ void land_row6(const float4& q, bool ok, bool has_l, bool has_r, Row6& r) {
    // zeros by a bit mask, one v_and per value: as `ok ? q : 0` the compiler builds a branch around four copies (eight v_mov per row)
    const int m = ok ? -1 : 0;
    const float4 c = make_float4(keep_bits(q.x, m), keep_bits(q.y, m), keep_bits(q.z, m), keep_bits(q.w, m));
    const float l = from_lane_below(c.w), rr = from_lane_above(c.x);
    r.v[0] = has_l ? l : 0.f;
    r.v[1] = c.x; r.v[2] = c.y; r.v[3] = c.z; r.v[4] = c.w;
    r.v[5] = has_r ? rr : 0.f;
}

// Register blocking: one thread owns a 4x4 output block and reads its 6x6 input patch once (6 float4 rows + halo pixels): 2.25 loads
// per output instead of 4.5 for a 1x4 strip; a wavefront covers 64 consecutive quads of a plane row-block.  H % 4 == 0, W % 4 == 0.
__device__ __forceinline__ void load_patch(const float* __restrict__ plane, int H, int W, int y0, int x0, Patch& p) {
#pragma unroll
    for (int dy = 0; dy < 6; ++dy) load_row6(plane, H, W, y0 + dy - 1, x0, p.r[dy]);
}
// the neighbour-lane form, 6 loads per patch instead of 18, split in two so that a kernel can request all the rows it needs before it
// touches any of them
struct PatchRows { float4 c[6]; };
__device__ __forceinline__ void patch_request(const float* __restrict__ plane, int H, int W, int y0, int x0, PatchRows& q) {
#pragma unroll
    for (int dy = 0; dy < 6; ++dy) {
        const int yy = min(max(y0 + dy - 1, 0), H - 1);
        q.c[dy] = *reinterpret_cast<const float4*>(plane + (long)yy * W + x0);
    }
}
__device__ __forceinline__ void patch_land(const PatchRows& q, int H, int W, int y0, int x0, Patch& p) {
    const bool has_l = x0 > 0, has_r = x0 + 4 < W;
#pragma unroll
    for (int dy = 0; dy < 6; ++dy) {
        const int yy = y0 + dy - 1;
        land_row6(q.c[dy], yy >= 0 && yy < H, has_l, has_r, p.r[dy]);
    }
}

// one output quad from three input rows
// (ROT: with the 180-degree rotated filter, read in place as w[8 - i])
template <bool ROT = false>
__device__ __forceinline__ void stencil_row(const Row6& a, const Row6& b, const Row6& c, const float (&w)[9], float (&o)[4]) {
    constexpr int o0 = ROT ? 8 : 0, st = ROT ? -1 : 1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {                                  // explicit FMAs: the file is built with -ffp-contract=off
        float t = w[o0] * a.v[j];
        t = fmaf(w[o0 + st], a.v[j + 1], t); t = fmaf(w[o0 + 2 * st], a.v[j + 2], t);
        t = fmaf(w[o0 + 3 * st], b.v[j], t); t = fmaf(w[o0 + 4 * st], b.v[j + 1], t); t = fmaf(w[o0 + 5 * st], b.v[j + 2], t);
        t = fmaf(w[o0 + 6 * st], c.v[j], t); t = fmaf(w[o0 + 7 * st], c.v[j + 1], t); t = fmaf(w[o0 + 8 * st], c.v[j + 2], t);
        o[j] = t;
    }
}
template <bool FLIP>
__device__ __forceinline__ void stencil16(const Patch& p, const float* __restrict__ w9, float out[4][4]) {
    float w[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) w[i] = FLIP ? w9[8 - i] : w9[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) stencil_row(p.r[i], p.r[i + 1], p.r[i + 2], w, out[i]);
}

// the two gate derivatives of one quad from the depthwise outputs d1, d2 and dg:  av = dg * d2 * gelu'(d1),  cv = dg * gelu(d1)
// (av, cv: four floats each, wherever the caller keeps them)
__device__ __forceinline__ void gate_grad_row(const float4& gq, const float (&d1)[4], const float (&d2)[4], float* av, float* cv) {
    const float gv[4] = {gq.x, gq.y, gq.z, gq.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float ge, gd;
        gelu_and_grad(d1[k], ge, gd);
        av[k] = gv[k] * d2[k] * gd;
        cv[k] = gv[k] * ge;
    }
}

// weight gradient of one channel from one quad of output gradient v and the three input rows around it:
// s[3 di + dj] += sum_k v[k] * row_di[k + dj]   (each sum its own fmaf chain: dj outer, k inner)
__device__ __forceinline__ void wgrad_row(const float* v, const Row6& up, const Row6& mid, const Row6& dn, float* s) {
#pragma unroll
    for (int dj = 0; dj < 3; ++dj)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s[0 + dj] = fmaf(v[k], up.v[k + dj], s[0 + dj]);
            s[3 + dj] = fmaf(v[k], mid.v[k + dj], s[3 + dj]);
            s[6 + dj] = fmaf(v[k], dn.v[k + dj], s[6 + dj]);
        }
}

struct BlockIdx4 { long plane; int y0, x0; };
__device__ __forceinline__ BlockIdx4 block4(long q, int H, int W) {
    const int wq = W >> 2, hq = H >> 2;
    BlockIdx4 b;
    b.plane = q / ((long)hq * wq);
    const int rem = (int)(q - b.plane * (long)hq * wq);
    const int ys = rem / wq;
    b.y0 = ys * 4;
    b.x0 = (rem - ys * wq) * 4;
    return b;
}

// ------------------------------------------------------------------ 4x4-block kernels
// y[plane] = dw3x3(x[plane]; w[plane % C])  (FLIP: correlation with the 180-degree rotated filter
// == the data gradient of the same depthwise conv)
template <bool FLIP, bool NB>
__global__ __launch_bounds__(256) void dwconv_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                     float* __restrict__ y, long nblocks, int C, int H, int W) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= nblocks) return;
    const BlockIdx4 b = block4(q, H, W);
    const int c = (int)(b.plane % C);
    Patch r;
    if (NB) {
        PatchRows rows;
        patch_request(x + b.plane * H * W, H, W, b.y0, b.x0, rows);
        patch_land(rows, H, W, b.y0, b.x0, r);
    } else {
        load_patch(x + b.plane * H * W, H, W, b.y0, b.x0, r);
    }
    float o[4][4];
    stencil16<FLIP>(r, w + c * 9, o);
    float* yp = y + b.plane * H * W + (long)b.y0 * W + b.x0;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(yp + (long)i * W) = make_float4(o[i][0], o[i][1], o[i][2], o[i][3]);
}

// GDFN gate forward: g[b][j] = gelu(dw(p[b][j])) * dw(p[b][j+hid])
template <bool NB>
__global__ __launch_bounds__(256) void gate_fwd_kernel(const float* __restrict__ p, const float* __restrict__ w,
                                                       float* __restrict__ g, long nblocks, int hid, int H, int W) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= nblocks) return;
    const BlockIdx4 b = block4(q, H, W);                 // planes over B*hid
    const long bi = b.plane / hid;
    const int j = (int)(b.plane - bi * hid);
    const long hw = (long)H * W;
    const float* p1 = p + (bi * 2 * hid + j) * hw;
    Patch r;
    float d1[4][4], d2[4][4];
    if (NB) {
        PatchRows q1, q2;                                  // twelve loads in flight before the first is used
        patch_request(p1, H, W, b.y0, b.x0, q1);
        patch_request(p1 + (long)hid * hw, H, W, b.y0, b.x0, q2);
        patch_land(q1, H, W, b.y0, b.x0, r);
        stencil16<false>(r, w + j * 9, d1);
        patch_land(q2, H, W, b.y0, b.x0, r);
        stencil16<false>(r, w + (j + hid) * 9, d2);
    } else {
        load_patch(p1, H, W, b.y0, b.x0, r);
        stencil16<false>(r, w + j * 9, d1);
        load_patch(p1 + (long)hid * hw, H, W, b.y0, b.x0, r);
        stencil16<false>(r, w + (j + hid) * 9, d2);
    }
    float* gp = g + b.plane * hw + (long)b.y0 * W + b.x0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        *reinterpret_cast<float4*>(gp + (long)i * W) = make_float4(gelu_erf(d1[i][0]) * d2[i][0], gelu_erf(d1[i][1]) * d2[i][1],
                                                                   gelu_erf(d1[i][2]) * d2[i][2], gelu_erf(d1[i][3]) * d2[i][3]);
}

// Plane sizes that are not multiples of 4 (whole-image validation at H, W = 8 x odd: trainer.py:179-227 feeds any image
// whose sides divide by 8): one output pixel per thread, bounds-checked taps.  Forward only; training patches take the
// blocked kernels above.
__device__ __forceinline__ float tap9(const float* __restrict__ plane, const float* __restrict__ w9, int H, int W, int y, int x) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int yy = y + i - 1;
        if (yy < 0 || yy >= H) continue;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int xx = x + j - 1;
            if (xx >= 0 && xx < W) s += w9[i * 3 + j] * plane[(long)yy * W + xx];
        }
    }
    return s;
}

__global__ __launch_bounds__(256) void dwconv_any_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         float* __restrict__ y, long total, int C, int H, int W) {
    const long hw = (long)H * W;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long plane = i / hw;
        const int pix = (int)(i - plane * hw), yy = pix / W, xx = pix - yy * W;
        y[i] = tap9(x + plane * hw, w + (plane % C) * 9, H, W, yy, xx);
    }
}

__global__ __launch_bounds__(256) void gate_fwd_any_kernel(const float* __restrict__ p, const float* __restrict__ w,
                                                           float* __restrict__ g, long total, int hid, int H, int W) {
    const long hw = (long)H * W;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long plane = i / hw, bi = plane / hid;
        const int j = (int)(plane - bi * hid);
        const int pix = (int)(i - plane * hw), yy = pix / W, xx = pix - yy * W;
        const float* p1 = p + (bi * 2 * hid + j) * hw;
        const float d1 = tap9(p1, w + j * 9, H, W, yy, xx);
        const float d2 = tap9(p1 + (long)hid * hw, w + (j + hid) * 9, H, W, yy, xx);
        g[i] = gelu_erf(d1) * d2;
    }
}

// ------------------------------------------------------------------ rolling-row strip kernels
// A thread owns a 4-pixel-wide column of RS consecutive rows of one plane and keeps only three input rows (one Row6 each) in
// registers; consecutive lanes own consecutive 4-pixel columns of the same rows, so every load is a run of full row segments.
struct StripIdx { long plane; int y0, x0; bool live; };
__device__ __forceinline__ StripIdx strip_of(long t, long nthreads, int H, int W, int RS) {
    const int wq = W >> 2, ns = (H + RS - 1) / RS;
    StripIdx s;
    s.live = t < nthreads;
    if (!s.live) t = 0;
    s.plane = t / ((long)ns * wq);
    const int rem = (int)(t - s.plane * (long)ns * wq);
    const int st = rem / wq;
    s.y0 = st * RS;
    s.x0 = (rem - st * wq) * 4;
    return s;
}

// Commits a strip thread's NS weight-gradient sums (NS = 9: channel c0; NS = 18: s[0..9) of channel c0, s[9..18) of channel c1) to
// dwg[channel][3][3].  G = lanes that share one plane: 256 (whole workgroup: every thread is live), 64 (one wavefront) or 1 (= gsub
// lanes, a power of two < 64); the sums are combined over those lanes (shuffles, then the four wavefronts through LDS) before one
// atomicAdd per value (level 1: 8 per address).  Every thread of the workgroup calls it.
template <int G, int NS>
__device__ __forceinline__ void strip_commit(float (&s)[NS], float* __restrict__ dwg, int c0, int c1, int gsub, bool live) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gl = G >= 64 ? 64 : gsub;                     // lanes combined by shuffles
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        float v = s[i];
        for (int o = gl >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        s[i] = v;
    }
    if (G == 256) {
        __shared__ float red[4][NS];
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < NS; ++i) red[wave][i] = s[i];
        }
        __syncthreads();
        if (threadIdx.x < NS) {
            const int i = threadIdx.x;
            const bool first = NS == 9 || i < 9;
            atomicAdd(&dwg[(first ? c0 : c1) * 9 + (first ? i : i - 9)], (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]));
        }
    } else if ((lane & (gl - 1)) == 0 && live) {
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            atomicAdd(&dwg[c0 * 9 + i], s[i]);
            if (NS == 18) atomicAdd(&dwg[c1 * 9 + i], s[NS - 9 + i]);
        }
    }
}

// GDFN gate backward (recomputes the depthwise outputs from p):
// dd[b][j] = dg * d2 * gelu'(d1) ; dd[b][j+hid] = dg * gelu(d1)
// G > 0 additionally accumulates the depthwise WEIGHT gradient  dwg[c][3][3] += sum dd[c] (*) p[c]  for c = j, j+hid:
// both operands (the dd values just formed and the three live rows of p) are already in registers, so the separate
// pass that re-read the two 2*hid-channel tensors is gone.  G: lanes that share one plane (strip_commit).
template <int G, int RS>
__global__ __launch_bounds__(256) void gate_bwd_kernel(const float* __restrict__ p, const float* __restrict__ w,
                                                       const float* __restrict__ dg, float* __restrict__ dd,
                                                       float* __restrict__ dwg, long nthreads, int hid, int H, int W,
                                                       int gsub) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const StripIdx b = strip_of(t, nthreads, H, W, RS);
    if (G == 0 && !b.live) return;
    const long bi = b.plane / hid;
    const int j = (int)(b.plane - bi * hid);
    const long hw = (long)H * W;
    const float* p1 = p + (bi * 2 * hid + j) * hw;
    const float* p2 = p1 + (long)hid * hw;
    float* dd1 = dd + (bi * 2 * hid + j) * hw;
    float* dd2 = dd1 + (long)hid * hw;
    const float* gp = dg + b.plane * hw;
    float w1[9], w2[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { w1[i] = w[j * 9 + i]; w2[i] = w[(j + hid) * 9 + i]; }
    float s[18];
#pragma unroll
    for (int i = 0; i < 18; ++i) s[i] = 0.f;
    if (b.live) {
        Row6 a1[3], a2[3];                                     // rows y-1, y, y+1 live in slots (y-1)%3, y%3, (y+1)%3
        load_row6(p1, H, W, b.y0 - 1, b.x0, a1[2]);           // y0 % 3 == 1 would break slot arithmetic: use offsets from y0
        load_row6(p2, H, W, b.y0 - 1, b.x0, a2[2]);
        load_row6(p1, H, W, b.y0, b.x0, a1[0]);
        load_row6(p2, H, W, b.y0, b.x0, a2[0]);
#pragma unroll
        for (int i = 0; i < RS; ++i) {
            const int y = b.y0 + i;
            if (y < H) {                                       // uniform per strip row; H % 4 == 0 but maybe not % RS
                Row6& up1 = a1[(i + 2) % 3]; Row6& mid1 = a1[i % 3]; Row6& dn1 = a1[(i + 1) % 3];
                Row6& up2 = a2[(i + 2) % 3]; Row6& mid2 = a2[i % 3]; Row6& dn2 = a2[(i + 1) % 3];
                load_row6(p1, H, W, y + 1, b.x0, dn1);
                load_row6(p2, H, W, y + 1, b.x0, dn2);
                const float4 gq = *reinterpret_cast<const float4*>(gp + (long)y * W + b.x0);
                float d1[4], d2[4], av[4], cv[4];
                stencil_row(up1, mid1, dn1, w1, d1);
                stencil_row(up2, mid2, dn2, w2, d2);
                gate_grad_row(gq, d1, d2, av, cv);
                *reinterpret_cast<float4*>(dd1 + (long)y * W + b.x0) = make_float4(av[0], av[1], av[2], av[3]);
                *reinterpret_cast<float4*>(dd2 + (long)y * W + b.x0) = make_float4(cv[0], cv[1], cv[2], cv[3]);
                if (G > 0) {
                    wgrad_row(av, up1, mid1, dn1, s);
                    wgrad_row(cv, up2, mid2, dn2, s + 9);
                }
            }
        }
    }
    if (G == 0) return;
    strip_commit<G>(s, dwg, j, j + hid, gsub, b.live);
}

// ---- the whole depthwise part of the GDFN backward in ONE pass: from p (pre-activation, 2*hid channels) and dg
//   dd = gate'(dw3x3(p)) . dg   (never written)   dp = dw3x3(dd; rotated w)   dwg += sum dd (*) p
// A strip thread forms dd for rows y0-1 .. y0+RS (one halo row per strip end is recomputed) and its 4 columns; the two
// halo COLUMNS of dd come from the neighbouring lanes (lane +-1 owns the adjacent 4 pixels of the same rows whenever
// W/4 divides 64, which the dispatcher checks), so the 2*hid-channel dd tensor makes no HBM round trip and the separate
// rotated depthwise convolution (4 ms/step) is gone.
template <int G, int RS>
__global__ __launch_bounds__(256) void gdfn_bwd_kernel(const float* __restrict__ p, const float* __restrict__ w,
                                                       const float* __restrict__ dg, float* __restrict__ dp,
                                                       float* __restrict__ dwg, long nthreads, int hid, int H, int W,
                                                       int gsub) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const StripIdx b = strip_of(t, nthreads, H, W, RS);
    const long bi = b.plane / hid;
    const int j = (int)(b.plane - bi * hid);
    const long hw = (long)H * W;
    const float* p1 = p + (bi * 2 * hid + j) * hw;
    const float* p2 = p1 + (long)hid * hw;
    float* o1 = dp + (bi * 2 * hid + j) * hw;
    float* o2 = o1 + (long)hid * hw;
    const float* gp = dg + b.plane * hw;
    float w1[9], w2[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { w1[i] = w[j * 9 + i]; w2[i] = w[(j + hid) * 9 + i]; }
    const bool has_l = b.x0 > 0, has_r = b.x0 + 4 < W;
    float s[18];
#pragma unroll
    for (int i = 0; i < 18; ++i) s[i] = 0.f;
    Row6 a1[3], a2[3];            // p rows   y0-2+q   in slot q % 3
    Row6 e1[3], e2[3];            // dd rows  y0-1+i   in slot i % 3   (v[0], v[5] = halo columns)
    // Software pipeline: the three 16-byte loads an iteration needs (row r+1 of both p planes, row r of dg) are REQUESTED one
    // iteration ahead, unconditionally, from clamped row indices (out-of-range rows and dead tail threads are zeroed by masks
    // when the data lands).  With the loads inside `if (row exists)` blocks each one was followed by s_waitcnt vmcnt(0) — three
    // serialised memory round trips per row, 54 per strip (ISA of round 3, scripts/README.md "stencil ISA").
    // One iteration and no more: two rows ahead fit the registers of three waves per SIMD only with the filters held in SGPRs, and
    // then measured the same at 128x128 and 3-6 % slower at 64x64 and 32x32; every row of a 4-row strip ahead costs the third
    // wave and 5-9 % (profiles/stencil_issue_diet.txt).
    float4 n1, n2, ng;
    auto request = [&](int yp, bool with_g) {                   // row yp of both p planes, row yp - 1 of dg
        const int ypc = min(max(yp, 0), H - 1);
        n1 = *reinterpret_cast<const float4*>(p1 + (long)ypc * W + b.x0);
        n2 = *reinterpret_cast<const float4*>(p2 + (long)ypc * W + b.x0);
        if (with_g) ng = *reinterpret_cast<const float4*>(gp + (long)min(max(yp - 1, 0), H - 1) * W + b.x0);
    };
    auto land = [&](const float4& q, int y, Row6& r) { land_row6(q, b.live && y >= 0 && y < H, has_l, has_r, r); };
    request(b.y0 - 2, false);
    land(n1, b.y0 - 2, a1[0]); land(n2, b.y0 - 2, a2[0]);
    request(b.y0 - 1, false);
    land(n1, b.y0 - 1, a1[1]); land(n2, b.y0 - 1, a2[1]);
    request(b.y0, true);
#pragma unroll
    for (int i = 0; i < RS + 2; ++i) {
        const int r = b.y0 - 1 + i;                             // dd row formed in this iteration
        Row6& up1 = a1[i % 3]; Row6& mid1 = a1[(i + 1) % 3]; Row6& dn1 = a1[(i + 2) % 3];
        Row6& up2 = a2[i % 3]; Row6& mid2 = a2[(i + 1) % 3]; Row6& dn2 = a2[(i + 2) % 3];
        land(n1, r + 1, dn1);
        land(n2, r + 1, dn2);
        const float4 gq = ng;
        if (i < RS + 1) request(r + 2, true);                   // next iteration's rows fly under this iteration's arithmetic
        Row6& ec1 = e1[i % 3];                                  // the dd rows are formed in place: v[1..4]
        Row6& ec2 = e2[i % 3];
        if (b.live && r >= 0 && r < H) {
            float d1[4], d2[4];
            stencil_row(up1, mid1, dn1, w1, d1);
            stencil_row(up2, mid2, dn2, w2, d2);
            gate_grad_row(gq, d1, d2, ec1.v + 1, ec2.v + 1);
            if (i >= 1 && i <= RS) {                            // rows of this strip: weight gradient (halo rows belong to others)
                wgrad_row(ec1.v + 1, up1, mid1, dn1, s);
                wgrad_row(ec2.v + 1, up2, mid2, dn2, s + 9);
            }
        } else {
#pragma unroll
            for (int k = 1; k < 5; ++k) ec1.v[k] = ec2.v[k] = 0.f;
        }
        // the halo columns of the two dd rows from the neighbouring lanes, outside the condition above: the four shifts issued together
        // (through land_row6, two and two, the kernel is 1.8 % longer: 8599 against 8445 instructions at <256, 16>)
        const float l1 = from_lane_below(ec1.v[4]), r1 = from_lane_above(ec1.v[1]);
        const float l2 = from_lane_below(ec2.v[4]), r2 = from_lane_above(ec2.v[1]);
        ec1.v[0] = has_l ? l1 : 0.f; ec1.v[5] = has_r ? r1 : 0.f;
        ec2.v[0] = has_l ? l2 : 0.f; ec2.v[5] = has_r ? r2 : 0.f;
        if (i >= 2) {
            const int y = r - 1;                                // dp row: dd rows y-1, y, y+1 are in slots (i-2)%3, (i-1)%3, i%3
            if (b.live && y < H) {
                float o[4];
                stencil_row<true>(e1[(i + 1) % 3], e1[(i + 2) % 3], e1[i % 3], w1, o);       // 180-degree rotated filters
                *reinterpret_cast<float4*>(o1 + (long)y * W + b.x0) = make_float4(o[0], o[1], o[2], o[3]);
                stencil_row<true>(e2[(i + 1) % 3], e2[(i + 2) % 3], e2[i % 3], w2, o);
                *reinterpret_cast<float4*>(o2 + (long)y * W + b.x0) = make_float4(o[0], o[1], o[2], o[3]);
            }
        }
    }
    strip_commit<G>(s, dwg, j, j + hid, gsub, b.live);
}

// Depthwise 3x3 backward in one pass: dx = dw3x3(dy; rotated w) and dwg[c][3][3] += sum dy (*) x, on the rolling-row
// strips of gate_bwd_kernel (dy is read once for both results).  G: lanes sharing a plane (strip_commit).
template <int G, int RS, bool NB>
__global__ __launch_bounds__(256) void dwconv_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                         const float* __restrict__ w, float* __restrict__ dx,
                                                         float* __restrict__ dwg, long nthreads, int C, int H, int W,
                                                         int gsub) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const StripIdx b = strip_of(t, nthreads, H, W, RS);
    const int c = (int)(b.plane % C);
    const long hw = (long)H * W;
    const float* gp = dy + b.plane * hw;
    const float* xp = x + b.plane * hw;
    float* op = dx + b.plane * hw;
    float wf[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) wf[i] = w[c * 9 + 8 - i];      // 180-degree rotated filter
    float s[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) s[i] = 0.f;
    const bool has_l = b.x0 > 0, has_r = b.x0 + 4 < W;
    // the lane shifts of NB sit under `if (b.live)` safely only because the last live thread of the grid owns a right-edge column
    // (threads per plane are a multiple of W/4): no live lane takes a halo pixel from a dead one
    if (b.live) {
        Row6 g3[3], x3[3];
        // NB: the NR rows of dy and x (row k = y0 - 1 + k, slot (k + 2) % 3 of g3 / x3) are requested LA rows ahead of their use, from
        // clamped indices, and zeroed by masks when they land (see gdfn_bwd_kernel).  A 4-row strip asks for all six before its first
        // arithmetic: one memory round trip per strip instead of five, 13 % off the launch at 2304 planes of 64x64 for 96 registers
        // instead of 80 (five waves per SIMD, not six); on 8-row strips two or three rows ahead measured the same as one.
        constexpr int NR = RS + 2, LA = (NB && RS == 4) ? NR : 1;
        float4 ng[LA], nx[LA];
        auto request = [&](int k) {
            const int yc = min(max(b.y0 - 1 + k, 0), H - 1);
            ng[k % LA] = *reinterpret_cast<const float4*>(gp + (long)yc * W + b.x0);
            nx[k % LA] = *reinterpret_cast<const float4*>(xp + (long)yc * W + b.x0);
        };
        auto land = [&](int k) {                                // the slot is free again afterwards
            const int y = b.y0 - 1 + k;
            const bool ok = y >= 0 && y < H;
            land_row6(ng[k % LA], ok, has_l, has_r, g3[(k + 2) % 3]);
            land_row6(nx[k % LA], ok, has_l, has_r, x3[(k + 2) % 3]);
            if (k + LA < NR) request(k + LA);
        };
        if (NB) {
#pragma unroll
            for (int k = 0; k < LA; ++k) request(k);
            land(0);
            land(1);
        } else {
            load_row6(gp, H, W, b.y0 - 1, b.x0, g3[2]);
            load_row6(xp, H, W, b.y0 - 1, b.x0, x3[2]);
            load_row6(gp, H, W, b.y0, b.x0, g3[0]);
            load_row6(xp, H, W, b.y0, b.x0, x3[0]);
        }
#pragma unroll
        for (int i = 0; i < RS; ++i) {
            const int y = b.y0 + i;
            if (y < H) {
                Row6& gu = g3[(i + 2) % 3]; Row6& gm = g3[i % 3]; Row6& gd = g3[(i + 1) % 3];
                Row6& xu = x3[(i + 2) % 3]; Row6& xm = x3[i % 3]; Row6& xd = x3[(i + 1) % 3];
                if (NB) {
                    land(i + 2);
                } else {
                    load_row6(gp, H, W, y + 1, b.x0, gd);
                    load_row6(xp, H, W, y + 1, b.x0, xd);
                }
                float o[4];
                stencil_row(gu, gm, gd, wf, o);
                *reinterpret_cast<float4*>(op + (long)y * W + b.x0) = make_float4(o[0], o[1], o[2], o[3]);
                wgrad_row(gm.v + 1, xu, xm, xd, s);
            }
        }
    }
    strip_commit<G>(s, dwg, c, c, gsub, b.live);
}

// The 6x6 patch of dwconv_wgrad_kernel, kept in the form that kernel has always had (one array, the row load written out): with
// Patch / load_row6 its code came out two instructions shorter and measured 4 % slower at 510 x 64 x 64 (37.2 -> 38.7 us,
// profiles/stencil_family_speed.txt), so this one kernel keeps a private copy and its machine code stays as it was.
struct Patch36 { float v[6][6]; };   // rows y0-1..y0+4, columns x0-1..x0+4
__device__ __forceinline__ void load_patch36(const float* __restrict__ plane, int H, int W, int y0, int x0, Patch36& r) {
#pragma unroll
    for (int dy = 0; dy < 6; ++dy) {
        const int yy = y0 + dy - 1;
        if (yy < 0 || yy >= H) {
#pragma unroll
            for (int j = 0; j < 6; ++j) r.v[dy][j] = 0.f;
        } else {
            const float* p = plane + (long)yy * W + x0;
            const float4 c = *reinterpret_cast<const float4*>(p);
            r.v[dy][0] = (x0 > 0) ? p[-1] : 0.f;
            r.v[dy][1] = c.x; r.v[dy][2] = c.y; r.v[dy][3] = c.z; r.v[dy][4] = c.w;
            r.v[dy][5] = (x0 + 4 < W) ? p[4] : 0.f;
        }
    }
}

// dw[c][i][j] += sum_{b,y,x} dy[b][c][y][x] * x[b][c][y+i-1][x+j-1].  TPP threads work on one (b, c) plane
// (4x4 blocks per thread), 256/TPP planes per workgroup so that small planes still fill the wavefronts.
template <int TPP>
__global__ __launch_bounds__(256) void dwconv_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                           float* __restrict__ dw, long planes, int C, int H, int W) {
    __shared__ float red[4];
    constexpr int PPB = 256 / TPP;
    const long plane = (long)blockIdx.x * PPB + threadIdx.x / TPP;
    const int t = threadIdx.x % TPP;
    const bool live = plane < planes;
    const long hw = (long)H * W;
    const float* xp = x + (live ? plane : 0) * hw;
    const float* gp = dy + (live ? plane : 0) * hw;
    const int wq = W >> 2, hq = H >> 2;
    float acc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = 0.f;
    if (live)
        for (int q = t; q < hq * wq; q += TPP) {
            const int ys = q / wq, y0 = ys * 4, x0 = (q - ys * wq) * 4;
            Patch36 r;
            load_patch36(xp, H, W, y0, x0, r);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 gq = *reinterpret_cast<const float4*>(gp + (long)(y0 + i) * W + x0);
                const float gv[4] = {gq.x, gq.y, gq.z, gq.w};
#pragma unroll
                for (int di = 0; di < 3; ++di)
#pragma unroll
                    for (int dj = 0; dj < 3; ++dj)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[di * 3 + dj] += gv[j] * r.v[i + di][j + dj];
            }
        }
    const int c = (int)((live ? plane : 0) % C);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        float v = acc[i];
        if (TPP == 256) {
            v = block_sum<256>(v, red);
        } else {
#pragma unroll
            for (int o = TPP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        }
        if (t == 0 && live) atomicAdd(&dw[c * 9 + i], v);
    }
}

// ------------------------------------------------------------------ host: which instantiation takes a shape
// consecutive lanes own consecutive pixel quads of one row and rows start at lane positions that are multiples of W/4
inline bool nb_lanes_ok(int W) { const int wq = W >> 2; return (W & 3) == 0 && wq >= 1 && wq <= 64 && (64 % wq) == 0; }

// strip height: the tallest of 16 / 8 / 4 rows that still leaves min_threads strip threads (cols = 4-pixel columns of all planes)
inline int strip_rows(long cols, int H, long min_threads) {
    if (cols * cdiv(H, 16) >= min_threads) return 16;
    if (cols * cdiv(H, 8) >= min_threads) return 8;
    return 4;
}
// lanes that share one plane in the fused weight gradient (strip_commit), from the strip threads per plane; G == 0: no grouping
// fits (odd plane sizes), the weight gradient takes a pass of its own
struct LaneGroup { int G, sub; };
inline LaneGroup lane_group(int tpp) {
    if (tpp % 256 == 0) return {256, 64};
    if (tpp % 64 == 0) return {64, 64};
    if (tpp < 64 && (tpp & (tpp - 1)) == 0) return {1, tpp};
    return {0, 0};
}
struct StripPlan {
    int rs;              // rows per strip
    LaneGroup lg;
    long nt;             // strip threads
    dim3 grid;
};
inline StripPlan strip_plan(long planes, int H, int W, long min_threads) {
    StripPlan sp;
    sp.rs = strip_rows(planes * (W >> 2), H, min_threads);
    const int tpp = cdiv(H, sp.rs) * (W >> 2);              // threads (RS-row strips x 4-pixel columns) per plane
    sp.lg = lane_group(tpp);
    sp.nt = planes * tpp;
    sp.grid = dim3(cdiv(sp.nt, 256));
    return sp;
}
// f(G, RS) with both as compile-time constants.  with_strip covers the fused groupings G = 256 / 64 / 1 only, so that a kernel
// without a G = 0 form is not instantiated for it.
template <int V> using Int = std::integral_constant<int, V>;
template <int G, typename F>
void with_rs(int rs, F&& f) {
    if (rs == 16) f(Int<G>{}, Int<16>{});
    else if (rs == 8) f(Int<G>{}, Int<8>{});
    else f(Int<G>{}, Int<4>{});
}
template <typename F>
void with_strip(int G, int rs, F&& f) {
    if (G == 256) with_rs<256>(rs, f);
    else if (G == 64) with_rs<64>(rs, f);
    else with_rs<1>(rs, f);
}

}  // namespace

extern "C" {

int rcot_dwconv3x3(const float* x, const float* w, float* y, int B, int C, int H, int W, int flip, void* stream) {
    if (!x || !w || !y || B <= 0 || C <= 0 || H <= 0 || W <= 0) return RCOT_EINVAL;
    if ((W & 3) || (H & 3)) {
        if (flip) return RCOT_EINVAL;                      // the data gradient is only needed at training patch sizes
        const long total = (long)B * C * H * W;
        note_kernel("dwconv_any_kernel");
        RCOT_LAUNCH(dwconv_any_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, w, y, total, C, H, W);
        RCOT_LAUNCH_CHECK();
        return RCOT_OK;
    }
    if (!al16(x) || !al16(y)) return RCOT_EINVAL;          // the quad kernels load and store float4
    const long nq = (long)B * C * (H >> 2) * (W >> 2);
    const bool nb = nb_lanes_ok(W);
#define RCOT_DW(F, NB_) do { note_kernel("dwconv_kernel<%s, %s>", tf(F), tf(NB_)); RCOT_LAUNCH((dwconv_kernel<F, NB_>), dim3(cdiv(nq, 256)), dim3(256), 0, (hipStream_t)stream, x, w, y, nq, C, H, W); } while (0)
    if (flip) { if (nb) RCOT_DW(true, true); else RCOT_DW(true, false); }
    else { if (nb) RCOT_DW(false, true); else RCOT_DW(false, false); }
#undef RCOT_DW
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

int rcot_gdfn_gate_fwd(const float* p, const float* w, float* g, int B, int hid, int H, int W, void* stream) {
    if (!p || !w || !g || B <= 0 || hid <= 0 || H <= 0 || W <= 0) return RCOT_EINVAL;
    if ((W & 3) || (H & 3)) {
        const long total = (long)B * hid * H * W;
        note_kernel("gate_fwd_any_kernel");
        RCOT_LAUNCH(gate_fwd_any_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, p, w, g, total, hid, H, W);
        RCOT_LAUNCH_CHECK();
        return RCOT_OK;
    }
    if (!al16(p) || !al16(g)) return RCOT_EINVAL;
    const long nq = (long)B * hid * (H >> 2) * (W >> 2);
    // the neighbour-lane form of the patch loads (all twelve rows of both planes requested before the first lane shift; with the
    // loads inside per-row `if` blocks it measured SLOWER than the scalar-halo form, 33.8 vs 30.8 us)
    const bool nb = nb_lanes_ok(W);
    note_kernel("gate_fwd_kernel<%s>", tf(nb));
    if (nb)
        RCOT_LAUNCH(gate_fwd_kernel<true>, dim3(cdiv(nq, 256)), dim3(256), 0, (hipStream_t)stream, p, w, g, nq, hid, H, W);
    else
        RCOT_LAUNCH(gate_fwd_kernel<false>, dim3(cdiv(nq, 256)), dim3(256), 0, (hipStream_t)stream, p, w, g, nq, hid, H, W);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

int rcot_gdfn_gate_bwd(const float* p, const float* w, const float* dg, float* dd, float* dwg, int B, int hid, int H,
                       int W, void* stream) {
    if (!p || !w || !dg || !dd || B <= 0 || hid <= 0 || H <= 0 || W <= 0 || (W & 3) || (H & 3)) return RCOT_EINVAL;
    if (!al16(p) || !al16(dg) || !al16(dd)) return RCOT_EINVAL;
    // strips that still leave >= 400k threads (about 6 wavefronts per SIMD); without dwg, or when no lane grouping fits: G = 0
    const StripPlan sp = strip_plan((long)B * hid, H, W, 400000);
    const LaneGroup lg = dwg ? sp.lg : LaneGroup{0, 0};
    auto launch = [&](auto g, auto rs) {
        RCOT_LAUNCH((gate_bwd_kernel<decltype(g)::value, decltype(rs)::value>), sp.grid, dim3(256), 0, (hipStream_t)stream, p, w, dg,
                    dd, dwg, sp.nt, hid, H, W, lg.sub);
    };
    if (lg.G) with_strip(lg.G, sp.rs, launch);
    else with_rs<0>(sp.rs, launch);
    RCOT_LAUNCH_CHECK();
    if (dwg && !lg.G) return rcot_dwconv3x3_wgrad(dd, p, dwg, B, 2 * hid, H, W, stream);   // odd plane sizes: separate pass
    return RCOT_OK;
}

int rcot_dwconv3x3_wgrad(const float* dy, const float* x, float* dw, int B, int C, int H, int W, void* stream) {
    if (!dy || !x || !dw || B <= 0 || C <= 0 || H <= 0 || W <= 0 || (W & 3) || (H & 3) || B > 65535) return RCOT_EINVAL;
    if (!al16(dy) || !al16(x)) return RCOT_EINVAL;
    const long planes = (long)B * C;
    const int nb4 = (H >> 2) * (W >> 2);
    if (nb4 <= 16)
        RCOT_LAUNCH(dwconv_wgrad_kernel<16>, dim3(cdiv(planes, 16)), dim3(256), 0, (hipStream_t)stream, dy, x, dw, planes, C, H, W);
    else if (nb4 <= 64)
        RCOT_LAUNCH(dwconv_wgrad_kernel<64>, dim3(cdiv(planes, 4)), dim3(256), 0, (hipStream_t)stream, dy, x, dw, planes, C, H, W);
    else
        RCOT_LAUNCH(dwconv_wgrad_kernel<256>, dim3(planes), dim3(256), 0, (hipStream_t)stream, dy, x, dw, planes, C, H, W);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

int rcot_gdfn_bwd(const float* p, const float* w, const float* dg, float* dp, float* dwg, float* dd_scratch, int B, int hid,
                  int H, int W, void* stream) {
    if (!p || !w || !dg || !dp || !dwg || B <= 0 || hid <= 0 || H <= 0 || W <= 0 || (W & 3) || (H & 3)) return RCOT_EINVAL;
    if (!al16(p) || !al16(dg) || !al16(dp) || !al16(dd_scratch)) return RCOT_EINVAL;
    // strip height: halo rows cost (RS+2)/RS, so prefer tall strips while >= 200k threads remain
    const StripPlan sp = strip_plan((long)B * hid, H, W, 200000);
    if (nb_lanes_ok(W) && sp.lg.G) {                          // the neighbour-lane exchange needs whole row segments per wavefront
        with_strip(sp.lg.G, sp.rs, [&](auto g, auto rs) {
            constexpr int G = decltype(g)::value, RS = decltype(rs)::value;
            note_kernel("gdfn_bwd_kernel<%d, %d>", G, RS);
            RCOT_LAUNCH((gdfn_bwd_kernel<G, RS>), sp.grid, dim3(256), 0, (hipStream_t)stream, p, w, dg, dp, dwg, sp.nt, hid, H, W,
                        sp.lg.sub);
        });
        RCOT_LAUNCH_CHECK();
        return RCOT_OK;
    }
    if (!dd_scratch) return RCOT_EWORKSPACE;                  // other geometries: the two-kernel route through dd
    const int rc = rcot_gdfn_gate_bwd(p, w, dg, dd_scratch, dwg, B, hid, H, W, stream);
    if (rc != RCOT_OK) return rc;
    return rcot_dwconv3x3(dd_scratch, w, dp, B, 2 * hid, H, W, 1, stream);
}

int rcot_dwconv3x3_bwd(const float* dy, const float* x, const float* w, float* dx, float* dwg, int B, int C, int H, int W,
                       void* stream) {
    if (!dy || !x || !w || !dx || !dwg || B <= 0 || C <= 0 || H <= 0 || W <= 0 || (W & 3) || (H & 3) || B > 65535)
        return RCOT_EINVAL;
    if (!al16(dy) || !al16(x) || !al16(dx)) return RCOT_EINVAL;
    const StripPlan sp = strip_plan((long)B * C, H, W, 400000);
    if (!sp.lg.G) {                                           // odd plane sizes: the two separate passes
        const int rc = rcot_dwconv3x3(dy, w, dx, B, C, H, W, 1, stream);
        if (rc != RCOT_OK) return rc;
        return rcot_dwconv3x3_wgrad(dy, x, dwg, B, C, H, W, stream);
    }
    const bool nb = nb_lanes_ok(W);
    with_strip(sp.lg.G, sp.rs, [&](auto g, auto rs) {
        constexpr int G = decltype(g)::value, RS = decltype(rs)::value;
        if (nb) RCOT_LAUNCH((dwconv_bwd_kernel<G, RS, true>), sp.grid, dim3(256), 0, (hipStream_t)stream, dy, x, w, dx, dwg, sp.nt, C, H, W, sp.lg.sub);
        else RCOT_LAUNCH((dwconv_bwd_kernel<G, RS, false>), sp.grid, dim3(256), 0, (hipStream_t)stream, dy, x, w, dx, dwg, sp.nt, C, H, W, sp.lg.sub);
    });
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

}  // extern "C"
