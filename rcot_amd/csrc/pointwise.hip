// HBM-bound kernels of the RCOT hot path: per-pixel LayerNorm statistics / backward, depthwise
// 3x3 stencils (plain, GELU-gated, transposed, weight gradient), row reductions and the small
// elementwise pieces of the minimax step.  NCHW fp32; pixels are the fastest axis so a wavefront
// always touches 64 consecutive pixels of one channel plane (coalesced 256 B segments).
#include <cstdlib>
#include "common.h"
#include "../../include/rcot_hip.h"

using namespace rcot;

namespace {

// ------------------------------------------------------------------ LayerNorm over C per pixel
// Tile = 64 pixels x all channels per workgroup: 16 lanes x float4 cover the pixels (256 B contiguous per
// channel row), 16 thread-rows stride over the channels, so every channel plane row is one coalesced segment
// and 16 loads per pixel column are in flight.  Cross-row reduction through LDS.
constexpr int LN_TX = 16, LN_TY = 16, LN_PIX = LN_TX * 4;

__device__ __forceinline__ float4 f4_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// sums over the TY thread-rows of a (TY x TX)-thread block; result valid in every thread
template <int TX>
__device__ __forceinline__ float4 reduce_rows(float4 v, float4* red, int tx, int ty) {
    constexpr int TY = 256 / TX;
    __syncthreads();
    red[ty * TX + tx] = v;
    __syncthreads();
    float4 t = red[tx];
#pragma unroll
    for (int i = 1; i < TY; ++i) t = f4_add(t, red[i * TX + tx]);
    return t;
}

__global__ __launch_bounds__(256) void ln_stats_kernel(const float* __restrict__ x, float* __restrict__ mu,
                                                       float* __restrict__ rs, int C, int N) {
    __shared__ float4 red[256];
    const int tx = threadIdx.x & (LN_TX - 1), ty = threadIdx.x >> 4;
    const int n = blockIdx.x * LN_PIX + tx * 4;
    const int b = blockIdx.y;
    const bool ok = n < N;                         // N % 4 == 0
    const float* p = x + (long)b * C * N + (ok ? n : 0);
    // shifted sums (shift = channel 0) keep E[d^2] - E[d]^2 well conditioned
    const float4 sh = ok ? *reinterpret_cast<const float4*>(p) : make_float4(0, 0, 0, 0);
    float4 s = make_float4(0, 0, 0, 0), ss = make_float4(0, 0, 0, 0);
    if (ok) {
#pragma unroll 4
        for (int c = ty; c < C; c += LN_TY) {
            const float4 v = *reinterpret_cast<const float4*>(p + (long)c * N);
            const float dx_ = v.x - sh.x, dy_ = v.y - sh.y, dz_ = v.z - sh.z, dw_ = v.w - sh.w;
            s.x += dx_; s.y += dy_; s.z += dz_; s.w += dw_;
            ss.x += dx_ * dx_; ss.y += dy_ * dy_; ss.z += dz_ * dz_; ss.w += dw_ * dw_;
        }
    }
    s = reduce_rows<LN_TX>(s, red, tx, ty);
    ss = reduce_rows<LN_TX>(ss, red, tx, ty);
    if (ty == 0 && ok) {
        const float inv = 1.0f / (float)C;
        float4 m, r;
#define RCOT_LN_FIN(q)                                              \
    {                                                               \
        const float e = s.q * inv;                                  \
        const float var = fmaxf(ss.q * inv - e * e, 0.f);           \
        m.q = sh.q + e;                                             \
        r.q = 1.0f / sqrtf(var + 1e-5f);                            \
    }
        RCOT_LN_FIN(x) RCOT_LN_FIN(y) RCOT_LN_FIN(z) RCOT_LN_FIN(w)
#undef RCOT_LN_FIN
        *reinterpret_cast<float4*>(mu + (long)b * N + n) = m;
        *reinterpret_cast<float4*>(rs + (long)b * N + n) = r;
    }
}

// dx = dres + r*(gh - mean_C gh - xh*mean_C(gh*xh)), gh = g*w ; dw += sum g*xh ; db += sum g
// Thread block = TY channel-rows x TX pixel-quads (TX*4 pixels of one image); a block walks pixel tiles
// blockIdx.x, +gridDim.x, ... and keeps its share of the dw/db sums in LDS, then writes ONE partial row
// part[block][2C]; ln_param_reduce_kernel adds the rows up in a fixed order (deterministic, and no same-address
// atomics: those serialise at ~30 ns each, which used to bound this kernel at every level).
// NC > 0: C == TY*NC and every thread keeps its NC channels of g and x in registers between the reduction and
// the update (one HBM read of g and x instead of two); NC == 0: generic C, second pass re-reads (L2).
template <int NC, int TX>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                     const float* __restrict__ mu, const float* __restrict__ rs,
                                                     const float* __restrict__ w, const float* __restrict__ dres,
                                                     float* __restrict__ dx, float* __restrict__ part, int C, int N) {
    constexpr int TY = 256 / TX, PIX = TX * 4;
    __shared__ float4 red[256];
    __shared__ float sdw[512], sdb[512];
    const int tid = threadIdx.x;
    const int tx = tid % TX, ty = tid / TX;
    const int b = blockIdx.y;
    for (int c = tid; c < C; c += 256) { sdw[c] = 0.f; sdb[c] = 0.f; }   // channel c is only ever touched by thread (c % TY, 0)
    __syncthreads();
    const int ntiles = (N + PIX - 1) / PIX;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int n = tile * PIX + tx * 4;
        const bool ok = n < N;
        const long base = (long)b * C * N + (ok ? n : 0);
        const float4 m = ok ? *reinterpret_cast<const float4*>(mu + (long)b * N + n) : make_float4(0, 0, 0, 0);
        const float4 r = ok ? *reinterpret_cast<const float4*>(rs + (long)b * N + n) : make_float4(0, 0, 0, 0);
        float4 s1 = make_float4(0, 0, 0, 0), s2 = make_float4(0, 0, 0, 0);
        constexpr int NR = NC > 0 ? NC : 1;
        float4 gk[NR], xk[NR];                                   // xk holds xhat
        const int niter = NC > 0 ? NC : (C - ty + TY - 1) / TY;
#pragma unroll
        for (int it = 0; it < NR; ++it) { gk[it] = make_float4(0, 0, 0, 0); xk[it] = gk[it]; }
        if (NC > 0 && ok) {                                       // issue every load first
#pragma unroll
            for (int it = 0; it < NR; ++it) {
                const long i = base + (long)(ty + it * TY) * N;
                gk[it] = *reinterpret_cast<const float4*>(g + i);
                xk[it] = *reinterpret_cast<const float4*>(x + i);
            }
        }
        for (int it = 0; it < niter; ++it) {
            const int c = ty + it * TY;
            float4 gv = make_float4(0, 0, 0, 0), xh = gv;
            if (NC > 0) {
#pragma unroll
                for (int q = 0; q < NR; ++q)
                    if (q == it) { gv = gk[q]; xh = xk[q]; }
                xh = make_float4((xh.x - m.x) * r.x, (xh.y - m.y) * r.y, (xh.z - m.z) * r.z, (xh.w - m.w) * r.w);
#pragma unroll
                for (int q = 0; q < NR; ++q)
                    if (q == it) xk[q] = xh;
            } else if (ok) {
                gv = *reinterpret_cast<const float4*>(g + base + (long)c * N);
                const float4 xv = *reinterpret_cast<const float4*>(x + base + (long)c * N);
                xh = make_float4((xv.x - m.x) * r.x, (xv.y - m.y) * r.y, (xv.z - m.z) * r.z, (xv.w - m.w) * r.w);
            }
            const float wc = w[c];
            s1.x += gv.x * wc; s1.y += gv.y * wc; s1.z += gv.z * wc; s1.w += gv.w * wc;
            s2.x += gv.x * wc * xh.x; s2.y += gv.y * wc * xh.y; s2.z += gv.z * wc * xh.z; s2.w += gv.w * wc * xh.w;
            float a = gv.x * xh.x + gv.y * xh.y + gv.z * xh.z + gv.w * xh.w;
            float bb = gv.x + gv.y + gv.z + gv.w;
#pragma unroll
            for (int o = TX / 2; o > 0; o >>= 1) {           // the TX lanes of one thread-row are contiguous in the wave
                a += __shfl_xor(a, o, 64);
                bb += __shfl_xor(bb, o, 64);
            }
            if (tx == 0) {                                   // one owner per channel in this block
                sdw[c] += a;
                sdb[c] += bb;
            }
        }
        s1 = reduce_rows<TX>(s1, red, tx, ty);
        s2 = reduce_rows<TX>(s2, red, tx, ty);
        if (ok) {
            const float inv = 1.0f / (float)C;
            s1.x *= inv; s1.y *= inv; s1.z *= inv; s1.w *= inv;
            s2.x *= inv; s2.y *= inv; s2.z *= inv; s2.w *= inv;
#pragma unroll
            for (int it = 0; it < NR; ++it) {
                if (NC == 0) break;
                const int c = ty + it * TY;
                const long i = base + (long)c * N;
                const float wc = w[c];
                float4 v;
                v.x = r.x * (gk[it].x * wc - s1.x - xk[it].x * s2.x);
                v.y = r.y * (gk[it].y * wc - s1.y - xk[it].y * s2.y);
                v.z = r.z * (gk[it].z * wc - s1.z - xk[it].z * s2.z);
                v.w = r.w * (gk[it].w * wc - s1.w - xk[it].w * s2.w);
                if (dres) v = f4_add(v, *reinterpret_cast<const float4*>(dres + i));
                *reinterpret_cast<float4*>(dx + i) = v;
            }
            if (NC == 0)
                for (int c = ty; c < C; c += TY) {
                    const long i = base + (long)c * N;
                    const float4 gv = *reinterpret_cast<const float4*>(g + i);
                    const float4 xv = *reinterpret_cast<const float4*>(x + i);
                    const float wc = w[c];
                    float4 v;
                    v.x = r.x * (gv.x * wc - s1.x - (xv.x - m.x) * r.x * s2.x);
                    v.y = r.y * (gv.y * wc - s1.y - (xv.y - m.y) * r.y * s2.y);
                    v.z = r.z * (gv.z * wc - s1.z - (xv.z - m.z) * r.z * s2.z);
                    v.w = r.w * (gv.w * wc - s1.w - (xv.w - m.w) * r.w * s2.w);
                    if (dres) v = f4_add(v, *reinterpret_cast<const float4*>(dres + i));
                    *reinterpret_cast<float4*>(dx + i) = v;
                }
        }
    }
    __syncthreads();
    float* row = part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * (2 * C);
    for (int c = tid; c < C; c += 256) {
        row[c] = sdw[c];
        row[C + c] = sdb[c];
    }
}

// dw[c] += sum_r part[r][c], db[c] += sum_r part[r][C + c]: 32 columns x 32 row-lanes per workgroup (1024 threads),
// rows in a fixed order (deterministic)
__global__ __launch_bounds__(1024) void ln_param_reduce_kernel(const float* __restrict__ part, int rows, int C,
                                                               float* __restrict__ dw, float* __restrict__ db) {
    __shared__ float red[32][33];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int col = blockIdx.x * 32 + cl, C2 = 2 * C;
    float s0 = 0.f, s1 = 0.f;
    if (col < C2) {
        const float* p = part + col;
        int r = rl;
        for (; r + 32 < rows; r += 64) {
            s0 += p[(long)r * C2];
            s1 += p[(long)(r + 32) * C2];
        }
        if (r < rows) s0 += p[(long)r * C2];
    }
    red[rl][cl] = s0 + s1;
    __syncthreads();
    if (rl == 0 && col < C2) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 32; ++i) s += red[i][cl];
        if (col < C) dw[col] += s;
        else db[col - C] += s;
    }
}

// Every parameter-gradient reduction that closes the backward of one transformer block, in ONE launch (1024 threads per
// workgroup): the two LayerNorms' partial rows (part1 -> gw1/gb1, part2 -> gw2/gb2, as ln_param_reduce_kernel), the
// per-image dW_o (-> gWo) and the per-image temperature partials (-> gtemp).  Fixed summation order: deterministic.
// Up to four split-K slab sets of the block's 1x1 weight gradients (rcot_conv1x1_wgrad_slabs) ride along: dst += sum_s slab[s]
// (256 outputs per workgroup, the slabs in four interleaved groups, fixed order), which replaces their reduce launches.
struct SlabSets {
    const float* ws[4];
    float* dst[4];
    int S[4], M[4], N[4], ldws[4];
    int per[4];                       // outputs per workgroup of the set's chunks (4096: S <= 8; 1024 / 256: S > 8, by the size of the gradient)
    long ldd[4];
    int chunk0[5];                    // first workgroup (after the parameter reductions) of every set; chunk0[n] = total
    int n;
};

__global__ __launch_bounds__(1024) void block_param_reduce_kernel(const float* __restrict__ part1, const float* __restrict__ part2,
                                                                  int rows, int C, float* __restrict__ gw1, float* __restrict__ gb1,
                                                                  float* __restrict__ gw2, float* __restrict__ gb2,
                                                                  const float* __restrict__ dWo_part, float* __restrict__ gWo,
                                                                  const float* __restrict__ dtemp_part, float* __restrict__ gtemp,
                                                                  int B, int heads, int nw, SlabSets ss) {
    __shared__ float red[32][33];
    const int nl = (2 * C + 31) / 32;
    const int blk = blockIdx.x;
    if (blk >= 2 * nl + nw) {
        // ---- slab set d, ss.per[d] outputs per workgroup.  S > 8: thread = (one or four outputs, slab group q); S <= 8:
        // outputs [4096 c, 4096 c + 4096), four outputs per thread with all their slabs in flight
        const int cb = blk - 2 * nl - nw;
        int d = 0;
        while (d + 1 < ss.n && cb >= ss.chunk0[d + 1]) ++d;
        const int c = cb - ss.chunk0[d];
        const long mn = (long)ss.M[d] * ss.N[d];
        const long slab = (long)ss.M[d] * ss.ldws[d];
        if (ss.S[d] <= 8) {
            // four outputs per thread (1024 apart: every load of a wavefront is one contiguous 256-byte piece), all 4 x S slab reads and
            // the four old values in flight before the first add; 32-bit index arithmetic (a weight gradient is far below 2^31
            // elements; the 64-bit division of the one-output form was most of its instructions), loads from clamped indices
            // instead of under branches.  Same sum, same order per output as before: bit-identical results (round 6: the launch
            // that closes a 16 x 16 block 43 -> 2x us; it sits on the main stream behind a join in exact fp32)
            const unsigned Nn = (unsigned)ss.N[d], mnu = (unsigned)mn, S = (unsigned)ss.S[d];
            const unsigned ldw = (unsigned)ss.ldws[d];
            const float* wsb = ss.ws[d];
            float* dstb = ss.dst[d];
            float v[4][8], old[4];
            long doff[4];
            bool ok[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned idx = (unsigned)c * 4096u + 1024u * j + threadIdx.x;
                ok[j] = idx < mnu;
                const unsigned ic = ok[j] ? idx : mnu - 1;
                const unsigned m = ic / Nn, n = ic - m * Nn;
                const float* w = wsb + (size_t)m * ldw + n;
                doff[j] = (long)m * ss.ldd[d] + n;
#pragma unroll
                for (unsigned u = 0; u < 8; ++u) {
                    const unsigned uc = u < S ? u : S - 1;
                    v[j][u] = w[(long)uc * slab];
                }
                old[j] = dstb[doff[j]];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (unsigned u = 0; u < 8; ++u) v[j][u] = u < S ? v[j][u] : 0.f;
                const float sum = ((v[j][0] + v[j][1]) + (v[j][2] + v[j][3])) + ((v[j][4] + v[j][5]) + (v[j][6] + v[j][7]));
                if (ok[j]) dstb[doff[j]] = old[j] + sum;
            }
            return;
        }
        if (ss.per[d] == 256) {
            // few outputs (the weight gradients of the 128 x 128 and 64 x 64 planes: 25 000 - 100 000 elements, up to 256 slabs each): one
            // output per thread keeps 100 - 400 workgroups on the chip (four outputs per thread there: 33 -> 113 us, profiles/r06_block_reduce.txt)
            const int o = threadIdx.x & 255, q = threadIdx.x >> 8;
            const long idx = (long)c * 256 + o;
            float* part = &red[0][0];                                        // [4][256] inside the 32 x 33 scratch
            float a = 0.f;
            int m = 0, n = 0;
            if (idx < mn) {
                m = (int)(idx / ss.N[d]);
                n = (int)(idx - (long)m * ss.N[d]);
                const float* w = ss.ws[d] + (long)m * ss.ldws[d] + n;
                float acc8[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) acc8[u] = 0.f;
                int s = q;
                for (; s + 28 < ss.S[d]; s += 32) {
#pragma unroll
                    for (int u = 0; u < 8; ++u) acc8[u] += w[(long)(s + 4 * u) * slab];
                }
                for (; s < ss.S[d]; s += 4) acc8[0] += w[(long)s * slab];
                a = ((acc8[0] + acc8[1]) + (acc8[2] + acc8[3])) + ((acc8[4] + acc8[5]) + (acc8[6] + acc8[7]));
            }
            part[q * 256 + o] = a;
            __syncthreads();
            if (q == 0 && idx < mn)
                ss.dst[d][(long)m * ss.ldd[d] + n] += (part[o] + part[256 + o]) + (part[512 + o] + part[768 + o]);
            return;
        }
        // S > 8: outputs [1024 c, 1024 c + 1024): thread (o, q) takes slab group q (slabs q, q + 4, ...) of the FOUR outputs o + 256 j —
        // 32-bit index arithmetic, every load of a wavefront one contiguous 256-byte piece, up to 32 loads in flight per thread
        // (round 6; one output per thread before: 6 500 workgroups for the three weight gradients of a 16 x 16 block).  Per output the
        // sum and its order are unchanged (eight interleaved chains per group, then the four groups): bit-identical results.
        const int o = threadIdx.x & 255, q = threadIdx.x >> 8;
        const unsigned Nn = (unsigned)ss.N[d], mnu = (unsigned)mn, ldw = (unsigned)ss.ldws[d];
        const int S = ss.S[d];
        float a[4];
        long doff[4];
        bool ok[4];
        const float* w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned idx = (unsigned)c * 1024u + 256u * j + o;
            ok[j] = idx < mnu;
            const unsigned ic = ok[j] ? idx : mnu - 1;
            const unsigned m = ic / Nn, n = ic - m * Nn;
            w[j] = ss.ws[d] + (size_t)m * ldw + n;
            doff[j] = (long)m * ss.ldd[d] + n;
        }
        float acc8[4][8];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int u = 0; u < 8; ++u) acc8[j][u] = 0.f;
        int sl = q;
        for (; sl + 28 < S; sl += 32) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int u = 0; u < 8; ++u) acc8[j][u] += w[j][(long)(sl + 4 * u) * slab];
        }
        for (; sl < S; sl += 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc8[j][0] += w[j][(long)sl * slab];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            a[j] = ((acc8[j][0] + acc8[j][1]) + (acc8[j][2] + acc8[j][3])) + ((acc8[j][4] + acc8[j][5]) + (acc8[j][6] + acc8[j][7]));
        __shared__ float part4[4][1024];
#pragma unroll
        for (int j = 0; j < 4; ++j) part4[q][256 * j + o] = a[j];
        __syncthreads();
        {   // thread t finishes output t of the chunk
            const int t = threadIdx.x;
            const unsigned idx = (unsigned)c * 1024u + t;
            if (idx < mnu) {
                const unsigned m = idx / Nn, n = idx - m * Nn;
                ss.dst[d][(long)m * ss.ldd[d] + n] += (part4[0][t] + part4[1][t]) + (part4[2][t] + part4[3][t]);
            }
        }
        (void)doff; (void)ok;
        return;
    }
    if (blk < 2 * nl) {
        const float* part = blk < nl ? part1 : part2;
        float* dw = blk < nl ? gw1 : gw2;
        float* db = blk < nl ? gb1 : gb2;
        const int cb = blk < nl ? blk : blk - nl;
        const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
        const int col = cb * 32 + cl, C2 = 2 * C;
        float a8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) a8[u] = 0.f;
        if (col < C2) {
            // eight rows in flight per trip (two per trip left 16 dependent round trips for the 1024 partial rows of a level)
            const float* p = part + col;
            int r = rl;
            for (; r + 224 < rows; r += 256) {
#pragma unroll
                for (int u = 0; u < 8; ++u) a8[u] += p[(long)(r + 32 * u) * C2];
            }
            for (; r < rows; r += 32) a8[0] += p[(long)r * C2];
        }
        red[rl][cl] = ((a8[0] + a8[1]) + (a8[2] + a8[3])) + ((a8[4] + a8[5]) + (a8[6] + a8[7]));
        __syncthreads();
        if (rl == 0 && col < C2) {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 32; ++i) s += red[i][cl];
            if (col < C) dw[col] += s;
            else db[col - C] += s;
        }
        return;
    }
    const long n = (long)C * C;
    const long i = (long)(blk - 2 * nl) * 1024 + threadIdx.x;
    if (i < n) {
        float s = 0.f;
        int b = 0;
        for (; b + 8 <= B; b += 8) {                             // eight images in flight (fixed order)
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = dWo_part[(long)(b + u) * n + i];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; b < B; ++b) s += dWo_part[(long)b * n + i];
        gWo[i] += s;
    }
    if (blk == 2 * nl && threadIdx.x < heads) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += dtemp_part[(long)b * heads + threadIdx.x];
        gtemp[threadIdx.x] += s;
    }
}

// ------------------------------------------------------------------ depthwise 3x3 (pad 1)
// Register blocking: one thread owns a 4x4 output block and reads its 6x6 input patch once (6 float4 rows + halo
// scalars): 2.25 loads per output instead of 4.5 for a 1x4 strip; a wavefront covers 64 consecutive quads of a
// plane row-block, i.e. 256-byte coalesced row segments.  H % 4 == 0, W % 4 == 0.
// Halo pixels from the NEIGHBOURING LANES: when the NEIGHBOURING LANES own the adjacent pixel quads of the same row (W/4 divides 64: rows start at lane
// boundaries of that size): the two halo pixels come from lanes -1 / +1 by DPP wave shifts (VALU speed) instead of two more
// scalar loads per row, and nothing is branched on (every lane executes the shifts; out-of-range rows load as zeros).
__device__ __forceinline__ float from_lane_below(float v) {      // lane i <- lane i-1   (v_mov_b32_dpp wave_shr:1)
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float from_lane_above(float v) {      // lane i <- lane i+1   (wave_shl:1)
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, false));
}
struct Patch { float v[6][6]; };   // rows y0-1..y0+4, columns x0-1..x0+4

__device__ __forceinline__ void load_patch(const float* __restrict__ plane, int H, int W, int y0, int x0, Patch& r) {
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

// the same patch with the two halo columns taken from lanes -1 / +1 (consecutive lanes = consecutive quads of one row block,
// W/4 divides 64): 6 loads per patch instead of 18
// Split in two so that a kernel can REQUEST all the rows it needs (unconditional 16-byte loads from clamped row indices) before it
// touches any of them: a load inside `if (row exists)` followed by the lane shift costs one full memory round trip per row.
struct PatchRows { float4 c[6]; };
__device__ __forceinline__ void patch_request(const float* __restrict__ plane, int H, int W, int y0, int x0, PatchRows& q) {
#pragma unroll
    for (int dy = 0; dy < 6; ++dy) {
        const int yy = min(max(y0 + dy - 1, 0), H - 1);
        q.c[dy] = *reinterpret_cast<const float4*>(plane + (long)yy * W + x0);
    }
}
__device__ __forceinline__ void patch_land(const PatchRows& q, int H, int W, int y0, int x0, Patch& r) {
    const bool has_l = x0 > 0, has_r = x0 + 4 < W;
#pragma unroll
    for (int dy = 0; dy < 6; ++dy) {
        const int yy = y0 + dy - 1;
        const bool ok = yy >= 0 && yy < H;
        const float4 c = ok ? q.c[dy] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float l = from_lane_below(c.w), rr = from_lane_above(c.x);
        r.v[dy][0] = has_l ? l : 0.f;
        r.v[dy][1] = c.x; r.v[dy][2] = c.y; r.v[dy][3] = c.z; r.v[dy][4] = c.w;
        r.v[dy][5] = has_r ? rr : 0.f;
    }
}
__device__ __forceinline__ void load_patch_nb(const float* __restrict__ plane, int H, int W, int y0, int x0, Patch& r) {
    PatchRows q;
    patch_request(plane, H, W, y0, x0, q);
    patch_land(q, H, W, y0, x0, r);
}

template <bool FLIP>
__device__ __forceinline__ void stencil16(const Patch& r, const float* __restrict__ w9, float out[4][4]) {
    float w[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) w[i] = FLIP ? w9[8 - i] : w9[i];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float a = w[0] * r.v[i][j];                      // explicit FMAs (the file is built with -ffp-contract=off)
#pragma unroll
            for (int q = 1; q < 9; ++q) a = fmaf(w[q], r.v[i + q / 3][j + q % 3], a);
            out[i][j] = a;
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
    if (NB) load_patch_nb(x + b.plane * H * W, H, W, b.y0, b.x0, r);
    else load_patch(x + b.plane * H * W, H, W, b.y0, b.x0, r);
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

// ---- rolling-row strips.  A thread owns a 4-pixel-wide column of RS consecutive rows of one plane and keeps only
// three input rows (6 floats each: the float4 plus one halo pixel per side) in registers; consecutive lanes own
// consecutive 4-pixel columns of the same rows, so every load is a run of full row segments.
struct Row6 { float v[6]; };
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
// (the neighbour-lane form of load_row6: halo pixels by DPP wave shifts, see from_lane_below above load_patch)
__device__ __forceinline__ void load_row6_nb(const float* __restrict__ plane, int H, int W, int y, int x0, bool has_l, bool has_r,
                                             bool live, Row6& r) {
    const bool ok = live && y >= 0 && y < H;
    const float* q = plane + (long)(ok ? y : 0) * W + x0;
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) c = *reinterpret_cast<const float4*>(q);
    const float l = from_lane_below(c.w), rr = from_lane_above(c.x);
    r.v[0] = has_l ? l : 0.f;
    r.v[1] = c.x; r.v[2] = c.y; r.v[3] = c.z; r.v[4] = c.w;
    r.v[5] = has_r ? rr : 0.f;
}
__device__ __forceinline__ void stencil_row(const Row6& a, const Row6& b, const Row6& c, const float (&w)[9], float (&o)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {                                  // explicit FMAs: the file is built with -ffp-contract=off
        float t = w[0] * a.v[j];
        t = fmaf(w[1], a.v[j + 1], t); t = fmaf(w[2], a.v[j + 2], t);
        t = fmaf(w[3], b.v[j], t); t = fmaf(w[4], b.v[j + 1], t); t = fmaf(w[5], b.v[j + 2], t);
        t = fmaf(w[6], c.v[j], t); t = fmaf(w[7], c.v[j + 1], t); t = fmaf(w[8], c.v[j + 2], t);
        o[j] = t;
    }
}
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

// GDFN gate backward (recomputes the depthwise outputs from p):
// dd[b][j] = dg * d2 * gelu'(d1) ; dd[b][j+hid] = dg * gelu(d1)
// G > 0 additionally accumulates the depthwise WEIGHT gradient  dwg[c][3][3] += sum dd[c] (*) p[c]  for c = j, j+hid:
// both operands (the dd values just formed and the three live rows of p) are already in registers, so the separate
// pass that re-read the two 2*hid-channel tensors is gone.  G = lanes that share one plane: 256 (whole workgroup),
// 64 (one wavefront) or 1 (= gsub lanes, a power of two < 64); sums are combined over those lanes before one
// atomicAdd per value (level 1: 8 per address).
template <int G, int RS>
__global__ __launch_bounds__(256) void gate_bwd_kernel(const float* __restrict__ p, const float* __restrict__ w,
                                                       const float* __restrict__ dg, float* __restrict__ dd,
                                                       float* __restrict__ dwg, long nthreads, int hid, int H, int W,
                                                       int gsub) {
    __shared__ float red[4][18];
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
                const float gv[4] = {gq.x, gq.y, gq.z, gq.w};
                float d1[4], d2[4], av[4], cv[4];
                stencil_row(up1, mid1, dn1, w1, d1);
                stencil_row(up2, mid2, dn2, w2, d2);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float ge, gd;
                    gelu_and_grad(d1[k], ge, gd);
                    av[k] = gv[k] * d2[k] * gd;
                    cv[k] = gv[k] * ge;
                }
                *reinterpret_cast<float4*>(dd1 + (long)y * W + b.x0) = make_float4(av[0], av[1], av[2], av[3]);
                *reinterpret_cast<float4*>(dd2 + (long)y * W + b.x0) = make_float4(cv[0], cv[1], cv[2], cv[3]);
                if (G > 0) {
#pragma unroll
                    for (int dj = 0; dj < 3; ++dj)
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            s[0 + dj] = fmaf(av[k], up1.v[k + dj], s[0 + dj]);
                            s[3 + dj] = fmaf(av[k], mid1.v[k + dj], s[3 + dj]);
                            s[6 + dj] = fmaf(av[k], dn1.v[k + dj], s[6 + dj]);
                            s[9 + dj] = fmaf(cv[k], up2.v[k + dj], s[9 + dj]);
                            s[12 + dj] = fmaf(cv[k], mid2.v[k + dj], s[12 + dj]);
                            s[15 + dj] = fmaf(cv[k], dn2.v[k + dj], s[15 + dj]);
                        }
                }
            }
        }
    }
    if (G == 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gl = G >= 64 ? 64 : gsub;                     // lanes combined by shuffles
#pragma unroll
    for (int i = 0; i < 18; ++i) {
        float v = s[i];
        for (int o = gl >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        s[i] = v;
    }
    if (G == 256) {
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 18; ++i) red[wave][i] = s[i];
        }
        __syncthreads();
        if (threadIdx.x < 18) {                              // G == 256: every thread of the workgroup is live
            const int i = threadIdx.x;
            const float v = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
            atomicAdd(&dwg[(i < 9 ? j : j + hid) * 9 + (i < 9 ? i : i - 9)], v);
        }
    } else if ((lane & (gl - 1)) == 0 && b.live) {
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            atomicAdd(&dwg[j * 9 + i], s[i]);
            atomicAdd(&dwg[(j + hid) * 9 + i], s[9 + i]);
        }
    }
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
    __shared__ float red[4][18];
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
    float w1[9], w2[9], f1[9], f2[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { w1[i] = w[j * 9 + i]; w2[i] = w[(j + hid) * 9 + i]; }
#pragma unroll
    for (int i = 0; i < 9; ++i) { f1[i] = w1[8 - i]; f2[i] = w2[8 - i]; }      // 180-degree rotated filters
    const bool has_l = b.x0 > 0, has_r = b.x0 + 4 < W;
    float s[18];
#pragma unroll
    for (int i = 0; i < 18; ++i) s[i] = 0.f;
    Row6 a1[3], a2[3];            // p rows   y0-2+q   in slot q % 3
    Row6 e1[3], e2[3];            // dd rows  y0-1+i   in slot i % 3   (v[0], v[5] = halo columns)
    // Software pipeline: the three 16-byte loads an iteration needs (row r+1 of both p planes, row r of dg) are REQUESTED one
    // iteration ahead, unconditionally, from clamped row indices (out-of-range rows and dead tail threads are zeroed by selects
    // when the data lands).  With the loads inside `if (row exists)` blocks each one was followed by s_waitcnt vmcnt(0) — three
    // serialised memory round trips per row, 54 per strip (ISA of round 3, scripts/README.md "stencil ISA").
    float4 n1, n2, ng;
    auto request = [&](int yp, int yg) {
        const int ypc = min(max(yp, 0), H - 1), ygc = min(max(yg, 0), H - 1);
        n1 = *reinterpret_cast<const float4*>(p1 + (long)ypc * W + b.x0);
        n2 = *reinterpret_cast<const float4*>(p2 + (long)ypc * W + b.x0);
        ng = *reinterpret_cast<const float4*>(gp + (long)ygc * W + b.x0);
    };
    auto land = [&](const float4& q, int y, Row6& r) {
        const bool ok = b.live && y >= 0 && y < H;
        const float4 c = ok ? q : make_float4(0.f, 0.f, 0.f, 0.f);
        const float l = from_lane_below(c.w), rr = from_lane_above(c.x);
        r.v[0] = has_l ? l : 0.f;
        r.v[1] = c.x; r.v[2] = c.y; r.v[3] = c.z; r.v[4] = c.w;
        r.v[5] = has_r ? rr : 0.f;
    };
    request(b.y0 - 2, 0);
    land(n1, b.y0 - 2, a1[0]); land(n2, b.y0 - 2, a2[0]);
    request(b.y0 - 1, 0);
    land(n1, b.y0 - 1, a1[1]); land(n2, b.y0 - 1, a2[1]);
    request(b.y0, b.y0 - 1);
#pragma unroll
    for (int i = 0; i < RS + 2; ++i) {
        const int r = b.y0 - 1 + i;                             // dd row formed in this iteration
        Row6& up1 = a1[i % 3]; Row6& mid1 = a1[(i + 1) % 3]; Row6& dn1 = a1[(i + 2) % 3];
        Row6& up2 = a2[i % 3]; Row6& mid2 = a2[(i + 1) % 3]; Row6& dn2 = a2[(i + 2) % 3];
        land(n1, r + 1, dn1);
        land(n2, r + 1, dn2);
        const float4 gq = ng;
        if (i < RS + 1) request(r + 2, r + 1);                  // next iteration's rows fly under this iteration's arithmetic
        float av[4] = {0.f, 0.f, 0.f, 0.f}, cv[4] = {0.f, 0.f, 0.f, 0.f};
        if (b.live && r >= 0 && r < H) {
            const float gv[4] = {gq.x, gq.y, gq.z, gq.w};
            float d1[4], d2[4];
            stencil_row(up1, mid1, dn1, w1, d1);
            stencil_row(up2, mid2, dn2, w2, d2);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float ge, gd;
                gelu_and_grad(d1[k], ge, gd);
                av[k] = gv[k] * d2[k] * gd;
                cv[k] = gv[k] * ge;
            }
            if (i >= 1 && i <= RS) {                            // rows of this strip: weight gradient (halo rows belong to others)
#pragma unroll
                for (int dj = 0; dj < 3; ++dj)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        s[0 + dj] = fmaf(av[k], up1.v[k + dj], s[0 + dj]);
                        s[3 + dj] = fmaf(av[k], mid1.v[k + dj], s[3 + dj]);
                        s[6 + dj] = fmaf(av[k], dn1.v[k + dj], s[6 + dj]);
                        s[9 + dj] = fmaf(cv[k], up2.v[k + dj], s[9 + dj]);
                        s[12 + dj] = fmaf(cv[k], mid2.v[k + dj], s[12 + dj]);
                        s[15 + dj] = fmaf(cv[k], dn2.v[k + dj], s[15 + dj]);
                    }
            }
        }
        Row6& ec1 = e1[i % 3];
        Row6& ec2 = e2[i % 3];
        const float l1 = from_lane_below(av[3]), r1 = from_lane_above(av[0]);
        const float l2 = from_lane_below(cv[3]), r2 = from_lane_above(cv[0]);
        ec1.v[0] = has_l ? l1 : 0.f; ec1.v[5] = has_r ? r1 : 0.f;
        ec2.v[0] = has_l ? l2 : 0.f; ec2.v[5] = has_r ? r2 : 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) { ec1.v[1 + k] = av[k]; ec2.v[1 + k] = cv[k]; }
        if (i >= 2) {
            const int y = r - 1;                                // dp row: dd rows y-1, y, y+1 are in slots (i-2)%3, (i-1)%3, i%3
            if (b.live && y < H) {
                float o[4];
                stencil_row(e1[(i + 1) % 3], e1[(i + 2) % 3], e1[i % 3], f1, o);
                *reinterpret_cast<float4*>(o1 + (long)y * W + b.x0) = make_float4(o[0], o[1], o[2], o[3]);
                stencil_row(e2[(i + 1) % 3], e2[(i + 2) % 3], e2[i % 3], f2, o);
                *reinterpret_cast<float4*>(o2 + (long)y * W + b.x0) = make_float4(o[0], o[1], o[2], o[3]);
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gl = G >= 64 ? 64 : gsub;
#pragma unroll
    for (int i = 0; i < 18; ++i) {
        float v = s[i];
        for (int o = gl >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        s[i] = v;
    }
    if (G == 256) {
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 18; ++i) red[wave][i] = s[i];
        }
        __syncthreads();
        if (threadIdx.x < 18) {
            const int i = threadIdx.x;
            const float v = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
            atomicAdd(&dwg[(i < 9 ? j : j + hid) * 9 + (i < 9 ? i : i - 9)], v);
        }
    } else if ((lane & (gl - 1)) == 0 && b.live) {
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            atomicAdd(&dwg[j * 9 + i], s[i]);
            atomicAdd(&dwg[(j + hid) * 9 + i], s[9 + i]);
        }
    }
}

// Depthwise 3x3 backward in one pass: dx = dw3x3(dy; rotated w) and dwg[c][3][3] += sum dy (*) x, on the rolling-row
// strips of gate_bwd_kernel (dy is read once for both results).  G: lanes sharing a plane, as in gate_bwd_kernel.
template <int G, int RS, bool NB>
__global__ __launch_bounds__(256) void dwconv_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                         const float* __restrict__ w, float* __restrict__ dx,
                                                         float* __restrict__ dwg, long nthreads, int C, int H, int W,
                                                         int gsub) {
    __shared__ float red[4][9];
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
    auto ld = [&](const float* pl, int y, Row6& r) {
        if (NB) load_row6_nb(pl, H, W, y, b.x0, has_l, has_r, true, r);
        else load_row6(pl, H, W, y, b.x0, r);
    };
    if (b.live) {
        Row6 g3[3], x3[3];
        // NB: rows are requested one iteration ahead from clamped indices and zeroed by selects when they land (see gdfn_bwd_kernel)
        float4 ng = make_float4(0.f, 0.f, 0.f, 0.f), nx = ng;
        auto request = [&](int y) {
            const int yc = min(max(y, 0), H - 1);
            ng = *reinterpret_cast<const float4*>(gp + (long)yc * W + b.x0);
            nx = *reinterpret_cast<const float4*>(xp + (long)yc * W + b.x0);
        };
        auto land = [&](const float4& q, int y, Row6& r) {
            const bool ok = y >= 0 && y < H;
            const float4 c = ok ? q : make_float4(0.f, 0.f, 0.f, 0.f);
            const float l = from_lane_below(c.w), rr = from_lane_above(c.x);
            r.v[0] = has_l ? l : 0.f;
            r.v[1] = c.x; r.v[2] = c.y; r.v[3] = c.z; r.v[4] = c.w;
            r.v[5] = has_r ? rr : 0.f;
        };
        if (NB) {
            request(b.y0 - 1);
            land(ng, b.y0 - 1, g3[2]); land(nx, b.y0 - 1, x3[2]);
            request(b.y0);
            land(ng, b.y0, g3[0]); land(nx, b.y0, x3[0]);
            request(b.y0 + 1);
        } else {
            ld(gp, b.y0 - 1, g3[2]);
            ld(xp, b.y0 - 1, x3[2]);
            ld(gp, b.y0, g3[0]);
            ld(xp, b.y0, x3[0]);
        }
#pragma unroll
        for (int i = 0; i < RS; ++i) {
            const int y = b.y0 + i;
            if (y < H) {
                Row6& gu = g3[(i + 2) % 3]; Row6& gm = g3[i % 3]; Row6& gd = g3[(i + 1) % 3];
                Row6& xu = x3[(i + 2) % 3]; Row6& xm = x3[i % 3]; Row6& xd = x3[(i + 1) % 3];
                if (NB) {
                    land(ng, y + 1, gd);
                    land(nx, y + 1, xd);
                    if (i + 1 < RS) request(y + 2);
                } else {
                    ld(gp, y + 1, gd);
                    ld(xp, y + 1, xd);
                }
                float o[4];
                stencil_row(gu, gm, gd, wf, o);
                *reinterpret_cast<float4*>(op + (long)y * W + b.x0) = make_float4(o[0], o[1], o[2], o[3]);
#pragma unroll
                for (int dj = 0; dj < 3; ++dj)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        s[0 + dj] = fmaf(gm.v[1 + k], xu.v[k + dj], s[0 + dj]);
                        s[3 + dj] = fmaf(gm.v[1 + k], xm.v[k + dj], s[3 + dj]);
                        s[6 + dj] = fmaf(gm.v[1 + k], xd.v[k + dj], s[6 + dj]);
                    }
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gl = G >= 64 ? 64 : gsub;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        float v = s[i];
        for (int o = gl >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        s[i] = v;
    }
    if (G == 256) {
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) red[wave][i] = s[i];
        }
        __syncthreads();
        if (threadIdx.x < 9) {
            const int i = threadIdx.x;
            atomicAdd(&dwg[c * 9 + i], (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]));
        }
    } else if ((lane & (gl - 1)) == 0 && b.live) {
#pragma unroll
        for (int i = 0; i < 9; ++i) atomicAdd(&dwg[c * 9 + i], s[i]);
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
            Patch r;
            load_patch(xp, H, W, y0, x0, r);
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

// ------------------------------------------------------------------ reductions / elementwise
// out[b*R + r] = sum_n x[b*sXb + r*N + n]^2
__global__ __launch_bounds__(256) void row_sumsq_kernel(const float* __restrict__ x, float* __restrict__ out, int R,
                                                        int N, long sXb) {
    __shared__ float red[4];
    const int r = blockIdx.x, b = blockIdx.y;
    const float* p = x + (long)b * sXb + (long)r * N;
    float s = 0.f;
#pragma unroll 4
    for (int n = threadIdx.x * 4; n < N; n += 1024) {
        const float4 v = *reinterpret_cast<const float4*>(p + n);
        s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    s = block_sum<256>(s, red);
    if (threadIdx.x == 0) out[(long)b * R + r] = s;
}

__global__ void lrelu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ a, float* __restrict__ dz,
                                 long n, float slope) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        dz[i] = a[i] > 0.f ? dy[i] : dy[i] * slope;
}

// db[c] += sum_{b,p} dz[b][c][p]
__global__ __launch_bounds__(256) void bias_grad_kernel(const float* __restrict__ dz, float* __restrict__ db, int B,
                                                        int C, int P) {
    __shared__ float red[4];
    const int c = blockIdx.x;
    float s = 0.f;
    for (int b = 0; b < B; ++b) {
        const float* p = dz + ((long)b * C + c) * P;
#pragma unroll 8
        for (int i = threadIdx.x; i < P; i += 256) s += p[i];
    }
    s = block_sum<256>(s, red);
    if (threadIdx.x == 0) atomicAdd(&db[c], s);
}

// out[r][c] = a*x[r][c] + b*y[r][c]   (row strides sx/sy/so; y may be null; out may alias x or y)
__global__ void axpby2d_kernel(const float* x, long sx, const float* y, long sy, float* out, long so, long rows,
                               long cols, float a, float b) {
    const long n = rows * cols;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long r = i / cols, c = i - r * cols;
        out[r * so + c] = a * x[r * sx + c] + (y ? b * y[r * sy + c] : 0.f);
    }
}

// p[0:n) = v: 16-byte stores over the aligned middle, scalar stores at the two ends
__global__ void fill_kernel(float* __restrict__ p, long n, float v) {
    const long head = min(n, (long)((4 - (((uintptr_t)p >> 2) & 3)) & 3));
    const long n4 = (n - head) >> 2;
    float4* q = reinterpret_cast<float4*>(p + head);
    const float4 v4 = make_float4(v, v, v, v);
    const long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x, ts = (long)gridDim.x * blockDim.x;
    for (long i = t0; i < n4; i += ts) q[i] = v4;
    if (t0 < head) p[t0] = v;
    const long tail = head + 4 * n4;
    if (t0 < n - tail) p[tail + t0] = v;
}

// out[b] = alpha[b]*t[b] + (1-alpha[b])*f[b]
__global__ void lerp_kernel(const float* __restrict__ t, const float* __restrict__ f, const float* __restrict__ alpha,
                            float* __restrict__ out, long per, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float a = alpha[i / per];
        out[i] = a * t[i] + (1.f - a) * f[i];
    }
}

// gradient penalty: norms[b] = ||g_b||_2 ; u0 = (20/Bg) (n-1)/n * g ; gp += (10/Bg) sum_b (n_b - 1)^2
__global__ __launch_bounds__(256) void gp_norm_kernel(const float* __restrict__ g, float* __restrict__ norms, long per) {
    __shared__ float red[4];
    const float* p = g + (long)blockIdx.x * per;
    float s = 0.f;
    for (long i = threadIdx.x; i < per; i += 256) s += p[i] * p[i];
    s = block_sum<256>(s, red);
    if (threadIdx.x == 0) norms[blockIdx.x] = sqrtf(s);
}
__global__ void gp_scale_kernel(const float* __restrict__ g, const float* __restrict__ norms, float* __restrict__ u0,
                                float* __restrict__ gp_out, long per, int B, float inv_bg) {
    const long n = per * B;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += (norms[b] - 1.f) * (norms[b] - 1.f);
        *gp_out = 10.f * inv_bg * s;
    }
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float nm = norms[i / per];
        const float coef = nm > 0.f ? 20.f * inv_bg * (nm - 1.f) / nm : 0.f;
        u0[i] = coef * g[i];
    }
}

// PixelUnshuffle(2) (mode 1): in [P][H][W] -> out [4P][H/2][W/2]; PixelShuffle(2) (mode 2): in [4P][H][W] -> out [P][2H][2W]
__global__ void pixel_shuffle_kernel(const float* __restrict__ in, float* __restrict__ out, long n, int H, int W, int mode) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % W);
        const long t = i / W;
        const int y = (int)(t % H);
        const long ch = t / H;
        long o;
        if (mode == 1) {
            const long oc = 4 * ch + 2 * (y & 1) + (x & 1);
            o = (oc * (H >> 1) + (y >> 1)) * (W >> 1) + (x >> 1);
        } else {
            const long oc = ch >> 2;
            const int ii = (int)((ch >> 1) & 1), jj = (int)(ch & 1);
            o = (oc * (2 * H) + (2 * y + ii)) * (2L * W) + (2 * x + jj);
        }
        out[o] = in[i];
    }
}

// consecutive lanes own consecutive pixel quads of one row and rows start at lane positions that are multiples of W/4
inline bool nb_lanes_ok(int W) { const int wq = W >> 2; return (W & 3) == 0 && wq >= 1 && wq <= 64 && (64 % wq) == 0; }

}  // namespace

namespace {
template <int RS>
int launch_gdfn_bwd(const float* p, const float* w, const float* dg, float* dp, float* dwg, int B, int hid, int H, int W,
                    hipStream_t st, bool& fused) {
    const int tpp = cdiv(H, RS) * (W >> 2);
    const long nt = (long)B * hid * tpp;
    const dim3 grid(cdiv(nt, 256));
#define RCOT_GF(G, SUB) do { note_kernel("gdfn_bwd_kernel<%d, %d>", G, RS); RCOT_LAUNCH((gdfn_bwd_kernel<G, RS>), grid, dim3(256), 0, st, p, w, dg, dp, dwg, nt, hid, H, W, SUB); } while (0)
    fused = true;
    if (tpp % 256 == 0) { RCOT_GF(256, 64); }
    else if (tpp % 64 == 0) { RCOT_GF(64, 64); }
    else if (tpp < 64 && (tpp & (tpp - 1)) == 0) { RCOT_GF(1, tpp); }
    else fused = false;
#undef RCOT_GF
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}
}  // namespace

namespace {
template <int RS>
int launch_dwconv_bwd(const float* dy, const float* x, const float* w, float* dx, float* dwg, int B, int C, int H, int W,
                      hipStream_t st, bool& fused) {
    const int tpp = cdiv(H, RS) * (W >> 2);
    const long nt = (long)B * C * tpp;
    const dim3 grid(cdiv(nt, 256));
    const bool nb = nb_lanes_ok(W);
#define RCOT_DB(G, SUB)                                                                                                       \
    do {                                                                                                                       \
        if (nb) RCOT_LAUNCH((dwconv_bwd_kernel<G, RS, true>), grid, dim3(256), 0, st, dy, x, w, dx, dwg, nt, C, H, W, SUB); \
        else RCOT_LAUNCH((dwconv_bwd_kernel<G, RS, false>), grid, dim3(256), 0, st, dy, x, w, dx, dwg, nt, C, H, W, SUB);   \
    } while (0)
    fused = true;
    if (tpp % 256 == 0) { RCOT_DB(256, 64); }
    else if (tpp % 64 == 0) { RCOT_DB(64, 64); }
    else if (tpp < 64 && (tpp & (tpp - 1)) == 0) { RCOT_DB(1, tpp); }
    else fused = false;
#undef RCOT_DB
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}
}  // namespace

namespace {
template <int RS>
int launch_gate_bwd(const float* p, const float* w, const float* dg, float* dd, float* dwg, int B, int hid, int H, int W,
                    hipStream_t st, bool& fused) {
    const int tpp = cdiv(H, RS) * (W >> 2);                 // threads (RS-row strips x 4-pixel columns) per plane
    const long nt = (long)B * hid * tpp;
    const dim3 grid(cdiv(nt, 256));
#define RCOT_GB(G, SUB) RCOT_LAUNCH((gate_bwd_kernel<G, RS>), grid, dim3(256), 0, st, p, w, dg, dd, dwg, nt, hid, H, W, SUB)
    fused = true;
    if (!dwg) { RCOT_GB(0, 0); }
    else if (tpp % 256 == 0) { RCOT_GB(256, 64); }
    else if (tpp % 64 == 0) { RCOT_GB(64, 64); }
    else if (tpp < 64 && (tpp & (tpp - 1)) == 0) { RCOT_GB(1, tpp); }
    else { RCOT_GB(0, 0); fused = false; }
#undef RCOT_GB
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}
}  // namespace

extern "C" {

int rcot_ln_stats(const float* x, float* mu, float* rs, int B, int C, int N, void* stream) {
    if (!x || !mu || !rs || B <= 0 || C <= 0 || N <= 0) return RCOT_EINVAL;
    if ((N & 3) || (reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(mu) & 15) ||
        (reinterpret_cast<uintptr_t>(rs) & 15))
        return RCOT_EINVAL;
    RCOT_LAUNCH(ln_stats_kernel, dim3(cdiv(N, LN_PIX), B), dim3(256), 0, (hipStream_t)stream, x, mu, rs, C, N);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

int rcot_ln_bwd(const float* g, const float* x, const float* mu, const float* rs, const float* w, const float* dres,
                float* dx, float* dw, float* db, int B, int C, int N, void* ws, long ws_bytes, void* stream) {
    if (!g || !x || !mu || !rs || !w || !dx || !ws || B <= 0 || C <= 0 || C > 512 || N <= 0 || B > 65535) return RCOT_EINVAL;
    if ((dw == nullptr) != (db == nullptr)) return RCOT_EINVAL;   // both null: the partial rows stay in ws (deferred reduce)
    if ((N & 3) || !al16(g) || !al16(x) || !al16(mu) || !al16(rs) || !al16(dx) || !al16(dres)) return RCOT_EINVAL;   // float4 rows
    // 64-pixel tiles while they still give >= 512 workgroups, 16-pixel tiles on the small levels; at most ~1024 partial rows
    const bool wide = (long)cdiv(N, 64) * B >= 512;
    const int tiles = cdiv(N, wide ? 64 : 16);
    int gx = 1024 / B;
    if (gx < 1) gx = 1;
    if (gx > tiles) gx = tiles;
    const long need = (long)gx * B * 2 * C * (long)sizeof(float);
    if (ws_bytes < need) return RCOT_EINVAL;
    float* part = static_cast<float*>(ws);
    const dim3 grid(gx, B);
    const int TY = wide ? 16 : 64;
    const int nc = (C % TY == 0 && (C / TY == 3 || C / TY == 6)) ? C / TY : 0;
#define RCOT_LNB(NC, TX) do { note_kernel("ln_bwd_kernel<%d, %d>", NC, TX); RCOT_LAUNCH((ln_bwd_kernel<NC, TX>), grid, dim3(256), 0, (hipStream_t)stream, g, x, mu, rs, w, dres, dx, part, C, N); } while (0)
    if (wide) {
        if (nc == 3) RCOT_LNB(3, 16);
        else if (nc == 6) RCOT_LNB(6, 16);
        else RCOT_LNB(0, 16);
    } else {
        if (nc == 3) RCOT_LNB(3, 4);
        else if (nc == 6) RCOT_LNB(6, 4);
        else RCOT_LNB(0, 4);
    }
#undef RCOT_LNB
    RCOT_LAUNCH_CHECK();
    if (dw) {
        RCOT_LAUNCH(ln_param_reduce_kernel, dim3(cdiv(2 * C, 32)), dim3(1024), 0, (hipStream_t)stream, part, gx * B, C, dw, db);
        RCOT_LAUNCH_CHECK();
    }
    return RCOT_OK;
}

int rcot_ln_bwd_rows(int B, int C, int N) {
    (void)C;
    if (B <= 0 || N <= 0) return 0;
    const bool wide = (long)cdiv(N, 64) * B >= 512;
    const int tiles = cdiv(N, wide ? 64 : 16);
    int gx = 1024 / B;
    if (gx < 1) gx = 1;
    if (gx > tiles) gx = tiles;
    return gx * B;
}

int rcot_block_param_reduce(const float* part1, const float* part2, int rows, int C, float* gw1, float* gb1, float* gw2,
                            float* gb2, const float* dWo_part, float* gWo, const float* dtemp_part, float* gtemp, int B,
                            int heads, const long long* slab_sets, int n_sets, void* stream) {
    if (!part1 || !part2 || !gw1 || !gb1 || !gw2 || !gb2 || !dWo_part || !gWo || !dtemp_part || !gtemp || rows <= 0 || C <= 0 ||
        B <= 0 || heads <= 0 || heads > 1024 || n_sets < 0 || n_sets > 4 || (n_sets && !slab_sets))
        return RCOT_EINVAL;
    const int nl = cdiv(2 * C, 32);
    const int nw = cdiv((long)C * C, 1024);
    SlabSets ss{};
    ss.n = n_sets;
    int chunks = 0;
    for (int d = 0; d < n_sets; ++d) {                                  // HOST rows { ws, S, M, N, ldws, dst, ldd }
        const long long* r = slab_sets + 7 * d;
        ss.ws[d] = reinterpret_cast<const float*>(r[0]);
        ss.S[d] = (int)r[1]; ss.M[d] = (int)r[2]; ss.N[d] = (int)r[3]; ss.ldws[d] = (int)r[4];
        ss.dst[d] = reinterpret_cast<float*>(r[5]);
        ss.ldd[d] = r[6];
        if (!ss.ws[d] || !ss.dst[d] || ss.S[d] <= 0 || ss.M[d] <= 0 || ss.N[d] <= 0 || ss.ldws[d] < ss.N[d]) return RCOT_EINVAL;
        ss.chunk0[d] = chunks;
        const long mn_ = (long)ss.M[d] * ss.N[d];
        ss.per[d] = ss.S[d] <= 8 ? 4096 : (mn_ >= 256 * 1024 ? 1024 : 256);
        chunks += cdiv(mn_, ss.per[d]);
    }
    ss.chunk0[n_sets] = chunks;
    RCOT_LAUNCH(block_param_reduce_kernel, dim3(2 * nl + nw + chunks), dim3(1024), 0, (hipStream_t)stream, part1, part2, rows,
                       C, gw1, gb1, gw2, gb2, dWo_part, gWo, dtemp_part, gtemp, B, heads, nw, ss);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

int rcot_dwconv3x3(const float* x, const float* w, float* y, int B, int C, int H, int W, int flip, void* stream) {
    if (!x || !w || !y || B <= 0 || C <= 0 || H <= 0 || W <= 0) return RCOT_EINVAL;
    if ((W & 3) || (H & 3)) {
        if (flip) return RCOT_EINVAL;                      // the data gradient is only needed at training patch sizes
        const long total = (long)B * C * H * W;
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
        RCOT_LAUNCH(gate_fwd_any_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, p, w, g, total, hid, H, W);
        RCOT_LAUNCH_CHECK();
        return RCOT_OK;
    }
    if (!al16(p) || !al16(g)) return RCOT_EINVAL;
    const long nq = (long)B * hid * (H >> 2) * (W >> 2);
    // the neighbour-lane form of the patch loads (all twelve rows of both planes requested before the first lane shift; with the
    // loads inside per-row `if` blocks it measured SLOWER than the scalar-halo form, 33.8 vs 30.8 us)
    if (nb_lanes_ok(W))
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
    // strip height: the tallest of 16 / 8 / 4 rows that still leaves >= 400k threads (about 6 wavefronts per SIMD)
    const long cols = (long)B * hid * (W >> 2);
    bool fused = true;
    int rc;
    if (cols * cdiv(H, 16) >= 400000) rc = launch_gate_bwd<16>(p, w, dg, dd, dwg, B, hid, H, W, (hipStream_t)stream, fused);
    else if (cols * cdiv(H, 8) >= 400000) rc = launch_gate_bwd<8>(p, w, dg, dd, dwg, B, hid, H, W, (hipStream_t)stream, fused);
    else rc = launch_gate_bwd<4>(p, w, dg, dd, dwg, B, hid, H, W, (hipStream_t)stream, fused);
    if (rc != RCOT_OK) return rc;
    if (dwg && !fused) return rcot_dwconv3x3_wgrad(dd, p, dwg, B, 2 * hid, H, W, stream);   // odd plane sizes: separate pass
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
    const int wq = W >> 2;
    bool fused = wq <= 64 && (64 % wq) == 0;                  // the neighbour-lane exchange needs whole row segments per wavefront
    if (fused) {
        // strip height: halo rows cost (RS+2)/RS, so prefer tall strips while >= 200k threads remain
        const long cols = (long)B * hid * wq;
        int rc;
        if (cols * cdiv(H, 16) >= 200000) rc = launch_gdfn_bwd<16>(p, w, dg, dp, dwg, B, hid, H, W, (hipStream_t)stream, fused);
        else if (cols * cdiv(H, 8) >= 200000) rc = launch_gdfn_bwd<8>(p, w, dg, dp, dwg, B, hid, H, W, (hipStream_t)stream, fused);
        else rc = launch_gdfn_bwd<4>(p, w, dg, dp, dwg, B, hid, H, W, (hipStream_t)stream, fused);
        if (rc != RCOT_OK) return rc;
        if (fused) return RCOT_OK;
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
    const long cols = (long)B * C * (W >> 2);
    bool fused = true;
    int rc;
    if (cols * cdiv(H, 16) >= 400000) rc = launch_dwconv_bwd<16>(dy, x, w, dx, dwg, B, C, H, W, (hipStream_t)stream, fused);
    else if (cols * cdiv(H, 8) >= 400000) rc = launch_dwconv_bwd<8>(dy, x, w, dx, dwg, B, C, H, W, (hipStream_t)stream, fused);
    else rc = launch_dwconv_bwd<4>(dy, x, w, dx, dwg, B, C, H, W, (hipStream_t)stream, fused);
    if (rc != RCOT_OK) return rc;
    if (!fused) {                                             // odd plane sizes: the two separate passes
        rc = rcot_dwconv3x3(dy, w, dx, B, C, H, W, 1, stream);
        if (rc != RCOT_OK) return rc;
        return rcot_dwconv3x3_wgrad(dy, x, dwg, B, C, H, W, stream);
    }
    return RCOT_OK;
}

int rcot_row_sumsq(const float* x, float* out, int B, int R, int N, long sXb, void* stream) {
    if (!x || !out || B <= 0 || R <= 0 || N <= 0 || (N & 3) || (sXb & 3) || !al16(x) || B > 65535) return RCOT_EINVAL;
    RCOT_LAUNCH(row_sumsq_kernel, dim3(R, B), dim3(256), 0, (hipStream_t)stream, x, out, R, N, sXb);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

int rcot_lrelu_bwd(const float* dy, const float* a, float* dz, long n, float slope, void* stream) {
    if (!dy || !a || !dz || n <= 0) return RCOT_EINVAL;
    RCOT_LAUNCH(lrelu_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, dy, a, dz, n, slope);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

int rcot_bias_grad(const float* dz, float* db, int B, int C, int P, void* stream) {
    if (!dz || !db || B <= 0 || C <= 0 || P <= 0) return RCOT_EINVAL;
    RCOT_LAUNCH(bias_grad_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, dz, db, B, C, P);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

int rcot_axpby2d(const float* x, long sx, const float* y, long sy, float* out, long so, long rows, long cols, float a,
                 float b, void* stream) {
    if (!x || !out || rows <= 0 || cols <= 0) return RCOT_EINVAL;
    RCOT_LAUNCH(axpby2d_kernel, dim3(grid_for(rows * cols)), dim3(256), 0, (hipStream_t)stream, x, sx, y, sy, out,
                       so, rows, cols, a, b);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

int rcot_fill(float* p, long n, float v, void* stream) {
    if (!p || n <= 0) return RCOT_EINVAL;
    RCOT_LAUNCH(fill_kernel, dim3(grid_for((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p, n, v);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

int rcot_lerp(const float* t, const float* f, const float* alpha, float* out, int B, long per, void* stream) {
    if (!t || !f || !alpha || !out || B <= 0 || per <= 0) return RCOT_EINVAL;
    RCOT_LAUNCH(lerp_kernel, dim3(grid_for(per * B)), dim3(256), 0, (hipStream_t)stream, t, f, alpha, out, per, per * B);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

int rcot_gp_penalty(const float* g, float* norms, float* u0, float* gp_out, int B, long per, float inv_global_batch,
                    void* stream) {
    if (!g || !norms || !u0 || !gp_out || B <= 0 || per <= 0) return RCOT_EINVAL;
    RCOT_LAUNCH(gp_norm_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, g, norms, per);
    RCOT_LAUNCH_CHECK();
    RCOT_LAUNCH(gp_scale_kernel, dim3(grid_for(per * B)), dim3(256), 0, (hipStream_t)stream, g, norms, u0, gp_out,
                       per, B, inv_global_batch);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

int rcot_pixel_shuffle(const float* in, float* out, long planes, int H, int W, int mode, void* stream) {
    if (!in || !out || planes <= 0 || H <= 0 || W <= 0 || (mode != 1 && mode != 2)) return RCOT_EINVAL;
    if (mode == 1 && ((H | W) & 1)) return RCOT_EINVAL;
    if (mode == 2 && (planes & 3)) return RCOT_EINVAL;
    const long n = planes * H * W;
    RCOT_LAUNCH(pixel_shuffle_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, in, out, n, H, W, mode);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

}  // extern "C"
