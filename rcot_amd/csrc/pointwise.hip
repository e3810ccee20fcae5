// HBM-bound kernels of the RCOT hot path: per-pixel LayerNorm statistics / backward, the parameter-gradient
// reduce that closes a block, row reductions and the small elementwise pieces of the minimax step (the
// depthwise 3x3 stencils live in stencil.hip).  NCHW fp32; pixels are the fastest axis so a wavefront
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

// The slab part of the launch above, also a launch of its own (slab_sets_reduce_kernel): workgroup ``cb`` of the sets' chunks, 1024 threads.
__device__ __forceinline__ void slab_chunk_sum(const SlabSets& ss, int cb) {
    __shared__ float part4[4][1024];
    // ---- slab set d, ss.per[d] outputs per workgroup.  S > 8: thread = (one or four outputs, slab group q); S <= 8:
    // outputs [4096 c, 4096 c + 4096), four outputs per thread with all their slabs in flight
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
        float* part = &part4[0][0];                                      // [4][256] at the start of the S > 8 scratch
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
        slab_chunk_sum(ss, blk - 2 * nl - nw);
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

// dst += sum_s slab[s] for up to four slab sets and nothing else (rcot_slab_sets_reduce): the slab workgroups of the launch above in a
// launch of their own, so that sets which are complete long before the block closes can be summed where a stream is idle.  That launch
// runs NEXT TO the other stream's kernels: on a grid of all its chunks (100 - 1150 workgroups) it takes the memory system for 35 - 70 us
// and the latency-bound kernels beside it last up to twice as long (the 64-workgroup dM product 39 -> 67 us), which gave back 0.56 of
// the 1.33 ms per step the closing launch lost.  So at most SLAB_SETS_WGS workgroups walk the chunks: the sum has 140 - 300 us of idle
// stream to finish in.  ms per step, exact fp32, B = 8, 128 x 128, four alternating rounds: all chunks 73.29, 96 workgroups 72.89,
// 64: 72.47, 48: 72.67, 32: 74.25, 16: 79.8 (too few: presumably the sum is then in the way of the qkv weight gradient) — profiles/early_slab_sums.txt
constexpr int SLAB_SETS_WGS = 64;
__global__ __launch_bounds__(1024) void slab_sets_reduce_kernel(SlabSets ss) {
    const int total = ss.chunk0[ss.n];
    for (int cb = blockIdx.x; cb < total; cb += gridDim.x) {
        slab_chunk_sum(ss, cb);
        __syncthreads();                  // the next chunk re-uses the LDS scratch (the form is uniform over a workgroup: every thread arrives)
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

// Grid of ln_bwd_kernel, gx x B workgroups (returns gx): 64-pixel tiles while they still give >= 512 workgroups (*wide), 16-pixel
// tiles on the small levels; at most ~1024 partial rows.  The launch, its workspace check and rcot_ln_bwd_rows all read it here.
inline int ln_bwd_grid(int B, int N, bool* wide) {
    *wide = (long)cdiv(N, 64) * B >= 512;
    const int tiles = cdiv(N, *wide ? 64 : 16);
    int gx = 1024 / B;
    if (gx < 1) gx = 1;
    if (gx > tiles) gx = tiles;
    return gx;
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
    bool wide;
    const int gx = ln_bwd_grid(B, N, &wide);
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
    bool wide;
    return ln_bwd_grid(B, N, &wide) * B;
}

// HOST rows { ws, S, M, N, ldws, dst, ldd } -> the kernels' SlabSets; returns the number of chunks (workgroups) of all sets, -1 for a
// row that cannot be.  The one place that decides how many outputs a workgroup of a set takes.
static int slab_sets_fill(SlabSets& ss, const long long* slab_sets, int n_sets) {
    ss.n = n_sets;
    int chunks = 0;
    for (int d = 0; d < n_sets; ++d) {
        const long long* r = slab_sets + 7 * d;
        ss.ws[d] = reinterpret_cast<const float*>(r[0]);
        ss.S[d] = (int)r[1]; ss.M[d] = (int)r[2]; ss.N[d] = (int)r[3]; ss.ldws[d] = (int)r[4];
        ss.dst[d] = reinterpret_cast<float*>(r[5]);
        ss.ldd[d] = r[6];
        if (!ss.ws[d] || !ss.dst[d] || ss.S[d] <= 0 || ss.M[d] <= 0 || ss.N[d] <= 0 || ss.ldws[d] < ss.N[d]) return -1;
        ss.chunk0[d] = chunks;
        const long mn_ = (long)ss.M[d] * ss.N[d];
        ss.per[d] = ss.S[d] <= 8 ? 4096 : (mn_ >= 256 * 1024 ? 1024 : 256);
        chunks += cdiv(mn_, ss.per[d]);
    }
    ss.chunk0[n_sets] = chunks;
    return chunks;
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
    const int chunks = slab_sets_fill(ss, slab_sets, n_sets);
    if (chunks < 0) return RCOT_EINVAL;
    RCOT_LAUNCH(block_param_reduce_kernel, dim3(2 * nl + nw + chunks), dim3(1024), 0, (hipStream_t)stream, part1, part2, rows,
                       C, gw1, gb1, gw2, gb2, dWo_part, gWo, dtemp_part, gtemp, B, heads, nw, ss);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

int rcot_slab_sets_reduce(const long long* slab_sets, int n_sets, void* stream) {
    if (!slab_sets || n_sets < 1 || n_sets > 4) return RCOT_EINVAL;
    SlabSets ss{};
    const int chunks = slab_sets_fill(ss, slab_sets, n_sets);
    if (chunks < 0) return RCOT_EINVAL;
    RCOT_LAUNCH(slab_sets_reduce_kernel, dim3(chunks < SLAB_SETS_WGS ? chunks : SLAB_SETS_WGS), dim3(1024), 0, (hipStream_t)stream, ss);
    RCOT_LAUNCH_CHECK();
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
