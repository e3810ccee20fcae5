// Fourier residual-guided OT cost of the generator step (reference: trainer.py:320-343; math: SURVEY.md A.5).
//   res = degraded - T(x);  rmse = sqrt(mean res^2) over the (global) batch
//   de_id < 3 : f_i = mean|FFT2(res_i)|^2 / 2  ==  sum(res_i^2)/6          (Parseval: no FFT needed)
//   else      : f_i = mean|FFT2(res_i)|        -> real 2-D FFT, line by line through LDS
//   loss_T   += sigma*(rmse + sum_i f_i) [+ Sigma*mean|T(x)-y|]
// Elementwise / bandwidth-bound work, no MFMA.  The spectrum branch runs three line-FFT passes
// (rows forward; columns forward -> |F|, F/|F| -> columns inverse; rows inverse) over an L2-resident
// complex scratch; each wavefront owns one line in LDS.  The line transform is chosen per axis by rcot_fft_plan (rows: W,
// columns: H): powers of two run the in-place radix-2 fft_line; lengths with prime factors <= 13 a mixed-radix Stockham
// autosort between two LDS buffers; every other length <= 1024 Bluestein's chirp-z over three radix-2 transforms.
#include "common.h"
#include "../../include/rcot_hip.h"

using namespace rcot;

namespace {

constexpr int MAXP = 1024;         // longest FFT line
constexpr int LPB = 4;             // lines per block (one per wavefront)

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// In-place radix-2 DIT FFT of one line of length P = 1<<logP held in LDS (owned by one wavefront).
// sign = -1 forward, +1 inverse (unnormalised).
__device__ void fft_line(float2* line, int P, int logP, float sign, int lane) {
    for (int i = lane; i < P; i += 64) {
        const int r = (int)(__brev((unsigned)i) >> (32 - logP));
        if (i < r) { const float2 t = line[i]; line[i] = line[r]; line[r] = t; }
    }
    __syncthreads();
    for (int s = 0; s < logP; ++s) {
        const int half = 1 << s;
        for (int q = lane; q < (P >> 1); q += 64) {
            const int grp = q >> s, pos = q & (half - 1);
            const int i0 = (grp << (s + 1)) + pos, i1 = i0 + half;
            float sn, cs;
            sincospif(sign * (float)pos / (float)half, &sn, &cs);
            const float2 a = line[i0], bt = cmul(line[i1], make_float2(cs, sn));
            line[i0] = make_float2(a.x + bt.x, a.y + bt.y);
            line[i1] = make_float2(a.x - bt.x, a.y - bt.y);
        }
        __syncthreads();
    }
}

// sums[b] += sum res^2 ; sums[B+b] += sum |out-tgt| ; sums[2B] += total res^2 ; sums[2B+1] += total |out-tgt|
__global__ __launch_bounds__(256) void ot_reduce_kernel(const float* __restrict__ deg, const float* __restrict__ out,
                                                        const float* __restrict__ tgt, float* __restrict__ sums, int B,
                                                        long per) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const long base = (long)b * per;
    float s2 = 0.f, l1 = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long)gridDim.x * 256) {
        const float o = out[base + i];
        const float r = deg[base + i] - o;
        s2 += r * r;
        if (tgt) l1 += fabsf(o - tgt[base + i]);
    }
    s2 = block_sum<256>(s2, red);
    l1 = block_sum<256>(l1, red);
    if (threadIdx.x == 0) {
        atomicAdd(&sums[b], s2);
        atomicAdd(&sums[2 * B], s2);
        if (tgt) { atomicAdd(&sums[B + b], l1); atomicAdd(&sums[2 * B + 1], l1); }
    }
}

// pass 1: forward FFT of every row of res (planes of samples with de_id >= 3 only)
__global__ __launch_bounds__(256) void ot_rows_fwd_kernel(const float* __restrict__ deg, const float* __restrict__ out,
                                                          const int* __restrict__ de_id, float2* __restrict__ scr,
                                                          int H, int W, int logW) {
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    const int plane = blockIdx.y, b = plane / 3;
    if (de_id[b] < 3) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * LPB + wave;
    float2* line = sm + wave * W;
    const long base = ((long)plane * H + row) * W;
    if (row < H)
        for (int i = lane; i < W; i += 64) line[i] = make_float2(deg[base + i] - out[base + i], 0.f);
    __syncthreads();
    fft_line(line, W, logW, -1.f, lane);
    if (row < H)
        for (int i = lane; i < W; i += 64) scr[base + i] = line[i];
}

// pass 2: forward FFT of every column -> |F| (sum into spec[b]) and U = F/|F| -> inverse FFT along the column
__global__ __launch_bounds__(256) void ot_cols_kernel(const int* __restrict__ de_id, float2* __restrict__ scr,
                                                      float* __restrict__ spec, int H, int W, int logH) {
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    __shared__ float red[4];
    const int plane = blockIdx.y, b = plane / 3;
    if (de_id[b] < 3) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col = blockIdx.x * LPB + wave;
    float2* line = sm + wave * H;
    float2* p = scr + (long)plane * H * W + col;
    if (col < W)
        for (int i = lane; i < H; i += 64) line[i] = p[(long)i * W];
    __syncthreads();
    fft_line(line, H, logH, -1.f, lane);
    float s = 0.f;
    if (col < W)
        for (int i = lane; i < H; i += 64) {
            const float2 f = line[i];
            const float mag = sqrtf(f.x * f.x + f.y * f.y);
            s += mag;
            line[i] = mag > 0.f ? make_float2(f.x / mag, f.y / mag) : make_float2(0.f, 0.f);
        }
    s = block_sum<256>(s, red);
    if (threadIdx.x == 0) atomicAdd(&spec[b], s);
    __syncthreads();
    fft_line(line, H, logH, 1.f, lane);
    if (col < W)
        for (int i = lane; i < H; i += 64) p[(long)i * W] = line[i];
}

// pass 3: inverse FFT of every row; gF = Re(.) / (3*H*W)   ( == Re(ifft2(U)) / 3 )
__global__ __launch_bounds__(256) void ot_rows_inv_kernel(const int* __restrict__ de_id, const float2* __restrict__ scr,
                                                          float* __restrict__ gF, int H, int W, int logW) {
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    const int plane = blockIdx.y, b = plane / 3;
    if (de_id[b] < 3) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * LPB + wave;
    float2* line = sm + wave * W;
    const long base = ((long)plane * H + row) * W;
    if (row < H)
        for (int i = lane; i < W; i += 64) line[i] = scr[base + i];
    __syncthreads();
    fft_line(line, W, logW, 1.f, lane);
    const float sc = 1.0f / (3.0f * (float)H * (float)W);
    if (row < H)
        for (int i = lane; i < W; i += 64) gF[base + i] = line[i].x * sc;
}

// ---- line transforms for lengths that are not powers of two ------------------------------------------------------------------
constexpr int MAXST = 10;          // stages of a plan (rcot_fft_plan): 2 * 3^5 = 486 needs 6, 2^10 needs 10

// How one axis is transformed; passed by value to the kernels.  ns > 0: mixed radix, rad[0..ns) with product n.
// ns == 0: Bluestein over the power of two M = 1 << logM >= 2n - 1.
struct LinePlan {
    int n, ns, M, logM;
    int rad[MAXST];
};

// One Stockham stage of radix R (decimation in time): src viewed as [R][n/(R L)][L] -> dst [n/(R L)][R][L], L = product of the
// radices already done.  Lane `lane` owns butterflies lane, lane + 64, ...  The twiddle w_{RL}^{q k} has q k < R L, so its
// argument is exact in integers whatever n is; w_R^{q s} are evaluated once per stage.
template <int R>
__device__ void mr_stage(const float2* __restrict__ src, float2* __restrict__ dst, int n, int L, float sign, int lane) {
    const int m = n / R;
    const float invRL = 1.0f / (float)(R * L);
    float2 w[R];
    if constexpr (R != 2 && R != 4) {
#pragma unroll
        for (int q = 0; q < R; ++q) sincospif(sign * (float)(2 * q) / (float)R, &w[q].y, &w[q].x);
    }
    for (int t = lane; t < m; t += 64) {
        const int k = t % L;
        float2 x[R];
        x[0] = src[t];
#pragma unroll
        for (int q = 1; q < R; ++q) {
            float2 v = src[q * m + t];
            if (L > 1) {
                float sn, cs;
                sincospif(sign * ((float)(2 * q * k) * invRL), &sn, &cs);
                v = cmul(v, make_float2(cs, sn));
            }
            x[q] = v;
        }
        float2* o = dst + (t - k) * R + k;
        if constexpr (R == 2) {
            o[0] = make_float2(x[0].x + x[1].x, x[0].y + x[1].y);
            o[L] = make_float2(x[0].x - x[1].x, x[0].y - x[1].y);
        } else if constexpr (R == 4) {
            const float2 a = make_float2(x[0].x + x[2].x, x[0].y + x[2].y), b = make_float2(x[0].x - x[2].x, x[0].y - x[2].y);
            const float2 c = make_float2(x[1].x + x[3].x, x[1].y + x[3].y), d = make_float2(x[1].x - x[3].x, x[1].y - x[3].y);
            const float2 e = make_float2(-sign * d.y, sign * d.x);            // (sign i) d
            o[0] = make_float2(a.x + c.x, a.y + c.y);
            o[L] = make_float2(b.x + e.x, b.y + e.y);
            o[2 * L] = make_float2(a.x - c.x, a.y - c.y);
            o[3 * L] = make_float2(b.x - e.x, b.y - e.y);
        } else {
#pragma unroll
            for (int s = 0; s < R; ++s) {
                float2 acc = x[0];
#pragma unroll
                for (int q = 1; q < R; ++q) {
                    const float2 pr = cmul(x[q], w[(q * s) % R]);
                    acc.x += pr.x;
                    acc.y += pr.y;
                }
                o[s * L] = acc;
            }
        }
    }
    __syncthreads();
}

// Mixed-radix FFT of the line at `cur` (one of the two halves of buf[2n]); returns the half that holds the result.
__device__ float2* mr_line(float2* buf, float2* cur, const LinePlan& p, float sign, int lane) {
    int L = 1;
    for (int s = 0; s < p.ns; ++s) {
        float2* dst = cur == buf ? buf + p.n : buf;
        const int r = p.rad[s];
        switch (r) {
            case 2: mr_stage<2>(cur, dst, p.n, L, sign, lane); break;
            case 3: mr_stage<3>(cur, dst, p.n, L, sign, lane); break;
            case 4: mr_stage<4>(cur, dst, p.n, L, sign, lane); break;
            case 5: mr_stage<5>(cur, dst, p.n, L, sign, lane); break;
            case 7: mr_stage<7>(cur, dst, p.n, L, sign, lane); break;
            case 11: mr_stage<11>(cur, dst, p.n, L, sign, lane); break;
            default: mr_stage<13>(cur, dst, p.n, L, sign, lane); break;
        }
        L *= r;
        cur = dst;
    }
    return cur;
}

// exp(sign i pi k^2 / n), k^2 reduced mod 2n in integers
__device__ __forceinline__ float2 chirp(int k, int n, float sign) {
    const int k2 = (int)(((unsigned)k * (unsigned)k) % (unsigned)(2 * n));
    float sn, cs;
    sincospif(sign * ((float)k2 / (float)n), &sn, &cs);
    return make_float2(cs, sn);
}

// Bluestein: X_k = c_k sum_j (x_j c_j) conj(c)_{k-j}, c_k = exp(sign i pi k^2/n): a circular convolution of length M with the
// chirp filter.  filt = FFT_M(conj(c)) / M for sign = -1 (bs_filter_kernel); conj(c) is even, so the filter of sign = +1 is its
// conjugate.  line[0..n) holds the input, line[0..M) is this wavefront's; the result is left in line[0..n).
__device__ void bs_line(float2* line, const LinePlan& p, float sign, int lane, const float2* __restrict__ filt) {
    for (int i = lane; i < p.M; i += 64) line[i] = i < p.n ? cmul(line[i], chirp(i, p.n, sign)) : make_float2(0.f, 0.f);
    __syncthreads();
    fft_line(line, p.M, p.logM, -1.f, lane);
    for (int i = lane; i < p.M; i += 64) {
        float2 f = filt[i];
        f.y *= -sign;
        line[i] = cmul(line[i], f);
    }
    __syncthreads();
    fft_line(line, p.M, p.logM, 1.f, lane);
    for (int i = lane; i < p.n; i += 64) line[i] = cmul(line[i], chirp(i, p.n, sign));
    __syncthreads();
}

template <bool BS>
__device__ __forceinline__ float2* line_fft(float2* buf, float2* cur, const LinePlan& p, float sign, int lane,
                                            const float2* __restrict__ filt) {
    if constexpr (BS) {
        bs_line(buf, p, sign, lane, filt);
        return buf;
    } else {
        return mr_line(buf, cur, p, sign, lane);
    }
}

// float2 of LDS one wavefront needs for one line
__host__ __device__ inline int line_lds(const LinePlan& p) { return p.ns ? 2 * p.n : p.M; }

// The transformed chirp filter of one Bluestein length, once per call: filt[0..M) = FFT_M(b) / M, b_k = b_{M-k} = exp(+i pi k^2/n)
// for k < n, zero between.  One wavefront.
__global__ __launch_bounds__(64) void bs_filter_kernel(float2* __restrict__ filt, LinePlan p) {
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    const int lane = threadIdx.x;
    for (int i = lane; i < p.M; i += 64) {
        const int k = i < p.n ? i : p.M - i;
        sm[i] = k < p.n ? chirp(k, p.n, 1.f) : make_float2(0.f, 0.f);
    }
    __syncthreads();
    fft_line(sm, p.M, p.logM, -1.f, lane);
    const float sc = 1.0f / (float)p.M;
    for (int i = lane; i < p.M; i += 64) filt[i] = make_float2(sm[i].x * sc, sm[i].y * sc);
}

// The three passes again, over a LinePlan instead of a radix-2 length (same launch geometry, same scratch layout).
template <bool BS>
__device__ __forceinline__ void rows_fwd_body(const float* __restrict__ deg, const float* __restrict__ out,
                                              const int* __restrict__ de_id, float2* __restrict__ scr, int H, int W,
                                              const LinePlan& p, const float2* __restrict__ filt) {
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    const int plane = blockIdx.y, b = plane / 3;
    if (de_id[b] < 3) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * LPB + wave;
    float2* line = sm + wave * line_lds(p);
    const long base = ((long)plane * H + row) * W;
    for (int i = lane; i < W; i += 64) line[i] = row < H ? make_float2(deg[base + i] - out[base + i], 0.f) : make_float2(0.f, 0.f);
    __syncthreads();
    const float2* r = line_fft<BS>(line, line, p, -1.f, lane, filt);
    if (row < H)
        for (int i = lane; i < W; i += 64) scr[base + i] = r[i];
}

template <bool BS>
__device__ __forceinline__ void cols_body(const int* __restrict__ de_id, float2* __restrict__ scr, float* __restrict__ spec,
                                          int H, int W, const LinePlan& p, const float2* __restrict__ filt) {
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    __shared__ float red[4];
    const int plane = blockIdx.y, b = plane / 3;
    if (de_id[b] < 3) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col = blockIdx.x * LPB + wave;
    float2* line = sm + wave * line_lds(p);
    float2* g = scr + (long)plane * H * W + col;
    for (int i = lane; i < H; i += 64) line[i] = col < W ? g[(long)i * W] : make_float2(0.f, 0.f);
    __syncthreads();
    float2* f = line_fft<BS>(line, line, p, -1.f, lane, filt);
    float s = 0.f;
    if (col < W)
        for (int i = lane; i < H; i += 64) {
            const float2 v = f[i];
            const float mag = sqrtf(v.x * v.x + v.y * v.y);
            s += mag;
            f[i] = mag > 0.f ? make_float2(v.x / mag, v.y / mag) : make_float2(0.f, 0.f);
        }
    s = block_sum<256>(s, red);
    if (threadIdx.x == 0) atomicAdd(&spec[b], s);
    __syncthreads();
    const float2* r = line_fft<BS>(line, f, p, 1.f, lane, filt);
    if (col < W)
        for (int i = lane; i < H; i += 64) g[(long)i * W] = r[i];
}

template <bool BS>
__device__ __forceinline__ void rows_inv_body(const int* __restrict__ de_id, const float2* __restrict__ scr,
                                              float* __restrict__ gF, int H, int W, const LinePlan& p,
                                              const float2* __restrict__ filt) {
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    const int plane = blockIdx.y, b = plane / 3;
    if (de_id[b] < 3) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * LPB + wave;
    float2* line = sm + wave * line_lds(p);
    const long base = ((long)plane * H + row) * W;
    for (int i = lane; i < W; i += 64) line[i] = row < H ? scr[base + i] : make_float2(0.f, 0.f);
    __syncthreads();
    const float2* r = line_fft<BS>(line, line, p, 1.f, lane, filt);
    const float sc = 1.0f / (3.0f * (float)H * (float)W);
    if (row < H)
        for (int i = lane; i < W; i += 64) gF[base + i] = r[i].x * sc;
}

#define RCOT_OT_LINE_KERNELS(sfx, BS)                                                                                          \
    __global__ __launch_bounds__(256) void ot_rows_fwd_##sfx##_kernel(                                                         \
        const float* __restrict__ deg, const float* __restrict__ out, const int* __restrict__ de_id, float2* __restrict__ scr, \
        int H, int W, LinePlan p, const float2* __restrict__ filt) {                                                           \
        rows_fwd_body<BS>(deg, out, de_id, scr, H, W, p, filt);                                                                \
    }                                                                                                                          \
    __global__ __launch_bounds__(256) void ot_cols_##sfx##_kernel(const int* __restrict__ de_id, float2* __restrict__ scr,     \
                                                                  float* __restrict__ spec, int H, int W, LinePlan p,          \
                                                                  const float2* __restrict__ filt) {                           \
        cols_body<BS>(de_id, scr, spec, H, W, p, filt);                                                                        \
    }                                                                                                                          \
    __global__ __launch_bounds__(256) void ot_rows_inv_##sfx##_kernel(const int* __restrict__ de_id,                           \
                                                                      const float2* __restrict__ scr, float* __restrict__ gF,  \
                                                                      int H, int W, LinePlan p,                                \
                                                                      const float2* __restrict__ filt) {                       \
        rows_inv_body<BS>(de_id, scr, gF, H, W, p, filt);                                                                      \
    }
RCOT_OT_LINE_KERNELS(mixed, false)
RCOT_OT_LINE_KERNELS(bluestein, true)
#undef RCOT_OT_LINE_KERNELS

// dout += -sigma*( res/(Mg*rmse) + [de_id<3 ? res/3 : gF] ) + Sigma*sign(out-tgt)/Mg
// scal[0]=rmse (global), scal[1]=local Fourier penalty sum, scal[2]=local sum|out-tgt| / Mg
__global__ __launch_bounds__(256) void ot_grad_kernel(const float* __restrict__ deg, const float* __restrict__ out,
                                                      const float* __restrict__ tgt, const int* __restrict__ de_id,
                                                      const float* __restrict__ gF, const float* __restrict__ sums,
                                                      const float* __restrict__ spec, float* __restrict__ dout,
                                                      float* __restrict__ scal, int B, long per, float sigma,
                                                      float Sigma, float Mg) {
    const float tot = sums[2 * B];
    const float rmse = sqrtf(tot / Mg);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        float four = 0.f;
        for (int i = 0; i < B; ++i) four += de_id[i] < 3 ? sums[i] / 6.0f : spec[i] / (float)per;
        scal[0] = rmse;
        scal[1] = four;
        scal[2] = sums[2 * B + 1] / Mg;
    }
    const int b = blockIdx.y;
    const bool l2 = de_id[b] < 3;
    const long base = (long)b * per;
    const float k_rmse = rmse > 0.f ? 1.0f / (Mg * rmse) : 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long)gridDim.x * 256) {
        const float o = out[base + i];
        const float r = deg[base + i] - o;
        float g = -sigma * (r * k_rmse + (l2 ? r * (1.0f / 3.0f) : gF[base + i]));
        if (tgt) {
            const float d = o - tgt[base + i];
            g += Sigma / Mg * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
        }
        dout[base + i] += g;
    }
}

// Host side of a LinePlan: what rcot_fft_plan answers for n.  kind: 0 radix-2 (today's kernels), 1 mixed radix, 2 Bluestein.
int make_plan(int n, LinePlan& p, int& kind) {
    int rad[MAXST];
    const int ns = rcot_fft_plan(n, rad, MAXST);
    if (ns < 0) return ns;
    p.n = n;
    p.ns = ns;
    p.M = p.logM = 0;
    bool two = ns > 0;
    for (int i = 0; i < MAXST; ++i) {
        p.rad[i] = i < ns ? rad[i] : 1;
        if (i < ns && rad[i] != 2) two = false;
    }
    if (ns == 0) {
        p.M = rad[0];
        while ((1 << p.logM) < p.M) ++p.logM;
    }
    kind = two ? 0 : (ns > 0 ? 1 : 2);
    return RCOT_OK;
}

}  // namespace

extern "C" {

int rcot_ot_reduce(const float* degraded, const float* restored, const float* target, float* sums, int B, long per,
                   void* stream) {
    if (!degraded || !restored || !sums || B <= 0 || per <= 0 || B > 65535) return RCOT_EINVAL;
    hipError_t e = hipMemsetAsync(sums, 0, sizeof(float) * (2 * (size_t)B + 2), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    int gx = (int)((per + 256 * 8 - 1) / (256 * 8));
    if (gx < 1) gx = 1;
    RCOT_LAUNCH(ot_reduce_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, degraded, restored, target, sums,
                       B, per);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

int rcot_fft_plan(int n, int* radices, int cap) {
    if (!radices || cap < 1 || n < 2) return RCOT_EINVAL;
    if (n > MAXP) return RCOT_EUNSUPPORTED;
    int ns = 0, m = n;
    if ((n & (n - 1)) == 0) {                            // powers of two: the radix-2 kernel's stage count
        for (; m > 1; m >>= 1, ++ns)
            if (ns < cap) radices[ns] = 2;
        return ns <= cap ? ns : RCOT_EINVAL;
    }
    static const int order[7] = {4, 2, 3, 5, 7, 11, 13};   // radix 4 as often as possible, then 2, then the odd radices
    int rad[MAXST];
    for (int r : order)
        while (m % r == 0) {
            rad[ns++] = r;
            m /= r;
        }
    if (m != 1) {                                        // a prime factor above 13: Bluestein over M >= 2n - 1
        int M = 1;
        while (M < 2 * n - 1) M <<= 1;
        radices[0] = M;
        return 0;
    }
    if (ns > cap) return RCOT_EINVAL;
    for (int i = 0; i < ns; ++i) radices[i] = rad[i];
    return ns;
}

int rcot_ot_spectrum(const float* degraded, const float* restored, const int* de_id, float* gF, float* spec, float* ws,
                     size_t ws_bytes, int B, int H, int W, void* stream) {
    if (!degraded || !restored || !de_id || !gF || !spec || !ws || B <= 0 || B * 3 > 65535) return RCOT_EINVAL;
    LinePlan pw, ph;
    int kw = 0, kh = 0;
    int rc = make_plan(W, pw, kw);
    if (rc == RCOT_OK) rc = make_plan(H, ph, kh);
    if (rc != RCOT_OK) return rc;
    // scratch, then the chirp filter of each axis that runs Bluestein
    const size_t n_scr = (size_t)B * 3 * H * W;
    if (ws_bytes < sizeof(float2) * (n_scr + (kw == 2 ? pw.M : 0) + (kh == 2 ? ph.M : 0))) return RCOT_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(spec, 0, sizeof(float) * (size_t)B, st);
    if (e != hipSuccess) return (int)e;
    float2* scr = reinterpret_cast<float2*>(ws);
    float2* fw = scr + n_scr;
    float2* fh = fw + (kw == 2 ? pw.M : 0);
    if (kw | kh) {
        // LDS per block: 4 lines of 2n (mixed radix, n <= 1000) or M <= 2048 (Bluestein) complex values = up to 64 KiB, plus the
        // columns kernels' 16 static bytes: above the default limit of a launch
        // (a refusal here is not an error of its own: the launch below reports a size it cannot have)
        static const bool raised = [] {
            bool ok = true;
            for (const void* k : {(const void*)ot_rows_fwd_mixed_kernel, (const void*)ot_cols_mixed_kernel,
                                  (const void*)ot_rows_inv_mixed_kernel, (const void*)ot_rows_fwd_bluestein_kernel,
                                  (const void*)ot_cols_bluestein_kernel, (const void*)ot_rows_inv_bluestein_kernel})
                if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) != hipSuccess) {
                    (void)hipGetLastError();
                    ok = false;
                }
            return ok;
        }();
        (void)raised;
    }
    if (kw == 2) {
        RCOT_LAUNCH(bs_filter_kernel, dim3(1), dim3(64), sizeof(float2) * pw.M, st, fw, pw);
        RCOT_LAUNCH_CHECK();
    }
    if (kh == 2) {
        RCOT_LAUNCH(bs_filter_kernel, dim3(1), dim3(64), sizeof(float2) * ph.M, st, fh, ph);
        RCOT_LAUNCH_CHECK();
    }
    const dim3 grows(cdiv(H, LPB), B * 3), gcols(cdiv(W, LPB), B * 3);
    const size_t lw = sizeof(float2) * LPB * line_lds(pw), lh = sizeof(float2) * LPB * line_lds(ph);
    if (kw == 0)
        RCOT_LAUNCH(ot_rows_fwd_kernel, grows, dim3(256), sizeof(float2) * LPB * W, st, degraded, restored, de_id, scr, H, W,
                    pw.ns);
    else if (kw == 1)
        RCOT_LAUNCH(ot_rows_fwd_mixed_kernel, grows, dim3(256), lw, st, degraded, restored, de_id, scr, H, W, pw, fw);
    else
        RCOT_LAUNCH(ot_rows_fwd_bluestein_kernel, grows, dim3(256), lw, st, degraded, restored, de_id, scr, H, W, pw, fw);
    RCOT_LAUNCH_CHECK();
    if (kh == 0)
        RCOT_LAUNCH(ot_cols_kernel, gcols, dim3(256), sizeof(float2) * LPB * H, st, de_id, scr, spec, H, W, ph.ns);
    else if (kh == 1)
        RCOT_LAUNCH(ot_cols_mixed_kernel, gcols, dim3(256), lh, st, de_id, scr, spec, H, W, ph, fh);
    else
        RCOT_LAUNCH(ot_cols_bluestein_kernel, gcols, dim3(256), lh, st, de_id, scr, spec, H, W, ph, fh);
    RCOT_LAUNCH_CHECK();
    note_kernel("%s", kw == 0 ? "ot_rows_inv_kernel" : kw == 1 ? "ot_rows_inv_mixed_kernel" : "ot_rows_inv_bluestein_kernel");
    if (kw == 0)
        RCOT_LAUNCH(ot_rows_inv_kernel, grows, dim3(256), sizeof(float2) * LPB * W, st, de_id, scr, gF, H, W, pw.ns);
    else if (kw == 1)
        RCOT_LAUNCH(ot_rows_inv_mixed_kernel, grows, dim3(256), lw, st, de_id, scr, gF, H, W, pw, fw);
    else
        RCOT_LAUNCH(ot_rows_inv_bluestein_kernel, grows, dim3(256), lw, st, de_id, scr, gF, H, W, pw, fw);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

int rcot_ot_grad(const float* degraded, const float* restored, const float* target, const int* de_id, const float* gF,
                 const float* sums, const float* spec, float* dout, float* scal, int B, long per, float sigma,
                 float Sigma, long global_batch, void* stream) {
    if (!degraded || !restored || !de_id || !sums || !spec || !dout || !scal || B <= 0 || per <= 0 || global_batch <= 0 ||
        B > 65535)
        return RCOT_EINVAL;
    int gx = (int)((per + 256 * 4 - 1) / (256 * 4));
    if (gx < 1) gx = 1;
    RCOT_LAUNCH(ot_grad_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, degraded, restored, target, de_id,
                       gF, sums, spec, dout, scal, B, per, sigma, Sigma, (float)global_batch * (float)per);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

}  // extern "C"
