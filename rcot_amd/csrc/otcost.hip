// Fourier residual-guided OT cost of the generator step (reference: trainer.py:320-343; math: SURVEY.md A.5).
//   res = degraded - T(x);  rmse = sqrt(mean res^2) over the (global) batch
//   de_id < 3 : f_i = mean|FFT2(res_i)|^2 / 2  ==  sum(res_i^2)/6          (Parseval: no FFT needed)
//   else      : f_i = mean|FFT2(res_i)|        -> real 2-D FFT, line by line through LDS
//   loss_T   += sigma*(rmse + sum_i f_i) [+ Sigma*mean|T(x)-y|]
// Elementwise / bandwidth-bound work, no MFMA.  The spectrum branch runs three line-FFT passes
// (rows forward; columns forward -> |F|, F/|F| -> columns inverse; rows inverse) over an L2-resident
// complex scratch; each wavefront owns one line in LDS.  Each pass is one kernel template over the line transform (LineKind),
// chosen per axis by rcot_fft_plan (rows: W, columns: H): powers of two run the in-place radix-2 fft_line; lengths with prime
// factors <= 13 a mixed-radix Stockham autosort between two LDS buffers; every other length <= 1024 Bluestein's chirp-z over
// three radix-2 transforms.
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

// ---- line transforms: one per LineKind ---------------------------------------------------------------------------------------
constexpr int MAXST = 10;          // stages of a plan (rcot_fft_plan): 2 * 3^5 = 486 needs 6, 2^10 needs 10
constexpr int MAXMR = 8;           // radices a LinePlan stores (see there)

enum LineKind { RADIX2, MIXED, BLUESTEIN };

// How one axis is transformed; passed by value to the kernels.  RADIX2: n = 1 << ns, fft_line in place (rad unused).  MIXED:
// rad[0..ns) with product n.  BLUESTEIN (ns == 0): over the power of two M = 1 << logM >= 2n - 1.  kind and lds (float2 of LDS
// one wavefront needs for one line: n, 2n, M) are for the host's dispatch.  rad[] holds MAXMR = 8 radices, not MAXST: only mixed
// plans read it and none up to MAXP has more than 6 stages (2 * 3^5), and with the two host fields the struct then keeps the
// 56 bytes it had, so bs_filter_kernel's kernarg segment and descriptor stay what they were.
struct LinePlan {
    int n, ns, M, logM;
    int rad[MAXMR];
    int kind, lds;
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

// p.lds on the device, from n / M: with W, H and the pointers these sit in the first 64 bytes of the kernarg segment, so a radix-2
// pass loads no more of it than when it took one integer (p.lds lies in the second cache line: a miss per launch)
template <int KIND>
__device__ __forceinline__ int line_lds(const LinePlan& p) { return KIND == RADIX2 ? p.n : (KIND == MIXED ? 2 * p.n : p.M); }

// Transform of the line at `cur` inside this wavefront's buf[p.lds]; returns where the result is.
template <int KIND>
__device__ __forceinline__ float2* line_fft(float2* buf, float2* cur, const LinePlan& p, float sign, int lane,
                                            const float2* __restrict__ filt) {
    if constexpr (KIND == RADIX2) {
        fft_line(buf, p.n, p.ns, sign, lane);
        return buf;
    } else if constexpr (KIND == BLUESTEIN) {
        bs_line(buf, p, sign, lane, filt);
        return buf;
    } else {
        return mr_line(buf, cur, p, sign, lane);
    }
}

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

// pass 1: forward FFT of every row of res (planes of samples with de_id >= 3 only).  Lines of a block beyond H / W are zero.
template <int KIND>
__global__ __launch_bounds__(256) void ot_rows_fwd_kernel(const float* __restrict__ deg, const float* __restrict__ out,
                                                          const int* __restrict__ de_id, float2* __restrict__ scr, int H,
                                                          int W, LinePlan p, const float2* __restrict__ filt) {
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    const int plane = blockIdx.y, b = plane / 3;
    if (de_id[b] < 3) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * LPB + wave;
    float2* line = sm + wave * line_lds<KIND>(p);
    const long base = ((long)plane * H + row) * W;
    if (row < H)
        for (int i = lane; i < W; i += 64) line[i] = make_float2(deg[base + i] - out[base + i], 0.f);
    else
        for (int i = lane; i < W; i += 64) line[i] = make_float2(0.f, 0.f);
    __syncthreads();
    const float2* r = line_fft<KIND>(line, line, p, -1.f, lane, filt);
    if (row < H)
        for (int i = lane; i < W; i += 64) scr[base + i] = r[i];
}

// pass 2: forward FFT of every column -> |F| (sum into spec[b]) and U = F/|F| -> inverse FFT along the column
template <int KIND>
__global__ __launch_bounds__(256) void ot_cols_kernel(const int* __restrict__ de_id, float2* __restrict__ scr,
                                                      float* __restrict__ spec, int H, int W, LinePlan p,
                                                      const float2* __restrict__ filt) {
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    __shared__ float red[4];
    const int plane = blockIdx.y, b = plane / 3;
    if (de_id[b] < 3) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col = blockIdx.x * LPB + wave;
    float2* line = sm + wave * line_lds<KIND>(p);
    float2* g = scr + (long)plane * H * W + col;
    if (col < W)
        for (int i = lane; i < H; i += 64) line[i] = g[(long)i * W];
    else
        for (int i = lane; i < H; i += 64) line[i] = make_float2(0.f, 0.f);
    __syncthreads();
    float2* f = line_fft<KIND>(line, line, p, -1.f, lane, filt);
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
    const float2* r = line_fft<KIND>(line, f, p, 1.f, lane, filt);
    if (col < W)
        for (int i = lane; i < H; i += 64) g[(long)i * W] = r[i];
}

// pass 3: inverse FFT of every row; gF = Re(.) / (3*H*W)   ( == Re(ifft2(U)) / 3 )
template <int KIND>
__global__ __launch_bounds__(256) void ot_rows_inv_kernel(const int* __restrict__ de_id, const float2* __restrict__ scr,
                                                          float* __restrict__ gF, int H, int W, LinePlan p,
                                                          const float2* __restrict__ filt) {
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    const int plane = blockIdx.y, b = plane / 3;
    if (de_id[b] < 3) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * LPB + wave;
    float2* line = sm + wave * line_lds<KIND>(p);
    const long base = ((long)plane * H + row) * W;
    if (row < H)
        for (int i = lane; i < W; i += 64) line[i] = scr[base + i];
    else
        for (int i = lane; i < W; i += 64) line[i] = make_float2(0.f, 0.f);
    __syncthreads();
    const float2* r = line_fft<KIND>(line, line, p, 1.f, lane, filt);
    const float sc = 1.0f / (3.0f * (float)H * (float)W);
    if (row < H)
        for (int i = lane; i < W; i += 64) gF[base + i] = r[i].x * sc;
}

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

// Host side of a LinePlan: what rcot_fft_plan answers for n.
int make_plan(int n, LinePlan& p) {
    int rad[MAXST];
    const int ns = rcot_fft_plan(n, rad, MAXST);
    if (ns < 0) return ns;
    p.n = n;
    p.ns = ns;
    p.M = p.logM = 0;
    bool two = ns > 0;
    for (int i = 0; i < ns; ++i)
        if (rad[i] != 2) two = false;
    for (int i = 0; i < MAXMR; ++i) p.rad[i] = i < ns ? rad[i] : 1;
    if (ns == 0) {
        p.M = rad[0];
        while ((1 << p.logM) < p.M) ++p.logM;
    }
    p.kind = two ? RADIX2 : (ns > 0 ? MIXED : BLUESTEIN);
    p.lds = two ? n : (ns > 0 ? 2 * n : p.M);
    return RCOT_OK;
}

// The instantiations of the three passes, indexed by LineKind.
#define RCOT_OT_KINDS(k) {k<RADIX2>, k<MIXED>, k<BLUESTEIN>}
constexpr decltype(&ot_rows_fwd_kernel<RADIX2>) k_rows_fwd[3] = RCOT_OT_KINDS(ot_rows_fwd_kernel);
constexpr decltype(&ot_cols_kernel<RADIX2>) k_cols[3] = RCOT_OT_KINDS(ot_cols_kernel);
constexpr decltype(&ot_rows_inv_kernel<RADIX2>) k_rows_inv[3] = RCOT_OT_KINDS(ot_rows_inv_kernel);
#undef RCOT_OT_KINDS
const char* const k_rows_inv_name[3] = {"ot_rows_inv_kernel", "ot_rows_inv_mixed_kernel", "ot_rows_inv_bluestein_kernel"};

// One pass over one axis: the instantiation of plan p's kind, LPB lines of p.lds per block; a... is what the kernel takes before
// (p, filt).
template <typename K, typename... A>
int launch_pass(K* const (&k)[3], dim3 grid, hipStream_t st, const LinePlan& p, const float2* filt, A... a) {
    RCOT_LAUNCH(k[p.kind], grid, dim3(256), sizeof(float2) * LPB * p.lds, st, a..., p, filt);
    RCOT_LAUNCH_CHECK();
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
    int rc = make_plan(W, pw);
    if (rc == RCOT_OK) rc = make_plan(H, ph);
    if (rc != RCOT_OK) return rc;
    // scratch, then the chirp filter of each axis that runs Bluestein
    const size_t n_scr = (size_t)B * 3 * H * W;
    const size_t n_fw = pw.kind == BLUESTEIN ? pw.M : 0, n_fh = ph.kind == BLUESTEIN ? ph.M : 0;
    if (ws_bytes < sizeof(float2) * (n_scr + n_fw + n_fh)) return RCOT_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(spec, 0, sizeof(float) * (size_t)B, st);
    if (e != hipSuccess) return (int)e;
    float2* scr = reinterpret_cast<float2*>(ws);
    float2* fw = scr + n_scr;
    float2* fh = fw + n_fw;
    if (pw.kind != RADIX2 || ph.kind != RADIX2) {
        // LDS per block: 4 lines of 2n (mixed radix, n <= 1000) or M <= 2048 (Bluestein) complex values = up to 64 KiB, plus the
        // columns kernels' 16 static bytes: above the default limit of a launch
        // (a refusal here is not an error of its own: the launch below reports a size it cannot have)
        static const bool raised = [] {
            bool ok = true;
            for (int kind : {MIXED, BLUESTEIN})
                for (const void* k : {(const void*)k_rows_fwd[kind], (const void*)k_cols[kind], (const void*)k_rows_inv[kind]})
                    if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) != hipSuccess) {
                        (void)hipGetLastError();
                        ok = false;
                    }
            return ok;
        }();
        (void)raised;
    }
    if (pw.kind == BLUESTEIN) {
        RCOT_LAUNCH(bs_filter_kernel, dim3(1), dim3(64), sizeof(float2) * pw.M, st, fw, pw);
        RCOT_LAUNCH_CHECK();
    }
    if (ph.kind == BLUESTEIN) {
        RCOT_LAUNCH(bs_filter_kernel, dim3(1), dim3(64), sizeof(float2) * ph.M, st, fh, ph);
        RCOT_LAUNCH_CHECK();
    }
    const dim3 grows(cdiv(H, LPB), B * 3), gcols(cdiv(W, LPB), B * 3);
    rc = launch_pass(k_rows_fwd, grows, st, pw, fw, degraded, restored, de_id, scr, H, W);
    if (rc == RCOT_OK) rc = launch_pass(k_cols, gcols, st, ph, fh, de_id, scr, spec, H, W);
    if (rc != RCOT_OK) return rc;
    note_kernel("%s", k_rows_inv_name[pw.kind]);
    return launch_pass(k_rows_inv, grows, st, pw, fw, de_id, scr, gF, H, W);
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
