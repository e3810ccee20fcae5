// MATLAB-rule bicubic resize, one axis per launch (rcot_amd/resize.py; the super-resolution task: DIV2K LR images "undergo bicubic
// rescaling to match the dimensions of their respective high-resolution counterparts", the reference's README).
//
// THE RULE (imresize(..., 'bicubic') with antialiasing; the only place it is defined — resize.py builds the tables from it).
// For one axis of input length n and output length m, scale s = m / n:
//   kernel        c(x) = 1.5|x|^3 - 2.5|x|^2 + 1 for |x| <= 1,  -0.5|x|^3 + 2.5|x|^2 - 4|x| + 2 for 1 < |x| <= 2,  else 0
//   kernel width  kw = 4 for s >= 1;  for s < 1 (antialiasing) kw = 4 / s and the kernel becomes s c(s x)
//   output sample o = 1..m sits at input coordinate u = o / s + 0.5 (1 - 1 / s)          (1-based pixel centres)
//   taps          K = ceil(kw) + 2, at input pixels floor(u - kw / 2) - 1 + k, k = 0..K-1 (0-based)
//   weights       the kernel at u - pixel - 1, in fp64, divided by their row sum, then rounded to fp32; zero-weight taps stay
//   border        out-of-range pixels are mirrored symmetrically: index i reads j = i mod 2n (mathematical modulus), and
//                 2n - 1 - j when j >= n  (-1 -> 0, n -> n - 1)
// For an image the axis with the smaller scale goes first, rows first on a tie.  (The reference's util/imresize.py follows this
// rule except along the top and left borders: DESIGN.md section 5.)
//
// The host evaluates the rule into two tables per (n, m): idx[m][K] (already mirrored) and taps[m][K].  The kernel applies them:
//   acc = 0;  for k ascending: acc = acc + taps[o][k] * src[idx[o][k]]       every product and every sum rounded to fp32
// so a numpy fp32 restatement matches bit for bit.  Every index is clamped into [0, n - 1] before it is used.  No atomics, no workspace.
//
// Both forms are HBM-bound.  axis 0 (rows): one workgroup per output row and 256-lane column segment; the K source rows are read
// with coalesced loads (float4 where W and the pointers allow), idx / taps of the row are wave-uniform; every XCD works on a contiguous
// run of output rows.  axis 1 (columns): one
// workgroup owns 256 consecutive outputs of a band of image rows; a lane keeps the K taps of its output in registers, the span of the
// source row the 256 outputs read is staged in LDS with coalesced loads (several rows per barrier), and the taps read LDS —
// neighbouring outputs are s or 1/s source pixels apart, so the reads from global memory would be strided or repeated.  The LDS
// image is skewed by one word per 32 (element j at j + j / 32): lanes 2, 4 or 8 source pixels apart (x2, x4, x8 shrink) would
// otherwise share banks 2-, 4- or 8-fold.  A tile whose span does not fit (a table that is not a resampling table) reads global memory.
#include "../../include/rcot_hip.h"
#include "common.h"

using namespace rcot;

namespace {

constexpr int KMAX = 64;                                // largest tap count (x8 shrink needs 34)
constexpr int TO = 256;                                 // outputs of one workgroup of the column form = its threads
constexpr int SPAN_MAX = 8192;                          // source pixels of one LDS image (all staged rows together)
constexpr int LDS_WORDS = SPAN_MAX + SPAN_MAX / 32 + 1;
constexpr int ROWS_PER_WG = 32;                         // image rows one workgroup of the column form walks, at most

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }
__device__ __forceinline__ int skew(int j) { return j + (j >> 5); }

// ------------------------------------------------------------------ axis 0: dst[p][o][x] = sum_k taps[o][k] src[p][idx[o][k]][x]
// V = 4: W % 4 == 0 and both pointers 16-byte aligned.  Work item w = r * gx + (column segment), r = plane * out_len + o.  The grid is
// one-dimensional with a multiple of 8 workgroups, and workgroup b takes item (b % 8) * (grid / 8) + b / 8: consecutive workgroups go to
// the 8 XCDs in turn, so this hands every XCD a contiguous run of output rows — neighbouring output rows share K - 1/s of their K source
// rows, which then hit that XCD's L2 (dealt out row by row, every XCD pulls the whole source through the Infinity Cache;
// profiles/resize_passes.txt has both forms).
template <int V>
__global__ __launch_bounds__(256) void resize_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, long rows_out, int H, int W,
                                                          int out_len, const int* __restrict__ idx, const float* __restrict__ taps, int K,
                                                          int gx) {
#pragma clang fp contract(off)
    const long total = rows_out * gx;
    const long first = (long)(blockIdx.x % 8) * (gridDim.x / 8) + blockIdx.x / 8;
    for (long w = first; w < total; w += gridDim.x) {               // uniform over the workgroup
        const long r = w / gx;
        const int x = ((int)(w - r * gx) * 256 + threadIdx.x) * V;
        if (x >= W) continue;
        const long plane = r / out_len;
        const int o = (int)(r - plane * out_len);
        const float* s = src + plane * H * (long)W + x;
        const int* ix = idx + (long)o * K;
        const float* tp = taps + (long)o * K;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};             // V == 1 uses the first
#pragma unroll 6                                         // six rows in flight (K = 6, 18 whole; 10, 14 with a short tail)
        for (int k = 0; k < K; ++k) {
            const float t = tp[k];
            const float* row = s + (long)clampi(ix[k], H - 1) * W;
            if (V == 4) {
                const float4 q = *reinterpret_cast<const float4*>(row);
                acc[0] = acc[0] + t * q.x;
                acc[1] = acc[1] + t * q.y;
                acc[2] = acc[2] + t * q.z;
                acc[3] = acc[3] + t * q.w;
            } else {
                acc[0] = acc[0] + t * row[0];
            }
        }
        float* d = dst + r * W + x;
        if (V == 4)
            *reinterpret_cast<float4*>(d) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        else
            d[0] = acc[0];
    }
}

// ------------------------------------------------------------------ axis 1: dst[row][o] = sum_k taps[o][k] src[row][idx[o][k]]
// rows = planes * H image rows of W floats.  KT >= K: the taps a lane keeps in registers.
template <int KT>
__global__ __launch_bounds__(TO) void resize_cols_kernel(const float* __restrict__ src, float* __restrict__ dst, long rows, int W, int out_len,
                                                         const int* __restrict__ idx, const float* __restrict__ taps, int K, int rpw) {
#pragma clang fp contract(off)
    __shared__ float sm[LDS_WORDS];
    __shared__ int s_lo[TO / WAVE], s_hi[TO / WAVE];
    const int t = threadIdx.x;
    const int o = blockIdx.x * TO + t;
    const bool live = o < out_len;
    int ix[KT];
    float tp[KT];
    int lo = W - 1, hi = 0;
    // slots k >= K repeat tap K - 1 and dead lanes the last output (no branch per tap; a select drops them from the sum below)
    const long orow = (long)min(o, out_len - 1) * K;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        const int kk = min(k, K - 1);
        ix[k] = clampi(idx[orow + kk], W - 1);
        tp[k] = taps[orow + kk];
        lo = min(lo, ix[k]);
        hi = max(hi, ix[k]);
    }
    // the span [lo, hi] of source columns the tile reads
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        lo = min(lo, __shfl_xor(lo, m, 64));
        hi = max(hi, __shfl_xor(hi, m, 64));
    }
    if ((t & 63) == 0) {
        s_lo[t >> 6] = lo;
        s_hi[t >> 6] = hi;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < TO / WAVE; ++w) {
        lo = min(lo, s_lo[w]);
        hi = max(hi, s_hi[w]);
    }
    const int span = hi - lo + 1;                        // 1 .. W
    const bool staged = span <= SPAN_MAX;
    const int pitch = skew(span - 1) + 1;                // LDS words of one staged row
    const int nst = staged ? min(rpw, SPAN_MAX / span) : 1;             // rows per barrier pair
    if (staged) {
#pragma unroll
        for (int k = 0; k < KT; ++k) ix[k] = skew(ix[k] - lo);
    }
    const long nchunk = (rows + rpw - 1) / rpw;          // rpw image rows per workgroup (<= ROWS_PER_WG; the host sizes the grid with it)
    for (long c = blockIdx.y; c < nchunk; c += gridDim.y) {
        const long r0 = c * rpw;
        const int nr = (int)min((long)rpw, rows - r0);
        if (!staged) {
#pragma unroll 1
            for (int rr = 0; rr < nr; ++rr) {
                const float* s = src + (r0 + rr) * W;
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < KT; ++k) {
                    const float a = acc + tp[k] * s[ix[k]];
                    acc = k < K ? a : acc;
                }
                if (live) dst[(r0 + rr) * out_len + o] = acc;
            }
            continue;
        }
        for (int b = 0; b < nr; b += nst) {
            const int nb = min(nst, nr - b);
            __syncthreads();                             // the previous image has been read
            // all nb rows as one list of nb * span pixels: every lane loads, several loads in flight (row by row, a 70-pixel span keeps
            // 70 of 256 lanes busy and the rows' load latencies follow one another)
            const float* s = src + (r0 + b) * W + lo;
            const int n = nb * span;
#pragma unroll 4
            for (int e = t; e < n; e += TO) {
                const int rr = e / span, j = e - rr * span;
                sm[rr * pitch + skew(j)] = s[(long)rr * W + j];
            }
            __syncthreads();
#pragma unroll 1
            for (int rr = 0; rr < nb; ++rr) {
                const float* l = sm + rr * pitch;
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < KT; ++k) {
                    const float a = acc + tp[k] * l[ix[k]];
                    acc = k < K ? a : acc;
                }
                if (live) dst[(r0 + b + rr) * out_len + o] = acc;
            }
        }
    }
}

template <int KT>
void launch_cols(const float* src, float* dst, long rows, int W, int out_len, const int* idx, const float* taps, int K, hipStream_t st) {
    // rows per workgroup: as many as leave about 2048 workgroups (4 .. ROWS_PER_WG: a workgroup loads its 256 x K table once)
    const long tiles = cdiv(out_len, TO);
    long rpw = rows * tiles / 2048;
    rpw = rpw < 4 ? 4 : rpw > ROWS_PER_WG ? ROWS_PER_WG : rpw;
    const long nchunk = (rows + rpw - 1) / rpw;
    const dim3 grid((unsigned)tiles, (unsigned)(nchunk > 65535 ? 65535 : nchunk));
    RCOT_LAUNCH(resize_cols_kernel<KT>, grid, dim3(TO), 0, st, src, dst, rows, W, out_len, idx, taps, K, (int)rpw);
}

}  // namespace

extern "C" int rcot_resize_axis(const float* src, float* dst, long planes, int H, int W, int axis, int out_len, const int* idx,
                                const float* taps, int K, void* stream) {
    if (!src || !dst || !idx || !taps || planes < 1 || H < 1 || W < 1 || out_len < 1 || K < 1 || (axis != 0 && axis != 1)) return RCOT_EINVAL;
    if (K > KMAX) return RCOT_EUNSUPPORTED;
    const long in_plane = (long)H * W, out_plane = axis == 0 ? (long)out_len * W : (long)H * out_len;
    if (in_plane > 0x7fffffffL || out_plane > 0x7fffffffL) return RCOT_EUNSUPPORTED;
    if (planes > 0x7fffffffffffffffL / (in_plane > out_plane ? in_plane : out_plane)) return RCOT_EUNSUPPORTED;   // element offsets stay in a long
    hipStream_t st = (hipStream_t)stream;
    if (axis == 0) {
        const long rows_out = planes * out_len;
        const bool vec = (W & 3) == 0 && al16(src) && al16(dst);
        const int gx = cdiv(W, vec ? 1024 : 256);
        long g = rows_out * gx;                          // work items; the grid: at most 2^22 workgroups, a multiple of 8 (the XCDs)
        g = ((g > (1L << 22) ? (1L << 22) : g) + 7) / 8 * 8;
        if (vec)
            RCOT_LAUNCH(resize_rows_kernel<4>, dim3((unsigned)g), dim3(256), 0, st, src, dst, rows_out, H, W, out_len, idx, taps, K, gx);
        else
            RCOT_LAUNCH(resize_rows_kernel<1>, dim3((unsigned)g), dim3(256), 0, st, src, dst, rows_out, H, W, out_len, idx, taps, K, gx);
    } else {
        const long rows = planes * H;
        if (K <= 8)
            launch_cols<8>(src, dst, rows, W, out_len, idx, taps, K, st);
        else if (K <= 20)
            launch_cols<20>(src, dst, rows, W, out_len, idx, taps, K, st);
        else
            launch_cols<KMAX>(src, dst, rows, W, out_len, idx, taps, K, st);
    }
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}
