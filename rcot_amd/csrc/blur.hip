// Per-image PSF blur on the device (rcot_amd/blur.py; the deblurring tasks blur_<spec> and the "BD" degradation of super-resolution
// tables, sr_bd_x3): a K x K correlation of a uint8 HWC image with arbitrary per-call integer weights, three border rules and an optional
// sampling of the output.  All arithmetic is integer, so the kernels and the numpy restatement of this comment (tests/blur_double.py)
// agree byte for byte.
//
// THE RULE (the only place it is defined).
//   weights      a PSF is q, int32 [K][K], K odd, every q >= 0, sum q = 2^22.  The host makes it from a float64 PSF h (h >= 0, sum h = 1):
//                t = h 2^22, q = floor(t); the remainder 2^22 - sum q (at most K^2) goes as +1 to the taps with the largest fractional
//                parts of t, ties to the lower row-major index (a stable sort).
//   output       a correlation (MATLAB imfilter's orientation, not a flipped convolution).  With r = (K - 1) / 2, per channel,
//                  acc = sum_i sum_j q[i][j] src[by(y + i - r)][bx(x + j - r)],   out = (acc + 2^21) >> 22.
//                acc + 2^21 <= 255 2^22 + 2^21 < 2^31: 32-bit arithmetic never overflows and no clamp is needed.
//   border maps  b(p) for an axis of length n, valid for any distance outside the image, n smaller than r and n = 1 included:
//                  replicate (0)  clamp p to [0, n - 1]                         (imfilter 'replicate', scipy 'nearest')
//                  mirror    (1)  reflection that does not repeat the edge sample: with the period P = 2 (n - 1), m = p mod P,
//                                 b = m < n ? m : P - m; n = 1 maps to 0       (scipy 'mirror', numpy 'reflect', cv2's default)
//                  wrap      (2)  p mod n, the mathematical modulo             (the circular convention of non-blind deblurring)
//   step, phase  dst[oy][ox] is out at (oy step + phase, ox step + phase); dst is [H / step][W / step][3], H and W multiples of step,
//                0 <= phase < step.  step 1, phase 0 is the plain blur; step 3, phase 1 is BD's "every third pixel, the centre of each
//                3 x 3 cell".  Only the sampled outputs are computed.
//
// THE WEIGHT CONTRACT.  The weights are the caller's: rcot_amd/blur.py makes them and checks non-negativity and the sum on the host before
// the upload.  For anything else the kernels still run: a product takes the low 24 bits of its weight (pixel x weight is one 24-bit
// multiply-add), the sum wraps modulo 2^32 and the low 8 bits of (acc + 2^21) >> 22 are stored.  Every image index the kernels form goes
// through a border map, so no PSF can make them read outside the image.
//
// THE KERNELS.  blur_tile_kernel (step 1): the image is taken as H rows of 3 W BYTES — in that view the correlation is the same for
// every channel, tap j sits 3 (j - r) bytes to the side — and one workgroup of four waves owns a tile of TH = 32 rows x TB = 256 bytes
// (85 1/3 pixels; tiles need not start on a pixel).  The tile and its halo of r rows and 3 r bytes are staged once into LDS as bytes with
// the border maps applied (a lane makes the byte offsets of the columns it stages once and keeps them in registers, so the loads of a row
// are in flight together; the row map is made once per row; the result goes out as one word per lane and row where the address allows), so the inner
// loops have no bounds logic.  A lane owns 4 consecutive bytes of 8 rows: 32 accumulators.  Taps are walked in groups of four along a PSF
// row: the 16 bytes (four aligned words; the lanes of a wave read consecutive words: no bank conflict) that four taps of four outputs
// read are loaded once per row and the bytes extracted.  A weight is wave-uniform (scalar loads); a group of four zero weights is skipped
// before its LDS reads and a zero tap before its multiply-adds by uniform branches — a motion PSF has about 2 L non-zeros in L^2.  LDS:
// (31 + K) rows of 260 + 12 ceil(K / 4) bytes, 41.5 KB at K = 63, 10.5 KB at K = 7.
// blur_sample_kernel (step > 1): one thread per output pixel reads its K x K pixels from global memory through the border maps (the
// identity inside the image: the modulo is taken only outside).  The sampled outputs of step >= 2 read disjoint or nearly disjoint
// windows, so a staged tile would be read about once per byte.
#include "../../include/rcot_hip.h"
#include "common.h"

using namespace rcot;

namespace {

constexpr int TH = 32;                                   // rows of a tile
constexpr int TB = 256;                                  // bytes of a tile's row: 4 per lane of a wave
constexpr int RPT = 8;                                   // rows per thread: TH / 4 waves
constexpr int NT = 256;
constexpr int KMAX = 63;
constexpr int CPL = 8;                                   // tile columns a lane stages: ceil(tile_pitch(KMAX) / 64)

__host__ __device__ constexpr int tile_pitch(int K) { return TB + 12 * ((K + 3) / 4) + 4; }     // every byte a lane's words reach
static_assert(tile_pitch(KMAX) <= 64 * CPL, "a lane stages at most CPL columns of a row");

// b(p) of the rule for an axis of length n >= 1
__device__ __forceinline__ int border_map(int p, int n, int border) {
    if ((unsigned)p < (unsigned)n) return p;
    if (border == 0) return p < 0 ? 0 : n - 1;
    if (border == 2) {
        const int m = p % n;
        return m < 0 ? m + n : m;
    }
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    int m = p % period;
    m = m < 0 ? m + period : m;
    return m < n ? m : period - m;
}

__device__ __forceinline__ unsigned byte_of(unsigned d0, unsigned d1, unsigned d2, unsigned d3, int k) {     // k: a constant after unrolling
    const unsigned d = k < 4 ? d0 : k < 8 ? d1 : k < 12 ? d2 : d3;
    return (d >> (8 * (k & 3))) & 0xffu;
}

__global__ __launch_bounds__(NT) void blur_tile_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int H, int W,
                                                        const int* __restrict__ psf, int K, int border, int tiles_x) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int r = (K - 1) >> 1;
    const int pitch = tile_pitch(K);
    const int rows = TH + K - 1;
    unsigned char* tile = lds;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * TH, xb0 = tx * TB;
    const int W3 = 3 * W;

    // a lane stages the tile columns lane, lane + 64, ...: their byte offsets inside a source row, made once and kept in registers, so
    // that the loads of a row are independent and in flight together
    int cm[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const long xb = (long)xb0 - 3 * r + (lane + 64 * k) + 3 * 64;       // + 192: non-negative (r <= 31), so / and % are the floor forms
        const int px = (int)(xb / 3) - 64, ch = (int)(xb % 3);
        cm[k] = 3 * border_map(px, W, border) + ch;
    }
#pragma unroll 2
    for (int rr = wave; rr < rows; rr += 4) {
        const unsigned char* s = src + (long)border_map(y0 - r + rr, H, border) * W3;
        unsigned char* d = tile + rr * pitch;
        unsigned char v[CPL];
#pragma unroll
        for (int k = 0; k < CPL; ++k)
            if (lane + 64 * k < pitch) v[k] = s[cm[k]];
#pragma unroll
        for (int k = 0; k < CPL; ++k)
            if (lane + 64 * k < pitch) d[lane + 64 * k] = v[k];
    }
    __syncthreads();

    unsigned acc[RPT][4];
#pragma unroll
    for (int rr = 0; rr < RPT; ++rr)
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[rr][o] = 0u;
    const unsigned char* mine = tile + (wave * RPT) * pitch + 4 * lane;
    const int groups = (K + 3) >> 2;
#pragma unroll 1
    for (int i = 0; i < K; ++i) {
        const int* qrow = psf + i * K;
#pragma unroll 1
        for (int g = 0; g < groups; ++g) {
            const int j = 4 * g;
            unsigned w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = j + k < K ? (unsigned)qrow[j + k] : 0u;      // uniform: scalar loads
            if ((w[0] | w[1] | w[2] | w[3]) == 0u) continue;
            const unsigned char* p = mine + i * pitch + 12 * g;
            unsigned d[RPT][4];
#pragma unroll
            for (int rr = 0; rr < RPT; ++rr) {
                const unsigned* q = reinterpret_cast<const unsigned*>(p + rr * pitch);
                d[rr][0] = q[0], d[rr][1] = q[1], d[rr][2] = q[2], d[rr][3] = q[3];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (w[k] == 0u) continue;
#pragma unroll
                for (int rr = 0; rr < RPT; ++rr)
#pragma unroll
                    for (int o = 0; o < 4; ++o)
                        acc[rr][o] += __umul24(w[k], byte_of(d[rr][0], d[rr][1], d[rr][2], d[rr][3], o + 3 * k));
            }
        }
    }

    const long xb = (long)xb0 + 4 * lane;              // 3 W may be within a tile of 2^31
#pragma unroll
    for (int rr = 0; rr < RPT; ++rr) {
        const int y = y0 + wave * RPT + rr;
        if (y >= H) break;
        unsigned char* o = dst + (long)y * W3 + xb;
        unsigned v = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) v |= (((acc[rr][k] + (1u << 21)) >> 22) & 0xffu) << (8 * k);
        if (xb + 3 < W3 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {       // one word where the row's address allows
            *reinterpret_cast<unsigned*>(o) = v;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (xb + k < W3) o[k] = (unsigned char)(v >> (8 * k));
        }
    }
}

__global__ __launch_bounds__(NT) void blur_sample_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int H, int W,
                                                          const int* __restrict__ psf, int K, int border, int step, int phase) {
    const int OW = W / step;
    const long n = (long)(H / step) * OW;
    const long e = (long)blockIdx.x * NT + threadIdx.x;
    if (e >= n) return;
    const int oy = (int)(e / OW), ox = (int)(e - (long)oy * OW);
    const int r = (K - 1) >> 1;
    const int y = oy * step + phase - r, x = ox * step + phase - r;
    unsigned a0 = 0u, a1 = 0u, a2 = 0u;
#pragma unroll 1
    for (int i = 0; i < K; ++i) {
        const unsigned char* s = src + (long)border_map(y + i, H, border) * (3 * W);
#pragma unroll 1
        for (int j = 0; j < K; ++j) {
            const unsigned w = (unsigned)psf[i * K + j];     // uniform
            if (w == 0u) continue;
            const unsigned char* p = s + 3 * border_map(x + j, W, border);
            a0 += __umul24(w, p[0]);
            a1 += __umul24(w, p[1]);
            a2 += __umul24(w, p[2]);
        }
    }
    unsigned char* o = dst + e * 3;
    o[0] = (unsigned char)((a0 + (1u << 21)) >> 22);
    o[1] = (unsigned char)((a1 + (1u << 21)) >> 22);
    o[2] = (unsigned char)((a2 + (1u << 21)) >> 22);
}

}  // namespace

extern "C" int rcot_blur_u8(const unsigned char* src, unsigned char* dst, int H, int W, const int* psf, int K, int border, int step,
                            int phase, void* stream) {
    if (!src || !dst || !psf || H < 1 || W < 1 || K < 1 || (K & 1) == 0 || border < 0 || border > 2 || step < 1 || phase < 0 ||
        phase >= step || H % step || W % step)
        return RCOT_EINVAL;
    if (K > KMAX || (long)H * W * 3 >= (1L << 31)) return RCOT_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (step == 1) {
        const int tiles_x = cdiv(3 * W, TB);
        const long tiles = (long)tiles_x * cdiv(H, TH);                       // below 2^31 / (TH TB) + tiles_x + H / TH
        const size_t lds = (size_t)tile_pitch(K) * (TH + K - 1);
        RCOT_LAUNCH(blur_tile_kernel, dim3((unsigned)tiles), dim3(NT), lds, st, src, dst, H, W, psf, K, border, tiles_x);
    } else {
        const long n = (long)(H / step) * (W / step);
        RCOT_LAUNCH(blur_sample_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, st, src, dst, H, W, psf, K, border, step, phase);
    }
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}
