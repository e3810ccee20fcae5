// Standard image-quality figures on the device (rcot_amd/quality.py; the testers' --ssim_window / --color):
//   rcot_image_quality    : two uint8 HWC images -> the sums under PSNR and under the windowed SSIM of the usual protocols
//   rcot_image_blockiness : two uint8 HWC images -> the sums under PSNR-B (the tester's --psnrb), and rcot_crop_u8, the border shave
//                           (--shave): both at the end of this file
//
// Definitions (a, b: uint8 [h][w][3], data range 255)
//   space  0 rgb : the three channels are three planes.
//          1 y   : one plane, the 8-bit BT.601 luma of MATLAB's rgb2ycbcr / basicsr's bgr2ycbcr(y_only) for uint8 input, in integers:
//                  n = 65481 R + 128553 G + 24966 B,  Y = 16 + (n + 127500) / 255000  (floor; round-half-up, 16..235).
//   window 0 uniform7 : 7 taps of 1/7 per axis, cov_norm = 49/48 (skimage's structural_similarity defaults, sample covariance).
//          1 gauss11  : 11 taps exp(-x^2 / (2 1.5^2)), x = -5..5, normalised to sum 1, cov_norm = 1 (cv2.getGaussianKernel(11, 1.5),
//                       basicsr's calculate_ssim, skimage with gaussian_weights=True, use_sample_covariance=False).
//   The window, applied separably to a, b, a^2, b^2, ab, gives ux, uy, uxx, uyy, uxy;  vx = cov_norm (uxx - ux^2), vy and vxy alike;
//   C1 = (0.01 255)^2, C2 = (0.03 255)^2;  S = ((2 ux uy + C1)(2 vxy + C2)) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),
//   evaluated only where the whole window lies inside the image: (h - win + 1)(w - win + 1) positions per plane (skimage's crop by
//   (win - 1) / 2, basicsr's [5:-5]); no border rule is involved.  The metric is sum S / count; an image smaller than the window has
//   sum 0 and count 0.  PSNR = 10 log10(255^2 / mean (a - b)^2) over the planes of the space.
//
// One workgroup per TH x TW tile of one plane.  The rows of both images that the tile's windows reach cross LDS as aligned dwords (the
// 3w-byte rows are unaligned for most widths), the plane (a channel, or the luma) is picked out as integers, then a horizontal and a
// vertical pass of the five moments: integer sums for the uniform window (exact), fp64 for the Gaussian, whose weights the host computes
// and passes by value.  The quotient and the sums are fp64 (the uniform window's numerator and denominator are formed from the integer
// sums, scaled by 49^2 each, so that one division remains); the squared error is a 64-bit integer.  Per-workgroup partials go to the
// caller's workspace and a second one-workgroup launch sums them in a fixed order: bitwise reproducible, no atomics.  gfx950 only.
#include "../../include/rcot_hip.h"
#include "common.h"
#include <cmath>
#include <type_traits>

using namespace rcot;

namespace {

constexpr int TH = 16, TW = 32;                         // map positions of one workgroup (tests/test_quality_gpu.py places images around them)

struct QualityArgs {
    const uint8_t* a;             // [h][w][3]
    const uint8_t* b;
    double* part_s;               // [nblocks]: SSIM map sum
    long long* part_i;            // [nblocks]: squared error
    int h, w, space;
    double wt[11];                // the Gaussian's taps (unused by the uniform window)
};

__device__ __forceinline__ int plane_value(const uint8_t* px, int plane, int space) {
    if (space == 0) return px[plane];
    const int n = 65481 * px[0] + 128553 * px[1] + 24966 * px[2];
    return 16 + (n + 127500) / 255000;
}

// The tile's windows start at (y0, x0) and reach R x C pixels from there; the tile OWNS its first TH x TW pixels for the squared error,
// so every pixel of the image counts once whether or not a window starts at it.
// LDS strides: s_p rows are odd in dwords and s_h rows TW + 1 elements, so that the horizontal pass (a lane per row) reads and writes
// without bank conflicts; the vertical pass (a lane per column) reads consecutive elements.
template <int WINDOW>
__global__ __launch_bounds__(256) void quality_kernel(QualityArgs q) {
    constexpr bool GAUSS = WINDOW == 1;
    constexpr int WIN = GAUSS ? 11 : 7;
    using M = std::conditional_t<GAUSS, double, int>;
    constexpr int R = TH + WIN - 1, C = TW + WIN - 1, CP = C | 1;
    constexpr int LWQ = (3 + 3 * C + 3) / 4 + 1;        // LDS words of one staged row: phase <= 3 + C pixels
    constexpr int NG = TW / 4;                          // groups of four columns in the horizontal pass
    constexpr int NROW = R * LWQ, NST = (NROW + 255) / 256;             // staged words of one image, steps of 256 threads over them
    __shared__ uint32_t s_raw[2][NROW];                 // [image][row][LWQ]: byte k of a row's segment at LDS byte (its address & 3) + k
    __shared__ int s_p[2][R][CP];
    __shared__ M s_h[5][R][TW + 1];
    __shared__ double s_ds[4];
    __shared__ long long s_is[4];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int h = q.h, w = q.w;
    const int y0 = blockIdx.y * TH, x0 = blockIdx.x * TW, plane = blockIdx.z;
    const int nrows = min(R, h - y0), ncols = min(C, w - x0);      // >= 1 by the grid

    // Everything below addresses the images RELATIVE to the tile's first byte, in 32 bits (the host refuses widths at which R rows
    // do not fit): off0 is uniform, row r starts 3 w r bytes on, and its address phase follows from the tile's.
    const int w3 = 3 * w, nc3 = 3 * ncols;
    const long off0 = ((long)y0 * w + x0) * 3, nbytes = (long)h * w3;
    const uint8_t* const tile[2] = {q.a + off0, q.b + off0};
    const int ph0[2] = {(int)(reinterpret_cast<uintptr_t>(tile[0]) & 3), (int)(reinterpret_cast<uintptr_t>(tile[1]) & 3)};

    // Staging: one aligned dword per thread and step, all steps' loads in flight together (no load waits for an earlier one's LDS
    // store).  A dword is loaded whole when it lies inside the image's 3 h w bytes — bytes of it beyond the row segment are never
    // picked — and byte by byte, in a pass that only the workgroups at the two ends of the image enter, where it does not.
    {
        // a dword at relative offset rel is inside the image when lo_rel <= rel <= hi_rel (both uniform, clamped to int)
        const int lo_rel = (int)max(-off0, -8L), hi_rel = (int)min(nbytes - off0 - 4, (long)R * w3 + 8);
        // step s of this thread in image `img`: the relative offset of its dword; false: nothing to stage
        auto locate = [&](int s, int img, int& rel) {
            const int i = t + 256 * s, r = i / LWQ, j = i - r * LWQ;
            const int inrow = 4 * j - ((ph0[img] + r * w3) & 3);                   // relative to the row segment's first byte: > -4
            rel = r * w3 + inrow;
            return i < NROW && r < nrows && inrow < nc3;
        };
        uint32_t v[2][NST];
#pragma unroll
        for (int img = 0; img < 2; ++img)
#pragma unroll
            for (int s = 0; s < NST; ++s) {
                int rel;
                v[img][s] = 0;
                if (locate(s, img, rel) && rel >= lo_rel && rel <= hi_rel) v[img][s] = *reinterpret_cast<const uint32_t*>(tile[img] + rel);
            }
#pragma unroll
        for (int img = 0; img < 2; ++img)
#pragma unroll
            for (int s = 0; s < NST; ++s)
                if (t + 256 * s < NROW) s_raw[img][t + 256 * s] = v[img][s];
        if (lo_rel > -4 || hi_rel < nrows * w3) {                                   // uniform: a dword of this tile may cross an end of the image
#pragma unroll
            for (int img = 0; img < 2; ++img)
#pragma unroll
                for (int s = 0; s < NST; ++s) {
                    int rel;
                    if (locate(s, img, rel) && !(rel >= lo_rel && rel <= hi_rel)) {   // the same thread rewrites its own word
                        uint32_t u = 0;
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (off0 + rel + k >= 0 && off0 + rel + k < nbytes) u |= (uint32_t)tile[img][rel + k] << (8 * k);
                        s_raw[img][t + 256 * s] = u;
                    }
                }
        }
    }
    __syncthreads();

    long long si = 0;
    for (int i = t; i < R * C; i += 256) {
        const int r = i / C, c = i - r * C;
        int va = 0, vb = 0;
        if (r < nrows && c < ncols) {
            const int pa = (ph0[0] + r * w3) & 3, pb = (ph0[1] + r * w3) & 3;
            va = plane_value(reinterpret_cast<const uint8_t*>(s_raw[0] + r * LWQ) + pa + 3 * c, plane, q.space);
            vb = plane_value(reinterpret_cast<const uint8_t*>(s_raw[1] + r * LWQ) + pb + 3 * c, plane, q.space);
            if (r < TH && c < TW) {
                const int d = va - vb;
                si += d * d;
            }
        }
        s_p[0][r][c] = va;
        s_p[1][r][c] = vb;
    }
    __syncthreads();

    // horizontal pass: one staged row and four neighbouring windows per item
    for (int it = t; it < R * NG; it += 256) {
        const int g = it / R, r = it - g * R;
        M acc[4][5];
#pragma unroll
        for (int o = 0; o < 4; ++o)
#pragma unroll
            for (int e = 0; e < 5; ++e) acc[o][e] = 0;
#pragma unroll
        for (int j = 0; j < WIN + 3; ++j) {
            const int va = s_p[0][r][4 * g + j], vb = s_p[1][r][4 * g + j];
            const M m[5] = {(M)va, (M)vb, (M)(va * va), (M)(vb * vb), (M)(va * vb)};
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                const int k = j - o;
                if (k < 0 || k >= WIN) continue;
#pragma unroll
                for (int e = 0; e < 5; ++e) {
                    if constexpr (GAUSS) acc[o][e] = fma(q.wt[k], m[e], acc[o][e]);
                    else acc[o][e] += m[e];
                }
            }
        }
#pragma unroll
        for (int o = 0; o < 4; ++o)
#pragma unroll
            for (int e = 0; e < 5; ++e) s_h[e][r][4 * g + o] = acc[o][e];
    }
    __syncthreads();

    // vertical pass: one column and two neighbouring windows per thread, then the quotient
    double ss = 0.0;
    {
        const int c = t & (TW - 1), i0 = 2 * (t / TW);
        M acc[2][5];
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
            for (int e = 0; e < 5; ++e) acc[o][e] = 0;
#pragma unroll
        for (int k = 0; k < WIN + 1; ++k) {
#pragma unroll
            for (int e = 0; e < 5; ++e) {
                const M m = s_h[e][i0 + k][c];
                if constexpr (GAUSS) {
                    if (k < WIN) acc[0][e] = fma(q.wt[k < WIN ? k : 0], m, acc[0][e]);
                    if (k >= 1) acc[1][e] = fma(q.wt[k >= 1 ? k - 1 : 0], m, acc[1][e]);
                } else {
                    if (k < WIN) acc[0][e] += m;
                    if (k >= 1) acc[1][e] += m;
                }
            }
        }
        constexpr double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            if (y0 + i0 + o > h - WIN || x0 + c > w - WIN) continue;
            if constexpr (GAUSS) {
                const double ux = acc[o][0], uy = acc[o][1];
                const double vx = acc[o][2] - ux * ux, vy = acc[o][3] - uy * uy, vxy = acc[o][4] - ux * uy;
                ss += ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
            } else {
                // u = S / 49 and v = cov_norm (49 Sxx - Sx^2) / 49^2: numerator and denominator of S times 49^4.  The window sums are at
                // most 49 * 255^2, so every integer below is exact in 32 bits (49^2 * 255^2 = 1.6e8), and one division remains
                constexpr double K = 49.0 * 49.0, cov_norm = 49.0 / 48.0;
                const int sa = acc[o][0], sb = acc[o][1];
                const int nx = 49 * acc[o][2] - sa * sa, ny = 49 * acc[o][3] - sb * sb, nxy = 49 * acc[o][4] - sa * sb;
                ss += (((double)(2 * sa * sb) + K * C1) * (2 * cov_norm * (double)nxy + K * C2)) /
                      (((double)(sa * sa + sb * sb) + K * C1) * (cov_norm * (double)(nx + ny) + K * C2));
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ss += __shfl_xor(ss, o, 64);
        si += __shfl_xor(si, o, 64);
    }
    if (lane == 0) {
        s_ds[wave] = ss;
        s_is[wave] = si;
    }
    __syncthreads();
    if (t == 0) {
        const long b = ((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        q.part_s[b] = (s_ds[0] + s_ds[1]) + (s_ds[2] + s_ds[3]);
        q.part_i[b] = s_is[0] + s_is[1] + s_is[2] + s_is[3];
    }
}

// stats[0..4) from the partials, one workgroup, fixed order (final_sums)
__global__ __launch_bounds__(256) void quality_final_kernel(const double* __restrict__ part_s, const long long* __restrict__ part_i, long nb,
                                                            double elements, double positions, double* __restrict__ stats) {
    double d[1];
    long long n;
    final_sums<1>(part_s, part_i, nb, d, n);
    if (threadIdx.x == 0) {
        stats[0] = (double)n;
        stats[1] = elements;
        stats[2] = d[0];
        stats[3] = positions;
    }
}

}  // namespace

extern "C" {

int rcot_image_quality(const unsigned char* a, const unsigned char* b, int h, int w, int window, int space, double* stats, float* ws,
                       size_t ws_bytes, void* stream) {
    if (!a || !b || !stats || !ws || h < 1 || w < 1 || window < 0 || window > 1 || space < 0 || space > 1) return RCOT_EINVAL;
    if (reinterpret_cast<uintptr_t>(stats) & 7) return RCOT_EINVAL;
    const int planes = space == 0 ? 3 : 1, win = window == 0 ? 7 : 11;
    const dim3 grid(cdiv(w, TW), cdiv(h, TH), planes);
    if (grid.y > 65535u || w > (1 << 24)) return RCOT_EINVAL;        // the kernel addresses a tile's rows relative to its first byte, in 32 bits
    const long nb = (long)grid.x * grid.y * grid.z;
    if ((size_t)nb * 16 > ws_bytes || (reinterpret_cast<uintptr_t>(ws) & 7)) return RCOT_EWORKSPACE;
    QualityArgs q;
    q.a = a;
    q.b = b;
    q.part_s = reinterpret_cast<double*>(ws);
    q.part_i = reinterpret_cast<long long*>(ws) + nb;
    q.h = h; q.w = w; q.space = space;
    double sum = 0.0;
    for (int k = 0; k < 11; ++k) {
        q.wt[k] = std::exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5));
        sum += q.wt[k];                                 // in this order: quality.window_weights does the same
    }
    for (int k = 0; k < 11; ++k) q.wt[k] /= sum;
    if (window == 0)
        RCOT_LAUNCH(quality_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, q);
    else
        RCOT_LAUNCH(quality_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, q);
    RCOT_LAUNCH_CHECK();
    const double elements = (double)planes * h * w;
    const double positions = (double)planes * (h >= win ? h - win + 1 : 0) * (w >= win ? w - win + 1 : 0);
    RCOT_LAUNCH(quality_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)q.part_s, (const long long*)q.part_i, nb,
                elements, positions, stats);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------------
// rcot_image_blockiness: the sums under PSNR-B (Yim & Bovik 2011; quality.py's psnrb_from_sums) — per plane the squared error between
// a and b and the squared steps of a between horizontal and vertical neighbours, apart for the pairs that cross a border of the
// 8 x 8 block grid whose origin the caller gives.  Memory-bound: one workgroup takes a BTH x BTW tile of the image with one more row
// below and one more column to the right of a, stages those bytes once as aligned dwords (as quality_kernel does; never a byte outside
// the 3 h w of an image), and then handles the planes of the space in turn: every plane value of a is formed once, by the thread
// that owns the pixel, which takes its right neighbour from the next lane and its lower one through LDS.  Everything is an integer and
// exact; per-workgroup 64-bit partials go to the workspace and one workgroup adds them in a fixed order.  All addresses are 64-bit.
// rcot_crop_u8: a rectangle of an HWC image to a dense buffer, a dword of the destination per thread.
namespace {

constexpr int BTH = 32, BTW = 63;                       // pixels of one workgroup (tests/test_psnrb_gpu.py places images around them):
                                                        // with the halo column a staged row is 64 pixels, one wave

struct BlockinessArgs {
    const uint8_t* a;             // [h][w][3], the image whose steps are measured
    const uint8_t* b;
    long long* part;              // [planes][5][nbp]
    int h, w, space, oy, ox;
};

// Thread (wave, lane) has column `lane` of the staged tile and its rows wave, wave + 4, ...: the right neighbour is the next lane's
// value, the lower one crosses LDS once.  A workgroup's sums stay below 2^31 (2016 pixels x 255^2 = 1.3e8), so they are exact in 32
// bits; the partials and everything after them are 64-bit.
__global__ __launch_bounds__(256) void blockiness_kernel(BlockinessArgs q) {
    constexpr int R = BTH + 1, C = BTW + 1;
    static_assert(C == 64 && BTH % 4 == 0, "a staged row is one wave, the rows go round the four waves");
    constexpr int LW = ((3 + 3 * C + 3) / 4) | 1;       // LDS words of one staged row: phase <= 3 + C pixels (odd: rows on different banks)
    constexpr int NROW = R * LW, NST = (NROW + 255) / 256;
    __shared__ uint32_t s_raw[2][NROW];                 // [image][row][LW]: byte k of a row's segment at LDS byte (its address & 3) + k
    __shared__ int s_pa[R][C];                          // the plane of a
    __shared__ int s_red[4][5];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int h = q.h, w = q.w;
    const int y0 = blockIdx.y * BTH, x0 = blockIdx.x * BTW;
    // a: the tile and its halo; b: the tile alone
    const int nr[2] = {min(R, h - y0), min(BTH, h - y0)};
    const int nb3[2] = {3 * min(C, w - x0), 3 * min(BTW, w - x0)};
    const long w3 = 3L * w, nbytes = (long)h * w3, off0 = ((long)y0 * w + x0) * 3;
    const uintptr_t lo[2] = {reinterpret_cast<uintptr_t>(q.a), reinterpret_cast<uintptr_t>(q.b)};

    // Staging: one aligned dword per thread and step, all loads in flight together.  A dword is loaded whole when it lies inside the
    // image's bytes and byte by byte, in a pass that only the workgroups at the two ends of the image enter, where it does not.
    {
        // step s of this thread in image `img`: the address of its dword; false: nothing to stage
        auto locate = [&](int s, int img, uintptr_t& p) {
            const int i = t + 256 * s, r = i / LW, j = i - r * LW;
            const uintptr_t row = lo[img] + off0 + r * w3;                      // the first byte of the row's segment
            p = (row & ~(uintptr_t)3) + 4 * j;
            return i < NROW && r < nr[img] && p < row + nb3[img];
        };
        auto inside = [&](uintptr_t p, int img) { return p >= lo[img] && p + 4 <= lo[img] + nbytes; };
        uint32_t v[2][NST];
#pragma unroll
        for (int img = 0; img < 2; ++img)
#pragma unroll
            for (int s = 0; s < NST; ++s) {
                uintptr_t p;
                v[img][s] = 0;
                if (locate(s, img, p) && inside(p, img)) v[img][s] = *reinterpret_cast<const uint32_t*>(p);
            }
#pragma unroll
        for (int img = 0; img < 2; ++img)
#pragma unroll
            for (int s = 0; s < NST; ++s)
                if (t + 256 * s < NROW) s_raw[img][t + 256 * s] = v[img][s];
        // uniform: the first dword of the tile may start before the image, the last one of its last row may end behind it
        if (off0 < 4 || off0 + (nr[0] - 1) * w3 + nb3[0] + 3 > nbytes) {
#pragma unroll
            for (int img = 0; img < 2; ++img)
#pragma unroll
                for (int s = 0; s < NST; ++s) {
                    uintptr_t p;
                    if (locate(s, img, p) && !inside(p, img)) {                 // the same thread rewrites its own word
                        uint32_t u = 0;
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (p + k >= lo[img] && p + k < lo[img] + nbytes) u |= (uint32_t)*reinterpret_cast<const uint8_t*>(p + k) << (8 * k);
                        s_raw[img][t + 256 * s] = u;
                    }
                }
        }
    }
    __syncthreads();

    const int planes = q.space == 0 ? 3 : 1;
    const long nbp = (long)gridDim.x * gridDim.y, blk = (long)blockIdx.y * gridDim.x + blockIdx.x;
    const int x = x0 + lane;
    const bool incol = x < w, owned = lane < BTW && incol, hpair = x + 1 < w, hborder = ((x + q.ox) & 7) == 7;
    // byte phase of row r of the staged tile: (phase of the tile's first byte + r 3 w) mod 4
    const int ph[2] = {(int)((lo[0] + off0) & 3), (int)((lo[1] + off0) & 3)}, w3m = (int)(w3 & 3);
    auto pixel = [&](int img, int r) {
        return reinterpret_cast<const uint8_t*>(s_raw[img] + r * LW) + ((ph[img] + r * w3m) & 3) + 3 * lane;
    };
    for (int plane = 0; plane < planes; ++plane) {
        int va[BTH / 4 + 1];
#pragma unroll
        for (int k = 0; k <= BTH / 4; ++k) {
            const int r = wave + 4 * k;                                         // k == BTH / 4: the halo row, wave 0 alone
            va[k] = 0;
            if (r < nr[0] && incol) va[k] = plane_value(pixel(0, r), plane, q.space);
            if (r < R) s_pa[r][lane] = va[k];
        }
        __syncthreads();

        int se = 0, shb = 0, shi = 0, svb = 0, svi = 0;
#pragma unroll
        for (int k = 0; k < BTH / 4; ++k) {
            const int r = wave + 4 * k, y = y0 + r;
            const int right = __shfl_down(va[k], 1, 64);                        // every lane takes part; lane 63 owns nothing
            if (owned && y < h) {
                const int d = va[k] - plane_value(pixel(1, r), plane, q.space);
                se += d * d;
                if (hpair) {
                    const int e = va[k] - right, e2 = e * e;
                    shb += hborder ? e2 : 0;
                    shi += hborder ? 0 : e2;
                }
                if (y + 1 < h) {
                    const int e = va[k] - s_pa[r + 1][lane], e2 = e * e;
                    const bool vborder = ((y + q.oy) & 7) == 7;
                    svb += vborder ? e2 : 0;
                    svi += vborder ? 0 : e2;
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            se += __shfl_xor(se, o, 64);
            shb += __shfl_xor(shb, o, 64);
            shi += __shfl_xor(shi, o, 64);
            svb += __shfl_xor(svb, o, 64);
            svi += __shfl_xor(svi, o, 64);
        }
        if (lane == 0) {
            s_red[wave][0] = se;
            s_red[wave][1] = shb;
            s_red[wave][2] = shi;
            s_red[wave][3] = svb;
            s_red[wave][4] = svi;
        }
        __syncthreads();                                // also: every read of s_pa is behind, the next plane may overwrite it
        if (t < 5) q.part[(plane * 5 + t) * nbp + blk] = (long long)s_red[0][t] + s_red[1][t] + s_red[2][t] + s_red[3][t];
        // (s_red is written again only behind the next plane's first barrier)
    }
}

// stats[planes][5] from the partials, one workgroup: the integer sibling of final_sums (common.h).  Stream s = plane * 5 + k (nbp int64
// values at part[s * nbp ..)) belongs to wave s: strided per-lane sums (the loads of eight steps in flight, the sums in order), then a
// tree over the 64 lanes.  Up to 16 streams.
__global__ __launch_bounds__(1024) void blockiness_final_kernel(const long long* __restrict__ part, long nbp, int nstreams,
                                                                long long* __restrict__ stats) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave >= nstreams) return;
    const long long* __restrict__ p = part + wave * nbp;
    long long n = 0;
#pragma unroll 8
    for (long b = lane; b < nbp; b += 64) n += p[b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) stats[wave] = n;
}

// dword i of the destination's aligned cover: destination bytes 4 i - pad .. 4 i - pad + 3 (pad = dst & 3), whole when all four exist
__global__ __launch_bounds__(256) void crop_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long w3, long off0,
                                                      long wc3, long n, int pad, long nq) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < nq; i += gridDim.x * 256L) {
        const long d0 = 4 * i - pad, first = d0 < 0 ? 0 : d0;
        long row = first / wc3, col = first - row * wc3;
        uint32_t u = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long d = d0 + k;
            if (d < first || d >= n) continue;
            u |= (uint32_t)src[off0 + row * w3 + col] << (8 * k);
            if (++col == wc3) {
                col = 0;
                ++row;
            }
        }
        if (d0 >= 0 && d0 + 4 <= n) {
            *reinterpret_cast<uint32_t*>(dst + d0) = u;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (d0 + k >= 0 && d0 + k < n) dst[d0 + k] = (uint8_t)(u >> (8 * k));
        }
    }
}

}  // namespace

extern "C" {

int rcot_image_blockiness(const unsigned char* a, const unsigned char* b, int h, int w, int space, int oy, int ox, long long* stats,
                          float* ws, size_t ws_bytes, void* stream) {
    if (!a || !b || !stats || !ws || h < 1 || w < 1 || space < 0 || space > 1 || oy < 0 || oy > 7 || ox < 0 || ox > 7) return RCOT_EINVAL;
    if (reinterpret_cast<uintptr_t>(stats) & 7) return RCOT_EINVAL;
    const int planes = space == 0 ? 3 : 1;
    const dim3 grid(cdiv(w, BTW), cdiv(h, BTH));
    if (grid.y > 65535u) return RCOT_EINVAL;
    const long nbp = (long)grid.x * grid.y;
    if ((size_t)nbp * planes * 40 > ws_bytes || (reinterpret_cast<uintptr_t>(ws) & 7)) return RCOT_EWORKSPACE;
    BlockinessArgs q;
    q.a = a;
    q.b = b;
    q.part = reinterpret_cast<long long*>(ws);
    q.h = h; q.w = w; q.space = space; q.oy = oy; q.ox = ox;
    RCOT_LAUNCH(blockiness_kernel, grid, dim3(256), 0, (hipStream_t)stream, q);
    RCOT_LAUNCH_CHECK();
    RCOT_LAUNCH(blockiness_final_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const long long*)q.part, nbp, planes * 5, stats);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

int rcot_crop_u8(const unsigned char* src, int h, int w, int y0, int x0, int hc, int wc, unsigned char* dst, void* stream) {
    if (!src || !dst || h < 1 || w < 1 || y0 < 0 || x0 < 0 || hc < 1 || wc < 1 || hc > h - y0 || wc > w - x0) return RCOT_EINVAL;
    const long wc3 = 3L * wc, n = hc * wc3;
    const int pad = (int)(reinterpret_cast<uintptr_t>(dst) & 3);
    const long nq = (pad + n + 3) / 4;
    RCOT_LAUNCH(crop_u8_kernel, dim3(grid_for(nq)), dim3(256), 0, (hipStream_t)stream, src, dst, 3L * w, ((long)y0 * w + x0) * 3, wc3, n, pad,
                nq);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

}  // extern "C"
