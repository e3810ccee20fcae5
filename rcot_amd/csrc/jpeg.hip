// Baseline JPEG round trip on the device (rcot_amd/jpeg.py; the compression-artifact task: the degraded image is the clean one saved as a
// JPEG of quality Q and loaded again).  Entropy coding is lossless, so no bitstream is made: the image goes through colour conversion,
// chroma subsampling, the integer DCT, quantisation and their inverses.  The result equals, byte for byte, what Pillow on libjpeg-turbo
// holds after Image.open(BytesIO(<saved with quality=Q, subsampling=S>)) — that codec is the source of truth (tests/test_jpeg_cpu.py
// compares the numpy restatement of this comment, tests/jpeg_double.py, with it; tests/test_jpeg_gpu.py the kernel with the restatement).
//
// THE RULE (libjpeg's baseline path with the "islow" DCT; the only place it is defined).  >> is an arithmetic shift,
// D(x, n) = (x + (1 << (n - 1))) >> n, FIX(x) = int(x * 65536 + 0.5).  Every intermediate fits 32 bits.
//   tables       the Annex K luminance / chrominance tables, scale s = 5000 / Q (integer division) for Q < 50, else 200 - 2 Q;
//                entry q = clamp((base * s + 50) / 100, 1, 255)
//   RGB -> YCbCr Y  = ( FIX(.299) R + FIX(.587) G + FIX(.114) B + 32768) >> 16
//                Cb = (-FIX(.16874) R - FIX(.33126) G + FIX(.5) B + (128 << 16) + 32767) >> 16
//                Cr = ( FIX(.5) R - FIX(.41869) G - FIX(.08131) B + (128 << 16) + 32767) >> 16
//   4:4:4        every plane is padded by edge replication to multiples of 8
//   4:2:0        Y is padded by replication to multiples of 16.  Chroma at full resolution is padded by replication to an even height and
//                a width that is a multiple of 16, then averaged 2 x 2 as (a + b + c + d + bias) >> 2, bias 1 on even output columns and
//                2 on odd ones; the DOWNSAMPLED plane is then padded by replicating its last row to a multiple of 8 rows
//   forward DCT  on samples - 128, rows first.  With t0..t3 = d0 + d7, d1 + d6, d2 + d5, d3 + d4 and t7..t4 = d0 - d7, d1 - d6, d2 - d5,
//                d3 - d4;  t10, t13 = t0 +- t3;  t11, t12 = t1 +- t2:
//                  out0, out4 = (t10 +- t11) << 2 in the row pass, D(t10 +- t11, 2) in the column pass
//                  z = (t12 + t13) 4433;  out2 = D(z + 6270 t13, n);  out6 = D(z - 15137 t12, n)       n = 11 (rows), 15 (columns)
//                  z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7, z5 = 9633 (z3 + z4);  z3 = z5 - 16069 z3, z4 = z5 - 3196 z4
//                  out7 = D(2446 t4 - 7373 z1 + z3, n);  out5 = D(16819 t5 - 20995 z2 + z4, n)
//                  out3 = D(25172 t6 - 20995 z2 + z3, n);  out1 = D(12299 t7 - 7373 z1 + z4, n)
//                the coefficients come out scaled by 8
//   quantise     with d = 8 q:  sign(c) ((|c| + (d >> 1)) / d);  dequantise: times q
//   inverse DCT  columns first with n = 11, then rows with n = 18:
//                  z = (c2 + c6) 4433;  t2 = z - 15137 c6;  t3 = z + 6270 c2;  t0, t1 = (c0 +- c4) << 13
//                  t10, t13 = t0 +- t3;  t11, t12 = t1 +- t2
//                  a0..a3 = c7, c5, c3, c1;  z1 = a0 + a3, z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3, z5 = 9633 (z3 + z4)
//                  z3 = z5 - 16069 z3, z4 = z5 - 3196 z4
//                  a0 = 2446 a0 - 7373 z1 + z3;  a1 = 16819 a1 - 20995 z2 + z4;  a2 = 25172 a2 - 20995 z2 + z3;  a3 = 12299 a3 - 7373 z1 + z4
//                  out0, out7 = D(t10 +- a3, n);  out1, out6 = D(t11 +- a2, n);  out2, out5 = D(t12 +- a1, n);  out3, out4 = D(t13 +- a0, n)
//                the result has 128 added and is clamped to 0 .. 255
//   upsampling   (4:2:0) the decoded chroma is cropped to ceil(H / 2) x ceil(W / 2) and enlarged by the triangle filter: the vertical
//                sum is v = 3 row + neighbour, the neighbour the row above for even output rows and the row below for odd ones,
//                replicated at the top and bottom of the CROPPED plane; even output columns are (3 v + v_last + 8) >> 4, odd ones
//                (3 v + v_next + 7) >> 4, the neighbour replicated at both ends; the result is cropped to H x W.  (A codec uses another
//                rule when the chroma plane is 2 samples wide or less: W <= 4 is refused.)
//   YCbCr -> RGB with cb, cr taken - 128:  R = Y + ((FIX(1.402) cr + 32768) >> 16);  B = Y + ((FIX(1.772) cb + 32768) >> 16);
//                G = Y + ((-FIX(.34414) cb + 32768 - FIX(.71414) cr) >> 16);  each clamped to 0 .. 255
//
// THE KERNELS.  32-bit integer arithmetic only.  roundtrip_kernel<S>: one workgroup of three waves owns a tile of 64 columns x 8 rows
// (4:4:4) or 16 rows (4:2:0) = 24 blocks of 8 x 8.  The RGB bytes of the tile's rows are read as coalesced bytes of whole row segments
// (indices clamped to the image: the edge replication) into LDS, converted there into three sample planes of 8 rows x 64 columns —
// Y, Cb, Cr for 4:4:4; Y rows 0..7, Y rows 8..15 and (Cb | Cr, 32 columns each, averaged 2 x 2) for 4:2:0 — and wave w transforms
// plane w: a lane holds one row of one of the wave's 8 blocks, the transposes between the row and column passes go through an LDS
// image of 9-word rows and 72-word blocks (no bank conflict for the 32 lanes of a half wave, writing or reading).  The division of the
// quantiser is a multiplication by m = 2^32 / d + 1 (high word; exact for |c| + d / 2 < 2^21, the coefficients stay below 2^16).  The
// tables travel by value.  4:4:4 finishes in the same launch: the decoded planes go back to LDS and every thread writes one byte of
// each row's RGB segment.  4:2:0 writes the decoded planes to the workspace (tile-aligned pitches: no bounds inside the planes) and
// upsample_kernel, the second launch, enlarges the chroma (it needs one sample of halo from the neighbouring tiles), converts and
// writes RGB through an LDS row segment so that the stores are coalesced bytes.
#include "../../include/rcot_hip.h"
#include "common.h"

using namespace rcot;

namespace {

constexpr int TW = 64;                                   // tile width in pixels
constexpr int NT = 192;                                  // threads of a workgroup of roundtrip_kernel = the bytes of a tile's RGB row
constexpr int PP = 72;                                   // bytes of one row of a sample plane in LDS (64 + one 8-byte access)
constexpr int TB = 72;                                   // words of one block in the transpose image (8 rows of 9)

struct Tables {
    unsigned q[128];                                     // divisors, natural order: luminance, then chrominance
    unsigned m[128];                                     // 2^32 / (8 q) + 1
};

const unsigned char kLumaBase[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                     69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                                     81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const unsigned char kChromaBase[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                       99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                       99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

Tables make_tables(int quality) {
    Tables t;
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int k = 0; k < 128; ++k) {
        const int base = k < 64 ? kLumaBase[k] : kChromaBase[k - 64];
        int q = (base * s + 50) / 100;
        q = q < 1 ? 1 : q > 255 ? 255 : q;
        t.q[k] = (unsigned)q;
        t.m[k] = (unsigned)((1ull << 32) / (unsigned)(8 * q)) + 1u;
    }
    return t;
}

__device__ __forceinline__ int dsc(int x, int n) { return (x + (1 << (n - 1))) >> n; }
__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

__device__ __forceinline__ int ycc_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ __forceinline__ int ycc_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
__device__ __forceinline__ int ycc_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }
// channel c (0 R, 1 G, 2 B) of a decoded pixel
__device__ __forceinline__ int rgb_channel(int c, int y, int cb, int cr) {
    cb -= 128;
    cr -= 128;
    const int v = c == 0 ? (91881 * cr + 32768) >> 16 : c == 2 ? (116130 * cb + 32768) >> 16 : (-22554 * cb + 32768 - 46802 * cr) >> 16;
    return clamp255(y + v);
}

template <bool FIRST>
__device__ __forceinline__ void fdct8(int (&d)[8]) {
    constexpr int n = FIRST ? 11 : 15;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = FIRST ? (t10 + t11) << 2 : dsc(t10 + t11, 2);
    d[4] = FIRST ? (t10 - t11) << 2 : dsc(t10 - t11, 2);
    const int z = (t12 + t13) * 4433;
    d[2] = dsc(z + t13 * 6270, n);
    d[6] = dsc(z - t12 * 15137, n);
    const int z1 = (t4 + t7) * -7373, z2 = (t5 + t6) * -20995;
    const int z5 = (t4 + t6 + t5 + t7) * 9633;
    const int z3 = (t4 + t6) * -16069 + z5, z4 = (t5 + t7) * -3196 + z5;
    d[7] = dsc(t4 * 2446 + z1 + z3, n);
    d[5] = dsc(t5 * 16819 + z2 + z4, n);
    d[3] = dsc(t6 * 25172 + z2 + z3, n);
    d[1] = dsc(t7 * 12299 + z1 + z4, n);
}

template <int N>
__device__ __forceinline__ void idct8(int (&c)[8]) {
    const int z = (c[2] + c[6]) * 4433;
    const int t2 = z - c[6] * 15137, t3 = z + c[2] * 6270;
    const int t0 = (c[0] + c[4]) << 13, t1 = (c[0] - c[4]) << 13;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int a0 = c[7], a1 = c[5], a2 = c[3], a3 = c[1];
    const int z1 = (a0 + a3) * -7373, z2 = (a1 + a2) * -20995;
    const int z5 = (a0 + a2 + a1 + a3) * 9633;
    const int z3 = (a0 + a2) * -16069 + z5, z4 = (a1 + a3) * -3196 + z5;
    a0 = a0 * 2446 + z1 + z3;
    a1 = a1 * 16819 + z2 + z4;
    a2 = a2 * 25172 + z2 + z3;
    a3 = a3 * 12299 + z1 + z4;
    c[0] = dsc(t10 + a3, N);
    c[7] = dsc(t10 - a3, N);
    c[1] = dsc(t11 + a2, N);
    c[6] = dsc(t11 - a2, N);
    c[2] = dsc(t12 + a1, N);
    c[5] = dsc(t12 - a1, N);
    c[3] = dsc(t13 + a0, N);
    c[4] = dsc(t13 - a0, N);
}

// 8 x 8 transpose inside each of the wave's 8 blocks: lane (block b, index j) hands in element k of its row / column j and gets
// element j of row / column k.  tw: the wave's image.  The barriers are uniform over the workgroup.
__device__ __forceinline__ void transpose8(int* tw, int b, int j, int (&v)[8]) {
    __syncthreads();                                     // the image's previous use is over
#pragma unroll
    for (int k = 0; k < 8; ++k) tw[b * TB + j * 9 + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = tw[b * TB + k * 9 + j];
}

// S = 0: 4:4:4, one launch, writes dst.  S = 2: 4:2:0, writes the decoded planes: wy [tiles_y * 16][tiles_x * 64], wcb and wcr
// [tiles_y * 8][tiles_x * 32].
template <int S>
__global__ __launch_bounds__(NT) void roundtrip_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int H, int W,
                                                       int tiles_x, const Tables tab, unsigned char* __restrict__ wy,
                                                       unsigned char* __restrict__ wcb, unsigned char* __restrict__ wcr) {
    constexpr int TH = S == 2 ? 16 : 8;                  // tile rows
    __shared__ unsigned char rgb[TH * NT];               // the tile's RGB rows
    __shared__ __attribute__((aligned(16))) unsigned char plane[3][8 * PP];
    __shared__ unsigned sq[128], sm[128];
    __shared__ int timg[3][8 * TB];
    const int t = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * TH, x0 = tx * TW;

    if (t < 128) {
        sq[t] = tab.q[t];
        sm[t] = tab.m[t];
    }
    {   // byte t of every row of the tile: pixel t / 3, channel t % 3, both indices clamped into the image
        const int px = t / 3, c = t - 3 * px;
        const long col = (long)min(x0 + px, W - 1) * 3 + c;
#pragma unroll
        for (int r = 0; r < TH; ++r) rgb[r * NT + t] = src[(long)min(y0 + r, H - 1) * W * 3 + col];
    }
    __syncthreads();
    if (S == 0) {
        for (int p = t; p < 8 * TW; p += NT) {
            const int r = p >> 6, px = p & 63;
            const unsigned char* s = rgb + r * NT + 3 * px;
            const int R = s[0], G = s[1], B = s[2];
            plane[0][r * PP + px] = (unsigned char)ycc_y(R, G, B);
            plane[1][r * PP + px] = (unsigned char)ycc_cb(R, G, B);
            plane[2][r * PP + px] = (unsigned char)ycc_cr(R, G, B);
        }
    } else {
        for (int p = t; p < 16 * TW; p += NT) {
            const int r = p >> 6, px = p & 63;
            const unsigned char* s = rgb + r * NT + 3 * px;
            plane[r >> 3][(r & 7) * PP + px] = (unsigned char)ycc_y(s[0], s[1], s[2]);
        }
        const int hc = (H + 1) >> 1;
        for (int p = t; p < 2 * 8 * 32; p += NT) {       // Cb samples, then Cr samples, of 8 chroma rows x 32 columns
            const int which = p >> 8, i = (p >> 5) & 7, cx = p & 31;
            // chroma rows below the cropped plane repeat its last row (the tile that holds a real row holds that one too)
            const int r0 = 2 * min(y0 / 2 + i, hc - 1) - y0, r1 = r0 + 1;            // 0 .. 15: row r of the tile is image row min(y0 + r, H - 1)
            int sum = 1 + (cx & 1);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned char* s = rgb + ((k & 2) ? r1 : r0) * NT + 3 * (2 * cx + (k & 1));
                sum += which ? ycc_cr(s[0], s[1], s[2]) : ycc_cb(s[0], s[1], s[2]);
            }
            plane[2][i * PP + which * 32 + cx] = (unsigned char)(sum >> 2);
        }
    }
    __syncthreads();

    // wave w transforms plane w: lane = (block b of 8 across, row j)
    const int w = t >> 6, b = (t >> 3) & 7, j = t & 7;
    const bool luma = S == 2 ? w < 2 : w == 0;
    const unsigned* q = sq + (luma ? 0 : 64);
    const unsigned* m = sm + (luma ? 0 : 64);
    int v[8];
    {
        const uint2 raw = *reinterpret_cast<const uint2*>(&plane[w][j * PP + b * 8]);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = (int)(((k < 4 ? raw.x : raw.y) >> (8 * (k & 3))) & 255u) - 128;
    }
    fdct8<true>(v);
    transpose8(timg[w], b, j, v);                        // now: column j of the block, v[k] in row k
    fdct8<false>(v);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const unsigned qq = q[k * 8 + j];
        const unsigned n = (unsigned)abs(v[k]) + 4u * qq;
        const int lev = (int)__umulhi(n, m[k * 8 + j]);
        v[k] = (v[k] < 0 ? -lev : lev) * (int)qq;
    }
    idct8<11>(v);
    transpose8(timg[w], b, j, v);                        // now: row j of the block
    idct8<18>(v);
    uint2 pk = make_uint2(0u, 0u);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const unsigned byte = (unsigned)clamp255(v[k] + 128);
        if (k < 4)
            pk.x |= byte << (8 * k);
        else
            pk.y |= byte << (8 * (k - 4));
    }
    if (S == 2) {
        // the planes are whole tiles wide and high: every store is inside them
        if (w < 2) {
            const long pitch = (long)tiles_x * TW;
            *reinterpret_cast<uint2*>(wy + ((long)y0 + w * 8 + j) * pitch + x0 + b * 8) = pk;
        } else {
            const long pitch = (long)tiles_x * (TW / 2);
            unsigned char* pl = b < 4 ? wcb : wcr;
            *reinterpret_cast<uint2*>(pl + ((long)(y0 / 2) + j) * pitch + x0 / 2 + (b & 3) * 8) = pk;
        }
    } else {
        *reinterpret_cast<uint2*>(&plane[w][j * PP + b * 8]) = pk;        // (only wave w read plane w since the last barrier)
        __syncthreads();
        const int px = t / 3, c = t - 3 * px;
        if (x0 + px < W) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                if (y0 + r < H)
                    dst[((long)(y0 + r) * W + x0 + px) * 3 + c] =
                        (unsigned char)rgb_channel(c, plane[0][r * PP + px], plane[1][r * PP + px], plane[2][r * PP + px]);
            }
        }
    }
}

// 4:2:0, second launch: one work item = 256 consecutive pixels of one image row.
__global__ __launch_bounds__(256) void upsample_kernel(const unsigned char* __restrict__ wy, const unsigned char* __restrict__ wcb,
                                                       const unsigned char* __restrict__ wcr, unsigned char* __restrict__ dst, int H, int W,
                                                       long ypitch, long cpitch, int segs) {
    __shared__ unsigned char out[3 * 256];
    const int t = threadIdx.x;
    const int hc = (H + 1) >> 1, wc = (W + 1) >> 1;
    const long items = (long)H * segs;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {           // uniform over the workgroup
        const int y = (int)(it / segs), xs = (int)(it - (long)y * segs) * 256;
        const int x = xs + t;
        if (x < W) {
            const int cy = y >> 1, cx = x >> 1;
            const int ny = (y & 1) ? min(cy + 1, hc - 1) : max(cy - 1, 0);
            const int nx = (x & 1) ? min(cx + 1, wc - 1) : max(cx - 1, 0);
            const int rnd = (x & 1) ? 7 : 8;
            const long a = cy * cpitch, n = ny * cpitch;
            const int cb = (3 * (3 * wcb[a + cx] + wcb[n + cx]) + (3 * wcb[a + nx] + wcb[n + nx]) + rnd) >> 4;
            const int cr = (3 * (3 * wcr[a + cx] + wcr[n + cx]) + (3 * wcr[a + nx] + wcr[n + nx]) + rnd) >> 4;
            const int Y = wy[y * ypitch + x];
            out[3 * t + 0] = (unsigned char)rgb_channel(0, Y, cb, cr);
            out[3 * t + 1] = (unsigned char)rgb_channel(1, Y, cb, cr);
            out[3 * t + 2] = (unsigned char)rgb_channel(2, Y, cb, cr);
        }
        __syncthreads();
        const int nbytes = 3 * min(256, W - xs);
        unsigned char* d = dst + ((long)y * W + xs) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k * 256 + t < nbytes) d[k * 256 + t] = out[k * 256 + t];
        __syncthreads();                                 // before the next item overwrites the segment
    }
}

// tiles of the image, or false when it is beyond the kernels' reach (tile counts and plane offsets stay far inside an int / a long)
bool geometry(int H, int W, int subsampling, long* tiles_x, long* tiles_y) {
    if (H < 1 || W < 1 || (subsampling != 0 && subsampling != 2)) return false;
    *tiles_x = (W + TW - 1) / TW;
    *tiles_y = subsampling == 2 ? ((long)H + 15) / 16 : ((long)H + 7) / 8;
    return *tiles_x * *tiles_y <= (1L << 20);            // 2^30 padded pixels
}

}  // namespace

extern "C" int rcot_jpeg_ws_bytes(int H, int W, int subsampling) {
    long tiles_x, tiles_y;
    if (!geometry(H, W, subsampling, &tiles_x, &tiles_y)) return RCOT_EINVAL;
    if (subsampling == 0) return 0;
    return (int)(tiles_x * tiles_y * (16 * TW + 2 * 8 * (TW / 2)) + 16);             // Y, Cb, Cr planes and the slack of a 16-byte alignment
}

extern "C" int rcot_jpeg_roundtrip(const unsigned char* src, unsigned char* dst, int H, int W, int quality, int subsampling, void* ws,
                                   size_t ws_bytes, void* stream) {
    long tiles_x, tiles_y;
    if (!src || !dst || !geometry(H, W, subsampling, &tiles_x, &tiles_y) || quality < 1 || quality > 100) return RCOT_EINVAL;
    if (subsampling == 2 && (W <= 4 || !ws || ws_bytes < (size_t)rcot_jpeg_ws_bytes(H, W, subsampling))) return RCOT_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const Tables tab = make_tables(quality);
    const dim3 grid((unsigned)(tiles_x * tiles_y));
    if (subsampling == 0) {
        RCOT_LAUNCH(roundtrip_kernel<0>, grid, dim3(NT), 0, st, src, dst, H, W, (int)tiles_x, tab, (unsigned char*)nullptr,
                    (unsigned char*)nullptr, (unsigned char*)nullptr);
        RCOT_LAUNCH_CHECK();
        return RCOT_OK;
    }
    unsigned char* wy = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(ws) + 15) & ~(uintptr_t)15);
    unsigned char* wcb = wy + tiles_x * tiles_y * 16 * TW;
    unsigned char* wcr = wcb + tiles_x * tiles_y * 8 * (TW / 2);
    RCOT_LAUNCH(roundtrip_kernel<2>, grid, dim3(NT), 0, st, src, dst, H, W, (int)tiles_x, tab, wy, wcb, wcr);
    RCOT_LAUNCH_CHECK();
    const int segs = (W + 255) / 256;
    const long items = (long)H * segs;
    RCOT_LAUNCH(upsample_kernel, dim3((unsigned)(items < 8192 ? items : 8192)), dim3(256), 0, st, (const unsigned char*)wy,
                (const unsigned char*)wcb, (const unsigned char*)wcr, dst, H, W, tiles_x * TW, tiles_x * (TW / 2), segs);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}
