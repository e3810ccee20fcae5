// Whole-image validation at any size (rcot_amd/wholeimage.py; reference trainer.py:179-227, tester.py:56-113, evaluate.py:43-106):
//   rcot_image_ingest : uint8 HWC image -> float CHW / 255, padded at the bottom / right to the network's size multiple
//   rcot_pad2d        : the same padding for float planes (the testers' noisy input, batched tensors)
//   rcot_image_egress : crop of the network's output, 8-bit quantisation as torchvision's save_image does it, the scaled residual, and the
//                       sums under PSNR (float and 8-bit) and under the testers' 2 x 2 box-window SSIM
//   rcot_image_ingest_batch / rcot_image_egress_batch : the same for N images of one padded shape in one launch (two with statistics), from
//                       a device table of one row per image (rcot_amd/valsuite.py); the device code is the single kernels', so are the bits
// All of it is HBM-bound row work.  One wave owns TILE pixels of one image row (4 per lane: float4 on the planes where the row length
// and the pointers allow); the 3w-byte HWC rows are generally unaligned, so their bytes cross LDS: aligned dwords on the global side,
// single bytes only for a row segment's first / last partial dword.  The statistics are per-workgroup partials in the caller's
// workspace, summed by a second one-workgroup launch in a fixed order: bitwise reproducible, no float atomics.  gfx950 only.
#include "../../include/rcot_hip.h"
#include "common.h"

using namespace rcot;

namespace {

constexpr int TILE = 256;                               // pixels of one row per wave
constexpr int ROWS = 4;                                 // waves (image rows) per workgroup
constexpr int LW = (4 + 3 + 3 * (TILE + 1) + 3) / 4 + 1;   // LDS words of one staged row segment: offset 4 + phase <= 3 + halo pixel + TILE pixels

// source row / column of padded row / column r of an n-long axis: torch's 'reflect' (mode 1) or 'replicate' (mode 2)
__device__ __forceinline__ int src_index(int r, int n, int mode) { return r < n ? r : (mode == 1 ? 2 * (n - 1) - r : n - 1); }

__host__ __device__ inline bool pad_geometry_ok(int h, int w, int Hp, int Wp, int mode) {
    if (h <= 0 || w <= 0 || Hp < h || Wp < w) return false;
    if (mode == 0) return Hp == h && Wp == w;
    if (mode == 1) return Hp - h <= h - 1 && Wp - w <= w - 1;
    return mode == 2;
}

// n bytes at g (any alignment) -> LDS: byte k lands at LDS byte (g & 3) + k.  One wave; aligned dwords, bytes for the partial ends.
__device__ __forceinline__ void stage_in(const uint8_t* __restrict__ g, int n, uint32_t* lds, int lane) {
    const int ph = (int)(reinterpret_cast<uintptr_t>(g) & 3);
    const uint8_t* ga = g - ph;
    const int nd = (ph + n + 3) >> 2;
    for (int j = lane; j < nd; j += WAVE) {
        const int lo = 4 * j;
        uint32_t v = 0;
        if (lo >= ph && lo + 4 <= ph + n) {
            v = *reinterpret_cast<const uint32_t*>(ga + lo);
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (lo + b >= ph && lo + b < ph + n) v |= (uint32_t)ga[lo + b] << (8 * b);
        }
        lds[j] = v;
    }
}

// the reverse: LDS byte (g & 3) + k -> g[k], k < n
__device__ __forceinline__ void stage_out(uint8_t* __restrict__ g, int n, const uint32_t* lds, int lane) {
    const int ph = (int)(reinterpret_cast<uintptr_t>(g) & 3);
    uint8_t* ga = g - ph;
    const int nd = (ph + n + 3) >> 2;
    for (int j = lane; j < nd; j += WAVE) {
        const int lo = 4 * j;
        const uint32_t v = lds[j];
        if (lo >= ph && lo + 4 <= ph + n) {
            *reinterpret_cast<uint32_t*>(ga + lo) = v;
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (lo + b >= ph && lo + b < ph + n) ga[lo + b] = (uint8_t)(v >> (8 * b));
        }
    }
}

// ------------------------------------------------------------------ ingest: uint8 [h][w][3] -> float [3][Hp][Wp] / 255, padded
// VEC: Wp % 4 == 0 and `out` 16-byte aligned (every lane's four pixels are inside the row)
// The workgroup's part of one image: rows blockIdx.x * ROWS .., columns blockIdx.y * TILE .. (shared by the single and the batched kernel)
template <bool VEC>
__device__ __forceinline__ void ingest_tile(const uint8_t* __restrict__ img, float* __restrict__ out, int h, int w, int Hp, int Wp,
                                            int mode) {
    __shared__ uint32_t sm[ROWS][LW];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int y = blockIdx.x * ROWS + wave, x0 = blockIdx.y * TILE;
    const bool live = y < Hp;
    const uint8_t* row = img + (long)(live ? src_index(y, h, mode) : 0) * w * 3;
    const int nin = min(TILE, w - x0);                   // source pixels of this segment (<= 0: padding columns only)
    int ph = 0;
    if (live && nin > 0) {
        const uint8_t* g = row + (long)x0 * 3;
        ph = (int)(reinterpret_cast<uintptr_t>(g) & 3);
        stage_in(g, nin * 3, sm[wave], lane);
    }
    __syncthreads();
    const int x = x0 + 4 * lane;
    if (!live || x >= Wp) return;
    const uint8_t* lb = reinterpret_cast<const uint8_t*>(sm[wave]) + ph;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int xx = x + k;
            uint8_t u = 0;
            if (xx < w) u = lb[(xx - x0) * 3 + c];
            else if (xx < Wp) u = row[(long)src_index(xx, w, mode) * 3 + c];
            v[k] = __fdiv_rn((float)u, 255.0f);          // correctly rounded: the bits of torch's .float().div(255)
        }
        float* o = out + ((long)c * Hp + y) * Wp + x;
        if (VEC) {
            *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x + k < Wp) o[k] = v[k];
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void ingest_kernel(const uint8_t* __restrict__ img, float* __restrict__ out, int h, int w, int Hp, int Wp,
                                                     int mode) {
    ingest_tile<VEC>(img, out, h, w, Hp, Wp, mode);
}

// image blockIdx.z of a batch: row {img, h, w, 0} of the table, slot blockIdx.z of out [N][3][Hp][Wp].  The caller has checked every row;
// a row whose geometry `mode` cannot pad is left out all the same (its reads would leave the image).
template <bool VEC>
__global__ __launch_bounds__(256) void ingest_batch_kernel(const long long* __restrict__ table, float* __restrict__ out, int Hp, int Wp,
                                                           int mode) {
    const long long* row = table + 4 * (long)blockIdx.z;
    const uint8_t* img = reinterpret_cast<const uint8_t*>(row[0]);
    const int h = (int)row[1], w = (int)row[2];
    if (!img || !pad_geometry_ok(h, w, Hp, Wp, mode)) return;
    ingest_tile<VEC>(img, out + (long)blockIdx.z * 3 * Hp * Wp, h, w, Hp, Wp, mode);
}

// ------------------------------------------------------------------ pad2d: float [planes][h][w] -> [planes][Hp][Wp]
// one workgroup row per output row (blockIdx.x), 256 lanes x 4 columns per blockIdx.y.  VOUT: Wp % 4 == 0 and dst aligned;
// vin: w % 4 == 0 and src aligned (float4 reads of the unpadded part)
template <bool VOUT>
__global__ __launch_bounds__(256) void pad2d_kernel(const float* __restrict__ src, float* __restrict__ dst, int h, int w, int Hp, int Wp,
                                                    int mode, int vin) {
    const long orow = blockIdx.x;                        // plane * Hp + y
    const long plane = orow / Hp;
    const int y = (int)(orow - plane * Hp);
    const int x = (blockIdx.y * 256 + threadIdx.x) * 4;
    if (x >= Wp) return;
    const float* s = src + (plane * h + src_index(y, h, mode)) * w;
    float* o = dst + orow * Wp + x;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (vin && x + 3 < w) {
        const float4 t = *reinterpret_cast<const float4*>(s + x);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x + k < Wp) v[k] = s[src_index(x + k, w, mode)];
    }
    if (VOUT) {
        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x + k < Wp) o[k] = v[k];
    }
}

// ------------------------------------------------------------------ egress
// trainer.save_image for B = 1 (torchvision): clamp(0, 1), * 255, + 0.5, clamp(0, 255), truncate — every step an fp32 rounding of its own
__device__ __forceinline__ int quant8(float v) {
#pragma clang fp contract(off)
    const float c = fminf(fmaxf(v, 0.f), 1.f);
    const float m = c * 255.0f;
    float a = m + 0.5f;
    a = fminf(fmaxf(a, 0.f), 255.f);
    return (int)a;
}

struct EgressArgs {
    const float* restored;        // [3][Hp][Wp]
    const float* degraded;        // same geometry, or null
    const uint8_t* target;        // [h][w][3], or null
    uint8_t* out_u8;              // [h][w][3], or null
    uint8_t* res_u8;              // [h][w][3], or null
    double* part_d;               // [2][nblocks]: float-PSNR sum, SSIM map sum (null: no statistics)
    long long* part_i;            // [nblocks]: 8-bit squared error
    int h, w, Hp, Wp;
    float res_scale;
};

// four pixels of row y from column x of plane c (x < w; VEC: the whole float4 is inside the padded row)
template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ p, const EgressArgs& a, int c, int y, int x, float (&v)[4]) {
    const float* s = p + ((long)c * a.Hp + y) * a.Wp + x;
    if (VEC) {
        const float4 t = *reinterpret_cast<const float4*>(s);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = x + k < a.w ? s[k] : 0.f;
    }
}

// One wave per TILE pixels of image row y.  LDS per wave: the quantised rows y (0) and y - 1 (1) and the target's, each with the pixel left
// of the segment (the 2 x 2 SSIM window ends at (y, x)), and the residual row.  Row y - 1 is re-quantised from `restored` (an L2 hit).
// `gx`: workgroups along the rows of THIS image's own grid (ceil(h / ROWS)), `nb`: workgroups of that grid — the partials are laid out by
// them, whatever the launch grid is (the batched launch is sized by the padded shape).
template <bool VEC>
__device__ __forceinline__ void egress_tile(const EgressArgs& a, long gx, long nb) {
    __shared__ uint32_t s_q[ROWS][2][LW], s_t[ROWS][2][LW], s_r[ROWS][LW];
    __shared__ double s_d[ROWS][2];
    __shared__ long long s_i[ROWS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int y = blockIdx.x * ROWS + wave, x0 = blockIdx.y * TILE;
    const int h = a.h, w = a.w;
    const bool live = y < h;
    const int npx = min(TILE, w - x0);                   // >= 1 by the grid
    const int hal = x0 > 0 ? 1 : 0;
    const bool stats = a.part_d != nullptr;
    const bool srow = stats && live && y >= 5 && y < h - 5 && w > 10;     // this row holds SSIM map elements
    const int x = x0 + 4 * lane;
    const bool lact = live && x < w;
    const long rowb = ((long)y * w + x0) * 3;            // byte offset of the segment in an [h][w][3] image
    // byte of pixel i (-1 .. npx - 1), channel c: q rows at qo + 3 i + c (both rows: phase of out_u8's segment), target rows at t?o + 3 i + c
    const int qo = 4 + (a.out_u8 ? (int)(reinterpret_cast<uintptr_t>(a.out_u8 + rowb) & 3) : 0);
    const int ro = a.res_u8 ? (int)(reinterpret_cast<uintptr_t>(a.res_u8 + rowb) & 3) : 0;
    uint8_t* q0 = reinterpret_cast<uint8_t*>(s_q[wave][0]);
    uint8_t* q1 = reinterpret_cast<uint8_t*>(s_q[wave][1]);
    uint8_t* rb = reinterpret_cast<uint8_t*>(s_r[wave]);
    int t0o = 0, t1o = 0;
    if (stats && live) {
        const uint8_t* g = a.target + rowb - 3 * hal;
        t0o = (int)(reinterpret_cast<uintptr_t>(g) & 3) + 3 * hal;
        stage_in(g, (npx + hal) * 3, s_t[wave][0], lane);
        if (srow) {
            const uint8_t* gp = g - (long)w * 3;
            t1o = (int)(reinterpret_cast<uintptr_t>(gp) & 3) + 3 * hal;
            stage_in(gp, (npx + hal) * 3, s_t[wave][1], lane);
        }
    }
    float r[3][4];
    int q[3][4];
    if (lact) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            load4<VEC>(a.restored, a, c, y, x, r[c]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                q[c][k] = quant8(r[c][k]);
                if (x + k < w) q0[qo + 3 * (4 * lane + k) + c] = (uint8_t)q[c][k];
            }
            if (a.res_u8) {
                float d[4];
                load4<VEC>(a.degraded, a, c, y, x, d);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float diff = d[k] - r[c][k];           // (xd - out), then * scale: two fp32 roundings
                    const float sc = diff * a.res_scale;
                    if (x + k < w) rb[ro + 3 * (4 * lane + k) + c] = (uint8_t)quant8(sc);
                }
            }
            if (srow) {
                float p[4];
                load4<VEC>(a.restored, a, c, y - 1, x, p);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (x + k < w) q1[qo + 3 * (4 * lane + k) + c] = (uint8_t)quant8(p[k]);
            }
        }
    }
    if (srow && hal && lane == 0) {                      // the pixel left of the segment, rows y and y - 1
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* s = a.restored + ((long)c * a.Hp + y) * a.Wp + (x0 - 1);
            q0[qo - 3 + c] = (uint8_t)quant8(s[0]);
            q1[qo - 3 + c] = (uint8_t)quant8(s[-(long)a.Wp]);
        }
    }
    __syncthreads();
    if (live && a.out_u8) stage_out(a.out_u8 + rowb, npx * 3, s_q[wave][0] + 1, lane);
    if (live && a.res_u8) stage_out(a.res_u8 + rowb, npx * 3, s_r[wave], lane);
    if (!stats) return;

    double sf = 0.0, ss = 0.0;
    long long si = 0;
    if (lact) {
        const uint8_t* t0 = reinterpret_cast<const uint8_t*>(s_t[wave][0]) + t0o;
        const uint8_t* t1 = reinterpret_cast<const uint8_t*>(s_t[wave][1]) + t1o;
        constexpr double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int xx = x + k, i = 4 * lane + k;
                if (xx >= w) continue;
                const int t = t0[3 * i + c];
                const double df = (double)r[c][k] - (double)__fdiv_rn((float)t, 255.0f);
                sf += df * df;
                const int di = q[c][k] - t;
                si += di * di;
                if (srow && xx >= 5 && xx < w - 5) {
                    // window sums over 8-bit integers are exact; mu = S / 4 and the (co)variances are exact in fp64 as well
                    const int a11 = q[c][k], a10 = q0[qo + 3 * (i - 1) + c], a01 = q1[qo + 3 * i + c], a00 = q1[qo + 3 * (i - 1) + c];
                    const int b11 = t, b10 = t0[3 * (i - 1) + c], b01 = t1[3 * i + c], b00 = t1[3 * (i - 1) + c];
                    const int Sa = a00 + a01 + a10 + a11, Sb = b00 + b01 + b10 + b11;
                    const int Saa = a00 * a00 + a01 * a01 + a10 * a10 + a11 * a11, Sbb = b00 * b00 + b01 * b01 + b10 * b10 + b11 * b11;
                    const int Sab = a00 * b00 + a01 * b01 + a10 * b10 + a11 * b11;
                    const double mu1 = 0.25 * Sa, mu2 = 0.25 * Sb;
                    const double s1 = 0.25 * Saa - mu1 * mu1, s2 = 0.25 * Sbb - mu2 * mu2, s12 = 0.25 * Sab - mu1 * mu2;
                    ss += ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2));
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sf += __shfl_xor(sf, o, 64);
        ss += __shfl_xor(ss, o, 64);
        si += __shfl_xor(si, o, 64);
    }
    if (lane == 0) {
        s_d[wave][0] = sf;
        s_d[wave][1] = ss;
        s_i[wave] = si;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const long b = (long)blockIdx.y * gx + blockIdx.x;
        double f = 0.0, s = 0.0;
        long long n = 0;
#pragma unroll
        for (int v = 0; v < ROWS; ++v) {
            f += s_d[v][0];
            s += s_d[v][1];
            n += s_i[v];
        }
        a.part_d[b] = f;
        a.part_d[nb + b] = s;
        a.part_i[b] = n;
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void egress_kernel(EgressArgs a) {
    egress_tile<VEC>(a, gridDim.x, (long)gridDim.x * gridDim.y);
}

// The batched form.  Image i = blockIdx.z: row {target, out_u8 (0: none), h, w} of the table, slot i of restored [N][3][Hp][Wp].  The launch
// grid covers Hp x Wp; the workgroups beyond an image's own grid leave at once.  Image i owns `slot` = 3 * ceil(Hp / ROWS) * ceil(Wp / TILE)
// 8-byte words of the workspace and lays its partials out there as the single kernel does: by its own grid.
__device__ __forceinline__ long own_grid(int h, int w, long& gx) {
    gx = (h + ROWS - 1) / ROWS;
    return gx * ((w + TILE - 1) / TILE);
}

template <bool VEC>
__global__ __launch_bounds__(256) void egress_batch_kernel(const float* __restrict__ restored, const long long* __restrict__ table, int Hp,
                                                           int Wp, double* __restrict__ ws, long slot) {
    const long i = blockIdx.z;
    const long long* row = table + 4 * i;
    EgressArgs a;
    a.h = (int)row[2]; a.w = (int)row[3]; a.Hp = Hp; a.Wp = Wp;
    if (a.h <= 0 || a.w <= 0 || a.h > Hp || a.w > Wp) return;             // (checked by the caller; never reached with a checked table)
    long gx;
    const long nb = own_grid(a.h, a.w, gx);
    if ((long)blockIdx.x >= gx || (long)blockIdx.y * TILE >= a.w) return;
    a.restored = restored + i * 3 * Hp * Wp;
    a.degraded = nullptr;
    a.target = reinterpret_cast<const uint8_t*>(row[0]);
    a.out_u8 = reinterpret_cast<uint8_t*>(row[1]);
    a.res_u8 = nullptr;
    a.res_scale = 0.f;
    a.part_d = ws && a.target ? ws + i * slot : nullptr;
    a.part_i = a.part_d ? reinterpret_cast<long long*>(a.part_d) + 2 * nb : nullptr;
    egress_tile<VEC>(a, gx, nb);
}

// stats[0..4) from the partials, one workgroup, fixed order (final_sums)
__device__ __forceinline__ void egress_final(const double* __restrict__ part_d, const long long* __restrict__ part_i, long nb, int h, int w,
                                             double* __restrict__ stats) {
    double d[2];
    long long n;
    final_sums<2>(part_d, part_i, nb, d, n);
    if (threadIdx.x == 0) {
        stats[0] = d[0];
        stats[1] = (double)n;
        stats[2] = d[1];
        stats[3] = 3.0 * (double)(h > 10 ? h - 10 : 0) * (double)(w > 10 ? w - 10 : 0);
    }
}

__global__ __launch_bounds__(256) void egress_final_kernel(const double* __restrict__ part_d, const long long* __restrict__ part_i, long nb,
                                                           int h, int w, double* __restrict__ stats) {
    egress_final(part_d, part_i, nb, h, w, stats);
}

// one workgroup per image of the batch: stats [N][4]
__global__ __launch_bounds__(256) void egress_batch_final_kernel(const long long* __restrict__ table, int Hp, int Wp,
                                                                 const double* __restrict__ ws, long slot, double* __restrict__ stats) {
    const long i = blockIdx.x;
    const long long* row = table + 4 * i;
    const int h = (int)row[2], w = (int)row[3];
    if (!row[0] || h <= 0 || w <= 0 || h > Hp || w > Wp) return;
    long gx;
    const long nb = own_grid(h, w, gx);
    const double* part_d = ws + i * slot;
    egress_final(part_d, reinterpret_cast<const long long*>(part_d) + 2 * nb, nb, h, w, stats + 4 * i);
}

}  // namespace

extern "C" {

int rcot_image_ingest(const unsigned char* img, int h, int w, float* out, int Hp, int Wp, int mode, void* stream) {
    if (!img || !out || !pad_geometry_ok(h, w, Hp, Wp, mode)) return RCOT_EINVAL;
    const dim3 grid(cdiv(Hp, ROWS), cdiv(Wp, TILE));
    if (grid.y > 65535u) return RCOT_EINVAL;
    if ((Wp & 3) == 0 && al16(out))
        RCOT_LAUNCH(ingest_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, img, out, h, w, Hp, Wp, mode);
    else
        RCOT_LAUNCH(ingest_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, img, out, h, w, Hp, Wp, mode);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

int rcot_image_ingest_batch(const long long* table, int N, int Hp, int Wp, int mode, float* out, void* stream) {
    if (!table || !out || N < 1 || N > 65535 || mode < 0 || mode > 2 || Hp < 1 || Wp < 1) return RCOT_EINVAL;
    const dim3 grid(cdiv(Hp, ROWS), cdiv(Wp, TILE), N);
    if (grid.y > 65535u) return RCOT_EINVAL;
    if ((Wp & 3) == 0 && al16(out))                       // (every slot is 12 Hp Wp bytes behind the one before: aligned alike)
        RCOT_LAUNCH(ingest_batch_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, table, out, Hp, Wp, mode);
    else
        RCOT_LAUNCH(ingest_batch_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, table, out, Hp, Wp, mode);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

int rcot_pad2d(const float* src, float* dst, long planes, int h, int w, int Hp, int Wp, int mode, void* stream) {
    if (!src || !dst || planes <= 0 || !pad_geometry_ok(h, w, Hp, Wp, mode)) return RCOT_EINVAL;
    if (planes * (long)Hp > 0x7fffffffL || cdiv(Wp, 1024) > 65535) return RCOT_EINVAL;
    const dim3 grid((unsigned)(planes * Hp), cdiv(Wp, 1024));
    const int vin = (w & 3) == 0 && al16(src);
    if ((Wp & 3) == 0 && al16(dst))
        RCOT_LAUNCH(pad2d_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, src, dst, h, w, Hp, Wp, mode, vin);
    else
        RCOT_LAUNCH(pad2d_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, src, dst, h, w, Hp, Wp, mode, vin);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

int rcot_image_egress(const float* restored, const float* degraded, const unsigned char* target, int h, int w, int Hp, int Wp,
                      float res_scale, unsigned char* out_u8, unsigned char* res_u8, double* stats, float* ws, size_t ws_bytes,
                      void* stream) {
    if (!restored || h <= 0 || w <= 0 || Hp < h || Wp < w) return RCOT_EINVAL;
    if (res_u8 && !degraded) return RCOT_EINVAL;
    if (stats && (!target || !ws || (reinterpret_cast<uintptr_t>(ws) & 7) || (reinterpret_cast<uintptr_t>(stats) & 7))) return RCOT_EINVAL;
    if (!out_u8 && !res_u8 && !stats) return RCOT_EINVAL;
    const dim3 grid(cdiv(h, ROWS), cdiv(w, TILE));
    if (grid.y > 65535u) return RCOT_EINVAL;
    const long nb = (long)grid.x * grid.y;
    if (stats && (size_t)nb * 24 > ws_bytes) return RCOT_EWORKSPACE;
    EgressArgs a;
    a.restored = restored;
    a.degraded = degraded;
    a.target = target;
    a.out_u8 = out_u8;
    a.res_u8 = res_u8;
    a.part_d = stats ? reinterpret_cast<double*>(ws) : nullptr;
    a.part_i = stats ? reinterpret_cast<long long*>(ws) + 2 * nb : nullptr;
    a.h = h; a.w = w; a.Hp = Hp; a.Wp = Wp;
    a.res_scale = res_scale;
    const bool vec = (Wp & 3) == 0 && al16(restored) && (!res_u8 || al16(degraded));
    if (vec)
        RCOT_LAUNCH(egress_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else
        RCOT_LAUNCH(egress_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
    RCOT_LAUNCH_CHECK();
    if (stats) {
        RCOT_LAUNCH(egress_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)a.part_d, (const long long*)a.part_i, nb, h,
                    w, stats);
        RCOT_LAUNCH_CHECK();
    }
    return RCOT_OK;
}

int rcot_image_egress_batch(const float* restored, const long long* table, int N, int Hp, int Wp, double* stats, float* ws, size_t ws_bytes,
                            void* stream) {
    if (!restored || !table || N < 1 || N > 65535 || Hp < 1 || Wp < 1) return RCOT_EINVAL;
    const dim3 grid(cdiv(Hp, ROWS), cdiv(Wp, TILE), N);
    if (grid.y > 65535u) return RCOT_EINVAL;
    if (stats && (reinterpret_cast<uintptr_t>(stats) & 7)) return RCOT_EINVAL;
    const long slot = 3L * grid.x * grid.y;
    if (stats && (!ws || (reinterpret_cast<uintptr_t>(ws) & 7) || (size_t)N * slot * 8 > ws_bytes)) return RCOT_EWORKSPACE;
    double* wsd = stats ? reinterpret_cast<double*>(ws) : nullptr;
    if ((Wp & 3) == 0 && al16(restored))
        RCOT_LAUNCH(egress_batch_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, restored, table, Hp, Wp, wsd, slot);
    else
        RCOT_LAUNCH(egress_batch_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, restored, table, Hp, Wp, wsd, slot);
    RCOT_LAUNCH_CHECK();
    if (stats) {
        RCOT_LAUNCH(egress_batch_final_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, table, Hp, Wp, (const double*)wsd, slot, stats);
        RCOT_LAUNCH_CHECK();
    }
    return RCOT_OK;
}

}  // extern "C"
