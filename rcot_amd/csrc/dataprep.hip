// Patch preparation on the device: the per-sample work of the reference's TrainDataset.__getitem__
// (util/dataset_utils.py:215-281) after the image file has been decoded —
//   crop a P x P window            (RandomCrop / _crop_patch, :57-60, :188-196)
//   one of the 8 dihedral maps      (util/image_utils.py:133-163 data_augmentation, mode drawn by :177-182)
//   Gaussian noise + uint8 quantise (util/degradation_utils.py:21-27: clip(clean + randn*sigma, 0, 255).astype(uint8))
//   ToTensor                        (HWC uint8 -> CHW float / 255, :264-265)
// in ONE pass from the uint8 HWC image(s) resident in HBM straight into the sample's slot of the batch tensors.
// Two routes reach it (rcot_amd/data.py).  Uncached (the default): the host decodes the files of every sample, uploads them, draws
// (y0, x0, mode, seed) and launches patch_prep_kernel once per sample.  Cached (--data_cache device, rcot_amd/imagecache.py): every
// file is decoded and uploaded ONCE, the images stay in HBM, and the host only draws (y0, x0, mode, seed) per sample, writes one
// table row per sample and launches patch_prep_batch_kernel once per batch.  At >= 1000 patches/s the PIL/numpy chain of the
// reference (num_workers = 0, trainer.py:32,134) would be the bottleneck of the training loop.
#include "common.h"
#include "../../include/rcot_hip.h"

namespace {

// One pixel p = i P + j of the mapped patch, all three channels: what both kernels below do per pixel (ONE copy, so row b of the batch
// kernel runs the instruction sequence of the per-sample kernel and gives its bits, noise included).
__device__ __forceinline__ void prep_pixel(const unsigned char* __restrict__ deg, const unsigned char* __restrict__ clean, int W, int y0,
                                           int x0, int P, int mode, float sigma, uint64_t seed, int p, int n,
                                           float* __restrict__ deg_out, float* __restrict__ clean_out) {
    const int i = p / P, j = p - i * P;
    int sy, sx;
    rcot::dihedral(mode, P, P, i, j, sy, sx);
    const long src = ((long)(y0 + sy) * W + (x0 + sx)) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float cv = (float)clean[src + c];
        float dv;
        if (deg) {
            dv = (float)deg[src + c];
        } else {
            // the reference adds noise AFTER the augmentation, element by element of the HWC patch
            const float v = cv + sigma * rcot::counter_randn(seed, ((uint64_t)p) * 3 + c);
            dv = floorf(fminf(fmaxf(v, 0.f), 255.f));                        // clip, then astype(uint8) truncation
        }
        clean_out[(long)c * n + p] = cv / 255.0f;            // ToTensor divides (bit-equal to the reference's values)
        deg_out[(long)c * n + p] = dv / 255.0f;
    }
}

__global__ __launch_bounds__(256) void patch_prep_kernel(const unsigned char* __restrict__ deg, const unsigned char* __restrict__ clean,
                                                         int W, int y0, int x0, int P, int mode, float sigma, uint64_t seed,
                                                         float* __restrict__ deg_out, float* __restrict__ clean_out) {
    const int n = P * P;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256)
        prep_pixel(deg, clean, W, y0, x0, P, mode, sigma, seed, p, n, deg_out, clean_out);
}

// A whole batch in ONE launch: blockIdx.y is the sample, blockIdx.x the pixel block.  tab[b] = { clean image, degraded image (0: synthetic
// noise), W, y0, x0, mode, sigma as float32 bits, seed } (8 x int64 per sample, as rcot_pack_weights takes its table); the images of
// different rows may differ in size, and paired and noise rows may share a launch (the branch is uniform per workgroup).  The row is
// read through uniform addresses (scalar loads); the outputs of sample b are the b-th [3][P][P] slots of deg_out / clean_out.
// The transposing maps (modes 2, 3, 6, 7) read the window down its columns: a P x P window of uint8 RGB is 3 P^2 bytes (48 KiB at
// P = 128) and stays in L2, so there is no LDS transpose here.  Measured on an MI355X at B = 8, P = 128 (scripts/bench_loader.py,
// profiles/loader_cache.txt; two runs): kernel time about 5 us for the batch against 34 - 38 us for the eight per-sample launches;
// paired rows 4.6 - 4.7 us with the identity, 4.8 - 4.9 us with mode 5 (mirrored rows), 5.5 - 5.8 us with mode 2 (transposing), noise
// rows 4.8 - 5.1 us in all three — one microsecond at most for reading down the columns, in a launch the host takes > 20 us to issue.
__global__ __launch_bounds__(256) void patch_prep_batch_kernel(const long long* __restrict__ tab, int P, float* __restrict__ deg_out,
                                                               float* __restrict__ clean_out) {
    const long long* t = tab + (long)blockIdx.y * 8;
    const unsigned char* clean = reinterpret_cast<const unsigned char*>(t[0]);
    const unsigned char* deg = reinterpret_cast<const unsigned char*>(t[1]);
    const int W = (int)t[2], y0 = (int)t[3], x0 = (int)t[4], mode = (int)t[5];
    const float sigma = __int_as_float((int)t[6]);
    const uint64_t seed = (uint64_t)t[7];
    const int n = P * P;
    const long slot = (long)blockIdx.y * 3 * n;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256)
        prep_pixel(deg, clean, W, y0, x0, P, mode, sigma, seed, p, n, deg_out + slot, clean_out + slot);
}

}  // namespace

extern "C" int rcot_patch_prep(const unsigned char* deg_img, const unsigned char* clean_img, int H, int W, int y0, int x0,
                               int P, int mode, float noise_sigma, unsigned long long seed, float* deg_out, float* clean_out,
                               void* stream) {
    if (!clean_img || !deg_out || !clean_out || P <= 0 || y0 < 0 || x0 < 0 || y0 + P > H || x0 + P > W || mode < 0 || mode > 7)
        return RCOT_EINVAL;
    const int nb = (P * P + 255) / 256;
    RCOT_LAUNCH(patch_prep_kernel, dim3(nb > 256 ? 256 : nb), dim3(256), 0, (hipStream_t)stream, deg_img, clean_img, W, y0, x0,
                       P, mode, noise_sigma, (uint64_t)seed, deg_out, clean_out);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}

extern "C" int rcot_patch_prep_batch(const long long* table, int B, int P, float* deg_out, float* clean_out, void* stream) {
    if (!table || !deg_out || !clean_out || B <= 0 || B > 65535 || P <= 0 || P > 32768) return RCOT_EINVAL;   // B: gridDim.y; P: P * P as int
    const int nb = (int)(((long)P * P + 255) / 256);
    RCOT_LAUNCH(patch_prep_batch_kernel, dim3(nb > 256 ? 256 : nb, B), dim3(256), 0, (hipStream_t)stream, table, P, deg_out, clean_out);
    RCOT_LAUNCH_CHECK();
    return RCOT_OK;
}
