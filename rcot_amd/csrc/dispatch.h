// Functions that one .hip of the library defines and another calls: each prototype once, default arguments included.  The
// defining and the calling file both include this header, so a definition that drifts from its callers does not compile.
// A try_* dispatcher returns RCOT_OK after launching, an error code, or NOT_ELIGIBLE when the shape is not one of its own.
#pragma once
#include "common.h"

namespace rcot {

struct EpiP;   // gemm_core.h

// gemm_x3.hip / gemm_x3w.hip: split-bf16 K-major projections; called by gemm_glds.hip
int try_gemm_kmajor_x3(const float* At, long lda, long sAo, long sAi, const float* Bm, long ldb, long sBo, long sBi,
                       const EpiP& ep, const float* ln_mu, const float* ln_rs, long sLN, const float* ln_c1,
                       const float* ln_c2, int Zo, int Zi, int M, int N, int K, float* ws, size_t ws_bytes, hipStream_t st);
int try_gemm_kmajor_x3w(const float* At, long lda, long sAo, long sAi, const void* Apk, const float* Bm, long ldb, long sBo,
                        long sBi, const EpiP& ep, const float* ln_mu, const float* ln_rs, long sLN, const float* ln_c1,
                        const float* ln_c2, int Zo, int Zi, int M, int N, int K, float* ws, size_t ws_bytes, hipStream_t st,
                        bool ln_compute, int nterms);

// gemm_nt_glds.hip: LDS-DMA pipelined pixel-reduction kernel; called by gemm_ops.hip
int try_gemm_nt_glds(int M, int N, int K, int Zo, int Zi, const float* A, long lda, long sAo, long sAi, const float* B,
                     long ldb, long sBo, long sBi, int Kb, long sAk, long sBk, const float* mu, const float* rs,
                     long sLNb, const float* lnw, const float* lnb, const EpiP& ep, float* ws, size_t ws_bytes,
                     hipStream_t st, int prec, int* slabs_S = nullptr, int* slabs_ld = nullptr, int conv_wp = 0);

// gemm_x3w.hip: data gradient + weight-gradient slabs of one incoming gradient in one launch; called by gemm_ops.hip
int pair_dgrad_wgrad_x3(const float* WP, long ldp, const void* WPs, const float* dY, long sdYb, float* dX, long sdXb, const float* X,
                        long sXb, int B, int Ci, int Co, int N, const float* ln_mu, const float* ln_rs, const float* ln_w,
                        const float* ln_b, float* ws, size_t ws_bytes, float* ws_slabs, size_t ws_slabs_bytes, int* S_out,
                        int* ld_out, hipStream_t st);

// gemm_x3w.hip: 3x3 convolution over padded channel-major planes; called by conv_pcm.hip
int conv_pcm_x3w(const void* Apk, int M, int K, const float* Xp, long ldb, int N, const int* tapoff, int ntaps, const float* bias,
                 float lrelu, const int* colmap, float* Y, long ldy, float* ws, size_t ws_bytes, hipStream_t st);

// conv_thin.hip: direct kernels of the 3-channel output side; called by conv_ops.hip
int try_conv_few_out(const float* in, const float* wt, long wb, long sco, long sci, long sky, long skx, const float* bias,
                     const float* R, float* out, int B, int Cin, int H, int W, int Cout, int KS, int pad, float lrelu,
                     float beta, hipStream_t st);
int try_wgrad_few_out(const float* dy, const float* x, float* dw, int B, int Cin, int H, int W, int Cout, int KS, int pad,
                      float beta, hipStream_t st);

}  // namespace rcot
