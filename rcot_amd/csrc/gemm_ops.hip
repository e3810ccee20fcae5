// C-ABI entry points built on the MFMA fp32 GEMM engine: 1x1 projections (fwd / data-grad /
// weight-grad, with the WithBias-LayerNorm prologue fused into the operand load), the
// batched small-matrix products of MDTA (Gram over H*W, attention apply, their gradients)
// and the critic's Linear layers.  See include/rcot_hip.h for the contract.
#include "gemm_core.h"
#include "dispatch.h"
#include "../../include/rcot_hip.h"

using namespace rcot;

namespace {

using CfgL = TileCfg<128, 128>;
using CfgS = TileCfg<64, 64>;
using CfgM = TileCfg<96, 128, 1, 4>;

template <class Cfg> using AStrK = StridedLoader<Cfg::BM, Cfg::SA, true>;
template <class Cfg> using AStrM = StridedLoader<Cfg::BM, Cfg::SA, false>;
template <class Cfg> using BStrK = StridedLoader<Cfg::BN, Cfg::SB, true>;
template <class Cfg> using BXc = XContigLoader<Cfg::BN, Cfg::SB>;
template <class Cfg> using AKc = KContigLoader<Cfg::BM, Cfg::SA>;
template <class Cfg> using BKc = KContigLoader<Cfg::BN, Cfg::SB>;

EpiP epi_default(float* C, long ldc) {
    EpiP e{};
    e.C = C; e.ldc = ldc;
    e.alpha = 1.f; e.beta = 0.f; e.lrelu = 1.f;
    return e;
}

// A strided (weights), B x-contiguous (activations, pixels along N).
int run_strided_xcontig(bool a_kfast, GemmDims d, const StridedP& ap, const XContigP& bp, const EpiP& ep, int Z,
                        hipStream_t st) {
    const bool big = plan_splitk(d, Z, nullptr, 0);
    // 96-row tile (1x4 wavefronts, each 96x32): M = 96/192/288/576 (C, 3C of the 96- and 192-channel levels)
    // fill it exactly, where the 128-row tile would idle a quarter of its MFMAs.
    const long pad96 = (long)cdiv(d.M, 96) * 96, pad128 = (long)cdiv(d.M, 128) * 128;
    // (k-fast A operands only: the x-fast element map of StridedLoader needs GEMM_NT % rows == 0, which 96 rows violate —
    // the unpacked data gradient of a 96-channel level at B*N >= 384 tiles used to come out wrong on this tile)
    if (big && pad96 < pad128 && a_kfast)
        return launch_gemm_cfg<CfgM, AStrK<CfgM>, StridedP, BXc<CfgM>, XContigP>(d, ap, bp, ep, Z, st);
    if (big) {
        if (a_kfast) return launch_gemm_cfg<CfgL, AStrK<CfgL>, StridedP, BXc<CfgL>, XContigP>(d, ap, bp, ep, Z, st);
        return launch_gemm_cfg<CfgL, AStrM<CfgL>, StridedP, BXc<CfgL>, XContigP>(d, ap, bp, ep, Z, st);
    }
    if (a_kfast) return launch_gemm_cfg<CfgS, AStrK<CfgS>, StridedP, BXc<CfgS>, XContigP>(d, ap, bp, ep, Z, st);
    return launch_gemm_cfg<CfgS, AStrM<CfgS>, StridedP, BXc<CfgS>, XContigP>(d, ap, bp, ep, Z, st);
}

// Both operands k-contiguous (reduction over pixels), split-K slabs.
int run_kcontig(GemmDims d, const KContigP& ap, const KContigP& bp, const EpiP& ep, int Z, float* ws,
                size_t ws_bytes, hipStream_t st) {
    const bool big = plan_splitk(d, Z, ws, ws_bytes);
    if (d.S > 1 && (size_t)d.M * d.N * Z * d.S * sizeof(float) > ws_bytes) return RCOT_EWORKSPACE;
    if (big) return launch_gemm_cfg<CfgL, AKc<CfgL>, KContigP, BKc<CfgL>, KContigP>(d, ap, bp, ep, Z, st);
    return launch_gemm_cfg<CfgS, AKc<CfgS>, KContigP, BKc<CfgS>, KContigP>(d, ap, bp, ep, Z, st);
}

// Both operands scalar-strided (Linear layers: tiny batch, weight-bandwidth bound), split-K.
int run_strided2(bool a_kfast, GemmDims d, const StridedP& ap, const StridedP& bp, const EpiP& ep, float* ws,
                 size_t ws_bytes, hipStream_t st) {
    plan_splitk(d, 1, ws, ws_bytes);
    if (a_kfast) return launch_gemm_cfg<CfgS, AStrK<CfgS>, StridedP, BStrK<CfgS>, StridedP, true>(d, ap, bp, ep, 1, st);
    return launch_gemm_cfg<CfgS, AStrM<CfgS>, StridedP, BStrK<CfgS>, StridedP, true>(d, ap, bp, ep, 1, st);
}

}  // namespace

extern "C" {

int rcot_conv1x1_fwd(const float* W, long ldw, const float* X, long sXb, float* Y, long sYb, int B, int Ci, int Co,
                     int N, const float* ln_mu, const float* ln_rs, const float* ln_w, const float* ln_b,
                     const float* R, long sRb, float beta, void* stream) {
    if (!W || !X || !Y || B <= 0 || Ci <= 0 || Co <= 0 || N <= 0) return RCOT_EINVAL;
    if ((N & 3) || (sXb & 3) || !al16(X)) return RCOT_EINVAL;
    if (ln_mu && (!ln_rs || !ln_w || !ln_b || !al16(ln_mu) || !al16(ln_rs))) return RCOT_EINVAL;
    GemmDims d{};
    d.M = Co; d.N = N; d.K = Ci; d.Zi = 1;
    StridedP ap{W, ldw, 1, 0, 0, Co, Ci};
    XContigP bp{X, (long)N, sXb, 0, N, Ci, ln_mu, ln_rs, (long)N, ln_w, ln_b};
    EpiP ep = epi_default(Y, N);
    ep.sCo = sYb;
    ep.R = R; ep.ldr = N; ep.sRo = sRb;
    ep.beta = beta;
    return run_strided_xcontig(true, d, ap, bp, ep, B, (hipStream_t)stream);
}

int rcot_conv1x1_dgrad(const float* W, long ldw, const float* dY, long sdYb, float* dX, long sdXb, int B, int Ci,
                       int Co, int N, float beta, void* stream) {
    if (!W || !dY || !dX || B <= 0 || Ci <= 0 || Co <= 0 || N <= 0) return RCOT_EINVAL;
    if ((N & 3) || (sdYb & 3) || !al16(dY)) return RCOT_EINVAL;
    GemmDims d{};
    d.M = Ci; d.N = N; d.K = Co; d.Zi = 1;
    StridedP ap{W, 1, ldw, 0, 0, Ci, Co};            // A(m=ci,k=co) = W[co*ldw + ci]
    XContigP bp{dY, (long)N, sdYb, 0, N, Co, nullptr, nullptr, 0, nullptr, nullptr};
    EpiP ep = epi_default(dX, N);
    ep.sCo = sdXb;
    ep.beta = beta;
    return run_strided_xcontig(false, d, ap, bp, ep, B, (hipStream_t)stream);
}

int rcot_conv1x1_wgrad(const float* dY, long sdYb, const float* X, long sXb, float* dW, long ldw, int B, int Ci,
                       int Co, int N, const float* ln_mu, const float* ln_rs, const float* ln_w, const float* ln_b,
                       float beta, float* ws, size_t ws_bytes, int prec, void* stream) {
    if (!dY || !X || !dW || B <= 0 || Ci <= 0 || Co <= 0 || N <= 0) return RCOT_EINVAL;
    if ((N & 15) || (sdYb & 3) || (sXb & 3) || !al16(dY) || !al16(X)) return RCOT_EINVAL;
    if (ln_mu && (!ln_rs || !ln_w || !ln_b || !al16(ln_mu) || !al16(ln_rs))) return RCOT_EINVAL;
    GemmDims d{};
    d.M = Co; d.N = Ci; d.K = B * N; d.Zi = 1;        // batch folded into the reduction
    KContigP ap{dY, (long)N, 0, 0, Co, d.K, N, sdYb, nullptr, nullptr, 0, nullptr, nullptr};
    KContigP bp{X, (long)N, 0, 0, Ci, d.K, N, sXb, ln_mu, ln_rs, (long)N, ln_w, ln_b};
    EpiP ep = epi_default(dW, ldw);
    ep.beta = beta;
    const int rc = try_gemm_nt_glds(Co, Ci, d.K, 1, 1, dY, N, 0, 0, X, N, 0, 0, N, sdYb, sXb, ln_mu, ln_rs, N, ln_w, ln_b, ep,
                                    ws, ws_bytes, (hipStream_t)stream, prec);
    if (rc != NOT_ELIGIBLE) return rc;
    return run_kcontig(d, ap, bp, ep, 1, ws, ws_bytes, (hipStream_t)stream);
}

int rcot_conv_pcm_wgrad(const float* dZp, const float* Xp, long ld, int N, int Wp, int Co, int Ci, float* dW, float beta, float* ws,
                        size_t ws_bytes, int prec, void* stream) {
    if (!dZp || !Xp || !dW || !ws || Co <= 0 || Ci <= 0 || N <= 0 || (N & 15) || (ld & 3) || Wp < 3 || !al16(dZp) || !al16(Xp))
        return RCOT_EINVAL;
    EpiP ep = epi_default(dW, 9L * Ci);
    ep.beta = beta;
    const int rc = try_gemm_nt_glds(Co, 9 * Ci, N, 1, 1, dZp, ld, 0, 0, Xp, ld, 0, 0, 0, 0, 0, nullptr, nullptr, 0, nullptr, nullptr, ep, ws,
                                    ws_bytes, (hipStream_t)stream, prec, nullptr, nullptr, Wp);
    return rc == NOT_ELIGIBLE ? RCOT_EUNSUPPORTED : rc;
}

int rcot_conv1x1_wgrad_slabs(const float* dY, long sdYb, const float* X, long sXb, int B, int Ci, int Co, int N,
                             const float* ln_mu, const float* ln_rs, const float* ln_w, const float* ln_b, float* ws,
                             size_t ws_bytes, int prec, int* S, int* ldws, void* stream) {
    if (!dY || !X || !ws || !S || !ldws || B <= 0 || Ci <= 0 || Co <= 0 || N <= 0) return RCOT_EINVAL;
    if ((N & 15) || (sdYb & 3) || (sXb & 3) || !al16(dY) || !al16(X) || !al16(ws)) return RCOT_EINVAL;
    if (ln_mu && (!ln_rs || !ln_w || !ln_b || !al16(ln_mu) || !al16(ln_rs))) return RCOT_EINVAL;
    EpiP ep{};
    const int rc = try_gemm_nt_glds(Co, Ci, B * N, 1, 1, dY, N, 0, 0, X, N, 0, 0, N, sdYb, sXb, ln_mu, ln_rs, N, ln_w, ln_b, ep, ws,
                                    ws_bytes, (hipStream_t)stream, prec, S, ldws);
    return rc == NOT_ELIGIBLE ? RCOT_EUNSUPPORTED : rc;
}

int rcot_conv1x1_dgrad_wgrad_slabs(const float* WP, long ldp, const void* WPs, const float* dY, long sdYb, float* dX, long sdXb,
                                   const float* X, long sXb, int B, int Ci, int Co, int N, const float* ln_mu, const float* ln_rs,
                                   const float* ln_w, const float* ln_b, float* ws, size_t ws_bytes, float* ws_slabs,
                                   size_t ws_slabs_bytes, int prec, int* S, int* ldws, void* stream) {
    if (!WP || !dY || !dX || !X || !ws_slabs || !S || !ldws || B <= 0 || Ci <= 0 || Co <= 0 || N <= 0) return RCOT_EINVAL;
    if ((N & 15) || (sdYb & 3) || (sXb & 3) || (sdXb & 3) || (ldp & 3) || !al16(dY) || !al16(X) || !al16(dX) || !al16(ws_slabs) || !al16(WP))
        return RCOT_EINVAL;
    if (ln_mu && (!ln_rs || !ln_w || !ln_b || !al16(ln_mu) || !al16(ln_rs))) return RCOT_EINVAL;
    if (prec != RCOT_PREC_BF16X3 || !WPs || B > 65535) return RCOT_EUNSUPPORTED;
    const int rc = pair_dgrad_wgrad_x3(WP, ldp, WPs, dY, sdYb, dX, sdXb, X, sXb, B, Ci, Co, N, ln_mu, ln_rs, ln_w, ln_b, ws, ws_bytes,
                                       ws_slabs, ws_slabs_bytes, S, ldws, (hipStream_t)stream);
    return rc == NOT_ELIGIBLE ? RCOT_EUNSUPPORTED : rc;
}

int rcot_bmm_nn(const float* A, long lda, long sAo, long sAi, int transA, const float* Bm, long ldb, long sBo,
                long sBi, float* C, long ldc, long sCo, long sCi, const float* R, long ldr, long sRo, long sRi,
                const float* rowscale, long sSo, long sSi, int Zo, int Zi, int M, int N, int K, float beta,
                void* stream) {
    if (!A || !Bm || !C || Zo <= 0 || Zi <= 0 || M <= 0 || N <= 0 || K <= 0) return RCOT_EINVAL;
    if ((ldb & 3) || (sBo & 3) || (sBi & 3) || !al16(Bm)) return RCOT_EINVAL;
    GemmDims d{};
    d.M = M; d.N = N; d.K = K; d.Zi = Zi;
    StridedP ap{A, transA ? 1 : lda, transA ? lda : 1, sAo, sAi, M, K};
    XContigP bp{Bm, ldb, sBo, sBi, N, K, nullptr, nullptr, 0, nullptr, nullptr};
    EpiP ep = epi_default(C, ldc);
    ep.sCo = sCo; ep.sCi = sCi;
    ep.R = R; ep.ldr = ldr; ep.sRo = sRo; ep.sRi = sRi;
    ep.rowscale = rowscale; ep.sSo = sSo; ep.sSi = sSi;
    ep.beta = beta;
    return run_strided_xcontig(!transA, d, ap, bp, ep, Zo * Zi, (hipStream_t)stream);
}

int rcot_bmm_nt(const float* A, long lda, long sAo, long sAi, const float* Bm, long ldb, long sBo, long sBi,
                float* C, long ldc, long sCo, long sCi, int Zo, int Zi, int M, int N, int K, float* ws,
                size_t ws_bytes, int prec, void* stream) {
    if (!A || !Bm || !C || Zo <= 0 || Zi <= 0 || M <= 0 || N <= 0 || K <= 0) return RCOT_EINVAL;
    if ((K & 3) || (lda & 3) || (ldb & 3) || (sAo & 3) || (sAi & 3) || (sBo & 3) || (sBi & 3) || !al16(A) || !al16(Bm))
        return RCOT_EINVAL;
    GemmDims d{};
    d.M = M; d.N = N; d.K = K; d.Zi = Zi;
    KContigP ap{A, lda, sAo, sAi, M, K, 0, 0, nullptr, nullptr, 0, nullptr, nullptr};
    KContigP bp{Bm, ldb, sBo, sBi, N, K, 0, 0, nullptr, nullptr, 0, nullptr, nullptr};
    EpiP ep = epi_default(C, ldc);
    ep.sCo = sCo; ep.sCi = sCi;
    const int rc = try_gemm_nt_glds(M, N, K, Zo, Zi, A, lda, sAo, sAi, Bm, ldb, sBo, sBi, 0, 0, 0, nullptr, nullptr, 0, nullptr,
                                    nullptr, ep, ws, ws_bytes, (hipStream_t)stream, prec);
    if (rc != NOT_ELIGIBLE) return rc;
    return run_kcontig(d, ap, bp, ep, Zo * Zi, ws, ws_bytes, (hipStream_t)stream);
}

int rcot_bmm_nt_slabs(const float* A, long lda, long sAo, long sAi, const float* Bm, long ldb, long sBo, long sBi, int Zo, int Zi,
                      int M, int N, int K, float* ws, size_t ws_bytes, int prec, int* S, int* ldws, void* stream) {
    if (!A || !Bm || !ws || !S || !ldws || Zo <= 0 || Zi <= 0 || M <= 0 || N <= 0 || K <= 0) return RCOT_EINVAL;
    if ((K & 3) || (lda & 3) || (ldb & 3) || (sAo & 3) || (sAi & 3) || (sBo & 3) || (sBi & 3) || !al16(A) || !al16(Bm) || !al16(ws))
        return RCOT_EINVAL;
    EpiP ep{};
    const int rc = try_gemm_nt_glds(M, N, K, Zo, Zi, A, lda, sAo, sAi, Bm, ldb, sBo, sBi, 0, 0, 0, nullptr, nullptr, 0, nullptr,
                                    nullptr, ep, ws, ws_bytes, (hipStream_t)stream, prec, S, ldws);
    return rc == NOT_ELIGIBLE ? RCOT_EUNSUPPORTED : rc;
}

int rcot_linear_fwd(const float* X, const float* W, const float* bias, float* Y, int B, int in, int out, float lrelu,
                    float* ws, size_t ws_bytes, void* stream) {
    if (!X || !W || !Y || B <= 0 || in <= 0 || out <= 0) return RCOT_EINVAL;
    GemmDims d{};
    d.M = out; d.N = B; d.K = in; d.Zi = 1;
    StridedP ap{W, (long)in, 1, 0, 0, out, in};
    StridedP bp{X, (long)in, 1, 0, 0, B, in};        // B(k,n) = X[n*in + k]
    EpiP ep = epi_default(Y, out);
    ep.transC = 1;
    ep.bias = bias;
    ep.lrelu = lrelu;
    return run_strided2(true, d, ap, bp, ep, ws, ws_bytes, (hipStream_t)stream);
}

int rcot_linear_dgrad(const float* dY, const float* W, float* dX, int B, int in, int out, float* ws, size_t ws_bytes,
                      void* stream) {
    if (!dY || !W || !dX || B <= 0 || in <= 0 || out <= 0) return RCOT_EINVAL;
    GemmDims d{};
    d.M = in; d.N = B; d.K = out; d.Zi = 1;
    StridedP ap{W, 1, (long)in, 0, 0, in, out};      // A(m=i,k=o) = W[o*in + i]
    StridedP bp{dY, (long)out, 1, 0, 0, B, out};     // B(k=o,n=b) = dY[b*out + o]
    EpiP ep = epi_default(dX, in);
    ep.transC = 1;
    return run_strided2(false, d, ap, bp, ep, ws, ws_bytes, (hipStream_t)stream);
}

int rcot_linear_wgrad(const float* dY, const float* X, float* dW, int B, int in, int out, float beta, void* stream) {
    if (!dY || !X || !dW || B <= 0 || in <= 0 || out <= 0) return RCOT_EINVAL;
    GemmDims d{};
    d.M = out; d.N = in; d.K = B; d.Zi = 1;
    StridedP ap{dY, 1, (long)out, 0, 0, out, B};     // A(m=o,k=b) = dY[b*out + o]
    EpiP ep = epi_default(dW, in);
    ep.beta = beta;
    if ((in & 3) == 0 && al16(X)) {
        XContigP bp{X, (long)in, 0, 0, in, B, nullptr, nullptr, 0, nullptr, nullptr};
        return run_strided_xcontig(false, d, ap, bp, ep, 1, (hipStream_t)stream);
    }
    StridedP bp{X, 1, (long)in, 0, 0, in, B};        // B(k=b,n=i) = X[b*in + i]
    plan_splitk(d, 1, nullptr, 0);
    // n-contiguous B through the scalar k-fast loader would be uncoalesced; this path is only the unaligned fallback
    return launch_gemm_cfg<CfgS, AStrM<CfgS>, StridedP, BStrK<CfgS>, StridedP, true>(d, ap, bp, ep, 1, (hipStream_t)stream);
}

}  // extern "C"
