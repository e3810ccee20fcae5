"""GPU tier: WHICH kernel the host layer of the four GEMM units picks (csrc/gemm_glds.hip, gemm_x3.hip, gemm_x3w.hip, gemm_nt_glds.hip),
branch by branch, at the smallest shape that reaches the branch.  Every case calls a public entry point through the backend (or
ctypes, as tests/test_kernels_gpu.py does), reads rcot_last_kernel() and compares it with the symbol written out here — read off the
dispatch code by hand, not computed by it — and checks the result against the fp64 statements of tests/host_double.py at the bar the
neighbouring tests hold that arithmetic to (2e-5 exact fp32 and bf16x6, 4e-5 bf16x3), on guard-banded buffers (tests/guarded.py).
Where an entry point reports its split (slabs_S, slabs_ld of the slab-returning weight gradients) that is asserted too.

The split factors asserted below follow from the two-term cost model of nt_configure evaluated by hand: a 512-pixel reduction
(32 slabs of 16) may split 1, 2, 4 or 8 ways, one tile on 640 slots is MFMA-bound by four orders of magnitude in every arithmetic, so the
largest candidate wins: S = 8, 64 pixels each.  The paired launch reduces 4096 pixels (256 slabs, up to 64 pieces) on 320 slots in the
bf16x3 model: one tile (128x128, 128x96, 96x128, 64x128) 5.8 / 4.5 / 4.5 / 3.2 us at 64 pieces against 6.9 / 5.3 / 5.3 / 3.7 us at 32:
S = 64; five tiles (128x320, 64x320) 9.7 / 5.6 us at 32 against 11.6 / 6.6 us at 64 and 10.5 / 6.0 us at 16: S = 32.

Left to the machine-code fingerprints (profiles/gemm_host_layer_fingerprints.txt): the second ring depth of each gemm_x3_kernel form —
the streaming depth of the 128-column tiles needs more than 256 of their workgroups (>= 32 MiB of output), the deep one of the
256-column tiles has no small shape at all (they are chosen from 1024 column tiles up) — and its LayerNorm forms, which differ from
the plain ones run here in the epilogue only."""
import ctypes

import pytest
import torch

from conftest import relerr
from guarded import GuardSet, poison_workspaces
from test_kernels_gpu import DBL, T, TOL, X3_TOL, _last_kernel, both, hip  # noqa: F401  (hip: the module-scoped backend fixture)

pytestmark = pytest.mark.gpu

PRECS = {"fp32": 0, "bf16x3": 1, "bf16x6": 2}            # RCOT_PREC_* of include/rcot_hip.h


class _prec:
    """the backend in one arithmetic for the duration"""
    def __init__(self, be, name):
        self.be, self.prec = be, PRECS[name]

    def __enter__(self):
        self.old, self.be.prec = self.be.prec, self.prec
        return self.be

    def __exit__(self, *exc):
        self.be.prec = self.old


def _at(A):
    """A [Z, M, K] as the transposed, zero-padded operand of rcot_gemm_kmajor: [Z, 1, ceil16(K), ceil4(M)]"""
    Z, M, Kk = A.shape
    At = torch.zeros(Z, 1, (Kk + 15) // 16 * 16, (M + 3) // 4 * 4)
    At[:, 0, :Kk, :M] = A.transpose(1, 2)
    return At


# ----------------------------------------------------------------------------- pixel-reduction family (gemm_nt_glds.hip)
# (M, N) -> cfg by the least padded area among 128x128, 128x96, 96x128, 128x64, 64x128, 64x64 (each shape below fits its own tile
# exactly); <TM, TN, WM, WN> of the tile, and the COOP form the split arithmetics have for it (0: none)
NT_TILES = {(128, 128): ("2, 2, 2, 2", 0), (128, 96): ("1, 3, 4, 1", 1), (96, 128): ("3, 1, 1, 4", 2),
            (128, 64): ("1, 2, 4, 1", 1), (64, 128): ("2, 1, 1, 4", 2), (64, 64): ("1, 1, 2, 2", 0)}


@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "bf16x6"])
@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("M,N", list(NT_TILES))
def test_pixel_reduction_tile_and_arithmetic(hip, M, N, ln, prec):
    """rcot_conv1x1_wgrad and rcot_conv1x1_wgrad_slabs of a Co = M, Ci = N projection over 2 x 16x16 pixels: tile by cfg, LayerNorm
    operand, arithmetic, and the cooperative form under both settings of rcot_debug_nt_coop (cfg 1..4; exact fp32 has none)."""
    B, P = 2, 256
    tile, coop_form = NT_TILES[(M, N)]
    x3, x6 = ("false", "false") if prec == "fp32" else ("true", "true" if prec == "bf16x6" else "false")

    def fn(be, dY, X, dW, mu, rs, lw, lb):
        if ln:
            be.ln_stats(X, mu, rs)
        be.conv1x1_wgrad(dY, X, dW, ln=(mu, rs, lw, lb) if ln else None, beta=0.0)
    arrs = [T(2, B, M, P), T(3, B, N, P) + 0.5, torch.zeros(M, N), torch.zeros(B, P), torch.zeros(B, P), 1 + 0.1 * T(4, N), 0.1 * T(5, N)]
    with _prec(hip, prec) as be:
        try:
            for mask in ((3, 0) if coop_form else (3,)):
                assert be.L.rcot_debug_nt_coop(mask) == 0
                coop = coop_form if (mask and prec != "fp32") else 0
                want = f"gemm_nt_kernel<{tile}, {'true' if ln else 'false'}, {x3}, {x6}, {coop}>"
                cpu, gpu = both(be, fn, arrs, [2])
                assert _last_kernel(be) == want
                dY, X, _, mu, rs, lw, lb = gpu
                d = be.conv1x1_wgrad_slabs(dY, X, gpu[2], ln=(mu, rs, lw, lb) if ln else None)
                assert d is not None and _last_kernel(be) == want
                S, ld = d[1], d[4]
                assert (S, ld) == (8, N)
                torch.cuda.synchronize()
                slabs = be._ws_slabs[:S * M * ld].view(S, M, ld).double().sum(0)[:, :N]
                e = relerr(slabs, cpu[2])
                assert e < (X3_TOL if prec == "bf16x3" else TOL), e
        finally:
            be.L.rcot_debug_nt_coop(-1)


# ----------------------------------------------------------------------------- K-major exact fp32 (gemm_glds.hip)
@pytest.mark.parametrize("Z,M,Kk,N,ln,want", [
    (6, 48, 48, 4096, False, "gemm_xx_kernel<64, 128, 1, 4, false>"),       # 192 big tiles (the threshold), M <= 64
    (6, 96, 48, 4096, False, "gemm_xx_kernel<96, 128, 1, 4, false>"),       # ... 96 rows pad less than 128
    (6, 128, 48, 4096, False, "gemm_xx_kernel<128, 128, 2, 2, false>"),
    (2, 64, 512, 256, False, "gemm_xx_kg_kernel"),                          # 4 big tiles; K >= 512 on 8 workgroups of 64x64
    (2, 64, 48, 256, False, "gemm_xx_kernel<64, 64, 2, 2, false>"),
    (2, 64, 48, 256, True, "gemm_xx_kernel<64, 64, 2, 2, true>")])
def test_kmajor_fp32_tile_rule(hip, Z, M, Kk, N, ln, want):
    def fn(be, At, Bm, C, R, mu, rs, lw, lb):
        if ln:
            be.ln_stats(Bm[:, 0], mu, rs)
        be.gemm_kmajor(At, Bm, C, M, Kk, R=R, ln=(mu, rs, lw, lb) if ln else None)
    arrs = [_at(T(1, Z, M, Kk, scale=0.1)), T(2, Z, 1, Kk, N), torch.zeros(Z, 1, M, N), T(3, Z, 1, M, N), torch.zeros(Z, N),
            torch.zeros(Z, N), 1 + 0.1 * T(4, Kk), 0.1 * T(5, Kk)]
    with _prec(hip, "fp32") as be:
        both(be, fn, arrs, [2])
        assert _last_kernel(be) == want


@pytest.mark.parametrize("M,want", [(48, "gemm_xx_stats_kernel<64>"), (96, "gemm_xx_stats_kernel<96>")])
def test_kmajor_stats_tile(hip, M, want):
    Z, Kk, N = 2, 48, 128

    def fn(be, At, Bm, C, R, mu, rs):
        be.gemm_kmajor_stats(At, Bm, C, M, Kk, R, (mu, rs))
    R = T(3, Z, 1, M, N) + 2.0 * T(13, Z, 1, 1, N)
    with _prec(hip, "fp32") as be:
        both(be, fn, [_at(T(1, Z, M, Kk, scale=0.1)), T(2, Z, 1, Kk, N), torch.zeros(Z, 1, M, N), R, torch.zeros(Z, N), torch.zeros(Z, N)],
             [2, 4, 5])
        assert _last_kernel(be) == want


@pytest.mark.parametrize("Z,M0,N,want", [(2, 96, 256, "gemm_xx_multi_kernel<64, 64, 2, 2>"), (6, 48, 4096, "gemm_xx_multi_kernel<64, 128, 1, 4>"),
                                         (6, 96, 4096, "gemm_xx_multi_kernel<96, 128, 1, 4>"), (6, 128, 4096, "gemm_xx_multi_kernel<128, 128, 2, 2>")])
def test_kmajor_multi_tile_rule(hip, Z, M0, N, want):
    """three products in one launch: the tile of the FIRST product's rows (48-row products beside it), never the k-group kernel"""
    Kk, M1 = 48, 48

    def fn(be, At0, B0, C0, At1, B1, C1, R1, s1, At2, B2, C2):
        items = [(At0, B0, C0, M0, Kk, None, None), (At1, B1, C1, M1, Kk, R1, s1), (At2, B2, C2, M1, Kk, None, None)]
        if be is DBL:
            for At, Bm, C, M, k, R, s in items:
                be.gemm_kmajor(At, Bm, C, M, k, R=R, rowscale=s)
        else:
            assert be.gemm_kmajor_multi(items)
    arrs = [_at(T(1, Z, M0, Kk, scale=0.1)), T(2, Z, 1, Kk, N), torch.zeros(Z, 1, M0, N),
            _at(T(3, Z, M1, Kk, scale=0.1)), T(4, Z, 1, Kk, N), torch.zeros(Z, 1, M1, N), T(5, Z, 1, M1, N), T(6, Z, 1, M1),
            _at(T(7, Z, M1, Kk, scale=0.1)), T(8, Z, 1, Kk, N), torch.zeros(Z, 1, M1, N)]
    with _prec(hip, "fp32") as be:
        both(be, fn, arrs, [2, 5, 10])
        assert _last_kernel(be) == want


# ----------------------------------------------------------------------------- K-major split bf16, no pack (gemm_x3.hip)
@pytest.mark.parametrize("Z,M,Kk,N,res,want", [
    (2, 48, 48, 256, True, "gemm_x3_kernel<2, 1, 1, false, 6>"),            # 64-row tile, ring as deep as a 6-bit vmcnt counts
    (32, 48, 32, 4096, False, "gemm_x3_kernel<2, 1, 2, false, 3>"),         # N / 128 * Z = 1024 columns: the 256-column form, 512 workgroups
    (2, 96, 48, 256, True, "gemm_x3_kernel<1, 3, 1, false, 8>"),
    (2, 128, 48, 256, True, "gemm_x3_kernel<1, 4, 1, false, 8>"),
    (32, 128, 32, 4096, False, "gemm_x3_kernel<2, 2, 2, false, 3>"),
    (2, 96, 256, 256, True, "gemm_x3_kernel<1, 3, 1, false, 8>")])          # 16 slabs on 4 tiles: two K pieces and x3_reduce_kernel
def test_kmajor_split_bf16_forms(hip, Z, M, Kk, N, res, want):
    def fn(be, At, Bm, C, R):
        be.gemm_kmajor(At, Bm, C, M, Kk, R=R if res else None)
    arrs = [_at(T(1, Z, M, Kk, scale=0.1)), T(2, Z, 1, Kk, N), torch.zeros(Z, 1, M, N), T(3, Z, 1, M, N) if res else None]
    with _prec(hip, "bf16x3") as be:
        both(be, fn, arrs, [2])
        assert _last_kernel(be) == want


# ----------------------------------------------------------------------------- producer / consumer kernel (gemm_x3w.hip)
@pytest.mark.parametrize("B,Ci,N,ln,res,six,lnc,want", [
    (2, 48, 128, False, False, False, False, "x3p_kernel<false, false, 1, 3, false, false, 2>"),     # N % 256 != 0: the 128-column tile
    (2, 48, 128, True, True, False, False, "x3p_kernel<true, true, 1, 3, false, false, 2>"),
    (2, 48, 256, True, True, False, False, "x3p_kernel<true, true, 2, 4, false, false, 2>"),
    (2, 48, 256, True, False, False, True, "x3p_kernel<true, false, 2, 4, false, true, 2>"),         # ln_compute: statistics made here
    (48, 48, 256, False, False, False, False, "x3p_kernel<false, false, 1, 3, false, false, 2>"),    # 48 tiles of 256 columns: narrow by occupancy
    (2, 256, 256, False, True, False, False, "x3p_kernel<false, false, 2, 4, false, false, 2>"),     # 16 slabs on 2 tiles: split, addend in the reduce
    (2, 48, 128, False, False, True, False, "x3p_kernel<false, false, 1, 3, false, false, 3>"),      # three-term packs
    (2, 48, 256, False, True, True, False, "x3p_kernel<false, true, 2, 3, false, false, 3>")])
def test_producer_consumer_forms(hip, B, Ci, N, ln, res, six, lnc, want):
    Co = 96

    def fn(be, W, X, Y, mu, rs, lw, lb, R, WT, WP, WTf, c12, WTs, WPs, WTfs):
        sp3 = (WTs, WPs, WTfs if ln else None)
        be.pack_weight(W, WT, WP, (lw, lb, WTf, c12) if ln else None, None if six else sp3, sp3 if six else None)
        z, v = (lambda t: t.view(1, 1, *t.shape).expand(B, 1, -1, -1)), (lambda t: t.unsqueeze(1))
        kw = dict(R=v(R) if res else None, ln=(mu, rs, lw, lb) if ln else None, beta=1.0 if res else 0.0)
        if be is DBL:
            if ln:
                be.ln_stats(X, mu, rs)
            be.gemm_kmajor(z(WT), v(X), v(Y), Co, Ci, **kw)
            return
        if ln and not lnc:
            be.ln_stats(X, mu, rs)
        assert be.gemm_kmajor(z(WT), v(X), v(Y), Co, Ci, fold=(z(WTf), c12) if ln else None, split=WTfs if ln else WTs, ln_compute=lnc, **kw)
    st, sp = DBL.pack_shapes(Co, Ci)
    sf, sc = DBL.fold_shapes(Co, Ci)
    ss, sq = (DBL.split6_shapes if six else DBL.split_shapes)(Co, Ci)
    X = T(2, B, Ci, N) + 1.0 * (1 + 0.2 * T(12, B, 1, N))          # |mean| / spread = 1 per pixel, as the neighbouring ln_compute test
    arrs = [T(1, Co, Ci, scale=0.1), X, T(8, B, Co, N), torch.zeros(B, N), torch.zeros(B, N), 1 + 0.1 * T(3, Ci), 0.1 * T(4, Ci),
            T(5, B, Co, N), torch.zeros(*st), torch.zeros(*sp), torch.zeros(*sf), torch.zeros(*sc), torch.zeros(*ss), torch.zeros(*sq),
            torch.zeros(*ss)]
    with _prec(hip, "bf16x6" if six else "bf16x3") as be:
        cpu, gpu = both(be, fn, arrs, [2])
        assert _last_kernel(be) == want
        if lnc:
            e_mu = float((gpu[3].double().cpu() - cpu[3]).abs().max() / cpu[3].abs().max())
            e_rs = float((gpu[4].double().cpu() / cpu[4] - 1).abs().max())
            assert e_mu < 2e-6 and e_rs < 2e-5 * 2, (e_mu, e_rs)


# ----------------------------------------------------------------------------- paired data / weight gradient (gemm_x3w.hip)
@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("Co,Ci,tile,S", [(128, 128, "2, 2, 2, 2", 64), (128, 96, "1, 3, 4, 1", 64), (96, 128, "3, 1, 1, 4", 64),
                                          (128, 320, "1, 2, 4, 1", 32), (64, 128, "2, 1, 1, 4", 64), (64, 320, "1, 1, 2, 2", 32)])
def test_paired_gradients_tile(hip, Co, Ci, tile, S, ln):
    """rcot_conv1x1_dgrad_wgrad_slabs at 4 x 32x32 pixels: the weight-gradient half takes the tile of (Co, Ci) — 320 columns pad
    least in 64-column tiles, which is how a data gradient of more than 64 rows reaches cfg 3 and 5; S and ld as reported."""
    B, N = 4, 1024
    W, dY, X = T(1, Co, Ci, scale=0.1), T(2, B, Co, N), T(3, B, Ci, N) + 0.5
    lw, lb = 1 + 0.1 * T(4, Ci), 0.1 * T(5, Ci)
    with _prec(hip, "bf16x3") as be:
        gs = GuardSet("cuda")
        poison_workspaces(be)
        Wg, dYg, Xg, lwg, lbg = (gs.tensor(t) for t in (W, dY, X, lw, lb))
        WT, WP = (gs.full(s, 0.0) for s in be.pack_shapes(Co, Ci))
        (st,), (sp,) = be.split_shapes(Co, Ci)
        WTs, WPs = gs.full((st,), 0.0), gs.full((sp,), 0.0)
        be.pack_weight(Wg, WT, WP, None, (WTs, WPs, None))
        mu, rs = gs.full((B, N), 0.0), gs.full((B, N), 1.0)
        be.ln_stats(Xg, mu, rs)
        dX, gW = gs.full((B, Ci, N), float("nan")), gs.full((Co, Ci), 0.0)
        d = be.conv1x1_dgrad_wgrad_slabs(Wg, dYg, dX, Xg, gW, ln=(mu, rs, lwg, lbg) if ln else None, packed=(WT, WP, None, (WTs, WPs, None)))
        assert d is not None
        assert _last_kernel(be) == f"x3p_nt_pair_kernel<{tile}, {'true' if ln else 'false'}>"
        assert (d[1], d[4]) == (S, Ci)
        torch.cuda.synchronize()
        Xd = X.double()
        if ln:
            m = Xd.mean(1, keepdim=True)
            Xd = (Xd - m) * (Xd.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt() * lw.double().view(1, Ci, 1) + lb.double().view(1, Ci, 1)
        e1 = relerr(dX, torch.einsum("oc,bon->bcn", W.double(), dY.double()))
        e2 = relerr(be._ws_slabs[:S * Co * Ci].view(S, Co, Ci).double().sum(0), torch.einsum("bon,bcn->oc", dY.double(), Xd))
        assert e1 < X3_TOL and e2 < X3_TOL, (e1, e2)
        gs.check()


# ----------------------------------------------------------------------------- rcot_conv_pcm (gemm_x3w.hip: launch_conv)
@pytest.mark.parametrize("narrow,want", [(False, "x3p_kernel<false, false, 2, 4, true, false>"), (True, "x3p_kernel<false, false, 1, 3, true, false>")])
def test_conv_pcm_column_forms(hip, narrow, want):
    """a k3s1p1 convolution over 2 x 16x16 planes: 864 padded pixels are N = 1024 columns as the backend rounds them (256-column
    tiles) and N = 896 = 7 x 128 rounded to the kernel's own granule (the 128-column form; called as the backend calls it)."""
    import torch.nn.functional as F
    B, Ci, Co, H, Wd = 2, 64, 128, 16, 16
    Wt, X, bias = T(1, Co, Ci, 3, 3, scale=0.05), T(2, B, Ci, H, Wd), T(3, Co, scale=0.1)
    ref = F.leaky_relu(F.conv2d(X.double(), Wt.double(), bias.double(), 1, 1), 0.2)
    gs = GuardSet("cuda")
    poison_workspaces(hip)
    pack = hip.conv_pcm_pack(gs.tensor(Wt, "W"), "fwd")
    Xg, bg, Y = gs.tensor(X, "X"), gs.tensor(bias, "bias"), gs.full((B, Co, H, Wd), float("nan"), name="Y")
    if not narrow:
        hip.conv_pcm_fwd(Xg, pack, bg, Y, 3, lrelu=0.2)
    else:
        g = hip._pcm_geom(B, H, Wd, Co, H, Wd, "same")
        N, G, Wp = g["N"] - 128, g["G"], g["Wp"]
        assert N % 256 == 128 and B * g["Ps"] <= N and G >= Wp + 1
        ldb = N + 2 * G
        buf = gs.full((Ci * ldb + 64,), 0.0, name="padded planes")
        colmap = gs.tensor(g["colmap"][:N // 4].contiguous(), "colmap")
        taps = [(ky - 1) * Wp + (kx - 1) for ky in range(3) for kx in range(3)]
        assert hip.L.rcot_conv_pcm_prep(Xg.data_ptr(), buf.data_ptr() + 4 * G, ldb, B, Ci, H, Wd, 0, hip._st()) == 0
        assert hip.L.rcot_conv_pcm(pack.data_ptr(), Co, Ci * 9, buf.data_ptr() + 4 * G, ldb, N, (ctypes.c_int * 9)(*taps), 9, bg.data_ptr(), 0.2,
                                   colmap.data_ptr(), Y.data_ptr(), H * Wd, hip.ws.data_ptr(), hip.ws_bytes, hip._st()) == 0
    assert _last_kernel(hip) == want
    torch.cuda.synchronize()
    e = relerr(Y, ref)
    assert e < X3_TOL, e
    gs.check()
