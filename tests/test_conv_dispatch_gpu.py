"""GPU tier: WHICH store path the dense-convolution engine takes (csrc/conv_ops.hip, the split-K reducers of csrc/gemm_core.h), branch by
branch, at the smallest shape that reaches the branch — the companion of tests/test_gemm_dispatch_gpu.py for rcot_conv2d_fwd / _dgrad /
_wgrad.  Every case calls the entry point through the backend on guard-banded buffers (tests/guarded.py) with a NaN-filled output and
NaN-filled workspaces, and asserts
  * the main kernel (rcot_last_kernel) against the symbol written out here,
  * the split-K reducer, or the absence of one (rcot_profile_begin / _end: exactly the named kernel among the launches),
  * the split factor S, from the workspace itself: the engine writes S slabs of the GEMM's M x N (x 4 parity classes) floats at its
    start and nothing else, so S x numel(output) floats of it are finite afterwards and none in the unsplit form,
  * the result against the fp64 statements of tests/host_double.py at TOL (2e-5 of max|ref|: the exact-fp32 chain, K <= 1024),
  * the masked store (mask / mslope: LeakyReLU's backward folded into the store) against the double AND, bit for bit, against the
    unmasked launch followed by lrelu_bwd — the mask does not enter the split plan and the store claims lrelu_bwd_kernel's expression.

Symbols, S and reducers are read off the dispatch code by hand (launch_conv_*_lean and the three entry points of conv_ops.hip;
plan_gemm, cut_k, reduce4_ok and launch_splitk_reduce of gemm_core.h), with 768 target workgroups, BK = 16 and the 256 MiB workspace.
GEMM view: forward M = Co, N = B OH OW, K = Ci k k; data gradient M = Ci, N = B H W, K = Co k k (k4s2: four parity classes of
N = B H/2 W/2, K = 4 Co); weight gradient M = Co, N = Ci k k, K = B OH OW.  blocks = ceil(M / 64) ceil(N / 64) Z (no case here plans
the 128 x 128 tile: fewer than 384 of them, or M = 64), S = min(ceil(768 / blocks), ceil(K / 16) / 2), then whole BK tiles per piece.
Partial slabs are stored 16 bytes at a time (epilogue_vec) when N % 4 == 0, else element by element; the reducer is
splitk_reduce_few4_kernel for S <= 8 when the store is plain (no residual, no parity scatter, pixel count and N multiples of 4),
splitk_reduce_few_kernel for S <= 8 otherwise, splitk_reduce_kernel above 8 slabs."""
import ctypes
import re
import time

import pytest
import torch

from conftest import relerr
from guarded import GuardSet, poison_workspaces
from rcot_amd.lib import RcotKernelError
from test_kernels_gpu import DBL, T, TOL, _last_kernel, both, hip  # noqa: F401  (hip: the module-scoped backend fixture)

pytestmark = pytest.mark.gpu

FEW4, FEW, GENERAL = "splitk_reduce_few4_kernel", "splitk_reduce_few_kernel", "splitk_reduce_kernel"
SLOPE = 0.2
NAN = float("nan")


def _out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def _mask(seed, *shape):
    """a GIVEN mask (no kink of a computed one nearby): seeded normal values with exact 0.0, -0.0 and 1e-30 on every seventh element
    (every parity class, every column phase of a 16-byte store), on the last eight pixels of the last image in every channel (the
    ragged last tile of the GEMM's N axis) and on the 2 x 2 corners of every plane (the borders of the four parity classes)"""
    m = T(seed, *shape)
    special = torch.tensor([0.0, -0.0, 1e-30])
    flat = m.view(-1)
    idx = torch.arange(0, flat.numel(), 7)
    flat[idx] = special[torch.arange(idx.numel()) % 3]
    m[-1].view(shape[1], -1)[:, -8:] = special[torch.arange(8) % 3]
    m[:, :, :2, :2] = special[torch.tensor([[0, 1], [2, 0]])]
    m[:, :, -2:, -2:] = special[torch.tensor([[1, 2], [0, 1]])]
    assert (m == 0).sum() > 0 and (m == 1e-30).sum() > 0 and torch.signbit(m[m == 0]).any()
    return m


def _launch(be, call):
    """call() on poisoned workspaces while the launches are collected: (main symbol, reducers that ran, finite floats in the workspace)"""
    buf = ctypes.create_string_buffer(1 << 12)
    poison_workspaces(be)
    torch.cuda.synchronize()
    be.L.rcot_profile_begin()
    try:
        call()
        torch.cuda.synchronize()
    finally:
        be.L.rcot_profile_end(buf, 1 << 12)
    ran = buf.value.decode(errors="replace")
    return _last_kernel(be), sorted(set(re.findall(r"splitk_reduce\w*", ran))), int(torch.isfinite(be.ws).sum())


def _expect(got, kern, S, red, numel):
    sym, reducers, live = got
    assert sym == kern, got
    assert reducers == ([red] if red else []), got
    assert live == (S * numel if S > 1 else 0), (got, S, numel)


def _record(op, case, what, kern, S, red, errs, t0):
    print(f"CONV-STORE-PATH {op} {case} {what}: {kern} S={S} reducer={red or 'none'} "
          + " ".join(f"{k}={v:.2e}" for k, v in errs.items()) + f" wall={1e3 * (time.perf_counter() - t0):.0f}ms")


# ----------------------------------------------------------------------------- forward
# (B, Ci, Co, H, W, k, s, p) -> main kernel, S, reducer of the plain store, reducer with a residual (reduce4_ok refuses R)
FWD = [
    # 64 x 832 tiles = 832 workgroups: unsplit, the lean kernel calls epi_store itself
    ((13, 32, 64, 64, 64, 3, 1, 1), "conv_fwd_lean_kernel<1>", 1, None, None),
    # Co % 128 == 0 and 2 x 512 = 1024 tiles of 64 rows: the 128-row tile, unsplit
    ((2, 8, 128, 128, 128, 3, 1, 1), "conv_fwd_lean_kernel<2>", 1, None, None),
    # N = 17424 = 272 tiles + 16 columns (ragged last tile): 546 blocks -> S = 2 (5 K tiles: pieces of 48 and 24), 1092 >= 1024
    ((1, 8, 128, 132, 132, 3, 1, 1), "conv_fwd_lean_kernel<2>", 2, FEW4, FEW),
    # 96 blocks -> S = 8, pieces of 48 -> 6 slabs; N % 4 == 0: 16-byte slab stores, 16-byte reducer
    ((6, 32, 64, 32, 32, 3, 1, 1), "conv_fwd_lean_kernel<1>", 6, FEW4, FEW),
    # N = 6138: scalar slab stores, scalar reducer
    ((6, 32, 64, 31, 33, 3, 1, 1), "conv_fwd_lean_kernel<1>", 6, FEW, FEW),
    # 8 blocks: S = 18 K tiles / 2 = 9
    ((2, 32, 64, 16, 16, 3, 1, 1), "conv_fwd_lean_kernel<1>", 9, GENERAL, GENERAL),
    # k4s2: 96 blocks, K = 256 -> S = 8 of 32
    ((6, 16, 64, 64, 64, 4, 2, 1), "conv_fwd_lean_kernel<1>", 8, FEW4, FEW),
]
# plain: bias = None, lrelu = 1;  bias + LeakyReLU(0.2);  the same with a residual, which epi_store adds BEFORE the activation
FWD_EPI = ["plain", "bias_lrelu", "bias_lrelu_res"]


def _fwd_case(be, case, epi, gs, Wg=None):
    """one forward case in one epilogue: unmasked, masked, and the unmasked result through lrelu_bwd; returns what ran and the errors"""
    B, Ci, Co, H, W, k, s, p = case
    OH, OW = _out_hw(H, W, k, s, p)
    X, Wt = T(1, B, Ci, H, W), T(2, Co, Ci, k, k, scale=0.05)
    bias = None if epi == "plain" else T(3, Co, scale=0.5)
    lrelu = 1.0 if epi == "plain" else 0.2
    R = T(4, B, Co, OH, OW) if epi == "bias_lrelu_res" else None
    mask = _mask(5, B, Co, OH, OW)
    dbl = lambda t: None if t is None else t.double()
    ref, ref_m = torch.zeros(B, Co, OH, OW, dtype=torch.float64), torch.zeros(B, Co, OH, OW, dtype=torch.float64)
    DBL.conv2d_fwd(dbl(X), dbl(Wt), dbl(bias), ref, s, p, lrelu, 0, dbl(R))
    DBL.conv2d_fwd(dbl(X), dbl(Wt), dbl(bias), ref_m, s, p, lrelu, 0, dbl(R), mask=dbl(mask), mslope=SLOPE)
    g = lambda t, n: None if t is None else gs.tensor(t, n)
    Xg, bg, Rg, mg = g(X, "X"), g(bias, "bias"), g(R, "R"), g(mask, "mask")
    Wg = g(Wt, "W") if Wg is None else Wg(Wt)
    Y, Ym, Y2 = (gs.full((B, Co, OH, OW), NAN, name=n) for n in ("Y", "Y masked", "lrelu_bwd(Y)"))
    plain = _launch(be, lambda: be.conv2d_fwd(Xg, Wg, bg, Y, s, p, lrelu, 0, Rg))
    masked = _launch(be, lambda: be.conv2d_fwd(Xg, Wg, bg, Ym, s, p, lrelu, 0, Rg, mask=mg, mslope=SLOPE))
    be.lrelu_bwd(Y, mg, Y2, slope=SLOPE)
    torch.cuda.synchronize()
    return plain, masked, {"err": relerr(Y, ref), "err_masked": relerr(Ym, ref_m)}, torch.equal(Ym, Y2), Y.numel()


@pytest.mark.parametrize("epi", FWD_EPI)
@pytest.mark.parametrize("case,kern,S,red,red_res", FWD, ids=["-".join(map(str, c[0])) for c in FWD])
def test_forward_store_paths(hip, case, kern, S, red, red_res, epi):
    t0 = time.perf_counter()
    gs = GuardSet("cuda")
    want = red_res if epi == "bias_lrelu_res" else red
    plain, masked, errs, same, numel = _fwd_case(hip, case, epi, gs)
    _record("fwd", case, epi, kern, S, want, errs, t0)
    _expect(plain, kern, S, want, numel)
    _expect(masked, kern, S, want, numel)
    assert errs["err"] < TOL and errs["err_masked"] < TOL, errs
    assert same, "the masked store differs from the unmasked launch + lrelu_bwd"
    gs.check()


def test_forward_unaligned_weight_takes_the_general_engine(hip):
    """forward case 4 with the weight one float into its allocation (not 16-byte aligned): the lean kernel's 16-byte weight loads are
    off, the general engine takes the product in its 64 x 64 tile with the same split plan (S = 6, the plain store: few4)"""
    t0 = time.perf_counter()
    case, kern = (6, 32, 64, 32, 32, 3, 1, 1), "gemm_kernel<TileCfg<64, 64, ..>, ..> (general engine)"
    gs = GuardSet("cuda")

    def shifted(Wt):
        buf = gs.full((Wt.numel() + 1,), NAN, name="W + 1 float")
        v = buf[1:].view(Wt.shape)
        v.copy_(Wt)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v
    plain, masked, errs, same, numel = _fwd_case(hip, case, "bias_lrelu", gs, Wg=shifted)
    _record("fwd", case, "bias_lrelu, W + 4 bytes", kern, 6, FEW4, errs, t0)
    _expect(plain, kern, 6, FEW4, numel)
    _expect(masked, kern, 6, FEW4, numel)
    assert errs["err"] < TOL and errs["err_masked"] < TOL, errs
    assert same
    gs.check()


@pytest.mark.parametrize("cmap", [1, 2])
def test_forward_mask_with_a_shuffled_store_is_refused(hip, cmap):
    """mask together with cmap 1 / 2 (the mask is laid out like the output, the shuffles permute it): RCOT_EINVAL, surfaced as
    RcotKernelError "invalid argument"; nothing is launched, the NaN-filled output and every band stay as they were.  The same call
    without the mask is taken."""
    B, Ci, Co, H, W = 2, 32, 64, 16, 16
    shape = (B, 4 * Co, H // 2, W // 2) if cmap == 1 else (B, Co // 4, 2 * H, 2 * W)
    gs = GuardSet("cuda")
    Xg, Wg = gs.tensor(T(1, B, Ci, H, W), "X"), gs.tensor(T(2, Co, Ci, 3, 3, scale=0.05), "W")
    mg, Y = gs.tensor(_mask(5, *shape), "mask"), gs.full(shape, NAN, name="Y")
    poison_workspaces(hip)
    before = _last_kernel(hip), hip.L.rcot_last_kernel(None, 0)
    with pytest.raises(RcotKernelError, match="rcot_conv2d_fwd: invalid argument"):
        hip.conv2d_fwd(Xg, Wg, None, Y, 1, 1, 1.0, cmap, None, mask=mg, mslope=SLOPE)
    torch.cuda.synchronize()
    assert (_last_kernel(hip), hip.L.rcot_last_kernel(None, 0)) == before
    assert bool(torch.isnan(Y).all()) and not bool(torch.isfinite(hip.ws).any())
    gs.check()
    both(hip, lambda be, X, Wt, Yo: be.conv2d_fwd(X, Wt, None, Yo, 1, 1, 1.0, cmap, None),
         [T(1, B, Ci, H, W), T(2, Co, Ci, 3, 3, scale=0.05), torch.full(shape, NAN)], [2])


# ----------------------------------------------------------------------------- data gradient
# (B, Ci, Co, H, W, k, s, p) of the FORWARD convolution (dX is [B, Ci, H, W]) -> main kernel, S, reducer
DGRAD = [
    # 768 blocks: unsplit
    ((12, 64, 8, 64, 64, 3, 1, 1), "conv_dgrad_lean_kernel<false>", 1, None),
    ((6, 64, 32, 32, 32, 3, 1, 1), "conv_dgrad_lean_kernel<false>", 6, FEW4),
    ((6, 64, 32, 31, 33, 3, 1, 1), "conv_dgrad_lean_kernel<false>", 6, FEW),          # N = 6138: scalar slab stores
    ((2, 64, 64, 16, 16, 3, 1, 1), "conv_dgrad_lean_kernel<false>", 18, GENERAL),     # 8 blocks, 36 K tiles
    # k4s2: four parity classes x 192 tiles = 768 blocks: unsplit, epi_store scatters by parity (cmap 3)
    ((3, 64, 16, 128, 128, 4, 2, 1), "conv_dgrad_lean_kernel<true>", 1, None),
    # 4 x 8 = 32 blocks: S = 16 K tiles / 2 = 8; the parity scatter is never a plain store: the scalar reducer
    ((2, 64, 64, 32, 32, 4, 2, 1), "conv_dgrad_lean_kernel<true>", 8, FEW),
    ((2, 64, 128, 32, 32, 4, 2, 1), "conv_dgrad_lean_kernel<true>", 16, GENERAL),
]


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("case,kern,S,red", DGRAD, ids=["-".join(map(str, c[0])) for c in DGRAD])
def test_data_gradient_store_paths(hip, case, kern, S, red, beta):
    """beta = 1 accumulates onto a seeded dX FIRST and masks the sum: the order of epi_store, of the 16-byte reducer and of the double"""
    t0 = time.perf_counter()
    B, Ci, Co, H, W, k, s, p = case
    OH, OW = _out_hw(H, W, k, s, p)
    dY, Wt, mask = T(1, B, Co, OH, OW), T(2, Co, Ci, k, k, scale=0.05), _mask(5, B, Ci, H, W)
    dX0 = T(6, B, Ci, H, W) if beta else None
    ref, ref_m = ((dX0.double().clone() if beta else torch.zeros(B, Ci, H, W, dtype=torch.float64)) for _ in range(2))
    DBL.conv2d_dgrad(dY.double(), Wt.double(), ref, s, p, beta=beta)
    DBL.conv2d_dgrad(dY.double(), Wt.double(), ref_m, s, p, beta=beta, mask=mask.double(), mslope=SLOPE)
    gs = GuardSet("cuda")
    dYg, Wg, mg = gs.tensor(dY, "dY"), gs.tensor(Wt, "W"), gs.tensor(mask, "mask")
    dX, dXm = ((gs.tensor(dX0, n) if beta else gs.full((B, Ci, H, W), NAN, name=n)) for n in ("dX", "dX masked"))
    dX2 = gs.full((B, Ci, H, W), NAN, name="lrelu_bwd(dX)")
    plain = _launch(hip, lambda: hip.conv2d_dgrad(dYg, Wg, dX, s, p, beta=beta))
    masked = _launch(hip, lambda: hip.conv2d_dgrad(dYg, Wg, dXm, s, p, beta=beta, mask=mg, mslope=SLOPE))
    hip.lrelu_bwd(dX, mg, dX2, slope=SLOPE)
    torch.cuda.synchronize()
    errs = {"err": relerr(dX, ref), "err_masked": relerr(dXm, ref_m)}
    _record("dgrad", case, f"beta={beta:g}", kern, S, red, errs, t0)
    _expect(plain, kern, S, red, dX.numel())
    _expect(masked, kern, S, red, dX.numel())
    assert errs["err"] < TOL and errs["err_masked"] < TOL, errs
    assert torch.equal(dXm, dX2), "the masked store differs from the unmasked launch + lrelu_bwd"
    gs.check()


# ----------------------------------------------------------------------------- weight gradient
WGRAD = [
    # 8 x 128 = 1024 blocks over K = 4 x 4 x 4 = 64 pixels: unsplit
    ((4, 512, 512, 8, 8, 4, 2, 1), "conv_wgrad_lean_kernel", 1, None),
    # 4 x 36 = 144 blocks -> S = 6 (K = 256: 16 K tiles, pieces of 48)
    ((1, 256, 256, 16, 16, 3, 1, 1), "conv_wgrad_lean_kernel", 6, FEW4),
    # N = ldc = 2295: scalar slab stores, scalar reducer
    ((1, 255, 256, 16, 16, 3, 1, 1), "conv_wgrad_lean_kernel", 6, FEW),
]


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("case,kern,S,red", WGRAD, ids=["-".join(map(str, c[0])) for c in WGRAD])
def test_weight_gradient_store_paths(hip, case, kern, S, red, beta):
    t0 = time.perf_counter()
    B, Ci, Co, H, W, k, s, p = case
    OH, OW = _out_hw(H, W, k, s, p)
    dY, X = T(1, B, Co, OH, OW), T(2, B, Ci, H, W)
    dW0 = T(3, Co, Ci, k, k) if beta else None
    ref = dW0.double().clone() if beta else torch.zeros(Co, Ci, k, k, dtype=torch.float64)
    DBL.conv2d_wgrad(dY.double(), X.double(), ref, s, p, beta=beta)
    gs = GuardSet("cuda")
    dYg, Xg = gs.tensor(dY, "dY"), gs.tensor(X, "X")
    dW = gs.tensor(dW0, "dW") if beta else gs.full((Co, Ci, k, k), NAN, name="dW")
    got = _launch(hip, lambda: hip.conv2d_wgrad(dYg, Xg, dW, s, p, beta=beta))
    errs = {"err": relerr(dW, ref)}
    _record("wgrad", case, f"beta={beta:g}", kern, S, red, errs, t0)
    _expect(got, kern, S, red, dW.numel())
    assert errs["err"] < TOL, errs
    gs.check()
