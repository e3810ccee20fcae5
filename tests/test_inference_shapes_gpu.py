"""GPU tier: the forward kernels at the plane sizes of WHOLE-IMAGE inference, against fp64 on the CPU (tests/host_double.py,
tests/inference_double.py, oracle/rcot_oracle.py).  tests/test_kernels_gpu.py holds every entry point to fp64 at training-patch shapes
(pixel counts that are multiples of 64, power-of-two widths); a 321 x 481 image padded to 328 x 488 runs the same entry points at
N = 160064 (64 * 2501: 64-wide K-major tiles only), 40016 (N % 64 = 16: the unpacked gemm_core.h path), 10004 (N % 16 = 4) and on a
41 x 61 plane that is width-padded to 41 x 44 under ``wmask``; a 1356 x 2040 image makes tensors of more than 2^31 bytes.

 1. every forward entry point at small planes of the same residue classes, in every arithmetic, the kernel family asserted;
 2. one transformer block under ``wmask`` against the oracle on the unpadded plane;
 3. the four planes of a 321 x 481 image at full size;
 4. tensors past 2^31 bytes against fp64 on sampled pixel columns and row bands;
 5. the whole network on a 161 x 241 image against the reference's output (tests/golden/wholeimage.npz), whole and tiled.

Bars: 2e-5 of max|ref| (exact fp32, bf16x6) and 4e-5 (bf16x3), as tests/test_kernels_gpu.py applies them.  Where a reduction runs over
more than 16384 pixels no bar follows from the formats alone: there the bar is max(that, 4 x the error of the same operation evaluated in
float32 on the CPU), never the kernel's own error (profiles/inference_shapes.txt holds both numbers for every case).
Every device tensor comes from a GuardSet and the workspaces hold NaN before the kernels run (tests/guarded.py).
RCOT_INFERENCE_SHAPES_LOG=<file>: one line per compared tensor (case, kernel symbols, error, float32-host error, bar).
"""
import contextlib
import ctypes
import itertools
import os

import pytest
import torch

from conftest import relerr, seeded_tensor
from guarded import GuardSet, all_finite, poison_workspaces
from host_double import TorchDouble
import inference_double as ID
from inference_double import LEVEL

pytestmark = pytest.mark.gpu
TOL, X3_TOL = 2e-5, 4e-5
PRECS = ("fp32", "bf16x3", "bf16x6")
DBL, F32 = TorchDouble(torch.float64), TorchDouble(torch.float32)
KMAJOR_FAMILIES = ("gemm_xx_kernel<", "gemm_xx_kg_kernel", "gemm_x3_kernel<", "x3p_kernel<")
GENERAL = "gemm_kernel<TileCfg<"

# small planes of the residue classes of whole images: (B, C, H, W); N % 64 = 48, N % 16 = 12, 4, 8, N = 64 * 3 (B = 16: enough
# workgroups for the K-major kernel, on 64-wide tiles), and the real 1/8-level plane 61 x 41 width-padded to 61 x 44
SMALL = [(2, 96, 20, 28), (2, 192, 10, 14), (2, 384, 6, 6), (2, 384, 5, 8), (16, 48, 24, 8), (1, 384, 61, 44)]
# the planes of a 321 x 481 image padded to 328 x 488 (the last: 41 x 61 width-padded to 41 x 44)
REAL = [(1, 48, 328, 488), (1, 96, 164, 244), (1, 192, 82, 122), (1, 384, 41, 44)]
LONG_N = 16384                    # above it the pixel reductions take the float32-host bar

_LOG = []
_REF = {}                         # fp64 results of the last case, shared by the arithmetics that follow it


def T(seed, *shape, scale=1.0):
    return seeded_tensor(seed, shape, scale=scale)


def _pid(p):
    return "x".join(map(str, p))


@pytest.fixture(scope="module")
def hip():
    from rcot_amd.ops import HipBackend
    return HipBackend()


@pytest.fixture(scope="module", autouse=True)
def _write_log():
    yield
    path = os.environ.get("RCOT_INFERENCE_SHAPES_LOG")
    if path and _LOG:
        with open(path, "a") as f:
            f.write("".join(line + "\n" for line in _LOG))


@contextlib.contextmanager
def arithmetic(be, prec):
    from rcot_amd import lib
    old = (be.prec, getattr(be, "x6_packs", False))
    be.prec = {"fp32": lib.PREC_FP32, "bf16x3": lib.PREC_BF16X3, "bf16x6": lib.PREC_BF16X6}[prec]
    be.x6_packs = prec == "bf16x6"
    try:
        yield
    finally:
        be.prec, be.x6_packs = old


def last_kernel(be):
    buf = ctypes.create_string_buffer(192)
    seq = be.L.rcot_last_kernel(buf, 192)
    return seq, buf.value.decode()


class Named:
    """forwards every call to the backend and notes the kernel symbol the library named during it ('-': the entry point names none)"""

    def __init__(self, be):
        self.be, self.log = be, []

    def __getattr__(self, name):
        attr = getattr(self.be, name)
        if not callable(attr):
            return attr

        def call(*a, **k):
            s0, _ = last_kernel(self.be)
            r = attr(*a, **k)
            s1, nm = last_kernel(self.be)
            self.log.append((name, nm if s1 != s0 else "-"))
            return r
        return call

    def of(self, name):
        return [k for n, k in self.log if n == name]


def record(case, what, kernels, err, host, bar):
    line = f"{case} | {what} | {kernels} | err {err:.3e} | fp32 host {'-' if host is None else format(host, '.3e')} | bar {bar:.3e}"
    _LOG.append(line)
    print(line)


def compare(hip, prec, case, fn, arrays, outs, key=None, host_bar=False, names=None):
    """``fn(backend, *tensors)`` on TorchDouble in fp64 and on HIP in ``prec``; tensors[outs] within the bar of max|ref|.
    ``key``: the inputs (``arrays`` may be a function that makes them) and the fp64 side are shared with the arithmetics that follow.
    ``host_bar``: the bar of every output is max(bar, 4 x the error of fn on TorchDouble in float32).  Returns (fp64 tensors, device tensors, Named)."""
    tol = X3_TOL if prec == "bf16x3" else TOL
    names = names or {}
    if key is None or key not in _REF:
        _REF.clear()
        arrays = arrays() if callable(arrays) else arrays
        cpu = [None if a is None else a.double().clone() for a in arrays]
        fn(DBL, *cpu)
        host = None
        if host_bar:
            h32 = [None if a is None else a.float().clone() for a in arrays]
            fn(F32, *h32)
            host = {i: relerr(h32[i], cpu[i]) for i in outs}
        if key is not None:
            _REF[key] = (cpu, host, arrays)
    else:
        cpu, host, arrays = _REF[key]
    with arithmetic(hip, prec):
        gs = GuardSet("cuda")
        gpu = [None if a is None else gs.tensor(a, f"arrays[{i}]") for i, a in enumerate(arrays)]
        poison_workspaces(hip)
        nb = Named(hip)
        fn(nb, *gpu)
        torch.cuda.synchronize()
    kernels = ", ".join(dict.fromkeys(k for _, k in nb.log if k != "-")) or "-"
    errs = {i: relerr(gpu[i], cpu[i]) for i in outs}
    bars = {i: max(tol, 4.0 * host[i]) if host else tol for i in outs}
    for i in outs:
        record(f"{case} {prec}", names.get(i, f"tensor {i}"), kernels, errs[i], host[i] if host else None, bars[i])
    for i in outs:
        assert errs[i] < bars[i], (case, prec, names.get(i, i), errs[i], bars[i])
        assert all_finite(gpu[i]), i
    gs.check()
    return cpu, gpu, nb


# ============================================================================= 1 + 3: the forward entry points, small and full size
def _proj_dims(mode, C):
    hid = LEVEL[C][1]
    return {"plain": (C, 3 * C, False, False), "ln_res": (C, 2 * hid, True, True), "out": (hid, C, False, True)}[mode]


def _check_proj_family(hip, prec, packed, Co, N, B, names, ln):
    assert names, "conv1x1_fwd named no kernel"
    if packed and hip.kmajor_worth(Co, N, B):
        for nm in names:
            assert nm.startswith(KMAJOR_FAMILIES), nm
            if prec == "fp32" and N % 128:
                assert nm.startswith("gemm_xx_kernel<64, 64,") or nm == "gemm_xx_kg_kernel", nm     # 64-wide tiles only
    else:
        for nm in names:
            assert nm.startswith(GENERAL), nm                    # the unpacked dispatcher of gemm_core.h, whatever the arithmetic


def _proj(hip, prec, packed, mode, plane, tag):
    B, C, H, W = plane
    N = H * W
    Ci, Co, ln, res = _proj_dims(mode, C)

    def fn(be, Wt, X, Y, mu, rs, lw, lb, R, WT, WP, WTf, c12, s3t, s3p, s3f, s6t, s6p, s6f):
        pk = None
        if packed:
            sp3, sp6 = (s3t, s3p, s3f if ln else None), (s6t, s6p, s6f if ln else None)
            be.pack_weight(Wt, WT, WP, (lw, lb, WTf, c12) if ln else None, sp3, sp6)
            pk = (WT, WP, (WTf, c12) if ln else None, sp3, sp6)
        if ln:
            be.ln_stats(X, mu, rs)
        be.conv1x1_fwd(Wt, X, Y, ln=(mu, rs, lw, lb) if ln else None, R=R if res else None, packed=pk)
    st, sp = DBL.pack_shapes(Co, Ci)
    sf, sc = DBL.fold_shapes(Co, Ci)
    (s3a,), (s3b,) = DBL.split_shapes(Co, Ci)
    (s6a,), (s6b,) = DBL.split6_shapes(Co, Ci)

    def arrs():                                             # X: a per-pixel mean comparable to the spread
        return [T(1, Co, Ci, scale=0.1), T(2, B, Ci, N) + 0.7 * T(12, B, 1, N), torch.zeros(B, Co, N), torch.zeros(B, N), torch.zeros(B, N),
                1 + 0.1 * T(3, Ci), 0.1 * T(4, Ci), T(5, B, Co, N), torch.zeros(*st), torch.zeros(*sp), torch.zeros(*sf), torch.zeros(*sc),
                torch.zeros(s3a), torch.zeros(s3b), torch.zeros(s3a), torch.zeros(s6a), torch.zeros(s6b), torch.zeros(s6a)]
    outs = [2, 3, 4] if ln else [2]
    _, _, nb = compare(hip, prec, f"{tag} conv1x1_fwd {mode} {_pid(plane)} packed={int(packed)}", fn, arrs, outs,
                       key=("proj", mode, plane, packed), names={2: "Y", 3: "mu", 4: "rstd"})
    _check_proj_family(hip, prec, packed, Co, N, B, nb.of("conv1x1_fwd"), ln)


def _proj_two_source(hip, prec, packed, plane, tag):
    """cat-free reduce of a decoder level: W[:, :C] x1 + W[:, C:] x2, the second product accumulating (beta = 1), on channel slices"""
    B, C, H, W = plane
    N = H * W

    def fn(be, Wt, big, Y, *packs):
        for h, sl in enumerate((slice(0, C), slice(C, 2 * C))):
            pk = None
            if packed:
                WT, WP, s3t, s3p, s6t, s6p = packs[6 * h:6 * h + 6]
                be.pack_weight(Wt[:, sl], WT, WP, None, (s3t, s3p, None), (s6t, s6p, None))
                pk = (WT, WP, None, (s3t, s3p, None), (s6t, s6p, None))
            be.conv1x1_fwd(Wt[:, sl], big[:, sl], Y, beta=float(h), packed=pk)
    st, sp = DBL.pack_shapes(C, C)
    (s3a,), (s3b,) = DBL.split_shapes(C, C)
    (s6a,), (s6b,) = DBL.split6_shapes(C, C)
    packs = [torch.zeros(*s) for s in (st, sp, (s3a,), (s3b,), (s6a,), (s6b,))] * 2
    arrs = lambda: [T(1, C, 2 * C, scale=0.1), T(2, B, 2 * C, N), torch.zeros(B, C, N)] + [p.clone() for p in packs]
    _, _, nb = compare(hip, prec, f"{tag} conv1x1_fwd two_source {_pid(plane)} packed={int(packed)}", fn, arrs, [2],
                       key=("proj2", plane, packed), names={2: "Y"})
    _check_proj_family(hip, prec, packed, C, N, B, nb.of("conv1x1_fwd"), False)


def _ln_stats(hip, plane, ratio, tag):
    B, C, H, W = plane
    N = H * W

    def fn(be, X, mu, rs):
        be.ln_stats(X, mu, rs)
    X = T(2, B, C, N) + ratio * (1 + 0.2 * T(12, B, 1, N))
    compare(hip, "fp32", f"{tag} ln_stats ratio={ratio} {_pid(plane)}", fn, [X, torch.zeros(B, N), torch.zeros(B, N)], [1, 2],
            names={1: "mu", 2: "rstd"})


def _mdta(hip, prec, plane, tag):
    B, C, H, W = plane
    N, heads = H * W, LEVEL[C][0]
    c = C // heads
    fast = hip.kmajor_worth(C, N, B)

    def fn(be, *t):
        ID.mdta_chain(be, fast, heads, *t)
    arrs = lambda: [ID.qkv_like(seeded_tensor, B, C, N), T(7, B, C, N), 1 + 0.2 * T(8, heads), T(9, C, C, scale=0.1), torch.zeros(B, 2 * C),
                    torch.zeros(B, heads, c, c), torch.zeros(B, heads, c, c), torch.zeros(B, heads, c, c), torch.zeros(B, C, C),
                    torch.zeros(B, C, N)]
    names = {4: "row_sumsq", 5: "Gram (bmm_nt)", 6: "Gn", 7: "A", 8: "MfT", 9: "y (apply + residual)"}
    _, _, nb = compare(hip, prec, f"{tag} mdta {_pid(plane)}", fn, arrs, [4, 5, 6, 7, 8, 9], key=("mdta", plane), host_bar=N > LONG_N,
                       names=names)
    assert all(k != "-" for k in nb.of("bmm_nt") + nb.of("bmm_nn")), nb.log
    if fast:
        assert nb.of("gemm_kmajor")[0].startswith(KMAJOR_FAMILIES), nb.log


def stencil_family(H, W):
    if H % 4 or W % 4:
        return "dwconv_any_kernel", "gate_fwd_any_kernel"
    nb = "true" if W // 4 <= 64 and 64 % (W // 4) == 0 else "false"
    return f"dwconv_kernel<false, {nb}>", f"gate_fwd_kernel<{nb}>"


def _stencils(hip, B, hid, H, W, tag):
    def fn(be, p, w, y, g):
        be.dwconv3x3(p, w, y)
        be.gdfn_gate_fwd(p, w, g)
    arrs = [T(1, B, 2 * hid, H, W), T(2, 2 * hid, 9, scale=0.5), torch.zeros(B, 2 * hid, H, W), torch.zeros(B, hid, H, W)]
    _, _, nb = compare(hip, "fp32", f"{tag} stencils {B}x{2 * hid}x{H}x{W}", fn, arrs, [2, 3], names={2: "dwconv3x3", 3: "gdfn_gate_fwd"})
    assert (nb.of("dwconv3x3")[0], nb.of("gdfn_gate_fwd")[0]) == stencil_family(H, W), nb.log


CASES_1 = [(pl, m, pk, pr) for pl in SMALL for m in ("plain", "ln_res", "out", "two_source") for pk in (False, True) for pr in PRECS]


@pytest.mark.parametrize("plane,mode,packed,prec", CASES_1, ids=lambda v: _pid(v) if isinstance(v, tuple) else str(v))
def test_conv1x1_fwd_small_planes(hip, plane, mode, packed, prec):
    if mode == "two_source":
        _proj_two_source(hip, prec, packed, plane, "small")
    else:
        _proj(hip, prec, packed, mode, plane, "small")


@pytest.mark.parametrize("ratio", [1.0, 20.0])
@pytest.mark.parametrize("plane", SMALL, ids=_pid)
def test_ln_stats_small_planes(hip, plane, ratio):
    _ln_stats(hip, plane, ratio, "small")


@pytest.mark.parametrize("plane,prec", list(itertools.product(SMALL, PRECS)), ids=lambda v: _pid(v) if isinstance(v, tuple) else v)
def test_mdta_chain_small_planes(hip, plane, prec):
    _mdta(hip, prec, plane, "small")


# W / 4 = 82 and 61 (quad kernels, no neighbour lanes), 6 (does not divide 64), 32 (neighbour lanes: the control); three gate planes /
# six depthwise planes: the last wavefront of the quad grid is partial (492, 549 and 36 quads; 8 x 128 always fills its wavefronts,
# there the last workgroup is partial); then the planes of the projections
@pytest.mark.parametrize("B,hid,H,W", [(1, 3, 8, 328), (1, 3, 12, 244), (1, 3, 8, 24), (1, 3, 8, 128)] +
                         [(1, 3, H, W) for _, _, H, W in SMALL])
def test_stencils_small_planes(hip, B, hid, H, W):
    _stencils(hip, B, hid, H, W, "small")


# (name, B, Ci, Co, H, W, cmap, residual): the PixelUnshuffle / PixelShuffle epilogues at planes with sides that are no multiple of 4,
# the thin RGB-side kernels at a small and the full padded image, MPRNet's 3 x 3 convolutions at its lower levels
CONVS = [("down cmap1", 1, 192, 96, 10, 14, 1, False), ("down cmap1", 1, 192, 96, 122, 82, 1, False),
         ("up cmap2", 1, 384, 768, 5, 7, 2, False), ("up cmap2", 1, 384, 768, 61, 41, 2, False),
         ("thin 3->48", 1, 3, 48, 40, 56, 0, False), ("thin 96->3", 1, 96, 3, 40, 56, 0, True),
         ("thin 3->48", 1, 3, 48, 328, 488, 0, False), ("thin 96->3", 1, 96, 3, 328, 488, 0, True),
         ("mprnet 3x3", 1, 176, 176, 19, 27, 0, False), ("mprnet 3x3", 1, 128, 128, 38, 54, 0, True)]


@pytest.mark.parametrize("name,B,Ci,Co,H,W,cmap,res", CONVS, ids=[f"{c[0].replace(' ', '_')}-{c[4]}x{c[5]}" for c in CONVS])
def test_conv2d_fwd_inference_planes(hip, name, B, Ci, Co, H, W, cmap, res):
    """against torch.nn.functional.conv2d in fp64 (+ pixel_unshuffle / pixel_shuffle): TorchDouble.conv2d_fwd"""
    oshape = {0: (B, Co, H, W), 1: (B, 4 * Co, H // 2, W // 2), 2: (B, Co // 4, 2 * H, 2 * W)}[cmap]

    def fn(be, X, Wt, Y, R):
        be.conv2d_fwd(X, Wt, None, Y, 1, 1, 1.0, cmap, R if res else None)
    arrs = [T(1, B, Ci, H, W), T(2, Co, Ci, 3, 3, scale=0.1), torch.zeros(*oshape), T(3, *oshape)]
    compare(hip, "fp32", f"conv2d_fwd {name} {Ci}->{Co} {H}x{W}", fn, arrs, [2], names={2: "Y"})


def test_mprnet_bilinear_resampling(hip):
    """bilinear_down2 at 10 x 14 -> 5 x 7 and bilinear_up2 back with the skip tensor"""
    def fn(be, x, d, s, y):
        be.bilinear_down2(x, d)
        be.bilinear_up2(d, s, y)
    compare(hip, "fp32", "mprnet bilinear 10x14", fn, [T(1, 2, 80, 10, 14), torch.zeros(2, 80, 5, 7), T(2, 2, 80, 10, 14), torch.zeros(2, 80, 10, 14)],
            [1, 3], names={1: "bilinear_down2", 3: "bilinear_up2 + skip"})


# ============================================================================= 3. the planes of a 321 x 481 image, full size
# the unpacked dispatcher does not read the arithmetic: once; the packed call in all three
CASES_3 = [(pl, m, pk, pr) for pl in REAL for m in ("plain", "ln_res", "out", "two_source")
           for pk, pr in [(False, "fp32")] + [(True, p) for p in PRECS]]


@pytest.mark.parametrize("plane,mode,packed,prec", CASES_3, ids=lambda v: _pid(v) if isinstance(v, tuple) else str(v))
def test_conv1x1_fwd_real_planes(hip, plane, mode, packed, prec):
    if mode == "two_source":
        _proj_two_source(hip, prec, packed, plane, "real")
    else:
        _proj(hip, prec, packed, mode, plane, "real")


@pytest.mark.parametrize("ratio", [1.0, 20.0])
@pytest.mark.parametrize("plane", REAL, ids=_pid)
def test_ln_stats_real_planes(hip, plane, ratio):
    _ln_stats(hip, plane, ratio, "real")


@pytest.mark.parametrize("plane,prec", list(itertools.product(REAL, PRECS)), ids=lambda v: _pid(v) if isinstance(v, tuple) else v)
def test_mdta_chain_real_planes(hip, plane, prec):
    """N = 160064 and 40016: the bars of the pixel reductions and of what follows them come from the float32 host evaluation"""
    _mdta(hip, prec, plane, "real")


@pytest.mark.parametrize("plane", REAL, ids=_pid)
def test_stencils_real_planes(hip, plane):
    """the GDFN's depthwise conv and gate at each level's hidden width would be 2 hid planes of the same kernel: 8 of them here (the
    grid covers planes x quads; the last workgroup is partial at 164 x 244 and 82 x 122 / 41 x 44)"""
    _, _, H, W = plane
    _stencils(hip, 1, 4, H, W, "real")


# ============================================================================= 2. one transformer block under wmask
@pytest.mark.parametrize("prec,bar", [("fp32", 2e-5), ("bf16x3", 1e-4)])
@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (2, 7, 9), (2, 3, 3), (2, 1, 1), (1, 61, 41)])
def test_transformer_block_under_wmask(B, H, W, prec, bar):
    """TransformerBlockOp.forward(x, save=False, wmask=W) on the plane width-padded as T_net._lat_pad pads it (C = 384, 8 heads) against
    oracle.rcot_oracle.transformer_block in fp64 on the UNPADDED plane, real columns; bars: test_transformer_block_vs_reference_fixture
    (fp32) and its B = 8 sibling (bf16x3).  The block promises that the padding columns never reach a real pixel (they are re-zeroed
    before every spatial or pixel-reducing operation), not that its result is zero there: the same call with large finite values in
    the padding columns of x gives the same bits in the real columns."""
    from oracle import rcot_oracle as O
    from rcot_amd import params as P
    from rcot_amd.net_restormer import ParamStore, TransformerBlockOp
    from rcot_amd.ops import HipBackend
    C, heads = 384, 8
    be = HipBackend()
    shapes = P.block_param_shapes("blk", C, heads)
    params = {k: torch.from_numpy(v) for k, v in P.seeded_params(shapes, 21, "T").items()}
    x = seeded_tensor(31, (B, C, H, W))
    with torch.no_grad():
        ref = O.transformer_block(x.double(), {k: v.double() for k, v in params.items()}, "blk", heads)
    Wp = (W + 3) // 4 * 4
    assert (H * W) % 4 and (H * Wp) % 4 == 0
    with arithmetic(be, prec):
        st = ParamStore(be, shapes, [n for n, _ in shapes], [])
        st.load(params)
        blk = TransformerBlockOp(be, st, "blk", C, heads)
        blk.repack()
        gs = GuardSet("cuda")
        xp = torch.zeros(B, C, H, Wp)
        xp[..., :W] = x
        xq = xp.clone()
        xq[..., W:] = 1.0e3
        with gs.adopt(be):
            y, _ = blk.forward(gs.tensor(xp, "x"), False, W)
            y2, _ = blk.forward(gs.tensor(xq, "x, padding columns 1e3"), False, W)
            torch.cuda.synchronize()
    e = relerr(y[..., :W], ref)
    record(f"block wmask {B}x{C}x{H}x{W}->{Wp} {prec}", "y[..., :W]", "TransformerBlockOp.forward", e, None, bar)
    assert e < bar, e
    assert torch.equal(y[..., :W], y2[..., :W]) and all_finite(y2)


# ============================================================================= 4. tensors past 2^31 bytes
def _pixel_samples(N, extra=()):
    """first and last 512 pixel columns, 512 in the middle, and 512 around each pixel of ``extra``"""
    spans = [(0, 512), (N - 512, N), (N // 2 - 256, N // 2 + 256)] + [(max(p - 256, 0), min(p + 256, N)) for p in extra]
    return torch.cat([torch.arange(a, b) for a, b in spans]).unique()


def _sampled_err(got, ref):
    return float((got.detach().double().cpu() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("B,H,W", [(1, 1456, 1456), (2, 22084, 48)], ids=["B1-1456x1456", "B2-22084x48"])
def test_gdfn_past_2gib(hip, B, H, W, prec):
    """The GDFN of the 48-channel level on a plane of 1456 x 1456 pixels: project_in's output P (254 planes) holds 2 153 854 976 bytes,
    byte 2^31 lies in its last plane; at B = 2 on 22084 x 48 = 1 060 032 pixels (1 060 000 rounded up to a multiple of 64) the batch
    stride carries the crossing.  ln_stats + conv1x1_fwd 48 -> 254 with the LayerNorm prologue, gdfn_gate_fwd on P, conv1x1_fwd
    127 -> 48 + residual; X is made on the device from a seeded generator and only samples come back: every channel at the first, the
    last and the middle 512 pixel columns and the 512 around the element at byte 2^31 (1x1 products), rows with a one-row halo at the
    top, the bottom and around that element of the first and the last gate plane and of the one that reads it (the gate).  All of P and
    of the gate's output is finite, the guard bands are intact.  About 4.1 GB of device memory."""
    C, hid = 48, 127
    N = H * W
    assert N % 64 == 0 and B * 2 * hid * N * 4 > 2 ** 31
    tol = X3_TOL if prec == "bf16x3" else TOL
    e31 = 2 ** 29                                             # the float at byte offset 2^31 of P: (image, plane, pixel)
    b31, ch31, px31 = e31 // (2 * hid * N), e31 % (2 * hid * N) // N, e31 % N
    case = f"past 2^31 bytes B={B} {H}x{W} {prec}"
    with arithmetic(hip, prec):
        gs = GuardSet("cuda")
        poison_workspaces(hip)
        gen = torch.Generator(device="cuda").manual_seed(5)
        X = gs.empty((B, C, N), name="X")
        X.normal_(generator=gen)
        X += 0.7 * torch.randn(B, 1, N, device="cuda", generator=gen)
        Win, Wout, Wdw = T(1, 2 * hid, C, scale=0.1), T(2, C, hid, scale=0.1), T(3, 2 * hid, 9, scale=0.5)
        lw, lb = 1 + 0.1 * T(4, C), 0.1 * T(5, C)
        g = lambda t, n: gs.tensor(t, n)
        Wi, Wo, Wd, lwg, lbg = g(Win, "W_in"), g(Wout, "W_out"), g(Wdw, "W_dw"), g(lw, "ln w"), g(lb, "ln b")

        def packs(Wt, fold):
            Co, Ci = Wt.shape
            z = lambda s: gs.full(s, 0.0)
            WT, WP = (z(s) for s in hip.pack_shapes(Co, Ci))
            fo = tuple(z(s) for s in hip.fold_shapes(Co, Ci)) if fold else None
            (a,), (b,) = hip.split_shapes(Co, Ci)
            sp3 = (z((a,)), z((b,)), z((a,)) if fold else None)
            hip.pack_weight(Wt, WT, WP, (lwg, lbg) + fo if fold else None, sp3, None)
            return (WT, WP, fo, sp3, None)
        pk_in, pk_out = packs(Wi, True), packs(Wo, False)
        nb = Named(hip)
        mu, rs = gs.empty((B, N), name="mu"), gs.empty((B, N), name="rstd")
        nb.ln_stats(X, mu, rs)
        P_ = gs.empty((B, 2 * hid, H, W), name="P")
        nb.conv1x1_fwd(Wi, X, P_, ln=(mu, rs, lwg, lbg), packed=pk_in)
        G = gs.empty((B, hid, H, W), name="gate")
        nb.gdfn_gate_fwd(P_, Wd, G)
        out = gs.empty((B, C, N), name="out")
        nb.conv1x1_fwd(Wo, G, out, R=X, packed=pk_out)
        torch.cuda.synchronize()
    k_in, k_out = nb.of("conv1x1_fwd")
    assert k_in.startswith(KMAJOR_FAMILIES) and k_out.startswith(KMAJOR_FAMILIES), nb.log
    assert nb.of("gdfn_gate_fwd")[0] == stencil_family(H, W)[1], nb.log
    assert bool(torch.isfinite(P_).all()), "P"
    assert bool(torch.isfinite(G).all()), "gate"
    # ---- 1x1 products on pixel columns
    cols = _pixel_samples(N, (px31,)).cuda()
    Pf, Gf = P_.view(B, 2 * hid, N), G.view(B, hid, N)
    errs = {}
    for b in range(B):
        ref, mu_r, rs_r = ID.proj_columns(Win, X[b][:, cols], ln=(lw, lb))
        errs[f"P[{b}]"] = _sampled_err(Pf[b][:, cols], ref)
        errs[f"mu[{b}]"] = _sampled_err(mu[b][cols], mu_r)
        errs[f"rstd[{b}]"] = _sampled_err(rs[b][cols], rs_r)
        ref, _, _ = ID.proj_columns(Wout, Gf[b][:, cols], R=X[b][:, cols])
        errs[f"out[{b}]"] = _sampled_err(out[b][:, cols], ref)
    # ---- the gate on row bands: first and last plane, and the plane whose input holds byte 2^31
    r31 = px31 // W
    bands = {(0, 6), (H - 6, H), (H // 2 - 3, H // 2 + 3), (max(r31 - 3, 0), min(r31 + 3, H))}
    for b, j in {(0, 0), (B - 1, hid - 1), (b31, ch31 % hid)}:
        for r0, r1 in sorted(bands):
            errs[f"gate[{b},{j}] rows {r0}:{r1}"] = _sampled_err(G[b, j, r0:r1], ID.gate_rows(P_, Wdw, b, j, r0, r1))
    for what, e in errs.items():
        kern = k_in if what.startswith("P") else k_out if what.startswith("out") else nb.of("gdfn_gate_fwd")[0] if what.startswith("gate") else "ln_stats_kernel"
        record(case, what, kern, e, None, tol)
    bad = {k: e for k, e in errs.items() if not e < tol}
    gs.check()
    del X, P_, G, out, Pf, Gf, gs
    torch.cuda.empty_cache()
    assert not bad, bad


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_gram_and_row_sumsq_over_two_million_pixels(hip, prec):
    """bmm_nt and row_sumsq over K = N = 1456^2 = 2 119 936 pixels, one head of 48 channels, k = 0.5 q + noise, against the whole fp64
    product; the bar is max(the format's, 4 x the float32 host evaluation's error), as for the real planes."""
    c, N = 48, 1456 * 1456
    tol = X3_TOL if prec == "bf16x3" else TOL
    with arithmetic(hip, prec):
        gs = GuardSet("cuda")
        poison_workspaces(hip)
        gen = torch.Generator(device="cuda").manual_seed(6)
        u = gs.empty((1, 2 * c, N), name="q | k")
        u.normal_(generator=gen)
        u[:, c:] += 0.5 * u[:, :c]
        sq, Gr = gs.empty((1, 2 * c), name="sq"), gs.empty((1, 1, c, c), name="Gram")
        nb = Named(hip)
        nb.row_sumsq(u, sq)
        uu = u.view(1, 2, 1, c, N)
        nb.bmm_nt(uu[:, 0], uu[:, 1], Gr)
        torch.cuda.synchronize()
    h = u.cpu()[0]
    del u
    torch.cuda.empty_cache()
    d = h.double()
    ref_g, ref_s = d[:c] @ d[c:].t(), (d * d).sum(1)
    del d
    host_g, host_s = relerr(h[:c] @ h[c:].t(), ref_g), relerr((h * h).sum(1), ref_s)
    e_g, e_s = relerr(Gr[0, 0], ref_g), relerr(sq[0], ref_s)
    record(f"N=1456^2 {prec}", "Gram (bmm_nt)", nb.of("bmm_nt")[0], e_g, host_g, max(tol, 4 * host_g))
    record(f"N=1456^2 {prec}", "row_sumsq", "row_sumsq_kernel", e_s, host_s, max(tol, 4 * host_s))
    gs.check()
    assert e_g < max(tol, 4 * host_g) and e_s < max(tol, 4 * host_s), (e_g, host_g, e_s, host_s)


# ============================================================================= 5. the whole network at a real size class
@pytest.fixture(scope="module")
def whole_net():
    from rcot_amd import params as P
    from rcot_amd.net_restormer import T_net
    from rcot_amd.ops import HipBackend
    net = T_net(decoder=True, backend=HipBackend())
    net.load_state_dict({k: torch.from_numpy(v) for k, v in P.seeded_params(P.tnet_param_shapes(), 11, "T").items()})
    return net


def _whole_image(fx):
    B, h, w, seed, pseed = (int(v) for v in fx["cfg"])
    assert (B, h, w, pseed) == (1, 161, 241, 11)
    return seeded_tensor(seed, (1, 3, h, w), lo=0.0, hi=1.0), h, w


@pytest.mark.parametrize("prec,bar", [("fp32", 2e-5), ("bf16x3", 1e-4)])
def test_whole_image_161x241_vs_reference(whole_net, gold, prec, bar):
    """restore_any_size on a 161 x 241 image, reflect-padded to 168 x 248 — planes of 84 x 124 = 64 * 651 (N % 128 = 64), 42 x 62 and
    21 x 31 -> 21 x 32 pixels — against the REFERENCE's T_net on the same padded image, cropped (tests/golden/wholeimage.npz,
    oracle/pin_against_reference.py --only wholeimage); bars: test_whole_image_with_odd_latent_plane_vs_reference."""
    from rcot_amd.wholeimage import restore_any_size
    fx = gold("wholeimage.npz")
    x, h, w = _whole_image(fx)
    with arithmetic(whole_net.be, prec):
        r = restore_any_size(whole_net, x, 8, "reflect")
        torch.cuda.synchronize()
    assert (r.Hp, r.Wp) == (168, 248)
    e = relerr(r.out[:, :, :h, :w], torch.from_numpy(fx["y"]))
    record(f"whole image 161x241 {prec}", "restored", "T_net.forward", e, None, bar)
    assert e < bar, e


def test_whole_image_161x241_tiles_equal_the_host_loop(whole_net, gold):
    """--tile 96 --overlap 16 with equal weights: the tiles as views on the device (rcot_amd/tiles.py, uniform window, one view per
    call) reproduce the tile loop of tester.restore bit for bit, as the README promises, on the real network at 168 x 248"""
    from rcot_amd import tester as TS, tiles as TL
    from rcot_amd.wholeimage import restore_any_size
    x, h, w = _whole_image(gold("wholeimage.npz"))
    want = restore_any_size(whole_net, x, 8, "reflect", tile=96, overlap=16)
    p = TL.plan(168, 248, 96, 16, 8, 1)
    assert p.n_views == 6 and (p.Th, p.Tw) == (96, 96)
    got = TL.restore_views(whole_net, want.x, p, "uniform", 1)
    torch.cuda.synchronize()
    assert torch.equal(got, want.out) and all_finite(got)
    assert torch.equal(TS.restore(whole_net, want.x, 96, 16, 8, window="uniform", tile_batch=1, ensemble=1), want.out)
