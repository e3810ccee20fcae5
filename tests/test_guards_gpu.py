"""GPU tier: what tests/test_kernels_gpu.py's ``both()`` does not reach, on guard-banded tensors with poisoned workspaces
(tests/guarded.py).  Every case compares with a restatement the repository already has, at that restatement's tolerance, and ends in
``GuardSet.check()``: a write outside an output damages a band, a read outside an input or of workspace nobody filled brings a NaN
into what is compared.  No case passes a misaligned or undersized buffer to a launch; the bands only observe.

  1. the harness's self-test on device memory;
  2. views (csrc/views.hip), byte images (csrc/imageio.hip, csrc/quality.hip), patch_prep, the OT cost with a workspace of exactly
     the documented size;
  3. the MPRNet pieces and the split-product kernels, the most ragged case of each test of test_mprnet_gpu.py / test_x3_gpu.py
     (the tests of test_x3_gpu.py that go through test_kernels_gpu's ``both()`` are guarded there);
  4. whole paths with ``GuardSet.adopt(backend)``: minimax iterations at P = 32 and P = 96, an MPRNet forward / backward, Restormer
     inference on a 37 x 45 uint8 image, whole and as 32 blended views.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import relerr, seeded_tensor
from guarded import GuardSet, all_finite, poison_workspaces
from host_double import TorchDouble
from rcot_amd import mprnet as MP
from rcot_amd import params as P
from rcot_amd import quality as Q
from rcot_amd import tiles as TL
from test_anysize_cpu import egress_stats, quantise, synth_pair
from test_anysize_gpu import _fpad, _modes, _tparams
from test_guarded_cpu import selftest
from test_iteration_grads_gpu import _compare, _np_params, _snapshot
from test_ot_sizes_gpu import _host_iteration, _inputs
from test_quality_cpu import PROTOCOLS, image_pairs
from test_tiles_cpu import GEOMETRIES, blend_views, gather_views

pytestmark = pytest.mark.gpu

DBL = TorchDouble(torch.float64)


@pytest.fixture(scope="module")
def hip():
    from rcot_amd.ops import HipBackend
    return HipBackend()


@pytest.fixture
def gs(hip):
    """a GuardSet on the device with the backend's workspaces poisoned; checked once more when the test is over"""
    s = GuardSet("cuda")
    poison_workspaces(hip)
    yield s
    s.check()


def _backend(prec):
    from rcot_amd import lib
    from rcot_amd.ops import HipBackend
    be = HipBackend()
    be.prec = {"fp32": lib.PREC_FP32, "bf16x3": lib.PREC_BF16X3, "bf16x6": lib.PREC_BF16X6, "bf16x1": lib.PREC_BF16X1}[prec]
    be.x6_packs = prec == "bf16x6"
    return be


def _flat(views):
    return np.concatenate([v.reshape(-1) for v in views])


# ------------------------------------------------------------------ 1. the harness on the device
def test_guardset_on_device_memory():
    assert selftest("cuda")


# ------------------------------------------------------------------ 2a. views
@pytest.mark.parametrize("case", list(GEOMETRIES) + ["i"])
def test_views_inside_their_tensors(hip, gs, case):
    """test_tiles_gpu.py::test_gather_and_blend_equal_the_restatement with ``out=`` from the set: exact equality, both tap forms"""
    H, W, tile, ov, mult, modes = GEOMETRIES["c" if case == "i" else case]
    planes = 6 if case == "i" else 3
    p = TL.plan(H, W, tile, ov, mult, 1)
    ys, xs, Th, Tw = list(p.ys), list(p.xs), p.Th, p.Tw
    img = seeded_tensor(H * 1000 + W, (planes, H, W))
    want = gather_views(img.numpy(), ys, xs, modes, Th, Tw)
    views = hip.view_gather(gs.tensor(img, "img"), ys, xs, modes, Th, Tw, out=gs.empty((len(want), planes * Th * Tw), name="views"))
    assert torch.equal(views.cpu().reshape(-1), torch.from_numpy(_flat(want)))
    g = np.random.Generator(np.random.PCG64(H + W))
    net_out = [g.uniform(-1.0, 1.0, v.shape).astype(np.float32) for v in want]
    dev = gs.tensor(torch.from_numpy(_flat(net_out)).view(len(want), -1), "network output")
    wy, wx = TL.window_taps(Th, ov or 4, "linear"), TL.window_taps(Tw, ov or 4, "linear")
    for taps in (None, (wy, wx)):
        kind = "uniform" if taps is None else "linear"
        wd = (None, None) if taps is None else (gs.tensor(torch.from_numpy(wy), "wy"), gs.tensor(torch.from_numpy(wx), "wx"))
        got = hip.view_blend(dev, H, W, ys, xs, modes, Th, Tw, *wd, out=gs.empty((planes, H, W), name=f"blend {kind}"))
        ref = blend_views(net_out, planes, H, W, ys, xs, modes, Th, Tw, *(taps or (None, None)))
        assert torch.equal(got.cpu(), torch.from_numpy(ref)), (case, kind)


# ------------------------------------------------------------------ 2b. byte images
@pytest.mark.parametrize("shape", [((37, 45), (40, 48)), ((5, 7), (8, 8)), ((1, 1), (1, 1))], ids=["37x45", "5x7", "1x1"])
def test_ingest_and_pad2d_inside_their_tensors(hip, gs, shape):
    (h, w), (Hp, Wp) = shape
    g = np.random.Generator(np.random.PCG64(h * 1000 + w))
    img = torch.from_numpy(g.integers(0, 256, size=(h, w, 3), dtype=np.uint8))
    planes = seeded_tensor(h + w, (2, 3, h, w))
    imgd, pld = gs.tensor(img, "img"), gs.tensor(planes, "planes")
    for mode in _modes(h, w, Hp, Wp):
        got = hip.image_ingest(imgd, Hp, Wp, mode, out=gs.empty((1, 3, Hp, Wp), name=f"ingest {mode}"))
        assert torch.equal(got.cpu(), _fpad(img.permute(2, 0, 1).float().div(255)[None], Hp, Wp, mode)), mode
        got = hip.pad2d(pld, Hp, Wp, mode, out=gs.empty((2, 3, Hp, Wp), name=f"pad2d {mode}"))
        assert torch.equal(got.cpu(), _fpad(planes, Hp, Wp, mode)), mode


@pytest.mark.parametrize("h,w", [(37, 45), (5, 7), (1, 1), (16, 33)])      # 3 h w = 4995, 105, 3 (odd) and 1584 (a multiple of 4)
def test_image_egress_inside_its_tensors(hip, gs, h, w):
    """rcot_image_egress through the library: guarded out_u8, res_u8, stats and a NaN-filled workspace of exactly the documented
    24 bytes per workgroup of 4 rows x 256 columns; against test_anysize_cpu.quantise / egress_stats and wholeimage.image_metrics"""
    from rcot_amd import tester as TS
    from rcot_amd.wholeimage import image_metrics
    Hp, Wp = -(-h // 8) * 8, -(-w // 8) * 8
    restored, target = synth_pair(h * 1000 + w, h, w)
    padded = seeded_tensor(h + w, (3, Hp, Wp), lo=-1.0, hi=2.0)            # what lies beyond the image must not count
    padded[:, :h, :w] = torch.from_numpy(restored)
    degraded = seeded_tensor(h + w + 1, (3, Hp, Wp), lo=-0.2, hi=1.2)
    need = 24 * (-(-h // 4)) * (-(-w // 256))
    rd, dd, td = gs.tensor(padded, "restored"), gs.tensor(degraded, "degraded"), gs.tensor(torch.from_numpy(target), "target")
    out_u8, res_u8 = gs.empty((h, w, 3), torch.uint8, "out_u8"), gs.empty((h, w, 3), torch.uint8, "res_u8")
    stats, ws = gs.empty((4,), torch.float64, "stats"), gs.empty((need // 4,), name="ws")
    args = (rd.data_ptr(), dd.data_ptr(), td.data_ptr(), h, w, Hp, Wp, 2.0, out_u8.data_ptr(), res_u8.data_ptr(), stats.data_ptr(),
            ws.data_ptr())
    assert hip.L.rcot_image_egress(*args, need - 1, hip._st()) == -2       # one byte short: RCOT_EWORKSPACE
    assert hip.L.rcot_image_egress(*args, need, hip._st()) == 0
    torch.cuda.synchronize()
    want_u8 = quantise(torch.from_numpy(restored))
    assert np.array_equal(out_u8.cpu().numpy(), want_u8)
    assert np.array_equal(res_u8.cpu().numpy(), quantise((degraded - padded)[:, :h, :w] * 2.0))
    want, got = egress_stats(restored, target, want_u8), stats.cpu().numpy()
    assert got[1] == want[1] and got[3] == want[3] == 3 * max(0, h - 10) * max(0, w - 10)
    assert abs(got[0] - want[0]) <= 1e-12 * want[0]
    m = image_metrics(stats, h, w)
    if want[3]:
        assert abs(m["ssim"] - TS.ssim_image(target, want_u8)) < 1e-10
    else:
        assert got[2] == 0.0 and np.isnan(m["ssim"])
    assert abs(m["psnr_u8"] - TS.psnr_uint8(target, want_u8)) < 1e-9


@pytest.mark.parametrize("h,w", [(37, 45), (5, 7), (1, 1), (16, 33)])
def test_image_quality_inside_its_tensors(hip, gs, h, w):
    """rcot_image_quality through the library on guarded images, stats and a NaN-filled workspace of exactly the documented
    16 planes ceil(h / 16) ceil(w / 32) bytes; against rcot_amd/quality.py as test_quality_gpu.py compares"""
    _, a, b = image_pairs(h * 1000 + w, h, w)[1]
    ad, bd = gs.tensor(torch.from_numpy(a), "a"), gs.tensor(torch.from_numpy(b), "b")
    for window, space in PROTOCOLS:
        need = 16 * (3 if space == "rgb" else 1) * (-(-h // 16)) * (-(-w // 32))
        assert need == hip.image_quality_ws_bytes(h, w, space)
        stats, ws = gs.empty((4,), torch.float64, f"stats {window} {space}"), gs.empty((need // 4,), name=f"ws {window} {space}")
        args = (ad.data_ptr(), bd.data_ptr(), h, w, hip.WINDOWS[window], hip.SPACES[space], stats.data_ptr(), ws.data_ptr())
        assert hip.L.rcot_image_quality(*args, need - 1, hip._st()) == -2
        assert hip.L.rcot_image_quality(*args, need, hip._st()) == 0
        torch.cuda.synchronize()
        got = stats.cpu().numpy()
        err, n = Q.sqerr_sums(a, b, space)
        total, count = Q.ssim_sums(a, b, window, space)
        assert got[0] == err and got[1] == n and got[3] == count, (window, space, got.tolist(), err, n, count)
        assert Q.quality_metrics(got)["psnr"] == Q.psnr_u8(a, b, space)
        if count == 0:
            assert got[2] == 0.0
        else:
            assert abs(got[2] / got[3] - Q.ssim_windowed(a, b, window, space)) < 1e-10, (window, space)


# ------------------------------------------------------------------ 2c. patch_prep
@pytest.mark.parametrize("y0,x0", [(0, 0), (0, 13), (5, 0), (5, 13)])
@pytest.mark.parametrize("paired", [False, True])
def test_patch_prep_at_the_corners(hip, gs, paired, y0, x0):
    """32 x 32 windows that end on the last row / column of a 37 x 45 image, all eight maps, against host_double.patch_prep
    (sigma 0, as tests/test_pipeline_gpu.py compares: the map itself, exactly)"""
    g = np.random.Generator(np.random.PCG64(y0 * 100 + x0))
    H, W, Pz = 37, 45, 32
    clean = torch.from_numpy(g.integers(0, 256, size=(H, W, 3), dtype=np.uint8))
    deg = torch.from_numpy(g.integers(0, 256, size=(H, W, 3), dtype=np.uint8)) if paired else None
    cd, dd = gs.tensor(clean, "clean"), None if deg is None else gs.tensor(deg, "deg")
    dbl = TorchDouble(torch.float32)
    for mode in range(8):
        d_ref, c_ref = torch.empty(3, Pz, Pz), torch.empty(3, Pz, Pz)
        dbl.patch_prep(clean, deg, y0, x0, Pz, mode, 0.0, 1, d_ref, c_ref)
        d, c = gs.empty((3, Pz, Pz), name=f"deg_out {mode}"), gs.empty((3, Pz, Pz), name=f"clean_out {mode}")
        hip.patch_prep(cd, dd, y0, x0, Pz, mode, 0.0, 1, d, c)
        assert torch.equal(c.cpu(), c_ref) and torch.equal(d.cpu(), d_ref), mode


# ------------------------------------------------------------------ 2d. OT cost
def _bluestein_m(n):
    """0 when the line FFT has a radix plan (prime factors <= 13), else the power of two M >= 2n - 1 of Bluestein's algorithm"""
    m = n
    for p in (2, 3, 5, 7, 11, 13):
        while m % p == 0:
            m //= p
    return 0 if m == 1 else 1 << (2 * n - 2).bit_length()


# radix-2; mixed radix; Bluestein on both axes (34 = 2 * 17, 46 = 2 * 23); mixed rows of Bluestein columns
@pytest.mark.parametrize("H,W", [(32, 32), (24, 40), (34, 46), (96, 34)])
@pytest.mark.parametrize("paired", [False, True])
def test_ot_cost_with_the_documented_workspace(hip, gs, H, W, paired):
    """test_kernels_gpu.py::test_ot_cost's construction and bars; rcot_ot_spectrum through the library with a guarded NaN-filled
    workspace of exactly B 3 H W complex values plus M per Bluestein axis (include/rcot_hip.h)"""
    import ctypes
    B, de = 4, [0, 2, 3, 7]
    rad = (ctypes.c_int * 16)()
    for n in (H, W):
        stages = hip.L.rcot_fft_plan(n, ctypes.cast(rad, ctypes.c_void_p), 16)
        assert (stages == 0) == (_bluestein_m(n) > 0) and (stages > 0 or rad[0] == _bluestein_m(n))
    assert [_bluestein_m(n) for n in (32, 24, 40, 96, 34, 46)] == [0, 0, 0, 0, 128, 128]
    need = 8 * (B * 3 * H * W + _bluestein_m(H) + _bluestein_m(W))
    deg, out = seeded_tensor(1, (B, 3, H, W), scale=0.3), seeded_tensor(2, (B, 3, H, W), scale=0.3)
    out[2, 0] = deg[2, 0]               # a plane with an exactly-zero spectrum
    out[3, 1] = deg[3, 1] - 0.25        # constant residual: one non-zero bin
    arrs = [deg, out, seeded_tensor(3, (B, 3, H, W), scale=0.3), seeded_tensor(4, (B, 3, H, W), scale=0.01), torch.zeros(2 * B + 2),
            torch.zeros(B), torch.zeros(3), torch.zeros(B, 3, H, W)]
    cpu = [a.double().clone() for a in arrs]
    d_host = torch.tensor(de, dtype=torch.int32)
    DBL.ot_reduce(cpu[0], cpu[1], cpu[2] if paired else None, cpu[4])
    DBL.ot_spectrum(cpu[0], cpu[1], d_host, cpu[7], cpu[5])
    DBL.ot_grad(cpu[0], cpu[1], cpu[2] if paired else None, d_host, cpu[7], cpu[4], cpu[5], cpu[3], cpu[6], 1.0, 10000.0, B)
    gdeg, gout, gtgt, gdout, gsums, gspec, gscal, ggF = [gs.tensor(a, f"arrs[{i}]") for i, a in enumerate(arrs)]
    d, ws = gs.tensor(d_host, "de_id"), gs.empty((need // 4,), name="ws")
    hip.ot_reduce(gdeg, gout, gtgt if paired else None, gsums)
    args = (gdeg.data_ptr(), gout.data_ptr(), d.data_ptr(), ggF.data_ptr(), gspec.data_ptr(), ws.data_ptr())
    assert hip.L.rcot_ot_spectrum(*args, need - 8, B, H, W, hip._st()) == -2
    assert hip.L.rcot_ot_spectrum(*args, need, B, H, W, hip._st()) == 0
    hip.ot_grad(gdeg, gout, gtgt if paired else None, d, ggF, gsums, gspec, gdout, gscal, 1.0, 10000.0, B)
    torch.cuda.synchronize()
    assert relerr(gsums, cpu[4]) < 1e-5 and relerr(gscal, cpu[6]) < 1e-5
    assert relerr(gspec[2:], cpu[5][2:]) < 1e-5
    m = torch.ones(B, 3, 1, 1)          # the |F| = 0 / single-bin planes are degenerate for F/|F| in fp32, as in test_ot_cost
    m[2, 0] = 0
    m[3, 1] = 0
    assert relerr(gdout.cpu() * m, cpu[3] * m) < 5e-5
    assert all_finite(gdout) and all_finite(gscal) and all_finite(gsums) and all_finite(gspec[2:])


# ------------------------------------------------------------------ 3a. MPRNet pieces (the most ragged case of test_mprnet_gpu.py's)
def test_prelu_guarded(hip, gs):
    n, off = 4099, 1                                                      # views that start 4 bytes into their tensors
    x = seeded_tensor(1, (n + off,))
    x[::17] = 0.0
    dy, a = seeded_tensor(2, (n + off,)), torch.tensor([0.2])
    xd, dyd, ad = gs.tensor(x, "x")[off:], gs.tensor(dy, "dy")[off:], gs.tensor(a, "slope")
    y = gs.empty((n + off,), name="y")[off:]
    hip.prelu_fwd(xd, ad, y)
    assert torch.equal(y.cpu(), F.prelu(x[off:].double(), a.double()).float())
    xr, ar = x[off:].double().requires_grad_(True), a.double().requires_grad_(True)
    F.prelu(xr, ar).backward(dy[off:].double())
    dx, da = gs.empty((n + off,), name="dx")[off:], gs.full((1,), 0.5, name="dslope")
    hip.prelu_bwd(dyd, xd, ad, dx, da)
    assert torch.equal(dx.cpu(), xr.grad.float())
    assert abs(float(da) - 0.5 - float(ar.grad)) <= 2e-6 * float((x[off:].double() * dy[off:].double()).abs().sum())
    g = gs.tensor(dy, "dy in place")[off:]
    hip.prelu_bwd(g, xd, ad, g, da)
    assert torch.equal(g, dx)
    z = gs.tensor(x, "x in place")[off:]
    hip.prelu_fwd(z, ad, z)
    assert torch.equal(z, y)


def test_row_dot_and_row_scale_add_guarded(hip, gs):
    shape = B, C, H, W = 3, 176, 9, 13
    a, b, x = seeded_tensor(3, shape), seeded_tensor(4, shape), seeded_tensor(5, shape)
    s, t = seeded_tensor(6, (B, C)), seeded_tensor(7, (B, C))
    ad, bd, xd, sd, td = (gs.tensor(v) for v in (a, b, x, s, t))
    out = gs.empty((B, C), name="out")
    hip.row_dot(ad, None, out, 1.0 / (H * W))
    assert float((out.cpu().double() - a.double().mean((2, 3))).abs().max()) <= 2e-6 * float(a.double().abs().mean((2, 3)).max())
    hip.row_dot(ad, bd, out, 1.0)
    want = (a.double() * b.double()).sum((2, 3))
    assert float((out.cpu().double() - want).abs().max()) <= 2e-6 * float((a.double() * b.double()).abs().sum((2, 3)).max())
    y = gs.empty(shape, name="y")
    hip.row_scale_add(ad, sd, xd, None, 0.0, y)
    assert relerr(y, a.double() * s.double()[:, :, None, None] + x.double()) < 1e-6
    hip.row_scale_add(ad, sd, None, td, 0.25, y)
    assert relerr(y, a.double() * s.double()[:, :, None, None] + 0.25 * t.double()[:, :, None, None]) < 1e-6
    z = gs.tensor(a, "a in place")
    hip.row_scale_add(z, sd, xd, td, 0.25, z)
    assert relerr(z, a.double() * s.double()[:, :, None, None] + x.double() + 0.25 * t.double()[:, :, None, None]) < 1e-6


def test_ca_gate_guarded(hip, gs):
    B, C = 3, 176
    Cr = C // 4
    mean, dg = seeded_tensor(8, (B, C)), seeded_tensor(9, (B, C))
    W1, W2 = seeded_tensor(10, (Cr, C), scale=C ** -0.5), seeded_tensor(11, (C, Cr), scale=Cr ** -0.5)
    md, w1d, w2d = gs.tensor(mean, "mean"), gs.tensor(W1, "W1"), gs.tensor(W2, "W2")
    hid, gate = gs.empty((B, Cr), name="hid"), gs.empty((B, C), name="gate")
    hip.ca_gate_fwd(md, w1d, w2d, hid, gate)
    m64, a64, b64 = mean.double().requires_grad_(True), W1.double().requires_grad_(True), W2.double().requires_grad_(True)
    h64 = torch.relu(m64 @ a64.t())
    g64 = torch.sigmoid(h64 @ b64.t())
    assert relerr(hid, h64) < 2e-6 and relerr(gate, g64) < 2e-6
    g64.backward(dg.double())
    dW1, dW2, dmean = gs.full((Cr, C), 0.5, name="dW1"), gs.full((C, Cr), -0.25, name="dW2"), gs.empty((B, C), name="dmean")
    hip.ca_gate_bwd(gs.tensor(dg, "dgate"), gate, hid, md, w1d, w2d, dW1, dW2, dmean)
    assert relerr(dmean, m64.grad) < 5e-6
    assert relerr(dW1 - 0.5, a64.grad) < 5e-6 and relerr(dW2 + 0.25, b64.grad) < 5e-6


def test_bilinear_maps_guarded(hip, gs):
    shape = B, C, H, W = 1, 5, 6, 4                                       # odd half-size, a row of one float4
    x = seeded_tensor(12, shape)
    xd = gs.tensor(x, "x")
    y = gs.empty((B, C, H // 2, W // 2), name="down")
    hip.bilinear_down2(xd, y)
    x64 = x.double().requires_grad_(True)
    r = F.interpolate(x64, scale_factor=0.5, mode="bilinear", align_corners=False)
    assert relerr(y, r) < 1e-6
    g = seeded_tensor(13, tuple(r.shape))
    r.backward(g.double())
    acc = seeded_tensor(14, shape)
    dx, gd = gs.tensor(acc, "dx"), gs.tensor(g, "dy")
    hip.bilinear_down2_bwd(gd, dx, beta=1.0)
    assert relerr(dx, acc.double() + x64.grad) < 1e-6
    hip.bilinear_down2_bwd(gd, dx, beta=0.0)
    assert relerr(dx, x64.grad) < 1e-6
    skip = seeded_tensor(15, (B, C, 2 * H, 2 * W))
    y2 = gs.empty((B, C, 2 * H, 2 * W), name="up")
    hip.bilinear_up2(xd, gs.tensor(skip, "skip"), y2)
    x64 = x.double().requires_grad_(True)
    r2 = F.interpolate(x64, scale_factor=2, mode="bilinear", align_corners=False)
    assert relerr(y2, r2 + skip.double()) < 1e-6
    hip.bilinear_up2(xd, None, y2)
    assert relerr(y2, r2) < 1e-6
    g2 = seeded_tensor(16, tuple(r2.shape))
    r2.backward(g2.double())
    dx2 = gs.empty(shape, name="dx2")
    hip.bilinear_up2_bwd(gs.tensor(g2, "dy2"), dx2)
    assert relerr(dx2, x64.grad) < 2e-6


# ------------------------------------------------------------------ 3b. split-product kernels (test_x3_gpu.py's hand-rolled tests)
def _packs(gs, be, Wg, Co, Ci, fold=None, split=False, split6=False):
    """zeroed guarded weight packs, filled by pack_weight: (WT, WP, (WTf, c12) | None, s3 | None, s6 | None) as ``packed=`` takes them"""
    z = lambda s, name: gs.full(s, 0.0, name=name)
    WT, WP = (z(s, n) for s, n in zip(be.pack_shapes(Co, Ci), ("WT", "WP")))
    f = tuple(z(s, n) for s, n in zip(be.fold_shapes(Co, Ci), ("WTf", "c12"))) if fold else None
    s3 = s6 = None
    if split:
        (st,), (sp,) = be.split_shapes(Co, Ci)
        s3 = (z(st, "WTs"), z(sp, "WPs"), z(st, "WTfs") if fold else None)
    if split6:
        (st,), (sp,) = be.split6_shapes(Co, Ci)
        s6 = (z(st, "WTs6"), z(sp, "WPs6"), None)
    be.pack_weight(Wg, WT, WP, (*fold, *f) if fold else None, s3, s6)
    return WT, WP, f, s3, s6


def test_x3_is_the_split_kernel_guarded(gs):
    from rcot_amd import lib
    be = _backend("bf16x3")
    poison_workspaces(be)
    B, Ci, Co, N = 2, 96, 510, 4096
    W, X = gs.tensor(seeded_tensor(1, (Co, Ci), scale=0.1), "W"), gs.tensor(seeded_tensor(2, (B, Ci, N)), "X")
    dY = gs.tensor(seeded_tensor(3, (B, Co, N)), "dY")
    WT, WP = _packs(gs, be, W, Co, Ci)[:2]
    outs = {}
    for name, prec in (("fp32", lib.PREC_FP32), ("x3", lib.PREC_BF16X3)):
        be.prec = prec
        Y, dW, G = gs.full((B, Co, N), 0.0), gs.full((Co, Ci), 0.0), gs.full((B, 1, Ci, Ci), 0.0)
        be.conv1x1_fwd(W, X, Y, packed=(WT, WP))
        be.conv1x1_wgrad(dY, X, dW, beta=0.0)
        be.bmm_nt(X.unsqueeze(1), X.unsqueeze(1), G)
        outs[name] = (Y, dW, G)
    torch.cuda.synchronize()
    for a, b in zip(outs["x3"], outs["fp32"]):
        assert not torch.equal(a, b)
        assert relerr(a, b) < 4e-5


def _ln_case(B, Ci, Co, N, ratio):
    W, lw, lb = seeded_tensor(1, (Co, Ci), scale=0.1), 1 + 0.1 * seeded_tensor(3, (Ci,)), 0.1 * seeded_tensor(4, (Ci,))
    X = seeded_tensor(2, (B, Ci, N)) + ratio * (1 + 0.2 * seeded_tensor(12, (B, 1, N)))
    Xd = X.double()
    mu = Xd.mean(1, keepdim=True)
    rstd = (Xd.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    ref = torch.einsum("oc,bcn->bon", W.double(), (Xd - mu) * rstd * lw.double().view(1, Ci, 1) + lb.double().view(1, Ci, 1))
    return W, lw, lb, X, mu, rstd, ref


def test_x3_ln_fold_guarded(gs):
    be = _backend("bf16x3")
    poison_workspaces(be)
    B, Ci, Co, N, ratio = 2, 96, 288, 4096, 20.0
    W, lw, lb, X, _, _, ref = _ln_case(B, Ci, Co, N, ratio)
    Wg, Xg, lwg, lbg = (gs.tensor(t) for t in (W, X, lw, lb))
    WT, WP, f, s3, _ = _packs(gs, be, Wg, Co, Ci, fold=(lwg, lbg), split=True)
    mu_, rs_ = gs.full((B, N), 0.0, name="mu"), gs.full((B, N), 0.0, name="rs")
    be.ln_stats(Xg, mu_, rs_)
    Y = gs.full((B, Co, N), 0.0, name="Y")
    be.conv1x1_fwd(Wg, Xg, Y, ln=(mu_, rs_, lwg, lbg), packed=(WT, WP, f, s3))
    torch.cuda.synchronize()
    assert relerr(Y, ref) < 1e-5 * (1 + ratio)


def test_x3_ln_statistics_guarded(gs):
    be = _backend("bf16x3")
    poison_workspaces(be)
    B, Ci, Co, N, ratio, fused = 3, 100, 130, 768, 1.0, False              # K % 16 != 0, a padded row tile: declined, rcot_ln_stats first
    W, lw, lb, X, mu, rstd, ref = _ln_case(B, Ci, Co, N, ratio)
    Wg, Xg, lwg, lbg = (gs.tensor(t) for t in (W, X, lw, lb))
    WT, WP, f, s3, _ = _packs(gs, be, Wg, Co, Ci, fold=(lwg, lbg), split=True)
    mu_, rs_ = gs.full((B, N), float("nan"), name="mu"), gs.full((B, N), float("nan"), name="rs")
    Y = gs.full((B, Co, N), float("nan"), name="Y")
    calls = []
    orig = be.ln_stats
    be.ln_stats = lambda *a: (calls.append(1), orig(*a))
    try:
        be.conv1x1_fwd(Wg, Xg, Y, ln=(mu_, rs_, lwg, lbg), packed=(WT, WP, f, s3), ln_compute=True)
    finally:
        del be.ln_stats
    torch.cuda.synchronize()
    assert (len(calls) == 0) == fused, "which path made the statistics"
    e_mu = float((mu_.double().cpu() - mu[:, 0]).abs().max() / mu.abs().max())
    e_rs = float((rs_.double().cpu() / rstd[:, 0] - 1).abs().max())
    assert e_mu < 2e-6 and e_rs < 2e-5 * (1 + ratio) and relerr(Y, ref) < 1e-5 * (1 + ratio)


def test_x3_paired_dgrad_wgrad_guarded(gs):
    be = _backend("bf16x3")
    poison_workspaces(be)
    B, Ci, Co, N = 8, 96, 255, 1152                                       # a ragged row tile on a 128-column plane, LayerNorm in the loop
    W, dY, X = seeded_tensor(1, (Co, Ci), scale=0.1), seeded_tensor(2, (B, Co, N)), seeded_tensor(3, (B, Ci, N)) + 0.5
    lw, lb = 1 + 0.1 * seeded_tensor(4, (Ci,)), 0.1 * seeded_tensor(5, (Ci,))
    Wg, dYg, Xg = gs.tensor(W, "W"), gs.tensor(dY, "dY"), gs.tensor(X, "X")
    WT, WP, _, s3, _ = _packs(gs, be, Wg, Co, Ci, split=True)
    mu, rs = gs.full((B, N), 0.0, name="mu"), gs.full((B, N), 1.0, name="rs")
    be.ln_stats(Xg, mu, rs)
    dX = gs.full((B, Ci, N), float("nan"), name="dX")
    gW0 = seeded_tensor(6, (Co, Ci))
    gW = gs.tensor(gW0, "gW")
    d = be.conv1x1_dgrad_wgrad_slabs(Wg, dYg, dX, Xg, gW, ln=(mu, rs, gs.tensor(lw, "lw"), gs.tensor(lb, "lb")),
                                     packed=(WT, WP, None, s3), region=(1, 3))
    assert d is not None
    zc = lambda *sh: gs.full(sh, 0.0)
    for sc in be._ln_scratch[be._gen]:
        sc[:2 * Ci].zero_()                                               # one row of zero LayerNorm partials: the rest stays NaN
    be._ln_rows = 1
    be.block_param_reduce(Ci, zc(Ci), zc(Ci), zc(Ci), zc(Ci), zc(B, Ci, Ci), zc(Ci, Ci), zc(B, 1), zc(1), [d])
    torch.cuda.synchronize()
    Xd = X.double()
    m = Xd.mean(1, keepdim=True)
    r = (Xd.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    Xd = (Xd - m) * r * lw.double().view(1, Ci, 1) + lb.double().view(1, Ci, 1)
    e1 = relerr(dX, torch.einsum("oc,bon->bcn", W.double(), dY.double()))
    e2 = relerr(gW, gW0.double() + torch.einsum("bon,bcn->oc", dY.double(), Xd))
    assert e1 < 4e-5 and e2 < 4e-5, (e1, e2)


def test_x6_is_as_accurate_as_the_fp32_kernel_guarded(gs):
    from rcot_amd import lib
    be = _backend("bf16x6")
    poison_workspaces(be)
    B, Ci, Co, N = 8, 1021, 384, 256                                      # a K tail on split-K planes
    W, X = seeded_tensor(1, (Co, Ci), scale=0.1), seeded_tensor(2, (B, Ci, N)) + 0.5
    ref = torch.einsum("oc,bcn->bon", W.double(), X.double())
    Wg, Xg = gs.tensor(W, "W"), gs.tensor(X, "X")
    WT, WP, _, s3, s6 = _packs(gs, be, Wg, Co, Ci, split=True, split6=True)
    errs, outs = {}, {}
    for name, prec in (("fp32", lib.PREC_FP32), ("bf16x3", lib.PREC_BF16X3), ("bf16x6", lib.PREC_BF16X6)):
        be.prec = prec
        Y = gs.full((B, Co, N), float("nan"), name=f"Y {name}")
        be.conv1x1_fwd(Wg, Xg, Y, packed=(WT, WP, None, s3, s6))
        torch.cuda.synchronize()
        errs[name], outs[name] = relerr(Y, ref), Y
    assert errs["bf16x6"] <= 1.5 * errs["fp32"] + 5e-8
    assert errs["bf16x3"] > 4 * errs["bf16x6"]
    assert not torch.equal(outs["bf16x6"], outs["fp32"]) and not torch.equal(outs["bf16x6"], outs["bf16x3"])


def test_x6_pixel_reductions_guarded(gs):
    from rcot_amd import lib
    be = _backend("bf16x6")
    poison_workspaces(be)
    B, Ci, Co, N = 4, 96, 510, 4096
    X, dY = seeded_tensor(2, (B, Ci, N)) + 0.5, seeded_tensor(3, (B, Co, N))
    ref_w = torch.einsum("bon,bcn->oc", dY.double(), X.double())
    ref_g = torch.einsum("bcn,bdn->bcd", X.double(), X.double()).unsqueeze(1)
    Xg, dYg = gs.tensor(X, "X"), gs.tensor(dY, "dY")
    errs, outs = {}, {}
    for name, prec in (("fp32", lib.PREC_FP32), ("bf16x3", lib.PREC_BF16X3), ("bf16x6", lib.PREC_BF16X6)):
        be.prec = prec
        dW, G = gs.full((Co, Ci), 0.0, name=f"dW {name}"), gs.full((B, 1, Ci, Ci), 0.0, name=f"G {name}")
        be.conv1x1_wgrad(dYg, Xg, dW, beta=0.0)
        be.bmm_nt(Xg.unsqueeze(1), Xg.unsqueeze(1), G)
        torch.cuda.synchronize()
        errs[name], outs[name] = (relerr(dW, ref_w), relerr(G, ref_g)), (dW, G)
    for i in range(2):
        assert errs["bf16x6"][i] <= 1.5 * errs["fp32"][i] + 5e-8
        assert errs["bf16x3"][i] > 3 * errs["bf16x6"][i]
        assert not torch.equal(outs["bf16x6"][i], outs["fp32"][i]) and not torch.equal(outs["bf16x6"][i], outs["bf16x3"][i])


def test_cooperative_split_guarded(gs):
    be = _backend("bf16x3")
    poison_workspaces(be)
    B, Ci, Co, N = 2, 127, 48, 1024                                       # odd channel count, fewer rows than a tile
    X, dY = gs.tensor(seeded_tensor(2, (B, Ci, N)) + 0.5, "X"), gs.tensor(seeded_tensor(3, (B, Co, N)), "dY")
    outs = []
    try:
        for c in (3, 0):
            assert be.L.rcot_debug_nt_coop(c) == 0
            dW, G = gs.full((Co, Ci), 0.0, name=f"dW coop={c}"), gs.full((B, 1, Ci, Ci), 0.0, name=f"G coop={c}")
            be.conv1x1_wgrad(dY, X, dW, ln=None, beta=0.0)
            be.bmm_nt(X.unsqueeze(1), X.unsqueeze(1), G)
            torch.cuda.synchronize()
            outs.append((dW, G))
    finally:
        be.L.rcot_debug_nt_coop(-1)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert all_finite(outs[0][0]) and float(outs[0][0].abs().max()) > 0


def _bf(t):
    return t.float().bfloat16().double()


def test_x1_single_products_guarded(gs):
    be, be3 = _backend("bf16x1"), _backend("bf16x3")
    poison_workspaces(be)
    poison_workspaces(be3)
    B, Ci, Co, N = 2, 255, 96, 256                                        # a K tail
    W, X, dY = seeded_tensor(1, (Co, Ci), scale=0.1), seeded_tensor(2, (B, Ci, N)), seeded_tensor(3, (B, Co, N))
    Wg, Xg, dYg = gs.tensor(W, "W"), gs.tensor(X, "X"), gs.tensor(dY, "dY")
    WT, WP, _, s3, _ = _packs(gs, be, Wg, Co, Ci, split=True)
    packed = (WT, WP, None, s3)
    outs = {}
    for name, b in (("x1", be), ("x3", be3)):
        Y, dX = gs.full((B, Co, N), float("nan"), name=f"Y {name}"), gs.full((B, Ci, N), float("nan"), name=f"dX {name}")
        b.conv1x1_fwd(Wg, Xg, Y, packed=packed)
        b.conv1x1_dgrad(Wg, dYg, dX, packed=packed)
        torch.cuda.synchronize()
        outs[name] = (Y, dX)
    if be.kmajor_worth(Co, N, B):
        got, exact = outs["x1"][0], torch.einsum("oc,bcn->bon", W.double(), X.double())
        assert relerr(got, torch.einsum("oc,bcn->bon", _bf(W), _bf(X))) < 2e-5
        assert 2e-4 < relerr(got, exact) < 2e-2
        assert not torch.equal(got, outs["x3"][0])
    if be.kmajor_worth(Ci, N, B):
        assert relerr(outs["x1"][1], torch.einsum("oc,bon->bcn", _bf(W), _bf(dY))) < 2e-5
    B, Ci, Co, N = 8, 384, 1152, 256                                      # the pixel reductions: split-K on 256-pixel planes
    X, dY = seeded_tensor(2, (B, Ci, N)), seeded_tensor(3, (B, Co, N))
    Xg, dYg = gs.tensor(X, "X wgrad"), gs.tensor(dY, "dY wgrad")
    dW, G = gs.full((Co, Ci), 0.0, name="dW"), gs.full((B, 1, Ci, Ci), float("nan"), name="G")
    be.conv1x1_wgrad(dYg, Xg, dW, beta=0.0)
    be.bmm_nt(Xg.view(B, 1, Ci, N), Xg.view(B, 1, Ci, N), G)
    torch.cuda.synchronize()
    assert relerr(dW, torch.einsum("bon,bcn->oc", _bf(dY), _bf(X))) < 2e-5
    assert relerr(G[:, 0], torch.einsum("bin,bjn->bij", _bf(X), _bf(X))) < 2e-5


# ------------------------------------------------------------------ 4. whole paths: the backend allocates from the set
def _iteration(ps, de, prec, tol):
    """one paired minimax iteration at B = 2 with every tensor of the networks, the optimisers and the schedule from a GuardSet and the
    workspaces poisoned, against the same MinimaxStep on the fp64 double: helpers and bars of
    tests/test_ot_sizes_gpu.py::test_iteration_at_new_sizes (same key, so the fp64 side is computed once per session)"""
    from rcot_amd.net_restormer import F_net, T_net
    from rcot_amd.trainer import FlatOptimizer, MinimaxStep
    B, paired = 2, True
    want, want_snap = _host_iteration(ps, B, de, paired)
    be = _backend(prec)
    deg, clean, alpha = _inputs(ps, B, de, paired)
    gs = GuardSet("cuda")
    snaps = {}
    with gs.adopt(be):
        Tn, Fn = T_net(decoder=True, backend=be), F_net(patch_size=ps, backend=be)
        Tn.load_state_dict(_np_params(P.tnet_param_shapes(), 41, "T"))
        Fn.load_state_dict(_np_params(P.fnet_param_shapes(ps), 42, "F"))
        st = MinimaxStep(Tn, Fn, FlatOptimizer(Tn, "RMSprop", 0.5e-4), FlatOptimizer(Fn, "RMSprop", 1e-4), 1.0, 10000.0)
        st.set_de_ids(de)
        st.grad_probe = lambda where: snaps.__setitem__(where, _snapshot(Tn, 128)) if where == "T_gen" else None
        st.iteration(gs.tensor(deg, "deg"), gs.tensor(clean, "clean"), gs.tensor(torch.tensor(de, dtype=torch.int32), "de_id"),
                     gs.tensor(alpha, "alpha"), paired)
        be.side_join()
        torch.cuda.synchronize()
        s = st.scalars()
    print(f"[guarded iteration P={ps} {prec}] {len(gs.items)} guarded tensors; hip {s} vs fp64 host {want}")
    ltol = {"Loss_F": 1e-3, "Loss_T": 5e-3, "Loss_mse": 1e-3, "gp": 1e-3}
    for k in ltol:
        assert abs(s[k] - want[k]) <= ltol[k] * max(abs(want[k]), 1e-3), (k, s[k], want[k])
    names, shapes = [n for n, _ in P.tnet_param_shapes()], [sh for _, sh in P.tnet_param_shapes()]
    gn = np.array([w[0] for w in want_snap])
    gsamp = np.concatenate([w[1] for w in want_snap])
    _compare(snaps["T_gen"], names, gn, gsamp, 128, shapes, tol, "T after generator loss")


# 32 is the smallest size check_patch_size accepts: planes go down to 4 x 4
@pytest.mark.parametrize("prec,tol", [("fp32", 2e-3), ("bf16x3", 1e-2), ("bf16x6", 2e-3)])
def test_iteration_at_32_on_guarded_tensors(prec, tol):
    _iteration(32, [0, 3], prec, tol)


# planes of 96 / 48 / 24 / 12: every non-fused stencil route, the general attention route, the mixed-radix FFT
@pytest.mark.parametrize("prec,tol", [("fp32", 2e-3), ("bf16x3", 1e-2)])
def test_iteration_at_96_on_guarded_tensors(prec, tol):
    _iteration(96, [3, 4], prec, tol)


def test_mprnet_iteration_on_guarded_tensors(hip):
    """MPRNetHip forward and backward at 2 x 3 x 20 x 28 against the stock-ops form, every element of every gradient, as
    tests/test_mprnet_gpu.py::test_mprnet_hip_vs_stock_ops_every_gradient compares"""
    from rcot_amd.mprnet_hip import MPRNetHip
    ref = MP.MPRNetT(seed=5)
    x, r = seeded_tensor(31, (2, 3, 20, 28), lo=0.0, hi=1.0), seeded_tensor(32, (2, 3, 20, 28))
    yr = ref(x)
    (yr * r).sum().backward()
    gs = GuardSet("cuda")
    with gs.adopt(hip):
        net = MPRNetHip(backend=hip, seed=5)
        sd = net.state_dict()
        assert all(torch.equal(sd[k].cpu(), v.detach()) for k, v in ref.p.items())
        net.zero_grad()
        y = net.forward(gs.tensor(x, "x"), save=True)
        net.backward(gs.tensor(r, "r"))
        hip.side_join()
        torch.cuda.synchronize()
    assert relerr(y, yr) < 1e-5
    seen = set()
    for n, _ in MP.mprnet_param_shapes():
        t = ref.p[n]
        if id(t) in seen:
            continue
        seen.add(id(t))
        key = net.slope_name if n.endswith("body.1.weight") else n
        if t.grad is None:
            assert float(net.store.g[key].abs().max()) == 0.0, n
        else:
            assert relerr(net.store.g[key], t.grad) < 5e-5, (n, relerr(net.store.g[key], t.grad))


def test_restormer_inference_on_guarded_tensors(hip):
    """a 37 x 45 uint8 image through wholeimage.restore_any_size(pad="reflect"), whole and as 32 x 32 tiles with overlap 8, linear
    window, one batch per shape class and the x8 self-ensemble; against T_net on the fp64 double applied to the F.pad-ded image (view by
    view for the tiled form, blended by the numpy restatement); the fp32 bar of tests/test_anysize_gpu.py"""
    from rcot_amd.net_restormer import T_net
    from rcot_amd.wholeimage import restore_any_size
    h, w, Hp, Wp = 37, 45, 40, 48
    img = torch.from_numpy(np.random.Generator(np.random.PCG64(3745)).integers(0, 256, size=(h, w, 3), dtype=np.uint8))
    xp = F.pad(img.permute(2, 0, 1).float().div(255)[None], (0, Wp - w, 0, Hp - h), mode="reflect")
    host = T_net(decoder=True, backend=DBL, seed=0)
    host.load_state_dict({k: v.double() for k, v in _tparams(11).items()})
    want_whole = host(xp.double())
    p = TL.plan(Hp, Wp, 32, 8, 8, 8)
    assert p.n_views == 32 and p.shape_classes() == [(0, 32, 32, 32)]
    cut = []
    for m in p.modes:
        for y0 in p.ys:
            for x0 in p.xs:
                v = torch.rot90(xp[0, :, y0:y0 + p.Th, x0:x0 + p.Tw], m // 2, dims=(1, 2))
                cut.append((torch.flip(v, dims=(1,)) if m & 1 else v).contiguous())
    restored = host(torch.stack(cut).double()).float().numpy()
    want_tiled = torch.from_numpy(blend_views(list(restored), 3, Hp, Wp, p.ys, p.xs, p.modes, p.Th, p.Tw, TL.window_taps(p.Th, p.ov_y, "linear"),
                                              TL.window_taps(p.Tw, p.ov_x, "linear")))
    gs = GuardSet("cuda")
    with gs.adopt(hip):
        net = T_net(decoder=True, backend=hip)
        net.load_state_dict(_tparams(11))
        imgd = gs.tensor(img, "img")
        whole = restore_any_size(net, imgd, net.size_multiple, "reflect")
        tiled = restore_any_size(net, imgd, net.size_multiple, "reflect", tile=32, overlap=8, window="linear", tile_batch=0, ensemble=8)
        torch.cuda.synchronize()
    assert (whole.h, whole.w, whole.Hp, whole.Wp) == (h, w, Hp, Wp) and torch.equal(whole.x.cpu(), xp) and torch.equal(tiled.x.cpu(), xp)
    e1, e2 = relerr(whole.out[..., :h, :w], want_whole[..., :h, :w]), relerr(tiled.out[0, :, :h, :w], want_tiled[:, :h, :w])
    print(f"guarded inference 37x45: whole {e1:.2e}, 32 blended views {e2:.2e}")
    assert e1 < 2e-5 and e2 < 2e-5
    assert all_finite(whole.out) and all_finite(tiled.out)
