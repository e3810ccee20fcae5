"""GPU tier: the batched image entry points of the validation suite (csrc/imageio.hip: rcot_image_ingest_batch,
rcot_image_egress_batch) against the single-image kernels they share their device code with, bit for bit, and the network on a batch
that the batched ingest made.

 1. ingest, batch against single: images of different sizes in one arena (the second starts at an odd byte), every padding mode, more
    than one 256-column tile, N = 1;
 2. egress, batch against single: the 8-bit outputs and the four statistics as int64 bits, images with and without SSIM rows, two column
    tiles, rows with and without an 8-bit output, values outside [0, 1], a poisoned workspace;
 3. refusals: nothing is launched — every output keeps its poison;
 4. the whole network on a batch of three 161 x 241 images, slot 0 against the REFERENCE's output (tests/golden/wholeimage.npz) under
    the bars of tests/test_inference_shapes_gpu.py.

Every device tensor comes from a GuardSet and the bands are checked (tests/guarded.py).
"""
import numpy as np
import pytest
import torch

from conftest import relerr, seeded_tensor
from guarded import GuardSet, all_finite, poison_workspaces

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from rcot_amd.ops import HipBackend
    return HipBackend()


def _arena(gs, sizes, seed, name="arena"):
    """uint8 images of ``sizes`` packed back to back in one guarded allocation -> the views [h, w, 3]"""
    g = np.random.Generator(np.random.PCG64(seed))
    total = sum(3 * h * w for h, w in sizes)
    arena = gs.tensor(torch.from_numpy(g.integers(0, 256, total, dtype=np.uint8)), name)
    views, off = [], 0
    for h, w in sizes:
        views.append(arena[off:off + 3 * h * w].view(h, w, 3))
        off += 3 * h * w
    return views


def _poisoned(t) -> bool:
    """every 4-byte word of a fresh GuardSet tensor is a NaN pattern"""
    return bool(torch.isnan(t.flatten().view(torch.uint8)[:t.numel() * t.element_size() // 4 * 4].view(torch.float32)).all())


# ============================================================================= 1. ingest
INGEST = [("reflect", [(13, 21), (16, 24), (9, 17)], 16, 24), ("replicate", [(13, 21), (16, 24), (9, 17)], 16, 24),
          ("none", [(16, 24)] * 3, 16, 24), ("reflect", [(12, 300), (9, 297)], 16, 304), ("replicate", [(5, 3)], 8, 8)]


@pytest.mark.parametrize("mode,sizes,Hp,Wp", INGEST, ids=[f"{m}-{len(s)}x{Hp}x{Wp}" for m, s, Hp, Wp in INGEST])
def test_ingest_batch_equals_single(hip, mode, sizes, Hp, Wp):
    gs = GuardSet("cuda")
    imgs = _arena(gs, sizes, 3)
    if len(sizes) > 1 and sizes[0] == (13, 21):
        assert imgs[1].data_ptr() % 2 == 1                          # the second image starts at an odd byte
    out = gs.empty((len(sizes), 3, Hp, Wp), name="out")
    got = hip.image_ingest_batch(imgs, Hp, Wp, mode, out=out)
    want = [hip.image_ingest(im.clone(), Hp, Wp, mode) for im in imgs]
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and all_finite(out)
    for i, w in enumerate(want):
        assert torch.equal(out[i], w[0]), (mode, i)
        assert torch.equal(out[i], hip.image_ingest(imgs[i], Hp, Wp, mode)[0]), (mode, i)   # the single kernel at the odd address too
    gs.check()


def test_ingest_batch_unaligned_out_takes_the_scalar_stores(hip):
    """Wp = 22: no float4 path; the bits stay the single kernel's"""
    gs = GuardSet("cuda")
    sizes = [(13, 21), (16, 22), (9, 17)]
    imgs = _arena(gs, sizes, 4)
    out = gs.empty((3, 3, 16, 22), name="out")
    hip.image_ingest_batch(imgs, 16, 22, "replicate", out=out)
    for i, im in enumerate(imgs):
        assert torch.equal(out[i], hip.image_ingest(im, 16, 22, "replicate")[0]), i
    gs.check()


# ============================================================================= 2. egress
EGRESS = [([(13, 21), (16, 24), (9, 17)], 16, 24), ([(40, 300), (13, 21), (9, 17), (33, 290)], 40, 304), ([(16, 22), (12, 13)], 16, 22),
          ([(13, 21)], 16, 24)]


@pytest.mark.parametrize("sizes,Hp,Wp", EGRESS, ids=[f"{len(s)}x{Hp}x{Wp}" for s, Hp, Wp in EGRESS])
def test_egress_batch_equals_single(hip, sizes, Hp, Wp):
    N = len(sizes)
    gs = GuardSet("cuda")
    targets = _arena(gs, sizes, 5, "targets")
    restored = gs.tensor(0.5 + 0.6 * seeded_tensor(6, (N, 3, Hp, Wp)), "restored")           # values below 0 and above 1
    assert float(restored.min()) < 0.0 and float(restored.max()) > 1.0
    out_sizes = [s for i, s in enumerate(sizes) if i != 1]                                    # row 1 (if any): statistics only
    out_views = _arena(gs, out_sizes, 7, "outs")
    before = [o.clone() for o in out_views]
    outs = [None if i == 1 else out_views[i - (i > 1)] for i in range(N)]
    stats = gs.empty((N, 4), torch.float64, "stats")
    ws = gs.empty((hip.image_egress_batch_ws_bytes(N, Hp, Wp) // 4,), name="ws")               # exactly what the header asks for, NaN
    poison_workspaces(hip)
    hip.image_egress_batch(restored, sizes, targets, ws=ws, outs=outs, stats=stats)
    torch.cuda.synchronize()
    for i, (h, w) in enumerate(sizes):
        o, _, st = hip.image_egress(restored[i], h, w, target=targets[i].clone(), want_out=True, want_stats=True)
        if outs[i] is not None:
            assert torch.equal(outs[i], o), i
        assert torch.equal(stats[i].view(torch.int64), st.view(torch.int64)), (i, stats[i].tolist(), st.tolist())
        assert (float(stats[i, 3]) == 0.0) == (h < 11 or w < 11), i
    assert all(not torch.equal(b, o) for b, o in zip(before, out_views))
    gs.check()
    # the 8-bit outputs alone: one launch, no statistics, no workspace read
    outs2 = _arena(gs, sizes, 8, "outs, no statistics")
    got, none = hip.image_egress_batch(restored, sizes, outs=outs2)
    assert none is None
    for i, (h, w) in enumerate(sizes):
        assert torch.equal(got[i], hip.image_egress(restored[i], h, w)[0]), i
    gs.check()


# ============================================================================= 3. refusals
def test_refusals_launch_nothing(hip):
    from rcot_amd import lib
    gs = GuardSet("cuda")
    sizes = [(13, 21), (16, 24)]
    imgs = _arena(gs, sizes, 9)
    out = gs.empty((2, 3, 16, 24), name="out")
    table = torch.tensor([imgs[0].data_ptr(), 13, 21, 0, imgs[1].data_ptr(), 16, 24, 0], dtype=torch.int64, device="cuda")
    L, st = hip.L, hip._st()
    assert L.rcot_image_ingest_batch(table.data_ptr(), 0, 16, 24, 1, out.data_ptr(), st) == -1
    assert L.rcot_image_ingest_batch(table.data_ptr(), 65536, 16, 24, 1, out.data_ptr(), st) == -1
    assert L.rcot_image_ingest_batch(None, 2, 16, 24, 1, out.data_ptr(), st) == -1
    assert L.rcot_image_ingest_batch(table.data_ptr(), 2, 16, 24, 1, None, st) == -1
    assert L.rcot_image_ingest_batch(table.data_ptr(), 2, 16, 24, 3, out.data_ptr(), st) == -1
    assert L.rcot_image_ingest_batch(table.data_ptr(), 2, 0, 24, 1, out.data_ptr(), st) == -1
    torch.cuda.synchronize()
    assert _poisoned(out)

    restored = gs.tensor(seeded_tensor(1, (2, 3, 16, 24)), "restored")
    o8 = [gs.empty((h, w, 3), torch.uint8, f"out_u8 {i}") for i, (h, w) in enumerate(sizes)]
    stats = gs.empty((2, 4), torch.float64, "stats")
    need = hip.image_egress_batch_ws_bytes(2, 16, 24)
    assert need == 24 * 2 * 4 * 1
    ws = gs.empty((need // 4,), name="ws")
    et = torch.tensor([imgs[0].data_ptr(), o8[0].data_ptr(), 13, 21, imgs[1].data_ptr(), o8[1].data_ptr(), 16, 24], dtype=torch.int64,
                      device="cuda")
    a = (restored.data_ptr(), et.data_ptr())
    assert L.rcot_image_egress_batch(*a, 0, 16, 24, stats.data_ptr(), ws.data_ptr(), need, st) == -1
    assert L.rcot_image_egress_batch(None, et.data_ptr(), 2, 16, 24, stats.data_ptr(), ws.data_ptr(), need, st) == -1
    assert L.rcot_image_egress_batch(restored.data_ptr(), None, 2, 16, 24, stats.data_ptr(), ws.data_ptr(), need, st) == -1
    assert L.rcot_image_egress_batch(*a, 2, 16, 24, stats.data_ptr(), ws.data_ptr(), need - 8, st) == -2
    assert L.rcot_image_egress_batch(*a, 2, 16, 24, stats.data_ptr(), ws.data_ptr() + 4, need, st) == -2
    assert L.rcot_image_egress_batch(*a, 2, 16, 24, stats.data_ptr(), None, need, st) == -2
    torch.cuda.synchronize()
    assert _poisoned(stats) and all(_poisoned(o) for o in o8) and _poisoned(ws)
    with pytest.raises(lib.RcotKernelError):
        hip.image_egress_batch(restored, sizes, imgs, outs=o8, stats=stats, ws=ws[:need // 4 - 2])
    torch.cuda.synchronize()
    assert _poisoned(stats) and all(_poisoned(o) for o in o8)

    # a bad row is refused by the host check: ValueError, nothing launched
    with pytest.raises(ValueError, match="row 1"):
        hip.image_ingest_batch([imgs[0], imgs[1][:, :20]], 16, 24, "reflect", out=out)          # not contiguous
    with pytest.raises(ValueError, match="row 0: reflect cannot pad 13 x 21 to 32 x 24"):
        hip.image_ingest_batch(imgs[:1], 32, 24, "reflect")
    with pytest.raises(ValueError, match="row 1"):
        hip.image_ingest_batch([imgs[0], imgs[1].cpu()], 16, 24, "reflect", out=out)
    with pytest.raises(ValueError, match="row 0: 17 x 21 is no crop"):
        hip.image_egress_batch(restored, [(17, 21), (16, 24)], imgs, outs=o8, stats=stats, ws=ws)
    with pytest.raises(ValueError, match="row 1: the target is 16 x 24"):
        hip.image_egress_batch(restored, [(13, 21), (15, 24)], imgs, want_out=False, want_stats=True, ws=ws)
    with pytest.raises(ValueError, match="row 0: neither"):
        hip.image_egress_batch(restored, sizes, want_out=[False, True])
    torch.cuda.synchronize()
    assert _poisoned(out) and _poisoned(stats) and all(_poisoned(o) for o in o8)
    gs.check()


# ============================================================================= 4. the network on a batch made by the batched ingest
@pytest.fixture(scope="module")
def whole_net():
    """the recipe of tests/test_inference_shapes_gpu.py: seeded parameters, seed 11"""
    from rcot_amd import params as P
    from rcot_amd.net_restormer import T_net
    from rcot_amd.ops import HipBackend
    net = T_net(decoder=True, backend=HipBackend())
    net.load_state_dict({k: torch.from_numpy(v) for k, v in P.seeded_params(P.tnet_param_shapes(), 11, "T").items()})
    return net


@pytest.mark.parametrize("prec,bar", [("fp32", 2e-5), ("bf16x3", 1e-4)])
def test_network_on_a_batch_of_three_vs_reference(whole_net, gold, prec, bar):
    """Three 161 x 241 images reflect-padded to 168 x 248 in ONE network call (the 1/8 plane is 21 x 31: the ``wmask`` path at B = 3).
    Slot 0 is the fixture's float input through pad2d and is held against the REFERENCE's output under the bars of
    test_whole_image_161x241_vs_reference; slots 1 and 2 are seeded 8-bit images through rcot_image_ingest_batch.  Slot 1 is compared
    with what the network gives for it alone: two evaluations that each lie within the bar of the exact result differ by at most twice
    the bar (the launch shapes, and with them the summation orders, differ between B = 3 and B = 1: no bit equality is promised)."""
    from rcot_amd import lib
    be = whole_net.be
    fx = gold("wholeimage.npz")
    B, h, w, seed, pseed = (int(v) for v in fx["cfg"])
    assert (B, h, w, pseed) == (1, 161, 241, 11)
    x0 = seeded_tensor(seed, (1, 3, h, w), lo=0.0, hi=1.0)
    gs = GuardSet("cuda")
    imgs = _arena(gs, [(h, w), (h, w)], 12)
    xb = gs.empty((3, 3, 168, 248), name="batch")
    old = (be.prec, getattr(be, "x6_packs", False))
    be.prec = {"fp32": lib.PREC_FP32, "bf16x3": lib.PREC_BF16X3}[prec]
    try:
        be.pad2d(gs.tensor(x0, "x0"), 168, 248, "reflect", out=xb[:1])
        be.image_ingest_batch(imgs, 168, 248, "reflect", out=xb[1:])
        out = whole_net(xb)
        alone = whole_net(xb[1:2].contiguous())
        torch.cuda.synchronize()
    finally:
        be.prec, be.x6_packs = old
    assert tuple(out.shape) == (3, 3, 168, 248) and all_finite(out)
    e = relerr(out[0, :, :h, :w], torch.from_numpy(fx["y"])[0])
    e1 = relerr(out[1], alone[0])
    print(f"batch of three 161x241 {prec}: slot 0 vs reference {e:.3e}, slot 1 vs alone {e1:.3e}, bar {bar:.1e}")
    assert e < bar, e
    assert e1 < 2 * bar, e1
    gs.check()
