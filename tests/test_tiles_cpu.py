"""CPU tier of tiled / self-ensemble inference (rcot_amd/tiles.py, csrc/views.hip): the numpy restatement of rcot_view_gather and
rcot_view_blend — the test double the GPU tier (tests/test_tiles_gpu.py) holds the kernels to, written from the definitions in
include/rcot_hip.h with np.rot90 / np.flipud —, the plan against the loops of ``tester.restore``, the window taps, the seam property the
blending window exists for, and the refusals of the two entry points (they return before any launch, so they need no device)."""
import ctypes as C

import numpy as np
import pytest
import torch

from rcot_amd import lib
from rcot_amd import tiles as TL

ALL8 = (0, 1, 4, 5, 2, 3, 6, 7)

# (H, W, tile, overlap, mult, modes): the geometries of the GPU tier, a .. h
GEOMETRIES = {
    "a": (8, 8, 8, 0, 8, ALL8),            # one window; every map on the smallest square
    "b": (8, 12, 8, 4, 4, (0,)),           # xs = [0, 4]: two-fold cover in x only
    "c": (24, 24, 16, 12, 4, (0,)),        # [0, 4, 8] on both axes: up to 9 views on one pixel
    "d": (8, 16, 0, 0, 8, ALL8),           # non-square whole image, views of 16 x 8
    "e": (40, 56, 0, 0, 8, ALL8),          # sides that are no multiple of 32: the edge of the LDS transpose tile
    "f": (72, 96, 40, 8, 8, ALL8),         # ys = [0, 32], xs = [0, 32, 56]: 48 views, several workgroups on each grid axis
    "g": (20, 28, 12, 4, 4, (0, 2)),       # the multiple-of-4 geometry of MPRNet, xs = [0, 8, 16]
    "h": (8, 1032, 520, 8, 8, (0, 3)),     # a row longer than one workgroup's column span
}


# ------------------------------------------------------------------ the test double of csrc/views.hip
def augment(a: np.ndarray, mode: int) -> np.ndarray:
    """the reference's data_augmentation (util/image_utils.py:133-163) on every plane of a [planes, h, w]"""
    return np.ascontiguousarray(np.stack([np.flipud(np.rot90(p, mode // 2)) if mode & 1 else np.rot90(p, mode // 2) for p in a]))


def unaugment(v: np.ndarray, mode: int) -> np.ndarray:
    """the inverse: undo the flip, then rotate back"""
    return np.ascontiguousarray(np.stack([np.rot90(np.flipud(p) if mode & 1 else p, -(mode // 2)) for p in v]))


def gather_views(img: np.ndarray, ys, xs, modes, Th: int, Tw: int):
    """rcot_view_gather: img float32 [planes, H, W] -> the views, a list in view order (mode-major, then rows of tiles, then columns)"""
    return [augment(img[:, y0:y0 + Th, x0:x0 + Tw], m) for m in modes for y0 in ys for x0 in xs]


def blend_views(views, planes: int, H: int, W: int, ys, xs, modes, Th: int, Tw: int, wy=None, wx=None) -> np.ndarray:
    """rcot_view_blend in numpy float32: num += w * a and den += w in ascending view order (one rounding each for w, w * a and the two
    sums), then one correctly rounded division"""
    num, den = np.zeros((planes, H, W), np.float32), np.zeros((H, W), np.float32)
    w = np.ones((Th, Tw), np.float32) if wy is None else (wy.astype(np.float32)[:, None] * wx.astype(np.float32)[None, :])
    assert w.dtype == np.float32
    v = 0
    for m in modes:
        for y0 in ys:
            for x0 in xs:
                a = unaugment(np.asarray(views[v], np.float32).reshape((planes, Tw, Th) if m & 2 else (planes, Th, Tw)), m)
                num[:, y0:y0 + Th, x0:x0 + Tw] += w * a
                den[y0:y0 + Th, x0:x0 + Tw] += w
                v += 1
    assert (den > 0).all()
    return num / den


def restore_loops(H, W, tile, overlap, mult):
    """the windows of the loops of ``tester.restore`` as they stand: (ys, xs, Th, Tw)"""
    if not tile or (tile >= H and tile >= W):
        return [0], [0], H, W
    tile = max(mult, tile // mult * mult)
    step = max(mult, (tile - overlap) // mult * mult)
    ys = sorted({min(y, max(H - tile, 0)) for y in range(0, H, step)})
    xs = sorted({min(c, max(W - tile, 0)) for c in range(0, W, step)})
    shapes = {(min(y0 + tile, H) - y0, min(x0 + tile, W) - x0) for y0 in ys for x0 in xs}
    assert len(shapes) == 1                                   # the clamped origins make every tile the same size
    return ys, xs, *shapes.pop()


def test_restatement_maps_are_inverse_and_shaped():
    a = np.arange(2 * 4 * 8, dtype=np.float32).reshape(2, 4, 8)
    for m in range(8):
        v = augment(a, m)
        assert v.shape == ((2, 8, 4) if m in (2, 3, 6, 7) else (2, 4, 8))
        assert np.array_equal(unaugment(v, m), a)
    assert np.array_equal(augment(a, 3)[0], a[0].T) and np.array_equal(augment(a, 1)[1], a[1][::-1])
    assert np.array_equal(augment(a, 2)[0][0], a[0][:, -1])   # rot90 counter-clockwise: the last column becomes the first row


# ------------------------------------------------------------------ plan() == the loops of tester.restore
def test_plan_equals_the_loops_of_restore():
    sweep = [(H, W, tile, ov, mult) for mult in (4, 8) for H in (8, 24, 40, 72, 200) for W in (8, 56, 96, 264)
             for tile in (0, 8, 12, 30, 32, 40, 64, 520) for ov in (0, 4, 8, 24, 32, 100)]
    sweep += [g[:5] for g in GEOMETRIES.values()]
    sweep += [(40, 56, 64, 8, 8), (40, 56, 40, 8, 8), (40, 200, 48, 8, 8),      # tile >= H (and >= W; and only >= H)
              (72, 96, 36, 8, 8), (72, 96, 7, 0, 8),                            # tile no multiple of mult (and below it)
              (72, 96, 32, 24, 8), (72, 96, 32, 28, 8), (72, 96, 32, 40, 8)]    # overlap >= tile - mult
    assert len(sweep) > 1500
    for H, W, tile, ov, mult in sweep:
        ys, xs, Th, Tw = restore_loops(H, W, tile, ov, mult)
        p = TL.plan(H, W, tile, ov, mult, 1)
        assert (list(p.ys), list(p.xs), p.Th, p.Tw, p.H, p.W) == (ys, xs, Th, Tw, H, W), (H, W, tile, ov, mult)
        assert p.modes == (0,) and TL.plan(H, W, tile, ov, mult, 8).modes == ALL8
        assert TL.plan(H, W, tile, ov, mult, 8)[:6] == p[:6]
        assert p.n_views == len(ys) * len(xs)
        # what the blend's refusals ask for holds for every plan: sorted origins from 0, no gap, the last window ends at the edge
        for o, T, L in ((ys, Th, H), (xs, Tw, W)):
            assert o[0] == 0 and o[-1] + T == L and all(0 < b - a <= T for a, b in zip(o, o[1:]))
    with pytest.raises(ValueError):
        TL.plan(8, 8, 0, 0, 8, 4)


def test_plan_origins_and_shape_classes_of_the_gpu_cases():
    want = {"a": ([0], [0], 8, 8), "b": ([0], [0, 4], 8, 8), "c": ([0, 4, 8], [0, 4, 8], 16, 16), "d": ([0], [0], 8, 16),
            "e": ([0], [0], 40, 56), "f": ([0, 32], [0, 32, 56], 40, 40), "g": ([0, 8], [0, 8, 16], 12, 12), "h": ([0], [0, 512], 8, 520)}
    for k, (H, W, tile, ov, mult, modes) in GEOMETRIES.items():
        p = TL.plan(H, W, tile, ov, mult, 1)
        assert (list(p.ys), list(p.xs), p.Th, p.Tw) == want[k], k
    assert TL.plan(72, 96, 40, 8, 8, 8).n_views == 48
    assert TL.plan(72, 96, 40, 8, 8, 8).shape_classes() == [(0, 48, 40, 40)]                         # square tiles: one shape
    assert TL.plan(32, 40, 0, 0, 8, 8).shape_classes() == [(0, 4, 32, 40), (4, 4, 40, 32)]           # two shapes of four
    assert TL.plan(40, 56, 32, 8, 8, 1).shape_classes() == [(0, 4, 32, 32)]
    p = TL.plan(8, 56, 32, 8, 8, 1)
    assert (p.ov_y, p.ov_x) == (0, 8) and TL.plan(72, 96, 36, 8, 8, 1).ov_x == 8 and TL.plan(72, 96, 32, 12, 8, 1).ov_x == 16


# ------------------------------------------------------------------ window taps
@pytest.mark.parametrize("kind", ["linear", "cosine"])
@pytest.mark.parametrize("T,ov", [(8, 4), (16, 8), (32, 8), (40, 8)])
def test_window_taps(kind, T, ov):
    w = TL.window_taps(T, ov, kind)
    assert w.dtype == np.float32 and w.shape == (T,) and (w > 0).all()
    assert np.array_equal(w, w[::-1])
    assert (w[ov:T - ov] == 1.0).all() and (w[:ov] < 1.0).all()
    w64 = TL._taps64(T, ov, kind)
    assert np.array_equal(w64.astype(np.float32), w)
    # across a regular overlap the neighbour's window starts T - ov further on: the two ramps sum to one
    assert np.abs(w64[T - ov:] + w64[:ov] - 1.0).max() < 1e-12
    if kind == "linear":
        assert np.allclose(w64[:ov], (np.arange(ov) + 1.0) / (ov + 1.0), rtol=0, atol=1e-15)


def test_window_taps_uniform_and_no_overlap():
    assert TL.window_taps(32, 8, "uniform") is None
    for kind in ("linear", "cosine"):
        assert np.array_equal(TL.window_taps(8, 0, kind), np.ones(8, np.float32))     # one window on the axis: equal weights
    with pytest.raises(ValueError):
        TL.window_taps(8, 4, "hann")


# ------------------------------------------------------------------ seams: what the window is for
def seam_errors(blend):
    """8 x 56 image, tile 32, overlap 8: two views at xs = [0, 24]; a network that is off by 0.02 k on view k.  ``blend(views, plan, x)``
    -> the column profile of out - x (the same in every row and plane, up to fp32 rounding)"""
    p = TL.plan(8, 56, 32, 8, 8, 1)
    assert (list(p.ys), list(p.xs), p.Th, p.Tw, p.ov_x) == ([0], [0, 24], 8, 32, 8)
    g = np.random.Generator(np.random.PCG64(56))
    x = g.uniform(0.0, 1.0, (3, 8, 56)).astype(np.float32)
    e = (np.asarray(blend(p, x), np.float64) - x).reshape(-1, 56)
    assert np.abs(e - e[0]).max() < 1e-6
    return e[0]


def check_seams(e_uniform, e_linear):
    # equal weights: a step of half the disagreement at either border of the overlap
    assert abs(e_uniform[24] - e_uniform[23]) >= 0.01 - 1e-6 and abs(e_uniform[32] - e_uniform[31]) >= 0.01 - 1e-6
    # the linear ramp has 9 steps across the overlap: no two neighbouring columns differ by more than one of them
    assert np.abs(np.diff(e_linear)).max() <= 0.02 / 9 + 1e-6
    want = np.concatenate([np.zeros(24), 0.02 * (np.arange(8) + 1.0) / 9.0, np.full(24, 0.02)])      # 0, 0.00222 .. 0.01778, 0.02
    assert np.abs(e_linear - want).max() < 1e-6


def test_seams_restated():
    def blend(kind):
        def run(p, x):
            views = gather_views(x, p.ys, p.xs, p.modes, p.Th, p.Tw)
            views = [v + np.float32(0.02 * k) for k, v in enumerate(views)]
            return blend_views(views, 3, p.H, p.W, p.ys, p.xs, p.modes, p.Th, p.Tw, TL.window_taps(p.Th, p.ov_y, kind),
                               TL.window_taps(p.Tw, p.ov_x, kind))
        return run
    check_seams(seam_errors(blend("uniform")), seam_errors(blend("linear")))


def test_restated_uniform_blend_is_the_average_of_restore():
    """NULL taps, modes {0}: acc / cnt of the loops of tester.restore, bit for bit (torch on the CPU, an elementwise stub network)"""
    from rcot_amd import tester as TS
    net = lambda t: t * 1.5 + 0.25
    for H, W, tile, ov, mult in [(24, 24, 16, 12, 4), (40, 56, 32, 8, 8), (8, 12, 8, 4, 4)]:
        x = torch.from_numpy(np.random.Generator(np.random.PCG64(H + W)).uniform(0, 1, (1, 3, H, W)).astype(np.float32))
        want = TS.restore(net, x, tile, ov, mult)
        p = TL.plan(H, W, tile, ov, mult, 1)
        views = [net(torch.from_numpy(v)).numpy() for v in gather_views(x[0].numpy(), p.ys, p.xs, p.modes, p.Th, p.Tw)]
        assert np.array_equal(blend_views(views, 3, H, W, p.ys, p.xs, p.modes, p.Th, p.Tw), want[0].numpy())


# ------------------------------------------------------------------ refusals of the C entry points (no launch: no device needed)
BASE = dict(planes=1, H=8, W=12, ys=[0], xs=[0, 4], modes=[0], Th=8, Tw=8)
MANY = list(range(0, 4 * 65, 4))                                        # 65 origins on one axis

# id -> what differs from BASE ("null" / "misalign": the pointer of that name; "taps": which of wy, wx is passed)
EINVAL_CASES = {
    "null img/views": dict(null="data"), "null out/views": dict(null="result"), "null ys": dict(null="ys"), "null xs": dict(null="xs"),
    "null modes": dict(null="modes"),
    "planes 0": dict(planes=0), "ny 0": dict(ys=[]), "nx 0": dict(xs=[]), "nm 0": dict(modes=[]),
    "mode 8": dict(modes=[8]), "mode -1": dict(modes=[-1]), "mode twice": dict(modes=[0, 3, 0]),
    "nine modes": dict(modes=[0, 1, 2, 3, 4, 5, 6, 7, 0]),
    "Th 0": dict(Th=0), "Th 2": dict(Th=2, H=2), "Th 6": dict(Th=6, ys=[0, 2]), "Tw 0": dict(Tw=0), "Tw 6": dict(Tw=6, xs=[0, 6]),
    "H 10": dict(H=10, Th=10), "W 10": dict(W=10, xs=[0, 2]),
    "origin 2": dict(xs=[0, 2, 4]), "origin y 2": dict(H=12, ys=[0, 2, 4]),
    "xs descending": dict(xs=[4, 0]), "xs repeated": dict(xs=[0, 4, 4]), "xs[0] 4": dict(xs=[4]), "xs gap": dict(W=16, Tw=4, xs=[0, 12]),
    "xs short": dict(W=16), "xs long": dict(W=8), "ys descending": dict(H=12, ys=[4, 0]), "ys[0] 4": dict(H=12, ys=[4]),
    "ys gap": dict(H=16, Th=4, ys=[0, 12]), "ys short": dict(H=16),
    "misaligned img/views": dict(misalign="data"), "misaligned out/views": dict(misalign="result"),
}
BLEND_ONLY_EINVAL = {"wy without wx": dict(taps="wy"), "wx without wy": dict(taps="wx"), "misaligned wy": dict(misalign="wy"),
                     "misaligned wx": dict(misalign="wx")}
EUNSUPPORTED_CASES = {"65 columns of tiles": dict(W=4 * 64 + 8, xs=MANY), "65 rows of tiles": dict(H=4 * 64 + 8, ys=MANY)}


def call_raw(L, which: str, case: dict, data: int, result: int, wy: int = 0, wx: int = 0) -> int:
    """``which`` ("gather" | "blend") on BASE changed by ``case``; data / result / wy / wx: addresses (16-byte aligned; 0 = NULL).
    For gather data is img and result views; for blend data is views and result out."""
    g = {**BASE, **{k: v for k, v in case.items() if k in BASE}}
    arr = lambda v: (C.c_int * max(len(v), 1))(*v)
    host = {k: arr(g[k]) for k in ("ys", "xs", "modes")}
    ptr = dict(data=data, result=result, wy=wy, wx=wx, **host)
    if case.get("taps") == "wy":
        ptr["wx"] = 0
    if case.get("taps") == "wx":
        ptr["wy"] = 0
    if "null" in case:
        ptr[case["null"]] = None
    if "misalign" in case:
        ptr[case["misalign"]] += 4
    a = (ptr["data"], g["planes"], g["H"], g["W"], ptr["ys"], len(g["ys"]), ptr["xs"], len(g["xs"]), ptr["modes"], len(g["modes"]),
         g["Th"], g["Tw"])
    if which == "gather":
        return L.rcot_view_gather(*a, ptr["result"], None)
    return L.rcot_view_blend(*a, ptr["wy"] or None, ptr["wx"] or None, ptr["result"], None)


@pytest.fixture(scope="module")
def buffers():
    """four 16-byte aligned addresses no kernel will touch: device memory where there is a device, host memory elsewhere"""
    if torch.cuda.is_available():
        keep = [torch.zeros(4096, device="cuda") for _ in range(4)]
        return keep, [t.data_ptr() for t in keep]
    keep = [np.zeros(4096 + 4, np.float32) for _ in range(4)]
    return keep, [(a.ctypes.data + 15) // 16 * 16 for a in keep]


@pytest.mark.parametrize("which", ["gather", "blend"])
def test_entry_points_refuse(which, buffers):
    L = lib.load()
    data, result, wy, wx = buffers[1]
    for with_taps in (False, True) if which == "blend" else (False,):
        taps = dict(wy=wy, wx=wx) if with_taps else {}
        for name, case in EINVAL_CASES.items():
            assert call_raw(L, which, case, data, result, **taps) == -1, (which, name)                 # RCOT_EINVAL
        for name, case in EUNSUPPORTED_CASES.items():
            assert call_raw(L, which, case, data, result, **taps) == lib.EUNSUPPORTED, (which, name)
    if which == "blend":
        for name, case in BLEND_ONLY_EINVAL.items():
            assert call_raw(L, which, case, data, result, wy=wy, wx=wx) == -1, name


def test_cli_flags_and_keywords():
    import inspect
    from rcot_amd import tester as TS
    from rcot_amd import wholeimage as WI
    o = TS.parser.parse_args([])
    assert (o.tile_window, o.tile_batch, o.ensemble) == ("uniform", 1, 1)
    o = TS.parser.parse_args(["--tile_window", "cosine", "--tile_batch", "0", "--ensemble", "8"])
    assert (o.tile_window, o.tile_batch, o.ensemble) == ("cosine", 0, 8)
    with pytest.raises(SystemExit):
        TS.parser.parse_args(["--ensemble", "4"])
    for fn in (TS.restore, WI.restore_any_size):
        prm = inspect.signature(fn).parameters
        assert [prm[k].default for k in ("window", "tile_batch", "ensemble")] == ["uniform", 1, 1]
    for flag in ("--tile_window", "--tile_batch", "--ensemble"):
        assert flag in TS.__doc__
