"""GPU tier: the launch that sums weight-gradient slab sets and nothing else (rcot_slab_sets_reduce) and the schedule that uses it
(TransformerBlockOp.backward with HipBackend.early_slab_sums: the project_out / project_in sets summed on the side stream right
behind their products, the closing launch left with the qkv set).

The kernel is held to the launch it was cut out of — the same set handed to rcot_block_param_reduce must give the same BITS — and to
an fp64 sum; the schedule is held to itself with the policy off: every gradient bit for bit, eagerly and from a launch plan.
Device tensors come from a GuardSet (tests/guarded.py); pad columns (ldws > N, ldd > N) hold NaN in the slabs and a marker in dst.
"""
import contextlib
import ctypes

import pytest
import torch

from conftest import seeded_tensor
from guarded import GuardSet, poison_workspaces

pytestmark = pytest.mark.gpu
EINVAL = -1
MARK = 7.0

# (M, N, S, ldws, ldd)
ONE_SET = [(33, 35, 3, 36, 35),         # S <= 8 (4096 outputs per workgroup), ragged last chunk
           (33, 35, 1, 36, 40),         # S = 1
           (96, 255, 9, 256, 255),      # per == 256, ldws > N, S no multiple of 4
           (510, 96, 64, 96, 96),       # per == 256, the unrolled 32-slab trips
           (512, 513, 9, 516, 520),     # >= 256 K outputs: the 1024 form, ragged tail, ldd > N
           # beyond the issue's list: the launch walks its chunks with at most 64 workgroups — cases 3 - 5 have 96 / 192 / 257 chunks of
           # the S > 8 forms; this one has 65 chunks of the S <= 8 form, so one workgroup takes a second, ragged chunk there too
           (512, 513, 3, 516, 520)]
TWO_SETS = (ONE_SET[0], ONE_SET[2])                             # two forms in one launch
FOUR_SETS = (ONE_SET[2], ONE_SET[1], ONE_SET[4], ONE_SET[3])    # every form, chunk0 walked over four sets


@pytest.fixture(scope="module")
def hip():
    from rcot_amd import lib
    from rcot_amd.ops import HipBackend
    be = HipBackend()
    be.prec = lib.PREC_FP32
    return be


@contextlib.contextmanager
def early(be, on):
    old = be._early_slabs_env
    be._early_slabs_env = "1" if on else "0"
    try:
        yield
    finally:
        be._early_slabs_env = old


def _rows(descs):
    return (ctypes.c_longlong * (7 * len(descs)))(*[v for d in descs for v in d])


def _close_args(be, gs):
    """the other arguments of the closing launch, as test_block_param_reduce_with_weight_gradient_slabs makes them: two slots of
    deferred LayerNorm partial rows, per-image dW_o and temperature parts"""
    B, C, N = 2, 48, 256
    t = lambda seed, *shape: gs.tensor(seeded_tensor(seed, shape))
    g1, x1, w, dx1 = t(1, B, C, N), t(2, B, C, N), gs.tensor(1 + 0.1 * seeded_tensor(5, (C,))), gs.tensor(torch.zeros(B, C, N))
    mu, rs = gs.tensor(torch.zeros(B, N)), gs.tensor(torch.ones(B, N))
    be.ln_stats(x1, mu, rs)
    be.ln_bwd(g1, x1, mu, rs, w, None, dx1, None, None, slot=0)
    be.ln_bwd(g1, x1, mu, rs, w, None, dx1, None, None, slot=1)
    return (C, t(6, C), t(7, C), t(8, C), t(9, C), t(10, B, C, C), t(11, C, C), t(12, B, 1), t(13, 1))


_RUNS = {}


def _run(be, cases):
    """both launches on the same sets, once per tuple of cases: [(ws host, dst0 host, dst of rcot_slab_sets_reduce, dst of
    rcot_block_param_reduce)] per set, the guard bands checked"""
    if cases in _RUNS:
        return _RUNS[cases]
    gs = GuardSet("cuda")
    poison_workspaces(be)
    host, new, old = [], [], []
    for i, (M, N, S, ldws, ldd) in enumerate(cases):
        ws = seeded_tensor(100 + i, (S, M, ldws))
        ws[:, :, N:] = float("nan")
        dst0 = seeded_tensor(200 + i, (M, ldd))
        dst0[:, N:] = MARK
        wd = gs.tensor(ws, f"slabs[{i}]")
        da, db = gs.tensor(dst0, f"dst new[{i}]"), gs.tensor(dst0, f"dst closing launch[{i}]")
        host.append((ws, dst0))
        new.append((wd.data_ptr(), S, M, N, ldws, da.data_ptr(), ldd))
        old.append((wd.data_ptr(), S, M, N, ldws, db.data_ptr(), ldd))
        host[-1] += (da, db)
    assert be.L.rcot_slab_sets_reduce(_rows(new), len(new), be._st()) == 0
    be.block_param_reduce(*_close_args(be, gs), old)
    torch.cuda.synchronize()
    gs.check()
    _RUNS[cases] = [(ws, dst0, da.cpu(), db.cpu()) for ws, dst0, da, db in host]
    return _RUNS[cases]


def _same_bits(res, cases):
    for (ws, dst0, da, db), (M, N, S, ldws, ldd) in zip(res, cases):
        assert torch.equal(da, db), (M, N, S)
        assert torch.equal(da[:, N:], dst0[:, N:])                     # pad columns of dst: not written
        assert not torch.equal(da[:, :N], dst0[:, :N])                 # (and something was added)


def _against_fp64(res, cases):
    for (ws, dst0, da, _), (M, N, S, ldws, ldd) in zip(res, cases):
        slabs = ws[:, :, :N].double()
        ref = dst0[:, :N].double() + slabs.sum(0)
        got = da[:, :N].double()
        bound = 2.0 ** -24 * (S * slabs.abs().sum(0) + got.abs())
        assert torch.isfinite(got).all()
        worst = float(((got - ref).abs() / bound).max())
        print(f"M={M} N={N} S={S}: largest error / bound = {worst:.3f}")
        assert bool(((got - ref).abs() <= bound).all()), (M, N, S, worst)


@pytest.mark.parametrize("case", ONE_SET)
def test_one_set_same_bits_as_the_closing_launch(hip, case):
    _same_bits(_run(hip, (case,)), (case,))


@pytest.mark.parametrize("case", ONE_SET)
def test_one_set_against_fp64(hip, case):
    _against_fp64(_run(hip, (case,)), (case,))


@pytest.mark.parametrize("cases", [TWO_SETS, FOUR_SETS], ids=["two", "four"])
def test_several_sets_in_one_launch(hip, cases):
    res = _run(hip, cases)
    _same_bits(res, cases)
    _against_fp64(res, cases)


def test_argument_checks(hip):
    """(nothing is launched by any of these)"""
    be = hip
    z = torch.zeros(64 * 64, device="cuda")
    good = (z.data_ptr(), 2, 8, 8, 8, z.data_ptr() + 4096, 8)
    call = lambda descs, n: be.L.rcot_slab_sets_reduce(_rows(descs) if descs else None, n, be._st())
    assert call([good], 0) == EINVAL
    assert call([good] * 5, 5) == EINVAL
    assert call([good[:4] + (7,) + good[5:]], 1) == EINVAL             # ldws < N
    assert call(None, 1) == EINVAL                                     # no rows at all
    assert call([(0,) + good[1:]], 1) == EINVAL                        # a row without slabs
    assert call([good[:5] + (0, 8)], 1) == EINVAL                      # a row without a destination
    assert call([good, (0,) + good[1:]], 2) == EINVAL                  # (the second row is checked too)
    torch.cuda.synchronize()
    assert float(z.abs().max()) == 0.0


# ----------------------------------------------------------------------------- the schedule
def _block(be, C, heads):
    from rcot_amd import params as P
    from rcot_amd.net_restormer import ParamStore, TransformerBlockOp
    shapes = P.block_param_shapes("blk", C, heads)
    st = ParamStore(be, shapes, [n for n, _ in shapes], [])
    st.load({k: torch.from_numpy(v) for k, v in P.seeded_params(shapes, 5, "T").items()})
    blk = TransformerBlockOp(be, st, "blk", C, heads)
    blk.repack()
    return blk, st


@contextlib.contextmanager
def _descriptors(be):
    """what conv1x1_wgrad_slabs returned inside"""
    seen, orig = [], be.conv1x1_wgrad_slabs

    def spy(*a, **kw):
        seen.append(orig(*a, **kw))
        return seen[-1]
    be.conv1x1_wgrad_slabs = spy
    try:
        yield seen
    finally:
        del be.conv1x1_wgrad_slabs


def _profiled(be, fn):
    buf = ctypes.create_string_buffer(1 << 16)
    be.L.rcot_profile_begin()
    out = fn()
    be.side_join()
    torch.cuda.synchronize()
    assert be.L.rcot_profile_end(buf, 1 << 16) > 10
    return out, buf.value.decode(errors="replace")


SHAPES = [(48, 1, 2, 32), (96, 2, 2, 16)]       # (C, heads, B, H = W): the smallest planes at which all three weight gradients leave slabs


@pytest.mark.parametrize("C,heads,B,HW", SHAPES)
def test_block_backward_same_bits_with_early_sums(hip, C, heads, B, HW):
    be = hip
    blk, st = _block(be, C, heads)
    x, gy = seeded_tensor(21, (B, C, HW, HW)).cuda(), seeded_tensor(22, (B, C, HW, HW)).cuda()
    res = {}
    for on in (False, True):
        with early(be, on), _descriptors(be) as seen:
            st.zero_grad()
            _, ctx = blk.forward(x, True)
            dx, ran = _profiled(be, lambda: blk.backward(ctx, gy))
        assert len(seen) == 3 and all(d is not None for d in seen), seen        # else the comparison below proves nothing
        assert ("slab_sets_reduce_kernel" in ran) == on
        res[on] = (dx.clone(), st.grad.clone())
    assert torch.equal(res[True][0], res[False][0])
    assert torch.equal(res[True][1], res[False][1])
    assert float(res[True][1].abs().max()) > 0


@pytest.mark.parametrize("C,heads,B,HW", SHAPES)
def test_block_backward_from_a_launch_plan(hip, C, heads, B, HW):
    """recorded with the policy off and on: one launch more, as many hand-overs, the close with one set; two replays of each give
    the bits of the eager pass"""
    from rcot_amd.plan import LaunchPlan
    be = hip
    blk, st = _block(be, C, heads)
    x, gy = seeded_tensor(21, (B, C, HW, HW)).cuda(), seeded_tensor(22, (B, C, HW, HW)).cuda()
    with early(be, False):
        st.zero_grad()
        _, ctx = blk.forward(x, True)
        want_dx = blk.backward(ctx, gy).clone()
        be.side_join()
        torch.cuda.synchronize()
        want_g = st.grad.clone()
    plans = {}
    for on in (False, True):
        box = {}
        with early(be, on):
            plans[on] = LaunchPlan(be).record(lambda: box.__setitem__("dx", blk.backward(ctx, gy)))
        for _ in range(2):
            st.zero_grad()
            plans[on].replay()
            torch.cuda.synchronize()
            assert torch.equal(box["dx"], want_dx)
            assert torch.equal(st.grad, want_g)
    off, on = plans[False], plans[True]
    assert on.n_launches == off.n_launches + 1
    hosts = lambda p: sum(1 for c in p.cmds if c[1] is None)
    assert hosts(on) == hosts(off)
    named = lambda p, name: [c for c in p.cmds if c[1] is not None and getattr(c[0], "__name__", "") == name]
    assert len(named(off, "rcot_slab_sets_reduce")) == 0 and len(named(on, "rcot_slab_sets_reduce")) == 1
    early_call, = named(on, "rcot_slab_sets_reduce")
    assert early_call[1][1] == 2 and early_call[2]                                  # two sets, on the side stream
    (close_off,), (close_on,) = named(off, "rcot_block_param_reduce"), named(on, "rcot_block_param_reduce")
    assert close_off[1][15] == 3 and close_on[1][15] == 1                           # n_sets of the closing launch
    for p in plans.values():
        p.release()


def test_tnet_gradients_same_bits_with_early_sums():
    from rcot_amd import lib
    from rcot_amd import params as P
    from rcot_amd.net_restormer import T_net
    net = T_net(decoder=True)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in P.seeded_params(P.tnet_param_shapes(), 11, "T").items()})
    be = net.store.be
    prec, be.prec = be.prec, lib.PREC_FP32
    x = seeded_tensor(31, (1, 3, 64, 64), lo=0.0, hi=1.0).cuda()
    r = seeded_tensor(32, (1, 3, 64, 64)).cuda()
    res = {}
    try:
        for on in (False, True):
            with early(be, on):
                net.zero_grad()
                net.forward(x, save=True)
                _, ran = _profiled(be, lambda: net.backward(r / r.numel()))
            assert ("slab_sets_reduce_kernel" in ran) == on
            res[on] = net.store.grad.clone()
    finally:
        be.prec = prec
    assert torch.equal(res[True], res[False])
    assert float(res[True].abs().max()) > 0


def test_no_early_launch_behind_the_paired_kernel():
    """bf16x3 at a shape where both products of a projection come from one launch on the main stream: the slabs are not the side
    stream's, nothing is summed early, the closing launch takes all three sets"""
    from rcot_amd import lib
    from rcot_amd.ops import HipBackend
    be = HipBackend()
    be.prec = lib.PREC_BF16X3
    C, heads, B, HW = 96, 2, 8, 32
    blk, st = _block(be, C, heads)
    x, gy = seeded_tensor(21, (B, C, HW, HW)).cuda(), seeded_tensor(22, (B, C, HW, HW)).cuda()
    with early(be, True):
        _, ctx = blk.forward(x, True)
        _, ran = _profiled(be, lambda: blk.backward(ctx, gy))
    assert "x3p_nt_pair_kernel" in ran, ran[:400]
    assert "slab_sets_reduce_kernel" not in ran
    assert "block_param_reduce_kernel" in ran
