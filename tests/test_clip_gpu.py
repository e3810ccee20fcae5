"""GPU tier: gradient-norm clipping and the non-finite step skip decided on the device — rcot_grad_sumsq / rcot_grad_decide and the guarded
step kernels (csrc/optim.hip) on guard-banded buffers against the host restatement (tests/clip_double.py), guarded optimizers through
eager and planned minimax iterations, and the trainer CLI.

Bars.  The device sums exact fp64 squares: its total is within n 2^-53 relative of the exact sum in any order, the restatement's too, and
the square root halves a relative error — 2^-26 for the norm is far above both.  The scale is one division and one minimum of such
values, compared at fp32 resolution (what the step kernels use of it): 1 fp32 ulp.  Updates: the 1e-5 of
tests/test_kernels_gpu.py::test_optimizers."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from clip_double import adam_guarded, decide, rmsprop_guarded, sumsq
from conftest import ROOT, relerr
from guarded import GuardSet
from rcot_amd import lib
from rcot_amd import params as P
from test_ema_gpu import _values

pytestmark = pytest.mark.gpu

EINVAL = -1
SWEEP4 = 4096 * 256 * 4          # elements of one full float4 sweep of the grid (at most 4096 workgroups of 256)
BIG = SWEEP4 + 4                 # 4 194 308: one float4 past it
NEW_ENTRY_POINTS = {"rcot_grad_sumsq", "rcot_grad_decide", "rcot_rmsprop_step_guarded", "rcot_adam_step_guarded"}


def _be():
    from rcot_amd.ops import default_backend
    return default_backend()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


class _Block:
    """a guarded control block and partials workspace; ``decide`` poisons the workspace before every call"""

    def __init__(self, gs, max_norm, lr=1e-3):
        self.ctrl = gs.full((lib.CB_WORDS,), 0.0, torch.float64, "ctrl")
        self.partials = gs.empty((lib.SUMSQ_MAX_PARTS,), torch.float64, "partials")
        self.ctrl[lib.CB_LR], self.ctrl[lib.CB_MAX_NORM] = lr, max_norm

    def decide(self, be, g, n, adam_mask=0, inherit=False):
        self.partials.fill_(float("nan"))
        parts = be.grad_sumsq(g, n, self.partials)
        be.grad_decide(self.partials, parts, self.ctrl, adam_mask, inherit=inherit)
        return parts

    def read(self):
        c = self.ctrl.cpu()
        i = c.view(torch.int64)
        return dict(norm=float(c[lib.CB_NORM]), scale=float(c[lib.CB_SCALE]), steps=int(i[lib.CB_STEPS]), clipped=int(i[lib.CB_CLIPPED]),
                    skipped=int(i[lib.CB_SKIPPED]), max_seen=float(c[lib.CB_MAX_SEEN]), skip=int(i[lib.CB_SKIP]), t=(int(i[lib.CB_T]), int(i[lib.CB_T + 1])))


def _check_decision(n, M, off=0, seed=0):
    be = _be()
    gs = GuardSet(be.device)
    g_host = _values(seed + 1, n + 3)
    g_buf = gs.tensor(torch.from_numpy(g_host), "g")
    blk = _Block(gs, M)
    parts = blk.decide(be, g_buf[off:off + n], n)
    gs.check()
    assert parts == min(4096, max(1, -(-(n // 4) // 256)))
    pt = blk.partials.cpu()
    assert bool(torch.isfinite(pt[:parts]).all()) and bool(torch.isnan(pt[parts:]).all())          # one store per workgroup, nothing else
    assert np.array_equal(g_buf.cpu().numpy().view(np.int32), g_host.view(np.int32))
    norm, scale, skip = decide(sumsq(g_host[off:off + n]), M)
    r = blk.read()
    print(f"n {n} off {off} M {M}: norm {r['norm']!r} vs {norm!r} (rel {abs(r['norm'] - norm) / norm:.2e}), scale {r['scale']!r} vs {scale!r}")
    assert not skip and r["skip"] == 0 and r["skipped"] == 0 and r["steps"] == 1
    assert abs(r["norm"] - norm) <= 2.0 ** -26 * norm
    assert abs(r["scale"] - scale) <= float(np.spacing(np.float32(scale)))
    assert r["clipped"] == int(scale < 1.0) and r["max_seen"] == r["norm"]
    return r


@pytest.mark.parametrize("M", [1e3, 1.0])
@pytest.mark.parametrize("n", [4, 5, 4004, 64000, BIG])
def test_norm_and_scale(n, M):
    """M = 1e3: scale exactly 1; M = 1: clipped from n = 4004 on (norm about 15); BIG runs the grid-stride second pass"""
    r = _check_decision(n, M, seed=n % 1000)
    if M == 1e3:
        assert r["scale"] == 1.0
    elif n >= 4004:
        assert r["scale"] < 0.1 and r["clipped"] == 1


@pytest.mark.parametrize("n", [5, 4004, BIG])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_norm_of_misaligned_views(k, n):
    """views 1, 2, 3 elements into the buffer: 3, 2, 1 head elements before the first 16-byte boundary, then float4 loads, then the tail"""
    _check_decision(n, 1.0, off=k, seed=10 * k + n % 7)


def test_all_zero_gradients_give_scale_one():
    be = _be()
    gs = GuardSet(be.device)
    for n in (5, 4004):
        blk = _Block(gs, 1.0)
        blk.decide(be, gs.full(n, 0.0, name="g"), n)
        gs.check()
        r = blk.read()
        assert r["norm"] == 0.0 and r["scale"] == 1.0 and r["skip"] == 0 and r["skipped"] == 0 and r["clipped"] == 0 and r["steps"] == 1


def _opt_buffers(gs, n, seed, adam):
    p = gs.tensor(torch.from_numpy(_values(seed, n)), "p")
    g = gs.tensor(torch.from_numpy(_values(seed + 1, n)), "g")
    state = [gs.full(n, 0.0, name=s) for s in (("m", "v") if adam else ("sq",))]
    return p, g, state


@pytest.mark.parametrize("n", [4, 4004, 64000, BIG])
def test_guarded_rmsprop_without_a_cap_is_the_plain_step_bit_for_bit(n):
    be = _be()
    gs = GuardSet(be.device)
    p1, g, (sq1,) = _opt_buffers(gs, n, 3, False)
    p2, sq2 = gs.tensor(p1.cpu(), "p2"), gs.full(n, 0.0, name="sq2")
    blk = _Block(gs, math.inf, lr=1e-3)
    for _ in range(3):
        blk.decide(be, g, n)
        be.rmsprop_step_guarded(p1, g, sq1, n, blk.ctrl)
        be.rmsprop_step(p2, g, sq2, n, 1e-3, grad_scale=1.0)
    gs.check()
    r = blk.read()
    assert r["scale"] == 1.0 and r["steps"] == 3 and r["clipped"] == 0 and r["skipped"] == 0
    assert _same_bits(p1, p2) and _same_bits(sq1, sq2)
    assert not _same_bits(p1, torch.from_numpy(_values(3, n)).to(p1.device))


@pytest.mark.parametrize("n", [4, 4004, 64000, BIG])
def test_guarded_adam_without_a_cap_is_the_plain_step(n):
    """the step counts and 1 - beta^t come from the device here (its pow may differ from the host's in the last bit): the 1e-5 bar"""
    be = _be()
    gs = GuardSet(be.device)
    p1, g, (m1, v1) = _opt_buffers(gs, n, 5, True)
    p2, m2, v2 = gs.tensor(p1.cpu(), "p2"), gs.full(n, 0.0, name="m2"), gs.full(n, 0.0, name="v2")
    blk = _Block(gs, math.inf, lr=1e-3)
    for t in range(1, 4):
        blk.decide(be, g, n, adam_mask=1)
        be.adam_step_guarded(p1, g, m1, v1, n, blk.ctrl, 0)
        be.adam_step(p2, g, m2, v2, n, 1e-3, t)
    gs.check()
    assert blk.read()["t"] == (3, 0)
    for a, b in ((p1, p2), (m1, m2), (v1, v2)):
        assert relerr(a, b) < 1e-5
    be.adam_step_guarded(p1, g, m1, v1, n, blk.ctrl, 1)                    # counter 1 was never advanced: the launch does nothing
    assert relerr(p1, p2) < 1e-5


@pytest.mark.parametrize("kind", ["RMSprop", "Adam"])
@pytest.mark.parametrize("n", [4004, 64000])
def test_clipped_steps_match_the_restatement_with_the_kernels_own_scale(n, kind):
    be = _be()
    gs = GuardSet(be.device)
    adam = kind == "Adam"
    p, g, state = _opt_buffers(gs, n, 9, adam)
    hp, hg = p.cpu().clone(), g.cpu().clone()
    hstate = [torch.zeros(n) for _ in state]
    blk = _Block(gs, 1.0, lr=1e-3)
    for t in range(1, 4):
        blk.decide(be, g, n, adam_mask=int(adam))
        scale = blk.read()["scale"]
        assert scale < 0.1
        if adam:
            be.adam_step_guarded(p, g, *state, n, blk.ctrl, 0)
            adam_guarded(hp, hg, *hstate, 1e-3, t, 1.0, scale=scale)
        else:
            be.rmsprop_step_guarded(p, g, *state, n, blk.ctrl)
            rmsprop_guarded(hp, hg, *hstate, 1e-3, 1.0, scale=scale)
    gs.check()
    assert blk.read()["clipped"] == 3
    for a, b in zip([p] + state, [hp] + hstate):
        assert relerr(a, b) < 1e-5


@pytest.mark.parametrize("kind", ["RMSprop", "Adam"])
@pytest.mark.parametrize("n,where,bad", [(4004, 4003, float("nan")), (4004, 0, float("inf")), (5, 4, float("nan")), (BIG, SWEEP4 + 1, -float("inf"))],
                         ids=["nan_last", "inf_first", "nan_tail_element", "neg_inf_second_pass"])
def test_a_non_finite_gradient_skips_the_step(n, where, bad, kind):
    """nothing moves, the step is counted as skipped, Adam's count stays, and the next finite step is the one a run that never saw the
    bad gradient takes, bit for bit"""
    be = _be()
    gs = GuardSet(be.device)
    adam = kind == "Adam"
    n_step = n // 4 * 4                                                    # the step kernels take multiples of 4; the norm any n
    p, g, state = _opt_buffers(gs, n, 13, adam)
    p_b = gs.tensor(p.cpu(), "p_b")                                        # run B never sees the bad gradient
    state_b = [gs.full(n, 0.0, name="b") for _ in state]
    blk, blk_b = _Block(gs, 1.0), _Block(gs, 1.0)

    def step(bk, pp, ss):
        bk.decide(be, g, n, adam_mask=int(adam))
        if adam:
            be.adam_step_guarded(pp, g, *ss, n_step, bk.ctrl, 0)
        else:
            be.rmsprop_step_guarded(pp, g, *ss, n_step, bk.ctrl)
    step(blk, p, state)                                                    # one finite step on both
    step(blk_b, p_b, state_b)
    keep = [t.clone() for t in [p] + state]
    good = float(g[where])
    g[where] = bad
    step(blk, p, state)
    gs.check()
    r = blk.read()
    assert r["skip"] == 1 and r["skipped"] == 1 and r["steps"] == 2 and r["scale"] == 0.0 and not math.isfinite(r["norm"])
    assert r["t"] == ((1, 0) if adam else (0, 0))
    assert all(_same_bits(a, b) for a, b in zip([p] + state, keep))
    assert math.isfinite(r["max_seen"])
    g[where] = good
    step(blk, p, state)
    step(blk_b, p_b, state_b)
    gs.check()
    r, rb = blk.read(), blk_b.read()
    assert r["skip"] == 0 and r["steps"] == 3 and rb["steps"] == 2 and r["skipped"] == 1 and r["t"] == rb["t"] == ((2, 0) if adam else (0, 0))
    assert all(_same_bits(a, b) for a, b in zip([p] + state, [p_b] + state_b))
    assert not _same_bits(p, keep[0])


@pytest.mark.parametrize("kind", ["RMSprop", "Adam"])
def test_a_step_on_the_same_batch_inherits_the_skip(kind):
    """RCOT_DECIDE_INHERIT: a decision that follows a skipped one on the same block skips too, though its own gradients are finite (the
    gradient-penalty step after a critic step that met a NaN); after a taken decision, and without the flag, it decides on its own sum"""
    be = _be()
    gs = GuardSet(be.device)
    adam = kind == "Adam"
    n = 4004
    p, g, state = _opt_buffers(gs, n, 21, adam)
    bad = gs.tensor(g.cpu(), "g_bad")
    bad[n - 1] = float("nan")
    blk = _Block(gs, 1.0)

    def step(grad, inherit):
        blk.decide(be, grad, n, adam_mask=int(adam), inherit=inherit)
        if adam:
            be.adam_step_guarded(p, grad, *state, n, blk.ctrl, 0)
        else:
            be.rmsprop_step_guarded(p, grad, *state, n, blk.ctrl)
        gs.check()
        return blk.read()
    want_norm = math.sqrt(sumsq(g.cpu().numpy()))
    keep = [t.clone() for t in [p] + state]
    r = step(bad, False)
    assert r["skip"] == 1 and r["skipped"] == 1
    r = step(g, True)                                                      # finite gradients, the same batch: skipped with it
    assert r["skip"] == 1 and r["skipped"] == 2 and r["steps"] == 2 and r["scale"] == 0.0 and r["clipped"] == 0 and r["t"] == (0, 0)
    assert abs(r["norm"] - want_norm) <= 2.0 ** -26 * want_norm and r["max_seen"] == 0.0
    assert all(_same_bits(a, b) for a, b in zip([p] + state, keep))
    r = step(g, False)                                                     # the next batch's first step decides afresh
    assert r["skip"] == 0 and r["skipped"] == 2 and r["steps"] == 3 and r["t"] == ((1, 0) if adam else (0, 0)) and not _same_bits(p, keep[0])
    after = p.clone()
    r = step(g, True)                                                      # nothing to inherit from a taken step
    assert r["skip"] == 0 and r["skipped"] == 2 and r["steps"] == 4 and r["clipped"] == 2 and not _same_bits(p, after)
    r = step(bad, True)                                                    # and its own sum still counts
    assert r["skip"] == 1 and r["skipped"] == 3


def test_refusals_launch_nothing():
    be = _be()
    gs = GuardSet(be.device)
    n = 64
    p, g, (m, v) = _opt_buffers(gs, n, 17, True)
    blk = _Block(gs, 1.0)
    blk.partials.fill_(float("nan"))
    c0, p0, state0 = blk.ctrl.clone(), p.clone(), (g.clone(), m.clone(), v.clone())
    L, st = be.L, be._st()
    P_, G, M_, V, C, W = (t.data_ptr() for t in (p, g, m, v, blk.ctrl, blk.partials))
    cases = [L.rcot_grad_sumsq(0, n, W, st), L.rcot_grad_sumsq(G, 0, W, st), L.rcot_grad_sumsq(G, n, 0, st), L.rcot_grad_sumsq(G + 2, n - 1, W, st),
             L.rcot_grad_sumsq(G, n, W + 4, st), L.rcot_grad_decide(0, 1, C, 0, 0.9, 0.999, st), L.rcot_grad_decide(W, 0, C, 0, 0.9, 0.999, st),
             L.rcot_grad_decide(W, 4097, C, 0, 0.9, 0.999, st), L.rcot_grad_decide(W, 1, 0, 0, 0.9, 0.999, st), L.rcot_grad_decide(W, 1, C, 8, 0.9, 0.999, st),
             L.rcot_rmsprop_step_guarded(0, G, M_, n, 0.99, 1e-8, C, st), L.rcot_rmsprop_step_guarded(P_, G, M_, n - 1, 0.99, 1e-8, C, st),
             L.rcot_rmsprop_step_guarded(P_, G, M_, 0, 0.99, 1e-8, C, st), L.rcot_rmsprop_step_guarded(P_ + 4, G, M_, n - 4, 0.99, 1e-8, C, st),
             L.rcot_rmsprop_step_guarded(P_, G, M_, n, 0.99, 1e-8, 0, st), L.rcot_adam_step_guarded(P_, G, M_, V, n, 0.9, 0.999, 1e-8, C, 2, st),
             L.rcot_adam_step_guarded(P_, G, M_, V, n, 0.9, 0.999, 1e-8, C, -1, st), L.rcot_adam_step_guarded(P_, G, M_, 0, n, 0.9, 0.999, 1e-8, C, 0, st),
             L.rcot_adam_step_guarded(P_, G, M_, V, n + 2, 0.9, 0.999, 1e-8, C, 0, st), L.rcot_adam_step_guarded(P_, G + 8, M_, V, n - 4, 0.9, 0.999, 1e-8, C, 0, st)]
    # the two plain steps refuse alike: a null pointer, n = 0, n = 6 (no multiple of 4), a pointer 4 bytes off, and for Adam step = 0
    rms = lambda p_=P_, g_=G, s_=M_, n_=n: L.rcot_rmsprop_step(p_, g_, s_, n_, 1e-3, 0.99, 1e-8, 1.0, st)
    adam = lambda p_=P_, g_=G, m_=M_, v_=V, n_=n, t=1: L.rcot_adam_step(p_, g_, m_, v_, n_, 1e-3, 0.9, 0.999, 1e-8, t, 1.0, st)
    cases += [rms(p_=0), rms(g_=0), rms(s_=0), rms(n_=0), rms(n_=6), rms(p_=P_ + 4, n_=n - 4), rms(g_=G + 4, n_=n - 4), rms(s_=M_ + 4, n_=n - 4),
              adam(p_=0), adam(g_=0), adam(m_=0), adam(v_=0), adam(n_=0), adam(n_=6), adam(p_=P_ + 4, n_=n - 4), adam(g_=G + 4, n_=n - 4),
              adam(m_=M_ + 4, n_=n - 4), adam(v_=V + 4, n_=n - 4), adam(t=0)]
    assert cases == [EINVAL] * len(cases), cases
    gs.check()
    assert _same_bits(blk.ctrl, c0) and _same_bits(p, p0) and bool(torch.isnan(blk.partials).all())
    assert all(_same_bits(a, b) for a, b in zip((g, m, v), state0))
    assert L.rcot_grad_sumsq_parts(0) == 0 and L.rcot_grad_sumsq_parts(3) == 1 and L.rcot_grad_sumsq_parts(BIG) == 4096


# ------------------------------------------------------------------------------- guarded optimizers through the iteration
def _stepper(plan, M_T=None, M_F=None, kind="RMSprop", ps=64):
    """the set-up of tests/test_plan_gpu.py::_run: seeded parameters, ps = 64, lr 1e-4, de ids [2, 3]"""
    from rcot_amd.net_restormer import F_net, T_net
    from rcot_amd.trainer import FlatOptimizer, MinimaxStep
    os.environ["RCOT_PLAN"] = "1" if plan else "0"
    try:
        lr = 1e-4
        Tn, Fn = T_net(decoder=True), F_net(patch_size=ps)
        Tn.load_state_dict({k: torch.from_numpy(v) for k, v in P.seeded_params(P.tnet_param_shapes(), 31, "T").items()})
        Fn.load_state_dict({k: torch.from_numpy(v) for k, v in P.seeded_params(P.fnet_param_shapes(ps), 32, "F").items()})
        st = MinimaxStep(Tn, Fn, FlatOptimizer(Tn, kind, lr / 2, M_T), FlatOptimizer(Fn, kind, lr, M_F), 1.0, 10000.0)
    finally:
        os.environ.pop("RCOT_PLAN", None)
    st.set_de_ids([2, 3])
    assert (st.planned is not None and st.planned.enabled) == plan
    return st


def _batch(i, ps=64, B=2):
    from rcot_amd.synth import make_batch
    de = [2, 3]
    _, x, y = make_batch(300 + i, B, ps, de)
    alpha = torch.rand(B, generator=torch.Generator().manual_seed(i))
    return x.cuda(), y.cuda(), torch.tensor(de, dtype=torch.int32).cuda(), alpha.cuda()


def _iterate(st, i, paired=False, target_edit=None):
    x, y, d, a = _batch(i)
    if target_edit is not None:
        target_edit(y)
    st.run(x, y, d, a, paired)
    torch.cuda.synchronize()


def _recorded_names(st):
    return [{getattr(fn, "__name__", "") for fn, a, _ in e["plan"].cmds if a is not None} for e in st.planned.cache.values()]


def test_guarded_minimax_eager_and_planned_agree_and_the_rate_travels_through_the_block():
    M = 1e-3                                                               # far below every gradient norm here: every step is clipped
    runs = {}
    for plan in (False, True):
        st = _stepper(plan, M, M)
        T0, F0 = st.T.store.flat.clone(), st.F.store.flat.clone()
        for i in range(3):
            _iterate(st, i)
        runs[plan] = (st, st.T.store.flat.clone(), st.F.store.flat.clone())
        cT, cF = st.To.guard_counters(), st.Fo.guard_counters()
        print(f"plan {plan}: T {cT}\n  F {cF}")
        # three and six: the warm-up pass before the recording left nothing behind
        assert (cT["steps"], cT["clipped"], cT["skipped"]) == (3, 3, 0) and (cF["steps"], cF["clipped"], cF["skipped"]) == (6, 6, 0)
        assert cT["max_seen"] > M and cF["max_seen"] > M
    (_, Te, Fe), (stp, Tp, Fp) = runs[False], runs[True]
    assert float((Tp - Te).norm() / (Te - T0).norm()) < 5e-2               # the bars of tests/test_plan_gpu.py
    assert float((Fp - Fe).norm() / (Fe - F0).norm()) < 5e-2
    assert float((Te - T0).norm()) > 0 and float((Fe - F0).norm()) > 0
    assert bool(torch.isfinite(Tp).all()) and bool(torch.isfinite(Fp).all())
    (names,) = _recorded_names(stp)                                        # one plan: one recording, two replays
    assert {"rcot_grad_sumsq", "rcot_grad_decide", "rcot_rmsprop_step_guarded"} <= names and "rcot_rmsprop_step" not in names
    # the learning rate reaches recorded launches through the block: rate 0 freezes the parameters while the state moves
    for o in (stp.To, stp.Fo):
        o.param_groups[0]["lr"] = 0.0
    sqT, sqF = stp.To.sq.clone(), stp.Fo.sq.clone()
    _iterate(stp, 3)
    assert stp.planned.recordings == 1
    assert _same_bits(stp.T.store.flat, Tp) and _same_bits(stp.F.store.flat, Fp)
    assert not _same_bits(stp.To.sq, sqT) and not _same_bits(stp.Fo.sq, sqF)
    assert stp.To.guard_counters()["steps"] == 4 and stp.Fo.guard_counters()["steps"] == 8


def test_default_flags_record_no_new_entry_point():
    st = _stepper(True)
    assert st.To.ctrl is None and st.Fo.ctrl is None
    for i in range(2):
        _iterate(st, i)
    (names,) = _recorded_names(st)
    assert not (names & NEW_ENTRY_POINTS) and "rcot_rmsprop_step" in names


def _nan_pixel(y):
    y[1, 2, 5, 7] = float("nan")


def test_a_nan_pixel_in_the_target_skips_both_steps_of_the_potential():
    """One planned run with both networks guarded (max_norm inf): a clean recording, a replay whose target has one NaN pixel, a clean
    replay.  The critic step's gradients are not finite (its weight gradients multiply the NaN activations: 14 755 456 non-finite
    elements of 14 760 192, measured) and it is skipped on its own sum.  The gradient-penalty step's own gradients ARE finite (0 of
    14 760 128: the potential is piecewise linear, so they are products of weights and LeakyReLU masks, and a NaN input only picks mask
    branches): it is skipped because it follows a skipped step on the same batch (FlatOptimizer.step(same_batch=True),
    RCOT_DECIDE_INHERIT).  So both steps are skipped and the potential keeps its bits; without the guard the same input leaves NaN."""
    st = _stepper(True, math.inf, math.inf)
    _iterate(st, 0)                                                        # the recording, on a clean batch
    F1, T1, sq1 = st.F.store.flat.clone(), st.T.store.flat.clone(), st.Fo.sq.clone()
    _iterate(st, 1, target_edit=_nan_pixel)                                # a replay: unpaired, so the target reaches the potential only
    cF, cT = st.Fo.guard_counters(), st.To.guard_counters()
    print(f"NaN pixel in the target: F_net {cF}; T_net {cT}")
    assert cF["skipped"] == 2 and cF["steps"] == 4 and _same_bits(st.F.store.flat, F1) and _same_bits(st.Fo.sq, sq1)
    assert math.isfinite(cF["last_norm"]) and cF["last_scale"] == 0.0       # the penalty step: a finite norm of its own, skipped all the same
    assert cT["skipped"] == 0 and cT["steps"] == 2
    assert not _same_bits(st.T.store.flat, T1) and bool(torch.isfinite(st.T.store.flat).all())
    _iterate(st, 2)                                                        # and the run goes on: the next critic step decides afresh
    cF = st.Fo.guard_counters()
    assert cF["skipped"] == 2 and cF["steps"] == 6
    assert not _same_bits(st.F.store.flat, F1) and bool(torch.isfinite(st.F.store.flat).all())
    # what the guard prevents: the same input without it
    st0 = _stepper(True)
    _iterate(st0, 0)
    _iterate(st0, 1, target_edit=_nan_pixel)
    assert not bool(torch.isfinite(st0.F.store.flat).all())


def test_a_nan_in_the_transport_maps_gradient_skips_its_step():
    st = _stepper(True, 1.0, None)
    _iterate(st, 0)
    T1, sq1, F1 = st.T.store.flat.clone(), st.To.sq.clone(), st.F.store.flat.clone()

    def probe(tag):
        if tag == "T_gen":
            st.T.store.grad[12345] = float("nan")
    st.grad_probe = probe                                                  # (an iteration with a probe walks the schedule)
    _iterate(st, 1)
    st.grad_probe = None
    c = st.To.guard_counters()
    assert c["skipped"] == 1 and c["steps"] == 2 and _same_bits(st.T.store.flat, T1) and _same_bits(st.To.sq, sq1)
    assert not _same_bits(st.F.store.flat, F1)                             # the potential, unguarded and unharmed, took its steps
    _iterate(st, 2)
    c = st.To.guard_counters()
    assert c["skipped"] == 1 and c["steps"] == 3
    assert not _same_bits(st.T.store.flat, T1) and bool(torch.isfinite(st.T.store.flat).all())


def test_guarded_adam_iteration_counts_on_the_device():
    """Adam stays out of plans: two eager iterations, the potential's counts 4 (main) and 2 (fc2.bias, not part of the penalty step)"""
    st = _stepper(False, math.inf, math.inf, kind="Adam")
    F0 = st.F.store.flat.clone()
    for i in range(2):
        _iterate(st, i)
    sdT, sdF = st.To.state_dict(), st.Fo.state_dict()
    assert (sdT["t_main"], sdT["t_tail"]) == (2, 0) and (sdF["t_main"], sdF["t_tail"]) == (4, 2)
    assert sdF["guard"]["steps"] == 4 and sdF["guard"]["skipped"] == 0
    assert bool(torch.isfinite(st.F.store.flat).all()) and not _same_bits(st.F.store.flat, F0)


# ------------------------------------------------------------------------------- the trainer CLI (subprocesses in a temporary directory)
def _py(args, cwd):
    r = subprocess.run([sys.executable, "-m"] + args, capture_output=True, text=True, timeout=900, cwd=cwd, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def test_trainer_cli_reports_saves_and_resumes_the_counters(tmp_path):
    from rcot_amd.compat import load_checkpoint
    from synth_folders import write_png
    tmp = str(tmp_path)
    g = np.random.Generator(np.random.PCG64(3))
    t = np.clip(128 + 60 * np.sin(np.linspace(0, 4, 32))[:, None, None] + g.normal(0, 4, (32, 32, 3)), 0, 255).astype(np.uint8)
    write_png(f"{tmp}/val/target/0.png", t)
    write_png(f"{tmp}/val/input/0.png", np.clip(t + g.normal(0, 15, t.shape), 0, 255).astype(np.uint8))
    base = ["rcot_amd.trainer", "--synthetic", "--iters", "3", "--batchSize", "2", "--patch_size", "64", "--de_type", "denoise_15", "--seed", "5",
            "--type", "ClipTest", "--sigma", "1", "--degset", f"{tmp}/val/input/", "--tarset", f"{tmp}/val/target/",
            "--clip_grad_norm", "0.01", "--clip_grad_norm_F", "inf"]
    r1 = _py(base + ["--nEpochs", "1"], tmp)
    lines = [ln for ln in r1.stdout.splitlines() if ln.startswith("clip ")]
    assert len(lines) == 2, r1.stdout[-2000:]
    assert lines[0].startswith("clip T_net: max_norm 0.01, steps 3, clipped 3, skipped 0,") and "(run so far: 3 steps, 0 skipped)" in lines[0]
    assert lines[1].startswith("clip F_net: max_norm inf, steps 6, clipped 0, skipped 0,") and "(run so far: 6 steps, 0 skipped)" in lines[1]
    ck1_path = os.path.join(tmp, "checkpoint", "model_ClipTest__1_1.0.pth")
    ck1 = load_checkpoint(ck1_path)
    gT, gF = ck1["T_optimizer"]["guard"], ck1["F_optimizer"]["guard"]
    assert (gT["max_norm"], gT["steps"], gT["clipped"], gT["skipped"]) == (0.01, 3, 3, 0) and gT["max_seen"] > 0.01
    assert (gF["max_norm"], gF["steps"], gF["clipped"], gF["skipped"]) == (math.inf, 6, 0, 0) and math.isfinite(gF["max_seen"])
    val = open(os.path.join(tmp, "checksample", "ClipTest", "validation_results.txt")).read().splitlines()
    assert len(val) == 1 and val[0].startswith("Patchsize 64 Epoch 1, psnr ") and val[0].endswith(", Batchsize 2")      # the format is untouched
    r2 = _py(base + ["--nEpochs", "2", "--resume", ck1_path], tmp)
    lines = [ln for ln in r2.stdout.splitlines() if ln.startswith("clip ")]
    assert len(lines) == 2 and "steps 3," in lines[0] and "(run so far: 6 steps, 0 skipped)" in lines[0] and "(run so far: 12 steps, 0 skipped)" in lines[1]
    ck2 = load_checkpoint(os.path.join(tmp, "checkpoint", "model_ClipTest__2_1.0.pth"))
    assert ck2["T_optimizer"]["guard"]["steps"] == 6 and ck2["F_optimizer"]["guard"]["steps"] == 12 and ck2["epoch"] == 2
    assert ck2["T_optimizer"]["guard"]["max_seen"] >= gT["max_seen"]
