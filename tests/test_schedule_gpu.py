"""GPU tier: per-iteration schedules held on the device — rcot_sched_advance, rcot_ema_step_dev, rcot_adamw_step and
rcot_adamw_step_guarded (csrc/optim.hip) on guard-banded buffers against their by-value twins and the host restatement
(tests/schedule_double.py), a scheduled minimax iteration eager and through the launch plans, and the trainer CLI.

Bars.  The advance launch multiplies one table entry by one factor in double: correctly rounded on both sides, compared bit for bit.
ema_omd is one division and one subtraction in double, used at float resolution: 1 fp32 ulp of (float)omd, and exactly 1 - D once
(1 + u) / (10 + u) >= D.  rcot_ema_step_dev against rcot_ema_step with the word 1 - decay: the same kernel body and the same fp32 omd,
bit for bit.  AdamW with weight_decay 0 against Adam: bit for bit (Adam's own launch).  AdamW with decay against the fp64 restatement
over 3 steps: the 1e-5 of tests/test_kernels_gpu.py::test_optimizers."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, relerr
from guarded import GuardSet
from rcot_amd import lib, schedule
from rcot_amd import params as P
from schedule_double import ScheduleBackend, ema_omd
from test_ema_gpu import _values

pytestmark = pytest.mark.gpu

EINVAL = -1
SWEEP4 = 4096 * 256 * 4
BIG = SWEEP4 + 4                 # 4 194 308: one float4 past a full sweep of the grid
NEW_ENTRY_POINTS = {"rcot_sched_advance", "rcot_ema_step_dev", "rcot_adamw_step", "rcot_adamw_step_guarded"}


def _be():
    from rcot_amd.ops import default_backend
    return default_backend()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _f64_bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


def _ctrl_pair(gs):
    """two control blocks with recognisable words everywhere"""
    out = []
    for k in range(2):
        host = torch.arange(lib.CB_WORDS, dtype=torch.float64) * 0.25 + 100.0 * (k + 1)
        out.append((gs.tensor(host, f"ctrl{k}"), host))
    return out


# ------------------------------------------------------------------------------- rcot_sched_advance
@pytest.mark.parametrize("n", [1, 2, 7])
def test_advance_hands_out_the_table_and_holds_its_last_entry(n):
    be = _be()
    gs = GuardSet(be.device)
    tb = (1e-4 * np.random.Generator(np.random.PCG64(n)).uniform(0.01, 1.0, n)).astype(np.float64)
    table = gs.tensor(torch.from_numpy(tb), "table")
    block = gs.full((lib.SB_WORDS,), 0.0, torch.float64, "sched")
    (c0, h0), (c1, h1) = _ctrl_pair(gs)
    m0, m1 = 0.5, 0.3                                                      # 0.3: a product that does round
    for k in range(n + 3):
        be.sched_advance(block, table, c0[lib.CB_LR:lib.CB_LR + 1], m0, c1[lib.CB_LR:lib.CB_LR + 1], m1)
        gs.check()
        v = tb[min(k, n - 1)]
        b = block.cpu()
        assert int(b.view(torch.int64)[lib.SB_T]) == k + 1
        assert _f64_bits(b[lib.SB_LR].item()) == _f64_bits(v)
        g0, g1 = c0.cpu(), c1.cpu()
        assert _f64_bits(g0[lib.CB_LR].item()) == _f64_bits(v * m0) and _f64_bits(g1[lib.CB_LR].item()) == _f64_bits(v * m1)
        for got, host in ((g0, h0), (g1, h1)):                             # the other words of the control blocks
            assert torch.equal(got[1:].view(torch.int64), host[1:].view(torch.int64))
        assert torch.equal(b.view(torch.int64)[2:], torch.zeros(lib.SB_WORDS - 2, dtype=torch.int64))      # no EMA word without a decay
        assert np.array_equal(_f64_bits(table.cpu().numpy()), _f64_bits(tb))


def test_advance_null_table_maintains_the_ema_words_only():
    be = _be()
    gs = GuardSet(be.device)
    (c0, h0), _ = _ctrl_pair(gs)
    for D, u0, steps in ((0.5, 0, 12), (0.999, 8985, 10)):
        host = torch.zeros(lib.SB_WORDS, dtype=torch.float64)
        host[lib.SB_EMA_DECAY], host[lib.SB_LR] = D, 0.125
        host.view(torch.int64)[lib.SB_T], host.view(torch.int64)[lib.SB_EMA_UPDATES] = 17, u0
        block = gs.tensor(host, "sched")
        reached = False
        for k in range(steps):
            be.sched_advance(block, None, c0[lib.CB_LR:lib.CB_LR + 1], 0.5, None, 1.0)       # a destination without a table: not written
            gs.check()
            b = block.cpu()
            i = b.view(torch.int64)
            u = u0 + k
            assert int(i[lib.SB_T]) == 17 and float(b[lib.SB_LR]) == 0.125 and float(b[lib.SB_EMA_DECAY]) == D and int(i[lib.SB_EMA_UPDATES]) == u + 1
            assert torch.equal(i[5:], torch.zeros(3, dtype=torch.int64))
            want, got = ema_omd(D, u), float(b[lib.SB_EMA_OMD])
            assert abs(got - want) <= float(np.spacing(np.float32(want))), (u, got, want)
            if (1.0 + u) / (10.0 + u) >= D:
                assert got == 1.0 - D
                reached = True
            else:
                assert got > 1.0 - D
        assert reached
        assert torch.equal(c0.cpu().view(torch.int64), h0.view(torch.int64))


def test_advance_skips_a_null_destination_and_runs_both_halves_together():
    be = _be()
    gs = GuardSet(be.device)
    tb = np.array([3e-4, 1e-4], dtype=np.float64)
    table = gs.tensor(torch.from_numpy(tb), "table")
    host = torch.zeros(lib.SB_WORDS, dtype=torch.float64)
    host[lib.SB_EMA_DECAY] = 0.9
    block = gs.tensor(host, "sched")
    (c0, h0), (c1, h1) = _ctrl_pair(gs)
    be.sched_advance(block, table, None, 0.5, c1[lib.CB_LR:lib.CB_LR + 1], 1.0)
    be.sched_advance(block, table, c0[lib.CB_LR:lib.CB_LR + 1], 0.5, None, 1.0)
    be.sched_advance(block, table)
    gs.check()
    assert float(c1[lib.CB_LR]) == 3e-4 and float(c0[lib.CB_LR]) == 0.5e-4
    assert torch.equal(c0.cpu()[1:], h0[1:]) and torch.equal(c1.cpu()[1:], h1[1:])
    b = block.cpu()
    assert int(b.view(torch.int64)[lib.SB_T]) == 3 and float(b[lib.SB_LR]) == 1e-4
    assert int(b.view(torch.int64)[lib.SB_EMA_UPDATES]) == 3 and float(b[lib.SB_EMA_OMD]) == ema_omd(0.9, 2)


def test_advance_refusals_launch_nothing():
    be = _be()
    gs = GuardSet(be.device)
    table = gs.tensor(torch.tensor([1e-4, 2e-4], dtype=torch.float64), "table")
    host = torch.zeros(lib.SB_WORDS, dtype=torch.float64)
    host[lib.SB_EMA_DECAY] = 0.9
    block = gs.tensor(host, "sched")
    (c0, h0), _ = _ctrl_pair(gs)
    L, st = be.L, be._st()
    S, T, C = block.data_ptr(), table.data_ptr(), c0.data_ptr()
    cases = [L.rcot_sched_advance(0, T, 2, C, 0.5, 0, 1.0, st), L.rcot_sched_advance(S + 4, T, 2, C, 0.5, 0, 1.0, st),
             L.rcot_sched_advance(S, T, 0, C, 0.5, 0, 1.0, st), L.rcot_sched_advance(S, T, -3, C, 0.5, 0, 1.0, st),
             L.rcot_sched_advance(S, T + 4, 1, C, 0.5, 0, 1.0, st), L.rcot_sched_advance(S, T, 2, C + 4, 0.5, 0, 1.0, st),
             L.rcot_sched_advance(S, T, 2, 0, 0.5, C + 2, 1.0, st)]
    assert cases == [EINVAL] * len(cases), cases
    gs.check()
    assert torch.equal(block.cpu().view(torch.int64), host.view(torch.int64)) and torch.equal(c0.cpu().view(torch.int64), h0.view(torch.int64))
    with pytest.raises(lib.RcotKernelError):
        be.sched_advance(block.float(), table)


# ------------------------------------------------------------------------------- rcot_ema_step_dev
def _ema_pair(n, decay, off=0, seed=0):
    be = _be()
    gs = GuardSet(be.device)
    e_host, p_host = _values(2 * seed + 1, n + 3), _values(2 * seed + 2, n + 3)
    e1, e2 = gs.tensor(torch.from_numpy(e_host), "ema_dev"), gs.tensor(torch.from_numpy(e_host), "ema_val")
    p = gs.tensor(torch.from_numpy(p_host), "p")
    word = gs.tensor(torch.tensor([1.0 - decay], dtype=torch.float64), "omd")
    be.ema_step_dev(e1[off:off + n], p[off:off + n], n, word)
    be.ema_step(e2[off:off + n], p[off:off + n], n, decay)
    gs.check()
    assert _same_bits(e1, e2)
    outside = np.ones(n + 3, dtype=bool)
    outside[off:off + n] = False
    got = e1.cpu().numpy()
    assert np.array_equal(got[outside].view(np.int32), e_host[outside].view(np.int32))
    assert not np.array_equal(got[~outside].view(np.int32), e_host[~outside].view(np.int32))
    assert np.array_equal(p.cpu().numpy().view(np.int32), p_host.view(np.int32)) and float(word[0]) == 1.0 - decay


@pytest.mark.parametrize("n", [1, 5, 4004, BIG])
def test_ema_step_dev_is_ema_step_bit_for_bit(n):
    _ema_pair(n, 0.999, seed=n % 1000)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_ema_step_dev_misaligned_views(k):
    _ema_pair(4004, 0.9, off=k, seed=k)


def test_ema_step_dev_refusals_touch_nothing():
    be = _be()
    gs = GuardSet(be.device)
    n = 300
    e_host = _values(5, n)
    e, p = gs.tensor(torch.from_numpy(e_host), "ema"), gs.tensor(torch.from_numpy(_values(6, n)), "p")
    word = gs.tensor(torch.tensor([0.5, 0.5], dtype=torch.float64), "omd")
    L, st = be.L, be._st()
    E, Pp, W = e.data_ptr(), p.data_ptr(), word.data_ptr()
    cases = [L.rcot_ema_step_dev(0, Pp, n, W, st), L.rcot_ema_step_dev(E, 0, n, W, st), L.rcot_ema_step_dev(E, Pp, 0, W, st),
             L.rcot_ema_step_dev(E, Pp, n, 0, st), L.rcot_ema_step_dev(E, Pp, n, W + 4, st), L.rcot_ema_step_dev(E + 2, Pp, n - 1, W, st),
             L.rcot_ema_step_dev(E, E + 400, 200, W, st), L.rcot_ema_step_dev(E, E, n, W, st)]
    assert cases == [EINVAL] * len(cases), cases
    gs.check()
    assert np.array_equal(e.cpu().numpy().view(np.int32), e_host.view(np.int32))


# ------------------------------------------------------------------------------- AdamW
def _adam_buffers(gs, n, seed, tag=""):
    p = gs.tensor(torch.from_numpy(_values(seed, n)), "p" + tag)
    g = gs.tensor(torch.from_numpy(_values(seed + 1, n)), "g" + tag)
    return p, g, gs.full(n, 0.0, name="m" + tag), gs.full(n, 0.0, name="v" + tag)


@pytest.mark.parametrize("n", [4, 4004, BIG])
def test_adamw_without_decay_is_adam_and_with_decay_the_restatement(n):
    be = _be()
    gs = GuardSet(be.device)
    lr, wd = 3e-4, 1e-2
    p1, g, m1, v1 = _adam_buffers(gs, n, 7)
    p2, m2, v2 = gs.tensor(p1.cpu(), "p2"), gs.full(n, 0.0, name="m2"), gs.full(n, 0.0, name="v2")
    p3, m3, v3 = gs.tensor(p1.cpu(), "p3"), gs.full(n, 0.0, name="m3"), gs.full(n, 0.0, name="v3")
    hb = ScheduleBackend(torch.float64)
    hp, hg = p1.cpu().double(), g.cpu().double()
    hm, hv = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t in range(1, 4):
        be.adamw_step(p1, g, m1, v1, n, lr, t, 0.0)
        be.adam_step(p2, g, m2, v2, n, lr, t)
        be.adamw_step(p3, g, m3, v3, n, lr, t, wd)
        hb.adamw_step(hp, hg, hm, hv, n, lr, t, wd)
    gs.check()
    assert _same_bits(p1, p2) and _same_bits(m1, m2) and _same_bits(v1, v2)
    errs = [relerr(a, b) for a, b in ((p3, hp), (m3, hm), (v3, hv))]
    print(f"n {n}: AdamW vs fp64 restatement, 3 steps: rel err p {errs[0]:.2e} m {errs[1]:.2e} v {errs[2]:.2e}")
    assert max(errs) < 1e-5
    assert _same_bits(m3, m1) and _same_bits(v3, v1) and not _same_bits(p3, p1)        # the decay is decoupled: the moments do not see it
    # what the decay took over the three steps is 3 lr wd p: nine roundings of at most 2^-24 |p| between the two runs (three in the
    # Adam run, six in the AdamW run), and the decay of the 3e-4-sized Adam steps themselves, far below that
    d = (p3.double() - p1.double()).cpu()
    want = -(3 * lr * wd) * p1.double().cpu()
    assert float((d - want).abs().max()) <= 5 * 2.0 ** -23 * float(p1.abs().max()) + 1e-3 * float(want.abs().max())
    assert float(want.abs().max()) > 10 * 5 * 2.0 ** -23 * float(p1.abs().max())


def test_adamw_refusals():
    be = _be()
    gs = GuardSet(be.device)
    n = 64
    p, g, m, v = _adam_buffers(gs, n, 3)
    ctrl = gs.full((lib.CB_WORDS,), 0.0, torch.float64, "ctrl")
    p0 = p.clone()
    L, st = be.L, be._st()
    Pp, G, M_, V, C = (t.data_ptr() for t in (p, g, m, v, ctrl))
    cases = [L.rcot_adamw_step(Pp, G, M_, V, n, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, -1e-2, st), L.rcot_adamw_step(Pp, G, M_, V, n, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, float("nan"), st),
             L.rcot_adamw_step(Pp, G, M_, V, n - 1, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, 1e-2, st), L.rcot_adamw_step(Pp, G, M_, V, n, 1e-3, 0.9, 0.999, 1e-8, 0, 1.0, 1e-2, st),
             L.rcot_adamw_step(0, G, M_, V, n, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, 1e-2, st), L.rcot_adamw_step(Pp + 4, G, M_, V, n - 4, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, 1e-2, st),
             L.rcot_adamw_step(Pp, G, M_, V, n - 1, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, 0.0, st),
             L.rcot_adamw_step_guarded(Pp, G, M_, V, n, 0.9, 0.999, 1e-8, C, 0, -1.0, st), L.rcot_adamw_step_guarded(Pp, G, M_, V, n, 0.9, 0.999, 1e-8, C, 0, float("nan"), st),
             L.rcot_adamw_step_guarded(Pp, G, M_, V, n, 0.9, 0.999, 1e-8, 0, 0, 1e-2, st), L.rcot_adamw_step_guarded(Pp, G, M_, V, n, 0.9, 0.999, 1e-8, C, 2, 1e-2, st),
             L.rcot_adamw_step_guarded(Pp, G, M_, V, n + 2, 0.9, 0.999, 1e-8, C, 0, 1e-2, st), L.rcot_adamw_step_guarded(Pp, G, M_, V, n, 0.9, 0.999, 1e-8, C + 4, 0, 1e-2, st)]
    assert cases == [EINVAL] * len(cases), cases
    gs.check()
    assert _same_bits(p, p0)


def _decide(be, gs_ctrl, partials, g, n, lr=None, skip_value=None):
    if lr is not None:
        gs_ctrl[lib.CB_LR] = lr
    partials.fill_(float("nan"))
    parts = be.grad_sumsq(g, n, partials)
    be.grad_decide(partials, parts, gs_ctrl, 1)


@pytest.mark.parametrize("n", [4, 4004, BIG])
def test_guarded_adamw_reads_rate_and_skip_from_the_block(n):
    be = _be()
    gs = GuardSet(be.device)
    wd = 1e-2
    pa, g, ma, va = _adam_buffers(gs, n, 11, "a")                          # AdamW guarded, wd = 0
    pb, mb, vb = gs.tensor(pa.cpu(), "pb"), gs.full(n, 0.0, name="mb"), gs.full(n, 0.0, name="vb")      # Adam guarded
    pc, mc, vc = gs.tensor(pa.cpu(), "pc"), gs.full(n, 0.0, name="mc"), gs.full(n, 0.0, name="vc")      # AdamW guarded, wd
    pd, md, vd = gs.tensor(pa.cpu(), "pd"), gs.full(n, 0.0, name="md"), gs.full(n, 0.0, name="vd")      # AdamW by value at the block's rate
    ctrl = gs.full((lib.CB_WORDS,), 0.0, torch.float64, "ctrl")
    ctrl[lib.CB_MAX_NORM] = math.inf
    partials = gs.empty((lib.SUMSQ_MAX_PARTS,), torch.float64, "partials")
    for t, lr in ((1, 3e-4), (2, 7e-5)):                                   # the word changes between the two launches
        _decide(be, ctrl, partials, g, n, lr=lr)
        be.adamw_step_guarded(pa, g, ma, va, n, ctrl, 0, 0.0)
        be.adam_step_guarded(pb, g, mb, vb, n, ctrl, 0)
        be.adamw_step_guarded(pc, g, mc, vc, n, ctrl, 0, wd)
        before = pd.clone()
        be.adamw_step(pd, g, md, vd, n, lr, t, wd)
        gs.check()
        assert _same_bits(pa, pb) and _same_bits(ma, mb) and _same_bits(va, vb)
        # the guarded launch forms 1 - beta^t on the device (its pow may differ from the host's in the last bit): the 1e-5 bar on the step
        e = relerr(pc, pd)
        print(f"n {n} t {t} lr {lr}: guarded vs by-value AdamW rel err {e:.2e}; step taken {relerr(before, pd):.2e}")
        assert e < 1e-5 and relerr(mc, md) < 1e-5 and relerr(vc, vd) < 1e-5
        assert relerr(before, pd) > 3e-5                                  # either rate moves p by far more than the bar
        pd.copy_(pc)                                                       # the two runs go on from the same point
    keep = [x.clone() for x in (pc, mc, vc)]
    ctrl.view(torch.int64)[lib.CB_SKIP] = 1                                # the skip flag set: nothing moves, decay included
    be.adamw_step_guarded(pc, g, mc, vc, n, ctrl, 0, wd)
    gs.check()
    assert all(_same_bits(a, b) for a, b in zip((pc, mc, vc), keep))
    ctrl.view(torch.int64)[lib.CB_SKIP] = 0
    be.adamw_step_guarded(pc, g, mc, vc, n, ctrl, 1, wd)                   # counter 1 never advanced: nothing moves either
    gs.check()
    assert all(_same_bits(a, b) for a, b in zip((pc, mc, vc), keep))


# ------------------------------------------------------------------------------- one small scheduled minimax iteration
K, PS, SPEC, WARM, TOTAL, DECAY, WD = 7, 32, "restarts:2,3", 1, 6, 0.999, 1e-2


def _stepper(plan, scheduled=True):
    from rcot_amd.ema import WeightAverage
    from rcot_amd.net_restormer import F_net, T_net
    from rcot_amd.trainer import FlatOptimizer, MinimaxStep
    os.environ["RCOT_PLAN"] = "1" if plan else "0"
    try:
        Tn, Fn = T_net(decoder=True), F_net(patch_size=PS)
        Tn.load_state_dict({k: torch.from_numpy(v) for k, v in P.seeded_params(P.tnet_param_shapes(), 31, "T").items()})
        Fn.load_state_dict({k: torch.from_numpy(v) for k, v in P.seeded_params(P.fnet_param_shapes(PS), 32, "F").items()})
        if scheduled:
            To, Fo = FlatOptimizer(Tn, "AdamW", 5e-5, math.inf, WD), FlatOptimizer(Fn, "AdamW", 1e-4, math.inf, WD)
            avg = WeightAverage(Tn, DECAY)
            sched = schedule.Schedule(Tn.be, SPEC, 1e-4, TOTAL, WARM, ema_decay=DECAY)     # TOTAL < K: the last entry is held
            sched.bind(To, Fo)
            avg.omd_word = sched.omd_word
            st = MinimaxStep(Tn, Fn, To, Fo, 1.0, 10000.0, ema=avg, schedule=sched)
        else:
            st = MinimaxStep(Tn, Fn, FlatOptimizer(Tn, "RMSprop", 5e-5), FlatOptimizer(Fn, "RMSprop", 1e-4), 1.0, 10000.0)
    finally:
        os.environ.pop("RCOT_PLAN", None)
    st.set_de_ids([2])
    assert (st.planned is not None and st.planned.enabled) == plan
    return st


def _iterate(st, i):
    from rcot_amd.synth import make_batch
    _, x, y = make_batch(300 + i, 1, PS, [2])
    alpha = torch.rand(1, generator=torch.Generator().manual_seed(i))
    st.run(x.cuda(), y.cuda(), torch.tensor([2], dtype=torch.int32).cuda(), alpha.cuda(), False)
    torch.cuda.synchronize()


def _state(st):
    return {"T": st.T.store.flat, "F": st.F.store.flat, "T.m": st.To.m, "T.v": st.To.v, "F.m": st.Fo.m, "F.v": st.Fo.v, "ema": st.ema.buf,
            "sched": st.schedule.block, "T.ctrl": st.To.ctrl, "F.ctrl": st.Fo.ctrl}


@pytest.fixture(scope="module")
def runs():
    """K iterations eagerly and K through the launch plans (warm-up pass, recording, K - 1 replays), rates read after every one"""
    out = {}
    for plan in (False, True):
        st = _stepper(plan)
        rates = []
        for i in range(K):
            _iterate(st, i)
            rates.append((float(st.schedule.block[lib.SB_LR]), float(st.To.ctrl[lib.CB_LR]), float(st.Fo.ctrl[lib.CB_LR]), float(st.schedule.block[lib.SB_EMA_OMD]),
                          st.Fo.param_groups[0]["lr"]))
        out[plan] = (st, rates, {k: v.clone() for k, v in _state(st).items()})
    return out


def test_scheduled_iteration_counts_rates_and_recorded_names(runs):
    tb = schedule.table(SPEC, 1e-4, TOTAL, WARM)
    for plan in (False, True):
        st, rates, state = runs[plan]
        i = state["sched"].cpu().view(torch.int64)
        assert int(i[lib.SB_T]) == K == st.schedule.t and int(i[lib.SB_EMA_UPDATES]) == K == st.schedule.ema_updates == st.ema.updates
        for k, (v, vT, vF, omd, shown) in enumerate(rates):
            want = tb[min(k, TOTAL - 1)]                                   # iteration 6 holds entry 5
            assert (v, vT, vF, shown) == (want, want * 0.5, want, want), (plan, k)
            assert abs(omd - ema_omd(DECAY, k)) <= float(np.spacing(np.float32(ema_omd(DECAY, k))))
        cT, cF = st.To.guard_counters(), st.Fo.guard_counters()
        assert (cT["steps"], cT["skipped"], cF["steps"], cF["skipped"]) == (K, 0, 2 * K, 0)       # the warm-up pass left nothing behind
        sdT, sdF = st.To.state_dict(), st.Fo.state_dict()
        assert (sdT["t_main"], sdF["t_main"], sdF["t_tail"]) == (K, 2 * K, K) and sdT["weight_decay"] == WD
        assert all(bool(torch.isfinite(t).all()) for k, t in state.items() if not k.endswith("ctrl"))      # (max_norm is inf)
    assert _same_bits(runs[False][2]["sched"], runs[True][2]["sched"])
    stp = runs[True][0]
    assert stp.planned.recordings == 1
    (ent,) = stp.planned.cache.values()
    names = [getattr(fn, "__name__", "") for fn, a, _ in ent["plan"].cmds if a is not None]
    assert names[0] == "rcot_sched_advance" and names.count("rcot_sched_advance") == 1
    assert names.count("rcot_adamw_step_guarded") == 4 and names.count("rcot_ema_step_dev") == 1
    assert not ({"rcot_rmsprop_step", "rcot_adam_step", "rcot_adamw_step", "rcot_ema_step", "rcot_adam_step_guarded"} & set(names))


def test_scheduled_iteration_eager_and_planned_agree_bit_for_bit(runs):
    """parameters, optimizer state, EMA buffer, schedule block and control blocks after K iterations, eager against planned"""
    (_, _, e), (_, _, p) = runs[False], runs[True]
    diff = {}
    for k in e:
        a, b = e[k].double(), p[k].double()
        diff[k] = (int((_bits(e[k]) != _bits(p[k])).sum()), float((a - b).abs().max() / a.abs().max().clamp_min(1e-300)))
    print("eager vs planned, (32-bit words that differ, max |a - b| / max |a|): " + ", ".join(f"{k} {v[0]} {v[1]:.2e}" for k, v in diff.items()))
    assert all(v[0] == 0 for v in diff.values()), diff


def test_default_flags_record_none_of_the_new_entry_points():
    st = _stepper(True, scheduled=False)
    assert st.schedule is None and st.To.ctrl is None and st.Fo.ctrl is None
    for i in range(2):
        _iterate(st, i)
    (ent,) = st.planned.cache.values()
    names = {getattr(fn, "__name__", "") for fn, a, _ in ent["plan"].cmds if a is not None}
    assert not (names & NEW_ENTRY_POINTS) and "rcot_rmsprop_step" in names


# ------------------------------------------------------------------------------- the trainer CLI (subprocesses in a temporary directory)
def _py(args, cwd, env=None):
    return subprocess.run([sys.executable, "-m"] + args, capture_output=True, text=True, timeout=600, cwd=cwd,
                          env=dict(os.environ, PYTHONPATH=ROOT, **(env or {})))


def test_trainer_cli_schedule_checkpoint_and_resume(tmp_path):
    from rcot_amd.compat import load_checkpoint
    tmp = str(tmp_path)
    base = ["rcot_amd.trainer", "--synthetic", "--iters", "3", "--batchSize", "1", "--patch_size", "32", "--de_type", "denoise_15", "--seed", "5",
            "--type", "SchedTest", "--sigma", "1", "--degset", f"{tmp}/none/", "--tarset", f"{tmp}/none/",
            "--lr_schedule", "restarts:4,8", "--warmup_iters", "2", "--optimizer", "AdamW", "--weight_decay", "1e-4", "--ema", "0.999", "--ema_warmup"]
    r1 = _py(base + ["--nEpochs", "2"], tmp)
    assert r1.returncode == 0, r1.stderr[-3000:]
    tb = schedule.table("restarts:4,8", 1e-4, 6, 2)
    lines = [ln for ln in r1.stdout.splitlines() if ln.startswith("Epoch=")]
    assert lines == [f"Epoch=1, lr={float(tb[0])}", f"Epoch=2, lr={float(tb[3])}"], lines
    assert "guarded steps with max_norm inf" in r1.stdout
    ck1_path = os.path.join(tmp, "checkpoint", "model_SchedTest__2_1.0.pth")
    ck1 = load_checkpoint(ck1_path)
    assert ck1["schedule"] == {"spec": "restarts:4,8", "warmup_iters": 2, "total_iters": 6, "t": 6, "ema_updates": 6}
    assert ck1["T_optimizer"]["kind"] == "AdamW" and ck1["T_optimizer"]["weight_decay"] == 1e-4 and ck1["T_optimizer"]["t_main"] == 6
    assert ck1["ema"] == {"decay": 0.999, "updates": 6} and ck1["epoch"] == 2
    r2 = _py(base + ["--nEpochs", "3", "--resume", ck1_path], tmp)
    assert r2.returncode == 0, r2.stderr[-3000:]
    tb3 = schedule.table("restarts:4,8", 1e-4, 9, 2)
    assert [ln for ln in r2.stdout.splitlines() if ln.startswith("Epoch=")] == [f"Epoch=3, lr={float(tb3[6])}"]
    ck2 = load_checkpoint(os.path.join(tmp, "checkpoint", "model_SchedTest__3_1.0.pth"))
    assert ck2["schedule"]["t"] == 9 and ck2["schedule"]["ema_updates"] == 9 and ck2["T_optimizer"]["t_main"] == 9


def test_trainer_cli_stock_mprnet_refuses_a_schedule(tmp_path):
    tmp = str(tmp_path)
    r3 = _py(["rcot_amd.trainer", "--synthetic", "--iters", "1", "--nEpochs", "1", "--backbone", "mprnet", "--lr_schedule", "cosine"], tmp,
             env={"RCOT_MPRNET_STOCK": "1"})
    assert r3.returncode != 0 and "--lr_schedule needs the fused optimizers over a flat parameter store" in r3.stderr, r3.stderr[-2000:]
