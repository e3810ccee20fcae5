"""CPU tier: gradient-norm clipping and the non-finite step skip — the restatement (tests/clip_double.py) against torch itself
(clip_grad_norm_ followed by torch.optim.RMSprop / Adam .step(), or no .step() when the norm is not finite), and the host side
(rcot_amd/trainer.py FlatOptimizer(max_norm=...)) on a backend double.

Bars.  torch sums the n squares in fp32 in an order of its choosing: its norm is within n 2^-24 relative of the exact one (the any-order
bound), n = 4004: 2.4e-4; the restatement's own fp64 error is nothing beside it.  The clip coefficient inherits that bound.  Parameters
and state after three steps: the 1e-5 of tests/test_kernels_gpu.py::test_optimizers plus twice that bound (every gradient carries the
coefficient once, its square twice).

What torch does when finite fp32 squares overflow its fp32 sum (a norm of Inf for a finite gradient) is not ours — the sum here is
fp64 and such a gradient is clipped like any other — and is deliberately not compared."""
import math

import numpy as np
import pytest
import torch

from clip_double import ClipBackend, adam_guarded, decide, rmsprop_guarded, sumsq
from rcot_amd import lib
from rcot_amd.net_restormer import F_net, ParamStore
from rcot_amd.trainer import FlatOptimizer, check_max_norm, guard_report

N = 4004
SPLIT = [(1000,), (3, 1001), (1,)]                     # 1000 + 3003 + 1 = N
ANY_ORDER = N * 2.0 ** -24                             # 2.4e-4


def _grads(seed):
    g = torch.Generator().manual_seed(seed)
    return [0.3 * torch.randn(s, generator=g) for s in SPLIT]       # norm about 0.3 sqrt(4004) = 19


def relerr(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("M", [1.0, 1e3, math.inf])
def test_clip_coefficient_against_torch(M):
    gs = _grads(1)
    ps = [torch.nn.Parameter(torch.zeros(s)) for s in SPLIT]
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    tn = float(torch.nn.utils.clip_grad_norm_(ps, M))
    flat = torch.cat([g.reshape(-1) for g in gs]).numpy()
    norm, scale, skip = decide(sumsq(flat), M)
    assert not skip and abs(norm - tn) <= ANY_ORDER * tn
    want = min(1.0, M / (tn + 1e-6))
    assert abs(scale - want) <= ANY_ORDER * want
    assert (scale < 1.0) == (M == 1.0)
    got = torch.cat([p.grad.reshape(-1) for p in ps])                      # what torch left in .grad is g * its coefficient
    assert relerr(torch.from_numpy(flat) * np.float32(scale), got) <= ANY_ORDER + 2.0 ** -23


@pytest.mark.parametrize("bad_at", [None, 1], ids=["finite", "step2_nan"])
@pytest.mark.parametrize("M", [1.0, 1e3, math.inf])
@pytest.mark.parametrize("kind", ["RMSprop", "Adam"])
def test_three_guarded_steps_against_torch(kind, M, bad_at):
    g0 = torch.Generator().manual_seed(7)
    init = [torch.randn(s, generator=g0) for s in SPLIT]
    ps = [torch.nn.Parameter(t.clone()) for t in init]
    opt = (torch.optim.RMSprop if kind == "RMSprop" else torch.optim.Adam)(ps, lr=1e-3)
    p = torch.cat([t.reshape(-1) for t in init]).clone()
    s1, s2 = torch.zeros(N), torch.zeros(N)
    t_adam, skips = 0, 0
    for it in range(3):
        gs = _grads(10 + it)
        if bad_at == it:
            gs[1][2, 17] = float("nan")
        for q, g in zip(ps, gs):
            q.grad = g.clone()
        tn = torch.nn.utils.clip_grad_norm_(ps, M)
        if bool(torch.isfinite(tn)):
            opt.step()                                                     # the oracle: no .step() when the norm is not finite
        flat = torch.cat([g.reshape(-1) for g in gs])
        before = (p.clone(), s1.clone(), s2.clone())
        if kind == "RMSprop":
            _, _, skip = rmsprop_guarded(p, flat, s1, 1e-3, M)
        else:
            _, _, skip, t_adam = adam_guarded(p, flat, s1, s2, 1e-3, t_adam + 1, M)
        assert skip == (bad_at == it)
        skips += skip
        if skip:
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, (p, s1, s2)))
    bar = 1e-5 + 2 * ANY_ORDER
    assert relerr(p, torch.cat([q.detach().reshape(-1) for q in ps])) <= bar
    key = {"RMSprop": ["square_avg"], "Adam": ["exp_avg", "exp_avg_sq"]}[kind]
    for mine, k in zip((s1, s2), key):
        theirs = torch.cat([opt.state[q][k].reshape(-1) for q in ps])
        assert relerr(mine, theirs) <= bar, k
    if kind == "Adam":
        assert t_adam == 3 - skips == int(opt.state[ps[0]]["step"])
    assert float((p - torch.cat([t.reshape(-1) for t in init])).abs().max()) > 0


def test_overflowing_fp32_squares_are_finite_here():
    """stated, not compared with torch: 1e20^2 overflows fp32, the fp64 sum is finite and the step is clipped, not skipped"""
    g = np.array([1e20, -3e19, 1.0, 0.0], dtype=np.float32)
    norm, scale, skip = decide(sumsq(g), 1.0)
    assert not skip and math.isfinite(norm) and 0 < scale < 1e-19
    for bad in (np.inf, -np.inf, np.nan):
        g[3] = bad
        assert decide(sumsq(g), 1.0)[2]
    assert decide(0.0, 1.0) == (0.0, 1.0, False)                           # all-zero gradients: scale 1, no skip


# ------------------------------------------------------------------------------- the host side on a backend double
SHAPES = [("a.weight", (5, 3)), ("b.bias", (7,)), ("c.weight", (2, 2, 3, 3)), ("dead.weight", (4,))]


class _Net:
    def __init__(self, live):
        self.be = ClipBackend()
        self.store = ParamStore(self.be, SHAPES, live, ["dead.weight"])

    def fill(self, seed, scale=1.0):
        g = torch.Generator().manual_seed(seed)
        for n, shp in SHAPES[:3]:
            self.store.p[n].copy_(torch.rand(shp, generator=g) + 0.1)
            self.store.g[n].copy_((torch.rand(shp, generator=g) - 0.5) * scale)


def test_flags_off_means_no_control_block():
    net = _Net(["a.weight", "b.bias", "c.weight"])
    net.fill(1)
    for kind in ("RMSprop", "Adam"):
        o = FlatOptimizer(net, kind, 1e-3)
        assert o.ctrl is None and o.partials is None and o.max_norm is None
        o.sync_lr()                                                        # nothing to write
        o.step()
        assert "guard" not in o.state_dict()
    assert net.be.calls == []                                              # the plain launches only


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), -math.inf])
def test_max_norm_refusals(bad):
    with pytest.raises(ValueError, match="max_norm"):
        check_max_norm(bad)
    with pytest.raises(ValueError, match="max_norm"):
        FlatOptimizer(_Net(["a.weight", "b.bias", "c.weight"]), "RMSprop", 1e-3, max_norm=bad)
    assert check_max_norm(math.inf) == math.inf and check_max_norm("0.01") == 0.01


@pytest.mark.parametrize("argv,word", [(["--clip_grad_norm", "-1"], "--clip_grad_norm -1"), (["--clip_grad_norm", "nan"], "--clip_grad_norm nan"),
                                       (["--clip_grad_norm_F", "-0.5"], "--clip_grad_norm_F -0.5"), (["--clip_grad_norm_F", "nan"], "--clip_grad_norm_F nan"),
                                       (["--clip_grad_norm", "0.01", "--backbone", "mprnet"], "flat parameter store"),
                                       (["--clip_grad_norm_F", "inf", "--backbone", "mprnet"], "flat parameter store")])
def test_trainer_flag_refusals(argv, word, monkeypatch):
    from rcot_amd import trainer
    monkeypatch.setenv("RCOT_MPRNET_STOCK", "1")                           # the stock-ops MPRNet path, with or without a GPU
    with pytest.raises(SystemExit, match=word) as e:
        trainer.main(["--synthetic", "--iters", "1", "--nEpochs", "1"] + argv)
    assert "--clip_grad_norm" in str(e.value)


def test_trainer_flags_default_off_and_accept_inf():
    from rcot_amd import trainer
    o = trainer.parser.parse_args([])
    assert o.clip_grad_norm == 0.0 and o.clip_grad_norm_F == 0.0
    trainer.check_clip_flags(o)
    o = trainer.parser.parse_args(["--clip_grad_norm", "inf", "--clip_grad_norm_F", "0.5"])
    trainer.check_clip_flags(o)
    assert o.clip_grad_norm == math.inf and o.clip_grad_norm_F == 0.5


def test_learning_rate_travels_through_the_block():
    net = _Net(["a.weight", "b.bias", "c.weight"])
    net.fill(2)
    o = FlatOptimizer(net, "RMSprop", 1e-3, max_norm=math.inf)
    assert float(o.ctrl[lib.CB_LR]) == 1e-3 and float(o.ctrl[lib.CB_MAX_NORM]) == math.inf
    o.param_groups[0]["lr"] = 0.0
    p0, sq0 = net.store.flat.clone(), o.sq.clone()
    o.step()
    assert float(o.ctrl[lib.CB_LR]) == 0.0
    assert torch.equal(net.store.flat, p0) and not torch.equal(o.sq, sq0)  # rate 0: the parameters stay, the state moves
    o.param_groups[0]["lr"] = 2.5e-4
    o.sync_lr()
    assert float(o.ctrl[lib.CB_LR]) == 2.5e-4
    o.step()
    assert not torch.equal(net.store.flat, p0)


@pytest.mark.parametrize("kind", ["RMSprop", "Adam"])
def test_guard_round_trip_between_two_layouts(kind):
    a, b = _Net(["a.weight", "b.bias", "c.weight"]), _Net(["c.weight", "a.weight", "b.bias"])
    assert a.store.layout.offset != b.store.layout.offset
    oa = FlatOptimizer(a, kind, 1e-2, max_norm=0.5)
    for it in range(4):
        a.fill(20 + it, scale=1.0 if it != 2 else 0.01)                    # norms about 2 (clipped) and 0.02 (not)
        if it == 1:
            a.store.g["b.bias"][3] = float("inf")
        oa.step()
    sd = oa.state_dict()
    g = sd["guard"]
    assert (g["max_norm"], g["steps"], g["clipped"], g["skipped"]) == (0.5, 4, 2, 1) and 1.0 < g["max_seen"] < 4.0
    assert set(g) == {"max_norm", "steps", "clipped", "skipped", "max_seen"}
    assert sd["t_main"] == (3 if kind == "Adam" else 0)
    ob = FlatOptimizer(b, kind, 1e-2, max_norm=0.5)
    b.store.load(a.store.state_dict())
    ob.load_state_dict(sd)
    back = ob.state_dict()
    assert back["guard"] == g and back["t_main"] == sd["t_main"] and back["t_tail"] == sd["t_tail"]
    for key in sd["state"]:
        for n, _ in SHAPES:
            assert torch.equal(back["state"][key][n], sd["state"][key][n])
    for net in (a, b):                                                     # one more step on both: the same named results
        net.fill(30)
    oa.step()
    ob.step()
    for n, _ in SHAPES[:3]:
        assert torch.equal(a.store.p[n], b.store.p[n]), n
    assert ob.state_dict()["guard"]["steps"] == 5 and ob.state_dict()["t_main"] == oa.state_dict()["t_main"]
    # a state without "guard" (saved by an unguarded run) starts the counters at zero
    plain = {k: v for k, v in sd.items() if k != "guard"}
    oc = FlatOptimizer(_Net(["a.weight", "b.bias", "c.weight"]), kind, 1e-2, max_norm=math.inf)
    oc.load_state_dict(plain)
    assert oc.state_dict()["guard"] == {"max_norm": math.inf, "steps": 0, "clipped": 0, "skipped": 0, "max_seen": 0.0}


@pytest.fixture(scope="module")
def fnet():
    return F_net(patch_size=32, backend=ClipBackend(), seed=3)


def test_gradient_penalty_step_takes_the_norm_of_its_own_range(fnet):
    """the gradient-penalty step covers [0, offset of fc2.bias): the norm leaves fc2.bias and everything behind it out"""
    net = fnet
    lay = net.store.layout
    n_gp = net.n_live_gp
    assert n_gp == lay.offset["fc2.bias"] and n_gp % 4 == 0 and n_gp < lay.n_live
    o = FlatOptimizer(net, "RMSprop", 1e-4, max_norm=1.0)
    gen = torch.Generator().manual_seed(5)
    net.store.grad.copy_(0.01 * torch.randn(lay.n_total, generator=gen))
    net.store.grad[n_gp:] = float("nan")                                   # fc2.bias and the rest: never read by this step
    p0 = net.store.flat.clone()
    net.be.calls.clear()
    o.step(n_gp)
    assert net.be.calls == [("grad_sumsq", n_gp), ("grad_decide", 0), ("rmsprop_step_guarded", n_gp)]
    c = o.guard_counters()
    want = math.sqrt(sumsq(net.store.grad[:n_gp].numpy()))
    assert c["skipped"] == 0 and abs(c["last_norm"] - want) <= 1e-12 * want
    assert not torch.equal(net.store.flat[:n_gp], p0[:n_gp]) and torch.equal(net.store.flat[n_gp:], p0[n_gp:])
    o.step()                                                               # the full range reads the NaN: skipped
    assert o.guard_counters()["skipped"] == 1 and o.guard_counters()["steps"] == 2


def test_the_penalty_step_follows_a_skipped_critic_step(fnet):
    """step(same_batch=True): skipped when the previous step of this optimizer was, though its own gradients are finite (how
    MinimaxStep makes the gradient-penalty step: tests/test_clip_gpu.py)"""
    net = fnet
    lay, n_gp = net.store.layout, net.n_live_gp
    o = FlatOptimizer(net, "RMSprop", 1e-4, max_norm=math.inf)
    gen = torch.Generator().manual_seed(8)
    net.store.grad.copy_(0.01 * torch.randn(lay.n_total, generator=gen))
    net.store.grad[n_gp:] = float("nan")                                   # the critic's gradients are bad past the penalty's range only
    p0 = net.store.flat.clone()
    net.be.calls.clear()
    o.step()
    o.step(n_gp, same_batch=True)                                          # finite on its own range, skipped with the critic step
    assert ("grad_decide", 0) in net.be.calls and ("grad_decide", lib.DECIDE_INHERIT) in net.be.calls
    c = o.guard_counters()
    assert (c["steps"], c["skipped"]) == (2, 2) and math.isfinite(c["last_norm"]) and torch.equal(net.store.flat, p0)
    o.step(n_gp)                                                           # without the flag the same gradients are stepped over
    assert o.guard_counters()["skipped"] == 2 and not torch.equal(net.store.flat[:n_gp], p0[:n_gp])
    p1 = net.store.flat.clone()
    o.step(n_gp, same_batch=True)                                          # after a taken step there is nothing to inherit
    assert o.guard_counters()["skipped"] == 2 and not torch.equal(net.store.flat[:n_gp], p1[:n_gp])
    plain = FlatOptimizer(net, "RMSprop", 1e-4)                            # unguarded: the argument changes nothing
    net.store.grad[n_gp:] = 0.0
    plain.step(n_gp, same_batch=True)


def test_adam_counters_do_not_advance_on_a_skip(fnet):
    net = fnet
    lay = net.store.layout
    o = FlatOptimizer(net, "Adam", 1e-4, max_norm=math.inf)
    tail = lay.offset["fc2.bias"]
    gen = torch.Generator().manual_seed(6)

    def counts():
        sd = o.state_dict()
        return sd["t_main"], sd["t_tail"]
    net.store.grad.copy_(0.01 * torch.randn(lay.n_total, generator=gen))
    net.be.calls.clear()
    o.step()                                                               # critic step: both ranges
    assert [c[0] for c in net.be.calls] == ["grad_sumsq", "grad_decide", "adam_step_guarded", "adam_step_guarded"]
    assert net.be.calls[1] == ("grad_decide", 3) and net.be.calls[2] == ("adam_step_guarded", tail)
    assert counts() == (1, 1)
    o.step(net.n_live_gp)                                                  # gradient penalty: fc2.bias keeps its count
    assert counts() == (2, 1)
    net.store.grad[7] = float("nan")
    p0, m0, v0 = net.store.flat.clone(), o.m.clone(), o.v.clone()
    o.step()
    o.step(net.n_live_gp)
    assert counts() == (2, 1) and o.guard_counters()["skipped"] == 2
    assert torch.equal(net.store.flat, p0) and torch.equal(o.m, m0) and torch.equal(o.v, v0)
    net.store.grad[7] = 0.0
    o.step()
    assert counts() == (3, 2) and not torch.equal(net.store.flat, p0)
    # the plain Adam over the same gradients with host counters 3 / 2 would have made this very step
    ref = p0.clone()
    m, v = m0.clone(), v0.clone()
    net.be.adam_step(ref, net.store.grad, m, v, tail, 1e-4, 3)
    net.be.adam_step(ref[tail:], net.store.grad[tail:], m[tail:], v[tail:], lay.n_total - tail, 1e-4, 2)
    assert torch.equal(ref, net.store.flat) and torch.equal(m, o.m) and torch.equal(v, o.v)
    # load_state_dict writes the counts into the block
    o2 = FlatOptimizer(net, "Adam", 1e-4, max_norm=math.inf)
    o2.load_state_dict(o.state_dict())
    i = o2.ctrl.view(torch.int64)
    assert (int(i[lib.CB_T]), int(i[lib.CB_T + 1])) == (3, 2)


def test_epoch_report_and_all_skipped_exit():
    now = {"max_norm": 0.01, "steps": 9, "clipped": 4, "skipped": 1, "max_seen": 3.5, "last_norm": 0.25, "last_scale": 0.04}
    before = {"steps": 6, "clipped": 3, "skipped": 0}
    line = guard_report("T_net", now, before)
    assert line.startswith("clip T_net: max_norm 0.01, steps 3, clipped 1, skipped 1, last norm 0.25, largest norm 3.5")
    with pytest.raises(SystemExit, match="every optimizer step of this epoch was skipped"):
        guard_report("F_net", dict(now, steps=12, skipped=6), dict(before, steps=6, skipped=0))
    assert "steps 0" in guard_report("F_net", now, now)                    # an epoch without iterations is not an all-skipped one
