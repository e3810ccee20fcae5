"""CPU tier: per-iteration learning-rate schedules (rcot_amd/schedule.py) against rates recorded from the reference's own scheduler
classes (tests/golden/lr_schedules.json, written by scripts/make_schedule_fixture.py), the grammar's refusals, the trainer's host logic
on a backend double (tests/schedule_double.py) and the AdamW restatement against torch.optim.AdamW.

Bars.  Table against recording: 1e-12 relative — both sides are a handful of double operations, the MultiStepRestartLR recursion adds at
most one rounding per milestone.  AdamW in float64 over 5 steps against torch.optim.AdamW: 1e-14 absolute on values of order 1 (torch
multiplies by 1 - lr wd, the restatement subtracts (lr wd) p: an ulp or two of 2.2e-16 per step).

One structural fact is stated here as the reference's closed form gives it, not as a restart at full height: position 0 of a cycle,
eta_min + w (base - eta_min), is taken by t = 0 alone.  The reference puts t = cumulative period at the END of a cycle (exactly
eta_min), so the iteration after it is position 1 of the next cycle: eta_min' + w' (base - eta_min') (1 + cos(pi / period')) / 2.
Both are checked exactly."""
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from rcot_amd import lib, schedule
from rcot_amd.net_restormer import F_net, T_net
from rcot_amd.trainer import FlatOptimizer, MinimaxStep, restore_schedule
from schedule_double import ScheduleBackend, advance, ema_omd

GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "lr_schedules.json")))
CASES = {c["name"]: c for c in GOLD["cases"]}
BASE = GOLD["base_lr"]
NEW = {"sched_advance", "ema_step_dev", "adamw_step", "adamw_step_guarded"}


@pytest.mark.parametrize("name", ["CosineAnnealingRestartCyclicLR", "CosineAnnealingRestartLR", "LinearLR", "MultiStepRestartLR",
                                  "LambdaLR(linear_warmup_decay)"])
def test_table_against_the_reference_recording(name):
    c = CASES[name]
    want = np.asarray(c["rates"], dtype=np.float64)
    got = schedule.table(c["spec"], BASE, c["iters"], c["warmup_iters"])
    assert got.dtype == np.float64 and got.shape == want.shape == (40,)
    rel = float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))
    print(f"{name}: max relative difference {rel:.3e}")
    assert rel <= 1e-12
    assert float(np.ptp(want)) > 0 or name == "never"                      # no recording is a constant


def test_all_five_cases_are_recorded():
    assert BASE == 1e-4 and len(CASES) == 5
    a = CASES["CosineAnnealingRestartCyclicLR"]["args"]
    assert a["periods"] == [12, 28] and a["eta_mins"] == [1e-4, 1e-6]
    a = CASES["CosineAnnealingRestartLR"]["args"]
    assert a["periods"] == [10, 10, 20] and a["restart_weights"] == [1, 0.5, 0.25] and a["eta_min"] == 1e-7
    assert CASES["LinearLR"]["args"] == {"total_iter": 40}
    assert CASES["MultiStepRestartLR"]["args"] == {"milestones": [10, 20, 30], "gamma": 0.5}
    assert CASES["LambdaLR(linear_warmup_decay)"]["args"] == {"warmup_steps": 5, "total_steps": 40, "cosine": True}


def test_structural_facts_are_exact():
    periods, weights, eta = [10, 10, 20], [1.0, 0.5, 0.25], 1e-7
    tb = schedule.table("restarts:10,10,20:1,0.5,0.25:1e-7", BASE, 41)
    assert tb[0] == eta + weights[0] * (BASE - eta)                        # position 0: the full height, at t = 0 only
    cum = np.cumsum(periods)
    for k, c in enumerate(cum):
        assert tb[c] == eta, (c, tb[c])                                    # the last iteration of a cycle sits at eta_min
        if k + 1 < len(periods):                                           # the one after it: position 1 of the next cycle
            w, q = weights[k + 1], periods[k + 1]
            assert tb[c + 1] == eta + w * 0.5 * (BASE - eta) * (1 + math.cos(math.pi * (1 / q)))
            assert eta < tb[c + 1] < eta + w * (BASE - eta) and tb[c + 1] > 0.9 * w * BASE
    cyc = schedule.table("restarts:12,28:1,1:1e-4,1e-6", BASE, 40)
    assert np.all(cyc[:13] == 1e-4)                                        # eta_min == base: a flat first cycle
    assert cyc[13] == 1e-6 + 0.5 * (BASE - 1e-6) * (1 + math.cos(math.pi * (1 / 28)))
    assert schedule.table("restarts:12,28:1,1:1e-4,1e-6", BASE, 42)[40] == 1e-6 == schedule.table("restarts:12,28:1,1:1e-4,1e-6", BASE, 42)[41]
    warm = schedule.table("cosine", BASE, 40, 5)
    assert warm[0] == 0.0 and warm[5] == BASE and np.all(np.diff(warm[:6]) > 0) and np.all(np.diff(warm[5:]) < 0)
    assert list(warm[:5]) == [BASE * (t / 5) for t in range(5)]
    assert np.all(schedule.table("const", BASE, 9) == BASE)
    assert schedule.table("cosine:1e-6", BASE, 10)[0] == BASE and abs(schedule.table("cosine:1e-6", BASE, 10)[9] - 1e-6) < 0.03 * BASE
    ms = schedule.table("multistep:3,3,5", 1.0, 8)                         # default gamma, a milestone listed twice
    assert list(ms[:3]) == [1.0] * 3 and ms[3] == 1.0 * 0.1 ** 2 and ms[5] == ms[3] * 0.1 and ms[7] == ms[5]
    assert schedule.parse("restarts:4,8") == {"kind": "restarts", "periods": [4, 8], "weights": [1.0, 1.0], "eta_mins": [0.0, 0.0]}
    assert schedule.parse("restarts:4,8::1e-6")["eta_mins"] == [1e-6, 1e-6] and schedule.parse("step") == {"kind": "step"}


@pytest.mark.parametrize("spec,piece", [("restarts:12,,28", "''"), ("restarts:", "''"), ("restarts:12,28:1", "'1'"), ("restarts:12,28:1,1:0,0,0", "'0,0,0'"),
                                        ("restarts:12,0", "'0'"), ("restarts:12,x", "'x'"), ("restarts:4:1:0:9", "'4:1:0:9'"), ("warmcos", "'warmcos'"),
                                        ("", "''"), ("cosine:-1", "'-1'"), ("cosine:1e-6:3", "'3'"), ("cosine:1,2", "'1,2'"), ("linear:3", "'3'"),
                                        ("multistep", "''"), ("multistep:10,-2", "'-2'"), ("multistep:10:0", "'0'"), ("multistep:10:nan", "'nan'"),
                                        ("step:20", "'20'"), ("const:1", "'1'")])
def test_bad_specs_are_refused_with_the_piece_named(spec, piece):
    with pytest.raises(ValueError) as e:
        schedule.parse(spec)
    assert piece in str(e.value) and "--lr_schedule" in str(e.value), str(e.value)


@pytest.mark.parametrize("total,warm,word", [(40, -1, "--warmup_iters -1"), (40, 40, "--warmup_iters 40"), (40, 41, "--warmup_iters 41"), (0, 0, "total_iters 0")])
def test_bad_warmups_are_refused(total, warm, word):
    with pytest.raises(ValueError, match=word):
        schedule.table("cosine", BASE, total, warm)


@pytest.mark.parametrize("argv,word", [(["--lr_schedule", "restarts:4,,8"], "''"), (["--lr_schedule", "bogus"], "'bogus'"),
                                       (["--warmup_iters", "-3", "--lr_schedule", "cosine"], "--warmup_iters -3"),
                                       (["--warmup_iters", "2"], "--warmup_iters 2"), (["--ema_warmup"], "--ema_warmup"),
                                       (["--optimizer", "AdamW", "--weight_decay", "-1"], "--weight_decay -1"),
                                       (["--optimizer", "AdamW", "--weight_decay_F", "nan"], "--weight_decay_F nan"),
                                       (["--lr_schedule", "cosine", "--backbone", "mprnet"], "--lr_schedule needs the fused optimizers"),
                                       (["--optimizer", "AdamW", "--backbone", "mprnet"], "--optimizer AdamW needs the fused optimizers")])
def test_trainer_flag_refusals(argv, word, monkeypatch):
    from rcot_amd import trainer
    monkeypatch.setenv("RCOT_MPRNET_STOCK", "1")                           # the stock-ops MPRNet path, with or without a GPU
    with pytest.raises(SystemExit, match=word):
        trainer.main(["--synthetic", "--iters", "1", "--nEpochs", "1"] + argv)


def test_trainer_flag_defaults():
    from rcot_amd import trainer
    o = trainer.parser.parse_args([])
    assert (o.lr_schedule, o.warmup_iters, o.weight_decay, o.weight_decay_F, o.ema_warmup, o.optimizer) == ("step", 0, 0.01, None, False, "RMSprop")
    trainer.check_schedule_flags(o)
    o = trainer.parser.parse_args(["--lr_schedule", "restarts:4,8", "--warmup_iters", "2", "--optimizer", "AdamW", "--weight_decay", "1e-4", "--ema", "0.999",
                                   "--ema_warmup"])
    trainer.check_schedule_flags(o)


# ------------------------------------------------------------------------------- the block on the double
def test_advance_restatement_and_schedule_object():
    be = ScheduleBackend()
    s = schedule.Schedule(be, "restarts:2,3", 1e-4, 6, 1, ema_decay=0.999)
    tb = schedule.table("restarts:2,3", 1e-4, 6, 1)
    assert np.array_equal(s.table, tb) and s.block.dtype == torch.float64 and s.block.numel() == lib.SB_WORDS
    assert float(s.block[lib.SB_EMA_DECAY]) == 0.999
    c0, c1 = torch.zeros(lib.CB_WORDS, dtype=torch.float64), torch.zeros(lib.CB_WORDS, dtype=torch.float64)
    for k in range(9):
        advance(s.block, s.table, c0[lib.CB_LR:lib.CB_LR + 1], 0.5, c1[lib.CB_LR:lib.CB_LR + 1], 1.0)
        v = tb[min(k, 5)]                                                  # past the end the last entry holds
        i = s.block.view(torch.int64)
        assert int(i[lib.SB_T]) == k + 1 and float(s.block[lib.SB_LR]) == v and float(c0[lib.CB_LR]) == v * 0.5 and float(c1[lib.CB_LR]) == v
        assert int(i[lib.SB_EMA_UPDATES]) == k + 1 and float(s.block[lib.SB_EMA_OMD]) == ema_omd(0.999, k)
    assert ema_omd(0.999, 0) == 1 - 0.1 and ema_omd(0.999, 8980) > 1 - 0.999 and ema_omd(0.999, 9000) == 1 - 0.999 == ema_omd(0.999, 10 ** 6)
    only_ema = schedule.Schedule(be, "step", 1e-4, 6, 0, ema_decay=0.9)
    assert only_ema.table is None and only_ema.rate() is None
    only_ema.advance(be)
    assert (only_ema.t, only_ema.ema_updates) == (0, 1) and int(only_ema.block.view(torch.int64)[lib.SB_T]) == 0


def test_state_round_trip_and_a_checkpoint_without_the_key():
    be = ScheduleBackend()
    a = schedule.Schedule(be, "restarts:4,8", 1e-4, 12, 2, ema_decay=0.999)
    for _ in range(6):
        a.advance(be)
    sd = a.state_dict()
    assert sd == {"spec": "restarts:4,8", "warmup_iters": 2, "total_iters": 12, "t": 6, "ema_updates": 6}
    b = schedule.Schedule(be, "restarts:4,8", 1e-4, 12, 2, ema_decay=0.999)
    assert restore_schedule(b, sd, 2, 3) is None
    assert b.mirror() == (6, 6) and torch.equal(b.block.view(torch.int64)[[lib.SB_T, lib.SB_EMA_UPDATES]], a.block.view(torch.int64)[[lib.SB_T, lib.SB_EMA_UPDATES]])
    a.advance(be)
    b.advance(be)
    assert torch.equal(a.block.view(torch.int64), b.block.view(torch.int64)) and b.t == 7 and float(b.block[lib.SB_LR]) == a.table[6]
    c = schedule.Schedule(be, "restarts:4,8", 1e-4, 12, 2, ema_decay=0.999)
    note = restore_schedule(c, None, 2, 3, ema_updates=5)                  # epoch 2 of 3 iterations each: iteration 6
    assert "holds no schedule state" in note and "iteration 6" in note
    assert c.mirror() == (6, 5) and int(c.block.view(torch.int64)[lib.SB_T]) == 6 and c.rate() == c.table[6]


# ------------------------------------------------------------------------------- the trainer's host logic on the double
def _stepper(be, kind="RMSprop", spec=None, warm=0, ema_warmup=False, wd=0.0, use_new_args=True):
    from rcot_amd.ema import WeightAverage
    ps = 32
    Tn, Fn = T_net(decoder=True, backend=be, seed=0), F_net(patch_size=ps, backend=be, seed=1)
    M = math.inf if spec is not None else None
    if use_new_args:
        To, Fo = FlatOptimizer(Tn, kind, 5e-5, M, weight_decay=wd), FlatOptimizer(Fn, kind, 1e-4, M, weight_decay=wd)
    else:                                                                  # the constructor calls of the code before schedules existed
        To, Fo = FlatOptimizer(Tn, kind, 5e-5), FlatOptimizer(Fn, kind, 1e-4)
    avg = WeightAverage(Tn, 0.999) if ema_warmup else None
    sched = None
    if spec is not None or ema_warmup:
        sched = schedule.Schedule(be, spec or "step", 1e-4, 6, warm, ema_decay=0.999 if ema_warmup else 0.0)
        sched.bind(To, Fo)
        if ema_warmup:
            avg.omd_word = sched.omd_word
    st = MinimaxStep(Tn, Fn, To, Fo, 1.0, 10000.0, ema=avg, schedule=sched) if use_new_args else MinimaxStep(Tn, Fn, To, Fo, 1.0, 10000.0)
    st.set_de_ids([2])
    return st


def _run(st, i):
    g = torch.Generator().manual_seed(100 + i)
    clean = torch.rand(1, 3, 32, 32, generator=g)
    deg = (clean + 0.1 * torch.randn(1, 3, 32, 32, generator=g)).clamp(0, 1)
    st.run(deg, clean, torch.tensor([2], dtype=torch.int32), torch.rand(1, generator=g), False)


def test_default_flags_launch_what_the_code_before_launched():
    """every new argument at its default: the launch list of an iteration, by name, is that of a stepper built with the constructor
    calls that existed before, and holds none of the new launches; nothing is allocated for a schedule"""
    lists = []
    for new_args in (False, True):
        be = ScheduleBackend()
        st = _stepper(be, use_new_args=new_args)
        assert st.schedule is None and st.To.ctrl is None and not st.To.scheduled and st.To.weight_decay == 0.0
        be.names.clear()
        _run(st, 0)
        lists.append(list(be.names))
        assert "weight_decay" not in st.To.state_dict()
    assert lists[0] == lists[1] and len(lists[0]) > 100
    assert not (set(lists[0]) & NEW) and lists[0].count("rmsprop_step") == 3 and be.calls == []


def test_scheduled_iterations_on_the_double():
    be = ScheduleBackend()
    st = _stepper(be, "AdamW", "restarts:2,3", warm=1, ema_warmup=True, wd=1e-2)
    tb = st.schedule.table
    assert st.To.scheduled and st.Fo.scheduled and st.To.ctrl is not None
    # sync_lr writes nothing for a scheduled optimizer, whatever param_groups says
    st.To.ctrl[lib.CB_LR] = 123.0
    st.To.param_groups[0]["lr"] = 7.0
    st.To.sync_lr()
    assert float(st.To.ctrl[lib.CB_LR]) == 123.0
    poisoned = []

    def probe(tag):                                                        # iteration 2: a NaN in the transport map's gradients
        if tag == "T_gen" and st.schedule.t == 3:
            st.T.store.grad[5] = float("nan")
            poisoned.append(tag)
    st.grad_probe = probe
    for k in range(4):
        be.names.clear()
        T_before = st.T.store.flat.clone()
        _run(st, k)
        assert be.names[0] == "sched_advance" and be.names.count("sched_advance") == 1            # the head of the iteration, once
        assert be.names.count("adamw_step_guarded") == 4 and be.names.count("ema_step_dev") == 1   # F: 2 + 1 ranges, T: 1; no by-value twins
        assert not ({"adam_step", "adamw_step", "rmsprop_step", "ema_step"} & set(be.names))
        assert st.schedule.t == k + 1 and int(st.schedule.block.view(torch.int64)[lib.SB_T]) == k + 1
        assert float(st.Fo.ctrl[lib.CB_LR]) == tb[k] and float(st.To.ctrl[lib.CB_LR]) == tb[k] * 0.5
        assert st.Fo.param_groups[0]["lr"] == tb[k] and st.To.param_groups[0]["lr"] == tb[k] * 0.5    # kept current from the mirror
        assert float(st.schedule.block[lib.SB_EMA_OMD]) == ema_omd(0.999, k)
        if k == 2:
            assert poisoned == ["T_gen"] and torch.equal(st.T.store.flat, T_before)               # the step was skipped, t advanced all the same
    g = st.To.guard_counters()
    assert (g["steps"], g["skipped"]) == (4, 1) and st.To.state_dict()["t_main"] == 3
    assert st.To.state_dict()["weight_decay"] == 1e-2 and st.To.state_dict()["kind"] == "AdamW"
    assert st.ema.updates == 4


def test_adamw_optimizer_state_round_trip_and_kind_check():
    be = ScheduleBackend()
    net = F_net(patch_size=32, backend=be, seed=3)
    o = FlatOptimizer(net, "AdamW", 1e-3, weight_decay=0.05)
    gen = torch.Generator().manual_seed(4)
    net.store.grad.copy_(0.01 * torch.randn(net.store.layout.n_total, generator=gen))
    p0 = net.store.flat.clone()
    o.step()
    o.step(net.n_live_gp)                                                  # fc2.bias keeps its count, as under Adam
    sd = o.state_dict()
    assert (sd["kind"], sd["t_main"], sd["t_tail"], sd["weight_decay"]) == ("AdamW", 2, 1, 0.05)
    assert be.names.count("adamw_step") == 3 and not torch.equal(net.store.flat, p0)
    o2 = FlatOptimizer(net, "AdamW", 1e-3, weight_decay=0.05)
    o2.load_state_dict(sd)
    back = o2.state_dict()
    assert (o2.t_main, o2.t_tail) == (2, 1) and back["weight_decay"] == 0.05
    for key in ("m", "v"):                                                 # by name: the padding between tensors is not state
        assert all(torch.equal(back["state"][key][k], sd["state"][key][k]) for k in sd["state"][key]) and len(sd["state"][key]) > 10
    with pytest.raises(ValueError, match="optimizer state is for AdamW"):
        FlatOptimizer(net, "Adam", 1e-3).load_state_dict(sd)
    with pytest.raises(ValueError, match="weight_decay"):
        FlatOptimizer(net, "AdamW", 1e-3, weight_decay=-1.0)
    # weight_decay 0: Adam's step, bit for bit
    a, b = F_net(patch_size=32, backend=be, seed=3), F_net(patch_size=32, backend=be, seed=3)
    for n_ in (a, b):
        n_.store.grad.copy_(net.store.grad)
    FlatOptimizer(a, "AdamW", 1e-3, weight_decay=0.0).step()
    FlatOptimizer(b, "Adam", 1e-3).step()
    assert torch.equal(a.store.flat, b.store.flat)


def test_adamw_restatement_against_torch_in_float64():
    be = ScheduleBackend(torch.float64)
    n, lr, wd = 4004, 3e-4, 1e-2
    g0 = torch.Generator().manual_seed(11)
    init = torch.randn(n, generator=g0, dtype=torch.float64)
    q = torch.nn.Parameter(init.clone())
    opt = torch.optim.AdamW([q], lr=lr, weight_decay=wd)
    p, m, v = init.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t in range(1, 6):
        g = torch.randn(n, generator=g0, dtype=torch.float64)
        q.grad = g.clone()
        opt.step()
        be.adamw_step(p, g, m, v, n, lr, t, wd)
    err = float((p - q.detach()).abs().max())
    print(f"AdamW restatement vs torch.optim.AdamW, float64, 5 steps: max abs difference {err:.2e}")
    assert err <= 1e-14
    assert float((p - init).abs().max()) > 1e-4
    plain = init.clone()                                                   # not vacuous: Adam without the decay is further away
    m2, v2 = torch.zeros_like(m), torch.zeros_like(v)
    g0 = torch.Generator().manual_seed(11)
    torch.randn(n, generator=g0, dtype=torch.float64)
    for t in range(1, 6):
        be.adam_step(plain, torch.randn(n, generator=g0, dtype=torch.float64), m2, v2, n, lr, t)
    assert float((plain - q.detach()).abs().max()) > 1e-6
