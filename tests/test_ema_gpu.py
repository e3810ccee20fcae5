"""GPU tier: weight averaging (rcot_amd/ema.py) — the rcot_ema_step kernel on guard-banded buffers against its host restatement
(tests/ema_double.py), the average through eager and planned minimax iterations, ``applied()``, and the trainer / tester / export CLIs."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from ema_double import ema_step, ulp
from guarded import GuardSet
from rcot_amd import params as P

pytestmark = pytest.mark.gpu

EINVAL = -1
SWEEP = 4096 * 256          # threads of one full sweep of ema_kernel's grid (csrc/optim.hip: at most 4096 workgroups of 256)


def _values(seed, n):
    """fp32 values with magnitudes in [1e-4, 1] and random signs (no difference of two of them is subnormal)"""
    g = np.random.Generator(np.random.PCG64(seed))
    return (np.where(g.random(n) < 0.5, -1.0, 1.0) * 10.0 ** g.uniform(-4.0, 0.0, n)).astype(np.float32)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _call(be, ema, p, n, decay):
    """the raw entry point: returns its code"""
    return be.L.rcot_ema_step(ema if isinstance(ema, int) else ema.data_ptr(), p if isinstance(p, int) else p.data_ptr(), n, decay, be._st())


def _check_launch(n, decay, off_e=0, off_p=0, seed=0):
    """one launch over views that start off_e / off_p elements into guarded buffers: within 1 ulp of the restatement, p unchanged bit
    for bit, nothing outside the views touched (the rest of each buffer, and the guard bands)"""
    from rcot_amd.ops import default_backend
    be = default_backend()
    gs = GuardSet(be.device)
    e_host, p_host = _values(2 * seed + 1, n + 3), _values(2 * seed + 2, n + 3)
    e_buf, p_buf = gs.tensor(torch.from_numpy(e_host), "ema"), gs.tensor(torch.from_numpy(p_host), "p")
    rc = _call(be, e_buf[off_e:off_e + n], p_buf[off_p:off_p + n], n, decay)
    gs.check()
    assert rc == 0, rc
    got, want = e_buf.cpu().numpy(), e_host.copy()
    want[off_e:off_e + n] = ema_step(e_host[off_e:off_e + n], p_host[off_p:off_p + n], decay)
    outside = np.ones(n + 3, dtype=bool)
    outside[off_e:off_e + n] = False
    assert np.array_equal(got[outside].view(np.int32), e_host[outside].view(np.int32))
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    worst = int(np.argmax(err - ulp(want)))
    assert np.all(err <= ulp(want)), (worst, got[worst], want[worst])
    assert np.array_equal(p_buf.cpu().numpy().view(np.int32), p_host.view(np.int32))


@pytest.mark.parametrize("decay", [0.5, 0.999, 0.0])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 4 * SWEEP + 7])
def test_ema_step_sizes(n, decay):
    """both pointers 16-byte aligned: float4 body and the tail of n % 4; 4 SWEEP + 7 reaches the second grid-stride pass and the tail"""
    _check_launch(n, decay, seed=n % 1000)


@pytest.mark.parametrize("which", ["ema", "p", "both"])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_ema_step_misaligned_views(k, which):
    """views 1, 2, 3 elements into the buffer: the scalar path"""
    _check_launch(1027, 0.999, off_e=k if which != "p" else 0, off_p=k if which != "ema" else 0, seed=10 * k)


def test_ema_step_scalar_path_second_pass():
    """the scalar path's own sweep is SWEEP elements: 7 more reach its second grid-stride pass"""
    _check_launch(SWEEP + 7, 0.5, off_e=1, off_p=1, seed=77)


def test_ema_step_zeros_give_plus_zero():
    from rcot_amd.ops import default_backend
    be = default_backend()
    gs = GuardSet(be.device)
    for n in (5, 1027):
        e, p = gs.full(n, 0.0, name="ema"), gs.full(n, 0.0, name="p")
        assert _call(be, e, p, n, 0.999) == 0
        gs.check()
        assert int(_bits(e).abs().max()) == 0 and int(_bits(p).abs().max()) == 0        # +0: all bits clear


def test_ema_step_refusals_touch_nothing():
    from rcot_amd.ops import default_backend
    be = default_backend()
    gs = GuardSet(be.device)
    n = 300
    e_host, p_host = _values(5, n), _values(6, n)
    e, p = gs.tensor(torch.from_numpy(e_host), "ema"), gs.tensor(torch.from_numpy(p_host), "p")
    cases = [("decay 1", (e, p, n, 1.0)), ("decay < 0", (e, p, n, -0.1)), ("decay NaN", (e, p, n, float("nan"))), ("n 0", (e, p, 0, 0.5)),
             ("n < 0", (e, p, -4, 0.5)), ("null ema", (0, p, n, 0.5)), ("null p", (e, 0, n, 0.5)),
             ("overlap", (e[:200], e[100:300], 200, 0.5)), ("overlap, p first", (e[100:300], e[:200], 200, 0.5)), ("same", (e, e, n, 0.5)),
             ("2-byte offset", (e.data_ptr() + 2, p, n - 1, 0.5))]
    for name, a in cases:
        assert _call(be, *a) == EINVAL, name
        gs.check()
        assert np.array_equal(e.cpu().numpy().view(np.int32), e_host.view(np.int32)), name
        assert np.array_equal(p.cpu().numpy().view(np.int32), p_host.view(np.int32)), name
    assert _call(be, e[:100], e[100:200], 100, 0.5) == 0                                  # adjacent ranges do not overlap
    gs.check()
    from rcot_amd import lib
    with pytest.raises(lib.RcotKernelError):
        be.ema_step(e, p, n, 1.0)                                                         # the backend method raises on a refusal


def test_ema_step_addresses_past_2_31_bytes():
    """n = 2^29 + 5: more than 2^31 bytes per buffer (plain allocations).  p = i mod 251, ema = 2 (i mod 241), decay 0.5: small integers,
    so every correct result is exactly (p + ema) / 2."""
    from rcot_amd.ops import default_backend
    be = default_backend()
    n = 2 ** 29 + 5
    i = torch.arange(n, device=be.device)
    p = (i % 251).float()
    e = (2 * (i % 241)).float()
    del i
    want = (p + e) / 2
    p0 = p.clone()
    be.ema_step(e, p, n, 0.5)
    torch.cuda.synchronize()
    assert torch.equal(e, want)
    assert torch.equal(p, p0)
    del e, p, p0, want
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------- the average through the iteration
def _stepper(plan, kind="RMSprop", decay=0.5, ps=64, with_avg=True):
    """the set-up of tests/test_plan_gpu.py::_run: seeded parameters, ps = 64, lr 1e-4, de ids [2, 3]"""
    from rcot_amd.ema import WeightAverage
    from rcot_amd.net_restormer import F_net, T_net
    from rcot_amd.trainer import FlatOptimizer, MinimaxStep
    os.environ["RCOT_PLAN"] = "1" if plan else "0"
    try:
        lr = 1e-4
        Tn, Fn = T_net(decoder=True), F_net(patch_size=ps)
        Tn.load_state_dict({k: torch.from_numpy(v) for k, v in P.seeded_params(P.tnet_param_shapes(), 31, "T").items()})
        Fn.load_state_dict({k: torch.from_numpy(v) for k, v in P.seeded_params(P.fnet_param_shapes(ps), 32, "F").items()})
        avg = WeightAverage(Tn, decay) if with_avg else None
        st = MinimaxStep(Tn, Fn, FlatOptimizer(Tn, kind, lr / 2), FlatOptimizer(Fn, kind, lr), 1.0, 10000.0, ema=avg)
    finally:
        os.environ.pop("RCOT_PLAN", None)
    st.set_de_ids([2, 3])
    return st, avg


def _iterate(st, i, ps=64, B=2):
    from rcot_amd.synth import make_batch
    de = [2, 3]
    _, x, y = make_batch(300 + i, B, ps, de)
    alpha = torch.rand(B, generator=torch.Generator().manual_seed(i))
    st.run(x.cuda(), y.cuda(), torch.tensor(de, dtype=torch.int32).cuda(), alpha.cuda(), i % 2 == 0)     # the paired flag alternates: two plans
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode,kind,K", [("eager", "RMSprop", 4), ("planned", "RMSprop", 4), ("eager", "Adam", 2)], ids=["eager", "planned", "adam"])
def test_ema_follows_every_iteration(mode, kind, K):
    """The average after K iterations equals the host recurrence over exactly the K parameter snapshots, starting from the initial
    weights: one update per iteration, none from the warm-up passes of the two recordings.  Bar: K 2^-23 |host| + 1e-30 — at most one ulp
    per step (tests/ema_double.py), an earlier step's error carried with the factor decay < 1."""
    planned = mode == "planned"
    st, avg = _stepper(planned, kind)
    assert (st.planned is not None and st.planned.enabled) == planned
    flat = st.T.store.flat
    ptr = flat.data_ptr()
    host = flat.cpu().numpy().copy()
    assert np.array_equal(avg.buf.cpu().numpy().view(np.int32), host.view(np.int32))      # starts as a copy of the weights
    snaps = []
    for i in range(K):
        _iterate(st, i)
        snaps.append(flat.cpu().numpy().copy())
        assert flat.data_ptr() == ptr
    for s in snaps:
        host = ema_step(host, s, 0.5)
    got = avg.buf.cpu().numpy().astype(np.float64)
    bar = K * 2.0 ** -23 * np.abs(host.astype(np.float64)) + 1e-30
    err = np.abs(got - host)
    print(f"{mode} {kind}: worst error / bar {float(np.max(err / bar)):.3f}")
    assert np.all(err <= bar), float(np.max(err / bar))
    assert avg.updates == K
    for s in (snaps[0], snaps[-1]):                                                       # not vacuous: the average is neither end
        assert np.any(np.abs(got - s) > 1000 * bar)
    if planned:
        with_avg = sorted(e["plan"].n_launches for e in st.planned.cache.values())
        assert len(with_avg) == 2
        st0, _ = _stepper(True, kind, with_avg=False)
        for i in range(2):
            _iterate(st0, i)
        without = sorted(e["plan"].n_launches for e in st0.planned.cache.values())
        assert with_avg == [v + 1 for v in without], (with_avg, without)


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_applied_swaps_and_restores(prec):
    from rcot_amd import lib
    from rcot_amd.net_restormer import T_net
    from rcot_amd.ops import default_backend
    be = default_backend()
    prec0 = be.prec
    be.prec = {"fp32": lib.PREC_FP32, "bf16x3": lib.PREC_BF16X3}[prec]                     # in bf16x3 the packs go through repack()
    try:
        st, avg = _stepper(True)
        flat = st.T.store.flat
        ptr = flat.data_ptr()
        for i in range(2):
            _iterate(st, i)
        x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(9)).cuda()
        y1, y2 = st.T(x).clone(), st.T(x).clone()
        d0 = float((y1 - y2).abs().max())                                                 # two forwards of one network on this input
        raw = flat.clone()
        assert not torch.equal(raw, avg.buf)
        with avg.applied():
            assert torch.equal(_bits(flat), _bits(avg.buf)) and flat.data_ptr() == ptr
            ya = st.T(x).clone()
        assert torch.equal(_bits(flat), _bits(raw)) and flat.data_ptr() == ptr
        fresh = T_net(decoder=True)
        fresh.load_state_dict(avg.state_dict()["params"])
        yf = fresh(x)
        if d0 == 0.0:
            assert torch.equal(ya, yf)
        else:
            assert float((ya - yf).abs().max()) <= 4 * d0, (float((ya - yf).abs().max()), d0)
        assert float((ya - y1).abs().max()) > 0                                           # the averaged weights were the ones computing
        y3 = st.T(x)                                                                      # the raw weights AND their packs are back
        assert torch.equal(y3, y1) if d0 == 0.0 else float((y3 - y1).abs().max()) <= 4 * d0
        with pytest.raises(ZeroDivisionError):
            with avg.applied():
                1 / 0
        assert torch.equal(_bits(flat), _bits(raw)) and flat.data_ptr() == ptr
        _iterate(st, 2)                                                                   # one more planned iteration (a replay)
        step = (flat - raw)
        assert bool(torch.isfinite(step).all()) and float(step.abs().max()) > 0
        assert avg.updates == 3
    finally:
        be.prec = prec0


def test_average_of_the_mprnet_backbone_keeps_its_state_dict_names():
    """MPRNetHip lists its shared PReLU slope 22 times in state_dict() and stores it once: the average's tensors carry the same 127
    names and shapes, and a second network loaded from them holds the averaged buffer"""
    from rcot_amd.ema import WeightAverage
    from rcot_amd.mprnet_hip import MPRNetHip
    net = MPRNetHip(seed=1)
    avg = WeightAverage(net, 0.5)
    w0 = net.store.flat.cpu().numpy().copy()
    net.store.flat.mul_(1.25)
    avg.update()
    torch.cuda.synchronize()
    want = ema_step(w0, net.store.flat.cpu().numpy(), 0.5)
    assert np.all(np.abs(avg.buf.cpu().numpy().astype(np.float64) - want) <= ulp(want))
    sd, t = net.state_dict(), avg.tensors()
    assert list(t) == list(sd) and all(tuple(t[k].shape) == tuple(sd[k].shape) for k in sd)
    other = MPRNetHip(seed=2)
    other.load_state_dict(t)
    assert torch.equal(other.store.flat, avg.buf)
    again = WeightAverage(other, 0.5)
    again.load_state_dict(t)
    assert torch.equal(again.buf, avg.buf)


# ------------------------------------------------------------------------------- CLIs (subprocesses in a temporary working directory)
def _py(args, cwd, ok=True):
    r = subprocess.run([sys.executable, "-m"] + args, capture_output=True, text=True, timeout=900, cwd=cwd, env=dict(os.environ, PYTHONPATH=ROOT))
    if ok:
        assert r.returncode == 0, r.stderr[-3000:]
    return r


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory):
    """one training run with --ema 0.9 (2 epochs of 3 iterations) and its continuation at --lr 0 (1 epoch), shared by the CLI tests"""
    from rcot_amd.compat import load_checkpoint
    from synth_folders import write_png
    tmp = str(tmp_path_factory.mktemp("ema_cli"))
    g = np.random.Generator(np.random.PCG64(3))
    for i in range(2):
        t = np.clip(128 + 60 * np.sin(np.linspace(0, 4 + i, 32))[:, None, None] + g.normal(0, 4, (32, 32, 3)), 0, 255).astype(np.uint8)
        write_png(f"{tmp}/val/target/{i}.png", t)
        write_png(f"{tmp}/val/input/{i}.png", np.clip(t + g.normal(0, 15, t.shape), 0, 255).astype(np.uint8))
    base = ["rcot_amd.trainer", "--synthetic", "--iters", "3", "--batchSize", "2", "--patch_size", "64", "--de_type", "denoise_15", "--seed", "5",
            "--type", "EmaTest", "--sigma", "1", "--degset", f"{tmp}/val/input/", "--tarset", f"{tmp}/val/target/"]
    _py(base + ["--nEpochs", "2", "--ema", "0.9"], tmp)
    ck1_path = os.path.join(tmp, "checkpoint", "model_EmaTest__2_1.0.pth")
    ck1 = load_checkpoint(ck1_path)
    lines1 = open(os.path.join(tmp, "checksample", "EmaTest", "validation_results.txt")).read().splitlines()
    _py(base + ["--nEpochs", "3", "--lr", "0", "--ema", "0.9", "--val_weights", "both", "--resume", ck1_path], tmp)
    ck2 = load_checkpoint(os.path.join(tmp, "checkpoint", "model_EmaTest__3_1.0.pth"))
    lines2 = open(os.path.join(tmp, "checksample", "EmaTest", "validation_results.txt")).read().splitlines()[len(lines1):]
    return dict(tmp=tmp, ck1_path=ck1_path, ck1=ck1, ck2=ck2, lines1=lines1, lines2=lines2)


def test_trainer_cli_saves_the_average(cli_run):
    ck = cli_run["ck1"]
    raw = ck["Tnet"].state_dict()
    assert list(ck["Tnet_ema"]) == list(raw) == [n for n, _ in P.tnet_param_shapes()]
    assert all(tuple(ck["Tnet_ema"][k].shape) == tuple(raw[k].shape) and ck["Tnet_ema"][k].device.type == "cpu" for k in raw)
    assert ck["ema"] == {"decay": 0.9, "updates": 6}
    assert any(not torch.equal(ck["Tnet_ema"][k], raw[k]) for k in raw)
    assert {"epoch", "Tnet", "Fnet", "T_optimizer", "F_optimizer"} <= set(ck) and ck["epoch"] == 2
    assert len(cli_run["lines1"]) == 2 and all(ln.endswith(", weights ema0.9") for ln in cli_run["lines1"]), cli_run["lines1"]


def test_trainer_cli_resume_continues_the_average(cli_run):
    """--lr 0 leaves the parameters bit for bit unchanged, so the new average is three host-restatement updates of the old one towards
    the old "Tnet" (bar 3 2^-23 |.|: one ulp per update); a re-initialised average would equal "Tnet" instead."""
    ck1, ck2 = cli_run["ck1"], cli_run["ck2"]
    raw1, raw2 = ck1["Tnet"].state_dict(), ck2["Tnet"].state_dict()
    assert ck2["ema"] == {"decay": 0.9, "updates": 9} and ck2["epoch"] == 3
    differs = False
    for k in raw1:
        assert torch.equal(raw1[k].view(torch.int32), raw2[k].view(torch.int32)), k
        w, h = raw1[k].numpy(), ck1["Tnet_ema"][k].numpy()
        for _ in range(3):
            h = ema_step(h, w, 0.9)
        got = ck2["Tnet_ema"][k].numpy().astype(np.float64)
        assert np.all(np.abs(got - h) <= 3 * 2.0 ** -23 * np.abs(h.astype(np.float64))), k
        differs = differs or not np.array_equal(got, w.astype(np.float64))
    assert differs
    (line,) = cli_run["lines2"]
    assert line.endswith(", weights ema0.9"), line
    fields = dict(f.strip().split(" ")[-2:] for f in line.split(",") if "psnr" in f)
    assert set(fields) == {"psnr", "psnr_raw"} and all(math.isfinite(float(v)) for v in fields.values()), line


def test_tester_cli_weights_and_export(cli_run):
    from rcot_amd.compat import load_checkpoint
    tmp, ck1_path = cli_run["tmp"], cli_run["ck1_path"]
    data = ["--degset", f"{tmp}/val/input/", "--tarset", f"{tmp}/val/target/"]

    def tester(model, tag, extra=(), ok=True):
        r = _py(["rcot_amd.tester", "--model", model, *data, "--save", f"{tmp}/{tag}/OUT/", "--savetar", f"{tmp}/{tag}/TAR/", "--saveres",
                 f"{tmp}/{tag}/RES/", *extra], tmp, ok)
        return r, [open(f"{tmp}/{tag}/OUT/{i}.png", "rb").read() for i in range(2)] if ok else None

    _, out_ema = tester(ck1_path, "t_ema", ["--weights", "ema"])
    _, out_raw = tester(ck1_path, "t_raw", ["--weights", "raw"])
    assert out_ema != out_raw
    # a checkpoint without an average
    plain = {k: v for k, v in cli_run["ck1"].items() if k not in ("Tnet_ema", "ema")}
    plain_path = os.path.join(tmp, "plain.pth")
    torch.save(plain, plain_path)
    r, _ = tester(plain_path, "t_none", ["--weights", "ema"], ok=False)
    assert r.returncode != 0 and "Tnet_ema" in r.stderr, r.stderr[-2000:]
    # export: the average as the "Tnet" of a reference-format checkpoint
    exp_path = os.path.join(tmp, "exported.pth")
    _py(["rcot_amd.ema", "--in", ck1_path, "--out", exp_path], tmp)
    ex = load_checkpoint(exp_path)
    assert "Tnet_ema" not in ex and "ema" not in ex and "T_optimizer" not in ex and "F_optimizer" not in ex
    assert type(ex["Tnet"]).__module__ == "Net_Restormer" and type(ex["Tnet"]).__name__ == "T_net"
    sd = ex["Tnet"].state_dict()
    assert list(sd) == list(cli_run["ck1"]["Tnet_ema"]) and all(torch.equal(sd[k], cli_run["ck1"]["Tnet_ema"][k]) for k in sd)
    _, out_exp = tester(exp_path, "t_exp")                                                # default flags
    assert len(out_exp) == 2 and out_exp != out_raw
