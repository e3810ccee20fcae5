"""GPU tier: the L1-spectrum OT cost (rcot_ot_spectrum) at sizes that are not powers of two — the mixed-radix Stockham line FFT
(prime factors <= 13) and Bluestein's algorithm (every other length <= 1024) — from the kernels up to the CLI.

  a. kernels vs the fp64 restatement (tests/host_double.py: torch.fft in fp64), bars of test_kernels_gpu.py::test_ot_cost;
  b. kernels vs the oracle in fp64 and vs the fixture otcost_sizes.npz (scripts/make_otcost_sizes_fixture.py), bars of
     test_kernels_gpu.py::test_ot_cost_golden;
  c. which kernel family the dispatcher chose (rcot_last_kernel);
  d. one real minimax iteration at P = 96 / 160 against the same schedule on the fp64 double with identical seeded parameters
     (the CPU tier holds that schedule to the oracle), bars of test_iteration_grads_gpu.py;
  e. the trainer CLI at --patch_size 96, and its refusal of --patch_size 40.
"""
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from conftest import ROOT, relerr, seeded_tensor
from host_double import TorchDouble
from test_iteration_grads_gpu import _compare, _np_params, _snapshot

pytestmark = pytest.mark.gpu

DBL = TorchDouble(torch.float64)


@pytest.fixture(scope="module")
def hip():
    from rcot_amd.ops import HipBackend
    return HipBackend()


def T(seed, *shape, scale=1.0):
    return seeded_tensor(seed, shape, scale=scale)


def _last_kernel(be):
    buf = ctypes.create_string_buffer(192)
    be.L.rcot_last_kernel(buf, 192)
    return buf.value.decode()


# ----------------------------------------------------------------------------- a. kernels vs fp64
SIZES = [(96, 96), (160, 160), (224, 224), (96, 160), (352, 352), (136, 200), (6, 10), (1000, 24), (544, 544), (992, 96),
         (2, 8), (8, 2), (64, 16)]      # radix-2 lines where a workgroup's four lines run past the image, or are few


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("paired", [False, True])
def test_ot_cost_sizes(hip, H, W, paired):
    """test_ot_cost's construction (B = 4, de = [0, 2, 3, 7], one exactly-zero plane, one constant plane) at H x W."""
    B = 4
    de = [0, 2, 3, 7]

    def fn(be, deg, out, tgt, dout, sums, spec, scal, gF):
        d = torch.tensor(de, dtype=torch.int32, device=deg.device)
        be.ot_reduce(deg, out, tgt if paired else None, sums)
        be.ot_spectrum(deg, out, d, gF, spec)
        be.ot_grad(deg, out, tgt if paired else None, d, gF, sums, spec, dout, scal, 1.0, 10000.0, B)
    deg, out = T(1, B, 3, H, W, scale=0.3), T(2, B, 3, H, W, scale=0.3)
    out[2, 0] = deg[2, 0]               # a plane with an exactly-zero spectrum
    out[3, 1] = deg[3, 1] - 0.25        # constant residual: one non-zero bin
    arrs = [deg, out, T(3, B, 3, H, W, scale=0.3), T(4, B, 3, H, W, scale=0.01), torch.zeros(2 * B + 2), torch.zeros(B),
            torch.zeros(3), torch.zeros(B, 3, H, W)]
    cpu = [a.double().clone() for a in arrs]
    gpu = [a.cuda() for a in arrs]
    fn(DBL, *cpu)
    fn(hip, *gpu)
    torch.cuda.synchronize()
    m = torch.ones(B, 3, 1, 1)          # the |F| = 0 / single-bin planes are degenerate for F/|F| in fp32, as in test_ot_cost
    m[2, 0] = 0
    m[3, 1] = 0
    e = dict(sums=relerr(gpu[4], cpu[4]), scal=relerr(gpu[6], cpu[6]), spec=relerr(gpu[5][2:], cpu[5][2:]),
             dout=relerr(gpu[3].cpu() * m, cpu[3] * m), gF=relerr(gpu[7][2:].cpu() * m[2:], cpu[7][2:] * m[2:]))
    print(f"[ot sizes {H}x{W} paired={paired}] " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()) + f" ({_last_kernel(hip)})")
    assert e["sums"] < 1e-5 and e["scal"] < 1e-5
    assert e["spec"] < 1e-5
    assert e["dout"] < 5e-5


def test_ot_spectrum_rejects_lengths_above_1024(hip):
    from rcot_amd.lib import RcotKernelError
    B, H, W = 1, 8, 1056
    deg, out = torch.zeros(B, 3, H, W).cuda(), torch.zeros(B, 3, H, W).cuda()
    de = torch.tensor([3], dtype=torch.int32).cuda()
    with pytest.raises(RcotKernelError) as e:
        hip.ot_spectrum(deg, out, de, hip.empty(B, 3, H, W), hip.empty(B))
    assert "1056" in str(e.value) and "1024" in str(e.value) and "H = 8" in str(e.value)


def test_ot_spectrum_workspace_rule():
    """B*3*H*W complex values, plus M per Bluestein axis: one byte short is RCOT_EWORKSPACE, nothing launched."""
    from rcot_amd.ops import HipBackend
    be = HipBackend(workspace_bytes=4 << 20)
    B, H, W = 1, 34, 64                                        # 34 = 2 * 17: Bluestein columns over M = 128, radix-2 rows
    need = 8 * (B * 3 * H * W + 128)
    deg, out = torch.rand(B, 3, H, W).cuda(), torch.rand(B, 3, H, W).cuda()
    de = torch.tensor([3], dtype=torch.int32).cuda()
    gF, spec = be.empty(B, 3, H, W), be.empty(B)
    args = (deg.data_ptr(), out.data_ptr(), de.data_ptr(), gF.data_ptr(), spec.data_ptr(), be.ws.data_ptr())
    assert be.L.rcot_ot_spectrum(*args, need - 8, B, H, W, be._st()) == -2
    assert be.L.rcot_ot_spectrum(*args, 8 * B * 3 * H * W, B, H, W, be._st()) == -2
    assert be.L.rcot_ot_spectrum(*args, need, B, H, W, be._st()) == 0
    torch.cuda.synchronize()
    ref_g, ref_s = torch.zeros(B, 3, H, W, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    DBL.ot_spectrum(deg.cpu().double(), out.cpu().double(), de.cpu(), ref_g, ref_s)
    assert relerr(spec, ref_s) < 1e-5 and relerr(gF, ref_g) < 5e-5


# ----------------------------------------------------------------------------- b. oracle and fixture
def _run_cost(hip, res, de):
    B = res.shape[0]
    deg, out = res.clone(), torch.zeros_like(res)
    sums, spec, scal, gF, dout = hip.empty(2 * B + 2), hip.empty(B), hip.empty(3), hip.empty(*res.shape), hip.zeros(*res.shape)
    hip.ot_reduce(deg, out, None, sums)
    hip.ot_spectrum(deg, out, de, gF, spec)
    hip.ot_grad(deg, out, None, de, gF, sums, spec, dout, scal, 1.0, 0.0, B)
    torch.cuda.synchronize()
    return scal.cpu().double(), dout.cpu()


@pytest.mark.parametrize("H,W", [(96, 96), (24, 40)])
def test_ot_cost_sizes_oracle_and_fixture(hip, gold, H, W):
    """The pinned oracle in fp64 with autograd, and the trainer's inline expression as recorded in otcost_sizes.npz."""
    from oracle import rcot_oracle as O
    fx = gold("otcost_sizes.npz")
    t = f"_{H}x{W}"
    res = torch.from_numpy(fx["res" + t])
    B = res.shape[0]
    de_host = [int(v) for v in fx["de_id" + t]]
    s, dout = _run_cost(hip, res.cuda(), torch.tensor(de_host, dtype=torch.int32).cuda())
    m = torch.ones(B, 3, 1, 1)          # d/d(out) = -d/d(res); degenerate planes (zero / constant) excluded as in test_ot_cost_golden
    m[1, 0] = 0
    m[3, 1] = 0
    ro = res.double().clone().requires_grad_(True)
    rm, fo = O.ot_cost(ro, torch.zeros_like(ro), de_host)
    (rm + fo).backward()
    eo = (abs(float(s[0]) - float(rm)) / float(rm), abs(float(s[1]) - float(fo)) / float(fo), relerr(-dout * m, ro.grad * m))
    ef = (abs(float(s[0]) - float(fx["rmse" + t])) / float(fx["rmse" + t]),
          abs(float(s[1]) - float(fx["per_sample" + t].sum())) / float(fx["per_sample" + t].sum()),
          relerr(-dout * m, torch.from_numpy(fx["dres" + t]) * m))
    print(f"[ot golden {H}x{W}] vs oracle fp64: rmse {eo[0]:.2e} fourier {eo[1]:.2e} dres {eo[2]:.2e}; "
          f"vs fixture: rmse {ef[0]:.2e} fourier {ef[1]:.2e} dres {ef[2]:.2e}")
    for e in (eo, ef):
        assert e[0] < 1e-5 and e[1] < 1e-5
        assert e[2] < 5e-5


# ----------------------------------------------------------------------------- c. dispatch
@pytest.mark.parametrize("H,W,symbol", [(128, 128, "ot_rows_inv_kernel"), (96, 96, "ot_rows_inv_mixed_kernel"),
                                        (544, 544, "ot_rows_inv_bluestein_kernel"), (96, 128, "ot_rows_inv_kernel"),
                                        (128, 96, "ot_rows_inv_mixed_kernel"), (64, 16, "ot_rows_inv_kernel")])
def test_dispatch_by_length(hip, H, W, symbol):
    """The rows passes follow W's plan, the columns pass H's: the last launch of a call is the inverse rows pass."""
    B = 1
    deg, out = T(5, B, 3, H, W).cuda(), T(6, B, 3, H, W).cuda()
    de = torch.tensor([4], dtype=torch.int32).cuda()
    gF, spec = hip.empty(B, 3, H, W), hip.empty(B)
    hip.ot_spectrum(deg, out, de, gF, spec)
    assert _last_kernel(hip) == symbol
    torch.cuda.synchronize()
    ref_g, ref_s = torch.zeros(B, 3, H, W, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    DBL.ot_spectrum(deg.cpu().double(), out.cpu().double(), de.cpu(), ref_g, ref_s)
    assert relerr(spec, ref_s) < 1e-5 and relerr(gF, ref_g) < 5e-5


def test_plan_replay_at_a_new_size():
    """The recorded launch plan (rcot_amd/plan.py) replays the spectrum kernels at 96 x 96: two planned iterations equal two eager
    ones up to the float atomics of spec."""
    from rcot_amd import params as P
    from rcot_amd.net_restormer import F_net, T_net
    from rcot_amd.ops import HipBackend
    from rcot_amd.synth import make_batch
    from rcot_amd.trainer import FlatOptimizer, MinimaxStep
    ps, B, de, lr = 96, 2, [3, 4], 1e-4
    _, deg, clean = make_batch(21, B, ps, de)
    alpha = seeded_tensor(22, (B,), lo=0.0, hi=1.0)
    outs = []
    for planned in (True, False):
        os.environ["RCOT_PLAN"] = "1" if planned else "0"
        try:
            be = HipBackend()
            Tn, Fn = T_net(decoder=True, backend=be), F_net(patch_size=ps, backend=be)
            Tn.load_state_dict(_np_params(P.tnet_param_shapes(), 31, "T"))
            Fn.load_state_dict(_np_params(P.fnet_param_shapes(ps), 32, "F"))
            st = MinimaxStep(Tn, Fn, FlatOptimizer(Tn, "RMSprop", lr / 2), FlatOptimizer(Fn, "RMSprop", lr), 1.0, 10000.0)
        finally:
            os.environ.pop("RCOT_PLAN", None)
        assert (st.planned is not None) == planned
        st.set_de_ids(de)
        a = (deg.cuda(), clean.cuda(), torch.tensor(de, dtype=torch.int32).cuda(), alpha.cuda(), True)
        for _ in range(2):
            st.run(*a)
        torch.cuda.synchronize()
        outs.append(st.scalars())
        if planned:
            syms = [sym for e in st.planned.cache.values() for _, sym in e["plan"].symbols]
            assert "ot_rows_inv_mixed_kernel" in syms, sorted(set(syms))[:40]
    for k in outs[0]:      # (tolerances of tests/test_plan_gpu.py: float atomics, then one sign-like RMSprop step)
        assert abs(outs[0][k] - outs[1][k]) <= max(2e-4 * max(1e-3, abs(outs[1][k])), 5e-6), (k, outs)


# ----------------------------------------------------------------------------- d. one real iteration
_HOST = {}


def _host_iteration(ps, B, de, paired):
    """The same MinimaxStep on the fp64 double (CPU), once per configuration: losses and the T gradients after the generator loss."""
    key = (ps, B, tuple(de), paired)
    if key not in _HOST:
        from rcot_amd import params as P
        from rcot_amd.net_restormer import F_net, T_net
        from rcot_amd.trainer import FlatOptimizer, MinimaxStep
        t0 = time.time()
        D = torch.float64
        be = TorchDouble(D)
        Tn, Fn = T_net(decoder=True, backend=be, seed=0), F_net(patch_size=ps, backend=be, seed=1)
        Tn.load_state_dict({k: v.to(D) for k, v in _np_params(P.tnet_param_shapes(), 41, "T").items()})
        Fn.load_state_dict({k: v.to(D) for k, v in _np_params(P.fnet_param_shapes(ps), 42, "F").items()})
        deg, clean, alpha = _inputs(ps, B, de, paired)
        st = MinimaxStep(Tn, Fn, FlatOptimizer(Tn, "RMSprop", 0.5e-4), FlatOptimizer(Fn, "RMSprop", 1e-4), 1.0, 10000.0)
        st.set_de_ids(de)
        snaps = {}
        st.grad_probe = lambda where: snaps.__setitem__(where, _snapshot(Tn, 128)) if where == "T_gen" else None
        st.iteration(deg.to(D), clean.to(D), torch.tensor(de, dtype=torch.int32), alpha.to(D), paired)
        _HOST[key] = (st.scalars(), snaps["T_gen"])
        print(f"[host fp64 iteration P={ps} paired={paired}] {time.time() - t0:.1f} s")
    return _HOST[key]


def _inputs(ps, B, de, paired):
    from rcot_amd.synth import make_batch
    _, deg, clean = make_batch(43, B, ps, de, unpaired=not paired)
    return deg, clean, seeded_tensor(44, (B,), lo=0.0, hi=1.0)


@pytest.mark.parametrize("prec,tol", [("fp32", 2e-3), ("bf16x3", 1e-2)])
@pytest.mark.parametrize("ps,de,paired", [(96, [3, 4], True), (96, [3, 4], False), (160, [3, 5], False)])
def test_iteration_at_new_sizes(ps, de, paired, prec, tol):
    from rcot_amd import lib
    from rcot_amd import params as P
    from rcot_amd.net_restormer import F_net, T_net
    from rcot_amd.ops import HipBackend
    from rcot_amd.trainer import FlatOptimizer, MinimaxStep
    B = 2
    want, want_snap = _host_iteration(ps, B, de, paired)
    be = HipBackend()
    be.prec = {"fp32": lib.PREC_FP32, "bf16x3": lib.PREC_BF16X3}[prec]
    Tn, Fn = T_net(decoder=True, backend=be), F_net(patch_size=ps, backend=be)
    Tn.load_state_dict(_np_params(P.tnet_param_shapes(), 41, "T"))
    Fn.load_state_dict(_np_params(P.fnet_param_shapes(ps), 42, "F"))
    deg, clean, alpha = _inputs(ps, B, de, paired)
    st = MinimaxStep(Tn, Fn, FlatOptimizer(Tn, "RMSprop", 0.5e-4), FlatOptimizer(Fn, "RMSprop", 1e-4), 1.0, 10000.0)
    st.set_de_ids(de)
    snaps = {}
    st.grad_probe = lambda where: snaps.__setitem__(where, _snapshot(Tn, 128)) if where == "T_gen" else None
    st.iteration(deg.cuda(), clean.cuda(), torch.tensor(de, dtype=torch.int32).cuda(), alpha.cuda(), paired)
    torch.cuda.synchronize()
    s = st.scalars()
    print(f"[iteration P={ps} paired={paired} {prec}] hip {s} vs fp64 host {want}")
    ltol = {"Loss_F": 1e-3, "Loss_T": 5e-3, "Loss_mse": 1e-3, "gp": 1e-3}       # tests/test_iteration_grads_gpu.py
    for k in ltol:
        assert abs(s[k] - want[k]) <= ltol[k] * max(abs(want[k]), 1e-3), (k, s[k], want[k])
    names, shapes = [n for n, _ in P.tnet_param_shapes()], [sh for _, sh in P.tnet_param_shapes()]
    gn = np.array([w[0] for w in want_snap])
    gs = np.concatenate([w[1] for w in want_snap])
    worst = _compare(snaps["T_gen"], names, gn, gs, 128, shapes, tol, "T after generator loss")
    print(f"[iteration P={ps} paired={paired} {prec}] worst T gradient-norm rel err / (1 - cos): {worst[0]:.1e} / {worst[1]:.1e}")


# ----------------------------------------------------------------------------- e. CLI
def test_trainer_cli_patch_size_96(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "rcot_amd.trainer", "--synthetic", "--iters", "3", "--batchSize", "2", "--patch_size", "96",
           "--de_type", "derain", "dehaze", "--nEpochs", "1", "--seed", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=tmp_path, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "Loss_F" in r.stdout and "Checkpoint saved" in r.stdout
    cks = [f for f in os.listdir(os.path.join(tmp_path, "checkpoint")) if f.endswith(".pth")]
    assert len(cks) == 1, cks
    ck = os.path.join(tmp_path, "checkpoint", cks[0])
    from rcot_amd.tester import load_network
    net, mult = load_network(ck)
    y = net(torch.rand(1, 3, 96, 96).cuda())
    assert tuple(y.shape) == (1, 3, 96, 96) and bool(torch.isfinite(y).all())


def test_trainer_cli_refuses_patch_size_40(tmp_path):
    """check_patch_size speaks before the GPU is touched: no device is visible to the child, and the message is still the answer."""
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="")
    cmd = [sys.executable, "-m", "rcot_amd.trainer", "--synthetic", "--iters", "1", "--batchSize", "2", "--patch_size", "40",
           "--de_type", "derain", "--nEpochs", "1", "--seed", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=tmp_path, env=env)
    assert r.returncode != 0
    assert "--patch_size 40" in r.stderr and "multiple of 32" in r.stderr and "stride-2" in r.stderr
    assert not os.path.exists(os.path.join(tmp_path, "checkpoint"))
