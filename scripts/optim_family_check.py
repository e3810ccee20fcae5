"""The optimizer step entry points of two builds of librcot_hip.so on ONE box: the same bits, and the same speed?

    python scripts/optim_family_check.py bits  build_variants/parent/rcot_amd/librcot_hip.so
    python scripts/optim_family_check.py speed build_variants/parent/rcot_amd/librcot_hip.so [--launches 200] [--runs 3]

bits:  two child processes per library (RCOT_LIB), each running every step entry point for three steps at n = 4 (one float4), 4004 (a
       ragged last workgroup) and 4 194 308 (one float4 past the 4096 x 256 grid) on seeded inputs whose gradient begins with zeros, and
       printing a sha256 of every buffer and control block.  None of these kernels uses atomics: every digest must agree in all four dumps.
speed: plain RMSprop, guarded RMSprop and guarded AdamW at the n_total of T_net and of F_net(128): device events around --launches
       back-to-back launches after a warm-up, rotating over six buffer sets (the Infinity Cache holds none of them), one child process per
       run, the two libraries alternately.  Accepted when this library's median is not above the other's by more than the other's own
       max - min, and that spread is below 5 % of its median (else: lengthen the window and repeat).
Every child has a time limit; the first one that fails ends the script.  Both modes print a table (profiles/optim_one_family.txt).
"""
import argparse
import hashlib
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (4, 4004, 4096 * 256 * 4 + 4)
STEPS = 3
ROT = 6


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def dump():
    """child of `bits`: {case: digest} as one JSON line"""
    import torch
    from rcot_amd import lib
    from rcot_amd.ops import default_backend
    be, out = default_backend(), {}
    dev = be.device
    for n in SIZES:
        gen = torch.Generator().manual_seed(1234 + n)
        p0 = torch.randn(n, generator=gen)
        grads = []
        for _ in range(STEPS):
            g = torch.randn(n, generator=gen)
            g[:max(1, n // 4)] = 0.0                                   # leading zeros: sqrt(0) + eps in the denominators
            grads.append(g.to(dev))

        def fresh(k):
            return [p0.to(dev)] + [torch.zeros(n, device=dev) for _ in range(k)]

        def note(name, bufs, ctrl=None):
            torch.cuda.synchronize()
            for tag, t in zip(("p", "s0", "s1"), bufs):
                out[f"{name} n={n} {tag}"] = _sha(t)
            if ctrl is not None:
                out[f"{name} n={n} ctrl"] = _sha(ctrl)

        for gs in (1.0, 0.5):
            b = fresh(1)
            for g in grads:
                be.rmsprop_step(b[0], g, b[1], n, 1e-3, grad_scale=gs)
            note(f"rmsprop gscale={gs}", b)
            b = fresh(2)
            for t, g in enumerate(grads):
                be.adam_step(b[0], g, b[1], b[2], n, 1e-3, t + 1, grad_scale=gs)
            note(f"adam gscale={gs}", b)
            for wd in (0.0, 1e-2):
                b = fresh(2)
                for t, g in enumerate(grads):
                    be.adamw_step(b[0], g, b[1], b[2], n, 1e-3, t + 1, wd, grad_scale=gs)
                note(f"adamw wd={wd} gscale={gs}", b)

        # the guarded steps behind rcot_grad_sumsq + rcot_grad_decide: a cap that clips, no cap, a NaN gradient in the second step, and
        # (Adam family) a range that follows counter 1 while the decisions advance counter 0 only: its launches do nothing
        rules = {"rmsprop": (1, lambda b, g, c, k: be.rmsprop_step_guarded(b[0], g, b[1], n, c)),
                 "adam": (2, lambda b, g, c, k: be.adam_step_guarded(b[0], g, b[1], b[2], n, c, k)),
                 "adamw wd=0.0": (2, lambda b, g, c, k: be.adamw_step_guarded(b[0], g, b[1], b[2], n, c, k, 0.0)),
                 "adamw wd=0.01": (2, lambda b, g, c, k: be.adamw_step_guarded(b[0], g, b[1], b[2], n, c, k, 1e-2))}
        for rule, (nstate, step) in rules.items():
            for scen in ("clips", "no cap", "nan", "counter 1"):
                if scen == "counter 1" and nstate == 1:
                    continue
                b = fresh(nstate)
                ctrl = torch.zeros(lib.CB_WORDS, dtype=torch.float64, device=dev)
                partials = torch.zeros(lib.SUMSQ_MAX_PARTS, dtype=torch.float64, device=dev)
                ctrl[lib.CB_LR], ctrl[lib.CB_MAX_NORM] = 1e-3, (1e-2 if scen == "clips" else math.inf)
                for t, g in enumerate(grads):
                    if scen == "nan" and t == 1:
                        g = g.clone()
                        g[n - 1] = float("nan")
                    parts = be.grad_sumsq(g, n, partials)
                    be.grad_decide(partials, parts, ctrl, adam_mask=1 if nstate == 2 else 0)
                    step(b, g, ctrl, 1 if scen == "counter 1" else 0)
                note(f"guarded {rule}, {scen}", b, ctrl)
    print(json.dumps(out))


def timed(launches):
    """child of `speed`: {row: us per launch} as one JSON line"""
    import torch
    from rcot_amd import lib
    from rcot_amd import params as P
    from rcot_amd.net_restormer import _fnet_live_order, _tnet_live_order
    from rcot_amd.ops import default_backend
    be, out = default_backend(), {}
    shapes, fshapes = P.tnet_param_shapes(), P.fnet_param_shapes(128)
    sizes = {"T_net": P.make_layout(shapes, _tnet_live_order(), [k for k, _ in shapes if P.tnet_is_dead(k)]).n_total,
             "F_net(128)": P.make_layout(fshapes, _fnet_live_order(128), []).n_total}
    for name, n in sizes.items():
        sets = [[torch.rand(n, device=be.device) for _ in range(4)] for _ in range(ROT)]          # p, g, two state buffers
        ctrl = torch.zeros(lib.CB_WORDS, dtype=torch.float64, device=be.device)
        partials = torch.zeros(lib.SUMSQ_MAX_PARTS, dtype=torch.float64, device=be.device)
        ctrl[lib.CB_LR], ctrl[lib.CB_MAX_NORM] = 1e-6, math.inf
        be.grad_decide(partials, be.grad_sumsq(sets[0][1], n, partials), ctrl, adam_mask=1)         # scale 1, counter 0 at 1: the steps are taken
        runs = {"rcot_rmsprop_step": lambda b: be.rmsprop_step(b[0], b[1], b[2], n, 1e-6),
                "rcot_rmsprop_step_guarded": lambda b: be.rmsprop_step_guarded(b[0], b[1], b[2], n, ctrl),
                "rcot_adamw_step_guarded": lambda b: be.adamw_step_guarded(b[0], b[1], b[2], b[3], n, ctrl, 0, 1e-2)}
        for row, fn in runs.items():
            for i in range(2 * ROT):
                fn(sets[i % ROT])
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for i in range(launches):
                fn(sets[i % ROT])
            e.record()
            torch.cuda.synchronize()
            out[f"{row}, {name} n={n}"] = s.elapsed_time(e) / launches * 1e3
    print(json.dumps(out))


def _child(mode, libpath, limit, *extra):
    env = dict(os.environ, PYTHONPATH=ROOT)
    if libpath:
        env["RCOT_LIB"] = os.path.abspath(libpath)
    else:
        env.pop("RCOT_LIB", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, *extra], cwd=ROOT, env=env, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        print(r.stderr[-2000:])
        raise SystemExit(f"{mode} with {libpath or 'this library'} failed with {r.returncode}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("bits", "speed", "dump", "timed"))
    ap.add_argument("other", nargs="?", help="the other build's librcot_hip.so")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    o = ap.parse_args()
    if o.mode == "dump":
        return dump()
    if o.mode == "timed":
        return timed(o.launches)
    if not o.other:
        ap.error("the other build's library is needed")
    ok = True
    if o.mode == "bits":
        dumps = [_child("dump", lp, o.limit) for lp in (o.other, o.other, None, None)]
        print(f"# sha256 (first 16 hex digits) of every buffer and control block after {STEPS} steps; dumps: other0, other1, this0, this1; other = {o.other}")
        for k in sorted(dumps[0]):
            same = all(d.get(k) == dumps[0][k] for d in dumps)
            ok &= same
            print(f"{k:>48}: " + (f"bit-equal in all four dumps  {dumps[0][k]}" if same else "DIFFERS  " + " ".join(str(d.get(k)) for d in dumps)))
        ok &= all(set(d) == set(dumps[0]) for d in dumps)
    else:
        t = {"other": [], "this": []}
        for _ in range(o.runs):
            for tag, lp in (("other", o.other), ("this", None)):
                t[tag].append(_child("timed", lp, o.limit, "--launches", str(o.launches)))
        print(f"# us per launch, {o.launches} back-to-back launches over {ROT} buffer sets in turn, {o.runs} processes per library, alternating; other = {o.other}")
        for k in t["other"][0]:
            a, b = sorted(r[k] for r in t["other"]), sorted(r[k] for r in t["this"])
            ma, mb, spread = a[len(a) // 2], b[len(b) // 2], a[-1] - a[0]
            verdict = "ok" if mb <= ma + spread and spread <= 0.05 * ma else ("SPREAD ABOVE 5 %: lengthen the window" if spread > 0.05 * ma else "SLOWER")
            ok &= verdict == "ok"
            print(f"{k:>48}: other {' '.join(f'{v:8.2f}' for v in a)} (median {ma:.2f}, max - min {spread:.2f})  this {' '.join(f'{v:8.2f}' for v in b)} "
                  f"(median {mb:.2f}, {100 * (mb - ma) / ma:+.2f} %)  {verdict}")
    print("# ALL OK" if ok else "# NOT OK")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
