"""Gradient-norm clipping and the non-finite step skip (FlatOptimizer(max_norm=...)): what the guard costs.  Writes profiles/grad_clip.txt (--out).

1. Kernel time of rcot_grad_sumsq (one buffer again and again, which the Infinity Cache holds, and six buffers in turn, which it does not) over gradient buffers of T_net's and F_net's (128 x 128 patches) n_live, next to a device-to-device copy of
   the same buffer in the same run: device events around --launches back-to-back launches after a warm-up, --rounds rounds alternating the
   two.  The sum reads 4 bytes per element, the copy moves 8; both are given in GB/s and the sum also as a multiple of the time its bytes take
   at the 6.3 TB/s a float4 copy reaches on this chip.  The decision launch (one workgroup) and the guarded step kernel are timed the same way.
2. Iteration time of one MinimaxStep at B = 8, 128 x 128, fp32, with both optimizers unguarded and both guarded (max_norm 0.01 / inf):
   blocks of --iters replayed iterations, alternating the two configurations in one process; the A/A spread is the range over blocks of one
   configuration.  The numbers are reported, no difference is asserted.
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from rcot_amd import lib
from rcot_amd import params as P

ROT = 6             # buffers walked in turn by the out-of-cache rows
PEAK = 6.3e12       # bytes/s of a float4 copy on the MI355X (measured; 8.0e12 is the specification)


def _events(fn, launches):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(launches):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / launches * 1e3          # us per launch


def kernels(be, name, n, launches, rounds, say):
    g, dst, p, sq = (torch.rand(n, device=be.device) for _ in range(4))
    partials = torch.zeros(lib.SUMSQ_MAX_PARTS, dtype=torch.float64, device=be.device)
    ctrl = torch.zeros(lib.CB_WORDS, dtype=torch.float64, device=be.device)
    ctrl[lib.CB_MAX_NORM] = 0.01
    parts = be.grad_sumsq(g, n, partials)
    # one buffer launched over and over stays in the 256 MiB Infinity Cache (178 MB for T_net): the "in turn" rows walk ROT buffers, a
    # footprint well past the cache, so every launch reads HBM.  In the iteration the gradients were written just before the sum reads them.
    rot, turn = [g] + [torch.rand(n, device=be.device) for _ in range(ROT - 1)], [0, 0]

    def sum_rot():
        turn[0] = (turn[0] + 1) % ROT
        be.grad_sumsq(rot[turn[0]], n, partials)

    def copy_rot():
        turn[1] = (turn[1] + 1) % ROT
        dst.copy_(rot[turn[1]])
    runs = {"rcot_grad_sumsq": (lambda: be.grad_sumsq(g, n, partials), 4), "copy (torch, d2d)": (lambda: dst.copy_(g), 8),
            f"rcot_grad_sumsq, {ROT} in turn": (sum_rot, 4), f"copy, {ROT} sources in turn": (copy_rot, 8),
            "rcot_grad_decide": (lambda: be.grad_decide(partials, parts, ctrl), 0),
            "rcot_rmsprop_step_guarded": (lambda: be.rmsprop_step_guarded(p, g, sq, n, ctrl), 20),
            "rcot_rmsprop_step": (lambda: be.rmsprop_step(p, g, sq, n, 0.0), 20)}
    for fn, _ in runs.values():
        _events(fn, 20)
    t = {k: [] for k in runs}
    for _ in range(rounds):
        for k, (fn, _) in runs.items():
            t[k].append(_events(fn, launches))
    say(f"kernel time, {name}: n = {n} elements ({4 * n / 1e6:.1f} MB per buffer, {parts} partials), {launches} launches per window, {rounds} alternating rounds")
    for k, (_, per) in runs.items():
        v = sorted(t[k])
        med = v[len(v) // 2]
        line = f"  {k:26s}: median {med:7.2f} us  (min {v[0]:.2f}, max {v[-1]:.2f})"
        if per:
            rate = per * n / (med * 1e-6)
            line += f"  {per:2d} B/element  {rate / 1e9:7.0f} GB/s = {rate / PEAK:.2f} of 6.3 TB/s = {med * 1e-6 / (per * n / PEAK):.2f} x the time of its bytes at 6.3 TB/s"
        say(line)


def iterations(iters, blocks, say):
    from rcot_amd.net_restormer import F_net, T_net
    from rcot_amd.synth import make_batch
    from rcot_amd.trainer import FlatOptimizer, MinimaxStep
    ps, B, lr, de = 128, 8, 1e-4, [2, 3, 2, 3, 2, 3, 2, 3]
    _, x, y = make_batch(11, B, ps, de)
    x, y, d, alpha = x.cuda(), y.cuda(), torch.tensor(de, dtype=torch.int32).cuda(), torch.full((B,), 0.5).cuda()
    steps = {}
    for name, (mT, mF) in (("unguarded", (None, None)), ("guarded", (0.01, math.inf))):
        Tn, Fn = T_net(decoder=True, seed=1), F_net(patch_size=ps, seed=2)
        st = MinimaxStep(Tn, Fn, FlatOptimizer(Tn, "RMSprop", lr / 2, mT), FlatOptimizer(Fn, "RMSprop", lr, mF), 1.0, 10000.0)
        st.set_de_ids(de)
        for _ in range(3):                              # the recording, then replays
            st.run(x, y, d, alpha, False)
        torch.cuda.synchronize()
        steps[name] = st
    t = {k: [] for k in steps}
    for _ in range(blocks):
        for k, st in steps.items():
            t[k].append(_events(lambda: st.run(x, y, d, alpha, False), iters) / 1e3)
    n = [next(iter(st.planned.cache.values()))["plan"].n_launches for st in steps.values()]
    say(f"iteration time, MinimaxStep B = {B}, {ps} x {ps}, fp32, launch plans of {n[0]} / {n[1]} launches; blocks of {iters} iterations, "
        f"{blocks} alternating blocks each")
    med = {}
    for k, v in t.items():
        s = sorted(v)
        med[k] = s[len(s) // 2]
        say(f"  {k:9s}: median {med[k]:.3f} ms per iteration  (blocks: {', '.join(f'{q:.3f}' for q in v)}; A/A spread {(s[-1] - s[0]):.3f} ms)")
    say(f"  guarded - unguarded: {med['guarded'] - med['unguarded']:+.3f} ms per iteration (three guarded steps: three more reads of a gradient buffer "
        "and six small launches)")
    for k in ("guarded",):
        for o, nm in ((steps[k].To, "T_net"), (steps[k].Fo, "F_net")):
            c = o.guard_counters()
            say(f"  {nm}: {c['steps']} steps, {c['clipped']} clipped, {c['skipped']} skipped, last norm {c['last_norm']:.4g}, largest {c['max_seen']:.4g}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "grad_clip.txt"))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    o = ap.parse_args()
    from rcot_amd.net_restormer import _fnet_live_order, _tnet_live_order
    from rcot_amd.ops import default_backend
    shapes = P.tnet_param_shapes()
    nT = P.make_layout(shapes, _tnet_live_order(), [k for k, _ in shapes if P.tnet_is_dead(k)]).n_live
    fshapes = P.fnet_param_shapes(128)
    nF = P.make_layout(fshapes, _fnet_live_order(128), []).n_live
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("scripts/bench_clip.py on " + torch.cuda.get_device_name(0))
    kernels(default_backend(), "T_net", nT, o.launches, o.rounds, say)
    kernels(default_backend(), "F_net (128 x 128)", nF, o.launches, o.rounds, say)
    if o.iters > 0:
        iterations(o.iters, o.blocks, say)
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
