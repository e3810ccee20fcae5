"""Weight averaging (rcot_amd/ema.py): what the update costs.  Writes profiles/ema_step.txt (--out).

1. Kernel time of rcot_ema_step next to rcot_rmsprop_step on buffers of T_net's n_total, in the same run: device events around
   --launches back-to-back launches after a warm-up, --rounds rounds alternating the two.  GB/s at 12 bytes per element (read ema, read p,
   write ema) resp. 20 (read p, g, sq; write p, sq), and both against the 6.3 TB/s a float4 copy reaches on this chip.  The yardstick is
   the existing optimizer kernel: the EMA kernel should reach 0.9 of its bytes per second; the spread of repeating one kernel is printed
   beside it.
2. Iteration time of one MinimaxStep at B = 8, 128 x 128, fp32, with and without the average: blocks of --iters replayed iterations,
   alternating the two configurations in one process; the A/A spread is the range over blocks of one configuration.  The expected cost is
   the kernel time plus one kernel boundary, far inside that spread: the numbers are reported, no difference is asserted.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from rcot_amd import params as P

PEAK = 6.3e12       # bytes/s of a float4 copy on the MI355X (measured; 8.0e12 is the specification)


def _events(fn, launches):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(launches):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / launches * 1e3          # us per launch


def kernels(be, n, launches, rounds, say):
    ema, p, g, sq = (torch.rand(n, device=be.device) for _ in range(4))
    runs = {"rcot_ema_step": (lambda: be.ema_step(ema, p, n, 0.999), 12), "rcot_rmsprop_step": (lambda: be.rmsprop_step(p, g, sq, n, 0.0), 20)}
    for fn, _ in runs.values():
        _events(fn, 20)
    t = {k: [] for k in runs}
    for _ in range(rounds):
        for k, (fn, _) in runs.items():
            t[k].append(_events(fn, launches))
    say(f"kernel time, n = {n} elements ({4 * n / 1e6:.1f} MB per buffer), {launches} launches per window, {rounds} alternating rounds")
    rate = {}
    for k, (_, per) in runs.items():
        v = sorted(t[k])
        med = v[len(v) // 2]
        rate[k] = per * n / (med * 1e-6)
        say(f"  {k:18s}: median {med:7.2f} us  (min {v[0]:.2f}, max {v[-1]:.2f}; spread {(v[-1] - v[0]) / med * 100:.1f} %)  "
            f"{per} B/element  {rate[k] / 1e9:7.0f} GB/s = {rate[k] / PEAK:.2f} of 6.3 TB/s")
    say(f"  bytes per second, rcot_ema_step over rcot_rmsprop_step: {rate['rcot_ema_step'] / rate['rcot_rmsprop_step']:.3f} (aim: at least 0.9)")


def iterations(iters, blocks, say):
    from rcot_amd.ema import WeightAverage
    from rcot_amd.net_restormer import F_net, T_net
    from rcot_amd.synth import make_batch
    from rcot_amd.trainer import FlatOptimizer, MinimaxStep
    ps, B, lr, de = 128, 8, 1e-4, [2, 3, 2, 3, 2, 3, 2, 3]
    _, x, y = make_batch(11, B, ps, de)
    x, y, d, alpha = x.cuda(), y.cuda(), torch.tensor(de, dtype=torch.int32).cuda(), torch.full((B,), 0.5).cuda()
    steps = {}
    for name in ("without", "with"):
        Tn, Fn = T_net(decoder=True, seed=1), F_net(patch_size=ps, seed=2)
        st = MinimaxStep(Tn, Fn, FlatOptimizer(Tn, "RMSprop", lr / 2), FlatOptimizer(Fn, "RMSprop", lr), 1.0, 10000.0,
                         ema=WeightAverage(Tn, 0.999) if name == "with" else None)
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
    for k, v in t.items():
        s = sorted(v)
        say(f"  {k:7s} the average: median {s[len(s) // 2]:.3f} ms per iteration  (blocks: {', '.join(f'{q:.3f}' for q in v)}; "
            f"A/A spread {(s[-1] - s[0]):.3f} ms)")
    say("  (expected cost of the average: its kernel time plus one kernel boundary of about 2 us; a difference inside the A/A spread is no finding)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ema_step.txt"))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    o = ap.parse_args()
    from rcot_amd.net_restormer import _tnet_live_order
    from rcot_amd.ops import default_backend
    shapes = P.tnet_param_shapes()
    n = P.make_layout(shapes, _tnet_live_order(), [k for k, _ in shapes if P.tnet_is_dead(k)]).n_total
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("scripts/bench_ema.py on " + torch.cuda.get_device_name(0))
    kernels(default_backend(), n, o.launches, o.rounds, say)
    if o.iters > 0:
        iterations(o.iters, o.blocks, say)
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
