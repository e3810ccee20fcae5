"""Per-iteration schedules held on the device (rcot_amd/schedule.py): what they cost.  Writes profiles/lr_schedule.txt (--out).

1. Kernel time of the advance launch (rcot_sched_advance, one workgroup), and of the two kernels that read a device word next to their
   by-value twins on buffers of T_net's size: rcot_ema_step_dev next to rcot_ema_step, rcot_adamw_step next to rcot_adam_step (and the
   guarded pair).  Device events around --launches back-to-back launches after a warm-up, --rounds rounds alternating all of them in
   one process.  Bytes per element and the rate are given as scripts/bench_clip.py gives them.
2. Iteration time of one MinimaxStep at B = 8, 128 x 128, fp32, RMSprop: both optimizers guarded with max_norm inf ("guard only"), next
   to the same plus a restarts schedule with warm-up and a weight average with EMA warm-up ("guard + schedule + EMA warm-up"), and, to
   tell the schedule from the average, guard only plus a constant-decay average.  Blocks of --iters replayed iterations, alternating the
   configurations in one process; the A/A spread is the range over the blocks of one configuration.  Numbers are reported, no
   difference is asserted.
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from rcot_amd import lib
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
    from rcot_amd import schedule
    p, g, m, v, ema = (torch.rand(n, device=be.device) for _ in range(5))
    partials = torch.zeros(lib.SUMSQ_MAX_PARTS, dtype=torch.float64, device=be.device)
    ctrl = torch.zeros(lib.CB_WORDS, dtype=torch.float64, device=be.device)
    ctrl2 = torch.zeros(lib.CB_WORDS, dtype=torch.float64, device=be.device)
    ctrl[lib.CB_MAX_NORM] = math.inf
    be.grad_decide(partials, be.grad_sumsq(g, n, partials), ctrl, 1)         # one taken decision: counter 0 and its bias corrections
    sched = schedule.Schedule(be, "restarts:1000,2000", 1e-4, 3000, 100, ema_decay=0.999)
    dT, dF = ctrl2[lib.CB_LR:lib.CB_LR + 1], ctrl[lib.CB_LR:lib.CB_LR + 1]
    word = sched.omd_word
    n4 = n // 4 * 4
    runs = {"rcot_sched_advance": (lambda: be.sched_advance(sched.block, sched.table_dev, dT, 0.5, dF, 1.0), 0),
            "rcot_ema_step": (lambda: be.ema_step(ema, p, n, 0.999), 12),
            "rcot_ema_step_dev": (lambda: be.ema_step_dev(ema, p, n, word), 12),
            "rcot_adam_step": (lambda: be.adam_step(p, g, m, v, n4, 1e-6, 10), 28),
            "rcot_adamw_step": (lambda: be.adamw_step(p, g, m, v, n4, 1e-6, 10, 1e-4), 28),
            "rcot_adam_step_guarded": (lambda: be.adam_step_guarded(p, g, m, v, n4, ctrl, 0), 28),
            "rcot_adamw_step_guarded": (lambda: be.adamw_step_guarded(p, g, m, v, n4, ctrl, 0, 1e-4), 28)}
    for fn, _ in runs.values():
        _events(fn, 20)
    t = {k: [] for k in runs}
    for _ in range(rounds):
        for k, (fn, _) in runs.items():
            t[k].append(_events(fn, launches))
    say(f"kernel time, T_net: n = {n} elements ({4 * n / 1e6:.1f} MB per buffer), {launches} launches per window, {rounds} alternating rounds")
    for k, (_, per) in runs.items():
        s = sorted(t[k])
        med = s[len(s) // 2]
        line = f"  {k:26s}: median {med:7.2f} us  (min {s[0]:.2f}, max {s[-1]:.2f})"
        if per:
            rate = per * n / (med * 1e-6)
            line += f"  {per:2d} B/element  {rate / 1e9:7.0f} GB/s = {rate / PEAK:.2f} of 6.3 TB/s"
        say(line)


def iterations(iters, blocks, say):
    from rcot_amd import schedule
    from rcot_amd.ema import WeightAverage
    from rcot_amd.net_restormer import F_net, T_net
    from rcot_amd.synth import make_batch
    from rcot_amd.trainer import FlatOptimizer, MinimaxStep
    ps, B, lr, de = 128, 8, 1e-4, [2, 3, 2, 3, 2, 3, 2, 3]
    _, x, y = make_batch(11, B, ps, de)
    x, y, d, alpha = x.cuda(), y.cuda(), torch.tensor(de, dtype=torch.int32).cuda(), torch.full((B,), 0.5).cuda()
    steps = {}
    for name in ("guard only", "guard + EMA", "guard + schedule + EMA warm-up"):
        Tn, Fn = T_net(decoder=True, seed=1), F_net(patch_size=ps, seed=2)
        To, Fo = FlatOptimizer(Tn, "RMSprop", lr / 2, math.inf), FlatOptimizer(Fn, "RMSprop", lr, math.inf)
        avg = sched = None
        if name != "guard only":
            avg = WeightAverage(Tn, 0.999)
        if "schedule" in name:
            sched = schedule.Schedule(Tn.be, "restarts:400,800", lr, 1200, 20, ema_decay=0.999)
            sched.bind(To, Fo)
            avg.omd_word = sched.omd_word
        st = MinimaxStep(Tn, Fn, To, Fo, 1.0, 10000.0, ema=avg, schedule=sched)
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
    say(f"iteration time, MinimaxStep B = {B}, {ps} x {ps}, fp32, RMSprop, launch plans of {' / '.join(str(q) for q in n)} launches; blocks of {iters} "
        f"iterations, {blocks} alternating blocks each")
    med, spread = {}, {}
    for k, v in t.items():
        s = sorted(v)
        med[k], spread[k] = s[len(s) // 2], s[-1] - s[0]
        say(f"  {k:31s}: median {med[k]:.3f} ms per iteration  (blocks: {', '.join(f'{q:.3f}' for q in v)}; A/A spread {spread[k]:.3f} ms)")
    base = "guard only"
    for k in list(steps)[1:]:
        say(f"  {k} - {base}: {med[k] - med[base]:+.3f} ms per iteration (block-to-block spread of {base}: {spread[base]:.3f} ms)")
    st = steps["guard + schedule + EMA warm-up"]
    say(f"  schedule: t = {st.schedule.t}, rate now {st.schedule.rate():.3e}; T_net {st.To.guard_counters()['steps']} steps, "
        f"{st.To.guard_counters()['skipped']} skipped; the average has {st.ema.updates} updates")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lr_schedule.txt"))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    o = ap.parse_args()
    from rcot_amd.net_restormer import _tnet_live_order
    from rcot_amd.ops import default_backend
    shapes = P.tnet_param_shapes()
    nT = P.make_layout(shapes, _tnet_live_order(), [k for k, _ in shapes if P.tnet_is_dead(k)]).n_total
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("python scripts/bench_schedule.py on " + torch.cuda.get_device_name(0))
    kernels(default_backend(), nT, o.launches, o.rounds, say)
    if o.iters > 0:
        iterations(o.iters, o.blocks, say)
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
