"""(Re)generate tests/golden/lr_schedules.json: learning rates handed out by the REFERENCE's own scheduler classes
(util/schedulers.py, which its trainer.py never calls) on a dummy optimizer, one value per iteration.

    python scripts/make_schedule_fixture.py

Runs only where the reference checkout is present (the path oracle/pin_against_reference.py names); its modules are imported the way
that script imports them.  Only numbers are written: for every case the class name, its arguments, the matching --lr_schedule spec of
rcot_amd/schedule.py and the recorded rates (the optimizer's param_groups[0]["lr"] before each scheduler.step(), read as Python
floats: JSON's repr round-trips a double exactly).  Base rate 1e-4 throughout.

Before anything is written rcot_amd.schedule.table is held to the recording at 1e-12 relative, the bar of tests/test_schedule_cpu.py.
The chained LinearWarmupCosineAnnealingLR differs from its own closed form by rounding that accumulates: it is not a case.
"""
import json
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pin_against_reference as PIN   # noqa: E402
from rcot_amd import schedule as S                # noqa: E402

BASE = 1e-4
ITERS = 40
BAR = 1e-12


def record(make, iters):
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=BASE)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sched = make(opt)
        out = []
        for _ in range(iters):
            out.append(float(opt.param_groups[0]["lr"]))
            opt.step()
            sched.step()
    return out


def main():
    PIN._stub_modules()
    sys.path.insert(0, PIN.REF)
    from util import schedulers as R
    cases = [
        dict(name="CosineAnnealingRestartCyclicLR", args=dict(periods=[12, 28], restart_weights=[1, 1], eta_mins=[1e-4, 1e-6]), iters=ITERS,
             spec="restarts:12,28:1,1:1e-4,1e-6", warmup_iters=0,
             make=lambda o: R.CosineAnnealingRestartCyclicLR(o, periods=[12, 28], restart_weights=[1, 1], eta_mins=[1e-4, 1e-6])),
        dict(name="CosineAnnealingRestartLR", args=dict(periods=[10, 10, 20], restart_weights=[1, 0.5, 0.25], eta_min=1e-7), iters=ITERS,
             spec="restarts:10,10,20:1,0.5,0.25:1e-7", warmup_iters=0,
             make=lambda o: R.CosineAnnealingRestartLR(o, periods=[10, 10, 20], restart_weights=[1, 0.5, 0.25], eta_min=1e-7)),
        dict(name="LinearLR", args=dict(total_iter=ITERS), iters=ITERS, spec="linear", warmup_iters=0,
             make=lambda o: R.LinearLR(o, ITERS)),
        dict(name="MultiStepRestartLR", args=dict(milestones=[10, 20, 30], gamma=0.5), iters=ITERS, spec="multistep:10,20,30:0.5", warmup_iters=0,
             make=lambda o: R.MultiStepRestartLR(o, milestones=[10, 20, 30], gamma=0.5)),
        dict(name="LambdaLR(linear_warmup_decay)", args=dict(warmup_steps=5, total_steps=ITERS, cosine=True), iters=ITERS, spec="cosine", warmup_iters=5,
             make=lambda o: torch.optim.lr_scheduler.LambdaLR(o, R.linear_warmup_decay(5, ITERS, cosine=True))),
    ]
    out = {"base_lr": BASE, "cases": []}
    for c in cases:
        rates = record(c.pop("make"), c["iters"])
        mine = S.table(c["spec"], BASE, c["iters"], c["warmup_iters"])
        rel = max(abs(a - b) / max(abs(b), 1e-300) for a, b in zip(mine.tolist(), rates))
        print(f"{c['name']}: {len(rates)} rates, schedule.table vs the reference: max relative difference {rel:.3e}")
        assert len(mine) == len(rates) and rel <= BAR, (c["name"], rel)
        out["cases"].append(dict(c, rates=rates))
    path = os.path.join(ROOT, "tests", "golden", "lr_schedules.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
