"""Per-iteration learning-rate schedules, and the EMA warm-up, held on the device.

The reference ships iteration-level schedulers in ``util/schedulers.py`` (CosineAnnealingRestartLR, CosineAnnealingRestartCyclicLR,
LinearLR, MultiStepRestartLR, linear_warmup_decay) that its ``trainer.py`` never calls; the only rate rule it runs is the epoch decay
lr * 0.1^(epoch // step).  Here they are a TABLE: ``table(spec, base_lr, total_iters, warmup_iters)`` evaluates the reference's closed
forms on the host, in double, once — one entry per iteration, the potential's rate (the transport map reads half of it).  The table
lives on the device; ``rcot_sched_advance`` (csrc/optim.hip, ONE small launch at the head of every minimax iteration) hands entry t to
the RCOT_CB_LR words of the two optimizers' control blocks and advances t.  The launch is recorded into the launch plans like any
other: nothing is patched into recorded calls and no scalar is read back.

``--lr_schedule`` grammar (GRAMMAR below):

    step                                   the reference's epoch decay (the default: no table, no launch, nothing changes)
    const                                  the base rate
    cosine[:<eta_min>]                     one half-cosine from the base rate to eta_min (default 0) over the run
    linear                                 LinearLR: base (1 - t / total)
    restarts:<p1>,<p2>,...[:<w1>,...][:<e1>,...]
                                           CosineAnnealingRestartCyclicLR: periods in iterations, one restart weight per period
                                           (default 1; an empty piece keeps the default: restarts:4,8::1e-6), one eta_min per period
                                           (default 0); a single eta_min serves every period: CosineAnnealingRestartLR
    multistep:<m1>,<m2>,...[:<gamma>]      MultiStepRestartLR without restarts: the rate is multiplied by gamma (default 0.1) at each
                                           milestone (a milestone listed k times: gamma^k), as the reference's recursion does

The reference's conventions are kept: a cycle of period p that starts after iteration r covers r < t <= r + p, its last iteration
t = r + p sits exactly at eta_min and the next one is position 1 of the next cycle (the full restart value eta_min + w (base - eta_min)
is position 0, which only t = 0 ever takes).  Past the last period the reference raises; here the last period's eta_min holds, as the
table's last entry holds on the device past the end of the table.

Warm-up (``--warmup_iters N``, the reference's linear_warmup_decay): base * t / N for t < N, then the schedule at t - N over
total - N iterations.

EMA warm-up (``--ema_warmup``): the decay of update u is min(D, (1 + u) / (10 + u)); the same launch leaves 1 - D_u in the block's
ema_omd word, which ``rcot_ema_step_dev`` reads.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import lib as _lib
from . import parallel as par

GRAMMAR = ("--lr_schedule is one of: step | const | cosine[:<eta_min>] | linear | restarts:<p1>,<p2>,...[:<w1>,...][:<e1>,...] | "
           "multistep:<m1>,<m2>,...[:<gamma>]")
NAMES = ("step", "const", "cosine", "linear", "restarts", "multistep")


def _refuse(spec, piece, why):
    raise ValueError(f"--lr_schedule {spec}: {piece!r} {why}; {GRAMMAR}")


def _floats(spec, piece, what, lo=None):
    out = []
    for item in piece.split(","):
        try:
            v = float(item)
        except ValueError:
            v = float("nan")
        if item.strip() == "" or not math.isfinite(v) or (lo is not None and v < lo):
            _refuse(spec, item, f"is not {what} (in {piece!r})")
        out.append(v)
    return out


def _ints(spec, piece, what, lo):
    out = []
    for item in piece.split(","):
        if not item.strip().isdigit() or int(item) < lo:
            _refuse(spec, item, f"is not {what} (in {piece!r})")
        out.append(int(item))
    return out


def parse(spec: str) -> dict:
    """``spec`` as {"kind": ..., parameters}; ValueError naming the offending piece otherwise"""
    if not isinstance(spec, str) or not spec:
        _refuse(spec, spec, "is empty")
    name, *pieces = spec.split(":")
    if name not in NAMES:
        _refuse(spec, name, "is not a schedule name")
    if name in ("step", "const", "linear"):
        if pieces:
            _refuse(spec, ":".join(pieces), f"follows {name}, which takes no parameter")
        return {"kind": name}
    if name == "cosine":
        if len(pieces) > 1:
            _refuse(spec, ":".join(pieces[1:]), "follows the eta_min of cosine, which takes one parameter")
        if pieces and "," in pieces[0]:
            _refuse(spec, pieces[0], "is a list: cosine takes one eta_min")
        return {"kind": name, "eta_min": _floats(spec, pieces[0], "a rate >= 0", 0.0)[0] if pieces else 0.0}
    if name == "restarts":
        if not pieces or len(pieces) > 3:
            _refuse(spec, ":".join(pieces), "is not periods[:weights][:eta_mins]")
        periods = _ints(spec, pieces[0], "a period of at least 1 iteration", 1)
        weights = [1.0] * len(periods)
        if len(pieces) > 1 and pieces[1] != "":
            weights = _floats(spec, pieces[1], "a restart weight >= 0", 0.0)
            if len(weights) != len(periods):
                _refuse(spec, pieces[1], f"holds {len(weights)} restart weights for {len(periods)} periods")
        etas = [0.0]
        if len(pieces) > 2:
            etas = _floats(spec, pieces[2], "a rate >= 0", 0.0)
        if len(etas) == 1:
            etas = etas * len(periods)
        if len(etas) != len(periods):
            _refuse(spec, pieces[2], f"holds {len(etas)} eta_mins for {len(periods)} periods (one for all, or one per period)")
        return {"kind": name, "periods": periods, "weights": weights, "eta_mins": etas}
    if not pieces or len(pieces) > 2:
        _refuse(spec, ":".join(pieces), "is not milestones[:gamma]")
    miles = _ints(spec, pieces[0], "a milestone of at least 1 iteration", 1)
    gamma = 0.1
    if len(pieces) > 1:
        if "," in pieces[1]:
            _refuse(spec, pieces[1], "is a list: multistep takes one gamma")
        gamma = _floats(spec, pieces[1], "a gamma > 0", 0.0)[0]
        if gamma <= 0.0:
            _refuse(spec, pieces[1], "is not a gamma > 0")
    return {"kind": name, "milestones": miles, "gamma": gamma}


def check_iters(total_iters, warmup_iters) -> None:
    if int(total_iters) < 1:
        raise ValueError(f"total_iters {total_iters}: a schedule covers at least one iteration")
    if int(warmup_iters) < 0:
        raise ValueError(f"--warmup_iters {warmup_iters}: the warm-up cannot be negative")
    if int(warmup_iters) >= int(total_iters):
        raise ValueError(f"--warmup_iters {warmup_iters}: the warm-up must be shorter than the run ({total_iters} iterations)")


def _body(p: dict, base: float, n: int) -> list:
    """the schedule proper at t = 0 .. n - 1 of a run of n iterations: the reference's closed forms (util/schedulers.py), in double"""
    kind = p["kind"]
    if kind == "const":
        return [base] * n
    if kind == "cosine":
        eta = p["eta_min"]
        return [eta + 0.5 * (base - eta) * (1.0 + math.cos(math.pi * (float(t) / float(max(1, n))))) for t in range(n)]
    if kind == "linear":
        return [(1 - t / n) * base for t in range(n)]
    if kind == "restarts":
        cum, s = [], 0
        for q in p["periods"]:
            s += q
            cum.append(s)
        out = []
        for t in range(n):
            idx = next((i for i, c in enumerate(cum) if t <= c), None)
            if idx is None:                                # past the last period: its eta_min holds (the reference raises here)
                out.append(float(p["eta_mins"][-1]))
                continue
            w, eta = p["weights"][idx], p["eta_mins"][idx]
            start = 0 if idx == 0 else cum[idx - 1]
            out.append(eta + w * 0.5 * (base - eta) * (1 + math.cos(math.pi * ((t - start) / p["periods"][idx]))))
        return out
    if kind == "multistep":
        count = {}
        for m in p["milestones"]:
            count[m] = count.get(m, 0) + 1
        out, lr = [], base
        for t in range(n):
            if t in count:
                lr = lr * p["gamma"] ** count[t]
            out.append(lr)
        return out
    raise ValueError(f"--lr_schedule {kind}: the epoch decay has no per-iteration table")


def table(spec: str, base_lr: float, total_iters: int, warmup_iters: int = 0) -> np.ndarray:
    """float64 [total_iters]: the potential's rate of every iteration"""
    p = parse(spec)
    check_iters(total_iters, warmup_iters)
    base, total, N = float(base_lr), int(total_iters), int(warmup_iters)
    if not (math.isfinite(base) and base >= 0.0):
        raise ValueError(f"base_lr {base_lr}: the base rate must be finite and >= 0")
    head = [base * (float(t) / float(N)) for t in range(N)]
    return np.asarray(head + _body(p, base, total - N), dtype=np.float64)


class Schedule:
    """The device side of a schedule: the table, the schedule block (include/rcot_hip.h RCOT_SB_*) and a host mirror of the counters.

    ``spec`` "step" builds no table: the block then only keeps the EMA warm-up.  ``ema_decay`` > 0 turns that warm-up on (the target D,
    written into the block once).  ``bind(T_opt, F_opt)`` names the two RCOT_CB_LR words the advance launch writes.  The mirror ``t`` /
    ``ema_updates`` exists for printing, ``param_groups`` and checkpoints: the device is never read."""

    def __init__(self, be, spec: str = "step", base_lr: float = 0.0, total_iters: int = 1, warmup_iters: int = 0, ema_decay: float = 0.0):
        self.spec, self.base_lr, self.total_iters, self.warmup_iters = spec, float(base_lr), int(total_iters), int(warmup_iters)
        self.ema_decay = float(ema_decay)
        dev = be.device
        self.table = None if parse(spec)["kind"] == "step" else table(spec, base_lr, total_iters, warmup_iters)
        self.table_dev = None if self.table is None else torch.from_numpy(self.table).to(dev)
        self.t, self.ema_updates = 0, 0
        self._dst = (None, None)
        self.block = torch.zeros(_lib.SB_WORDS, dtype=torch.float64, device=dev)
        self._write_block()

    def _write_block(self):
        h = torch.zeros(_lib.SB_WORDS, dtype=torch.float64)
        i = h.view(torch.int64)
        i[_lib.SB_T], i[_lib.SB_EMA_UPDATES] = self.t, self.ema_updates
        h[_lib.SB_EMA_DECAY] = self.ema_decay
        if self.ema_decay > 0.0:                           # what the next advance overwrites; never read before it
            h[_lib.SB_EMA_OMD] = 1.0 - min(self.ema_decay, (1.0 + self.ema_updates) / (10.0 + self.ema_updates))
        self.block.copy_(h)

    @property
    def omd_word(self):
        return self.block[_lib.SB_EMA_OMD:_lib.SB_EMA_OMD + 1]

    def bind(self, T_opt, F_opt):
        """the transport map's optimizer reads half the table's rate (mult 0.5 is exact: the reference's lr / 2), the potential's all"""
        self._opts = (T_opt, F_opt)
        if self.table is not None:
            for o in (T_opt, F_opt):
                if o.ctrl is None:
                    raise ValueError("a scheduled optimizer reads its rate from a control block: build it with max_norm (math.inf = guard only)")
                o.scheduled = True
            self._dst = tuple(o.ctrl[_lib.CB_LR:_lib.CB_LR + 1] for o in (T_opt, F_opt))
        self.show()

    def rate(self, t: Optional[int] = None) -> Optional[float]:
        """the table's entry of iteration t (default: the next one to run); the last entry holds past the end"""
        if self.table is None:
            return None
        return float(self.table[min(self.t if t is None else t, len(self.table) - 1)])

    def show(self):
        """param_groups[0]["lr"] of the bound optimizers <- the rate of the next iteration (host mirror; what the epoch line prints)"""
        v = self.rate()
        if v is not None and getattr(self, "_opts", None):
            self._opts[0].param_groups[0]["lr"] = v * 0.5
            self._opts[1].param_groups[0]["lr"] = v

    def advance(self, be):
        """the advance launch of one iteration, and the mirror"""
        be.sched_advance(self.block, self.table_dev, self._dst[0], 0.5, self._dst[1], 1.0)
        self.count()

    def count(self, n: int = 1):
        """the mirror alone: a replayed launch plan has issued the recorded advance launch"""
        if self.table is not None:
            self.t += n
        if self.ema_decay > 0.0:
            self.ema_updates += n

    def mirror(self):
        return (self.t, self.ema_updates)

    def set_mirror(self, m):
        self.t, self.ema_updates = m

    # ---- checkpoint / replica plumbing
    def state_dict(self):
        return {"spec": self.spec, "warmup_iters": self.warmup_iters, "total_iters": self.total_iters, "t": self.t, "ema_updates": self.ema_updates}

    def load_state_dict(self, sd):
        """continue at the stored counters (this run's own spec, warm-up and total stay: they come from its flags)"""
        self.t, self.ema_updates = int(sd.get("t", 0)), int(sd.get("ema_updates", 0))
        self._write_block()
        self.show()

    def start_at(self, t: int, ema_updates: Optional[int] = None):
        """a checkpoint without schedule state: start at iteration ``t``"""
        self.load_state_dict({"t": int(t) if self.table is not None else 0,
                              "ema_updates": (int(t) if ema_updates is None else int(ema_updates)) if self.ema_decay > 0.0 else 0})

    def broadcast(self, src: int = 0):
        par.broadcast_flat(self.block, src)
