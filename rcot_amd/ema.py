"""Weight averaging: an exponential moving average (EMA) of a network's parameters.

The last iterate of the transport map in the minimax game is noisy; what one validates, saves and ships is usually the average
    ema <- decay * ema + (1 - decay) * p         after every optimizer step.
Every network here keeps its parameters in one flat fp32 buffer (``ParamStore.flat``), so the average is one more buffer of the same
layout and one streaming launch per update (``rcot_ema_step``, csrc/optim.hip: the increment form ema += (1 - decay)(p - ema), one fused
multiply-add per element).  Dead tensors and the zero padding between tensors average to themselves.

    avg = WeightAverage(Tnet, 0.999)
    ... optimizer step ...; avg.update()
    with avg.applied():                          # the network computes with the averaged weights; the raw ones come back on exit
        evaluate(Tnet, ...)

``python -m rcot_amd.ema --in CKPT --out CKPT`` writes a checkpoint in the reference's own format whose "Tnet" is the averaged network
(no optimizer state, no "Tnet_ema"), so the reference's tools can use the average.

Works for any network with a ``store``: the Restormer map, ``MPRNetHip`` and the networks behind ``rcot_amd/autograd.py``.
"""
from __future__ import annotations

import contextlib
from collections import OrderedDict

import torch

from . import parallel as par


def check_decay(decay) -> float:
    """0 < decay < 1, as a float; ValueError naming the value otherwise (a NaN fails both comparisons)"""
    d = float(decay)
    if not (0.0 < d < 1.0):
        raise ValueError(f"EMA decay {decay}: the decay must satisfy 0 < decay < 1 (0.999 is usual)")
    return d


def _named(net):
    """(state_dict name, name in the store, shape) in the order of ``net.state_dict()``.  The two names differ only where a network lists
    one stored tensor several times (MPRNetHip's shared PReLU slope: ``shapes_all`` / ``slope_name``)."""
    st = net.store
    alias = getattr(net, "slope_name", None)
    return [(n, n if n in st.p else alias, tuple(shp)) for n, shp in (getattr(net, "shapes_all", None) or st.shapes)]


class WeightAverage:
    """EMA of ``net.store.flat`` in a buffer of the same layout."""

    def __init__(self, net, decay: float):
        self.net, self.decay = net, float(decay)
        if not (0.0 <= self.decay < 1.0):                       # (the kernel's own domain; the trainer's flag asks for 0 < D < 1)
            raise ValueError(f"EMA decay {decay}: the decay must be in [0, 1)")
        st = net.store
        self.n = st.layout.n_total
        self.buf = net.be.zeros(self.n)
        self.buf.copy_(st.flat)
        self.updates = 0
        #: None: the constant decay, by value.  A one-element float64 device view (the ema_omd word of a rcot_amd.schedule.Schedule built
        #: with ema_decay = this decay): every update reads its 1 - D_u from it (rcot_ema_step_dev) — the warm-up
        #: D_u = min(D, (1 + u) / (10 + u)), which that schedule's advance launch forms once per iteration
        self.omd_word = None

    def update(self):
        """one step of the average towards the current parameters: call it after the optimizer step"""
        if self.omd_word is not None:
            self.net.be.ema_step_dev(self.buf, self.net.store.flat, self.n, self.omd_word)
        else:
            self.net.be.ema_step(self.buf, self.net.store.flat, self.n, self.decay)
        self.updates += 1

    @contextlib.contextmanager
    def applied(self):
        """Inside, the network holds the averaged weights (in place: ``store.flat`` keeps its address, which recorded launch plans hold)
        and its private weight packs follow; on exit, after an exception too, the raw weights and their packs are back."""
        net = self.net
        flat = net.store.flat
        saved = flat.clone()
        try:
            flat.copy_(self.buf)
            if hasattr(net, "repack"):
                net.repack()
            yield net
        finally:
            flat.copy_(saved)
            if hasattr(net, "repack"):
                net.repack()

    # ---- checkpoint / replica plumbing
    def _view(self, store_name, shape):
        o, n = self.net.store.layout.offset[store_name], 1
        for v in shape:
            n *= v
        return self.buf[o:o + n].view(*shape)

    def tensors(self):
        """the averaged parameters under the names of ``net.state_dict()``, as CPU tensors"""
        return OrderedDict((n, self._view(s, shp).detach().cpu().clone()) for n, s, shp in _named(self.net))

    def state_dict(self):
        """Keyed by the reference's parameter names, so independent of the flat layout (as FlatOptimizer.state_dict)."""
        return {"decay": self.decay, "updates": self.updates, "params": self.tensors()}

    def load_state_dict(self, sd):
        """``sd``: what state_dict() returns, or a plain {name: tensor} dict (a checkpoint's "Tnet_ema").  The decay of this object stays."""
        params = sd["params"] if "params" in sd and isinstance(sd["params"], dict) else sd
        seen = set()
        for n, s, shp in _named(self.net):
            if s in seen:
                continue
            seen.add(s)
            if n not in params:
                raise KeyError(f"weight average: {n} is missing")
            t = params[n]
            if tuple(t.shape) != shp:
                raise ValueError(f"weight average: {n} has shape {tuple(t.shape)}, expected {shp}")
            self._view(s, shp).copy_(t.detach().to(self.buf.dtype))
        if "updates" in sd and not torch.is_tensor(sd["updates"]):
            self.updates = int(sd["updates"])

    def broadcast(self, src: int = 0):
        par.broadcast_flat(self.buf, src)


# ------------------------------------------------------------------------------- export: the average as a reference-format checkpoint
def export(ck: dict) -> dict:
    """A checkpoint dict of the reference's format whose "Tnet" is the average of ``ck``: a ``Net_Restormer.T_net`` object for the
    Restormer backbone, the state_dict form for the MPRNet backbone.  "Fnet" and "epoch" are kept; optimizer state and the average's
    own keys are not."""
    if not isinstance(ck, dict) or "Tnet_ema" not in ck:
        raise KeyError('the checkpoint has no "Tnet_ema" key: it was not written by a run with --ema')
    sd = OrderedDict((k, v.detach().cpu().clone()) for k, v in ck["Tnet_ema"].items())
    out = {"epoch": ck.get("epoch", 0)}
    if ck.get("backbone") == "mprnet":
        out.update(Tnet=sd, Fnet=ck["Fnet"], backbone="mprnet")
    else:
        from .compat import shim
        tn = ck["Tnet"]
        decoder = (tn.__dict__.get("_ctor") or {}).get("decoder", True) if not isinstance(tn, dict) else True
        out.update(Tnet=shim().T_net.from_state_dict(sd, decoder=decoder), Fnet=ck["Fnet"])
    return out


def main(argv=None):
    import argparse
    parser = argparse.ArgumentParser(description="write the averaged transport map of a --ema checkpoint as a reference-format checkpoint")
    parser.add_argument("--in", dest="inp", required=True, type=str, help="a checkpoint written by rcot_amd.trainer --ema")
    parser.add_argument("--out", required=True, type=str, help="the checkpoint to write: \"Tnet\" is the averaged network")
    o = parser.parse_args(argv)
    from .compat import load_checkpoint
    ck = load_checkpoint(o.inp)
    try:
        out = export(ck)
    except KeyError as e:
        raise SystemExit(f"{o.inp}: {e.args[0]}")
    torch.save(out, o.out)
    info = ck.get("ema") or {}
    print(f"{o.out}: Tnet = the average of {o.inp} (decay {info.get('decay')}, {info.get('updates')} updates)")
    return out


if __name__ == "__main__":
    main()
