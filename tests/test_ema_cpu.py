"""CPU tier: the host side of weight averaging (rcot_amd/ema.py) on a backend double — layout-independent state, applied() restoring on an
exception, the trainer's flag refusals and the export tool on a hand-made checkpoint."""
import os

import numpy as np
import pytest
import torch

from ema_double import ema_step
from rcot_amd import params as P
from rcot_amd.ema import WeightAverage, export
from rcot_amd.ema import main as ema_main
from rcot_amd.net_restormer import ParamStore


class _Backend:
    """what WeightAverage and ParamStore use of a backend: zeros, device, and an ema_step made from the restatement"""
    device = torch.device("cpu")

    def zeros(self, *shape):
        return torch.zeros(*shape, dtype=torch.float32)

    def ema_step(self, ema, p, n, decay):
        ema[:n].copy_(torch.from_numpy(ema_step(ema[:n].numpy(), p[:n].numpy(), decay)))


SHAPES = [("a.weight", (5, 3)), ("b.bias", (7,)), ("c.weight", (2, 2, 3, 3)), ("dead.weight", (4,))]


class _Net:
    def __init__(self, live):
        self.be = _Backend()
        self.store = ParamStore(self.be, SHAPES, live, ["dead.weight"])
        self.repacks = 0

    def repack(self):
        self.repacks += 1

    def fill(self, seed):
        g = torch.Generator().manual_seed(seed)
        for n, shp in SHAPES:
            self.store.p[n].copy_(torch.rand(shp, generator=g) + 0.1)


def test_state_round_trip_between_layouts():
    a, b = _Net(["a.weight", "b.bias", "c.weight"]), _Net(["c.weight", "a.weight", "b.bias"])
    assert a.store.layout.offset != b.store.layout.offset
    a.fill(1)
    avg = WeightAverage(a, 0.75)
    assert torch.equal(avg.buf, a.store.flat) and avg.buf.data_ptr() != a.store.flat.data_ptr() and avg.updates == 0
    before = a.store.flat.numpy().copy()
    a.fill(2)
    avg.update()
    avg.update()
    want = ema_step(ema_step(before, a.store.flat.numpy(), 0.75), a.store.flat.numpy(), 0.75)
    assert np.array_equal(avg.buf.numpy(), want) and avg.updates == 2
    sd = avg.state_dict()
    assert sd["decay"] == 0.75 and sd["updates"] == 2 and list(sd["params"]) == [n for n, _ in SHAPES]
    b.fill(3)
    other = WeightAverage(b, 0.75)
    other.load_state_dict(sd)
    assert other.updates == 2
    back = other.state_dict()["params"]
    for n, shp in SHAPES:                                                 # the same named tensors, laid out differently
        assert tuple(back[n].shape) == shp and torch.equal(back[n], sd["params"][n])
        o = b.store.layout.offset[n]
        assert torch.equal(other.buf[o:o + back[n].numel()], sd["params"][n].reshape(-1))
    assert not torch.equal(other.buf, avg.buf)
    other2 = WeightAverage(b, 0.75)
    other2.load_state_dict(sd["params"])                                  # a checkpoint's plain "Tnet_ema"
    assert torch.equal(other2.buf, other.buf) and other2.updates == 0
    with pytest.raises(KeyError):
        other2.load_state_dict({k: v for k, v in sd["params"].items() if k != "b.bias"})
    with pytest.raises(ValueError):
        WeightAverage(a, 1.0)


def test_applied_swaps_in_place_and_restores_on_exception():
    net = _Net(["a.weight", "b.bias", "c.weight"])
    net.fill(4)
    avg = WeightAverage(net, 0.5)
    net.fill(5)
    avg.update()
    raw, ptr = net.store.flat.clone(), net.store.flat.data_ptr()
    with avg.applied():
        assert torch.equal(net.store.flat, avg.buf) and net.store.flat.data_ptr() == ptr and net.repacks == 1
        assert torch.equal(net.store.p["b.bias"], avg.state_dict()["params"]["b.bias"])      # the named views follow
    assert torch.equal(net.store.flat, raw) and net.repacks == 2
    with pytest.raises(RuntimeError, match="inside"):
        with avg.applied():
            raise RuntimeError("inside")
    assert torch.equal(net.store.flat, raw) and net.store.flat.data_ptr() == ptr and net.repacks == 4


@pytest.mark.parametrize("argv,word", [(["--ema", "1"], "0 < D < 1"), (["--ema", "-0.1"], "0 < D < 1"), (["--ema", "nan"], "0 < D < 1"),
                                       (["--val_weights", "raw"], "needs --ema"),
                                       (["--ema", "0.9", "--backbone", "mprnet"], "flat parameter store")])
def test_trainer_flag_refusals(argv, word, monkeypatch):
    from rcot_amd import trainer
    monkeypatch.setenv("RCOT_MPRNET_STOCK", "1")                           # the stock-ops MPRNet path, with or without a GPU
    with pytest.raises(SystemExit, match=word) as e:
        trainer.main(["--synthetic", "--iters", "1", "--nEpochs", "1"] + argv)
    assert "--ema" in str(e.value) or "--val_weights" in str(e.value)


def _tparams(seed):
    return {k: torch.from_numpy(v) for k, v in P.seeded_params(P.tnet_param_shapes(), seed, "T").items()}


def test_export_tool_on_a_hand_made_checkpoint(tmp_path):
    from rcot_amd.compat import load_checkpoint, shim
    raw, avg = _tparams(31), _tparams(32)
    fn = shim().F_net.from_state_dict({k: torch.from_numpy(v) for k, v in P.seeded_params(P.fnet_param_shapes(32), 33, "F").items()}, patch_size=32)
    src, dst = str(tmp_path / "in.pth"), str(tmp_path / "out.pth")
    torch.save({"epoch": 7, "Tnet": shim().T_net.from_state_dict(raw, decoder=True), "Fnet": fn, "T_optimizer": {"kind": "RMSprop"},
                "Tnet_ema": avg, "ema": {"decay": 0.9, "updates": 6}}, src)
    ema_main(["--in", src, "--out", dst])
    ex = load_checkpoint(dst)
    assert set(ex) == {"epoch", "Tnet", "Fnet"} and ex["epoch"] == 7
    assert type(ex["Tnet"]).__module__ == "Net_Restormer" and type(ex["Tnet"]).__name__ == "T_net"
    sd = ex["Tnet"].state_dict()
    assert list(sd) == list(avg) and all(torch.equal(sd[k], avg[k]) for k in avg)
    assert list(ex["Fnet"].state_dict()) == [n for n, _ in P.fnet_param_shapes(32)]
    # the MPRNet backbone's form: state_dicts under the same keys
    m = export({"epoch": 2, "backbone": "mprnet", "Tnet": {"w": torch.zeros(2)}, "Fnet": {"f": torch.ones(1)}, "Tnet_ema": {"w": torch.ones(2)},
                "ema": {"decay": 0.5, "updates": 1}, "F_optimizer": {}})
    assert set(m) == {"epoch", "Tnet", "Fnet", "backbone"} and torch.equal(m["Tnet"]["w"], torch.ones(2)) and isinstance(m["Tnet"], dict)
    plain = str(tmp_path / "plain.pth")
    torch.save({"epoch": 1, "Tnet": raw}, plain)
    with pytest.raises(SystemExit, match="Tnet_ema"):
        ema_main(["--in", plain, "--out", os.path.join(str(tmp_path), "never.pth")])
    assert not os.path.exists(os.path.join(str(tmp_path), "never.pth"))
