"""(Re)generate tests/golden/otcost_sizes.npz: the OT cost of the generator step (reference trainer.py:320-332) at sizes that are
not powers of two, where rcot_ot_spectrum runs its mixed-radix line FFT.

    python scripts/make_otcost_sizes_fixture.py

Same recipe as section F4 of oracle/pin_against_reference.py (which made otcost.npz at 32 x 32): the trainer's inline expression —
torch.fft.fft2 of the residual, mean |F|^2 / 2 for de_id < 3 and mean |F| otherwise, plus the RMSE — evaluated in fp32 with torch's
own ops and autograd, checked here against the fp64 oracle (oracle.rcot_oracle.ot_cost) before anything is written.  One zero plane
and one constant plane per shape, as there.  Keys carry the shape: res_96x96, de_id_96x96, rmse_96x96, per_sample_96x96, dres_96x96, ...
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import rcot_oracle as O   # noqa: E402

SHAPES = [(96, 96), (24, 40)]
DE_ID = [0, 2, 3, 7]


def seeded(seed, shape, scale):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(np.ascontiguousarray(scale * g.standard_normal(shape), dtype=np.float32))


def relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def main():
    torch.set_num_threads(8)
    fx = {}
    for si, (H, W) in enumerate(SHAPES):
        B = len(DE_ID)
        res = seeded(711 + si, (B, 3, H, W), 0.2)
        res[1, 0] = 0.0                      # a plane whose spectrum is exactly zero (|F| = 0 branch)
        res[3, 1] = 0.25                     # constant plane: a single non-zero bin
        rr = res.clone().requires_grad_(True)
        deg = torch.zeros_like(res)
        res_fre = torch.fft.fft2(deg - (-rr))
        pen, per = 0, []
        for i in range(B):
            sl = res_fre[i, :]
            t_ = torch.mean(abs(sl) ** 2) ** 1 / 2 if DE_ID[i] < 3 else torch.mean(abs(sl))
            per.append(float(t_.detach()))
            pen = pen + t_
        mse_loss = (torch.mean(rr ** 2)) ** 0.5
        (mse_loss + pen).backward()
        ro = res.double().clone().requires_grad_(True)
        rm, fo = O.ot_cost(ro, torch.zeros_like(ro), DE_ID)
        (rm + fo).backward()
        m = torch.ones(B, 3, 1, 1)
        m[1, 0] = 0
        m[3, 1] = 0                          # the two degenerate planes: F/|F| of rounding-level bins
        e = max(abs(float(rm) - float(mse_loss)) / float(rm), abs(float(fo) - float(pen)) / float(fo),
                relerr(rr.grad * m, ro.grad * m))
        assert e < 1e-5, (H, W, e)
        print(f"{H}x{W}: fp32 expression vs fp64 oracle rel err {e:.2e}")
        t = f"_{H}x{W}"
        fx["res" + t], fx["de_id" + t] = res.numpy(), np.array(DE_ID)
        fx["rmse" + t], fx["per_sample" + t], fx["dres" + t] = np.array(float(mse_loss)), np.array(per), rr.grad.numpy()
    out = os.path.join(ROOT, "tests", "golden", "otcost_sizes.npz")
    np.savez_compressed(out, **fx)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
