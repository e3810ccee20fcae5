"""(Re)generate tests/golden/anysize.npz: outputs of the REFERENCE's own networks on images whose sizes are not multiples of the
networks' resampling levels, padded at the bottom and right as rcot_amd/wholeimage.py pads them and cropped back to the input size.

    python scripts/make_anysize_fixture.py

Runs only where the reference checkout is present (the path oracle/pin_against_reference.py names); the reference's modules are
imported the way that script imports them (stub modules for the packages this image lacks, save_image stubbed out).  Only arrays are
written.  Before anything is written the fp64 oracle is run on the same padded inputs and held to the Restormer outputs at the bar
tests/test_oracle_golden.py applies to T_net forward outputs (1e-5).

  restormer_cfg          [B, h, w, Hp, Wp, torch generator seed of the input, parameter seed]
  restormer_reflect_y    Net_Restormer.T_net(decoder=True) on torch.rand(1, 3, 37, 50) reflect-padded to 40 x 56, cropped to 37 x 50
  restormer_replicate_y  the same with replicate padding
  eval_psnr_70x90        PSNR (trainer.py:217-225) of the third validation pair of tests/synth_folders.py::dataset_tree(root, 1),
                         the 70 x 90 input reflect-padded to 72 x 96, the output cropped back; same parameters
  mprnet_reflect_y       Net.T_net with the parameters of tests/test_mprnet_gpu.py::_params() on the 38 x 54 input
                         seeded_tensor(75, (1, 3, 38, 54), lo=0, hi=1) reflect-padded to 40 x 56, cropped to 38 x 54
Every array is float32.
"""
import glob
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pin_against_reference as PIN   # noqa: E402
from oracle import rcot_oracle as O               # noqa: E402
from rcot_amd import mprnet as MP                 # noqa: E402
from rcot_amd import params as P                  # noqa: E402

BAR = 1e-5          # tests/test_oracle_golden.py::test_tnet_small


def padded(x, mult, mode):
    h, w = x.shape[-2:]
    return F.pad(x, (0, -w % mult, 0, -h % mult), mode=mode)


def main():
    PIN._stub_modules()
    sys.path.insert(0, PIN.REF)
    import Net as NM
    import Net_Restormer as NR
    torch.set_num_threads(8)
    fx = {}
    pT = PIN.to_t(P.seeded_params(P.tnet_param_shapes(), 11, "T"))
    refT = NR.T_net(decoder=True)
    refT.load_state_dict(pT)
    p64 = {k: v.double() for k, v in pT.items()}
    x = torch.rand(1, 3, 37, 50, generator=torch.Generator().manual_seed(5))
    fx["restormer_cfg"] = np.array([1, 37, 50, 40, 56, 5, 11], dtype=np.float32)
    with torch.no_grad():
        for mode in ("reflect", "replicate"):
            xp = padded(x, 8, mode)
            assert tuple(xp.shape[-2:]) == (40, 56)
            y = refT(xp)
            e = PIN.relerr(O.tnet_forward(p64, xp.double(), True), y)
            assert e < BAR, (mode, e)
            print(f"restormer 37x50 {mode}: fp64 oracle vs reference rel err {e:.2e}")
            fx[f"restormer_{mode}_y"] = y[..., :37, :50].contiguous().numpy()
        # the validation pair evaluate() skips without padding (tests/synth_folders.py)
        from PIL import Image
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from synth_folders import dataset_tree
        root = tempfile.mkdtemp()
        dataset_tree(root, 1)
        d, t = sorted(glob.glob(f"{root}/val/input/*"))[2], sorted(glob.glob(f"{root}/val/target/*"))[2]
        xi = torch.from_numpy(np.array(Image.open(d).convert("RGB")).transpose(2, 0, 1)).float().div(255).unsqueeze(0)
        yt = torch.from_numpy(np.array(Image.open(t).convert("RGB")).transpose(2, 0, 1)).float().div(255).unsqueeze(0)
        assert tuple(xi.shape[-2:]) == (70, 90)
        xp = padded(xi, 8, "reflect")
        y = refT(xp)
        e = PIN.relerr(O.tnet_forward(p64, xp.double(), True), y)
        assert e < BAR, e
        fx["eval_psnr_70x90"] = np.array(O.psnr(y[..., :70, :90], yt), dtype=np.float32)
        print(f"validation pair 70x90: fp64 oracle vs reference rel err {e:.2e}, reference PSNR {float(fx['eval_psnr_70x90']):.4f}")
        # the older transport map: a multiple of 4
        shapes = MP.mprnet_param_shapes()
        prm = PIN.to_t(P.seeded_params([(n, s) for n, s in shapes if not n.endswith("body.1.weight")], 71, "T"))
        for n, _s in shapes:
            if n.endswith("body.1.weight"):
                prm[n] = torch.full((1,), 0.2)
        refM = NM.T_net()
        refM.load_state_dict(prm)
        xm = PIN.seeded_tensor(75, (1, 3, 38, 54), lo=0.0, hi=1.0)
        xp = padded(xm, 4, "reflect")
        assert tuple(xp.shape[-2:]) == (40, 56)
        fx["mprnet_reflect_y"] = refM(xp)[..., :38, :54].contiguous().numpy()
    for k, v in fx.items():
        assert v.dtype == np.float32, (k, v.dtype)
    out = os.path.join(ROOT, "tests", "golden", "anysize.npz")
    np.savez_compressed(out, **fx)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
