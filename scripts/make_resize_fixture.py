"""(Re)generate tests/golden/resize.npz: outputs of the REFERENCE's own util/imresize.py (cubic, antialiased) for the cases of
tests/resize_double.py::CASES.

    python scripts/make_resize_fixture.py

Runs only where the reference checkout is present (the path oracle/pin_against_reference.py names); util/imresize.py is loaded from
there by file path when the script runs.  Only arrays are written.

The reference follows MATLAB's rule (csrc/resize.hip) except where a tap lies left of / above pixel 0, so every
case is resized in four orientations — as is, rows flipped, columns flipped, both — and each result is flipped back: an output pixel is
compared in an orientation whose unmirrored taps are all >= 0 along both axes (its *sound region*).  Before anything is written the
script asserts that every output pixel of every case lies in the sound region of at least one orientation.

  cases     int64 [n, 4]: H, W, out_h, out_w
  in_<i>    uint8 [H, W]: the seeded input of case i (tests/resize_double.py::case_input)
  ref_<i>   float64 [4, out_h, out_w]: the reference on in_<i> / 255 in the orientations of tests/resize_double.py::ORIENTATIONS, flipped back
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import pin_against_reference as PIN   # noqa: E402
import resize_double as RD                         # noqa: E402


def main():
    spec = importlib.util.spec_from_file_location("reference_imresize", os.path.join(PIN.REF, "util", "imresize.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    fx = {"cases": np.array([[*a, *b] for a, b in RD.CASES], dtype=np.int64)}
    for i, ((H, W), (oh, ow)) in enumerate(RD.CASES):
        u8 = RD.case_input(i)
        x = u8.astype(np.float64) / 255.0
        covered = np.zeros((oh, ow), dtype=bool)
        outs = []
        for fr, fc in RD.ORIENTATIONS:
            y = ref.imresize(np.ascontiguousarray(RD.flip(x, fr, fc)), output_shape=(oh, ow), kernel="cubic", antialiasing=True)
            assert y.shape == (oh, ow) and y.dtype == np.float64, (y.shape, y.dtype)
            outs.append(np.ascontiguousarray(RD.flip(y, fr, fc)))
            covered |= RD.sound_mask(H, W, oh, ow, fr, fc)
        assert covered.all(), f"case {i} ({H}x{W} -> {oh}x{ow}): {int((~covered).sum())} output pixels lie in no orientation's sound region"
        fx[f"in_{i}"] = u8
        fx[f"ref_{i}"] = np.stack(outs)
        mine = RD.imresize_np(x[None], oh, ow)[0]
        err = max(float(np.abs(mine - outs[k])[RD.sound_mask(H, W, oh, ow, *o)].max()) for k, o in enumerate(RD.ORIENTATIONS))
        print(f"case {i}: {H}x{W} -> {oh}x{ow}  the rule vs the reference on the sound regions: {err:.1e}")
    out = os.path.join(ROOT, "tests", "golden", "resize.npz")
    np.savez_compressed(out, **fx)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
