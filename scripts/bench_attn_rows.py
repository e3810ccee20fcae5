"""Kernel-level timing of the attention-matrix backward behind its own dM product, exact fp32, B = 8, the (c, heads, C, plane) of the
transport map's levels: the one-launch form (attn_rows = "off": rcot_bmm_nt with its reduce launch, then rcot_attn_core_bwd at every
head width) against the row-group form (rcot_attn_rows_bwd; up to 32x32 behind rcot_bmm_nt_slabs: the slabs the product really
chooses at that level go straight into the row-group kernel).  Every launch is timed by the library's own per-launch device time
stamps (rcot_profile_begin / _end); the operands of the measured kernels were written by the launch before them or belong to
another of NSETS rotating sets, never to the previous repetition.
    python scripts/bench_attn_rows.py [reps]"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from rcot_amd import lib
from rcot_amd.ops import HipBackend

be = HipBackend()
be.prec = lib.PREC_FP32
B, NSETS = int(os.environ.get("BT_BATCH", "8")), 16
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 48
LEVELS = [(48, 1, 128), (96, 1, 128), (48, 2, 64), (48, 4, 32), (48, 8, 16), (96, 4, 16)]          # c, heads, plane side
WATCH = ("nt_reduce", "attn_bwd_core", "attn_rows")


def profile(fn):
    buf = ctypes.create_string_buffer(1 << 16)
    for i in range(NSETS):
        fn(i)
    be.side_join()
    torch.cuda.synchronize()
    be.L.rcot_profile_begin()
    for i in range(REPS):
        fn(i % NSETS)
    torch.cuda.synchronize()
    be.L.rcot_profile_end(buf, 1 << 16)
    rows = {}
    for ln in buf.value.decode(errors="replace").splitlines():
        name, n, ms = ln.rsplit("|", 2)
        name = name.replace("(anonymous namespace)::", "").replace("void ", "").replace("rcot_nt::", "").split("(")[0]
        rows[name] = rows.get(name, 0.0) + float(ms) * 1e3 / REPS          # us per repetition
    return rows


for c, heads, side in LEVELS:
    C, N = heads * c, side * side
    dy, V = torch.randn(B, 1, C, N, device="cuda"), torch.randn(B, 1, C, N, device="cuda")
    Wo, temp = torch.randn(C, C, device="cuda") * 0.1, torch.ones(heads, device="cuda")
    sets = []
    for _ in range(NSETS):
        Gn = torch.tanh(torch.randn(B, heads, c, c, device="cuda"))
        outs = [torch.empty(s, device="cuda") for s in ((B, C, C), (B, C, C), (B, heads), (B, heads, c, c), (B, heads, c, c), (B, C), (B, C))]
        sets.append((torch.softmax(Gn, -1), Gn, 1 + torch.rand(B, 2 * C, device="cuda"), torch.empty(B, C, C, device="cuda"), outs))
    split = []

    def run(i, rows_form):
        A, Gn, sq, dM, outs = sets[i]
        be.attn_rows = "on" if rows_form else "off"
        if rows_form and N <= be.attn_rows_slab_maxn:                 # (the rule of TransformerBlockOp.backward)
            d = be.bmm_nt_slabs(dy, V)
            split.append(d[1])
            assert be.attn_core_bwd(d, Wo, A, Gn, sq, temp, *outs)
        elif rows_form:
            be.bmm_nt(dy, V, dM.unsqueeze(1))
            assert be.attn_core_bwd(dM, Wo, A, Gn, sq, temp, *outs)
        else:
            be.bmm_nt(dy, V, dM.unsqueeze(1))
            assert be.attn_core_bwd(dM, Wo, A, Gn, sq, temp, *outs)

    res = [profile(lambda i, f=f: run(i, f)) for f in (False, True)]
    print(f"c={c} heads={heads} C={C} {side}x{side} B={B}  (dM to the row groups: " + (f"{split[-1]} slabs)" if split else "dense)"))
    for tag, rows in zip(("one launch ", "row groups "), res):
        watched = {k: v for k, v in rows.items() if any(w in k for w in WATCH)}
        other = sum(v for k, v in rows.items() if k not in watched)
        print(f"  {tag}: " + " + ".join(f"{k} {v:.1f}" for k, v in watched.items()) + f" = {sum(watched.values()):.1f} us   (dM product {other:.1f} us)", flush=True)
