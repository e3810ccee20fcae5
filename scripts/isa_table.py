"""Static instruction counts of the compiled kernels of one csrc file (no GPU): per kernel symbol the instructions, the VALU ones
(`v_*`), `v_mov_b32`, packed (`v_pk_*`), global loads, `s_waitcnt vmcnt(0)`, VGPRs, waves per SIMD and scratch bytes, from the
assembly and the resource comments hipcc writes behind every kernel.

    python scripts/isa_table.py stencil.hip [--grep gdfn_bwd] [-- extra hipcc flags, e.g. -fno-slp-vectorize]

The flags are the Makefile's (FLAGS of csrc/Makefile without the per-object additions: give those after `--`)."""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = os.path.join(ROOT, "rcot_amd", "csrc")
args = sys.argv[1:]
extra = []
if "--" in args:
    extra = args[args.index("--") + 1:]
    args = args[:args.index("--")]
pat = None
if "--grep" in args:
    pat = args[args.index("--grep") + 1]
    del args[args.index("--grep"):args.index("--grep") + 2]
src = os.path.join(CS, os.path.basename(args[0]))
with tempfile.TemporaryDirectory() as tmp:
    out = os.path.join(tmp, "k.s")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                    "-ffp-contract=off", *extra, "-S", "--cuda-device-only", src, "-o", out], stderr=subprocess.DEVNULL, check=True)
    lines = open(out).read().splitlines()
KEYS = ("instr", "valu", "mov", "pk", "loads", "vm0", "vgpr", "occ", "scratch")
name, inside, stats = None, False, {}
for ln in lines:
    m = re.match(r"^(_Z\w+):", ln)
    if m:
        name, inside = m.group(1), True
        stats[name] = dict.fromkeys(KEYS, 0)
        continue
    if name is None:
        continue
    st = stats[name]
    if inside:
        op = ln.split()[0] if ln.startswith("\t") and not ln.startswith(("\t.", "\t;")) and ln.split() else None
        if op:
            st["instr"] += 1
            st["valu"] += op.startswith("v_")
            st["mov"] += op == "v_mov_b32_e32" or op == "v_mov_b32"
            st["pk"] += op.startswith("v_pk_")
            st["loads"] += op.startswith(("global_load", "buffer_load"))
            st["vm0"] += op == "s_waitcnt" and "vmcnt(0)" in ln
            inside = op != "s_endpgm"
    for key, tag in (("vgpr", "; NumVgprs:"), ("occ", "; Occupancy:"), ("scratch", "; ScratchSize:")):
        if ln.startswith(tag):
            st[key] = int(ln.split(":")[1])
print(f"# {os.path.basename(src)} {' '.join(extra) if extra else '(Makefile FLAGS)'}")
print(f"{'kernel':44s} {'instr':>6s} {'VALU':>6s} {'v_mov':>6s} {'mov/VALU':>8s} {'packed':>6s} {'loads':>5s} {'vmcnt0':>6s} {'VGPRs':>5s} {'waves':>5s} {'scratch':>7s}")
for k, v in stats.items():
    d = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip()
    d = re.sub(r"\(anonymous namespace\)::|^void ", "", d).split("(")[0]
    if pat and pat not in d:
        continue
    print(f"{d:44s} {v['instr']:6d} {v['valu']:6d} {v['mov']:6d} {100.0 * v['mov'] / max(v['valu'], 1):7.1f}% {v['pk']:6d} {v['loads']:5d} "
          f"{v['vm0']:6d} {v['vgpr']:5d} {v['occ']:5d} {v['scratch']:7d}")
