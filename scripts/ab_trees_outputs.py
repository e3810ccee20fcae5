"""Two checkouts of the repository on ONE box, alternately: does a change move the results or the speed of a bench workload?

    python scripts/ab_trees_outputs.py build_variants/parent [--reps 3] [--out DIR] -- --config 3 --steps 20 --warmup 5

Runs `python bench.py <args> --dump-outputs DIR/<tree><rep>` from the other checkout (built beforehand, e.g. `git archive <commit>`
unpacked under build_variants/) and from this tree, `--reps` times each, alternating.  Prints ms per step of every run, then for
every dumped array (generated, losses, tnet_params, fnet_params: bench.py dump_outputs) the largest difference relative to
max|array| between two runs of the OTHER tree (what atomics alone do), between two runs of THIS tree, and across the trees.
Every run is a child process of its own with a time limit; the first one that fails ends the script.
"""
import argparse
import itertools
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("generated", "losses", "tnet_params", "fnet_params")


def rel(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / max(float(np.abs(b).max()), 1e-30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "build_variants", "ab_outputs"))
    ap.add_argument("--limit", type=int, default=300, help="seconds per bench run")
    args, bench_args = ap.parse_known_args()          # everything this script does not know goes to bench.py
    bench_args = [a for a in bench_args if a != "--"]
    trees = {"other": os.path.abspath(args.other), "this": ROOT}
    ms = {k: [] for k in trees}
    print(f"# bench.py {' '.join(bench_args)}; other = {args.other}")
    for rep in range(args.reps):
        for tag, tree in trees.items():
            d = os.path.join(os.path.abspath(args.out), f"{tag}{rep}")
            r = subprocess.run([sys.executable, "bench.py", *bench_args, "--dump-outputs", d], cwd=tree, capture_output=True,
                               text=True, timeout=args.limit, env=dict(os.environ, PYTHONPATH=tree))
            if r.returncode != 0:
                print(r.stderr[-2000:])
                raise SystemExit(f"{tag} run {rep} failed with {r.returncode}")
            line = json.loads(r.stdout.strip().splitlines()[-1])
            ms[tag].append(line["ms_per_step"])
            print(f"{tag:>5} run {rep}: {line['ms_per_step']:.3f} ms/step  {line['value']:.2f} {line.get('unit', '')}", flush=True)
    for tag in trees:
        print(f"{tag:>5}: ms/step min {min(ms[tag]):.3f} median {float(np.median(ms[tag])):.3f} max {max(ms[tag]):.3f}")
    load = lambda tag, rep, n: np.load(os.path.join(args.out, f"{tag}{rep}", n + ".npy"))
    pairs = list(itertools.combinations(range(args.reps), 2))
    print("# largest |difference| / max|array|: other vs other, this vs this, other vs this (all pairs of runs)")
    for n in NAMES:
        oo = max(rel(load("other", i, n), load("other", j, n)) for i, j in pairs)
        tt = max(rel(load("this", i, n), load("this", j, n)) for i, j in pairs)
        ot = max(rel(load("this", i, n), load("other", j, n)) for i in range(args.reps) for j in range(args.reps))
        print(f"{n:>12}: {oo:.3e}  {tt:.3e}  {ot:.3e}")


if __name__ == "__main__":
    main()
