"""(Re)generate tests/golden/loader_trace.json: the call trace of ``FolderLoader`` over every task family, both routes, two cache
budgets and two world sizes (tests/loader_trace.py says what is logged and how the runs are driven).

    python scripts/make_loader_trace_fixture.py

The trace pins the loader's observable behaviour — the draws of every sample's stream, the calls of the whole-image entry points and
their arguments, the rows handed to ``patch_prep`` / ``patch_prep_batch``, the order of cache insertions and the counters — ACROSS a
change of the loader, so it is recorded from the commit BEFORE such a change and never from the tree that is being changed: the
script refuses a tree whose rcot_amd/ differs from HEAD, and writes the commit it ran on into the file.  No kernel, codec or image
library version enters (the backend records, the PNGs are lossless).

  recorded_from   the commit (git rev-parse HEAD)
  entries         the length of the list tests/loader_trace.py::record returns
  runs            tests/loader_trace.py::digest of it: a running SHA-256 per batch, the cache's numbers per epoch
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loader_trace as LT                          # noqa: E402


def main():
    git = lambda *a: subprocess.run(["git", "-C", ROOT, *a], check=True, capture_output=True, text=True).stdout.strip()
    if git("status", "--porcelain", "--", "rcot_amd"):
        raise SystemExit("rcot_amd/ differs from HEAD: the trace is recorded from a commit, before the loader is changed")
    with tempfile.TemporaryDirectory() as root:
        log = LT.record(root)
    out = os.path.join(ROOT, "tests", "golden", "loader_trace.json")
    with open(out, "w") as f:
        runs = ",\n".join(json.dumps(r, separators=(",", ":")) for r in LT.digest(log))       # one run per line
        f.write(f'{{"recorded_from": "{git("rev-parse", "HEAD")}", "entries": {len(log)}, "runs": [\n{runs}\n]}}\n')
    print("wrote", out, os.path.getsize(out), "bytes,", len(log), "entries")


if __name__ == "__main__":
    main()
