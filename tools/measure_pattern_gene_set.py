#!/usr/bin/env python3
"""The enrichment of gene sets in every pattern (cogaps_pattern_gsea) on one MI355X at the shape of a bulk result: 20000 x 50
gamma-distributed loadings with 30 % exact zeros, 5000 sets of 15 .. 500 rows, numPerm = 1000.  Recorded: the wall time of the library
call -- validation, transposition and upload of the matrix, the ranking, every score kernel, the copy back (host clock around the
call, which ends in a stream synchronise) -- for `--runs` calls after one warm-up, and, on the same box, the time of the numpy
restatement of the same definition (tests/pattern_gene_set_cases.py; one thread) on every hundredth set, whose outputs must equal the
library's.  The work runs in a worker process of its own under a time limit; a worker that exceeds it is ended, and the measurement
with it.

    python tools/measure_pattern_gene_set.py --out profiles/pattern_gene_set.json"""
import argparse
import json
import os
import subprocess
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def shape(small):
    return {"rows": 20000, "patterns": 50, "sets": 500 if small else 5000, "set_rows": [15, 500], "numPerm": 100 if small else 1000, "seed": 42}


def problem(s):
    import pattern_gene_set_cases as pc
    rng = np.random.Generator(np.random.PCG64(2026))
    stat = pc.gamma_loadings(s["rows"], s["patterns"], 2026)
    sizes = rng.integers(s["set_rows"][0], s["set_rows"][1] + 1, size=s["sets"])
    members = [np.sort(rng.choice(s["rows"], size=int(m), replace=False)).astype(np.uint32) for m in sizes]
    return stat, members


def worker(a):
    import pattern_gene_set_cases as pc
    from cogaps_amd import _capi
    lib = _capi.load()
    s = shape(a.small)
    stat, members = problem(s)
    seconds = []
    for _ in range(a.runs + 1):
        t0 = time.perf_counter()
        got = _capi.pattern_gsea(stat, members, s["numPerm"], seed=s["seed"], lib=lib)
        seconds.append(round(time.perf_counter() - t0, 4))
    # the restatement on every hundredth set: a set's index is part of the draw's key, so each goes in under its own
    picked = list(range(0, s["sets"], 100))
    t0 = time.perf_counter()
    for t in picked:
        want = pc.gsea(stat, [members[t]], s["numPerm"], s["seed"], set_base=t)
        for key in ("es", "peak", "nGe", "permSum"):
            assert np.array_equal(got[key][t], want[key][0]), (t, key)
    dt = time.perf_counter() - t0
    scores = s["sets"] * s["patterns"] * (s["numPerm"] + 1)
    print(json.dumps(dict(s, source_hash=lib.cogaps_source_hash().decode(), members=int(sum(m.size for m in members)), enrichment_scores=scores,
                          warm_up_s=seconds[0], library_call_s=seconds[1:], numpy_sets=len(picked), numpy_s=round(dt, 3), numpy_threads=1,
                          numpy_s_all_sets_extrapolated=round(dt * s["sets"] / len(picked), 1), outputs_equal_numpy=True)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=float, default=900.0, help="seconds the worker may take, the numpy restatement included")
    ap.add_argument("--small", action="store_true", help="a tenth of the sets and of the permutations (a dry run of the tool)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--runs", str(a.runs)] + (["--small"] if a.small else [])
    try:
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit)
    except subprocess.TimeoutExpired:
        raise SystemExit("the worker exceeded its time limit of %.0f s" % a.limit)
    if done.returncode:
        raise SystemExit("the worker ended with status %s" % done.returncode)
    record = json.loads(done.stdout.strip().splitlines()[-1])
    print(json.dumps(record), flush=True)
    out = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "runs": a.runs, "cpus_available": len(os.sched_getaffinity(0)), "case": record}
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
