#!/usr/bin/env python3
"""Consensus patterns (cogaps_pattern_match) on one MI355X against the host form (distributed.pattern_match, float64
numpy) on the same inputs, in the same process on the same box: planted patterns plus noise -- nSets copies of nPatterns patterns, so
that clusters exist -- at 20000 x 400 (20 sets of 20 patterns) and at 50000 x 2000 (40 sets of 50 patterns), cut = nPatterns, minNS
and maxNS the defaults of CogapsParams.  Recorded: the wall time of one library call from a numpy matrix in host memory -- upload,
staging, correlation, every clustering launch, the clusters' statistics, the copy back (host clock around the call, which ends in a
stream synchronise) -- for `--runs` runs after one warm-up, and the time of the host form with the threads it is given: the whole
pattern_match at the first shape; at the second the correlation (`_cor`) plus the first 50 merges of the first clustering only, which
the record states (`host_part`).  At the first shape the memberships of the two forms must be equal and the consensus matrices are
compared in float32 ulps.  The work runs in a worker process of its own; every shape has its own time limit, and a shape that exceeds
it ends the worker and the measurement.

    python tools/measure_consensus.py --out profiles/consensus.json"""
import argparse
import json
import os
import queue
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOST_MERGES = 50         # merges of the first clustering the host form is timed on at the second shape


def shapes(small):
    f = 10 if small else 1
    return [{"rows": 20000 // f, "sets": 20, "patterns": 20, "host_part": "all of pattern_match"},
            {"rows": 50000 // f, "sets": 40, "patterns": 50, "host_part": "_cor and the first %d merges of the first clustering" % HOST_MERGES}]


def problem(shape):
    """every set's copy of every pattern: the pattern times noise of its own, float32, the sets side by side"""
    rng = np.random.Generator(np.random.PCG64(5200 + shape["rows"]))
    base = rng.gamma(0.7, 1.0, size=(shape["rows"], shape["patterns"]))
    return np.concatenate([base * rng.uniform(0.6, 1.4, size=base.shape) for _ in range(shape["sets"])], axis=1).astype(np.float32)


def worker(a):
    from cogaps_amd import CogapsParams, _capi
    from cogaps_amd import distributed as dd
    lib = _capi.load()
    print(json.dumps({"ready": True, "source_hash": lib.cogaps_source_hash().decode()}), flush=True)
    for shape in shapes(a.small):
        X = problem(shape)
        p = CogapsParams(nPatterns=shape["patterns"])
        p.distributed = "genome-wide"
        p.setDistributedParams(nSets=shape["sets"])
        seconds = []
        for i in range(a.runs + 1):
            t0 = time.perf_counter()
            got = _capi.pattern_match(X, p.cut, p.minNS, p.maxNS, lib=lib)
            seconds.append(round(time.perf_counter() - t0, 4))
        rec = dict(shape, columns=int(X.shape[1]), cut=p.cut, minNS=p.minNS, maxNS=p.maxNS, clusters=got["nClusters"],
                   columns_dropped=int((got["cluster"] == 0).sum()), warm_up_s=seconds[0], library_call_s=seconds[1:],
                   host_threads=int(os.environ.get("OMP_NUM_THREADS") or len(os.sched_getaffinity(0))))
        t0 = time.perf_counter()
        if shape["host_part"].startswith("all"):
            host = dd.pattern_match(X, p)
            rec["host_s"] = round(time.perf_counter() - t0, 3)
            assert len(host["clusteredPatterns"]) == got["nClusters"]
            for ci, members in enumerate(host["clusteredPatterns"]):
                assert np.array_equal(X[:, got["cluster"] == ci + 1], members), ci
            ulps = np.abs(host["consensus"].view(np.int32).astype(np.int64) - got["consensus"].view(np.int32).astype(np.int64))
            rec["memberships_equal"], rec["consensus_largest_difference_ulps"] = True, int(ulps.max())
        else:
            d = 1.0 - dd._cor(X)
            rec["host_cor_s"] = round(time.perf_counter() - t0, 3)
            dd._complete_linkage_cutree(d, X.shape[1] - HOST_MERGES)
            rec["host_s"] = round(time.perf_counter() - t0, 3)
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=float, default=400.0, help="seconds one shape may take, building its problem and the host form included")
    ap.add_argument("--small", action="store_true", help="a tenth of the rows (a dry run of the tool)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--runs", str(a.runs)] + (["--small"] if a.small else [])
    child = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
    lines = queue.Queue()
    threading.Thread(target=lambda: [lines.put(ln) for ln in child.stdout] + [lines.put(None)], daemon=True).start()
    records, expected = [], 1 + len(shapes(a.small))
    try:
        while len(records) < expected:
            try:
                ln = lines.get(timeout=a.limit)
            except queue.Empty:
                child.kill()
                raise SystemExit("the worker exceeded its time limit of %.0f s; %d shapes had finished" % (a.limit, max(len(records) - 1, 0)))
            if ln is None:
                raise SystemExit("the worker ended early with status %s" % child.wait())
            records.append(json.loads(ln))
            print(ln.strip(), flush=True)
    finally:
        child.stdout.close()
        child.wait()
    out = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "runs": a.runs, "source_hash": records[0]["source_hash"],
           "cpus_available": len(os.sched_getaffinity(0)), "cases": records[1:]}
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
