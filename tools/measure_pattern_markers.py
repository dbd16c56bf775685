#!/usr/bin/env python3
"""Pattern markers (cogaps_pattern_markers) on one MI355X at two shapes: the genes of a bulk data set, 20000 x 50 with axis = 1, and
the cells of a single-cell one, 500000 x 50 with axis = 2, each for both thresholds.  Recorded: the wall time of the library call --
validation, transposition and upload of both matrices, every kernel, the copy back of ranks, scores and marker lists (host clock
around the call, which ends in a stream synchronise) -- for `--runs` runs after one warm-up, and, on the same box, the time of the
numpy restatement of the same definition (tests/pattern_marker_cases.py; one thread), whose ranks, scores and marker lists must equal
the library's.  The work runs in a worker process of its own; every step has its own time limit, and a step that exceeds it ends the
worker and the measurement.

    python tools/measure_pattern_markers.py --out profiles/pattern_markers.json"""
import argparse
import json
import os
import queue
import subprocess
import sys
import threading
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

THRESHOLDS = ("all", "cut")


def shapes(small):
    f = 10 if small else 1
    return [{"axis": 1, "rows": 20000 // f, "other_rows": 500 // f, "patterns": 50}, {"axis": 2, "rows": 500000 // f, "other_rows": 20000 // f, "patterns": 50}]


def problem(shape):
    """factor matrices as a run leaves them: float32 values, skewed, a few rows no pattern uses"""
    rng = np.random.Generator(np.random.PCG64(2025 + shape["axis"]))
    A = rng.gamma(0.7, 1.0, size=(shape["rows"], shape["patterns"])).astype(np.float32).astype(np.float64)
    O = rng.gamma(0.7, 1.0, size=(shape["other_rows"], shape["patterns"])).astype(np.float32).astype(np.float64)
    A[::4999] = 0.0
    return A, O


def worker(a):
    """per shape and threshold: warm-up + runs of the library call, then the restatement and the comparison; one JSON line per step"""
    import pattern_marker_cases as pc
    from cogaps_amd import _capi
    lib = _capi.load()
    print(json.dumps({"ready": True, "source_hash": lib.cogaps_source_hash().decode()}), flush=True)
    for shape in shapes(a.small):
        A, O = problem(shape)
        for threshold in THRESHOLDS:
            seconds = []
            for i in range(a.runs + 1):
                t0 = time.perf_counter()
                got = _capi.pattern_markers(A, O, threshold=threshold, lib=lib)
                seconds.append(round(time.perf_counter() - t0, 4))
            t0 = time.perf_counter()
            want = pc.restate(A, O, None, threshold)
            dt = time.perf_counter() - t0
            pc.check(got, want)
            print(json.dumps(dict(shape, threshold=threshold, warm_up_s=seconds[0], library_call_s=seconds[1:], markers=int(sum(m.size for m in got[2])),
                                  nan_rows=int(np.isnan(got[1][:, 0]).sum()), numpy_s=round(dt, 3), numpy_threads=1, outputs_equal_numpy=True)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=float, default=400.0, help="seconds one shape and threshold may take, the numpy restatement included")
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
    records, expected = [], 1 + len(shapes(a.small)) * len(THRESHOLDS)
    try:
        while len(records) < expected:
            try:
                ln = lines.get(timeout=a.limit)
            except queue.Empty:
                child.kill()
                raise SystemExit("the worker exceeded its time limit of %.0f s; %d steps had finished" % (a.limit, max(len(records) - 1, 0)))
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
