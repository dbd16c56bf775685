#!/usr/bin/env python3
"""Residuals of a result (cogaps_residuals) on one MI355X at two shapes: 20000 x 2000 with 50 patterns from a dense numpy matrix, and
50000 x 12500 with 50 patterns and 95 % zeros from a DeviceMatrix that already resides on the GPU, both with matrix=False (the
chi-square of every gene and sample and of the fit; no residual rows).  Recorded: the wall time of the call -- widening and upload of
both factor matrices, upload of the dense data or the build of the packed gene side from the handle, both kernels, the copy back (host
clock around the call, which ends in a stream synchronise) -- for `--runs` runs after one warm-up, the most device memory a call held,
and, on the same box with the threads it is given, the time of the float64 numpy formula ((D - A P^T) / pmax(0.1 D, 0.1))^2 summed
along both axes: over the whole matrix at the first shape, over the first `numpy_genes` genes (densified) at the second, which is
stated in the record.  The library's sums must agree with numpy's to 1e-10 relative (numpy adds in another order).  The work runs in a
worker process of its own; every step has its own time limit, and a step that exceeds it ends the worker and the measurement.

    python tools/measure_residuals.py --out profiles/residuals.json"""
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

NUMPY_GENES = 2000       # genes of the second shape the numpy formula is timed on


def shapes(small):
    f = 10 if small else 1
    return [{"input": "dense numpy", "genes": 20000 // f, "samples": 2000 // f, "patterns": 50, "zeros": 0.2},
            {"input": "DeviceMatrix", "genes": 50000 // f, "samples": 12500 // f, "patterns": 50, "zeros": 0.95}]


def problem(shape):
    """float32 factors as a run leaves them and data near their product, `zeros` of it absent; the second shape as scipy CSR, built in
    slabs of rows so that nothing dense of its whole size exists"""
    import scipy.sparse as sp
    rng = np.random.Generator(np.random.PCG64(4100 + shape["genes"]))
    G, N, K = shape["genes"], shape["samples"], shape["patterns"]
    A = rng.gamma(0.7, 1.0, size=(G, K)).astype(np.float32)
    P = rng.gamma(0.7, 1.0, size=(N, K)).astype(np.float32)
    slabs = []
    for g0 in range(0, G, 1000):
        slab = (A[g0:g0 + 1000] @ P.T) * rng.uniform(0.5, 1.5, size=(min(1000, G - g0), N)).astype(np.float32)
        slab[rng.random(slab.shape) < shape["zeros"]] = 0
        slabs.append(slab if shape["input"] == "dense numpy" else sp.csr_matrix(slab))
    return A, P, (np.concatenate(slabs) if shape["input"] == "dense numpy" else sp.vstack(slabs, format="csr"))


def numpy_formula(A, P, D):
    A64, P64, D64 = A.astype(np.float64), P.astype(np.float64), D.astype(np.float64)
    q = ((D64 - A64 @ P64.T) / np.maximum(0.1 * D64, 0.1)) ** 2
    return q.sum(axis=1), q.sum(axis=0)


def worker(a):
    from cogaps_amd import _capi
    lib = _capi.load()
    print(json.dumps({"ready": True, "source_hash": lib.cogaps_source_hash().decode()}), flush=True)
    for shape in shapes(a.small):
        A, P, D = problem(shape)
        rec = dict(shape, stored_entries=int(np.count_nonzero(D)) if isinstance(D, np.ndarray) else int(D.nnz))
        data = D
        if shape["input"] == "DeviceMatrix":
            t0 = time.perf_counter()
            data = _capi.DeviceMatrix(D, lib=lib)
            rec["device_matrix_upload_s"] = round(time.perf_counter() - t0, 4)
        seconds = []
        for i in range(a.runs + 1):
            t0 = time.perf_counter()
            got = _capi.residuals(A, P, data=data, lib=lib)
            seconds.append(round(time.perf_counter() - t0, 4))
        n = shape["genes"] if isinstance(D, np.ndarray) else min(NUMPY_GENES, shape["genes"])
        sub = D if isinstance(D, np.ndarray) else D[:n].toarray()
        t0 = time.perf_counter()
        gene, sample = numpy_formula(A[:n], P, sub)
        dt = time.perf_counter() - t0
        worst = float(np.max(np.abs(got["geneChiSq"][:n] - gene) / gene))
        if n == shape["genes"]:
            worst = max(worst, float(np.max(np.abs(got["sampleChiSq"] - sample) / sample)))
        assert worst < 1e-10, worst
        print(json.dumps(dict(rec, warm_up_s=seconds[0], library_call_s=seconds[1:], peak_device_bytes=got["peakDeviceBytes"], chiSq=got["chiSq"],
                              numpy_genes=n, numpy_s=round(dt, 3), numpy_threads=int(os.environ.get("OMP_NUM_THREADS") or len(os.sched_getaffinity(0))), largest_relative_difference=worst)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=float, default=400.0, help="seconds one shape may take, building its problem and the numpy formula included")
    ap.add_argument("--small", action="store_true", help="a tenth of the genes and samples (a dry run of the tool)")
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
