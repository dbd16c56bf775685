#!/usr/bin/env python3
"""The projection of new data onto a result's patterns (cogaps_project) on one MI355X at two shapes: 20 000 genes x
2000 samples x 50 patterns from a dense numpy matrix, and 50 000 x 12 500 x 50 with 95 % zeros from a DeviceMatrix (uploaded once,
before the clock starts).  Recorded per shape: the wall time of one _capi.project call -- the upload of the loadings (and of the dense
data), the packed form of the sparse data, the kernels, the copy back -- for the first call of the process and for `--runs` calls
after it, and the call's peakDeviceBytes; and, for comparison on the same box, numpy.linalg.lstsq in float64 with `--threads` threads
on the same data -- on a slice of the first samples where the whole matrix is not densified -- with the largest difference of the
coefficients, |library - lstsq| / max |lstsq|.  The library runs in a worker process of its own under a time limit.

    python tools/measure_projection.py --out profiles/projection.json

The kernels' own times come from one run of the worker under the profiler, without counters,
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/measure_projection.py --worker DIR
whose kernel_stats table `--kernel-stats CSV --out profiles/projection.json` adds to the record (the pj_ and spb_ rows)."""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (genes, samples, patterns, share of zeros, form, samples of the lstsq comparison)
SHAPES = [(20000, 2000, 50, 0.0, "dense numpy", 2000), (50000, 12500, 50, 0.95, "DeviceMatrix", 256)]


def problem(n, S, K, zeros, columns=None):
    """-> (L [n][K] float32, the data: [n][S] float32, or a scipy CSR matrix where zeros > 0); columns: only the first so many samples.
    Drawn in blocks of 1000 genes, so that a slice of the samples is the same numbers as the whole."""
    import numpy as np
    import scipy.sparse as sp
    rng = np.random.Generator(np.random.PCG64([2026, n, K]))
    L = (rng.gamma(2.0, 0.5, size=(n, K)) * (rng.random((n, K)) >= 0.3)).astype(np.float32)
    C = rng.gamma(2.0, 1.0, size=(K, S)).astype(np.float32)
    blocks = []
    for g0 in range(0, n, 1000):
        g1 = min(n, g0 + 1000)
        block = L[g0:g1] @ C * (0.8 + 0.4 * rng.random((g1 - g0, S), dtype=np.float32))
        if zeros > 0:
            block *= rng.random((g1 - g0, S), dtype=np.float32) >= zeros
        block = block[:, :columns] if columns else block
        blocks.append(sp.csr_matrix(block) if zeros > 0 and not columns else block)
    return L, (sp.vstack(blocks, format="csr") if zeros > 0 and not columns else np.concatenate(blocks))


def shapes(small):
    return [(s[0] // 20, s[1] // 20, s[2], s[3], s[4], min(s[5], s[1] // 20)) for s in SHAPES] if small else SHAPES


def worker(a):
    import numpy as np
    from cogaps_amd import _capi
    lib = _capi.load()
    out = {"source_hash": lib.cogaps_source_hash().decode(), "shapes": []}
    for n, S, K, zeros, form, cols in shapes(a.small):
        L, D = problem(n, S, K, zeros)
        nnz = int(D.nnz) if zeros > 0 else int(np.count_nonzero(D))
        data = _capi.DeviceMatrix(D, lib=lib) if form == "DeviceMatrix" else D
        calls = []
        for i in range(a.runs + 1):
            t0 = time.perf_counter()
            fit = _capi.project(L, data, lib=lib)
            calls.append(round(time.perf_counter() - t0, 5))
        np.save(os.path.join(a.worker, "coef_%d.npy" % n), fit["coef"][:, :cols])
        out["shapes"].append({"genes": n, "samples": S, "patterns": K, "zeros": zeros, "stored_entries": nnz, "data": form,
                              "multiply_adds_of_the_cross_product": n * S * K, "first_call_s": calls[0], "project_call_s": calls[1:],
                              "peakDeviceBytes": fit["peakDeviceBytes"], "bytes_of_an_fp32_densification": 4 * n * S})
        if form == "DeviceMatrix":
            data.close()
    print(json.dumps(out), flush=True)


def kernel_stats(path):
    with open(path, newline="") as fh:
        return [r for r in csv.DictReader(fh) if "pj_" in r.get("Name", "") or "spb_" in r.get("Name", "")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16, help="threads of the numpy comparison")
    ap.add_argument("--limit", type=float, default=420.0, help="seconds the worker may take")
    ap.add_argument("--small", action="store_true", help="a twentieth of the genes and samples (a dry run of the tool)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3's kernel_stats.csv of a run of the worker: added to the record at --out")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    for var in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):      # (before numpy is imported)
        os.environ[var] = str(a.threads)
    if a.worker:
        return worker(a)
    if a.kernel_stats:
        with open(a.out) as fh:
            out = json.load(fh)
        out["kernels"] = {"from": "one run of the worker under rocprofv3 --kernel-trace --stats, no counters", "rows": kernel_stats(a.kernel_stats)}
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
        return
    import numpy as np
    scratch = os.path.dirname(os.path.abspath(a.out)) if a.out else ROOT
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", scratch, "--runs", str(a.runs)] + (["--small"] if a.small else [])
    done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit)
    if done.returncode:
        raise SystemExit("the worker ended with status %s" % done.returncode)
    out = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "runs": a.runs}
    out.update(json.loads(done.stdout.strip().splitlines()[-1]))
    for shape, (n, S, K, zeros, form, cols) in zip(out["shapes"], shapes(a.small)):
        L, D = problem(n, S, K, zeros, columns=cols if cols < S else None)
        L64, D64 = L.astype(np.float64), np.asarray(D, dtype=np.float64)
        times = []
        for i in range(2):
            t0 = time.perf_counter()
            ref = np.linalg.lstsq(L64, D64, rcond=None)[0]
            times.append(round(time.perf_counter() - t0, 5))
        path = os.path.join(scratch, "coef_%d.npy" % n)
        got = np.load(path)
        os.remove(path)
        shape["lstsq"] = {"samples": cols, "first_s": times[0], "second_s": times[1], "threads": a.threads, "cpus_available": len(os.sched_getaffinity(0)),
                          "largest_difference_of_the_coefficients": float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))}
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
