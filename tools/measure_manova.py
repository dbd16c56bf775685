#!/usr/bin/env python3
"""MANOVA's sums (cogaps_manova_sscp) on one MI355X at two shapes: 500 000 x 50 patterns with p = 2 responses (a
single-cell result) and 20 000 x 50 with p = 2.  Recorded per shape: the wall time of one _capi.manova_sscp call -- the upload of X
and Y, the four kernels, the copy back -- for the first call of the process and for `--runs` calls after it; the wall time of
result.MANOVA on the same data (factor coding of two string columns, the call, the p x p algebra, the F tail) for as many calls; and,
for comparison on the same box, the time of the same two-pass formulas vectorised in numpy float64 (the centred cross-products by
matrix products) with `--threads` threads, whose sums must agree with the library's to 1e-10.  The library runs in a worker process of
its own under a time limit.

    python tools/measure_manova.py --out profiles/manova.json"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(500000, 50, 2), (20000, 50, 2)]


def problem(n, K, p):
    """-> (P [n][K] float32, annotations [n][p] of str)"""
    import numpy as np
    rng = np.random.Generator(np.random.PCG64([2025, n, K]))
    P = rng.gamma(2.0, 0.5, size=(n, K)).astype(np.float32)
    group = rng.integers(0, 4, size=(n, p))
    P[:, 0] += (0.5 * group[:, 0]).astype(np.float32)
    return P, np.array(["a", "b", "c", "d"])[group]


def codes(ann):
    import numpy as np
    return np.stack([np.unique(ann[:, j], return_inverse=True)[1].reshape(-1) + 1.0 for j in range(ann.shape[1])], axis=1)


def worker(a):
    import numpy as np
    from cogaps_amd import CogapsResult, _capi
    lib = _capi.load()
    out = {"source_hash": lib.cogaps_source_hash().decode(), "shapes": []}
    for n, K, p in ([(s[0] // 50, s[1], s[2]) for s in SHAPES] if a.small else SHAPES):
        P, ann = problem(n, K, p)
        Y = codes(ann)
        raw = {"Amean": np.ones((2, K), dtype=np.float32), "Asd": np.ones((2, K), dtype=np.float32), "Pmean": P, "Psd": np.ones_like(P)}
        res = CogapsResult(raw)
        entry, front = [], []
        for i in range(a.runs + 1):
            t0 = time.perf_counter()
            s = _capi.manova_sscp(P, Y, lib=lib)
            entry.append(round(time.perf_counter() - t0, 5))
        for i in range(a.runs):
            t0 = time.perf_counter()
            res.MANOVA(ann, lib=lib)
            front.append(round(time.perf_counter() - t0, 5))
        np.savez(os.path.join(a.worker, "sums_%d.npz" % n), **s)
        out["shapes"].append({"rows": n, "patterns": K, "responses": p, "upload_bytes": int(P.nbytes + Y.nbytes),
                              "first_call_s": entry[0], "manova_sscp_call_s": entry[1:], "result_MANOVA_s": front})
    print(json.dumps(out), flush=True)


def numpy_sums(P, Y):
    import numpy as np
    X = P.astype(np.float64)
    xm, ym = X.mean(axis=0), Y.mean(axis=0)
    dx, dy = X - xm, Y - ym
    return {"xMean": xm, "yMean": ym, "sxx": np.einsum("ik,ik->k", dx, dx), "sxy": dx.T @ dy, "syy": dy.T @ dy}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16, help="threads of the numpy comparison")
    ap.add_argument("--limit", type=float, default=300.0, help="seconds the worker may take")
    ap.add_argument("--small", action="store_true", help="a fiftieth of the rows (a dry run of the tool)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    for var in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):      # (before numpy is imported)
        os.environ[var] = str(a.threads)
    if a.worker:
        return worker(a)
    import numpy as np
    scratch = os.path.dirname(os.path.abspath(a.out)) if a.out else ROOT
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", scratch, "--runs", str(a.runs)] + (["--small"] if a.small else [])
    done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit)
    if done.returncode:
        raise SystemExit("the worker ended with status %s" % done.returncode)
    out = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "runs": a.runs}
    out.update(json.loads(done.stdout.strip().splitlines()[-1]))
    for shape in out["shapes"]:
        n, K, p = shape["rows"], shape["patterns"], shape["responses"]
        P, ann = problem(n, K, p)
        Y = codes(ann)
        times = []
        for i in range(a.runs + 1):
            t0 = time.perf_counter()
            ref = numpy_sums(P, Y)
            times.append(round(time.perf_counter() - t0, 5))
        path = os.path.join(scratch, "sums_%d.npz" % n)
        got = np.load(path)
        for key in ref:
            assert np.allclose(got[key], ref[key], rtol=1e-10, atol=1e-10 * float(np.abs(ref[key]).max())), "%s: the library's differs from numpy's" % key
        os.remove(path)
        shape["numpy"] = {"first_s": times[0], "seconds": times[1:], "threads": a.threads, "cpus_available": len(os.sched_getaffinity(0)),
                          "sums_agree_with_the_library's_to": 1e-10}
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
