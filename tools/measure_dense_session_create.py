#!/usr/bin/env python3
"""Creation of a sparse-model session from the DENSE matrix (cogaps_session_create with useSparseOptimization) at BASELINE configs[4]'s
shard shape -- 50000 x 12500, 95 % zeros, K = 50, the input bench.py --sparse feeds -- on one MI355X: wall time (host clock around the
call, which ends in a stream synchronise) and cogaps_session_device_bytes, three runs after a warm-up, and the device bytes of the
session created from the CSR form of the same matrix in the same process.  Works on any commit that has both entries (run it from the
tree whose library is to be measured).

    python tools/measure_dense_session_create.py --out dense_create.json

--parent-lib: libcogaps_hip.so built from the parent commit's csrc/ -- measured too, in this process on the same matrix, its runs taking
turns with this tree's ("parent_commit" in the output)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=50000)
    ap.add_argument("--samples", type=int, default=12500)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import scipy.sparse as sp
    import bench
    from cogaps_amd import _capi
    lib = _capi.load()
    libs = [(None, lib)] + ([("parent_commit", _capi.bind(ctypes.CDLL(a.parent_lib)))] if a.parent_lib else [])
    kw = dict(nPatterns=50, nIterations=100, seed=42, sparseOptimization=True)
    data = bench.synthetic_dense(a.genes, a.samples)
    data *= (np.random.Generator(np.random.MT19937(777)).random(data.shape) >= 0.95)
    out = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "shape": [a.genes, a.samples], "nnz": int((data > 0).sum()),
           "source_hash": lib.cogaps_source_hash().decode(), "dense_array_bytes": a.genes * a.samples * 4, "dense_create_s": []}
    res = {tag: (out if tag is None else out.setdefault(tag, {"source_hash": L.cogaps_source_hash().decode(), "dense_create_s": []})) for tag, L in libs}
    for tag, L in libs:
        _capi.Session(np.ascontiguousarray(data[:300, :200]), lib=L, **dict(kw, nPatterns=3)).close()      # code objects, first allocations
    for i in range(a.runs):
        for tag, L in libs:
            t0 = time.perf_counter()
            S = _capi.Session(data, lib=L, **kw)
            res[tag]["dense_create_s"].append(round(time.perf_counter() - t0, 4))
            res[tag]["dense_input_device_bytes"] = S.device_bytes()
            res[tag]["dense_input_ordered_sums_ms"] = round(S.sparse_build_ms(), 3)
            S.close()
    csr = sp.csr_matrix(data)
    for tag, L in libs:
        t0 = time.perf_counter()
        S = _capi.Session(csr, lib=L, **kw)
        res[tag]["csr_create_s"] = round(time.perf_counter() - t0, 4)
        res[tag]["csr_input_device_bytes"] = S.device_bytes()
        S.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
