#!/usr/bin/env python3
"""The state file (cogaps_session_save_state / _load_state) on one MI355X: save time, load time and file size at the headline shape
(20000 x 2000, dense model, K = 50) and at BASELINE configs[4]'s shard shape (50000 x 12500, 95 % zeros, sparse model, K = 50), after
`--iterations` equilibration iterations.  Per row: wall times of `--runs` saves and loads after a warm-up of each (host clock around
the call; both calls synchronise the session's stream), the first save apart (it computes the data digest), the file's size next to
the bytes of one genes x samples fp32 array, and the session's device bytes.

    python tools/measure_state_file.py --out profiles/state_file.json"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="a tenth of each dimension (a dry run of the tool)")
    ap.add_argument("--dir", default=None, help="where the state files are written (default: a temporary directory)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    from cogaps_amd import _capi
    lib = _capi.load()
    out = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "source_hash": lib.cogaps_source_hash().decode(), "runs": a.runs,
           "iterations": a.iterations, "rows": []}
    f = 10 if a.small else 1
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        for genes, samples, zeros, sparse in ((20000 // f, 2000 // f, 0.0, False), (50000 // f, 12500 // f, 0.95, True)):
            data = bench.synthetic_dense(genes, samples)
            if zeros:
                data *= (np.random.Generator(np.random.MT19937(777)).random(data.shape) >= zeros)
            kw = dict(nPatterns=50, nIterations=1000, seed=42, sparseOptimization=sparse)
            path = os.path.join(tmp, "run.state")
            S = _capi.Session(data, lib=lib, **kw)
            S.run_iterations(1, 0, a.iterations)

            def timed(call):
                t0 = time.perf_counter()
                call(path)
                return round(time.perf_counter() - t0, 4)
            row = {"shape": [genes, samples], "zeros": zeros, "model": "sparse" if sparse else "dense", "dense_array_bytes": genes * samples * 4,
                   "first_save_s": timed(S.save_state), "save_s": [timed(S.save_state) for _ in range(a.runs)],
                   "file_bytes": os.path.getsize(path), "atoms": [S.natoms("A"), S.natoms("P")], "session_device_bytes": S.device_bytes()}
            S.close()
            T = _capi.Session(data, lib=lib, **kw)
            row["first_load_s"] = timed(T.load_state)
            row["load_s"] = [timed(T.load_state) for _ in range(a.runs)]
            assert T.position() == (1, a.iterations)
            T.close()
            print(json.dumps(row), flush=True)
            out["rows"].append(row)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
