#!/usr/bin/env python3
"""Creation of a session from a DENSE matrix on one MI355X, by where the matrix lies: from host pointers and from device pointers on this
tree (from device pointers: built on the device, csrc/dense_build.h), and the same two with the library of the parent commit -- at 20000 x 2000 (dense model, K = 50) and at 50000 x 12500 with 95 % zeros (BASELINE configs[4]'s shard; both
models, K = 50).  Per row: wall time of three runs after a warm-up (host clock around the call, which ends in a stream synchronise),
the HIP-event time of the ordered sums, cogaps_session_device_bytes, and the peak of device memory during the build above what was
in use before it (cogaps_device_memory, polled from a second thread) next to it.

    python tools/measure_dense_device_session_create.py --parent-lib /path/to/parent/libcogaps_hip.so --out profiles/dense_device_input_session_create.json

--parent-lib: libcogaps_hip.so built from the parent commit's csrc/ (omitted: that route is left out)."""
import argparse
import ctypes
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_create(_capi, lib, make, runs):
    """make() -> Session; wall times, the session's bytes, the ordered sums' time and the build's peak of device memory"""
    out = {"create_s": [], "ordered_sums_ms": []}
    for i in range(runs + 1):      # (the first run is the warm-up)
        free0, _ = _capi.device_memory(lib=lib)
        low, stop = [free0], threading.Event()

        def poll():
            while not stop.is_set():
                low[0] = min(low[0], _capi.device_memory(lib=lib)[0])
                time.sleep(0.002)
        th = threading.Thread(target=poll)
        th.start()
        t0 = time.perf_counter()
        S = make()
        dt = time.perf_counter() - t0
        stop.set(), th.join()
        if i:
            out["create_s"].append(round(dt, 4))
            out["ordered_sums_ms"].append(round(S.sparse_build_ms(), 3))
        out["session_device_bytes"] = S.device_bytes()
        out["peak_device_bytes_during_build"] = int(free0 - low[0])
        S.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a tenth of each dimension (a dry run of the tool)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    from cogaps_amd import _capi
    lib = _capi.load()
    parent = _capi.bind(ctypes.CDLL(a.parent_lib)) if a.parent_lib else None
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "source_hash": lib.cogaps_source_hash().decode(),
           "parent_source_hash": parent.cogaps_source_hash().decode() if parent else None, "runs": a.runs, "rows": []}
    f = 10 if a.small else 1
    for genes, samples, zeros, models in ((20000 // f, 2000 // f, 0.0, (False,)), (50000 // f, 12500 // f, 0.95, (False, True))):
        data = bench.synthetic_dense(genes, samples)
        if zeros:
            data *= (np.random.Generator(np.random.MT19937(777)).random(data.shape) >= zeros)
        t = torch.from_numpy(data).to(dev)
        torch.cuda.synchronize()
        for sparse in models:
            kw = dict(nPatterns=50, nIterations=100, seed=42, sparseOptimization=sparse)
            row = {"shape": [genes, samples], "zeros": zeros, "model": "sparse" if sparse else "dense", "dense_array_bytes": genes * samples * 4}
            row["host_pointers"] = timed_create(_capi, lib, lambda: _capi.Session(data, lib=lib, **kw), a.runs)
            row["device_pointers"] = timed_create(_capi, lib, lambda: _capi.Session(_capi.DeviceDense(data.shape, t.data_ptr()), lib=lib, device=dev.index, **kw), a.runs)
            if parent:
                row["host_pointers_parent_commit"] = timed_create(_capi, parent, lambda: _capi.Session(data, lib=parent, **kw), a.runs)
                row["device_pointers_parent_commit"] = timed_create(_capi, parent, lambda: _capi.Session(_capi.DeviceDense(data.shape, t.data_ptr()), lib=parent, device=dev.index, **kw), a.runs)
            assert row["device_pointers"]["session_device_bytes"] == row["host_pointers"]["session_device_bytes"]
            print(json.dumps(row), flush=True)
            out["rows"].append(row)
        del t
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
