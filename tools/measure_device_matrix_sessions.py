#!/usr/bin/env python3
"""Sessions from a device-resident matrix (cogaps_device_matrix) at BASELINE configs[4]'s shard shape -- 50000 x 12500, 95 % zeros -- on one
MI355X, wall time by the host clock around each call (every call ends in a stream synchronise), three runs each in one process after a
warm-up: creating the handle from host CSR and from shuffled triplets (1 % repeated positions); eight sessions of a K sweep created from
the handle, beside the same eight through cogaps_session_create_sparse from host pointers; a 1/8 subset session on either axis from a
whole-matrix handle of 50000 x 100000 (the shard eight times side by side), beside the session created from the scipy-cut shard (the cut
itself timed apart); cogaps_session_device_bytes, the handles' bytes and the peak of device memory (cogaps_device_memory, polled).

    python tools/measure_device_matrix_sessions.py --out profiles/device_matrix_session_create.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

K_SWEEP = (3, 5, 8, 10, 12, 15, 18, 20)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, round(time.perf_counter() - t0, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=50000)
    ap.add_argument("--samples", type=int, default=12500)
    ap.add_argument("--copies", type=int, default=8, help="shards side by side in the whole-matrix handle (0: skip that part)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_matrix_session_create.json"))
    a = ap.parse_args()
    import scipy.sparse as sp
    import bench
    from cogaps_amd import _capi
    from measure_coo_session_create import FreeMemoryPoll
    lib = _capi.load()
    kw = dict(lib=lib, nIterations=100, seed=42, sparseOptimization=True)
    data = bench.synthetic_dense(a.genes, a.samples)
    data *= (np.random.Generator(np.random.MT19937(777)).random(data.shape) >= 0.95)
    csr = sp.csr_matrix(data)
    del data
    rng = np.random.default_rng(5)
    coo = csr.tocoo()
    r, c, v = coo.row.astype(np.uint32), coo.col.astype(np.uint32), coo.data.astype(np.float32)
    n = r.size
    rep = rng.choice(n, n // 100, replace=False)      # 1 % of the positions once more, with another value, before their deciding entry
    key = rng.random(n)
    r, c = np.concatenate([r, r[rep]]), np.concatenate([c, c[rep]])
    v = np.concatenate([v, np.where(rng.random(rep.size) < 0.5, 0.0, 3.0).astype(np.float32)])
    order = np.argsort(np.concatenate([key, key[rep] * rng.random(rep.size)]), kind="stable")
    triplets = _capi.CooMatrix(csr.shape, np.ascontiguousarray(r[order]), np.ascontiguousarray(c[order]), np.ascontiguousarray(v[order]))
    del coo, key, order, r, c, v
    host = _capi.SparseMatrix.from_scipy(csr)
    small = sp.random(300, 200, density=0.1, format="csr", dtype=np.float32, random_state=np.random.default_rng(1))
    with _capi.DeviceMatrix(small, lib=lib) as w:      # warm-up: code objects, first allocations
        _capi.Session(w, nPatterns=3, subsetIndices=np.arange(1, 101, dtype=np.uint32), subsetDim=1, **kw).close()
        _capi.Session(small, nPatterns=3, **kw).close()
    with _capi.DeviceMatrix(_capi.CooMatrix(small.shape, small.tocoo().row, small.tocoo().col, small.tocoo().data), lib=lib) as w:
        _capi.Session(w, nPatterns=3, **kw).close()
    out = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "command": " ".join(["python"] + sys.argv), "shape": [a.genes, a.samples],
           "matrix_nnz": int(csr.nnz), "triplets": int(triplets.nnz), "k_sweep": list(K_SWEEP), "source_hash": lib.cogaps_source_hash().decode(), "runs": []}
    for i in range(a.runs):
        row = {}
        with FreeMemoryPoll(_capi, lib) as poll:
            dm, row["handle_from_host_csr_s"] = timed(lambda: _capi.DeviceMatrix(host, lib=lib))
        row["handle_csr_bytes"], row["handle_csr_peak_bytes_during_creation"] = dm.device_bytes(), poll.before - poll.low
        with FreeMemoryPoll(_capi, lib) as poll:
            dt, row["handle_from_triplets_s"] = timed(lambda: _capi.DeviceMatrix(triplets, lib=lib))
        row["handle_triplets_bytes"], row["handle_triplets_peak_bytes_during_creation"] = dt.device_bytes(), poll.before - poll.low
        for name, src in (("from_csr_handle", dm), ("from_triplet_handle", dt), ("create_sparse_host_pointers", host)):
            per, ss = [], []
            with FreeMemoryPoll(_capi, lib) as poll:
                t0 = time.perf_counter()
                for k in K_SWEEP:
                    s, sec = timed(lambda: _capi.Session(src, nPatterns=k, **kw))
                    per.append(sec), ss.append(s)
                row["eight_sessions_%s_s" % name] = round(time.perf_counter() - t0, 4)
            row["each_%s_s" % name] = per
            row["ordered_sums_ms_%s" % name] = [round(s.sparse_build_ms(), 3) for s in ss]
            row["session_bytes_%s" % name] = [s.device_bytes() for s in ss]
            row["peak_bytes_eight_sessions_%s" % name] = poll.before - poll.low
            if i == 0 and name != "create_sparse_host_pointers":
                ref = _capi.Session(host, nPatterns=K_SWEEP[0], **kw)
                row["structures_equal_create_sparse_%s" % name] = bool(all(np.array_equal(ss[0].debug_sparse_data(w)[f], ref.debug_sparse_data(w)[f])
                                                                           for w in "AP" for f in ("flags", "prefix", "ptr", "vals", "lambda", "maxGibbsMass")))
                ref.close()
            for s in ss:
                s.close()
        dm.close(), dt.close()
        out["runs"].append(row)
        print(json.dumps(row), flush=True)
    if a.copies:
        whole = sp.hstack([csr] * a.copies, format="csr")
        whole_csc, to_csc_s = timed(whole.tocsc)
        out["whole"] = {"shape": list(whole.shape), "nnz": int(whole.nnz), "scipy_tocsc_for_the_column_cut_s": to_csc_s, "runs": []}
        wh, out["whole"]["handle_from_host_csr_s"] = timed(lambda: _capi.DeviceMatrix(whole, lib=lib))
        out["whole"]["handle_bytes"] = wh.device_bytes()
        rows_idx = np.sort(np.random.default_rng(6).choice(a.genes, a.genes // 8, replace=False) + 1).astype(np.uint32)
        cols_idx = np.sort(np.random.default_rng(7).choice(whole.shape[1], whole.shape[1] // 8, replace=False) + 1).astype(np.uint32)
        for i in range(a.runs):
            row = {}
            for name, idx, dim, cutter in (("rows", rows_idx, 1, lambda: whole[rows_idx.astype(np.int64) - 1]), ("columns", cols_idx, 2, lambda: whole_csc[:, cols_idx.astype(np.int64) - 1])):
                with FreeMemoryPoll(_capi, lib) as poll:
                    s, row["subset_session_%s_from_handle_s" % name] = timed(lambda: _capi.Session(wh, nPatterns=50, subsetIndices=idx, subsetDim=dim, **kw))
                row["subset_session_%s_bytes" % name], row["subset_session_%s_peak_bytes" % name] = s.device_bytes(), poll.before - poll.low
                shard, row["scipy_cut_%s_s" % name] = timed(cutter)
                with FreeMemoryPoll(_capi, lib) as poll:
                    e, row["session_%s_from_the_cut_shard_s" % name] = timed(lambda: _capi.Session(shard, nPatterns=50, **kw))
                row["session_%s_from_the_cut_shard_bytes" % name], row["session_%s_from_the_cut_shard_peak_bytes" % name] = e.device_bytes(), poll.before - poll.low
                if i == 0:
                    row["structures_equal_%s" % name] = bool(all(np.array_equal(s.debug_sparse_data(w)[f], e.debug_sparse_data(w)[f])
                                                                 for w in "AP" for f in ("flags", "prefix", "ptr", "vals", "lambda", "maxGibbsMass")))
                s.close(), e.close()
                del shard
            out["whole"]["runs"].append(row)
            print(json.dumps(row), flush=True)
        wh.close()
    out["notes"] = ("*_peak_bytes are hipMemGetInfo differences (free before the block minus the lowest free seen by a polling thread): device-wide, "
                    "allocation granularity included.  create_sparse_host_pointers is code this change does not touch: the comparison with the parent.")
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
