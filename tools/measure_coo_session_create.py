#!/usr/bin/env python3
"""Session creation from unordered triplets (cogaps_session_create_coo) at BASELINE configs[4]'s shard shape -- 50000 x 12500, 95 % zeros,
K = 50 -- on one MI355X: wall time (host clock around the call, which ends in a stream synchronise), cogaps_session_device_bytes, and
device memory before / during (lowest free bytes seen by a polling thread) / after from cogaps_device_memory, for host pointers and for
device pointers, three runs each after a warm-up, beside cogaps_session_create_sparse from the CSR form of the same matrix (host and
device pointers) in the same process.  The triplets are the matrix's entries in a shuffled order with about 1 % of the positions repeated (an earlier entry of another
value).  The structures of the triplet session are compared with the CSR session's once.

    python tools/measure_coo_session_create.py --out profiles/coo_input_session_create.json

--parent-lib: libcogaps_hip.so built from the parent commit's csrc/ -- every row is then measured with that library too, in this
process and on the same arrays (rows "<name>_parent_commit"), the two libraries taking turns row by row."""
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


class FreeMemoryPoll:
    """lowest free device memory seen while the block runs (hipMemGetInfo is device-wide: other processes on the GPU count too)"""

    def __init__(self, capi, lib):
        self.capi, self.lib, self.low, self.stop = capi, lib, None, False

    def __enter__(self):
        self.before = self.low = self.capi.device_memory(lib=self.lib)[0]
        self.t = threading.Thread(target=self.run)
        self.t.start()
        return self

    def run(self):
        while not self.stop:
            self.low = min(self.low, self.capi.device_memory(lib=self.lib)[0])
            time.sleep(0.0005)

    def __exit__(self, *a):
        self.stop = True
        self.t.join()
        self.after = self.capi.device_memory(lib=self.lib)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=50000)
    ap.add_argument("--samples", type=int, default=12500)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coo_input_session_create.json"))
    a = ap.parse_args()
    import torch
    import scipy.sparse as sp
    import bench
    from cogaps_amd import _capi
    lib = _capi.load()
    libs = [("", lib)] + ([("_parent_commit", _capi.bind(ctypes.CDLL(a.parent_lib)))] if a.parent_lib else [])
    kw = dict(nPatterns=50, nIterations=100, seed=42, sparseOptimization=True)
    data = bench.synthetic_dense(a.genes, a.samples)
    data *= (np.random.Generator(np.random.MT19937(777)).random(data.shape) >= 0.95)
    csr = sp.csr_matrix(data)
    del data
    rng = np.random.default_rng(5)
    coo = csr.tocoo()
    r, c, v = coo.row.astype(np.uint32), coo.col.astype(np.uint32), coo.data.astype(np.float32)
    n = r.size
    # 1 % of the positions once more, with another value (half of them zero), BEFORE their deciding entry in input order
    rep = rng.choice(n, n // 100, replace=False)
    key = rng.random(n)
    r, c = np.concatenate([r, r[rep]]), np.concatenate([c, c[rep]])
    v = np.concatenate([v, np.where(rng.random(rep.size) < 0.5, 0.0, 3.0).astype(np.float32)])
    order = np.argsort(np.concatenate([key, key[rep] * rng.random(rep.size)]), kind="stable")
    r, c, v = np.ascontiguousarray(r[order]), np.ascontiguousarray(c[order]), np.ascontiguousarray(v[order])
    del coo, key, order
    host = _capi.CooMatrix(csr.shape, r, c, v)
    dev = torch.device("cuda", torch.cuda.current_device())
    t = [torch.from_numpy(x.view(dt)).to(dev) for x, dt in ((r, np.int32), (c, np.int32), (v, np.float32))]
    torch.cuda.synchronize()
    onDev = _capi.CooMatrix(csr.shape, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), on_device=True, nnz=r.size)
    tc = [torch.from_numpy(x).to(dev) for x in (csr.indptr.astype(np.int64), csr.indices.astype(np.int32), csr.data.astype(np.float32))]
    torch.cuda.synchronize()
    csrDev = _capi.SparseMatrix(csr.shape, True, tc[0].data_ptr(), tc[1].data_ptr(), tc[2].data_ptr(), on_device=True)
    small = sp.random(300, 200, density=0.1, format="csr", dtype=np.float32, random_state=np.random.default_rng(1))
    for warm in (small, _capi.CooMatrix(small.shape, small.tocoo().row, small.tocoo().col, small.tocoo().data)):      # code objects, first allocations
        for _, L in libs:
            _capi.Session(warm, lib=L, **dict(kw, nPatterns=3)).close()
    out = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "command": " ".join(["python"] + sys.argv), "shape": [a.genes, a.samples],
           "matrix_nnz": int(csr.nnz), "triplets": int(r.size), "repeated_positions": int(rep.size), "source_hash": lib.cogaps_source_hash().decode(),
           "parent_source_hash": libs[-1][1].cogaps_source_hash().decode() if a.parent_lib else None,
           "parent_dense_route": {"create_s": [4.2, 4.3], "device_bytes": 15874467852, "from": "profiles/sparse_input_session_create.json (the route a .mtx file took)"},
           "parent_csr_route": {"create_s": [0.23, 0.24], "device_bytes": 874467852, "from": "profiles/sparse_input_session_create.json"}}
    ref = None
    for name, m in (("csr_host", csr), ("csr_device", csrDev), ("coo_host", host), ("coo_device", onDev)):
        for tag, L in libs:
            rows = []
            for i in range(a.runs):
                with FreeMemoryPoll(_capi, L) as poll:
                    t0 = time.perf_counter()
                    S = _capi.Session(m, lib=L, **kw)
                    dt = time.perf_counter() - t0
                    held = _capi.device_memory(lib=L)[0]
                rows.append({"create_s": round(dt, 4), "ordered_sums_ms": round(S.sparse_build_ms(), 3), "device_bytes": S.device_bytes(), "free_before": poll.before,
                             "lowest_free_during": poll.low, "free_after_create": held,
                             "peak_bytes_during_build": poll.before - poll.low, "peak_temporary_bytes": poll.before - poll.low - (poll.before - held)})
                if i == 0:
                    d = {w: S.debug_sparse_data(w) for w in "AP"}
                    if ref is None:
                        ref = d
                    else:
                        rows[-1]["structures_equal_csr_session"] = bool(all(np.array_equal(d[w][f], ref[w][f]) for w in "AP" for f in ("flags", "prefix", "ptr", "vals", "lambda", "maxGibbsMass")))
                    del d
                S.close()
            out[name + tag] = rows
            print(name + tag, json.dumps(rows), flush=True)
    out["dense_array_bytes"] = a.genes * a.samples * 4
    # the build's temporaries by arithmetic (cogaps_hip.cpp, spb_triplets): one sampler's present flags, prefix counts and
    # pointers; a winner index per present position; a keep bit per entry; with host pointers the three uploaded arrays
    words = a.genes * (a.samples // 64 + 1)
    out["temporaries_by_arithmetic"] = {"present_flags_prefix_ptr": words * 12 + (a.genes + 1) * 4, "winner": 4 * (int(csr.nnz) + 1),
                                        "keep_bits": 8 * (int(r.size) // 64 + 1), "uploaded_triplets_host_pointers_only": 12 * (int(r.size) + 1)}
    out["notes"] = ("free_* / lowest_free_during are hipMemGetInfo figures: device-wide, allocation granularity included, so free_before - "
                    "free_after_create exceeds device_bytes.  The lowest point falls at the end of the build, before the session's last "
                    "allocations (statistics, PUMP: 4 * K * (3 * genes + 2 * samples) bytes, padding aside): peak_bytes_during_build is the figure to compare with "
                    "dense_array_bytes; peak_temporary_bytes (= free_after_create - lowest_free_during) understates the temporaries by those "
                    "last allocations.")
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
