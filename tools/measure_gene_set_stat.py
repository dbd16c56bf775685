#!/usr/bin/env python3
"""The gene-set permutation statistic (cogaps_gene_set_stat) on one MI355X at the shape of a genome-wide question: a 20000 x 50 Z matrix,
5000 sets of 15 .. 500 rows from a fixed generator, numPerm = 1000.  Recorded: the wall time of the library call -- validation, repacking
and upload of Z, both kernels, the copy back (host clock around the call, which ends in a stream synchronise) -- for `--runs` runs after
one warm-up, and, for comparison on the same box, the time of a vectorised numpy implementation of the same definition (DESIGN.md 4.8;
one thread) on every `--cpu-every`-th set, whose counts must equal the library's.  The library runs in a worker process of its own;
every run has its own time limit, and a run that exceeds it ends the worker and the measurement.

    python tools/measure_gene_set_stat.py --out profiles/gene_set_stat.json"""
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

SEED = 42


def problem(small):
    f = 10 if small else 1
    n, K, nSets, numPerm = 20000 // f, 50, 5000 // f, 1000 // f
    rng = np.random.Generator(np.random.PCG64(2024))
    Z = rng.normal(size=(n, K))
    sizes = rng.integers(15, 501, size=nSets)
    members = [np.sort(rng.choice(n, size=int(s), replace=False)).astype(np.uint32) for s in sizes]
    return Z, members, [int(s) for s in sizes], numPerm


# ---- the definition in numpy, vectorised over the permutations of a set ----
def _mix(x):
    m = np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(16)); x = (x * np.uint64(0x85EBCA6B)) & m
    x = x ^ (x >> np.uint64(13)); x = (x * np.uint64(0xC2B2AE35)) & m
    return x ^ (x >> np.uint64(16))


def _draws(n, s, seed, t, numPerm):
    p = np.arange(numPerm, dtype=np.uint64).reshape(-1, 1)
    keys = [_mix(np.uint64(seed) ^ _mix(np.uint64(t) ^ _mix(p ^ np.uint64(((r + 1) * 0x9E3779B9) & 0xFFFFFFFF)))) for r in range(4)]
    h = (max(2, int(n - 1).bit_length()) + 1) // 2
    hh, mask = np.uint64(h), np.uint64((1 << h) - 1)
    x = np.broadcast_to(np.arange(s, dtype=np.uint64), (numPerm, s)).copy()
    rows = np.broadcast_to(np.arange(numPerm).reshape(-1, 1), x.shape)
    todo = np.ones(x.shape, dtype=bool)
    while todo.any():
        v, rw = x[todo], rows[todo]
        L, R = v >> hh, v & mask
        for r in range(4):
            L, R = R, L ^ (_mix(R ^ keys[r][rw, 0]) & mask)
        x[todo] = (L << hh) | R
        todo = x >= np.uint64(n)
    return x.astype(np.int64)


def numpy_counts(Z, members, sizes, numPerm, seed, which):
    out = {}
    for t in which:
        act = np.zeros(Z.shape[1])
        for i in members[t]:
            act = act + Z[i]
        act = act / np.float64(len(members[t]))
        idx = _draws(Z.shape[0], sizes[t], seed, t, numPerm)
        acc = np.zeros((numPerm, Z.shape[1]))
        for j in range(sizes[t]):
            acc = acc + Z[idx[:, j]]
        out[t] = (act[None, :] < acc / np.float64(sizes[t])).sum(axis=0)
    return out


def worker(a):
    """warm-up + runs of the library call; one JSON line per call"""
    from cogaps_amd import _capi
    lib = _capi.load()
    Z, members, sizes, numPerm = problem(a.small)
    print(json.dumps({"ready": True, "source_hash": lib.cogaps_source_hash().decode()}), flush=True)
    for i in range(a.runs + 1):
        t0 = time.perf_counter()
        cnt, _ = _capi.gene_set_stat(Z, members, sizes, numPerm, seed=SEED, lib=lib)
        dt = time.perf_counter() - t0
        np.save(a.worker, cnt)
        print(json.dumps({"run": i, "seconds": round(dt, 4), "count_sum": int(cnt.sum(dtype=np.uint64))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds one library call may take")
    ap.add_argument("--setup-limit", type=float, default=300.0, help="seconds the worker may take to load the library and make the problem")
    ap.add_argument("--cpu-every", type=int, default=100, help="the numpy comparison takes every n-th set")
    ap.add_argument("--small", action="store_true", help="a tenth of each dimension (a dry run of the tool)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    Z, members, sizes, numPerm = problem(a.small)
    gathered = int(sum(sizes)) * numPerm * Z.shape[1]
    out = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "shape": {"rows": Z.shape[0], "patterns": Z.shape[1], "sets": len(sizes), "numPerm": numPerm,
           "set_sizes": [min(sizes), max(sizes)], "gathered_values": gathered}, "runs": a.runs}
    counts_file = os.path.join(os.path.dirname(os.path.abspath(a.out)) if a.out else ROOT, ".gene_set_stat_counts.npy")
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", counts_file, "--runs", str(a.runs)] + (["--small"] if a.small else [])
    child = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
    lines = queue.Queue()
    threading.Thread(target=lambda: [lines.put(ln) for ln in child.stdout] + [lines.put(None)], daemon=True).start()
    records, limit = [], a.setup_limit
    try:
        while len(records) < a.runs + 2:
            try:
                ln = lines.get(timeout=limit)
            except queue.Empty:
                child.kill()
                raise SystemExit("the worker exceeded its time limit of %.0f s; %d calls had returned" % (limit, max(len(records) - 1, 0)))
            if ln is None:
                raise SystemExit("the worker ended early with status %s" % child.wait())
            records.append(json.loads(ln))
            limit = a.limit
    finally:
        child.stdout.close()
        child.wait()
    out["source_hash"] = records[0]["source_hash"]
    out["warm_up_s"] = records[1]["seconds"]
    out["library_call_s"] = [r["seconds"] for r in records[2:]]
    out["gathered_values_per_s"] = round(gathered / min(out["library_call_s"]), 1)
    cnt = np.load(counts_file)
    os.remove(counts_file)
    # the same definition in numpy on a fraction of the sets, and the check that both computed the same counts
    which = list(range(0, len(sizes), a.cpu_every))
    t0 = time.perf_counter()
    ref = numpy_counts(Z, members, sizes, numPerm, SEED, which)
    dt = time.perf_counter() - t0
    for t in which:
        assert np.array_equal(ref[t], cnt[t]), "set %d: the library's counts differ from numpy's" % t
    part = int(sum(sizes[t] for t in which)) * numPerm * Z.shape[1]
    out["numpy"] = {"sets": len(which), "of": len(sizes), "seconds": round(dt, 3), "gathered_values": part, "gathered_values_per_s": round(part / dt, 1),
                    "threads": 1, "cpus_available": len(os.sched_getaffinity(0)), "counts_equal_the_library's": True}
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
