#!/usr/bin/env python3
"""Gene-set membership (computeGeneGSProb) on one MI355X at the problem calcCoGAPSStat was measured at: a 20000 x 50 Z
matrix, 5000 sets of 15 .. 500 rows from a fixed generator, numPerm = 500.  Recorded: the wall time of result.computeGeneGSProb -- the
front end's set handling, the permutation test (cogaps_gene_set_stat), the weights, cogaps_gene_set_membership with its repacking, upload
and copy back, the probabilities -- for `--runs` runs after one warm-up; the wall times of the two library calls on the same inputs, each
on its own, which show what share the existing permutation test has and what the new kernels' call costs; and, for comparison on the same
box, the time of the numpy restatement of the same definition (tests/gene_membership_cases.py; one thread) on every `--cpu-every`-th set,
whose statistics, counts and probabilities must equal the library's.  The library runs in a worker process of its own; every run has its
own time limit, and a run that exceeds it ends the worker and the measurement.

    python tools/measure_gene_membership.py --out profiles/gene_membership.json"""
import argparse
import json
import os
import pickle
import queue
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED = 42


def problem(small):
    """-> (raw result whose Z is the measured matrix, the sets as 0-based rows, numPerm)"""
    f = 10 if small else 1
    n, K, nSets, numPerm = 20000 // f, 50, 5000 // f, 500 // f
    rng = np.random.Generator(np.random.PCG64(2024))
    raw = {"Amean": rng.gamma(2.0, 1.0, size=(n, K)).astype(np.float32), "Asd": (0.2 + rng.random((n, K))).astype(np.float32),
           "Pmean": np.ones((2, K), dtype=np.float32), "Psd": np.ones((2, K), dtype=np.float32), "seed": SEED}
    sizes = rng.integers(15, 501, size=nSets)
    members = [np.sort(rng.choice(n, size=int(s), replace=False)).astype(np.uint32) for s in sizes]
    return raw, members, numPerm


def numpy_prob(Z, members, numPerm, which):
    """the restatement for the sets `which` (a set's draws are keyed by its index in the call) -> {t: (prob, stat, greaterCount)}"""
    import gene_membership_cases as gm
    import gene_set_cases as gc
    out = {}
    for t in which:
        mem = members[t].astype(np.int64)
        act = np.zeros(Z.shape[1])
        for i in mem:
            act = act + Z[i]
        act = act / np.float64(mem.size)
        idx = gc.draws(Z.shape[0], mem.size, SEED, t, np.arange(numPerm))
        acc = np.zeros((numPerm, Z.shape[1]))
        for j in range(mem.size):
            acc = acc + Z[idx[:, j]]
        count = (act[None, :] < acc / np.float64(mem.size)).sum(axis=0)
        _, _, w = gm.weights(count[None, :], numPerm)
        stat, cnt, _ = gm.membership(Z, [mem], w)
        prob = cnt[0] / np.float64(Z.shape[0] - mem.size)
        if gm.weight_sum(w[0]) < 1e-6:
            prob[:] = np.nan
        prob[np.isnan(stat[0])] = np.nan
        out[t] = (prob, stat[0], cnt[0])
    return out


def worker(a):
    """warm-up + runs of the front-end call, then of the two library calls on their own; one JSON line per call"""
    from cogaps_amd import CogapsResult, _capi
    lib = _capi.load()
    raw, members, numPerm = problem(a.small)
    res = CogapsResult(raw)
    sets = [(m.astype(np.int64) + 1).tolist() for m in members]
    print(json.dumps({"ready": True, "source_hash": lib.cogaps_source_hash().decode()}), flush=True)
    for i in range(a.runs + 1):
        t0 = time.perf_counter()
        out = res.computeGeneGSProb(sets, numPerm=numPerm, lib=lib)
        dt = time.perf_counter() - t0
        print(json.dumps({"run": i, "seconds": round(dt, 4)}), flush=True)
    which = list(range(0, len(members), a.cpu_every))
    with open(a.worker, "wb") as fh:
        pickle.dump({t: (out["prob"][t], out["stat"][t], out["greaterCount"][t]) for t in which}, fh)
    z, sizes = res.calcZ(), [int(m.size) for m in members]
    for i in range(a.runs + 1):
        t0 = time.perf_counter()
        count, _ = _capi.gene_set_stat(z, members, sizes, numPerm, seed=SEED, lib=lib)
        t1 = time.perf_counter()
        w = -np.log(np.maximum(count, 1) / float(numPerm))
        t2 = time.perf_counter()
        _capi.gene_set_membership(z, members, w, lib=lib)
        t3 = time.perf_counter()
        print(json.dumps({"run": i, "gene_set_stat_s": round(t1 - t0, 4), "gene_set_membership_s": round(t3 - t2, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds one call may take")
    ap.add_argument("--setup-limit", type=float, default=300.0, help="seconds the worker may take to load the library and make the problem")
    ap.add_argument("--cpu-every", type=int, default=100, help="the numpy comparison takes every n-th set")
    ap.add_argument("--small", action="store_true", help="a tenth of each dimension (a dry run of the tool)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    raw, members, numPerm = problem(a.small)
    n, K = raw["Amean"].shape
    nMem = int(sum(m.size for m in members))
    out = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "shape": {"rows": n, "patterns": K, "sets": len(members), "numPerm": numPerm,
           "set_sizes": [min(m.size for m in members), max(m.size for m in members)], "multiply_adds": 2 * len(members) * n * K,
           "comparisons": int(sum(int(m.size) * (n - int(m.size)) for m in members)), "members": nMem}, "runs": a.runs}
    answer_file = os.path.join(os.path.dirname(os.path.abspath(a.out)) if a.out else ROOT, ".gene_membership_answer.pkl")
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", answer_file, "--runs", str(a.runs), "--cpu-every", str(a.cpu_every)] + (["--small"] if a.small else [])
    child = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
    lines = queue.Queue()
    threading.Thread(target=lambda: [lines.put(ln) for ln in child.stdout] + [lines.put(None)], daemon=True).start()
    records, limit = [], a.setup_limit
    try:
        while len(records) < 2 * (a.runs + 1) + 1:
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
    front, parts = records[1:a.runs + 2], records[a.runs + 2:]
    out["source_hash"] = records[0]["source_hash"]
    out["warm_up_s"] = front[0]["seconds"]
    out["computeGeneGSProb_s"] = [r["seconds"] for r in front[1:]]
    out["gene_set_stat_call_s"] = [r["gene_set_stat_s"] for r in parts[1:]]
    out["gene_set_membership_call_s"] = [r["gene_set_membership_s"] for r in parts[1:]]
    out["permutation_test_share_of_wall"] = round(min(out["gene_set_stat_call_s"]) / min(out["computeGeneGSProb_s"]), 3)
    with open(answer_file, "rb") as fh:
        got = pickle.load(fh)
    os.remove(answer_file)
    # the same definition in numpy on a fraction of the sets, and the check that both computed the same
    from cogaps_amd import CogapsResult
    Z = CogapsResult(raw).calcZ()
    which = sorted(got)
    t0 = time.perf_counter()
    ref = numpy_prob(Z, members, numPerm, which)
    dt = time.perf_counter() - t0
    for t in which:
        for x, y, name in zip(ref[t], got[t], ("prob", "stat", "greaterCount")):
            assert np.array_equal(x, y, equal_nan=True), "set %d: the library's %s differs from numpy's" % (t, name)
    out["numpy"] = {"sets": len(which), "of": len(members), "seconds": round(dt, 3), "threads": 1, "cpus_available": len(os.sched_getaffinity(0)),
                    "outputs_equal_the_library's": True}
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
