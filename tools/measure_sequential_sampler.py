#!/usr/bin/env python3
"""The sequential sampler (sampler="sequential", csrc/seq_kernel.h) on one MI355X at BASELINE configs[2]'s shard size (20000 x 2000,
dense model, K = 50): one chain, and batches of 8 and 32 chains (one launch, a workgroup per chain).  Per row: proposals per second
over `--iterations` equilibration iterations after `--warmup` (host clock around the call, which synchronises), and the mean duration
of a launch from the HIP events the library attaches to its launches (cogaps_session_set_timing / cogaps_batch_set_timing).

    python tools/measure_sequential_sampler.py --out profiles/sequential_sampler.json"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--chains", type=int, nargs="*", default=[1, 8, 32])
    ap.add_argument("--small", action="store_true", help="a tenth of each dimension (a dry run of the tool)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    from cogaps_amd import _capi
    lib = _capi.load()
    f = 10 if a.small else 1
    genes, samples = 20000 // f, 2000 // f
    data = bench.synthetic_dense(genes, samples)
    out = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "source_hash": lib.cogaps_source_hash().decode(), "shape": [genes, samples], "nPatterns": 50,
           "warmup": a.warmup, "iterations": a.iterations, "rows": []}
    for chains in a.chains:
        ss = [_capi.Session(data, lib=lib, nPatterns=50, nIterations=1000, seed=42 + c, sampler="sequential") for c in range(chains)]
        b = _capi.Batch(ss) if chains > 1 else None
        step = (lambda first, n: sum(b.run_iterations(1, first, n))) if b else (lambda first, n: ss[0].run_iterations(1, first, n))
        step(0, a.warmup)
        (b or ss[0]).set_timing(True)
        t0 = time.perf_counter()
        proposals = step(a.warmup, a.iterations)
        dt = time.perf_counter() - t0
        if b:
            perf = {w: b.perf(w) for w in "AP"}
            launch_us = {w: perf[w]["eval_us"] for w in "AP"}
            sampled = {w: perf[w]["sampled"] for w in "AP"}
        else:
            perf = {w: ss[0].perf(w) for w in "AP"}
            launch_us = {w: (1e3 * perf[w]["evalMs"] / perf[w]["evalTimed"] if perf[w]["evalTimed"] else 0.0) for w in "AP"}
            sampled = {w: perf[w]["evalTimed"] for w in "AP"}
        row = {"chains": chains, "proposals": int(proposals), "seconds": round(dt, 4), "proposals_per_s": round(proposals / dt, 1),
               "mean_launch_us": launch_us, "launches_sampled": sampled, "atoms": [ss[0].natoms("A"), ss[0].natoms("P")]}
        print(json.dumps(row), flush=True)
        out["rows"].append(row)
        if b:
            b.close()
        for s in ss:
            s.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
