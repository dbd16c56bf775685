"""Golden vectors of the BENCHMARKED chains themselves, run end to end by the CPU oracle in the kernels' lane order (portable log /
exp, OpenMP over the queue): what `cogaps_run` on the MI355X must reproduce bit for bit, including the iterations bench.py times
(181-200 of the schedule).  The loop is runOnePhase's (reference src/GapsRunner.cpp:272-327).  Run in the build container on its
eight host cores:

  python tools/make_golden_c3.py            the dense chain (52.9 M proposals), measured 7 min
  python tools/make_golden_c3.py --sparse   the sparse chain (145.2 M proposals), measured 34 min (its first half shared the cores
                                            with a compile; the first 100 iterations took 8 min)

dense:  BASELINE configs[2] -- bench.synthetic_dense(20000, 2000), nPatterns = 50, seed 42, nIterations = 100 (+100),
        outputFrequency 10; reduction widths 512 / 8192 lanes x float4 -> tests/golden/c3_k50_s42_i100_lane.npz
sparse: BASELINE configs[4]'s per-GPU shard as `bench.py --sparse --genes 50000 --samples 12500` builds it for rank 0 --
        bench.synthetic_dense(50000, 12500) with 95 % of the entries zeroed by MT19937(777), sparseOptimization, the rest as
        above; reduction widths 4096 / 16384 (they set the lane order of the Z tables and of chi2)
        -> tests/golden/c4shard_k50_s42_i100_sparse_lane.npz

Both files hold
  stepsA / stepsP [200]     the Poisson step counts drawn per iteration (equilibration 0-99, sampling 100-199)
  natomsA / natomsP [200]   domain sizes after every iteration
  atomsA / atomsP / chisq   the histories at outputFrequency 10 (diagnostics$atomsA, $atomsP, $chisq)
  totalUpdates, meanChiSq, avgQueueA / avgQueueP
  sha256_{Amean,Pmean,Asd,Psd}, sha256 of the final atom positions / masses (vector order) and factor matrices
  sample_idx_* / sample_*   a fixed sample of the entries of the four statistics matrices (so that a mismatch can be located):
                            1 % of them (dense), 4096 per matrix (sparse)
dense only:   sha256_ap_{A,P}  the A*P caches
sparse only:  sha256_rows_{A,P}  the HybridMatrix row copies (sha256_matrix_* is the column copy); sha256_input, redW_A / redW_P
              (the sparse model keeps no A*P cache)
"""
import argparse
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyoracle as po  # noqa: E402
import bench  # noqa: E402

N_ITER = 100
DENSE = dict(out="c3_k50_s42_i100_lane.npz", genes=20000, samples=2000, redW_A=512, redW_P=8192, sparse=False)
SPARSE = dict(out="c4shard_k50_s42_i100_sparse_lane.npz", genes=50000, samples=12500, redW_A=4096, redW_P=16384, sparse=True)
SPARSE_SAMPLE = 4096


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def configs4_shard():
    """the input of `bench.py --sparse --genes 50000 --samples 12500` on rank 0 (bench.py's recipe, written out)"""
    data = bench.synthetic_dense(50000, 12500)
    data *= (np.random.Generator(np.random.MT19937(777)).random(data.shape) >= 0.95)
    return data


def final_state_digests(S, sparse=False):
    """digests of the chain state after the last iteration; S: any session with atoms / matrix / ap / rows (oracle or library).
    The sparse model has no A*P cache: both HybridMatrix copies instead."""
    out = {}
    for w in "AP":
        a = S.atoms(w)
        out["sha256_atoms_pos_" + w] = sha(a["pos"])
        out["sha256_atoms_mass_" + w] = sha(a["mass"])
        out["sha256_matrix_" + w] = sha(S.matrix(w))
        if sparse:
            out["sha256_rows_" + w] = sha(S.rows(w))
        else:
            out["sha256_ap_" + w] = sha(S.ap(w))
    return out


def run_golden(data, cfg, threads):
    O = po.Session(data, omp=True, maxThreads=threads, math_mode=po.MATH_PORTABLE, redW_A=cfg["redW_A"], redW_P=cfg["redW_P"], redG=4,
                   nPatterns=50, nIterations=N_ITER, seed=42, outputFrequency=10, sparseOptimization=cfg["sparse"])
    stepsA, stepsP, natA, natP = [], [], [], []
    t0 = time.time()
    for phase in (1, 2):
        for it in range(N_ITER):
            a, b = O.run_iterations(phase, it, 1)
            stepsA.append(int(a[0])), stepsP.append(int(b[0]))
            natA.append(O.natoms("A")), natP.append(O.natoms("P"))
            if it % 10 == 9:
                print("phase %d iteration %d: atoms %d / %d, %.0f s" % (phase, it + 1, natA[-1], natP[-1], time.time() - t0), flush=True)
    state = final_state_digests(O, cfg["sparse"])
    r = O.finish()
    O.close()
    assert r["totalUpdates"] == sum(stepsA) + sum(stepsP)
    rng = np.random.Generator(np.random.MT19937(20260929))
    extra = {}
    for f in ("Amean", "Pmean", "Asd", "Psd"):
        flat = r[f].ravel()
        n = SPARSE_SAMPLE if cfg["sparse"] else max(1, flat.size // 100)
        idx = np.sort(rng.choice(flat.size, size=n, replace=False)).astype(np.uint32)
        extra["sha256_" + f] = sha(r[f])
        extra["sample_idx_" + f] = idx
        extra["sample_" + f] = flat[idx].copy()
    if cfg["sparse"]:
        extra.update(sha256_input=sha(data), redW_A=np.uint32(cfg["redW_A"]), redW_P=np.uint32(cfg["redW_P"]))
    arrays = dict(stepsA=np.array(stepsA, np.uint32), stepsP=np.array(stepsP, np.uint32), natomsA=np.array(natA, np.uint32), natomsP=np.array(natP, np.uint32),
                  atomsA=r["atomsA"], atomsP=r["atomsP"], chisq=r["chisq"], totalUpdates=np.uint64(r["totalUpdates"]), meanChiSq=np.float32(r["meanChiSq"]),
                  avgQueueA=np.float32(r["averageQueueLengthA"]), avgQueueP=np.float32(r["averageQueueLengthP"]), **state, **extra)
    print("totalUpdates", r["totalUpdates"], "meanChiSq", r["meanChiSq"], "queue", r["averageQueueLengthA"], r["averageQueueLengthP"], "%.0f s" % (time.time() - t0))
    return arrays


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sparse", action="store_true", help="configs[4]'s shard (sparse model) instead of configs[2] (dense)")
    ap.add_argument("--out", default=None, help="write here instead of tests/golden/<name>.npz (to compare with the committed file)")
    args = ap.parse_args()
    cfg = SPARSE if args.sparse else DENSE
    data = configs4_shard() if args.sparse else bench.synthetic_dense(cfg["genes"], cfg["samples"])
    arrays = run_golden(data, cfg, min(8, os.cpu_count() or 1))
    out = args.out or os.path.join(ROOT, "tests", "golden", cfg["out"])
    np.savez_compressed(out, **arrays)
    print("written", out)


if __name__ == "__main__":
    main()
