"""Re-run the reference-build probe on every configuration whose reference-printed numbers are typed into tests/test_oracle_pin.py
(FINGERPRINTS: SURVEY 8c; REFERENCE_PRINTED: judge round 1; JUDGE_R2; JUDGE_R3) and compare / print them.  Build container only.

    python tools/refprobe/regen_fingerprints.py            # check every table entry except the two headline-sized ones
    python tools/refprobe/regen_fingerprints.py --all      # ... those as well (minutes)
    python tools/refprobe/regen_fingerprints.py --print NAME   # the probe's output for one entry, as the table would hold it
    python tools/refprobe/regen_fingerprints.py --record   # write tests/golden/refprobe_outputs.npz: the probe's output for every
                                                           # entry but the big ones and for the random configurations of the tests
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import refprobe as rp          # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
RECORD = os.path.join(GOLDEN, "refprobe_outputs.npz")


def _synthetic(tmp, name, d):
    p = os.path.join(tmp, name + ".csv")
    if not os.path.exists(p):
        rp.write_matrix(p, d)
    return p


BIG = ("r3_headline_18", "r3_headline_100", "r2_k50_dense", "r2_k50_sparse")


def cases(tmp, skip=()):
    """name -> (data path, probe keyword arguments incl. file-valued ones, table entry); the inputs of the names in `skip` are not written"""
    import bench
    import pyoracle
    import test_oracle_pin as T
    out = {}
    gist = pyoracle.read_mtx(os.path.join(GOLDEN, "GIST.mtx"))
    modsim_csv = os.path.join(tmp, "modsim.csv")
    rp.write_matrix(modsim_csv, np.loadtxt(os.path.join(GOLDEN, "modsimdata.csv"), delimiter=",").astype(np.float32))

    def kw_of(kw, threads=1):
        k = dict(nPatterns=kw["nPatterns"], nIterations=kw["nIterations"], seed=kw["seed"], outFreq=kw["outputFrequency"], threads=threads, sparse=bool(kw.get("sparseOptimization", False)))
        if "subsetIndices" in kw:
            sp = os.path.join(tmp, "subset_%d_%d.txt" % (kw["subsetDim"], len(kw["subsetIndices"])))
            np.savetxt(sp, kw["subsetIndices"], fmt="%d")
            k.update(subsetDim=kw["subsetDim"], subset=sp)
        return k
    for name, fp in T.FINGERPRINTS.items():
        data = os.path.join(GOLDEN, "GIST.mtx") if name == "gist" else modsim_csv
        out["survey_" + name] = (data, dict(nPatterns=fp["k"], nIterations=1000, seed=42, outFreq=100, threads=1), fp)
    for name, fp in T.REFERENCE_PRINTED.items():
        out["r1_" + name] = (os.path.join(GOLDEN, "GIST.mtx"), kw_of(fp["kw"]), fp)
    r2_files = {"gist_tsv_k3": os.path.join(GOLDEN, "GIST.tsv"), "gist_csv_sparse_k6": os.path.join(GOLDEN, "GIST.csv"), "modsim_sparse_k4": modsim_csv,
                "shard_round1": os.path.join(GOLDEN, "GIST.mtx")}
    for name, fp in T.JUDGE_R2.items():
        if name == "shard_round2" or "r2_" + name in skip:
            continue          # needs round 1's Pmean as a file: regen_shard_round2 below
        if name in r2_files:
            data = r2_files[name]
        else:
            data = _synthetic(tmp, name, T._judge_data(name, gist, None))
        out["r2_" + name] = (data, kw_of(fp["kw"]), fp)
    r3_files = {"gist_gct_k9": os.path.join(GOLDEN, "GIST.gct"), "gist_tsv_sparse_k11_samples": os.path.join(GOLDEN, "GIST.tsv"), "gist_csv_sparse_k4_genes": os.path.join(GOLDEN, "GIST.csv")}
    thr = {"gist_gct_k9": 3, "synth1500_k50_unc": 4, "headline_18": 8, "headline_100": 8}
    for name, fp in T.JUDGE_R3.items():
        if "r3_" + name in skip:
            continue
        d, unc = T._judge3_data(name, gist) if name not in r3_files else (None, None)
        data = r3_files.get(name) or _synthetic(tmp, name, d)
        k = kw_of(fp["kw"], thr.get(name, 1))
        if unc is not None:
            k["unc"] = _synthetic(tmp, name + "_unc", unc)
        out["r3_" + name] = (data, k, fp)
    return out


def check(ref, fp):
    """the typed numbers against the probe's output, to the digits that were typed"""
    ok = ref["atomsA"].tolist() == list(fp["atomsA"])
    if fp.get("atomsP") is not None:
        ok &= ref["atomsP"].tolist() == list(fp["atomsP"])
    if fp.get("totalUpdates") is not None:
        ok &= ref["totalUpdates"] == fp["totalUpdates"]
    def close(a, b, digits):
        return b is None or abs(float(a) - b) <= max(abs(b) * 10.0 ** (1 - digits), 6e-4 if digits < 9 else 0.0)
    digits = 9 if "qA" in fp and fp["qA"] is not None and len(repr(fp["qA"])) > 8 else 7
    ok &= close(ref["meanChiSq"], fp.get("meanChiSq"), digits)
    for k in ("qA", "qP"):      # (the survey's two entries give the queue lengths to one decimal)
        ok &= fp.get(k) is None or (close(ref[k], fp[k], 9) if digits == 9 else abs(float(ref[k]) - fp[k]) < 0.06)
    return bool(ok)


def main():
    big = () if ("--all" in sys.argv or "--print" in sys.argv) else BIG
    binary = rp.build()
    with tempfile.TemporaryDirectory() as tmp:
        cs = cases(tmp, skip=big)
        if "--print" in sys.argv:
            name = sys.argv[sys.argv.index("--print") + 1]
            data, kw, _ = cs[name]
            ref = rp.run(binary, data, **kw)
            print(name, "atomsA=%s, atomsP=%s, totalUpdates=%d, meanChiSq=%.9g, qA=%.9g, qP=%.9g, lastChisq=%.9g" % (ref["atomsA"].tolist(), ref["atomsP"].tolist(), ref["totalUpdates"], ref["meanChiSq"], ref["qA"], ref["qP"], ref["chisq"][-1]))
            return 0
        if "--record" in sys.argv:
            import test_oracle_pin as T
            rec = {name: rp.run(binary, data, **kw) for name, (data, kw, _) in cs.items()}
            for i in range(T.N_RANDOM_REFERENCE_CONFIGS):
                sub = os.path.join(tmp, "random_%d" % i)
                os.makedirs(sub)
                rec["random_%d" % i] = T.run_reference_config(rp, binary, T.random_reference_config(i), sub)[0]
            rp.save_outputs(RECORD, rec)
            print("%d outputs -> %s (%d bytes)" % (len(rec), os.path.relpath(RECORD, ROOT), os.path.getsize(RECORD)))
            return 0
        bad = 0
        for name, (data, kw, fp) in cs.items():
            ref = rp.run(binary, data, **kw)
            good = check(ref, fp)
            bad += not good
            print("%-36s %s   (%.1f s)" % (name, "ok" if good else "MISMATCH", ref["samplerSeconds"]))
        return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
