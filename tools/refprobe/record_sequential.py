"""Record the reference build's SingleThreadedGibbsSampler (the probe's async=0) on the configurations of tests/sequential_cases.py
into tests/golden/refprobe_sequential_outputs.npz: printed results only, in the format of refprobe_outputs.npz.  Build container
only (the reference sources and a host compiler; CPU).

    python tools/refprobe/record_sequential.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import refprobe as rp              # noqa: E402
import sequential_cases as sc      # noqa: E402


def probe_arguments(tmp, name, data, kw):
    """_capi.run keywords -> the probe's (data path, keyword arguments)"""
    path = os.path.join(tmp, name + ".csv")
    rp.write_matrix(path, data)
    k = dict(nPatterns=kw["nPatterns"], nIterations=kw["nIterations"], seed=kw["seed"], outFreq=kw["outputFrequency"], threads=1, **{"async": 0})
    if "subsetIndices" in kw:
        sp = os.path.join(tmp, name + "_subset.txt")
        np.savetxt(sp, kw["subsetIndices"], fmt="%d")
        k.update(subsetDim=kw["subsetDim"], subset=sp)
    if kw.get("whichMatrixFixed", "N") != "N":
        fp = os.path.join(tmp, name + "_fixed.csv")
        rp.write_matrix(fp, kw["fixedPatterns"])
        k.update(fixed=kw["whichMatrixFixed"], fixedFile=fp)
    if kw.get("takePumpSamples"):
        k["pump"] = 1
    if kw.get("nSnapshots"):
        k.update(snapshots=kw["nSnapshots"], snapshotPhase={"equilibration": 1, "sampling": 2, "all": 3}[kw["snapshotPhase"]])
    return path, k


def main():
    import pyoracle
    binary = rp.build()
    gist = pyoracle.read_mtx(os.path.join(sc.GOLDEN, "GIST.mtx"))
    modsim = np.loadtxt(os.path.join(sc.GOLDEN, "modsimdata.csv"), delimiter=",").astype(np.float32)
    rec = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (data, kw) in sc.cases(gist, modsim).items():
            path, k = probe_arguments(tmp, name, data, kw)
            rec[name] = rp.run(binary, path, timeout=600, **k)
            print("%-28s atomsA %s atomsP %s totalUpdates %d" % (name, rec[name]["atomsA"].tolist()[-3:], rec[name]["atomsP"].tolist()[-3:], rec[name]["totalUpdates"]))
    rp.save_outputs(sc.RECORD, rec)
    print("%d outputs -> %s (%d bytes)" % (len(rec), os.path.relpath(sc.RECORD, ROOT), os.path.getsize(sc.RECORD)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
