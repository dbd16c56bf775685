"""The configurations of the sequential sampler's recorded reference runs (tests/golden/refprobe_sequential_outputs.npz), shared by
tools/refprobe/record_sequential.py, which records them from the reference build, and by tests/test_sequential_sampler*.py, which
compare the library with the recording.  Nothing here needs the reference sources or tools/refprobe."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RECORD = os.path.join(GOLDEN, "refprobe_sequential_outputs.npz")

# the reference's own arithmetic: one accumulator per sum, glibc's logf / expf
SEQ = dict(reductionMode="seq", mathMode="glibc-fma", sampler="sequential")


def tiny_matrix():
    """5 x 6: so few bins that the domain falls below two atoms (births without a draw), loses its highest atom (an exchange wraps to
    front()) and erases the atom at the last index (no swap) many times in 100 + 100 iterations"""
    i, j = np.meshgrid(np.arange(5), np.arange(6), indexing="ij")
    return np.ascontiguousarray(((i * 7 + j * 3) % 5) * 0.5 * ((i + j) % 3 != 0) + 0.05, dtype=np.float32)


def fixed_p():
    """the fixed P of the worker-subset case: GIST's 9 samples x 3 patterns"""
    s, k = np.meshgrid(np.arange(9), np.arange(3), indexing="ij")
    return np.ascontiguousarray(0.25 + ((s * 5 + k * 3) % 7) * 0.5 * ((s + k) % 4 != 0), dtype=np.float32)


def synthetic_6000x8():
    """6000 x 8, rank 3: the P sampler's data vectors have 6000 elements (N > 4096: reduction width 2048, two virtual lanes per thread)"""
    g = np.random.Generator(np.random.MT19937(6000))
    a = g.gamma(2.0, 0.5, (6000, 3)) * (g.random((6000, 3)) > 0.3)
    p = g.gamma(2.0, 0.5, (3, 8))
    return np.ascontiguousarray((a @ p) * (0.9 + 0.2 * g.random((6000, 8))) + 0.01, dtype=np.float32)


def cases(gist, modsim):
    """name -> (data, keyword arguments of _capi.run without the arithmetic and the sampler)"""
    rows300 = np.arange(1, 301, dtype=np.uint32)
    return {
        "modsim_k3": (modsim, dict(nPatterns=3, seed=42, nIterations=100, outputFrequency=10)),
        "gist_k7": (gist, dict(nPatterns=7, seed=42, nIterations=30, outputFrequency=10)),
        "gist_rows300_k3": (gist, dict(nPatterns=3, seed=5, nIterations=50, outputFrequency=10, subsetIndices=rows300, subsetDim=1)),
        "gist_rows300_k3_fixedP": (gist, dict(nPatterns=3, seed=5, nIterations=50, outputFrequency=10, subsetIndices=rows300, subsetDim=1,
                                              whichMatrixFixed="P", fixedPatterns=fixed_p())),
        "tiny_5x6_k2": (tiny_matrix(), dict(nPatterns=2, seed=7, nIterations=100, outputFrequency=5)),
        "gist_k4_pump_snapshots": (gist, dict(nPatterns=4, seed=42, nIterations=40, outputFrequency=10, takePumpSamples=True, nSnapshots=2,
                                              snapshotPhase="all")),
    }


def fnv_matrix(m):
    """the recording's hash of a matrix: FNV-1a 64 over the float32 bit patterns, row-major, little-endian bytes"""
    h = 1469598103934665603
    for b in np.ascontiguousarray(m, dtype="<f4").tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def load_record(path=RECORD):
    """case name -> {field: array}; fields as the recorder wrote them (atomsA, atomsP, chisq, totalUpdates, meanChiSq, qA, qP,
    row|<matrix>|<r>, hash|<matrix>, snapE, snapS)"""
    out = {}
    with np.load(path) as z:
        for key in z.files:
            name, field = key.split("|", 1)
            out.setdefault(name, {})[field] = z[key]
    return out


def compare_with_record(ref, o):
    """every recorded value against a result of _capi.run, bit for bit (the reference build prints %.9g, which identifies an fp32 value)"""
    assert ref["atomsA"].tolist() == o["atomsA"].tolist(), (ref["atomsA"].tolist(), o["atomsA"].tolist())
    assert ref["atomsP"].tolist() == o["atomsP"].tolist(), (ref["atomsP"].tolist(), o["atomsP"].tolist())
    assert int(ref["totalUpdates"]) == o["totalUpdates"]
    assert np.array_equal(ref["chisq"], o["chisq"].astype(np.float32)), (ref["chisq"], o["chisq"])
    assert np.float32(ref["meanChiSq"]) == np.float32(o["meanChiSq"]), (ref["meanChiSq"], o["meanChiSq"])
    # SingleThreadedGibbsSampler::getAverageQueueLength
    assert float(ref["qA"]) == 0.0 and float(ref["qP"]) == 0.0 and o["averageQueueLengthA"] == 0.0 and o["averageQueueLengthP"] == 0.0
    for name in ("Amean", "Asd", "Pmean", "Psd"):
        for field, vals in ref.items():
            if field.startswith("row|%s|" % name):
                assert np.array_equal(vals, o[name][int(field.split("|")[2])]), field
        h, cnt = (int(x) for x in ref["hash|" + name])
        assert cnt == o[name].size and h == fnv_matrix(o[name]), name
    if "hash|pump" in ref:
        assert int(ref["hash|pump"][0]) == fnv_matrix(o["pumpMatrix"]) and int(ref["hash|meanPattern"][0]) == fnv_matrix(o["meanPatternAssignment"])
    assert len(ref["snapE"]) == o["equilibrationSnapshotsA"].shape[0] and len(ref["snapS"]) == o["samplingSnapshotsA"].shape[0]
    for k, (ha, hp) in enumerate(ref["snapE"]):
        assert int(ha) == fnv_matrix(o["equilibrationSnapshotsA"][k]) and int(hp) == fnv_matrix(o["equilibrationSnapshotsP"][k])
    for k, (ha, hp) in enumerate(ref["snapS"]):
        assert int(ha) == fnv_matrix(o["samplingSnapshotsA"][k]) and int(hp) == fnv_matrix(o["samplingSnapshotsP"][k])
