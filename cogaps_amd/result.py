"""CogapsResult -- the numeric core of the reference's S4 result (R/class-CogapsResult.R): the four
factor matrices under their LinearEmbeddingMatrix names and the metadata list createCogapsResult fills
(R/methods-CogapsResult.R:8-20), and of its methods calcZ and calcCoGAPSStat -- the gene-set permutation statistic, computed on the GPU
(cogaps_gene_set_stat of include/cogaps_hip.h; DESIGN.md 4.8 has the definition, the draw and the deviations from R: the permutations
come from the library's keyed draw, not from R's sample() stream; a set none of whose members is a row gives NaN where R gives NA; a
set with one matching row uses that row where R fails), and patternMarkers -- every gene (or sample) ranked by its distance to each
pattern, and the marker lists, on the GPU as well (cogaps_pattern_markers; DESIGN.md 4.9: all-zero rows rank last and mark nothing
where R breaks on their NA, a column none of whose rows ranks better elsewhere gives every row where R fails, a wrong lp length is an
error), and reconstructGene, residuals -- plotResiduals' matrix, with the chi-square of every gene, every sample and the whole fit
beside it -- and binaryA: how well the result fits its data, on the GPU for dense and for sparse data, which is never densified
(cogaps_residuals; DESIGN.md 4.10: fp64 on the widened fp32 factors in fixed orders; the default uncertainty is R's pmax(0.1 * data,
0.1) in double; genes select rows in the order given where R's NULL means all), and getPatternGeneSet -- which gene sets go with which
pattern: the pre-ranked enrichment analysis of every set in every pattern with its permutation null on the GPU (cogaps_pattern_gsea;
DESIGN.md 4.11: ties rank in row order, the permutations are the keyed draw, the p-value is the simple one, a set that is not tested
is a NaN row where fgsea drops it), or the hypergeometric test of every set against patternMarkers' lists, and calcGeneGSStat and
computeGeneGSProb -- which genes of a set behave like the set: every gene's pattern-weighted statistic and the share of the genes
outside the set that exceed each member's, for any number of sets, on the GPU (cogaps_gene_set_membership; DESIGN.md 4.13: the weights
come from calcCoGAPSStat's counts, floored at 1 / numPerm where R's become infinite; one permutation test serves a set's members and
its null; fp64 in fixed orders), and toCSV / fromCSV, the eleven files of the reference's export, and MANOVA -- which patterns separate
the groups of the samples: manova of the factor-coded annotations on every pattern, from column means and centred sums of squares and
cross-products computed on the GPU in two passes (cogaps_manova_sscp; DESIGN.md 4.14: numpy's sort order for the levels, NaN for a
pattern without spread, a ValueError for a residual SSCP that is not positive definite), and the getters getOriginalParameters and
getVersion.  plotPatternGeneSet and the plots themselves are out of scope."""
import os
import re
import warnings

import numpy as np

_WHICH = {"featureLoadings": ("featureLoadings", "loadingStdDev", "geneNames"), "sampleFactors": ("sampleFactors", "factorStdDev", "sampleNames")}


def _is_index(x):
    return isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))


def _resolve_sets(sets, names, n, which):
    """-> (set names, per set the 0-based member rows ascending and unique, per set length(thisSet) as given)"""
    if isinstance(sets, dict):
        labels, groups = [str(k) for k in sets.keys()], list(sets.values())
    elif isinstance(sets, (list, tuple)):
        labels, groups = [str(i + 1) for i in range(len(sets))], list(sets)
    else:
        raise ValueError("sets must be a list of either measurements or samples")
    if not groups:
        raise ValueError("sets is empty")
    out = []
    for g in groups:
        if isinstance(g, (str, bytes)) or not hasattr(g, "__iter__"):
            raise ValueError("sets must be a list of either measurements or samples")
        out.append([x.item() if isinstance(x, np.generic) else x for x in g])
    flat = [x for g in out for x in g]
    by_name = [isinstance(x, str) for x in flat]
    if not all(by_name) and not all(_is_index(x) for x in flat):
        raise ValueError("sets must be all index sets or all name sets")
    if flat and all(by_name):
        if names is None:
            raise ValueError("sets holds names but the result carries no %s" % _WHICH[which][2])
        lookup = {}
        for i, nm in enumerate(names):
            lookup.setdefault(nm, []).append(i)
        members = [np.unique(np.array([i for x in set(g) for i in lookup.get(x, ())], dtype=np.int64)) for g in out]      # rownames %in% thisSet
    else:
        if any(x < 1 or x > n for x in flat):
            raise ValueError("sets holds an index outside 1 .. %d" % n)
        members = [np.unique(np.array(g, dtype=np.int64) - 1) for g in out]
    sizes = [len(g) for g in out]
    for lab, sz in zip(labels, sizes):
        if sz == 0:
            raise ValueError("set %s is empty" % lab)
        if sz > n:
            raise ValueError("set %s has %d entries, the matrix %d rows: no draw without replacement" % (lab, sz, n))
    return labels, members, sizes


def _benjamini_hochberg(p):
    """p.adjust(p, "BH") over the entries that are not NaN (a set that was not tested stays NaN and does not count)"""
    out = np.full(p.shape, np.nan)
    ok = np.flatnonzero(~np.isnan(p))
    if ok.size:
        down = ok[np.argsort(-p[ok], kind="stable")]
        out[down] = np.minimum(1.0, np.minimum.accumulate(p[down] * ok.size / np.arange(ok.size, 0, -1)))
    return out


_MANOVA_TESTS = ("Pillai", "Wilks", "Hotelling-Lawley", "Roy")
_MANOVA_PIVOT = 1e-12      # below this a pivot of the unit-diagonal Cholesky factorisation, or 1 - Pillai's trace, counts as zero


def _annotation_columns(annotations, columns, n, which):
    """the used columns of MANOVA's interestedVariables, each a 1-D numpy array of n entries"""
    if isinstance(columns, (int, np.integer)) and not isinstance(columns, (bool, np.bool_)):
        columns = (columns,)
    columns = list(columns)
    if not 1 <= len(columns) <= 8 or not all(_is_index(c) for c in columns):
        raise ValueError("columns must name one to eight columns of interestedVariables by their 0-based index")
    if hasattr(annotations, "iloc") and hasattr(annotations, "columns"):         # a pandas DataFrame
        shape, take = annotations.shape, lambda c: annotations.iloc[:, c].to_numpy()
    else:
        table = annotations if isinstance(annotations, np.ndarray) else np.array([list(r) if hasattr(r, "__iter__") and not isinstance(r, (str, bytes)) else r
                                                                               for r in annotations], dtype=object)
        if table.ndim != 2:
            raise ValueError("interestedVariables must have two dimensions: one row per %s, one column per variable" % ("sample" if which == "sampleFactors" else "gene"))
        shape, take = table.shape, lambda c: table[:, c]
    if shape[0] != n:
        raise ValueError("interestedVariables has %d rows, the %s %d" % (shape[0], which, n))
    for c in columns:
        if not 0 <= c < shape[1]:
            raise ValueError("column %d is outside the %d columns of interestedVariables" % (c, shape[1]))
    return [take(int(c)) for c in columns]


def _is_missing(col):
    """where a column of annotations holds None, a NaN or pandas' NA / NaT"""
    if col.dtype.kind in "fc":
        return np.isnan(col)
    if col.dtype.kind == "O":
        return np.array([v is None or (isinstance(v, (float, np.floating)) and v != v) or type(v).__name__ in ("NAType", "NaTType") for v in col], dtype=bool)
    if col.dtype.kind in "mM":
        return np.isnat(col)
    return np.zeros(col.shape[0], dtype=bool)


def _factor_codes(col):
    """unclass(factor(col)): -> (the 1-based index of every value among the sorted distinct values as float64, those values)"""
    try:
        levels, inverse = np.unique(col, return_inverse=True)
    except TypeError:
        raise ValueError("a column of interestedVariables holds values that do not sort against one another")
    return (inverse.reshape(-1) + 1).astype(np.float64), levels


def _unit_cholesky(S):
    """S [p][p] symmetric -> (L, rank): C = S scaled to a unit diagonal, C = L L^T row by row; a diagonal entry of S that is not
    positive, or a pivot below _MANOVA_PIVOT, drops its row and column from the factorisation and from the rank (L is then no factor)"""
    p = S.shape[0]
    d = np.diag(S)
    live = [j for j in range(p) if d[j] > 0]
    L, kept = np.zeros((p, p)), []
    for j in live:
        row = np.zeros(p)
        for m in kept:
            acc = S[j, m] / np.sqrt(d[j] * d[m])
            for q in kept:
                if q >= m:
                    break
                acc = acc - row[q] * L[m, q]
            row[m] = acc / L[m, m]
        pivot = 1.0
        for m in kept:
            pivot = pivot - row[m] * row[m]
        if pivot < _MANOVA_PIVOT:
            continue
        row[j] = np.sqrt(pivot)
        L[j] = row
        kept.append(j)
    return L, len(kept)


def _data_input(data, uncertainty, lib):
    """data (and its uncertainty, or None) as the C layer takes them, under CoGAPS()'s input checks: a path is read (.mtx as triplets,
    kept sparse), a dense matrix becomes float32, a sparse one takes no uncertainty"""
    from . import _capi
    from .api import check_values, warn_small_uncertainty
    from .io import read_matrix
    if isinstance(data, str):
        data = _capi.read_mtx_triplets(data, lib=lib) if data.lower().endswith(".mtx") else read_matrix(data)
    if isinstance(uncertainty, str):
        uncertainty = read_matrix(uncertainty)
    sparse = isinstance(data, (_capi.SparseMatrix, _capi.CooMatrix, _capi.DeviceMatrix)) or _capi.is_sparse(data)
    if sparse and uncertainty is not None:
        raise ValueError("a sparse matrix takes no uncertainty matrix: the default uncertainty only")
    if _capi.is_sparse(data):
        data = data.astype(np.float32)
    elif not sparse and not _capi.is_tensor(data):
        data = np.asarray(data, dtype=np.float32)
    if uncertainty is not None and not _capi.is_tensor(uncertainty):
        uncertainty = np.asarray(uncertainty, dtype=np.float32)
    check_values(data, uncertainty)               # CoGAPS()'s own: NA, negative values ...
    warn_small_uncertainty(uncertainty)           # ... and the warning for uncertainties below 1e-5
    return data, uncertainty


def _project(loadings, loadingsNames, data, dataNames, NP, full, transposeData, lib):
    """projectR's lmFit route: the fit on the GPU, sigma, t and the normal tail in float64 on the host"""
    from . import _capi
    from scipy.special import erfc
    L = np.asarray(loadings, dtype=np.float32)
    if L.ndim != 2:
        raise ValueError("the loadings must be a matrix (genes x patterns)")
    labels = ["Pattern_%d" % (k + 1) for k in range(L.shape[1])]
    if NP is not None:
        if isinstance(NP, (str, bytes)) or not hasattr(NP, "__iter__"):
            NP = [NP]
        flat = [x.item() if isinstance(x, np.generic) else x for x in NP]
        if not flat:
            raise ValueError("NP is empty")
        if all(isinstance(x, str) for x in flat):
            if any(x not in labels for x in flat):
                raise ValueError("unknown pattern name: %s" % [x for x in flat if x not in labels][0])
            cols = [labels.index(x) for x in flat]
        elif all(_is_index(x) for x in flat):
            if any(x < 1 or x > L.shape[1] for x in flat):
                raise ValueError("NP holds an index outside 1 .. %d" % L.shape[1])
            cols = [int(x) - 1 for x in flat]
        else:
            raise ValueError("NP must be all indices or all names")
        L, labels = L[:, cols], [labels[c] for c in cols]
    K = L.shape[1]
    data, _ = _data_input(data, None, lib)
    nData = int(tuple(data.shape)[1 if transposeData else 0])
    if dataNames is None:
        if nData != L.shape[0]:
            raise ValueError("projectR: the data has %d genes, the loadings have %d: give dataNames to match them by name" % (nData, L.shape[0]))
        rows, matched = None, (list(loadingsNames) if loadingsNames is not None else list(range(1, L.shape[0] + 1)))
    else:
        if loadingsNames is None:
            raise ValueError("projectR: dataNames are given but the loadings carry no gene names")
        if len(dataNames) != nData or len(loadingsNames) != L.shape[0]:
            raise ValueError("projectR: one name per gene: %d names for %d genes of the data, %d for %d of the loadings"
                             % (len(dataNames), nData, len(loadingsNames), L.shape[0]))
        first = {}
        for r, nm in enumerate(dataNames):
            first.setdefault(nm, r)                   # a duplicated name keeps its first row
        keep = [i for i, nm in enumerate(loadingsNames) if nm in first]      # the intersection, in the loadings' order
        if len(keep) < K + 1:
            raise ValueError("projectR: %d genes matched by name, %d patterns need at least %d" % (len(keep), K, K + 1))
        L, matched = L[keep], [loadingsNames[i] for i in keep]
        rows = np.array([first[nm] for nm in matched], dtype=np.uint32)
    fit = _capi.project(L, data, rows=rows, transposeData=transposeData, lib=lib)
    df = L.shape[0] - K
    with np.errstate(invalid="ignore", divide="ignore"):
        sigma = np.sqrt(fit["rss"] / df)
        t = fit["coef"] / fit["stdevUnscaled"][:, None] / sigma[None, :]
        pval = erfc(np.abs(t) / np.sqrt(2.0))
    out = {"projection": fit["coef"], "pval": pval}
    if full:
        out.update({"t": t, "sigma": sigma, "stdevUnscaled": fit["stdevUnscaled"], "df": df, "rss": fit["rss"], "gram": fit["gram"],
                    "genesMatched": matched, "patterns": labels})
    return out


class CogapsResult:
    def __init__(self, raw, params=None, geneNames=None, sampleNames=None):
        self.featureLoadings = np.asarray(raw["Amean"])      # Amean
        self.loadingStdDev = np.asarray(raw["Asd"])          # Asd
        self.sampleFactors = np.asarray(raw["Pmean"])        # Pmean
        self.factorStdDev = np.asarray(raw["Psd"])           # Psd
        self.geneNames = geneNames
        self.sampleNames = sampleNames
        diag = {k: raw[k] for k in ("chisq", "atomsA", "atomsP", "averageQueueLengthA", "averageQueueLengthP",
                                    "totalUpdates", "totalRunningTime") if k in raw}
        # Cogaps.cpp:176-185: pumpStat, meanPatternAssignment, the four snapshot lists
        if "pumpMatrix" in raw:
            diag["pumpStat"] = raw["pumpMatrix"]; diag["meanPatternAssignment"] = raw["meanPatternAssignment"]
        for k in ("equilibrationSnapshotsA", "equilibrationSnapshotsP", "samplingSnapshotsA", "samplingSnapshotsP"):
            if k in raw:
                diag[k] = list(raw[k])
        for k in ("firstPass", "unmatchedPatterns", "clusteredPatterns", "CorrToMeanPattern", "subsets", "consensus"):
            if k in raw:
                diag[k] = raw[k]
        self.metadata = {"meanChiSq": raw.get("meanChiSq"), "seed": raw.get("seed"), "diagnostics": diag, "params": params}

    # R/methods-CogapsResult.R getters
    def getFeatureLoadings(self):
        return self.featureLoadings

    def getSampleFactors(self):
        return self.sampleFactors

    def getAmplitudeMatrix(self):
        return self.featureLoadings

    def getPatternMatrix(self):
        return self.sampleFactors

    def getMeanChiSq(self):
        return self.metadata["meanChiSq"]

    def getSubsets(self):
        return self.metadata["diagnostics"].get("subsets")

    def getUnmatchedPatterns(self):
        return self.metadata["diagnostics"].get("unmatchedPatterns")

    def getClusteredPatterns(self):
        return self.metadata["diagnostics"].get("clusteredPatterns")

    def getCorrelationToMeanPattern(self):
        """per cluster the rounded correlation of every member with the cluster's mean pattern (a distributed run's; else None)"""
        return self.metadata["diagnostics"].get("CorrToMeanPattern")

    def calcZ(self, whichMatrix="featureLoadings"):
        """R/methods-CogapsResult.R:220-231: mean / standard deviation of the chosen matrix in float64; a zero deviation becomes 1e-6"""
        if whichMatrix not in _WHICH:
            raise ValueError("whichMatrix must be either 'featureLoadings' or 'sampleFactors'")
        mean = np.asarray(getattr(self, _WHICH[whichMatrix][0]), dtype=np.float64)
        sd = np.array(getattr(self, _WHICH[whichMatrix][1]), dtype=np.float64)
        if (sd == 0).any():
            warnings.warn("zeros detected in the standard deviation matrix")
            sd[sd == 0] = 1e-6
        return mean / sd

    def calcCoGAPSStat(self, sets=None, whichMatrix="featureLoadings", numPerm=1000, seed=None, GStoGenes=None, lib=None):
        """R/methods-CogapsResult.R:499-531 on the GPU: for every set the share of numPerm random row sets of its size whose mean Z
        exceeds the set's own, per pattern.  sets: a dict name -> members, or a list of member lists (named "1", "2", ...); members are
        row names (geneNames for featureLoadings, sampleNames for sampleFactors) or 1-based row indices, never both.  GStoGenes: the
        reference's older name of `sets`.  seed keys the draws (default: the run's seed).  -> {"twoSidedPValue", "GSUpreg", "GSDownreg",
        "GSActEst"}: arrays [nPatterns][nSets], and "sets": the set names in order.  A set none of whose members is a row: NaN."""
        from . import _capi
        if GStoGenes is not None:
            sets = GStoGenes
        if isinstance(numPerm, bool) or not isinstance(numPerm, (int, np.integer)) or numPerm < 1 or numPerm > 0xFFFFFFFF:
            raise ValueError("numPerm must be a whole number of at least 1")
        z = self.calcZ(whichMatrix)
        labels, members, sizes = _resolve_sets(sets, getattr(self, _WHICH[whichMatrix][2]), z.shape[0], whichMatrix)
        if seed is None:
            seed = self.metadata.get("seed") or 0
        count, _ = _capi.gene_set_stat(z, members, sizes, int(numPerm), seed=int(seed), lib=lib)
        up = count.T / float(numPerm)
        up[:, [m.size == 0 for m in members]] = np.nan
        down = 1.0 - up
        return {"twoSidedPValue": np.maximum(np.minimum(down, up), 1.0 / numPerm), "GSUpreg": up, "GSDownreg": down, "GSActEst": 1.0 - 2.0 * up, "sets": labels}

    def _gene_set_weights(self, sets, numPerm, Pw, seed, lib):
        """what calcGeneGSStat and computeGeneGSProb start from -> (Z, set names, member rows per set, GSUpreg
        [nSets][K] floored at 1 / numPerm, g = -log(GSUpreg), w = g * Pw -- g itself without a weighting)"""
        from . import _capi
        if isinstance(numPerm, bool) or not isinstance(numPerm, (int, np.integer)) or numPerm < 1 or numPerm > 0xFFFFFFFF:
            raise ValueError("numPerm must be a whole number of at least 1")
        z = self.calcZ("featureLoadings")
        labels, members, sizes = _resolve_sets(sets, self.geneNames, z.shape[0], "featureLoadings")
        if Pw is not None:
            Pw = np.asarray(Pw, dtype=np.float64).reshape(-1)
            if np.isnan(Pw).all():
                Pw = None                                                        # R: all(is.na(Pw)) means no weighting
            elif Pw.size != z.shape[1]:
                raise ValueError("Invalid weighting")
        if seed is None:
            seed = self.metadata.get("seed") or 0
        count, _ = _capi.gene_set_stat(z, members, sizes, int(numPerm), seed=int(seed), lib=lib)
        up = np.maximum(count, 1) / float(numPerm)
        g = -np.log(up)
        return z, labels, members, up, g, g if Pw is None else g * Pw[None, :]

    def _row_labels(self, rows):
        return [self.geneNames[i] for i in rows] if self.geneNames is not None else [int(i) + 1 for i in rows]

    def calcGeneGSStat(self, sets=None, numPerm=500, Pw=None, nullGenes=False, seed=None, GStoGenes=None, lib=None):
        """R/methods-CogapsResult.R:535-569 on the GPU, for any number of sets: the statistic T of the genes of every set (nullGenes:
        of the genes outside it) -- the gene's Z over the patterns, weighted by how active the set is in each pattern (-log GSUpreg of
        calcCoGAPSStat with numPerm permutations, GSUpreg floored at 1 / numPerm, times Pw if given: one weight per pattern), over the
        weights' sum and over the gene's plain sum of Z; 0 where either sum is below 1e-6.  sets, seed: as for calcCoGAPSStat;
        GStoGenes: the reference's name of `sets`.  -> {"sets": the set names, "genes": per set the rows' names (1-based indices if the
        result carries none) in ascending row order, "stat": per set their float64 T}.  DESIGN.md 4.13 has every deviation from R."""
        from . import _capi
        z, labels, members, _, _, w = self._gene_set_weights(GStoGenes if GStoGenes is not None else sets, numPerm, Pw, seed, lib)
        out = _capi.gene_set_membership(z, members, w, stat=not nullGenes, counts=False, allStat=bool(nullGenes), lib=lib)
        if nullGenes:
            rows = [np.setdiff1d(np.arange(z.shape[0], dtype=np.int64), m) for m in members]
            stat = [out["allStat"][t, r] for t, r in enumerate(rows)]
        else:
            rows = members
            stat = [out["memberStat"][out["offsets"][t]:out["offsets"][t + 1]].copy() for t in range(len(members))]
        return {"sets": labels, "genes": [self._row_labels(r) for r in rows], "stat": stat}

    def computeGeneGSProb(self, sets=None, numPerm=500, Pw=None, PwNull=False, seed=None, GStoGenes=None, lib=None):
        """R/methods-CogapsResult.R:571-594 on the GPU, for any number of sets: for every gene of a set the share of the genes outside
        the set whose statistic (calcGeneGSStat) is strictly greater than the gene's -- small for a gene that behaves like its set.
        The members' statistic is weighted by Pw; the null's as well if PwNull, else not (R's second call drops Pw).
        -> {"sets": the set names, "genes", "prob", "stat", "greaterCount": per set one entry per member in ascending row order (names
        or 1-based indices; float64; the members' T; int64), "nullSize": int64 [nSets], the rows outside each set, "GSUpreg": float64
        [nSets][K], the floored shares the weights were made from}.  prob is NaN for a member whose statistic is NaN, for a set whose
        weights sum to less than 1e-6 (the members' or the null's) and for a set that is every row.  A set none of whose members is
        a row gives empty arrays.  DESIGN.md 4.13 has every deviation from R."""
        from . import _capi
        z, labels, members, up, g, w = self._gene_set_weights(GStoGenes if GStoGenes is not None else sets, numPerm, Pw, seed, lib)
        wNull = None if PwNull or w is g else g
        out = _capi.gene_set_membership(z, members, w, wNull=wNull, lib=lib)
        inactive = np.zeros(len(members), dtype=bool)
        for v in (w,) if wNull is None else (w, wNull):
            W = np.zeros(len(members))
            for k in range(v.shape[1]):                                          # ascending k from +0, as the kernel adds
                W = W + v[:, k]
            inactive |= W < 1e-6
        nullSize = np.array([z.shape[0] - m.size for m in members], dtype=np.int64)
        stat, cnt, prob = [], [], []
        for t in range(len(members)):
            lo, hi = out["offsets"][t], out["offsets"][t + 1]
            stat.append(out["memberStat"][lo:hi].copy()); cnt.append(out["greaterCount"][lo:hi].astype(np.int64))
            with np.errstate(invalid="ignore", divide="ignore"):
                p = cnt[t] / np.float64(nullSize[t])
            p[np.isnan(stat[t])] = np.nan
            if inactive[t] or nullSize[t] == 0:
                p[:] = np.nan
            prob.append(p)
        return {"sets": labels, "genes": [self._row_labels(m) for m in members], "prob": prob, "stat": stat, "greaterCount": cnt,
                "nullSize": nullSize, "GSUpreg": up}

    def toCSV(self, save_location):
        """R/methods-CogapsResult.R:624-642: the result as eleven csv files in the directory save_location, under R's names -- the four
        matrices (a header of pattern names, a row per gene or sample), geneNames, sampleNames, meanChiSq, chisqHistory, version,
        atomsA, atomsP (a header "x", a value per line).  Numbers are written with the digits that read back to the same value; NA
        stands for a NaN and for what the result does not carry."""
        diag = self.metadata["diagnostics"]
        for name in ("featureLoadings", "sampleFactors", "loadingStdDev", "factorStdDev"):
            m = np.asarray(getattr(self, name))
            _csv_write(save_location, name, [",".join('"Pattern_%d"' % (k + 1) for k in range(m.shape[1]))] + [",".join(_csv_value(v) for v in row) for row in m])
        for name, v in (("geneNames", self.geneNames), ("sampleNames", self.sampleNames), ("meanChiSq", self.metadata.get("meanChiSq")),
                        ("chisqHistory", diag.get("chisq")), ("version", self.metadata.get("version")), ("atomsA", diag.get("atomsA")), ("atomsP", diag.get("atomsP"))):
            v = [None] if v is None else [v] if isinstance(v, (str, bytes)) or not hasattr(v, "__iter__") else list(v)
            _csv_write(save_location, name, ['"x"'] + [_csv_value(x) for x in v])

    def patternMarkers(self, threshold="all", lp=None, axis=1, lib=None):
        """R/methods-CogapsResult.R:397-494 on the GPU: the rows of featureLoadings (axis=1: genes) or sampleFactors (axis=2: samples),
        scaled by the other matrix's column maxima and normalised by their own maximum, scored by their distance to each pattern vector
        and ranked per pattern (ties in row order).  lp: a dict name -> vector or a list of vectors of nPatterns entries, none above 1;
        None: the unit vectors, one per pattern.  threshold "all": every row marks the pattern it ranks best in; "cut": a pattern's
        markers are its best rows up to the first that ranks better elsewhere.  -> {"PatternMarkers": label -> list of row names (1-based
        indices if the result carries no names), "PatternRanks": int [rows][L], "PatternScores": float64 [rows][L], "patterns": the labels}"""
        return self._pattern_markers(threshold, lp, axis, lib)[0]

    def _pattern_markers(self, threshold, lp, axis, lib):
        """-> (what patternMarkers returns, per label the markers' 0-based rows)"""
        from . import _capi
        if axis == 1:
            A, O, names = self.featureLoadings, self.sampleFactors, self.geneNames
        elif axis == 2:
            A, O, names = self.sampleFactors, self.featureLoadings, self.sampleNames
        else:
            raise ValueError("axis must be 1 or 2")
        if threshold not in ("all", "cut"):
            raise ValueError("threshold must be 'all' or 'cut'")
        A, O = np.asarray(A, dtype=np.float64), np.asarray(O, dtype=np.float64)
        K = A.shape[1]
        if lp is None:
            labels, vectors = ["Pattern_%d" % (k + 1) for k in range(K)], None
        else:
            if isinstance(lp, dict):
                labels, vectors = [str(k) for k in lp.keys()], list(lp.values())
            elif isinstance(lp, (list, tuple)):
                labels, vectors = [str(i + 1) for i in range(len(lp))], list(lp)
            else:
                raise ValueError("lp must be a list of vectors")
            if not vectors:
                raise ValueError("lp is empty")
            try:
                vectors = [np.asarray(v, dtype=np.float64).reshape(-1) for v in vectors]
            except (TypeError, ValueError):
                raise ValueError("lp must be a list of vectors")
            if any(v.size != K for v in vectors):
                raise ValueError("lp length must equal the number of columns of the Amatrix")
            if any(not (v <= 1).all() for v in vectors):
                raise ValueError("lp should be a list of vectors with max value of 1")
        ranks, scores, rows = _capi.pattern_markers(A, O, lp=vectors, threshold=threshold, lib=lib)
        if names is not None:
            lists = [[names[i] for i in r] for r in rows]
        else:
            lists = [[int(i) + 1 for i in r] for r in rows]
        return {"PatternMarkers": dict(zip(labels, lists)), "PatternRanks": ranks.astype(np.int64), "PatternScores": scores, "patterns": labels}, rows

    def getPatternGeneSet(self, sets=None, method="enrichment", whichMatrix="featureLoadings", numPerm=1000, minSize=1, maxSize=None,
                          seed=None, lib=None, **patternMarkerArgs):
        """R/methods-CogapsResult.R:300-344: which gene sets go with which pattern.  sets: as for calcCoGAPSStat (names or 1-based
        indices; a set's size is the number of its members that are rows).  A set of fewer than minSize or more than maxSize rows is
        not tested: NaN in every array, its size kept, no part in the adjustment.  DESIGN.md 4.11 has the definition and the
        deviations from fgsea.
        method "enrichment": the pre-ranked enrichment analysis (fgsea, scoreType = "pos") of every column of the chosen matrix, on the
        GPU, with numPerm keyed permutations per set (seed: default the run's).  maxSize: at most, and by default, the kernel's 4096; a
        set of all the rows is not tested either.  -> {"ES", "NES", "pval", "padj", "negLogPadj", "nMoreExtreme": [nPatterns][nSets];
        "size": [nSets]; "leadingEdge": [nPatterns][nSets] lists of row names (1-based indices if the result carries none) in rank
        order; "sets": the set names; "method"}.
        method "overrepresentation": the hypergeometric test (fgsea::fora) of every set against the marker list of every pattern;
        patternMarkerArgs (threshold, lp) go to patternMarkers, which runs on the GPU.  maxSize: default the reference's 2038.
        -> {"overlap", "pval", "padj", "negLogPadj", "k/K": [L][nSets]; "size"; "overlapGenes": [L][nSets] lists; "sets"; "patterns":
        the marker lists' labels; "method"}."""
        from . import _capi
        if method not in ("enrichment", "overrepresentation"):
            raise ValueError("method must be 'enrichment' or 'overrepresentation'")
        if whichMatrix not in _WHICH:
            raise ValueError("whichMatrix must be either 'featureLoadings' or 'sampleFactors'")
        for name, v in (("minSize", minSize), ("maxSize", maxSize)):
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0):
                raise ValueError("%s must be a whole number" % name)
        stat = np.asarray(getattr(self, _WHICH[whichMatrix][0]), dtype=np.float32)
        names = getattr(self, _WHICH[whichMatrix][2])
        n = stat.shape[0]
        labels, members, _ = _resolve_sets(sets, names, n, whichMatrix)
        size = np.array([m.size for m in members], dtype=np.int64)
        label_of = (lambda i: names[i]) if names is not None else (lambda i: int(i) + 1)
        nSets = len(members)

        if method == "overrepresentation":
            if "axis" in patternMarkerArgs:
                raise ValueError("whichMatrix chooses the axis of patternMarkers")
            if maxSize is None:
                maxSize = 2038
            tested = (size >= max(int(minSize), 1)) & (size <= int(maxSize))
            pm, rows = self._pattern_markers(patternMarkerArgs.pop("threshold", "all"), patternMarkerArgs.pop("lp", None),
                                             1 if whichMatrix == "featureLoadings" else 2, lib)
            if patternMarkerArgs:
                raise TypeError("getPatternGeneSet: unexpected argument %s" % sorted(patternMarkerArgs)[0])
            L = len(rows)
            lf = np.concatenate([[0.0], np.cumsum(np.log(np.arange(1, n + 1, dtype=np.float64)))])      # lf[j] = log(j!)
            overlap, pval = np.full((L, nSets), np.nan), np.full((L, nSets), np.nan)
            genes = [[[] for _ in range(nSets)] for _ in range(L)]
            for l, marked in enumerate(rows):
                is_marker = np.zeros(n, dtype=bool)
                is_marker[marked] = True
                M = int(marked.size)
                for t in np.flatnonzero(tested):
                    hit = members[t][is_marker[members[t]]]
                    x, m = int(hit.size), int(size[t])
                    i = np.arange(max(x, m - (n - M)), min(M, m) + 1)                                 # the tail P(X >= x), term by term
                    logs = (lf[M] - lf[i] - lf[M - i]) + (lf[n - M] - lf[m - i] - lf[n - M - (m - i)]) - (lf[n] - lf[m] - lf[n - m])
                    terms = -np.sort(-np.exp(logs))                                                   # from the largest to the smallest
                    overlap[l, t], pval[l, t] = x, min(1.0, float(np.add.accumulate(terms)[-1])) if terms.size else 0.0
                    genes[l][t] = [label_of(g) for g in hit]
            padj = np.stack([_benjamini_hochberg(pval[l]) for l in range(L)])
            with np.errstate(divide="ignore"):
                return {"overlap": overlap, "pval": pval, "padj": padj, "negLogPadj": -10.0 * np.log10(padj), "k/K": overlap / size[None, :],
                        "size": size, "overlapGenes": genes, "sets": labels, "patterns": pm["patterns"], "method": method}

        if patternMarkerArgs:
            raise TypeError("getPatternGeneSet: unexpected argument %s (the enrichment method takes no patternMarkers arguments)" % sorted(patternMarkerArgs)[0])
        if isinstance(numPerm, bool) or not isinstance(numPerm, (int, np.integer)) or numPerm < 1 or numPerm >= 0xFFFFFFFF:
            raise ValueError("numPerm must be a whole number of at least 1")
        if maxSize is None:
            maxSize = _capi.GSEA_MAX_SET
        if maxSize > _capi.GSEA_MAX_SET:
            raise ValueError("maxSize = %d is above the %d members the enrichment kernel holds of one set" % (maxSize, _capi.GSEA_MAX_SET))
        if stat.size and not (stat >= 0).all():
            raise ValueError("the %s hold a NaN or a negative value: factor matrices are non-negative" % whichMatrix)
        if seed is None:
            seed = self.metadata.get("seed") or 0
        K = stat.shape[1]
        tested = np.flatnonzero((size >= max(int(minSize), 1)) & (size <= int(maxSize)) & (size < n))
        out = {k: np.full((K, nSets), np.nan) for k in ("ES", "NES", "pval", "padj", "negLogPadj", "nMoreExtreme")}
        edges = [[[] for _ in range(nSets)] for _ in range(K)]
        if tested.size:
            dev = _capi.pattern_gsea(stat, [members[t] for t in tested], int(numPerm), seed=int(seed), ranks=True, lib=lib)
            es, nGe = dev["es"].T, dev["nGe"].T.astype(np.float64)
            mean = dev["permSum"].T.astype(np.float64) / 2.0 ** 40 / float(numPerm)
            with np.errstate(invalid="ignore", divide="ignore"):
                nes = np.where(dev["permSum"].T == 0, np.nan, es / mean)
            pval = (nGe + 1.0) / (float(numPerm) + 1.0)
            out["ES"][:, tested], out["NES"][:, tested], out["pval"][:, tested], out["nMoreExtreme"][:, tested] = es, nes, pval, nGe
            out["padj"] = np.stack([_benjamini_hochberg(out["pval"][k]) for k in range(K)])
            out["negLogPadj"] = -10.0 * np.log10(out["padj"])
            for j, t in enumerate(tested):
                r = dev["rank"][:, members[t]]                                   # [K][m]
                by_rank = np.argsort(r, axis=1)
                for k in range(K):
                    edges[k][t] = [label_of(g) for g in members[t][by_rank[k, :int(dev["peak"][j, k]) + 1]]]
        out.update({"size": size, "leadingEdge": edges, "sets": labels, "method": method})
        return out

    def _gene_rows(self, genes):
        """-> (0-based rows in the order given, their labels); genes: names or 1-based indices, never both; None: every gene"""
        G = np.asarray(self.featureLoadings).shape[0]
        if genes is None:
            rows = np.arange(G, dtype=np.int64)
        else:
            if isinstance(genes, (str, bytes)) or not hasattr(genes, "__iter__"):
                genes = [genes]
            flat = [x.item() if isinstance(x, np.generic) else x for x in genes]
            by_name = [isinstance(x, str) for x in flat]
            if not flat:
                raise ValueError("genes is empty")
            if all(by_name):
                if self.geneNames is None:
                    raise ValueError("genes holds names but the result carries no geneNames")
                lookup = {}
                for i, nm in enumerate(self.geneNames):
                    lookup.setdefault(nm, i)
                for x in flat:
                    if x not in lookup:
                        raise ValueError("unknown gene name: %s" % x)
                rows = np.array([lookup[x] for x in flat], dtype=np.int64)
            elif all(_is_index(x) for x in flat):
                if any(x < 1 or x > G for x in flat):
                    raise ValueError("genes holds an index outside 1 .. %d" % G)
                rows = np.array(flat, dtype=np.int64) - 1
            else:
                raise ValueError("genes must be all indices or all names")
        labels = [self.geneNames[i] for i in rows] if self.geneNames is not None else [int(i) + 1 for i in rows]
        return rows, labels

    def reconstructGene(self, genes=None, lib=None):
        """R/methods-CogapsResult.R:233-244 on the GPU: featureLoadings %*% t(sampleFactors) in float64, the rows of `genes` (names or
        1-based indices, in the order given, repeats allowed; None: all) -> float64 [rows][samples].  DESIGN.md 4.10 fixes the order
        of the sum."""
        from . import _capi
        rows, _ = self._gene_rows(genes)
        return _capi.residuals(self.featureLoadings, self.sampleFactors, rows=rows, lib=lib)["matrix"]

    def residuals(self, data, uncertainty=None, genes=None, matrix=True, transposeData=False, lib=None):
        """The matrix of R/methods-CogapsResult.R:265-286 (plotResiduals, without the plot) on the GPU: (data - M) / uncertainty in
        float64, the uncertainty defaulting to pmax(0.1 * data, 0.1), and what the library adds to it: the sum of the squared
        residuals of every gene, of every sample and of the whole fit (DESIGN.md 4.10 fixes every order).  data: whatever CoGAPS()
        takes -- a numpy array, a torch tensor (one on the GPU stays there), a scipy.sparse matrix or a DeviceMatrix (neither is
        densified; the default uncertainty only), a file path (.mtx: read as triplets and kept sparse) -- genes x samples unless
        transposeData, under CoGAPS()'s input checks.  genes: the rows of the residual matrix to return, as for reconstructGene;
        matrix=False: none.  -> {"residuals": float64 [rows][samples] or None, "geneChiSq", "sampleChiSq", "chiSq", "genes": the
        rows' labels}"""
        from . import _capi
        data, uncertainty = _data_input(data, uncertainty, lib)
        rows, labels = self._gene_rows(genes) if matrix else (None, [])
        out = _capi.residuals(self.featureLoadings, self.sampleFactors, data=data, unc=uncertainty, rows=rows, transposeData=transposeData, lib=lib)
        return {"residuals": out["matrix"], "geneChiSq": out["geneChiSq"], "sampleChiSq": out["sampleChiSq"], "chiSq": out["chiSq"], "genes": labels}

    def projectR(self, data, dataNames=None, NP=None, full=False, transposeData=False, lib=None):
        """How strongly each pattern shows in other data: projectR(data, loadings = result) by its lmFit route, on the GPU.  Every
        sample of `data` is regressed on featureLoadings by least squares and every coefficient gets a z-test.  data: whatever
        residuals() takes -- numpy, torch (one on the GPU stays there), scipy.sparse, DeviceMatrix (neither is densified), a file path
        -- genes x samples unless transposeData, under CoGAPS()'s input checks.  dataNames: the data's gene names; the genes are then
        matched with the result's geneNames (the intersection, in the result's order; a duplicated data name keeps its first row;
        fewer than K + 1 matches are a ValueError).  Without them the data must have the result's genes, matched by position.  NP:
        1-based pattern indices or names ("Pattern_3") that select the patterns before the fit.  -> {"projection": float64
        [K][samples], "pval": 2 Phi(-|t|), a normal tail}; full=True adds "t", "sigma" [samples], "stdevUnscaled" [K], "df" = genes -
        K, "rss" [samples], "gram" [K][K], "genesMatched" (their labels) and "patterns".  A sample with rss == 0 gets t = +-inf and
        pval = 0 where its coefficient is not zero, and NaN where it is zero.  Collinear or all-zero patterns are refused ("loadings
        are rank deficient"), as are more than 128.  DESIGN.md 4.15 has the definition, every order and every deviation from projectR."""
        return _project(self.featureLoadings, self.geneNames, data, dataNames, NP, full, transposeData, lib)

    def binaryA(self, threshold):
        """R/methods-CogapsResult.R:246-263 without the heatmap: 1 where calcZ() of featureLoadings exceeds threshold, 0 elsewhere"""
        return (self.calcZ() > threshold).astype(np.int8)

    def getOriginalParameters(self):
        """R/methods-CogapsResult.R getOriginalParameters: the parameters the run was made with (metadata["params"])"""
        return self.metadata["params"]

    def getVersion(self):
        """R/methods-CogapsResult.R getVersion: the version string toCSV writes (None for a result that carries none)"""
        return self.metadata.get("version")

    def MANOVA(self, interestedVariables, columns=(0, 1), test="Pillai", whichMatrix="sampleFactors", verbose=False, lib=None):
        """R/methods-CogapsResult.R:596-619 with the sums on the GPU: which patterns separate the groups of the samples.  For every
        pattern k the fit manova(Y ~ x_k) and its summary, where x_k is column k of the chosen matrix and Y holds the factor codes of
        the `columns` of interestedVariables (R: the first two) taken as numbers.  interestedVariables: one row per sample (per gene
        for featureLoadings) -- a 2-D numpy array of any dtype, a list of rows or a pandas DataFrame; a used column is coded as
        unclass(factor(column)) codes it, its sorted distinct values as 1, 2, ... (numpy's sort order); a row with a missing value
        (None, NaN, pandas NA) in a used column is dropped, as na.omit drops it.  test: "Pillai", "Wilks", "Hotelling-Lawley" or "Roy".
        -> {"patterns": the labels, "test", "Df": (1, n - 2), "stat", "approxF", "numDf", "denDf", "pvalue": float64 [K],
        "coefficients": [K][2][p] (intercepts, slopes), "SSCP": {"hypothesis", "residuals"}: [K][p][p], "levels": per used column its
        distinct values, "nOmitted": the rows dropped}.  A pattern without any spread gives NaN; a residual SSCP that is not positive
        definite is a ValueError ("residuals have rank ...").  verbose: one summary line per pattern.  DESIGN.md 4.14 has the
        definition, the order of every sum and every deviation from R."""
        from . import _capi
        if test not in _MANOVA_TESTS:
            raise ValueError("test must be one of %s" % ", ".join("'%s'" % t for t in _MANOVA_TESTS))
        if whichMatrix not in _WHICH:
            raise ValueError("whichMatrix must be either 'featureLoadings' or 'sampleFactors'")
        x = np.asarray(getattr(self, _WHICH[whichMatrix][0]), dtype=np.float32)
        used = _annotation_columns(interestedVariables, columns, x.shape[0], whichMatrix)
        missing = np.zeros(x.shape[0], dtype=bool)
        for col in used:
            missing |= _is_missing(col)
        nOmitted, p = int(missing.sum()), len(used)
        if nOmitted:
            x, used = x[~missing], [col[~missing] for col in used]
        n, K = x.shape
        if n < p + 2:
            raise ValueError("MANOVA: %d complete rows are fewer than the %d that %d response columns need" % (n, p + 2, p))
        coded = [_factor_codes(col) for col in used]
        s = _capi.manova_sscp(x, np.stack([c[0] for c in coded], axis=1), lib=lib)
        sxx, sxy, syy = s["sxx"], s["sxy"], s["syy"]

        # the p x p algebra, float64 on the host: C = the total SSCP scaled to a unit diagonal, C = L L^T
        L, rank = _unit_cholesky(syy)
        if rank < p:
            raise ValueError("MANOVA: residuals have rank %d < %d" % (rank, p))
        root = np.sqrt(np.diag(syy))
        with np.errstate(invalid="ignore", divide="ignore"):
            v = np.linalg.solve(L, (sxy / root[None, :]).T).T / np.sqrt(sxx)[:, None]      # [K][p]: Pillai's trace is |v|^2
            V = np.zeros(K)
            for j in range(p):
                V = V + v[:, j] * v[:, j]
            flat = sxx == 0
            V[flat] = np.nan
            fitted = (1.0 - V) < _MANOVA_PIVOT
            if fitted.any():                                                         # the residual SSCP has lost the direction of the fit
                raise ValueError("MANOVA: residuals have rank %d < %d (pattern %d is a perfect fit)" % (p - 1, p, int(np.flatnonzero(fitted)[0]) + 1))
            ratio = V / (1.0 - V)
            F = (n - p - 1) / p * ratio
            slope = sxy / sxx[:, None]
            H = sxy[:, :, None] * sxy[:, None, :] / sxx[:, None, None]
        from scipy.special import betainc
        num, den = float(p), float(n - p - 1)
        pvalue = np.full(K, np.nan)
        ok = ~flat
        pvalue[ok] = betainc(den / 2.0, num / 2.0, den / (den + num * F[ok]))
        stat = {"Pillai": V, "Wilks": 1.0 - V, "Hotelling-Lawley": ratio, "Roy": ratio}[test]
        labels = ["Pattern_%d" % (k + 1) for k in range(K)]
        out = {"patterns": labels, "test": test, "Df": (1, n - 2), "stat": stat, "approxF": F, "numDf": np.full(K, num), "denDf": np.full(K, den),
               "pvalue": pvalue, "coefficients": np.stack([s["yMean"][None, :] - slope * s["xMean"][:, None], slope], axis=1),
               "SSCP": {"hypothesis": H, "residuals": syy[None, :, :] - H}, "levels": [c[1].tolist() for c in coded], "nOmitted": nOmitted}
        if verbose:
            for k in range(K):
                print("%s: Df 1, %s %.5g, approx F %.5g, num Df %d, den Df %d, Pr(>F) %.4g; residuals Df %d" % (
                    labels[k], test, stat[k], F[k], p, n - p - 1, pvalue[k], n - 2))
        return out


def _csv_value(v):
    if v is None:
        return "NA"
    if isinstance(v, (str, bytes)):
        return '"%s"' % (v.decode() if isinstance(v, bytes) else v).replace('"', '""')
    if isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)):
        return str(int(v))
    v = float(v)                                                                 # (from float32: exact)
    return "NA" if v != v else "Inf" if v == float("inf") else "-Inf" if v == float("-inf") else repr(v)


def _csv_write(save_location, name, lines):
    with open(os.path.join(save_location, name + ".csv"), "w") as f:
        f.write("\n".join(lines) + "\n")


_CSV_FIELD = re.compile(r'"((?:[^"]|"")*)"|([^,]*)')


def _csv_read(save_location, name):
    """-> the fields of every line after the header: a str for a quoted field, None for NA, else an int or a float"""
    with open(os.path.join(save_location, name + ".csv")) as f:
        lines = f.read().splitlines()[1:]
    rows = []
    for line in lines:
        fields, pos = [], 0
        while True:
            m = _CSV_FIELD.match(line, pos)
            if m.group(1) is not None:
                fields.append(m.group(1).replace('""', '"'))
            else:
                x = m.group(2)
                fields.append(None if x == "NA" else int(x) if x.lstrip("+-").isdigit() else float(x.replace("Inf", "inf")))
            pos = m.end() + 1                                                    # (past the comma)
            if pos > len(line):
                break
        rows.append(fields)
    return rows


def toCSV(result, save_location):
    return result.toCSV(save_location)


def fromCSV(save_location):
    """R/methods-CogapsResult.R:644-682: the result toCSV wrote.  The four matrices come back as float32, the library's type of them
    (toCSV's digits are exact for it), the chi-square history as float64, the atom counts as int64."""
    def matrix(name):
        rows = _csv_read(save_location, name)
        return np.array([[np.nan if v is None else v for v in r] for r in rows], dtype=np.float64).astype(np.float32).reshape(len(rows), -1)

    def column(name, dtype=None):
        v = [r[0] for r in _csv_read(save_location, name)]
        if v == [None]:
            return None
        return v if dtype is None else np.array([np.nan if x is None else x for x in v], dtype=dtype)
    raw = {"Amean": matrix("featureLoadings"), "Asd": matrix("loadingStdDev"), "Pmean": matrix("sampleFactors"), "Psd": matrix("factorStdDev")}
    mean = column("meanChiSq", np.float64)
    raw["meanChiSq"] = None if mean is None else float(mean[0])
    for key, name, dtype in (("chisq", "chisqHistory", np.float64), ("atomsA", "atomsA", np.int64), ("atomsP", "atomsP", np.int64)):
        v = column(name, dtype)
        if v is not None:
            raw[key] = v
    res = CogapsResult(raw, geneNames=column("geneNames"), sampleNames=column("sampleNames"))
    version = column("version")
    res.metadata["version"] = None if version is None else version[0]
    return res


def calcGeneGSStat(result, sets=None, numPerm=500, Pw=None, nullGenes=False, **kw):
    return result.calcGeneGSStat(sets, numPerm=numPerm, Pw=Pw, nullGenes=nullGenes, **kw)


def computeGeneGSProb(result, sets=None, numPerm=500, Pw=None, PwNull=False, **kw):
    return result.computeGeneGSProb(sets, numPerm=numPerm, Pw=Pw, PwNull=PwNull, **kw)


def reconstructGene(result, genes=None, **kw):
    return result.reconstructGene(genes, **kw)


def residuals(result, data, uncertainty=None, genes=None, matrix=True, transposeData=False, **kw):
    return result.residuals(data, uncertainty=uncertainty, genes=genes, matrix=matrix, transposeData=transposeData, **kw)


def binaryA(result, threshold):
    return result.binaryA(threshold)


def getOriginalParameters(object):
    return object.getOriginalParameters()


def getVersion(object):
    return object.getVersion()


def MANOVA(interestedVariables, object, **kw):
    """the reference's argument order: the annotations first, then the result"""
    return object.MANOVA(interestedVariables, **kw)


def projectR(data, loadings, dataNames=None, loadingsNames=None, NP=None, full=False, transposeData=False, **kw):
    """projectR(data, loadings): loadings is a CogapsResult (CogapsResult.projectR) or a plain matrix, genes x patterns, with the
    loadingsNames of its rows where dataNames are given"""
    if isinstance(loadings, CogapsResult):
        if loadingsNames is not None:
            raise ValueError("projectR: a result carries its own gene names (loadingsNames is for a plain matrix)")
        return loadings.projectR(data, dataNames=dataNames, NP=NP, full=full, transposeData=transposeData, **kw)
    return _project(loadings, loadingsNames, data, dataNames, NP, full, transposeData, kw.pop("lib", None), **kw)


def patternMarkers(result, threshold="all", lp=None, axis=1, **kw):
    return result.patternMarkers(threshold=threshold, lp=lp, axis=axis, **kw)


def getPatternGeneSet(result, sets=None, method="enrichment", **kw):
    return result.getPatternGeneSet(sets, method=method, **kw)


def calcZ(result, whichMatrix="featureLoadings"):
    return result.calcZ(whichMatrix)


def calcCoGAPSStat(result, sets=None, whichMatrix="featureLoadings", numPerm=1000, **kw):
    return result.calcCoGAPSStat(sets, whichMatrix=whichMatrix, numPerm=numPerm, **kw)
