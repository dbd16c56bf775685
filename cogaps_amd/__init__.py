"""cogaps_amd -- the CoGAPS asynchronous Gibbs sampler hot path on MI355X (HIP, gfx950).

Public surface mirrors the reference's: CoGAPS(), GWCoGAPS(), scCoGAPS(), CogapsParams, CogapsResult, calcZ(), calcCoGAPSStat() (the gene-set permutation statistic of a result, on the GPU), patternMarkers() (every gene or sample ranked against every pattern, and the marker lists, on the GPU), getPatternGeneSet() (the gene sets of every pattern: enrichment with its permutation null on the GPU, or overrepresentation among the markers),
calcGeneGSStat() / computeGeneGSProb() (which genes of a gene set behave like the set, for any number of sets at once, on the GPU), toCSV() / fromCSV(), getOriginalParameters(), getVersion(),
MANOVA() (which patterns separate the groups of the samples: manova of the factor-coded annotations on every pattern, the sums of squares and cross-products on the GPU),
projectR() (how strongly each pattern shows in every sample of other data: the least-squares fit of the data on the loadings with a z-test, on the GPU; sparse data stays sparse),
findConsensusMatrix() / patternMatch() (the consensus of the patterns of a distributed run's first pass -- correlation distance, complete linkage, weighted mean patterns -- on the GPU),
reconstructGene(), residuals() (plotResiduals' matrix and the chi-square of every gene and sample, on the GPU; sparse data stays sparse), binaryA(),
DeviceMatrix (a sparse matrix uploaded to the GPU once, the source of any number of runs and subsets), DeviceDense (a dense matrix that
already resides on the GPU, by address; a torch tensor on the GPU is taken as one by every entry point), buildReport(), checkpointsEnabled(), compiledWithOpenMPSupport().  CoGAPS(..., stateFile=, stateInterval=, resume=) saves a run's chain to the
library's own state file and continues it bit for bit (checkpointsEnabled() stays False: the reference's checkpoint files are not read).  All compute goes through
csrc/libcogaps_hip.so (include/cogaps_hip.h); importing works without a GPU, running does not."""
from .params import CogapsParams
from .result import (CogapsResult, calcZ, calcCoGAPSStat, calcGeneGSStat, computeGeneGSProb, patternMarkers, getPatternGeneSet, reconstructGene,
                     residuals, binaryA, toCSV, fromCSV, MANOVA, getOriginalParameters, getVersion, projectR)
from .api import CoGAPS, GWCoGAPS, scCoGAPS
from .distributed import findConsensusMatrix, patternMatch
from ._capi import DeviceMatrix, DeviceDense


def buildReport():
    from . import _capi
    return _capi.load().cogaps_build_report().decode()


def checkpointsEnabled():
    return False


def compiledWithOpenMPSupport():
    from . import _capi
    return bool(_capi.load().cogaps_compiled_with_openmp())


__all__ = ["CoGAPS", "GWCoGAPS", "scCoGAPS", "CogapsParams", "CogapsResult", "DeviceMatrix", "DeviceDense", "buildReport", "checkpointsEnabled",
           "compiledWithOpenMPSupport", "calcZ", "calcCoGAPSStat", "calcGeneGSStat", "computeGeneGSProb", "toCSV", "fromCSV", "patternMarkers", "getPatternGeneSet", "reconstructGene", "residuals", "binaryA",
           "findConsensusMatrix", "patternMatch", "MANOVA", "getOriginalParameters", "getVersion", "projectR"]
