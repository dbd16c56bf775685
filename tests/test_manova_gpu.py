"""MANOVA on the MI355X: the device's means and centred sums against the numpy restatement of tests/manova_cases.py, bit for bit (the
grid of tests/test_manova.py), the strides, the offset and zero columns, more trips than the grid holds workgroups, a 50 000 x 50
matrix, and the rational anchor through the front end."""
import numpy as np
import pytest

import manova_cases as mc
from cogaps_amd import CogapsResult, _capi

pytestmark = pytest.mark.gpu

R = 256                                                     # csrc/manova_kernel.h: MV_TRIP, the rows of a trip


def _check(lib, X, Y, want=None, what=""):
    mc.check(_capi.manova_sscp(X, Y, lib=lib), want if want is not None else mc.restate(np.asarray(X), np.asarray(Y)), what)


@pytest.mark.parametrize("p", [1, 2, 8])
@pytest.mark.parametrize("K", [1, 3, 64, 65, 130, 513])
def test_sums_bit_for_bit(hip_lib, K, p):
    for n in mc.row_counts(p, R):
        _check(hip_lib, mc.x_matrix(n, K), mc.y_matrix(n, p), what="n %d K %d p %d" % (n, K, p))


def test_a_workgroup_takes_a_second_trip(hip_lib):
    """the grid is eight workgroups per compute unit: on the 256 units of a whole MI355X, 2048 R + 1 rows are the fewest that give a
    workgroup a second trip (a partition of the device has fewer units and takes second trips sooner)"""
    n = 2048 * R + 1
    _check(hip_lib, mc.x_matrix(n, 1), mc.y_matrix(n, 1), what="n %d" % n)


@pytest.mark.parametrize("n,K,p", [(65, 3, 2), (R + 1, 65, 8), (3 * R + 7, 130, 1)])
def test_strides(hip_lib, n, K, p):
    X, Y = mc.x_matrix(n, K), mc.y_matrix(n, p)
    want = mc.restate(X, Y)
    FX, FY = np.asfortranarray(X), np.asfortranarray(Y)
    _check(hip_lib, FX, Y, want, "column-major X")
    _check(hip_lib, X, FY, want, "column-major Y")
    wide = np.zeros((2 * n + 1, 3 * K + 2), dtype=np.float32)
    wide[1::2, 2::3][:n] = X
    _check(hip_lib, wide[1::2, 2::3][:n], FY, want, "a slice of X")


def test_offset_and_zero_columns(hip_lib):
    n = 3 * R + 7
    X, Y = mc.x_matrix(n, 3), mc.y_matrix(n, 2)
    out = _capi.manova_sscp(X, Y, lib=hip_lib)
    mc.check(out, mc.restate(X, Y))
    assert out["sxx"][2] == 0.0 and not out["sxy"][2].any()
    x = X[:, 1].astype(np.float64)
    exact = float(np.sum((x - x.mean()) ** 2))
    assert 0 < exact < 1e-3 and abs(out["sxx"][1] - exact) <= 1e-9 * exact


def test_a_single_cell_sized_matrix(hip_lib):
    """50 000 x 50, p = 2: 196 trips"""
    _check(hip_lib, mc.x_matrix(50000, 50), mc.y_matrix(50000, 2))


def test_rational_anchor_through_the_front_end(hip_lib):
    from scipy.stats import f
    out = CogapsResult(mc.raw_result(mc.ANCHOR_X[:, None])).MANOVA(mc.ANCHOR_Y, lib=hip_lib)
    mc.check_anchor(out)
    assert abs(out["pvalue"][0] - f.sf(out["approxF"][0], 2, 3)) <= 1e-12 * out["pvalue"][0]
    P, ann = mc.planted()
    planted = CogapsResult(mc.raw_result(P)).MANOVA(ann, lib=hip_lib)
    assert int(np.argmin(planted["pvalue"])) == 3 and planted["levels"] == [["ctrl", "dose", "high"], ["f", "m"]]
