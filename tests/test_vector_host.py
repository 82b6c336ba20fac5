"""msfno_vector_legendre_table (host fp64): the derivative tables D = dP/dtheta and
Q = m P / sin(theta) of the vector transforms against vector_util's independent formulas,
their exact zeros (pole columns but m = 1, rows l < m, the l = 0 row of the analysis
tables) and the equatorial parity that decides which Legendre layout a table gets."""
import numpy as np
import pytest

import vector_util as VU

CASES = [("equiangular", 33, 32, 33), ("legendre-gauss", 24, 24, 25), ("equiangular", 13, 7, 9)]
IDS = ["-".join(map(str, c)) for c in CASES]


def _native(grid, nlat, lmax, mmax, inverse, csphase=True):
    from msfno_amd.harmonics.vector import _vector_table
    return _vector_table(mmax, lmax, nlat, grid, inverse, csphase).numpy()


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_tables_match_the_independent_formulas(case, inverse):
    grid, nlat, lmax, mmax = case
    got = _native(grid, nlat, lmax, mmax, inverse)
    assert got.shape == (2, mmax, lmax, nlat) and got.dtype == np.float64
    want = np.stack(VU.dq_tables(grid, nlat, lmax, mmax)[:2] if inverse
                    else VU.analysis_tables(grid, nlat, lmax, mmax))
    for i, name in enumerate("DQ"):
        scale = np.abs(want[i]).max()
        err = np.abs(got[i] - want[i]).max()
        print(f"{name} {case} inverse={inverse}: max err / max|table| = {err / scale:.3e}")
        assert err <= 1e-11 * scale, (name, err / scale)
    l = np.arange(lmax)[None, :]
    m = np.arange(mmax)[:, None]
    assert (got[:, l < m] == 0).all()        # rows l < m, exactly
    assert (got[1, 0] == 0).all()            # Q at m = 0
    if not inverse:
        assert (got[:, :, 0] == 0).all()     # 1 / (l(l+1)): no degree 0
    if grid == "equiangular":                # pole columns: only m = 1, where D = Q
        for k in (0, nlat - 1):
            assert (got[:, np.arange(mmax) != 1, :, k] == 0).all()
            assert np.abs(got[:, 1, 1:, k]).min() > 0
        # two different three-factor expressions of one value: a few roundings apart
        assert np.allclose(got[0, 1, :, 0], got[1, 1, :, 0], rtol=1e-14, atol=0)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_row_parity(case, inverse):
    """D[nlat-1-k] = (-1)^(l-m+1) D[k] and Q[nlat-1-k] = (-1)^(l-m) Q[k], to 1e-12 of the
    table's largest entry: moved up one degree, D has the parity of a scalar table."""
    grid, nlat, lmax, mmax = case
    got = _native(grid, nlat, lmax, mmax, inverse)
    sgn = (-1.0) ** (np.arange(lmax)[None, :] - np.arange(mmax)[:, None])[:, :, None]
    for i, s in ((0, -sgn), (1, sgn)):
        err = np.abs(got[i][:, :, ::-1] - s * got[i]).max()
        print(f"{'DQ'[i]} {case} inverse={inverse}: parity defect {err:.3e}, "
              f"max|table| {np.abs(got[i]).max():.3e}")
        assert err <= 1e-12 * np.abs(got[i]).max()


def _folds(t):
    """The criterion of the table loader's symmetry check on an fp32 (mmax, lmax, nlat)
    table: t[nlat-1-k] = (-1)^(l-m) t[k] within 1e-5 of the row's maximum."""
    t = np.asarray(t, dtype=np.float32)
    mmax, lmax, nlat = t.shape
    tol = np.float32(1e-5) * np.abs(t).max(-1, keepdims=True)
    sgn = ((-1.0) ** (np.arange(lmax)[None, :] - np.arange(mmax)[:, None]))[:, :, None]
    h = nlat // 2
    return bool((np.abs(t[:, :, ::-1][:, :, :h] - sgn.astype(np.float32) * t[:, :, :h]) <= tol).all())


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_shifted_d_takes_the_folded_layout(case, inverse):
    """What the transforms load, rounded to fp32: D moved up one degree and Q meet the
    loader's criterion for the hemisphere-folded layout; D as it is does not."""
    grid, nlat, lmax, mmax = case
    got = _native(grid, nlat, lmax, mmax, inverse).astype(np.float32)
    shifted = np.zeros((mmax, lmax + 1, nlat), dtype=np.float32)
    shifted[:, 1:] = got[0]
    assert _folds(shifted) and _folds(got[1])
    assert not _folds(got[0])


def test_without_the_condon_shortley_phase():
    grid, nlat, lmax, mmax = CASES[2]
    a, b = _native(grid, nlat, lmax, mmax, True, True), _native(grid, nlat, lmax, mmax, True, False)
    sgn = ((-1.0) ** np.arange(mmax))[None, :, None, None]
    assert np.array_equal(b, sgn * a)
    d, q, _ = VU.dq_tables(grid, nlat, lmax, mmax, False)
    assert np.abs(b - np.stack((d, q))).max() <= 1e-11 * np.abs(d).max()


def test_constructor_refusals_and_buffers():
    import torch
    from msfno_amd.harmonics import InverseRealVectorSHT, RealVectorSHT
    with pytest.raises(NotImplementedError):
        RealVectorSHT(10, 20, grid="lobatto")
    with pytest.raises(NotImplementedError):
        InverseRealVectorSHT(10, 20, norm="schmidt")
    f = RealVectorSHT(13, 26, lmax=7, mmax=9)
    g = InverseRealVectorSHT(13, 26, lmax=7, mmax=9)
    assert f.weights.shape == g.dpct.shape == (2, 9, 7, 13)
    assert set(dict(f.named_buffers())) == {"weights"} and set(dict(g.named_buffers())) == {"dpct"}
    with pytest.raises(ValueError):
        f(torch.zeros(1, 2, 13, 26))
    with pytest.raises(ValueError):
        g(torch.zeros(1, 2, 7, 9, dtype=torch.complex64))
    with pytest.raises(AssertionError):
        f(torch.zeros(1, 3, 13, 26))
    with pytest.raises(AssertionError):
        g(torch.zeros(1, 2, 8, 9, dtype=torch.complex64))
