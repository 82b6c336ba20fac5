"""Host checks of the spherical random fields (msfno_amd/harmonics/random_fields.py and the
reference stream tests/noise_ref.py): the Philox core against the published Random123 known
answers, the spectra and the variance identity against the oracle's Legendre tables, the
reference stream's own statistics at the seed the GPU test uses, and the argument refusals."""
import math

import numpy as np
import pytest
import torch

import noise_ref as R

KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("ctr,key,want", KNOWN_ANSWERS)
def test_philox_known_answers(ctr, key, want):
    got = R.philox4x32_10(ctr, key)
    assert " ".join(f"{int(v):08x}" for v in got) == want


def test_binding_declares_the_noise_entry_points():
    from msfno_amd import _native as N
    names = {n for n, _, _ in N.SIGNATURES}
    assert {"msfno_noise_spectral", "msfno_noise_advance"} <= names
    lib = N.lib()
    assert hasattr(lib, "msfno_noise_spectral") and hasattr(lib, "msfno_noise_advance")


def test_reference_stream_layout():
    """The triangle and the m = 0 imaginary parts are exact zeros, a block serves m = 2p and
    2p + 1, fields are independent of how they are split, and the field row is f % K."""
    se = np.linspace(1.0, 2.0, 3 * 5, dtype=np.float32).reshape(3, 5)
    c = R.spectral(7, 3, 4, 2, 5, 7, se)
    l, m = np.arange(5)[:, None], np.arange(7)[None, :]
    assert (c[:, m > l] == 0).all() and (c[..., 0].imag == 0).all()
    assert (c[:, (m <= l) & (m > 0)].imag != 0).all()
    parts = np.concatenate([R.spectral(7, 3, 1, 2, 5, 7, se), R.spectral(7, 3, 3, 3, 5, 7, se)])
    assert np.array_equal(c, parts)
    re, _ = R.xi(7, 3, [2, 3, 4, 5], 5, 7)
    for i in range(4):
        assert np.allclose(c[i, :, 0].real, se[(2 + i) % 3] * re[i, :, 0], rtol=1e-15)
    assert not np.array_equal(c, R.spectral(8, 3, 4, 2, 5, 7, se))
    assert not np.array_equal(c, R.spectral(7, 4, 4, 2, 5, 7, se))
    # a draw above 2^32 reaches the fourth counter word
    assert not np.array_equal(c, R.spectral(7, 3 + (1 << 32), 4, 2, 5, 7, se))


def test_float32_reference_is_close_to_fp64():
    se = np.ones((1, 33), dtype=np.float32)
    e = np.abs(R.spectral(1, 0, 1, 0, 33, 33, se, dtype=np.float32)
               - R.spectral(1, 0, 1, 0, 33, 33, se)).max()
    assert 0 < e < 4e-6   # a few ulp of 2 pi u at |z| up to 5.8


@pytest.mark.parametrize("alpha,tau,sigma,radius", [(2.0, 3.0, None, 1.0), (1.5, 0.7, 2.5, 6.371e6),
                                                    (4.0, 10.0, None, 2.0)])
def test_matern_sqrt_eig_formula(alpha, tau, sigma, radius):
    from msfno_amd.harmonics import matern_sqrt_eig
    got = matern_sqrt_eig(24, alpha, tau, sigma, radius)
    assert got.dtype == torch.float64 and got.shape == (24,) and got[0] == 0
    sg = tau ** (alpha - 1.0) if sigma is None else sigma
    for l in range(1, 24):
        want = sg * (l * (l + 1) / radius ** 2 + tau ** 2) ** (-alpha / 2.0)
        assert abs(got[l].item() - want) <= 1e-14 * want
    with pytest.raises(ValueError):
        matern_sqrt_eig(8, alpha=1.0)


@pytest.mark.parametrize("grid,nlat,nlon,lmax", [("equiangular", 9, 16, 8),
                                                  ("legendre-gauss", 12, 24, 12)])
def test_field_variance_is_the_variance_at_every_latitude(grid, nlat, nlon, lmax):
    """sum_m e_m sum_l S_l pct[m, l, k]^2 (e_0 = 1, e_m = 2) of the oracle's inverse
    transform equals sum_l (2l + 1) / (4 pi) S_l at every latitude k."""
    from msfno_amd.harmonics import field_variance, matern_sqrt_eig, unit_variance
    from oracle import sht_ref as S
    pct = S.InverseRealSHT(nlat, nlon, lmax=lmax, mmax=lmax, grid=grid).pct.double()
    rows = torch.stack([matern_sqrt_eig(lmax), matern_sqrt_eig(lmax, alpha=1.2, tau=0.5, sigma=3.0),
                        torch.linspace(0.5, 2.0, lmax, dtype=torch.float64)])
    e = torch.full((lmax,), 2.0, dtype=torch.float64)
    e[0] = 1.0
    for row, want in zip(rows, field_variance(rows)):
        lat = torch.einsum("m,l,mlk->k", e, row * row, pct * pct)
        assert (lat - want).abs().max().item() <= 1e-12 * want.item()
    one = field_variance(unit_variance(rows))
    assert (one - 1).abs().max().item() < 1e-14
    assert abs(field_variance(rows[0]).item() - field_variance(rows)[0].item()) == 0


def test_reference_stream_power_per_degree():
    """The reference stream at the GPU test's seed: the mean power of degree l over 256
    fields lies within 4 standard deviations of (2l + 1) S_l."""
    from msfno_amd.harmonics import matern_sqrt_eig
    L = R.STAT_LMAX
    se = matern_sqrt_eig(L).float().numpy()
    c = R.spectral(R.STAT_SEED, 0, R.STAT_FIELDS, 0, L, L, se)
    dev = (R.degree_power_ratio(c, se) - 1) / R.degree_power_sigma(R.STAT_FIELDS, L)
    print("deviations per degree:", np.round(dev, 2))
    assert np.abs(dev).max() <= 4.0


def test_argument_refusals():
    from msfno_amd import ensemble as E
    from msfno_amd.harmonics import GaussianRandomFieldS2, SphericalAR1
    with pytest.raises(ValueError):
        GaussianRandomFieldS2(8, 16, lmax=9)          # the Nyquist bin
    with pytest.raises(ValueError):
        GaussianRandomFieldS2(8, 12, lmax=7)          # nlon // 2 = 6
    with pytest.raises(NotImplementedError):
        GaussianRandomFieldS2(8, 16, norm="backward")
    with pytest.raises(ValueError):
        GaussianRandomFieldS2(8, 16, sqrt_eig=torch.ones(3, 7))
    g = GaussianRandomFieldS2(8, seed=3)
    assert (g.nlon, g.lmax, g.mmax, g.K) == (16, 8, 8, None)
    assert g.sqrt_eig.dtype == torch.float32 and g.rng_state.tolist() == [3, 0]
    assert set(g.state_dict()) >= {"sqrt_eig", "rng_state"}
    x0 = torch.zeros(2, 8, 16)
    with pytest.raises(ValueError, match="even"):
        E.perturb(x0, 3, g)
    with pytest.raises(NotImplementedError):
        E.perturb(x0, E.MAX_MEMBERS + 2, g)
    with pytest.raises(ValueError):
        E.perturb(x0, 4, g)                            # a CPU tensor
    for phi in (-0.1, 1.0, 1.5, math.nan):
        with pytest.raises(ValueError, match="phi"):
            SphericalAR1(g, (1, 2), phi=phi)
    with pytest.raises(ValueError):
        SphericalAR1(g, (1, 2))                        # neither phi nor dt, tau_t
    with pytest.raises(ValueError):
        SphericalAR1(g, (1, 2), phi=0.5)               # a CPU field
    with pytest.raises(ValueError):
        g.sample_coeffs(2)
    with pytest.raises(ValueError):
        g(1, xi=torch.zeros(1, 8, 8, dtype=torch.complex64))


def test_native_argument_checks():
    """The C entry points refuse bad arguments before any launch (no GPU needed): null
    pointers, K < 1, pointers off the 8-byte grid, and extents the 32-bit counter words
    cannot hold."""
    from msfno_amd import _native as N
    lib = N.lib()
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data

    def rc(coeffs=p, prev=None, se=p, K=1, n=1, field0=0, lmax=2, mmax=2):
        return lib.msfno_noise_spectral(coeffs, prev, se, K, n, field0, lmax, mmax, 0.0, 1.0, 0,
                                        0, None, None)
    for bad in (dict(coeffs=None), dict(se=None), dict(K=0), dict(n=0), dict(lmax=0),
                dict(mmax=0), dict(field0=-1), dict(coeffs=p + 4), dict(prev=p + 4),
                dict(field0=1 << 32), dict(n=2, field0=(1 << 32) - 1),
                dict(lmax=1 << 16, mmax=1 << 17)):
        assert rc(**bad) == N.MSFNO_EINVAL, bad
        with pytest.raises(ValueError):
            N.check(N.MSFNO_EINVAL)
    assert b"2^32" in lib.msfno_last_error()
    assert lib.msfno_noise_advance(None, 1, None) == N.MSFNO_EINVAL
    assert lib.msfno_noise_advance(p + 4, 1, None) == N.MSFNO_EINVAL


def test_rollout_refuses_noise_on_a_sharded_model():
    from msfno_amd.rollout import Rollout

    class Sharded:
        world = 2
    with pytest.raises(NotImplementedError):
        Rollout(Sharded(), noise=object())
    assert Rollout(None).noise is None
