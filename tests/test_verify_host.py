"""CPU-side checks of the forecast verification (msfno_amd/verification.py,
csrc/verify.hip): the C-ABI additions are declared, exported and bound, refuse bad
arguments before any launch, and ``finish`` on fp64 host sums equals the restatement
(tests/verify_util.py) and the reference's own formulas (model.py:743, 755-757)."""
import ctypes
import os
import re

import pytest
import torch

import verify_util as VU
from conftest import REPO


def test_verify_symbols_declared_exported_and_bound():
    from msfno_amd import _native as N
    hdr = open(os.path.join(REPO, "include", "msfno.h")).read()
    bound = {n for n, _, _ in N.SIGNATURES}
    for s in ("msfno_verify_workspace_size", "msfno_verify_sums"):
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(N.lib(), s), s
        assert s in bound, s
    assert N.lib().msfno_abi_version() == 6


def test_verify_workspace_size_positive_and_monotone():
    from msfno_amd import _native as N
    f = N.lib().msfno_verify_workspace_size
    base = (73, 721, 1440)
    assert f(*base) > 0 and f(1, 1, 1) > 0
    for axis in range(3):
        prev = 0
        for v in (1, 2, 3, 7, 28, 29, 64, 65, 73, 128, 721, 1024, 1025, 2047, 2048, 2049, 5000):
            a = list(base)
            a[axis] = v
            cur = f(*a)
            assert cur > 0 and cur >= prev, (axis, v, cur, prev)
            prev = cur
    assert f(0, 721, 1440) == 0 and f(73, -1, 1440) == 0 and f(73, 721, 0) == 0


def test_verify_sums_refuses_bad_arguments_before_any_launch():
    """MSFNO_EINVAL for null pointers, extents below 1 and only one of clim / clim_slab,
    MSFNO_EWORKSPACE for a short workspace; on host pointers that no kernel may touch."""
    from msfno_amd import _native as N
    lib = N.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    big = 1 << 20

    def call(prd=p, tar=p, w=p, clim=None, slab=None, sums=p, BC=1, nlat=2, nlon=2, ws=p,
             nbytes=big):
        return lib.msfno_verify_sums(prd, tar, w, clim, slab, sums, BC, nlat, nlon, ws, nbytes,
                                     None)

    for name in ("prd", "tar", "w", "sums", "ws"):
        assert call(**{name: None}) == N.MSFNO_EINVAL, name
    for name in ("BC", "nlat", "nlon"):
        assert call(**{name: 0}) == N.MSFNO_EINVAL, name
        assert call(**{name: -3}) == N.MSFNO_EINVAL, name
    assert call(clim=p) == N.MSFNO_EINVAL
    assert call(slab=p) == N.MSFNO_EINVAL
    assert b"clim" in lib.msfno_last_error()
    assert call(nbytes=8) == N.MSFNO_EWORKSPACE
    assert call(clim=p, slab=p, nbytes=lib.msfno_verify_workspace_size(1, 2, 2) - 1) \
        == N.MSFNO_EWORKSPACE


def _host_problem(B=2, C=5, H=9, W=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    tar = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    prd = tar + 0.4 * torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    clim = 0.5 * torch.randn(C, H, W, generator=g, dtype=torch.float64)
    w = torch.rand(H, generator=g, dtype=torch.float64) + 0.1
    slab = [(-1 if c in (1, 3) else c) for _ in range(B) for c in range(C)]
    return prd, tar, clim, w, slab


def _assert_scores(got, want, tol=1e-12):
    for name in VU.NAMES:
        g, v = getattr(got, name), want[name]
        assert g.shape == v.shape, name
        assert torch.equal(torch.isnan(g), torch.isnan(v)), name
        ok = ~torch.isnan(v)
        assert ((g[ok] - v[ok]).abs() <= tol * v[ok].abs().clamp(min=1e-300)).all(), name


@pytest.mark.parametrize("batch_mean", [False, True])
def test_finish_equals_restatement(batch_mean):
    from msfno_amd import verification as V
    prd, tar, clim, w, slab = _host_problem()
    s, _ = VU.sums(prd, tar, w, clim, slab)
    has = (torch.tensor(slab).reshape(2, 5) >= 0)
    got = V.finish(s, w, prd.shape[3], batch_mean=batch_mean)
    want = VU.scores(s, w, prd.shape[3], has, batch_mean=batch_mean)
    assert got.mse.dtype == torch.float64
    assert got.mse.shape == ((5,) if batch_mean else (2, 5))
    _assert_scores(got, want)
    # slabs without a climatology: NaN skill and ACC, finite everything else
    nan_cols = torch.tensor([False, True, False, True, False])
    assert torch.equal(torch.isnan(got.skill).reshape(-1, 5).all(dim=0), nan_cols)
    assert torch.equal(torch.isnan(got.acc).reshape(-1, 5).any(dim=0), nan_cols)
    for name in ("mse", "rmse", "bias", "mae"):
        assert torch.isfinite(getattr(got, name)).all()
    # a leading scored-step axis passes through
    stacked = V.finish(torch.stack((s, 2 * s)), w, prd.shape[3], batch_mean=batch_mean)
    assert stacked.mse.shape == (2,) + got.mse.shape
    assert torch.equal(stacked.acc[0][~torch.isnan(got.acc)], got.acc[~torch.isnan(got.acc)])


def test_finish_matches_the_reference_formulas_for_one_sample_uniform_weights():
    """model.py:743: MSELoss(reduction='none')(prd, truth).mean(dim=(0, 2, 3)) / batch_size;
    :755-757: 1 - that / MSELoss()(clim_var, truth_var), at batch size 1."""
    from msfno_amd import verification as V
    prd, tar, clim, _, _ = _host_problem(B=1, C=4, H=7, W=10, seed=3)
    w = torch.ones(7, dtype=torch.float64)
    s, _ = VU.sums(prd, tar, w, clim, list(range(4)))
    got = V.finish(s, w, 10, batch_mean=True)
    pervar = torch.nn.MSELoss(reduction="none")(prd, tar).mean(dim=(0, 2, 3)) / 1
    skill = torch.stack([1 - pervar[c] / torch.nn.MSELoss()(clim[c], tar.squeeze(0)[c])
                         for c in range(4)])
    assert ((got.mse - pervar).abs() <= 1e-12 * pervar).all()
    assert ((got.skill - skill).abs() <= 1e-12 * skill.abs()).all()
    stds = torch.tensor([0.5, 2.0, 3.0, 1e3], dtype=torch.float64)
    means = torch.tensor([1.0, -2.0, 0.0, 5e4], dtype=torch.float64)

    def norm(x):
        return (x - means[None, :, None, None]) / stds[None, :, None, None]

    pervar_norm = torch.nn.MSELoss(reduction="none")(norm(prd), norm(tar)).mean(dim=(0, 2, 3))
    got_norm = V.mse_normalised(got.mse, stds.reshape(1, 4, 1, 1))
    assert torch.equal(got_norm, got.mse / stds ** 2)
    assert ((got_norm - pervar_norm).abs() <= 1e-12 * pervar_norm).all()
    with pytest.raises(ValueError):
        V.mse_normalised(got.mse, stds[:3])


def test_field_sums_refuses_host_tensors_and_bad_shapes():
    from msfno_amd import verification as V
    x = torch.zeros(1, 2, 4, 8)
    with pytest.raises(ValueError):
        V.field_sums(x, x, torch.ones(4))             # libmsfno has no CPU path
    with pytest.raises(ValueError):
        V.field_sums(x, x[:, :1], torch.ones(4))
    with pytest.raises(ValueError, match="requires grad"):
        V.field_sums(x.clone().requires_grad_(), x, torch.ones(4))
    with pytest.raises(ValueError):
        V.finish(torch.zeros(2, 5), torch.ones(4), 8)
