"""Host-side checks of the ensemble verification (msfno_amd/ensemble.py): ``finish`` on the
fp64 restatement's sums (tests/ensemble_util.py) against independent forms of each score,
the additivity of the sums over a row split, the argument refusals (Python and C-ABI, all
before any launch) and the declaration / binding / export of the three entry points."""
import os
import re

import pytest
import torch

import ensemble_util as EU
from conftest import REPO

SYMBOLS = ("msfno_ens_workspace_size", "msfno_ens_sums", "msfno_ens_crps_backward")


def _finish(ens, tar, w, with_hist=True):
    from msfno_amd import ensemble as E
    M, W = ens.shape[0], ens.shape[-1]
    s, _ = EU.sums(ens, tar, w)
    h = EU.hist(ens, tar, w) if with_hist else None
    return E.finish(s, h, w, W, M)


def _crps_integral(x, y):
    """int (F(z) - 1[z >= y])^2 dz of the empirical distribution F of the members x: the
    integrand is a step function, integrated piece by piece between the sorted members and
    the truth."""
    pts = torch.sort(torch.cat([x, y.reshape(1)])).values
    total = 0.0
    for a, b in zip(pts[:-1], pts[1:]):
        mid = 0.5 * (a + b)
        F = (x <= mid).double().mean()
        H = 1.0 if mid >= y else 0.0
        total += float((F - H) ** 2 * (b - a))
    return total


@pytest.mark.parametrize("M", [2, 3, 8, 17])
def test_crps_is_the_integral_of_the_squared_cdf_difference(M):
    g = torch.Generator().manual_seed(M)
    for trial in range(4):
        x = 300 + torch.randn(M, generator=g, dtype=torch.float64)
        y = 300.5 + torch.randn((), generator=g, dtype=torch.float64) * (trial + 0.5)
        got = _finish(x.view(M, 1, 1, 1, 1), y.view(1, 1, 1, 1), torch.ones(1).double())
        want = _crps_integral(x, y)
        assert abs(got.crps.item() - want) <= 1e-12 * max(1.0, want)
        # fair - plain = -gini (1 / (M (M - 1)) - 1 / M^2) = -gini / (M^2 (M - 1))
        pair = sum(abs(x[i] - x[j]) for i in range(M) for j in range(i + 1, M)).item()
        assert abs(got.fair_crps.item() - (want - pair / (M * M * (M - 1)))) <= 1e-12


def test_spread_is_the_unbiased_variance_and_the_mean_scores_are_the_means():
    M, B, C, H, W = 5, 2, 3, 6, 8
    ens, tar, w = EU.inputs(M, (B * C, H, W))
    ens = ens.double().view(M, B, C, H, W)
    tar = tar.double().view(B, C, H, W)
    w = w.double()
    got = _finish(ens, tar, w)
    ww = (w / (w.sum() * W))[:, None]
    var = (ww * torch.var(ens, dim=0, unbiased=True)).sum(dim=(-1, -2))
    assert torch.allclose(got.spread ** 2, var, rtol=1e-9, atol=0)   # 300 +- 1: var cancels
    mean_err = ens.mean(dim=0) - tar
    assert torch.allclose(got.mse, (ww * mean_err ** 2).sum(dim=(-1, -2)), rtol=1e-9, atol=0)
    assert torch.allclose(got.rmse, got.mse.sqrt())
    assert torch.allclose(got.bias, (ww * mean_err).sum(dim=(-1, -2)), rtol=1e-9, atol=0)
    assert torch.allclose(got.mae, (ww * (ens - tar).abs().mean(dim=0)).sum(dim=(-1, -2)),
                          rtol=1e-12, atol=0)
    want_ss = ((M + 1) / M) ** 0.5 * got.spread / got.rmse
    assert torch.allclose(got.spread_skill, want_ss, rtol=1e-12, atol=0)
    assert got.rank_hist.shape == (B, C, M + 1)
    assert torch.allclose(got.rank_hist.sum(dim=-1), torch.ones(B, C).double(), rtol=1e-12,
                          atol=0)
    assert (got.rank_hist >= 0).all()
    assert _finish(ens, tar, w, with_hist=False).rank_hist is None
    for name, v in EU.scores(*(EU.sums(ens, tar, w)[:1]), EU.hist(ens, tar, w), w, W, M).items():
        assert torch.allclose(getattr(got, name), v, rtol=1e-12, atol=0), name


def test_two_members_closed_form():
    ens, tar, w = EU.inputs(2, (3, 4, 5))
    ens, tar, w = ens.double().view(2, 1, 3, 4, 5), tar.double().view(1, 3, 4, 5), w.double()
    got = _finish(ens, tar, w)
    ww = (w / (w.sum() * 5))[:, None]
    want = (ens - tar).abs().mean(dim=0) - (ens[0] - ens[1]).abs() / 2
    assert torch.allclose(got.fair_crps, (ww * want).sum(dim=(-1, -2)), rtol=1e-12, atol=0)
    want = (ens - tar).abs().mean(dim=0) - (ens[0] - ens[1]).abs() / 4
    assert torch.allclose(got.crps, (ww * want).sum(dim=(-1, -2)), rtol=1e-12, atol=0)


def test_sums_and_counts_add_up_over_a_row_split():
    M, S, H, W = 4, 2, 9, 7
    ens, tar, w = (t.double() for t in EU.inputs(M, (S, H, W)))
    whole, _ = EU.sums(ens, tar, w)
    hw = EU.hist(ens, tar, w)
    for k in (1, 4, 8):
        a, _ = EU.sums(ens[..., :k, :], tar[..., :k, :], w[:k])
        b, _ = EU.sums(ens[..., k:, :], tar[..., k:, :], w[k:])
        assert torch.allclose(a + b, whole, rtol=1e-13, atol=1e-13)
        ha = EU.hist(ens[..., :k, :], tar[..., :k, :], w[:k])
        hb = EU.hist(ens[..., k:, :], tar[..., k:, :], w[k:])
        assert torch.allclose(ha + hb, hw, rtol=1e-13, atol=0)


def test_restated_gradient_is_the_sign_formula():
    """The formula of the issue against autograd of the restatement, ties included."""
    M, S, H, W = 4, 2, 3, 5
    ens, tar, w = (t.double() for t in EU.inputs(M, (S, H, W)))
    ens[1, :, 0] = tar[:, 0]          # x_1 = y on a row
    ens[2, :, 1] = ens[0, :, 1]       # x_2 = x_0 on a row
    g = torch.tensor([0.7, -1.3]).double()
    for fair in (True, False):
        k = EU.kappa(M, fair)
        x = ens.clone().requires_grad_()
        (g * EU.crps_sums(x, tar, w, k)).sum().backward()
        sy = torch.sign(ens - tar) / M
        sx = sum(torch.sign(ens - ens[j:j + 1]) for j in range(M))
        want = w[None, None, :, None] * g[None, :, None, None] * (sy - k * sx)
        assert torch.allclose(x.grad, want, rtol=1e-13, atol=1e-15)


def test_python_refusals():
    from msfno_amd import ensemble as E
    from msfno_amd.rollout import Rollout
    x = torch.zeros(3, 1, 2, 4, 8)
    t = torch.zeros(1, 2, 4, 8)
    w = torch.ones(4)
    with pytest.raises(ValueError, match="GPU"):
        E.ensemble_sums(x, t, w)                                    # no CPU path
    with pytest.raises(ValueError, match="at least 2"):
        E.ensemble_sums(x[:1], t, w)
    with pytest.raises(NotImplementedError, match="at most 32"):
        E.ensemble_sums(torch.zeros(33, 1, 2, 4, 8), t, w)
    with pytest.raises(ValueError, match="must be"):
        E.ensemble_sums(x, t[0], w)
    with pytest.raises(ValueError, match="must be"):
        E.ensemble_sums(x[0], t, w)
    with pytest.raises(ValueError, match="requires grad"):
        E.ensemble_sums(x.clone().requires_grad_(), t, w)
    with pytest.raises(NotImplementedError, match="target"):
        E.CRPSLoss()(x, t.clone().requires_grad_())
    with pytest.raises(ValueError, match="GPU"):
        E.CRPSLoss()(x, t)
    with pytest.raises(ValueError):
        E.CRPSLoss()(x[0], t)
    with pytest.raises(ValueError, match="at least 2"):
        E.EnsembleVerifier("uniform", 4, 8, 1, 1, 1, 2, device="cpu")
    with pytest.raises(NotImplementedError, match="at most 32"):
        E.EnsembleVerifier("uniform", 4, 8, 1, 33, 1, 2, device="cpu")
    with pytest.raises(ValueError):
        E.EnsembleVerifier("uniform", 4, 8, 0, 3, 1, 2, device="cpu")
    s = torch.zeros(1, 2, 5)
    with pytest.raises(ValueError):
        E.finish(torch.zeros(1, 2, 6), None, w, 8, 3)
    with pytest.raises(ValueError):
        E.finish(s, torch.zeros(1, 2, 5), w, 8, 3)                   # M + 1 = 4 bins
    with pytest.raises(ValueError):
        E.finish(s, None, w, 8, 1)

    class Sharded:
        world = 2

    with pytest.raises(NotImplementedError, match="ensemble_sums"):
        Rollout(Sharded(), graph=False).verify_ensemble(t[0].expand(3, 2, 4, 8), [t], 1)


def test_c_abi_refusals_come_before_any_launch():
    """Every refusal is decided on the arguments alone: the pointers here are never
    dereferenced (this test runs without a GPU)."""
    from msfno_amd import _native as N
    lib = N.lib()
    S, H, W = 2, 3, 8
    n = S * H * W
    p = 4096                       # any non-null address
    size = lib.msfno_ens_workspace_size(S, 4, H, W)
    assert size > 0 and size % 4 == 0
    assert lib.msfno_ens_workspace_size(S, 32, H, W) >= lib.msfno_ens_workspace_size(S, 2, H, W)
    for bad in ((0, 4, H, W), (S, 1, H, W), (S, 33, H, W), (S, 4, 0, W), (S, 4, H, 0)):
        assert lib.msfno_ens_workspace_size(*bad) == 0

    def sums(ens=p, stride=n, tar=p, w=p, out=p, hist=None, M=4, S=S, H=H, W=W, ws=p, nbytes=size):
        return lib.msfno_ens_sums(ens, stride, tar, w, out, hist, M, S, H, W, ws, nbytes, None)

    def bwd(ens=p, stride=n, tar=p, w=p, g=p, dens=p, dstride=n, M=4, S=S, H=H, W=W):
        return lib.msfno_ens_crps_backward(ens, stride, tar, w, g, 0.25, dens, dstride, M, S, H,
                                           W, None)

    for kw in (dict(ens=None), dict(tar=None), dict(w=None), dict(out=None), dict(ws=None),
               dict(S=0), dict(H=0), dict(W=0), dict(M=1), dict(M=0), dict(stride=n - 1)):
        assert sums(**kw) == N.MSFNO_EINVAL, kw
    assert sums(M=33, nbytes=1 << 30) == N.MSFNO_EUNSUPPORTED
    assert sums(nbytes=size - 1) == N.MSFNO_EWORKSPACE
    for kw in (dict(ens=None), dict(tar=None), dict(w=None), dict(g=None), dict(dens=None),
               dict(S=0), dict(H=0), dict(W=0), dict(M=1), dict(stride=n - 1),
               dict(dstride=n - 1)):
        assert bwd(**kw) == N.MSFNO_EINVAL, kw
    assert bwd(M=33) == N.MSFNO_EUNSUPPORTED
    with pytest.raises(NotImplementedError):
        N.check(sums(M=33, nbytes=1 << 30), "msfno_ens_sums")
    with pytest.raises(ValueError, match="stride"):
        N.check(sums(stride=n - 1), "msfno_ens_sums")
    with pytest.raises(ValueError, match="workspace"):
        N.check(sums(nbytes=0), "msfno_ens_sums")


def test_entry_points_are_declared_bound_and_exported():
    from msfno_amd import _native as N
    import msfno_amd
    assert hasattr(msfno_amd, "ensemble")
    header = open(os.path.join(REPO, "include", "msfno.h")).read()
    declared = set(re.findall(r"\b(msfno_[a-z0-9_]+)\s*\(", header))
    bound = {n for n, _, _ in N.SIGNATURES}
    for s in SYMBOLS:
        assert s in declared and s in bound and hasattr(N.lib(), s), s
    assert N.lib().msfno_abi_version() == 6
