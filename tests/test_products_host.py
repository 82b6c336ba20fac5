"""Host-side checks of the ensemble products and threshold scores (msfno_amd/ensemble.py):
the quantile position against torch.quantile, ``finish_thresholds`` on the fp64 restatement's
counts (tests/products_util.py) against the per-pixel forms of each score, the refusals and
the entry points.  No GPU."""
import os
import re

import pytest
import torch

import products_util as PU
from conftest import REPO

SYMBOLS = ("msfno_ens_products", "msfno_ens_threshold_workspace_size",
           "msfno_ens_threshold_sums")
MS = (2, 3, 5, 8, 9, 16, 17, 32)


def test_quantile_position_is_torch_quantile():
    from msfno_amd import ensemble as E
    g = torch.Generator().manual_seed(11)
    worst = 0.0
    for M in MS:
        x = (300 + torch.randn(M, 64, generator=g)).float().double()
        srt = x.sort(dim=0).values
        for q in PU.LEVELS:
            lo, hi, frac = E.quantile_position(q, M)
            assert (lo, hi, frac) == PU.position(q, M)
            assert 0 <= lo <= hi <= M - 1 and hi - lo <= 1 and 0.0 <= frac < 1.0
            got = srt[lo] + frac * (srt[hi] - srt[lo])
            want = torch.quantile(x, q, dim=0, interpolation="linear")
            worst = max(worst, (got - want).abs().max().item())
    print(f"quantile position against torch.quantile: max difference {worst:.3e}")
    assert worst <= 1e-12 * 300
    for M in MS:                                   # the top level stays on the last member
        assert E.quantile_position(1.0, M) == (M - 1, M - 1, 0.0)
        if M % 2:
            assert E.quantile_position(0.5, M) == (M // 2, M // 2 + 1, 0.0)
    for q in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="level"):
            E.quantile_position(q, 4)


def _counts(M, shape, seed=0):
    ens, tar, w, thr = PU.inputs(M, shape, seed)
    return ens.double(), tar.double(), w.double(), thr


@pytest.mark.parametrize("M", [2, 5, 8, 17])
def test_finish_thresholds_against_the_per_pixel_forms(M):
    from msfno_amd import ensemble as E
    shape = (4, 9, 40)
    ens, tar, w, thr = _counts(M, shape)
    c = PU.counts(ens, tar, w, thr)
    assert c.shape == (4, 4, 2, M + 1)
    sc = E.finish_thresholds(c, w, shape[2], M)
    brier, fair, base = PU.pixel_scores(ens, tar, w, thr)
    assert torch.allclose(sc.brier, brier, rtol=0, atol=1e-12)
    assert torch.allclose(sc.fair_brier, fair, rtol=0, atol=1e-12)
    assert torch.allclose(sc.base_rate, base, rtol=0, atol=1e-12)
    assert torch.allclose(sc.reliability - sc.resolution + sc.uncertainty, sc.brier, rtol=0,
                          atol=1e-12)
    assert torch.allclose(sc.forecast_hist.sum(dim=-1), torch.ones(4, 4, dtype=torch.float64))
    assert sc.hit_rate.shape == sc.false_alarm_rate.shape == (4, 4, M + 2)
    # 296.0 is below every truth value here (and all but a few member values, 4 sigma down):
    # base rate 1, finite Brier terms, no non-event to falsely warn of
    assert (tar > 296.0).all()
    always = thr == 296.0
    assert always.sum() == 4 and ((sc.base_rate[always] - 1).abs() <= 1e-12).all()
    for name in ("brier", "fair_brier", "reliability", "resolution", "uncertainty"):
        assert torch.isfinite(getattr(sc, name)).all(), name
    assert (sc.brier[always] <= 5e-3).all() and (sc.uncertainty[always].abs() <= 1e-12).all()
    assert torch.isnan(sc.false_alarm_rate[always]).all()
    assert torch.isnan(sc.roc_area[always]).all()
    assert torch.isfinite(sc.hit_rate[always]).all()
    rest = ~always
    assert (sc.hit_rate[rest][:, 0] == 1).all() and (sc.hit_rate[rest][:, -1] == 0).all()
    assert (sc.false_alarm_rate[rest][:, 0] == 1).all()
    assert (sc.false_alarm_rate[rest][:, -1] == 0).all()
    assert (sc.hit_rate[rest].diff(dim=-1) <= 0).all()
    # the ROC area is the probability that an event pixel has more members above than a
    # non-event pixel, ties counting half (slab 0, threshold 300.0)
    s, t = 0, int((thr[0] == 300.0).nonzero()[0])
    Nk, Ok = c[s, t, 0], c[s, t, 1]
    Mk = Nk - Ok
    conc = sum(Ok[a] * (Mk[:a].sum() + 0.5 * Mk[a]) for a in range(M + 1))
    assert abs(sc.roc_area[s, t] - conc / (Ok.sum() * Mk.sum())) <= 1e-12


def test_roc_area_of_a_useless_and_of_a_perfect_ensemble():
    from msfno_amd import ensemble as E
    M, S, H, W = 8, 1, 60, 200
    g = torch.Generator().manual_seed(5)
    w = torch.rand(H, generator=g).double() + 0.1
    thr = torch.tensor([[300.0]])
    tar = 300 + torch.randn(S, H, W, generator=g).double()
    ens = 300 + torch.randn(M, S, H, W, generator=g).double()      # independent of the truth
    sc = E.finish_thresholds(PU.counts(ens, tar, w, thr), w, W, M)
    # 12000 pixels, about half of them events: the area's standard error is about
    # sqrt(1 / (12 * 3000)) = 0.005 (the Mann-Whitney variance bound); 5 of them
    assert abs(sc.roc_area.item() - 0.5) <= 0.025
    assert abs(sc.resolution.item()) <= 1e-3
    perfect = tar[None] + 0.01 * torch.randn(M, S, H, W, generator=g).double().clamp(-3, 3)
    far = (tar - 300.0).abs() > 0.05                # keep the members on the truth's side
    tar2 = torch.where(far, tar, tar + 0.2)
    perfect = torch.where(far[None], perfect, perfect + 0.2)
    sc = E.finish_thresholds(PU.counts(perfect, tar2, w, thr), w, W, M)
    assert sc.roc_area.item() == 1.0 and sc.brier.item() == 0.0
    assert abs(sc.resolution.item() - sc.uncertainty.item()) <= 1e-12


def test_counts_add_up_over_a_row_split():
    M, shape = 5, (3, 12, 33)
    ens, tar, w, thr = _counts(M, shape)
    whole = PU.counts(ens, tar, w, thr)
    parts = sum(PU.counts(ens[..., a:b, :], tar[..., a:b, :], w[a:b], thr)
                for a, b in ((0, 5), (5, 6), (6, 12)))
    assert torch.allclose(whole, parts, rtol=1e-13, atol=0)
    n = shape[2] * w.sum()
    assert torch.allclose(whole[..., 0, :].sum(dim=-1), n.expand(3, 4), rtol=1e-13)
    assert (whole[..., 1, :] <= whole[..., 0, :]).all()


def test_python_refusals():
    from msfno_amd import ensemble as E
    from msfno_amd.rollout import Rollout
    x = torch.zeros(3, 1, 2, 4, 8)
    t = torch.zeros(1, 2, 4, 8)
    w = torch.ones(4)
    thr = torch.zeros(2, 1)
    with pytest.raises(ValueError, match="GPU"):
        E.products(x)                                               # no CPU path
    with pytest.raises(ValueError, match="at least 2"):
        E.products(x[:1])
    with pytest.raises(NotImplementedError, match="at most 32"):
        E.products(torch.zeros(33, 1, 2, 4, 8))
    with pytest.raises(ValueError, match="must be"):
        E.products(x[0])
    with pytest.raises(ValueError, match="requires grad"):
        E.products(x.clone().requires_grad_())
    with pytest.raises(ValueError, match="GPU"):
        E.threshold_sums(x, t, w, thr)
    with pytest.raises(ValueError, match="at least 2"):
        E.threshold_sums(x[:1], t, w, thr)
    with pytest.raises(NotImplementedError, match="at most 32"):
        E.threshold_sums(torch.zeros(33, 1, 2, 4, 8), t, w, thr)
    with pytest.raises(ValueError, match="must be"):
        E.threshold_sums(x, t[0], w, thr)
    with pytest.raises(ValueError, match="requires grad: the threshold sums have no gradient"):
        E.threshold_sums(x.clone().requires_grad_(), t, w, thr)
    with pytest.raises(ValueError, match="requires grad"):
        E.threshold_sums(x, t.clone().requires_grad_(), w, thr)
    c = torch.zeros(1, 2, 1, 2, 4)
    with pytest.raises(ValueError, match="counts must be"):
        E.finish_thresholds(c, w, 8, 4)                              # M + 1 = 5 bins
    with pytest.raises(ValueError, match="counts must be"):
        E.finish_thresholds(c[..., 0, :], w, 8, 3)
    with pytest.raises(ValueError, match="at least 2"):
        E.finish_thresholds(c, w, 8, 1)
    assert E.finish_thresholds(c, w, 8, 3).brier.shape == (1, 2, 1)
    with pytest.raises(ValueError, match="at least 2"):
        E.EnsembleVerifier("uniform", 4, 8, 1, 1, 1, 2, device="cpu", thresholds=thr)

    class Sharded:
        world = 2

    with pytest.raises(NotImplementedError, match="ensemble.products"):
        Rollout(Sharded(), graph=False).ensemble_products(t[0].expand(3, 2, 4, 8), 1)


def test_c_abi_refusals_come_before_any_launch():
    """Every refusal is decided on the arguments alone: the pointers here are never
    dereferenced (this test runs without a GPU)."""
    import ctypes
    from msfno_amd import _native as N
    lib = N.lib()
    S, H, W = 2, 3, 8
    n = S * H * W
    p = 4096                       # any non-null address
    size = lib.msfno_ens_threshold_workspace_size(S, 4, 2, H, W)
    assert size > 0 and size % 4 == 0
    assert (lib.msfno_ens_threshold_workspace_size(S, 32, 8, H, W)
            >= lib.msfno_ens_threshold_workspace_size(S, 2, 1, H, W))
    for bad in ((0, 4, 2, H, W), (S, 1, 2, H, W), (S, 33, 2, H, W), (S, 4, 0, H, W),
                (S, 4, 9, H, W), (S, 4, 2, 0, W), (S, 4, 2, H, 0)):
        assert lib.msfno_ens_threshold_workspace_size(*bad) == 0

    def sums(ens=p, stride=n, tar=p, w=p, thr=p, nt=2, out=p, M=4, S=S, H=H, W=W, ws=p,
             nbytes=size):
        return lib.msfno_ens_threshold_sums(ens, stride, tar, w, thr, nt, out, M, S, H, W, ws,
                                            nbytes, None)

    for kw in (dict(ens=None), dict(tar=None), dict(w=None), dict(thr=None), dict(out=None),
               dict(ws=None), dict(S=0), dict(H=0), dict(W=0), dict(M=1), dict(M=0),
               dict(nt=0), dict(nt=-1), dict(stride=n - 1)):
        assert sums(**kw) == N.MSFNO_EINVAL, kw
    assert sums(M=33, nbytes=1 << 30) == N.MSFNO_EUNSUPPORTED
    assert sums(nt=9, nbytes=1 << 30) == N.MSFNO_EUNSUPPORTED
    assert sums(nbytes=size - 1) == N.MSFNO_EWORKSPACE
    with pytest.raises(ValueError, match="workspace"):
        N.check(sums(nbytes=0), "msfno_ens_threshold_sums")

    def products(ens=p, stride=n, levels=(0.5,), nq=None, thr=p, nt=2, M=4, S=S, H=H, W=W,
                 no_out=False, **fields):
        q = (ctypes.c_double * max(1, len(levels)))(*levels) if levels is not None else None
        o = dict(mean=p, std=p, min=p, max=p, quant=p, prob=p)
        o.update(fields)
        out = None if no_out else ctypes.byref(N.EnsProductsOut(**o))
        nq = (0 if levels is None else len(levels)) if nq is None else nq
        return lib.msfno_ens_products(ens, stride, q, nq, thr, nt, out, M, S, H, W, None)

    none = dict(mean=None, std=None, min=None, max=None, quant=None, prob=None)
    for kw in (dict(ens=None), dict(no_out=True), none, dict(S=0), dict(H=0), dict(W=0), dict(M=1),
               dict(stride=n - 1), dict(levels=(-0.01,)), dict(levels=(0.5, 1.01)),
               dict(levels=(float("nan"),)), dict(levels=()), dict(levels=None, nq=1),
               dict(nt=0), dict(thr=None), dict(nq=-1), dict(nt=-1, prob=None)):
        assert products(**kw) == N.MSFNO_EINVAL, kw
    assert products(M=33) == N.MSFNO_EUNSUPPORTED
    assert products(levels=(0.5,) * 9) == N.MSFNO_EUNSUPPORTED
    assert products(nt=9) == N.MSFNO_EUNSUPPORTED
    with pytest.raises(ValueError, match="level"):
        N.check(products(levels=(2.0,)), "msfno_ens_products")
    with pytest.raises(ValueError, match="no output"):
        N.check(products(**none), "msfno_ens_products")
    with pytest.raises(NotImplementedError, match="8"):
        N.check(products(nt=9), "msfno_ens_products")


def test_entry_points_are_declared_bound_and_exported():
    from msfno_amd import _native as N
    from msfno_amd import ensemble as E
    header = open(os.path.join(REPO, "include", "msfno.h")).read()
    declared = set(re.findall(r"\b(msfno_[a-z0-9_]+)\s*\(", header))
    bound = {n for n, _, _ in N.SIGNATURES}
    for s in SYMBOLS:
        assert s in declared and s in bound and hasattr(N.lib(), s), s
    assert N.lib().msfno_abi_version() == 6
    assert "#define MSFNO_ENS_MAX_LEVELS 8" in header and N.ENS_MAX_LEVELS == 8
    assert [f for f, _ in N.EnsProductsOut._fields_] == ["mean", "std", "min", "max", "quant",
                                                        "prob"]
    for name in ("products", "threshold_sums", "finish_thresholds", "EnsembleProducts",
                 "ThresholdScores"):
        assert hasattr(E, name), name
