"""Ensemble verification and the (fair) CRPS loss on the device.

One run carries a whole ensemble in the batch dimension (FiLM takes a (B, C) modulation
per batch element, so one replayed graph steps M members under M scenarios or M perturbed
initial states).  The reference has no ensemble score; these are the standard ones.  One
native pass (``msfno_ens_sums``, csrc/ensemble.hip) over the M members ``x_i`` and the
truth ``y`` leaves five latitude-weighted sums per (batch, channel), with
``dbar = (1/M) sum_i (x_i - y)``,

    se   = sum w dbar^2                      gini = sum w sum_{i<j} |x_i - x_j|
    err  = sum w dbar                        sq   = sum w sum_{i<j} (x_i - x_j)^2
    abs  = sum w (1/M) sum_i |x_i - y|

and the weighted rank counts ``hist[r] = sum w [#{i : x_i < y} == r]``, r = 0..M (strict
``<``); ``finish`` turns them into scores with plain torch.  Every per-pixel quantity is
formed from a difference (``x_i - y``, ``x_i - x_j``), never from raw values or a raw
mean, so a 300 K field with 1 K of spread keeps its digits; ``sq = M sum_i (x_i - xbar)^2``
gives the unbiased variance without cancellation.

The sums are additive over rows: a latitude-band rank calls ``ensemble_sums`` on its own
rows with ``w[rows]``, all-reduces the (B, C, 5) and (B, C, M + 1) results and finishes
with the whole grid's ``w``.

``EnsembleVerifier`` is the preallocated form for a rollout (one launch pair per scored
step into a slot, nothing synchronises); ``Rollout.verify_ensemble`` drives it.
``CRPSLoss`` is the training objective: the mean over (B, C) of
``(abs - kappa gini) / (nlon sum w)`` with ``kappa = 1 / (M (M - 1))`` (fair) or
``1 / M^2``, with the native gradient (``msfno_ens_crps_backward``) to the members only.

``perturb`` makes the members of such a run from one state and a
``harmonics.GaussianRandomFieldS2``.

``products`` turns the members into the maps a forecast is issued as (``msfno_ens_products``,
csrc/ens_products.hip): the ensemble mean and spread (from differences ``x_i - x_0``), the
extremes, quantiles of the sorted members (linear interpolation) and the probability of
exceeding a threshold, in one pass, each output optional.  The maps are row-local: a
latitude-band rank calls it on its own rows.  ``threshold_sums`` leaves, per (batch, channel)
and threshold, the weighted counts of pixels with k members above the threshold and of those
where the truth is above it too (``msfno_ens_threshold_sums``; additive over rows, so a band
rank passes its rows and ``w[rows]`` and all-reduces); ``finish_thresholds`` turns them into
the Brier score with its decomposition, the reliability diagram and the ROC curve.
``EnsembleVerifier(..., thresholds=)`` keeps them per scored step.  Inputs are finite: that
is the caller's contract and is not checked.
"""
from __future__ import annotations

import ctypes
import math
from collections import namedtuple

import torch
import torch.nn as nn

from . import _fields as F
from . import _native as N

NSUMS = 5
SE, ERR, ABS, GINI, SQ = range(NSUMS)
MAX_MEMBERS = 32

MAX_LEVELS = N.ENS_MAX_LEVELS

EnsembleProducts = namedtuple("EnsembleProducts", ["mean", "std", "min", "max", "quantiles",
                                                   "prob"])
ThresholdScores = namedtuple("ThresholdScores", ["base_rate", "brier", "fair_brier",
                                                 "reliability", "resolution", "uncertainty",
                                                 "forecast_hist", "observed_freq", "hit_rate",
                                                 "false_alarm_rate", "roc_area"])
EnsembleScores = namedtuple("EnsembleScores", ["mse", "rmse", "bias", "mae", "crps", "fair_crps",
                                               "spread", "spread_skill", "rank_hist"])


def _members(ens, name="ens"):
    """``ens`` as fp32 device (M, B, C, H, W) with the inner four dimensions contiguous and a
    member stride of at least one member (a view into a larger buffer stays a view;
    anything else, an expanded member included, is copied)."""
    if not ens.is_cuda:
        raise ValueError(f"{name} must be a GPU (HIP) tensor; libmsfno has no CPU path")
    if ens.dtype != torch.float32:
        ens = ens.float()
    inner = ens[0]
    if not inner.is_contiguous() or (ens.shape[0] > 1 and ens.stride(0) < inner.numel()):
        ens = ens.contiguous()
    return ens


def _check_count(M):
    if M < 2:
        raise ValueError(f"an ensemble has at least 2 members, got {M}")
    if M > MAX_MEMBERS:
        raise NotImplementedError(f"at most {MAX_MEMBERS} members, got {M}")


def _check_members(ens, tar, w, grad_ok=False):
    if ens.dim() != 5 or tar.dim() != 4 or ens.shape[1:] != tar.shape:
        raise ValueError(f"ens must be (M, B, C, H, W) and tar (B, C, H, W), got "
                         f"{tuple(ens.shape)} and {tuple(tar.shape)}")
    _check_count(ens.shape[0])
    return F.check_fields(ens, tar, w, "ens", _members,
                          None if grad_ok else ("ensemble", "CRPSLoss"))


@torch.no_grad()
def perturb(x0, M, grf, amplitude=1.0, centred=True):
    """(M, C, H, W) perturbed copies of the state ``x0`` (C, H, W) or (1, C, H, W): what
    ``Rollout.verify_ensemble`` takes as its members.  ``grf`` is a
    ``harmonics.GaussianRandomFieldS2`` on the (H, W) grid with one spectrum per channel
    (K = C) or one for all; ``amplitude`` is a scalar or (C,) and scales the field, so with
    ``harmonics.unit_variance`` spectra it is a standard deviation in the units of ``x0``.
    ``centred``: members 2k and 2k + 1 are ``x0 + amplitude field_k`` and ``x0 - amplitude
    field_k``, so the member mean is ``x0`` (M must be even); otherwise every member has a
    field of its own.  Consumes one draw of ``grf``."""
    _check_count(M)
    if centred and M % 2:
        raise ValueError(f"a centred ensemble has an even number of members, got {M}")
    if x0.dim() == 4 and x0.shape[0] == 1:
        x0 = x0[0]
    if x0.dim() != 3:
        raise ValueError(f"x0 must be (C, H, W) or (1, C, H, W), got {tuple(x0.shape)}")
    C, H, W = x0.shape
    if (H, W) != (grf.nlat, grf.nlon):
        raise ValueError(f"x0 is on a {(H, W)} grid, the field on {(grf.nlat, grf.nlon)}")
    if grf.nrows not in (1, C):
        raise ValueError(f"the field has {grf.K} spectra, x0 has {C} channels")
    x0 = N.require_device_f32(x0, "x0")
    n = M // 2 if centred else M
    # K = C: (n, C, H, W) as sampled; one spectrum: n * C independent fields of it
    field = (grf(n) if grf.nrows == C and grf.K is not None else grf(n * C)).view(n, C, H, W)
    amp = torch.as_tensor(amplitude, dtype=torch.float32, device=x0.device)
    if amp.dim() > 1 or (amp.dim() == 1 and amp.shape[0] != C):
        raise ValueError(f"amplitude must be a scalar or ({C},), got {tuple(amp.shape)}")
    d = field * (amp.view(C, 1, 1) if amp.dim() else amp)
    if not centred:
        return x0 + d
    out = torch.empty(M, C, H, W, dtype=torch.float32, device=x0.device)
    out[0::2] = x0 + d
    out[1::2] = x0 - d
    return out


def workspace(M: int, B: int, C: int, nlat: int, nlon: int, device) -> torch.Tensor:
    """A workspace for ``msfno_ens_sums`` at this shape (contents do not matter)."""
    return torch.empty(N.lib().msfno_ens_workspace_size(B * C, M, nlat, nlon),
                       dtype=torch.uint8, device=device)


@N.on_input_device
def _launch(ens, tar, w, sums, hist, ws):
    M, B, C, H, W = ens.shape
    N.check(N.lib().msfno_ens_sums(ens.data_ptr(), ens.stride(0), tar.data_ptr(), w.data_ptr(),
                                   sums.data_ptr(), N.ptr(hist), M, B * C, H, W, ws.data_ptr(),
                                   ws.numel(), N.stream_of(ens.device)), "msfno_ens_sums")
    return sums, hist


@torch.no_grad()
def ensemble_sums(ens, tar, w, hist=True):
    """((B, C, 5) fp32 = {se, err, abs, gini, sq}, (B, C, M + 1) fp32 rank counts or None)
    of the members ``ens`` (M, B, C, H, W) against ``tar`` (B, C, H, W), fp32 device fields,
    under the latitude weights ``w`` (any fp32 device vector of length H).  The members may
    be views into a larger buffer (any member stride).  2 <= M <= 32.  No gradient."""
    ens, tar, w = _check_members(ens, tar, w)
    M, B, C, H, W = ens.shape
    sums = torch.empty(B, C, NSUMS, dtype=torch.float32, device=ens.device)
    h = torch.empty(B, C, M + 1, dtype=torch.float32, device=ens.device) if hist else None
    return _launch(ens, tar, w, sums, h, workspace(M, B, C, H, W, ens.device))


def _kappa(M: int, fair: bool) -> float:
    return 1.0 / (M * (M - 1)) if fair else 1.0 / (M * M)


def finish(sums, hist, w, nlon, M) -> EnsembleScores:
    """Scores from (..., 5) sums and (..., M + 1) rank counts (or None) taken under the
    weights ``w`` of the whole grid, with n = nlon * sum(w):

        mse = se / n, rmse = sqrt(mse), bias = err / n   (of the ensemble mean)
        mae = abs / n                                    (mean over the members)
        crps = (abs - gini / M^2) / n,  fair_crps = (abs - gini / (M (M - 1))) / n
        spread = sqrt(sq / (M (M - 1)) / n)              (root of the mean unbiased variance)
        spread_skill = sqrt((M + 1) / M) spread / rmse   (1 for a reliable ensemble)
        rank_hist = hist / n                             (rows sum to 1)"""
    if sums.shape[-1] != NSUMS:
        raise ValueError(f"sums must be (..., {NSUMS}), got {tuple(sums.shape)}")
    if M < 2:
        raise ValueError(f"an ensemble has at least 2 members, got {M}")
    if hist is not None and (hist.shape[-1] != M + 1 or hist.shape[:-1] != sums.shape[:-1]):
        raise ValueError(f"hist must be {tuple(sums.shape[:-1]) + (M + 1,)}, got "
                         f"{tuple(hist.shape)}")
    n = F.grid_weight(w, nlon, sums.device).to(sums.dtype)
    se, err, ab, gini, sq = sums.unbind(-1)
    mse = se / n
    rmse = torch.sqrt(mse)
    spread = torch.sqrt(sq / (M * (M - 1)) / n)
    return EnsembleScores(mse, rmse, err / n, ab / n, (ab - gini / (M * M)) / n,
                          (ab - gini / (M * (M - 1))) / n, spread,
                          math.sqrt((M + 1) / M) * spread / rmse,
                          None if hist is None else hist.to(sums.dtype) / n)


def quantile_position(q: float, M: int):
    """(lo, hi, frac) of level ``q`` among M sorted members, as the C side forms it in fp64:
    ``pos = q (M - 1)``, ``lo = floor(pos)``, ``hi = min(lo + 1, M - 1)``, ``frac = pos - lo``;
    the value is ``x_(lo) + frac (x_(hi) - x_(lo))`` (torch's linear interpolation)."""
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"a quantile level must be in [0, 1], got {q}")
    pos = float(q) * (M - 1)
    lo = min(int(math.floor(pos)), M - 1)
    return lo, min(lo + 1, M - 1), pos - lo


def _thresholds(thr, B, C, device):
    """``thr`` (C, nt) or (B, C, nt) as fp32 device (B, C, nt), contiguous."""
    thr = N.require_device_f32(thr, "thresholds")
    if thr.dim() == 2:
        thr = thr.unsqueeze(0).expand(B, *thr.shape)
    if thr.dim() != 3 or tuple(thr.shape[:2]) != (B, C) or thr.shape[2] < 1:
        raise ValueError(f"thresholds must be ({C}, nt) or ({B}, {C}, nt) with nt >= 1, got "
                         f"{tuple(thr.shape)}")
    if thr.device != device:
        raise ValueError("ens and thresholds must be on one device")
    return thr.contiguous()


@N.on_input_device
def _products_launch(ens, levels, thr, out):
    """One call of at most MAX_LEVELS levels and thresholds; ``out`` maps the names of
    ``msfno_ens_products_out`` to tensors."""
    M, B, C, H, W = ens.shape
    q = (ctypes.c_double * max(1, len(levels)))(*levels)
    o = N.EnsProductsOut(**{k: N.ptr(v) for k, v in out.items()})
    nt = 0 if thr is None else thr.shape[-1]
    N.check(N.lib().msfno_ens_products(ens.data_ptr(), ens.stride(0), q, len(levels),
                                       N.ptr(thr), nt, ctypes.byref(o), M, B * C, H, W,
                                       N.stream_of(ens.device)), "msfno_ens_products")


@torch.no_grad()
def products(ens, quantiles=(), thresholds=None, mean=True, std=True, minmax=False):
    """``EnsembleProducts(mean, std, min, max, quantiles, prob)`` of the members ``ens``
    (M, B, C, H, W), per pixel; fields not asked for are None.  ``mean`` and ``std`` (the
    unbiased spread, exactly 0 for equal members) are formed from the differences
    ``x_i - x_0``; ``min`` and ``max`` (``minmax``) are members bit for bit; ``quantiles``
    (nq, B, C, H, W) are the levels ``quantiles`` in [0, 1] of the sorted members with linear
    interpolation (torch's default), a member bit for bit where the level falls on one;
    ``prob`` (nt, B, C, H, W) is the fraction of members strictly above ``thresholds``
    ((C, nt) or (B, C, nt), in field units).  One native pass; more than 8 levels or
    thresholds take one more pass per 8.  The members may be views into a larger buffer (any
    member stride) and must be finite (not checked).  2 <= M <= 32.  No gradient.  The maps
    are row-local: a latitude-band rank passes its own rows."""
    if ens.dim() != 5:
        raise ValueError(f"ens must be (M, B, C, H, W), got {tuple(ens.shape)}")
    _check_count(ens.shape[0])
    if ens.requires_grad:
        raise ValueError("ens requires grad: the ensemble products have no gradient; pass "
                         "ens.detach() (for training use CRPSLoss)")
    ens = _members(ens)
    if ens.numel() == 0:
        raise ValueError("empty fields")
    M, B, C, H, W = ens.shape
    levels = [float(q) for q in quantiles]
    for q in levels:
        quantile_position(q, M)
    thr = None if thresholds is None else _thresholds(torch.as_tensor(thresholds), B, C,
                                                      ens.device)
    if not (mean or std or minmax or levels or thr is not None):
        raise ValueError("no product asked for")

    def new(*lead):
        return torch.empty(*lead, B, C, H, W, dtype=torch.float32, device=ens.device)

    res = dict(mean=new() if mean else None, std=new() if std else None,
               min=new() if minmax else None, max=new() if minmax else None,
               quant=new(len(levels)) if levels else None,
               prob=new(thr.shape[-1]) if thr is not None else None)
    nt = 0 if thr is None else thr.shape[-1]
    first = True
    for a in range(0, max(len(levels), nt, 1), MAX_LEVELS):
        lv = levels[a:a + MAX_LEVELS]
        th = None if thr is None or a >= nt else thr[..., a:a + MAX_LEVELS].contiguous()
        out = {k: res[k] if first else None for k in ("mean", "std", "min", "max")}
        out["quant"] = res["quant"][a:a + MAX_LEVELS] if lv else None
        out["prob"] = res["prob"][a:a + MAX_LEVELS] if th is not None else None
        _products_launch(ens, lv, th, out)
        first = False
    return EnsembleProducts(res["mean"], res["std"], res["min"], res["max"], res["quant"],
                            res["prob"])


def threshold_workspace(M: int, B: int, C: int, nt: int, nlat: int, nlon: int,
                        device) -> torch.Tensor:
    """A workspace for ``msfno_ens_threshold_sums`` at this shape and up to MAX_LEVELS
    thresholds a call (contents do not matter)."""
    nbytes = N.lib().msfno_ens_threshold_workspace_size(B * C, M, min(nt, MAX_LEVELS), nlat,
                                                        nlon)
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


@N.on_input_device
def _threshold_launch(ens, tar, w, thr, counts, ws):
    """``counts`` (B, C, nt, 2, M + 1), written whole; more than MAX_LEVELS thresholds in
    calls of MAX_LEVELS (through a contiguous block of counts each)."""
    M, B, C, H, W = ens.shape
    nt = thr.shape[-1]
    for a in range(0, nt, MAX_LEVELS):
        n = min(MAX_LEVELS, nt - a)
        whole = a == 0 and n == nt
        th = thr if whole else thr[..., a:a + n].contiguous()
        c = counts if whole else torch.empty(B, C, n, 2, M + 1, dtype=torch.float32,
                                             device=ens.device)
        N.check(N.lib().msfno_ens_threshold_sums(
            ens.data_ptr(), ens.stride(0), tar.data_ptr(), w.data_ptr(), th.data_ptr(), n,
            c.data_ptr(), M, B * C, H, W, ws.data_ptr(), ws.numel(), N.stream_of(ens.device)),
            "msfno_ens_threshold_sums")
        if not whole:
            counts[:, :, a:a + n] = c
    return counts


@torch.no_grad()
def threshold_sums(ens, tar, w, thresholds):
    """(B, C, nt, 2, M + 1) fp32 weighted counts of the members ``ens`` (M, B, C, H, W) and
    the truth ``tar`` (B, C, H, W) against ``thresholds`` ((C, nt) or (B, C, nt), in field
    units) under the latitude weights ``w``: with k the number of members strictly above the
    threshold at a pixel, ``[..., 0, k]`` is the weight of the pixels with that k and
    ``[..., 1, k]`` of those among them where the truth is strictly above it too.  Additive
    over rows (a latitude-band rank passes its rows and ``w[rows]`` and all-reduces), exact
    integer counts per row, no atomics on floats: two calls give the same bits.  No
    gradient."""
    for n, t in (("ens", ens), ("tar", tar), ("w", w)):
        if t.requires_grad:
            raise ValueError(f"{n} requires grad: the threshold sums have no gradient; pass "
                             f"{n}.detach() (for training use CRPSLoss)")
    ens, tar, w = _check_members(ens, tar, w, grad_ok=True)
    M, B, C, H, W = ens.shape
    thr = _thresholds(torch.as_tensor(thresholds), B, C, ens.device)
    counts = torch.empty(B, C, thr.shape[-1], 2, M + 1, dtype=torch.float32, device=ens.device)
    return _threshold_launch(ens, tar, w, thr, counts,
                             threshold_workspace(M, B, C, thr.shape[-1], H, W, ens.device))


def finish_thresholds(counts, w, nlon, M) -> ThresholdScores:
    """Scores of the probability forecasts ``p_k = k / M`` of the event "above the
    threshold" from (..., 2, M + 1) counts taken under the weights ``w`` of the whole grid,
    in the dtype of ``counts``.  With n = nlon * sum(w), N_k = counts[..., 0, k],
    O_k = counts[..., 1, k] and obar = sum_k O_k / n:

        base_rate = obar
        brier = sum_k [p_k^2 (N_k - O_k) + (1 - p_k)^2 O_k] / n
        fair_brier = brier - sum_k N_k k (M - k) / (M^2 (M - 1)) / n   (unbiased in M)
        reliability = sum_k N_k (p_k - O_k / N_k)^2 / n     (bins with N_k = 0 give 0)
        resolution = sum_k N_k (O_k / N_k - obar)^2 / n
        uncertainty = obar (1 - obar);  brier = reliability - resolution + uncertainty
        forecast_hist = N_k / n, observed_freq = O_k / N_k  (the reliability diagram; NaN
                                                            where N_k = 0)
        hit_rate[j], false_alarm_rate[j], j = 0..M + 1: of "warn when k >= j", from (1, 1) to
        (0, 0); roc_area their trapezoid

    Where the base rate is 0 (1) the hit rate (false alarm rate) and the ROC area are NaN,
    as the plain division gives; the Brier terms stay finite."""
    if M < 2:
        raise ValueError(f"an ensemble has at least 2 members, got {M}")
    if counts.dim() < 2 or tuple(counts.shape[-2:]) != (2, M + 1):
        raise ValueError(f"counts must be (..., 2, {M + 1}), got {tuple(counts.shape)}")
    n = F.grid_weight(w, nlon, counts.device).to(counts.dtype)
    Nk, Ok = counts[..., 0, :], counts[..., 1, :]
    k = torch.arange(M + 1, dtype=counts.dtype, device=counts.device)
    p = k / M
    # sums over k >= j, j = 0..M + 1 (the last is 0): the events and the non-events warned of;
    # their totals are the first entries, so the curves start at (1, 1) exactly
    zero = torch.zeros_like(Ok[..., :1])
    miss = Nk - Ok
    hits = torch.cat([Ok.flip(-1).cumsum(dim=-1).flip(-1), zero], dim=-1)
    fals = torch.cat([miss.flip(-1).cumsum(dim=-1).flip(-1), zero], dim=-1)
    obar = hits[..., 0] / n
    brier = (p * p * miss + (1 - p) ** 2 * Ok).sum(dim=-1) / n
    fair = brier - (Nk * (k * (M - k))).sum(dim=-1) / (M * M * (M - 1)) / n
    some = Nk > 0
    freq = Ok / Nk
    f0 = torch.where(some, freq, torch.zeros_like(freq))
    rel = (Nk * (p - f0) ** 2).sum(dim=-1) / n
    res = (Nk * torch.where(some, f0 - obar[..., None], torch.zeros_like(f0)) ** 2).sum(dim=-1) / n
    hr = hits / hits[..., :1]
    far = fals / fals[..., :1]
    area = ((far[..., :-1] - far[..., 1:]) * (hr[..., :-1] + hr[..., 1:])).sum(dim=-1) / 2
    return ThresholdScores(obar, brier, fair, rel, res, obar * (1 - obar), Nk / n, freq, hr, far,
                           area)


class EnsembleVerifier(F.SlotVerifier):
    """The sums and rank counts of ``n_scored`` scored steps of an M-member rollout of
    (B, C, nlat, nlon) fields, in preallocated (n_scored, B, C, 5) ``sums`` and
    (n_scored, B, C, M + 1) ``hist`` device tensors with one workspace.  ``weights`` as
    ``verification.Verifier`` takes them.  ``update`` launches into a slot and never
    synchronises, so it records into a graph; a slot that was never updated holds NaN.

    With ``thresholds`` ((C, nt) or (B, C, nt), in field units) it also keeps the threshold
    counts of every scored step in a (n_scored, B, C, nt, 2, M + 1) ``tcounts`` (one more
    launch pair per ``update``, a second workspace); ``threshold_scores`` finishes them."""

    def __init__(self, weights, nlat, nlon, n_scored, M, B, C, device="cuda", thresholds=None):
        _check_count(M)
        super().__init__(weights, nlat, nlon, n_scored, B, C, device)
        self.M = M
        self.shape = (M, B, C, nlat, nlon)
        self.sums = self._alloc(NSUMS)
        self.hist = self._alloc(M + 1)
        self._ws = workspace(M, B, C, nlat, nlon, self.device)
        if thresholds is not None:
            thr = torch.as_tensor(thresholds).detach().to(self.device)
            self.thresholds = _thresholds(thr, B, C, self.device)
            nt = self.thresholds.shape[-1]
            self.tcounts = torch.full((n_scored, B, C, nt, 2, M + 1), float("nan"),
                                      dtype=torch.float32, device=self.device)
            self._tws = threshold_workspace(M, B, C, nt, nlat, nlon, self.device)

    @torch.no_grad()
    def update(self, k, ens, tar):
        """Score the members ``ens`` (M, B, C, nlat, nlon) against ``tar`` into slot ``k``.
        A host ``tar`` is copied with non_blocking=True."""
        self._check_slot(k, ens, "members")
        ens, tar, w = _check_members(ens, self._on_device(tar), self.w)
        _launch(ens, tar, w, self.sums[k], self.hist[k], self._ws)
        if getattr(self, "tcounts", None) is not None:
            _threshold_launch(ens, tar, w, self.thresholds, self.tcounts[k], self._tws)

    def scores(self) -> EnsembleScores:
        """``finish`` of all slots: EnsembleScores of (n_scored, B, C) tensors and the
        (n_scored, B, C, M + 1) rank histograms."""
        return finish(self.sums, self.hist, self.w, self.shape[4], self.M)

    def threshold_scores(self) -> ThresholdScores:
        """``finish_thresholds`` of all slots: ThresholdScores of (n_scored, B, C, nt)
        tensors (and their (…, M + 1) and (…, M + 2) curves)."""
        if getattr(self, "tcounts", None) is None:
            raise ValueError("this verifier was built without thresholds")
        return finish_thresholds(self.tcounts, self.w, self.shape[4], self.M)


@N.on_input_device
def _native_backward(ens, tar, w, g, kappa):
    M, B, C, H, W = ens.shape
    dens = torch.empty((M, B, C, H, W), dtype=torch.float32, device=ens.device)
    N.check(N.lib().msfno_ens_crps_backward(ens.data_ptr(), ens.stride(0), tar.data_ptr(),
                                            w.data_ptr(), g.data_ptr(), kappa, dens.data_ptr(),
                                            dens.stride(0), M, B * C, H, W,
                                            N.stream_of(ens.device)), "msfno_ens_crps_backward")
    return dens


class _CRPSSums(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ens, tar, w, kappa):
        ctx.save_for_backward(ens, tar, w)
        ctx.kappa = kappa
        M, B, C, H, W = ens.shape
        sums = torch.empty(B, C, NSUMS, dtype=torch.float32, device=ens.device)
        _launch(ens, tar, w, sums, None, workspace(M, B, C, H, W, ens.device))
        return sums[..., ABS] - kappa * sums[..., GINI]

    @staticmethod
    def backward(ctx, grad):
        ens, tar, w = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        g = N.require_device_f32(grad, "grad")
        return _native_backward(ens, tar, w, g, ctx.kappa), None, None, None


def crps_sums(ens, tar, w, fair=True):
    """(B, C) = abs - kappa gini, the unnormalised (fair) CRPS of ``ens`` (M, B, C, H, W)
    against ``tar`` under the latitude weights ``w``; differentiable in ``ens``.  The
    band-local entry: a latitude-band rank passes its rows and ``w[rows]`` and all-reduces."""
    if tar.requires_grad:
        raise NotImplementedError(
            "the gradient with respect to the target is not implemented; pass tar.detach()")
    ens, tar, w = _check_members(ens, tar, w.detach(), grad_ok=True)
    return _CRPSSums.apply(ens, tar, w, _kappa(ens.shape[0], fair))


class CRPSLoss(nn.Module):
    """The mean over (B, C) of the latitude-weighted CRPS of M members (M, B, C, H, W)
    against the truth (B, C, H, W):  (abs - kappa gini) / (W sum w), kappa = 1 / (M (M - 1))
    (``fair``: unbiased in the ensemble size, the usual objective for ensemble fine-tuning)
    or 1 / M^2.  ``weights`` is one of ``losses.KINDS`` or an fp32 vector of H weights."""

    def __init__(self, weights="cosine", fair=True):
        super().__init__()
        self.weights = weights
        self.fair = fair

    def forward(self, ens, tar):
        if ens.dim() != 5:
            raise ValueError(f"ens must be (M, B, C, H, W), got {tuple(ens.shape)}")
        w = F.lat_weights(self.weights, ens.shape[3], ens.device)
        if not isinstance(w, torch.Tensor):
            w = torch.as_tensor(w, dtype=torch.float32)
        s = crps_sums(ens, tar, w, fair=self.fair)
        return s.mean() / F.grid_weight(w, ens.shape[4], s.device).to(s.dtype)
