"""Torch restatement of the ensemble products and the threshold scores (msfno_amd/ensemble.py,
csrc/ens_products.hip), written from the formulas, in the dtype of its inputs (the tests use
fp64), plus the shared problems of the GPU tests.

Members x_i (i < M), truth y, latitude weights w, thresholds thr (S, nt) per slab:
  mean, std (unbiased), min, max over the members, per pixel
  quantile q: pos = q (M - 1), lo = floor(pos), hi = min(lo + 1, M - 1), frac = pos - lo,
              x_(lo) + frac (x_(hi) - x_(lo)) on the sorted members (sort + index, not
              torch.quantile, which refuses large inputs)
  k = #{i : x_i > thr}, o = [y > thr] (strict), prob = k / M
  counts[s][t][0][k] = sum w [count == k],  counts[s][t][1][k] = sum w [count == k][o]
  per pixel: brier = (k/M - o)^2, fair = brier - k (M - k) / (M^2 (M - 1))."""
import functools
import math

import torch

import ensemble_util as EU

LEVELS = (0.0, 0.1, 0.25, 0.5, 0.9, 1.0)
THRESHOLDS = (296.0, 300.0, 300.7, 302.0)      # always, common, middling, rare


def position(q, M):
    pos = q * (M - 1)
    lo = min(math.floor(pos), M - 1)
    return lo, min(lo + 1, M - 1), pos - lo


def quantile(srt, q):
    """Level q of the members sorted along dimension 0; also x_(lo), x_(hi) and frac."""
    lo, hi, frac = position(q, srt.shape[0])
    return srt[lo] + frac * (srt[hi] - srt[lo]), srt[lo], srt[hi], frac


def exceed(ens, thr):
    """(nt, S, H, W) integer counts of the members of ens (M, S, H, W) above thr (S, nt)."""
    t = thr.to(ens.dtype).t()[:, None, :, None, None]           # (nt, 1, S, 1, 1)
    return (ens[None] > t).sum(dim=1)


def counts(ens, tar, w, thr):
    """(S, nt, 2, M + 1) weighted counts."""
    M = ens.shape[0]
    k = exceed(ens, thr)                                         # (nt, S, H, W)
    o = tar[None] > thr.to(tar.dtype).t()[:, :, None, None]
    w = w.to(ens.dtype)[:, None]
    rows = []
    for oo in (torch.ones_like(o), o):
        rows.append(torch.stack([(w * ((k == r) & oo).to(ens.dtype)).sum(dim=(-1, -2))
                                 for r in range(M + 1)], dim=-1))   # (nt, S, M + 1)
    return torch.stack(rows, dim=-2).transpose(0, 1).contiguous()   # (S, nt, 2, M + 1)


def pixel_scores(ens, tar, w, thr):
    """((S, nt) brier, (S, nt) fair brier, (S, nt) base rate): weighted per-pixel means."""
    M = ens.shape[0]
    k = exceed(ens, thr).to(ens.dtype)
    o = (tar[None] > thr.to(tar.dtype).t()[:, :, None, None]).to(ens.dtype)
    w = w.to(ens.dtype)[:, None]
    n = ens.shape[-1] * w.sum()

    def mean(x):
        return ((w * x).sum(dim=(-1, -2)) / n).t()

    b = (k / M - o) ** 2
    return mean(b), mean(b - k * (M - k) / (M * M * (M - 1))), mean(o)


def thresholds(S, nt=4):
    """(S, nt) fp32: the four thresholds, rotated by the slab."""
    return torch.tensor([[THRESHOLDS[(s + t) % 4] for t in range(nt)] for s in range(S)],
                        dtype=torch.float32)


def untie(x, thr):
    """x (..., S, H, W) with every value that equals one of its slab's thresholds moved to the
    next fp32 value (fp32 values near 300 are 3e-5 apart, so some do)."""
    for t in range(thr.shape[1]):
        tt = thr[:, t][:, None, None]
        x = torch.where(x == tt, torch.nextafter(x, torch.full_like(x, 1e9)), x)
    return x


def inputs(M, shape, seed=0, nt=4):
    """EU.inputs and (S, nt) thresholds, with no member and no truth value on a threshold of
    its slab (asserted), so that fp32 and fp64 counts are the same."""
    ens, tar, w = EU.inputs(M, shape, seed)
    thr = thresholds(shape[0], nt)
    ens, tar = untie(ens, thr), untie(tar, thr)
    for t in range(nt):
        tt = thr[:, t][:, None, None]
        assert not (ens == tt).any() and not (tar == tt).any()
    return ens, tar, w, thr


@functools.lru_cache(maxsize=None)
def problem(M, shape):
    """inputs(M, shape) with the sorted fp32 members and the fp64 counts; computed once,
    shared, never modified."""
    ens, tar, w, thr = inputs(M, shape)
    srt = ens.sort(dim=0).values
    return ens, tar, w, thr, srt, counts(ens.double(), tar.double(), w.double(), thr)
