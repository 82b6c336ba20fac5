"""Torch restatement of the ensemble verification and the CRPS (msfno_amd/ensemble.py,
csrc/ensemble.hip), written from the formulas, in the dtype of its inputs (the tests use
fp64), plus the shared problems of the GPU tests.

Members x_i (i < M), truth y, latitude weights w; per slab, summed over its pixels, with
dbar = (1/M) sum_i (x_i - y):
  se = sum w dbar^2    err = sum w dbar    abs = sum w (1/M) sum_i |x_i - y|
  gini = sum w sum_{i<j} |x_i - x_j|       sq = sum w sum_{i<j} (x_i - x_j)^2
  hist[r] = sum w [#{i : x_i < y} == r], r = 0..M
  n = nlon sum(w):  mse = se/n, rmse, bias = err/n, mae = abs/n, crps = (abs - gini/M^2)/n,
  fair_crps = (abs - gini/(M(M-1)))/n, spread = sqrt(sq/(M(M-1))/n),
  spread_skill = sqrt((M+1)/M) spread/rmse, rank_hist = hist/n."""
import functools

import torch

NAMES = ("mse", "rmse", "bias", "mae", "crps", "fair_crps", "spread", "spread_skill")
SE, ERR, ABS, GINI, SQ = range(5)


def tol(M):
    """The bound of the GPU sums relative to their magnitude sums: the project's chain bound
    (3 + 128) of tests/test_gpu_loss.py, 2 (M + 2) for the member mean, squared, and
    M (M - 1) / 2 for the pair loop in any summation order, in units of 2^-24."""
    return (131 + 2 * (M + 2) + M * (M - 1) / 2) * 2.0 ** -24


def _pairs(ens):
    """(sum_{i<j} |x_i - x_j|, sum_{i<j} (x_i - x_j)^2) per pixel, without an (M, M, ...)
    tensor."""
    M = ens.shape[0]
    g = torch.zeros_like(ens[0])
    q = torch.zeros_like(ens[0])
    for i in range(M - 1):
        d = ens[i:i + 1] - ens[i + 1:]
        g = g + d.abs().sum(dim=0)
        q = q + (d * d).sum(dim=0)
    return g, q


def sums(ens, tar, w):
    """((..., 5) sums, (..., 5) magnitude sums) of ens (M, ..., H, W) against tar
    (..., H, W) under w (H): the magnitude sum of se is sum w ((1/M) sum |x_i - y|)^2, of
    err it is sum w (1/M) sum |x_i - y|, and abs, gini, sq are their own."""
    w = w.to(ens.dtype)[:, None]
    d = ens - tar
    dbar = d.mean(dim=0)
    ad = d.abs().mean(dim=0)
    g, q = _pairs(ens)

    def red(x):
        return (w * x).sum(dim=(-1, -2))

    want = torch.stack([red(dbar * dbar), red(dbar), red(ad), red(g), red(q)], dim=-1)
    mag = torch.stack([red(ad * ad), red(ad), red(ad), red(g), red(q)], dim=-1)
    return want, mag


def hist(ens, tar, w):
    """(..., M + 1) weighted rank counts, strict <."""
    M = ens.shape[0]
    rank = (ens < tar).sum(dim=0)
    w = w.to(ens.dtype)[:, None]
    return torch.stack([(w * (rank == r).to(ens.dtype)).sum(dim=(-1, -2)) for r in range(M + 1)],
                       dim=-1)


def crps_sums(ens, tar, w, kappa):
    """(...,) = abs - kappa gini; differentiable (torch's |.| has sign(0) = 0)."""
    w = w.to(ens.dtype)[:, None]
    g, _ = _pairs(ens)
    return (w * ((ens - tar).abs().mean(dim=0) - kappa * g)).sum(dim=(-1, -2))


def kappa(M, fair):
    return 1.0 / (M * (M - 1)) if fair else 1.0 / (M * M)


def scores(s, h, w, nlon, M):
    """dict of the scores (and rank_hist) from (..., 5) sums and (..., M + 1) counts."""
    n = nlon * w.to(s.dtype).sum()
    se, err, ab, gini, sq = s.unbind(-1)
    mse = se / n
    spread = (sq / (M * (M - 1)) / n).sqrt()
    return dict(mse=mse, rmse=mse.sqrt(), bias=err / n, mae=ab / n,
                crps=(ab - gini / M ** 2) / n, fair_crps=(ab - gini / (M * (M - 1))) / n,
                spread=spread, spread_skill=((M + 1) / M) ** 0.5 * spread / mse.sqrt(),
                rank_hist=None if h is None else h / n)


def inputs(M, shape, seed=0):
    """fp32 members 300 + N(0, 1) (M, S, H, W) against the truth 300.5 + N(0, 1) (S, H, W):
    a raw mean or a raw square would lose 5 digits to cancellation.  A member that equals
    the truth (fp32 values near 300 are 3e-5 apart, so some do) is moved to the next fp32
    value, so that no x_i == y tie remains and ranks compare exactly."""
    S, H, W = shape
    g = torch.Generator().manual_seed(7000 + 1000 * M + 100 * S + 10 * H + W + seed)
    tar = (300.5 + torch.randn(S, H, W, generator=g)).float()
    ens = (300.0 + torch.randn(M, S, H, W, generator=g)).float()
    ens = torch.where(ens == tar, torch.nextafter(ens, torch.full_like(ens, 1e9)), ens)
    w = (torch.rand(H, generator=g) + 0.1).float()
    return ens, tar, w


@functools.lru_cache(maxsize=None)
def problem(M, shape):
    """inputs(M, shape) with the fp64 sums, magnitude sums and rank counts; computed once,
    shared, never modified."""
    ens, tar, w = inputs(M, shape)
    want, mag = sums(ens.double(), tar.double(), w.double())
    return ens, tar, w, want, mag, hist(ens.double(), tar.double(), w.double())
