"""Torch restatement of the forecast verification (msfno_amd/verification.py,
csrc/verify.hip), written from the formulas, in the dtype of its inputs (the tests use
fp64), plus the shared problems of the GPU tests.

Per (b, c), with c the climatology slab clim[slab[bc]] (none where slab[bc] < 0):
  se = sum w (p-t)^2   err = sum w (p-t)     ae = sum w |p-t|
  pa2 = sum w (p-c)^2  ta2 = sum w (t-c)^2   cross = sum w (p-c)(t-c)
  n = nlon sum(w):  mse = se/n, rmse = sqrt(mse), bias = err/n, mae = ae/n,
  skill = 1 - se/ta2, acc = cross / sqrt(pa2 ta2); the last two NaN without a climatology."""
import functools

import torch

NAMES = ("mse", "rmse", "bias", "mae", "skill", "acc")


def sums(prd, tar, w, clim=None, slab=None):
    """((B, C, 6) sums, (B, C, 6) magnitude sums: the same with every term's absolute
    value).  clim (K, H, W) and slab a sequence of B * C slab indices (-1 = none)."""
    B, C, H, W = prd.shape
    w = w.to(prd.dtype)[None, None, :, None]
    d = prd - tar
    zero = torch.zeros(B, C, dtype=prd.dtype)
    if clim is None:
        pa = ta = None
    else:
        idx = torch.as_tensor(slab, dtype=torch.int64).reshape(B, C)
        has = (idx >= 0)[:, :, None, None].to(prd.dtype)
        c = clim.to(prd.dtype)[idx.clamp(min=0)]
        pa, ta = (prd - c) * has, (tar - c) * has

    def red(x):
        return zero if x is None else (w * x).sum(dim=(-1, -2))

    terms = [d * d, d, d.abs()] + ([None] * 3 if pa is None else [pa * pa, ta * ta, pa * ta])
    return (torch.stack([red(x) for x in terms], dim=-1),
            torch.stack([red(None if x is None else x.abs()) for x in terms], dim=-1))


def scores(s, w, nlon, has_clim, batch_mean=False):
    """dict of the six scores from (B, C, 6) sums; has_clim (B, C) bool."""
    n = nlon * w.to(s.dtype).sum()
    if batch_mean:
        n = n * s.shape[0]
        s = s.sum(dim=0)
        has_clim = has_clim.all(dim=0)
    se, err, ae, pa2, ta2, cross = s.unbind(-1)
    nan = torch.full_like(se, float("nan"))
    mse = se / n
    return dict(mse=mse, rmse=mse.sqrt(), bias=err / n, mae=ae / n,
                skill=torch.where(has_clim, 1 - se / ta2, nan),
                acc=torch.where(has_clim, cross / (pa2 * ta2).sqrt(), nan))


def slab_maps(B, C):
    """The climatology maps of the tests as (name, rows, slab): the stack is
    problem(shape)'s climatology[rows] and slab the list of B * C indices into it.  None;
    one slab for every (b, c); and a mixed one: some -1 (all of them at B C = 1), the rest
    a batch-broadcast (every sample of a channel reads one slab, sample 0's) from a stack
    in reversed channel order."""
    full = list(range(B * C))
    mixed = []
    for b in range(B):
        for c in range(C):
            mixed.append(-1 if (c % 3 == 1 or B * C == 1) else (C - 1 - c))
    return [("none", None, None), ("full", full, full),
            ("mixed", [C - 1 - j for j in range(C)], mixed)]


@functools.lru_cache(maxsize=None)
def problem(shape):
    """fp32 inputs (channel scales 1e-3 .. 1e4, as test_gpu_loss._problem), weights, a
    (B C, H, W) climatology stack near the truth, and per map of slab_maps the fp64 sums
    and magnitude sums; computed once, shared, never modified."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(2000 + B + 10 * C + 100 * H + W)
    scale = torch.logspace(-3, 4, C)[None, :, None, None] if C > 1 else torch.ones(1, 1, 1, 1)
    tar = ((torch.randn(shape, generator=g) + 0.5) * scale).float()
    prd = (tar + 0.3 * scale * torch.randn(shape, generator=g)).float()
    clim = ((torch.randn(shape, generator=g) * 0.7 + 0.5) * scale).float().reshape(B * C, H, W)
    w = (torch.rand(H, generator=g) + 0.1).float()
    want = {}
    for name, rows, slab in slab_maps(B, C):
        want[name] = sums(prd.double(), tar.double(), w.double(),
                          None if slab is None else clim[rows].double(), slab)
    return prd, tar, clim, w, want
