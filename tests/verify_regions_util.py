"""Torch restatement of the regional verification sums (msfno_amd/verification.py
region_sums, csrc/verify_regions.hip), written from the definition on dense boolean
membership (never from the bit tables), in the dtype of its inputs (the tests use fp64), plus
the shared region problems of the tests.

Per (b, c, region r), over the pixels that are in r and valid (v = 1; with skip_nan a pixel
is invalid where tar is NaN or, for a slab with a climatology, clim is):
  n = sum w   se = sum w (p-t)^2   err = sum w (p-t)   ae = sum w |p-t|
  pa2 = sum w (p-c)^2   ta2 = sum w (t-c)^2   cross = sum w (p-c)(t-c)
  mse = se/n, rmse = sqrt(mse), bias = err/n, mae = ae/n, skill = 1 - se/ta2,
  acc = cross / sqrt(pa2 ta2); all NaN where n = 0, the last two NaN without a climatology."""
import functools

import numpy as np
import torch

import verify_util as VU

NAMES = VU.NAMES
NONNEG = [0, 1, 3, 4, 5]   # n, se, ae, pa2, ta2
R_VALUES = [1, 2, 8, 9, 13, 32]


def sums(prd, tar, w, member, clim=None, slab=None, skip_nan=False):
    """((B, C, R, 7) sums, (B, C, R, 7) magnitude sums) under the (R, H, W) boolean
    ``member``.  clim (K, H, W) and slab a sequence of B * C slab indices (-1 = none).
    prd must be finite at the valid pixels."""
    B, C, H, W = prd.shape
    dt = prd.dtype
    member = torch.as_tensor(member, dtype=torch.bool)
    R = member.shape[0]
    valid = torch.ones(B, C, H, W, dtype=torch.bool)
    if skip_nan:
        valid &= ~torch.isnan(tar)
    zero = torch.zeros(B, C, H, W, dtype=dt)
    d = prd - tar
    if clim is None:
        pa = ta = zero
    else:
        idx = torch.as_tensor(slab, dtype=torch.int64).reshape(B, C)
        has = (idx >= 0)[:, :, None, None].expand(B, C, H, W)
        c = clim.to(dt)[idx.clamp(min=0)]
        if skip_nan:
            valid &= ~(has & torch.isnan(c))
        pa, ta = torch.where(has, prd - c, zero), torch.where(has, tar - c, zero)
    ww = w.to(dt)[None, None, :, None].expand(B, C, H, W)
    terms = [torch.ones_like(d), d * d, d, d.abs(), pa * pa, ta * ta, pa * ta]
    m = member.reshape(R, H * W).to(dt).T                       # (HW, R)

    def red(x):
        x = torch.where(valid, ww * x, zero)                    # invalid pixels: selected out
        return x.reshape(B, C, H * W) @ m                       # (B, C, R)

    return (torch.stack([red(x) for x in terms], dim=-1),
            torch.stack([red(x.abs()) for x in terms], dim=-1))


def scores(s, has_clim, batch_mean=False):
    """dict of the six scores from (B, C, R, 7) sums; has_clim (B, C) bool."""
    if batch_mean:
        s = s.sum(dim=0)
        has_clim = has_clim.all(dim=0)
    n, se, err, ae, pa2, ta2, cross = s.unbind(-1)
    nan = torch.full_like(se, float("nan"))
    some = n != 0
    has = has_clim[..., None] & some
    mse = torch.where(some, se / n, nan)
    return dict(mse=mse, rmse=mse.sqrt(), bias=torch.where(some, err / n, nan),
                mae=torch.where(some, ae / n, nan),
                skill=torch.where(has, 1 - se / ta2, nan),
                acc=torch.where(has, cross / (pa2 * ta2).sqrt(), nan))


def bit_tables(rows, cols, pix):
    """uint32 (row_bits, col_bits, pix_bits or None) of the boolean stacks rows (R, H), cols
    (R, W) and pix, a list of R entries: an (H, W) boolean plane or None (all ones)."""
    R, H = rows.shape
    W = cols.shape[1]
    rb, cb = np.zeros(H, dtype=np.uint32), np.zeros(W, dtype=np.uint32)
    pb = None if all(p is None for p in pix) else np.zeros((H, W), dtype=np.uint32)
    for r in range(R):
        bit = np.uint32(1 << r)
        rb[rows[r]] |= bit
        cb[cols[r]] |= bit
        if pb is not None:
            pb[np.ones((H, W), dtype=bool) if pix[r] is None else pix[r]] |= bit
    return rb, cb, pb


@functools.lru_cache(maxsize=None)
def region_problem(H, W, R):
    """(Regions, member): R regions of an (H, W) grid and their dense (R, H, W) boolean
    membership, both formed from the same row sets, column sets and planes.  Region 0 is all
    ones and region 1 empty; the others cycle through a longitude box that wraps through
    column 0, a union of two row sets, a random plane inside a box, and a single pixel; the
    last region sits on the highest bit in use.  Shared, never modified."""
    from msfno_amd.regions import Regions
    rng = np.random.default_rng(31 * H + 7 * W + R)
    rows = np.zeros((R, H), dtype=bool)
    cols = np.zeros((R, W), dtype=bool)
    pix = [None] * R
    h, x = np.arange(H), np.arange(W)
    for r in range(R):
        if r == 0:
            rows[r], cols[r] = True, True
        elif r == 1:
            pass
        elif r % 4 == 2:      # a box that wraps through column 0
            x0 = (3 * W) // 4 + r % 3
            rows[r] = (h >= H // 5) & (h <= H - 1 - H // 7)
            cols[r] = (x - x0) % W <= W // 2
        elif r % 4 == 3:      # two caps
            rows[r] = (h <= H // 4 - r % 2) | (h >= H - 1 - H // 3)
            cols[r] = True
        elif r % 4 == 0:      # a random plane inside rows and columns of its own
            rows[r] = rng.random(H) < 0.8
            cols[r] = rng.random(W) < 0.8
            pix[r] = rng.random((H, W)) < 0.5
        else:                 # a single pixel
            rows[r, int(rng.integers(H))] = True
            cols[r, int(rng.integers(W))] = True
    member = rows[:, :, None] & cols[:, None, :]
    for r in range(R):
        if pix[r] is not None:
            member[r] &= pix[r]
    names = tuple(f"r{r}" for r in range(R))
    return Regions(names, *bit_tables(rows, cols, pix)), torch.from_numpy(member)


@functools.lru_cache(maxsize=None)
def want(shape, R, name):
    """The fp64 (sums, magnitude sums) of VU.problem(shape) under region_problem(H, W, R) and
    the climatology map ``name`` of VU.slab_maps; computed once, shared, never modified."""
    B, C, H, W = shape
    prd, tar, clim, w, _ = VU.problem(shape)
    _, member = region_problem(H, W, R)
    rows, slab = next((r, s) for n, r, s in VU.slab_maps(B, C) if n == name)
    return sums(prd.double(), tar.double(), w.double(), member,
                None if slab is None else clim[rows].double(), slab)
