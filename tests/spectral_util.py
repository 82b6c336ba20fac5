"""Torch restatement of the reference's spectral losses (MSFNO/Models/losses.py:158-232:
spectral_l2loss_sphere, spectral_loss_sphere, h1loss_sphere), written from their formulas
over oracle.sht_ref.RealSHT, in the dtype of the inputs (the tests use fp64), plus the
loaders of tests/golden/spectral_loss/*.npz.

With c = sht(prd - tar), (B, C, lmax, mmax), and per degree
    P[b, c, l] = |c[l, 0]|^2 + 2 sum_{m >= 1} |c[l, m]|^2
  l2:        v[b] = sum_{c, l} P
  spectral:  v[b] = sum_{c, l} l (l + 1) P          (l (l + 1) formed in fp32)
  both:      v = v / (the same of tar) if relative;  v = sqrt(v) unless squared;  mean_b v
  h1:        mean_b (spectral + l2), or mean_b (sqrt(spectral) + sqrt(l2)) unless squared
The sum over the last two dimensions of P takes the channels with it, as the reference's
``torch.sum(norm2, dim=(-1, -2))`` does."""
import glob
import os

import numpy as np
import torch

from oracle import sht_ref

SPECTRAL_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                               "spectral_loss")
# (B, C, nlat, nlon, lmax, mmax, grid)
SHAPES = [
    (2, 3, 5, 12, 5, 7, "equiangular"),
    (2, 3, 33, 64, 32, 33, "equiangular"),
    (2, 3, 24, 48, 24, 25, "legendre-gauss"),
    (1, 2, 20, 45, 20, 21, "legendre-gauss"),
    (1, 2, 13, 26, 7, 9, "equiangular"),
]
VARIANTS = ([(fn, rel, sq) for fn in ("l2", "spectral") for rel in (False, True)
             for sq in (True, False)] + [("h1", False, True), ("h1", False, False)])


def power(c):
    """(..., lmax, mmax) complex -> (..., lmax) real."""
    a = c.real ** 2 + c.imag ** 2
    return a[..., 0] + 2 * a[..., 1:].sum(dim=-1)


def degree_weights(lmax, dtype):
    ls = torch.arange(lmax).float()
    return (ls * (ls + 1)).to(dtype)


def loss(fn, sht, prd, tar, relative=False, squared=True):
    """The scalar loss `fn` ("l2", "spectral", "h1") under the transform `sht`."""
    p = power(sht(prd - tar))
    w = degree_weights(p.shape[-1], p.dtype)
    l2 = p.sum(dim=(-1, -2))
    h1 = (w * p).sum(dim=(-1, -2))
    if fn == "h1":
        assert not relative
        return (h1 + l2).mean() if squared else (torch.sqrt(h1) + torch.sqrt(l2)).mean()
    v = l2 if fn == "l2" else h1
    if relative:
        pt = power(sht(tar))
        v = v / (pt if fn == "l2" else w * pt).sum(dim=(-1, -2))
    if not squared:
        v = torch.sqrt(v)
    return v.mean()


def oracle_sht(meta):
    return sht_ref.RealSHT(meta["nlat"], meta["nlon"], lmax=meta["lmax"], mmax=meta["mmax"],
                           grid=meta["grid"]).double()


def fixture_files():
    return sorted(glob.glob(os.path.join(SPECTRAL_GOLDEN, "*.npz")))


def load_fixture(path):
    """dict: prd, tar (fp32-representable fp64 tensors), fn, relative, squared, grid, nlat,
    nlon, lmax, mmax, loss (fp64 scalar tensor), grad (fp64, the shape of prd)."""
    d = np.load(path, allow_pickle=False)
    prd, tar = torch.from_numpy(d["prd"]), torch.from_numpy(d["tar"])
    assert prd.dtype == torch.float32 and tar.dtype == torch.float32
    return dict(prd=prd.double(), tar=tar.double(), fn=str(d["fn"]),
                relative=bool(d["relative"]), squared=bool(d["squared"]), grid=str(d["grid"]),
                nlat=prd.shape[2], nlon=prd.shape[3], lmax=int(d["lmax"]), mmax=int(d["mmax"]),
                loss=torch.from_numpy(d["loss"]), grad=torch.from_numpy(d["grad"]))


def fixture_id(path):
    return os.path.basename(path)[:-4]
