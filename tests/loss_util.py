"""Torch restatement of the reference's sphere-weighted losses (MSFNO/Models/losses.py:
CosineMSELoss, L2Sphere, L2Sphere_noSine), written from their formulas, in whatever dtype
the inputs have (the tests use fp64), plus the loaders of tests/golden/loss/*.npz.

Per (b, c):  num = sum_h w[h] sum_x (prd - tar)^2,  den = sum_h w[h] sum_x tar^2;
  L2Sphere*:  v = num / den if relative else num;  v = sqrt(v) unless squared;
              "mean" and "sum" both return sum_bc v
  CosineMSE:  "mean" = sum_bc num / (B C H W),  "sum" = sum_bc num / W
The Gauss-Legendre weights go through oracle.sht_ref.legendre_gauss_weights."""
import glob
import os

import numpy as np
import torch

from oracle import sht_ref

LOSS_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss")
KIND_OF = {"L2Sphere": "l2sphere", "L2Sphere_noSine": "l2sphere_nosine",
           "CosineMSELoss": "cosine"}


def weights(kind, H, eps=1e-4):
    """float64 torch vector of the latitude weights of `kind`."""
    lat = torch.linspace(-torch.pi / 2, torch.pi / 2, H, dtype=torch.float64)
    if kind == "uniform":
        return torch.ones(H, dtype=torch.float64)
    if kind == "cosine":
        w = torch.clamp(torch.cos(lat), min=0.0) + eps
        return w / w.sum()
    w_quad = torch.as_tensor(sht_ref.legendre_gauss_weights(H, -1, 1)[1], dtype=torch.float64)
    if kind == "l2sphere_nosine":
        return w_quad
    if kind == "l2sphere":
        return (w_quad * torch.cos(lat)).abs()
    raise ValueError(kind)


def sums(prd, tar, w):
    """(B, C, 2) {num, den} in the dtype of prd."""
    w = w.to(prd.dtype)[None, None, :, None]
    num = (w * (prd - tar) ** 2).sum(dim=(-1, -2))
    den = (w * tar ** 2).sum(dim=(-1, -2))
    return torch.stack((num, den), dim=-1)


def loss(cls, prd, tar, reduction, relative=True, squared=False, eps=1e-4):
    """The scalar loss of class name `cls` ("L2Sphere", "L2Sphere_noSine",
    "CosineMSELoss") for reduction "mean" or "sum"."""
    assert reduction in ("mean", "sum")
    B, C, H, W = prd.shape
    s = sums(prd, tar, weights(KIND_OF[cls], H, eps))
    if cls == "CosineMSELoss":
        total = s[..., 0].sum()
        return total / (B * C * H * W) if reduction == "mean" else total / W
    v = s[..., 0] / s[..., 1] if relative else s[..., 0]
    if not squared:
        v = torch.sqrt(v)
    return v.sum()


def loss_and_grad(cls, prd, tar, reduction, relative=True, squared=False, eps=1e-4):
    p = prd.detach().clone().requires_grad_()
    v = loss(cls, p, tar, reduction, relative, squared, eps)
    v.backward()
    return v.detach(), p.grad


def fixture_files():
    return sorted(glob.glob(os.path.join(LOSS_GOLDEN, "*.npz")))


def load_fixture(path):
    """(prd, tar) fp32-representable fp64 tensors and the list of cases: dicts with cls,
    relative, squared, reduction, eps, w (H), loss (scalar), grad (B, C, H, W), fp64."""
    d = np.load(path, allow_pickle=False)
    prd, tar = torch.from_numpy(d["prd"]).double(), torch.from_numpy(d["tar"]).double()
    cases = []
    for i in range(int(d["n_cases"])):
        cases.append(dict(cls=str(d[f"c{i}_cls"]), relative=bool(d[f"c{i}_relative"]),
                          squared=bool(d[f"c{i}_squared"]), reduction=str(d[f"c{i}_reduction"]),
                          eps=float(d[f"c{i}_eps"]), w=torch.from_numpy(d[f"c{i}_w"]),
                          loss=torch.from_numpy(d[f"c{i}_loss"]),
                          grad=torch.from_numpy(d[f"c{i}_grad"])))
    return prd, tar, cases


def case_id(c):
    if c["cls"] == "CosineMSELoss":
        return f"{c['cls']}-{c['reduction']}"
    return (f"{c['cls']}-{'rel' if c['relative'] else 'abs'}-"
            f"{'sq' if c['squared'] else 'sqrt'}-{c['reduction']}")
