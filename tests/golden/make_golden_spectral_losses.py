"""Generate tests/golden/spectral_loss/*.npz from the REFERENCE spectral losses
(MSFNO/Models/losses.py:158-232: spectral_l2loss_sphere, spectral_loss_sphere,
h1loss_sphere), run in fp64.

Like make_golden_losses.py this runs only where the reference checkout exists; its outputs
are committed.  losses.py is imported through make_golden_losses.load_reference_losses();
the ``solver`` the functions take is ``SimpleNamespace(sht=oracle.sht_ref.RealSHT(...)
.double())``, the restatement of the torch-harmonics transform the reference would use.

One file per (shape, function, relative, squared) holds the fp32-representable inputs
(make_golden_losses.make_inputs: channel scales spread over 1e-3 .. 1e4), the fp64 loss
and the fp64 gradient with respect to prd.  h1loss_sphere has no relative form.

Usage:  python tests/golden/make_golden_spectral_losses.py [--check]
--check writes nothing: it compares what it would write with the committed files, array
by array, bit for bit (the zip container itself carries time stamps).
"""
from __future__ import annotations

import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_losses  # noqa: E402  (puts the repository root on sys.path)

from oracle import sht_ref  # noqa: E402

# (B, C, nlat, nlon, lmax, mmax, grid)
SHAPES = [
    (2, 3, 5, 12, 5, 7, "equiangular"),
    (2, 3, 33, 64, 32, 33, "equiangular"),
    (2, 3, 24, 48, 24, 25, "legendre-gauss"),
    (1, 2, 20, 45, 20, 21, "legendre-gauss"),   # odd nlon
    (1, 2, 13, 26, 7, 9, "equiangular"),        # mmax > lmax + 1
]
FUNCTIONS = {"l2": "spectral_l2loss_sphere", "spectral": "spectral_loss_sphere",
             "h1": "h1loss_sphere"}
OUT = os.path.join(HERE, "spectral_loss")


def variants():
    out = []
    for fn in ("l2", "spectral"):
        for relative in (False, True):
            for squared in (True, False):
                out.append((fn, relative, squared))
    for squared in (True, False):
        out.append(("h1", False, squared))
    return out


def file_name(shape, fn, relative, squared):
    B, C, nlat, nlon, lmax, mmax, grid = shape
    g = "eq" if grid == "equiangular" else "lg"
    return (f"{fn}_{'rel' if relative else 'abs'}_{'sq' if squared else 'sqrt'}_"
            f"{B}x{C}x{nlat}x{nlon}_l{lmax}m{mmax}{g}.npz")


def main():
    check = "--check" in sys.argv[1:]
    ref = make_golden_losses.load_reference_losses()
    os.makedirs(OUT, exist_ok=True)
    for si, shape in enumerate(SHAPES):
        B, C, nlat, nlon, lmax, mmax, grid = shape
        prd, tar = make_golden_losses.make_inputs((B, C, nlat, nlon), 5151 + si)
        solver = SimpleNamespace(sht=sht_ref.RealSHT(nlat, nlon, lmax=lmax, mmax=mmax,
                                                     grid=grid).double())
        for fn, relative, squared in variants():
            p = torch.from_numpy(prd).double().requires_grad_()
            v = getattr(ref, FUNCTIONS[fn])(solver, p, torch.from_numpy(tar).double(),
                                            relative=relative, squared=squared)
            v.backward()
            assert torch.isfinite(v) and torch.isfinite(p.grad).all()
            out = {"prd": prd, "tar": tar, "fn": np.array(fn), "relative": np.array(relative),
                   "squared": np.array(squared), "grid": np.array(grid),
                   "lmax": np.array(lmax), "mmax": np.array(mmax),
                   "loss": v.detach().numpy(), "grad": p.grad.numpy()}
            path = os.path.join(OUT, file_name(shape, fn, relative, squared))
            if check:
                have = np.load(path, allow_pickle=False)
                assert sorted(have.files) == sorted(out), path
                for k, a in out.items():
                    b = have[k]
                    assert a.dtype == b.dtype and a.shape == b.shape and \
                        np.asarray(a).tobytes() == b.tobytes(), (path, k)
                print("same", path)
            else:
                np.savez_compressed(path, **out)
                print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
