"""Generate tests/golden/loss/*.npz from the REFERENCE loss classes
(MSFNO/Models/losses.py: CosineMSELoss, L2Sphere, L2Sphere_noSine), run in fp64.

Like make_golden.py this runs only where the reference checkout exists; its outputs are
committed.  losses.py is imported under make_golden's synthetic package; of its imports
only ``torch_harmonics.quadrature.legendre_gauss_weights`` is absent here, and
make_golden.load_reference() stubs it with the oracle's restatement (oracle/sht_ref.py).

One file per (shape, class, relative, squared) holds the fp32-representable inputs and,
for each usable reduction ("mean", "sum"), the class's own latitude weights (read back
from a reduction="none" call on a field of ones), the fp64 loss and the fp64 gradient
with respect to prd.  Channel scales spread over 1e-3 .. 1e4, so a loss that weighs a
small channel wrongly cannot hide behind a large one.

Usage:  python tests/golden/make_golden_losses.py
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402

SHAPES = [(2, 3, 5, 12), (2, 5, 33, 64)]
OUT = os.path.join(HERE, "loss")


def load_reference_losses():
    make_golden.load_reference()
    full = "refmsfno.losses"
    spec = importlib.util.spec_from_file_location(full, os.path.join(make_golden.REF, "losses.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[full] = mod
    spec.loader.exec_module(mod)
    return mod


def make_inputs(shape, seed):
    B, C, H, W = shape
    rng = np.random.default_rng(seed)
    scale = np.logspace(-3, 4, C).astype(np.float32)[None, :, None, None]
    tar = (rng.standard_normal(shape, dtype=np.float32) + np.float32(0.5)) * scale
    prd = tar + np.float32(0.3) * scale * rng.standard_normal(shape, dtype=np.float32)
    return prd.astype(np.float32), tar.astype(np.float32)


def ref_weights(make, H):
    """The weights the class applies: its reduction="none" output on (prd, tar) = (1, 0)."""
    field = make("none")(torch.ones(1, 1, H, 1, dtype=torch.float64),
                         torch.zeros(1, 1, H, 1, dtype=torch.float64))
    return field[0, 0, :, 0].numpy().copy()


def main():
    ref = load_reference_losses()
    os.makedirs(OUT, exist_ok=True)
    variants = [("CosineMSELoss", None, None)]
    for cls in ("L2Sphere", "L2Sphere_noSine"):
        for relative in (True, False):
            for squared in (True, False):
                variants.append((cls, relative, squared))
    for si, shape in enumerate(SHAPES):
        prd, tar = make_inputs(shape, 4242 + si)
        for cls, relative, squared in variants:
            if cls == "CosineMSELoss":
                def make(reduction):
                    return ref.CosineMSELoss(reduction=reduction)
                tag, eps = "cosine", make("mean").eps
            else:
                def make(reduction, _c=getattr(ref, cls), _r=relative, _s=squared):
                    # weights: the un-normalised field, whatever the variant
                    return _c(relative=_r and reduction != "none", squared=_s,
                              reduction=reduction)
                tag = (f"{cls.lower()}_{'rel' if relative else 'abs'}_"
                       f"{'sq' if squared else 'sqrt'}")
                eps = 0.0
            out = {"prd": prd, "tar": tar}
            w = ref_weights(make, shape[2])
            for i, reduction in enumerate(("mean", "sum")):
                p = torch.from_numpy(prd).double().requires_grad_()
                v = make(reduction)(p, torch.from_numpy(tar).double())
                v.backward()
                out.update({f"c{i}_cls": np.array(cls), f"c{i}_relative": np.array(bool(relative)),
                            f"c{i}_squared": np.array(bool(squared)),
                            f"c{i}_reduction": np.array(reduction), f"c{i}_eps": np.array(eps),
                            f"c{i}_w": w, f"c{i}_loss": v.detach().numpy(),
                            f"c{i}_grad": p.grad.numpy()})
            out["n_cases"] = np.array(2)
            path = os.path.join(OUT, f"{tag}_{'x'.join(map(str, shape))}.npz")
            np.savez_compressed(path, **out)
            print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
