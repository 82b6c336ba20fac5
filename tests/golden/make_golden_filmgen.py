"""Generate tests/golden/filmgen/filmgen_*.npz from the REFERENCE graph FiLM generator.

(A directory of their own: tests/golden/*.npz are the block fixtures, globbed as such.)

Runs only where the reference checkout exists; the .npz files (mask, adjacency, parameters,
sst, outputs) are committed, this script's imports of the reference are not needed by any
test.  Import recipe as in make_golden.py: ``MSFNO/Models/gcn/{layers,gcn}.py`` are loaded
with importlib under a synthetic package after a ``sys.modules`` stub for
``torch_geometric`` (imported at gcn.py:5-6, used only by the PyG ``GCN`` class, absent
here).  ``GCN_custom`` loads its graph from two asset files that are not in the reference's
repository; synthetic ones are written to a temporary directory under the names it opens.

What is pinned: the reference's own ``GCN_custom.forward`` at depth 0, the only depth its
code executes (``GraphConvolution.forward`` takes ``input[0]``; a second layer then fails
in ``torch.mm``), at batch 1: the mask's node order, x W then A, the bias, the LeakyReLU
slope, the mean pool and the head.  Each case runs in fp32 and again in fp64;
``err_f32 = max|y32 - y64| / max|y64|`` is the yardstick of the tests' tolerance.

Usage:  python tests/golden/make_golden_filmgen.py
"""
from __future__ import annotations

import importlib.machinery
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/MSFNO/Models"
sys.path.insert(0, os.path.dirname(HERE))

import filmgen_ref as R  # noqa: E402

H, W = 12, 24
NUM_FILM_FEATURES = 256
CASES = [  # name, embed_dim, film_layers, seed
    ("h64_l1", 64, 1, 11),
    ("h64_l2", 64, 2, 12),
    ("h100_l1", 100, 1, 13),
    ("h100_l2", 100, 2, 14),
]


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, None)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def load_reference():
    _stub("torch_geometric")
    _stub("torch_geometric.nn", GCNConv=object)
    _stub("torch_geometric.nn.pool", global_mean_pool=None)
    pkg = "refmsfno_gcn"
    _stub(pkg).__path__ = []
    mods = {}
    for name in ("layers", "gcn"):
        full = f"{pkg}.{name}"
        spec = importlib.util.spec_from_file_location(full, os.path.join(REF, "gcn", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[full] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods


def main():
    ref = load_reference()["gcn"]
    for name, hidden, film_layers, seed in CASES:
        mask = R.make_mask(H, W, seed)
        n = int(mask.sum())
        idx, vals = R.make_adjacency(n, seed)
        out = NUM_FILM_FEATURES * film_layers * 2
        params = R.make_params(0, 1, hidden, out, seed)
        sst = torch.randn(1, H, W, generator=torch.Generator().manual_seed(seed + 100))
        ys = {}
        with tempfile.TemporaryDirectory() as tmp:
            np.save(os.path.join(tmp, "nan_mask_coarsen_4_notflatten.npy"), mask)
            for dtype in (torch.float32, torch.float64):
                # duplicates summed in fp32, as the module's loader does: A is fp32 data
                adj = R.coo_tensor(idx, vals, n).coalesce().to(dtype)
                torch.save(adj, os.path.join(tmp, "adj_coarsen_4_sparse.pt"))
                model = ref.GCN_custom(1, "cpu", 0, embed_dim=hidden, out_features=out, assets=tmp)
                model.load_state_dict(params)
                model = model.to(dtype)
                model.adj = model.adj.to(dtype)
                with torch.no_grad():
                    ys[dtype] = model(sst.to(dtype)).numpy()
        y32, y64 = ys[torch.float32], ys[torch.float64]
        assert y32.shape == (out,)
        err = float(np.abs(y32.astype(np.float64) - y64).max() / np.abs(y64).max())
        deg = np.bincount(torch.sparse_coo_tensor(torch.from_numpy(idx), torch.from_numpy(vals),
                                                  (n, n)).coalesce().indices()[0].numpy(),
                          minlength=n)
        assert deg.max() >= 100 and deg[1] == 1 and deg[2] == 0, deg[:3]
        path = os.path.join(HERE, "filmgen", f"filmgen_{name}.npz")
        np.savez(path, mask=mask, coo_idx=idx.astype(np.int32), coo_val=vals,
                 hidden=hidden, film_layers=film_layers, sst=sst.numpy(), y32=y32, y64=y64,
                 err_f32=err, **{k.replace(".", "__"): v.numpy() for k, v in params.items()})
        print(f"{path}: N={n} nnz={len(vals)} out={out} err_f32={err:.3e} "
              f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
