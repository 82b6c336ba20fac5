#!/usr/bin/env python
"""Time the native graph FiLM generator against the same math in eager torch ops.

Shape (the reference's 1-degree SST workload, synthetic): a 180 x 360 mask with about two
thirds ocean, ``grid_adjacency`` over it, hidden 512, depth 6, film_layers 1, B = 1.  The
eager side is ``torch.sparse.mm`` + ``matmul`` + autograd on the same device, with the same
parameters.  Both run in one process as interleaved pairs (native, eager, native, ...), timed
with device events; per variant the median and the minimum, per pair the ratio
eager / native, and the spread of those ratios (min, max) are reported.  Prints one JSON line.

    python tools/bench_filmgen.py [--pairs 20] [--warmup 3] [--hidden 512] [--depth 6]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "modulated-spherical-fourier-neural-operator_amd"))


def ocean_mask(H, W, seed=0):
    """Smooth random continents: about two thirds of the cells are ocean."""
    rng = np.random.default_rng(seed)
    f = np.zeros((H, W))
    yy, xx = np.mgrid[0:H, 0:W]
    for _ in range(24):
        cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(8, 40)
        dx = np.minimum(np.abs(xx - cx), W - np.abs(xx - cx))
        f += np.exp(-((yy - cy) ** 2 + dx ** 2) / (2 * r * r))
    return f < np.quantile(f, 2.0 / 3.0)


def eager_forward(p, A, x0, depth):
    leaky = torch.nn.functional.leaky_relu
    h = leaky(torch.sparse.mm(A, x0 @ p["conv1.weight"]) + p["conv1.bias"], 0.01)
    for i in range(depth):
        h = h + leaky(torch.sparse.mm(A, h @ p[f"conv_layers.{i}.weight"])
                      + p[f"conv_layers.{i}.bias"], 0.01)
    return h.mean(0, keepdim=True) @ p["head_film.weight"].T + p["head_film.bias"]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--nlat", type=int, default=180)
    ap.add_argument("--nlon", type=int, default=360)
    args = ap.parse_args()
    from msfno_amd.filmgen import Film_wrapper, grid_adjacency
    import types
    dev = "cuda"
    mask = ocean_mask(args.nlat, args.nlon)
    adj = grid_adjacency(mask)
    cfg = types.SimpleNamespace(batch_size=1, model_depth=args.depth, embed_dim=args.hidden,
                                film_layers=1, film_gen_type=None, assets=None)
    torch.manual_seed(0)
    fw = Film_wrapper(dev, cfg, adj=adj, nan_mask=mask)
    gen = fw.film_gen
    with torch.no_grad():  # a head that is not all ones, so that its columns differ
        gen.head_film.weight.normal_(0, args.hidden ** -0.5)
    sst = torch.randn(1, args.nlat, args.nlon, device=dev)
    dy = torch.randn(1, gen.out_features, device=dev)
    p = {k: v.detach().clone().requires_grad_() for k, v in gen.state_dict().items()}
    A = adj.to(dev).to_sparse_csr()
    cells = torch.from_numpy(np.flatnonzero(mask.ravel())).to(dev)
    x0 = sst.reshape(-1)[cells][:, None]

    def native_fwd():
        with torch.no_grad():
            gen(sst)

    def eager_fwd():
        with torch.no_grad():
            eager_forward(p, A, x0, args.depth)

    def native_fb():
        gen.zero_grad(set_to_none=True)
        (gen(sst) * dy).sum().backward()

    def eager_fb():
        for v in p.values():
            v.grad = None
        (eager_forward(p, A, x0, args.depth) * dy).sum().backward()

    with torch.no_grad():
        ref = eager_forward(p, A, x0, args.depth)
        err = ((gen(sst) - ref).abs().max() / ref.abs().max()).item()
    variants = {"native_fwd": native_fwd, "eager_fwd": eager_fwd, "native_fwd_bwd": native_fb,
                "eager_fwd_bwd": eager_fb}
    for _ in range(args.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.pairs):
        for k, fn in variants.items():
            times[k].append(timed(fn))
    out = {"nodes": int(mask.sum()), "nnz": int(adj._nnz()), "hidden": args.hidden,
           "depth": args.depth, "pairs": args.pairs, "fwd_rel_diff_vs_eager": err}
    for k, v in times.items():
        out[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    for kind in ("fwd", "fwd_bwd"):
        r = [e / n for e, n in zip(times["eager_" + kind], times["native_" + kind])]
        out["eager_over_native_" + kind] = {"median": statistics.median(r), "min": min(r),
                                            "max": max(r)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
