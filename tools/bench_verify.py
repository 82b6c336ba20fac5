#!/usr/bin/env python3
"""Time the native forecast verification sums on one GPU against the same six sums in
eager torch.

Workload: msfno_verify_sums on (1, 73, 721, 1440) fp32 fields (303 MB each) under the
cosine weights, timed with device events after warm-up, the variants taken in turn within
every repetition:
  (n0) native, no climatology        reads prd + tar: 606 MB algorithmic
  (n1) native, a climatology slab for every (b, c): 909 MB algorithmic
  (e0) / (e1) the same sums written as eager torch ops on the same device tensors (what a
       user of the library without this kernel runs after each rollout step)
Prints one JSON line: median / min milliseconds, achieved GB/s against the algorithmic
bytes, the ratios eager / native and native / (bytes at the 6.3 TB/s a float4 copy
reaches).  There is no CPU fallback: without a GPU it fails.

Usage:  python tools/bench_verify.py [--shape 1 73 721 1440] [--reps 30] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "modulated-spherical-fourier-neural-operator_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

COPY_RATE_GBPS = 6300


def time_interleaved(fns, reps, warmup):
    """{name: (median ms, min ms)}; every repetition runs each variant once, in order."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for _ in range(reps)] for k in fns}
    for i in range(reps):
        for k, fn in fns.items():
            a, b = ev[k][i]
            a.record()
            fn()
            b.record()
    torch.cuda.synchronize()
    out = {}
    for k in fns:
        t = [a.elapsed_time(b) for a, b in ev[k]]
        out[k] = (statistics.median(t), min(t))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, default=[1, 73, 721, 1440])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_verify.py needs a GPU (no CPU fallback)")
    from msfno_amd import losses as L
    from msfno_amd import verification as V

    B, C, H, W = args.shape
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    tar = torch.randn(B, C, H, W, device=dev, generator=g)
    prd = tar + 0.3 * torch.randn(B, C, H, W, device=dev, generator=g)
    clim = 0.7 * torch.randn(B, C, H, W, device=dev, generator=g)
    w = L.device_weights("cosine", H, dev)
    ver = V.Verifier(w, H, W, 2, B, C, device=dev)
    w4 = w[None, None, :, None]

    def eager(with_clim):
        d = prd - tar
        s = [(w4 * d * d).sum(dim=(-1, -2)), (w4 * d).sum(dim=(-1, -2)),
             (w4 * d.abs()).sum(dim=(-1, -2))]
        if with_clim:
            pa, ta = prd - clim, tar - clim
            s += [(w4 * pa * pa).sum(dim=(-1, -2)), (w4 * ta * ta).sum(dim=(-1, -2)),
                  (w4 * pa * ta).sum(dim=(-1, -2))]
        else:
            s += [torch.zeros_like(s[0])] * 3
        return torch.stack(s, dim=-1)

    fns = {"n0": lambda: ver.update(0, prd, tar), "n1": lambda: ver.update(1, prd, tar, clim),
           "e0": lambda: eager(False), "e1": lambda: eager(True)}
    # the two must agree before their times are compared (fp32 eager sums: 1e-4 of the
    # magnitude sums)
    fns["n0"]()
    fns["n1"]()
    mag = eager(True).abs()
    mag[..., 1] = (w4 * (prd - tar).abs()).sum(dim=(-1, -2))
    mag[..., 5] = (w4 * ((prd - clim) * (tar - clim)).abs()).sum(dim=(-1, -2))
    diff = float(((ver.sums[1] - eager(True)).abs() / mag).max())
    assert diff < 1e-4, diff

    t = time_interleaved(fns, args.reps, args.warmup)
    nbytes = 4 * B * C * H * W
    floor0, floor1 = 2 * nbytes / COPY_RATE_GBPS / 1e6, 3 * nbytes / COPY_RATE_GBPS / 1e6
    out = {
        "tool": "bench_verify", "shape": [B, C, H, W], "weights": "cosine",
        "reps": args.reps, "warmup": args.warmup,
        "timing": "device events, per call, variants interleaved",
        "verify_ms": round(t["n0"][0], 4), "verify_ms_min": round(t["n0"][1], 4),
        "verify_GBps": round(2 * nbytes / t["n0"][0] / 1e6, 1),
        "verify_clim_ms": round(t["n1"][0], 4), "verify_clim_ms_min": round(t["n1"][1], 4),
        "verify_clim_GBps": round(3 * nbytes / t["n1"][0] / 1e6, 1),
        "eager_ms": round(t["e0"][0], 4), "eager_clim_ms": round(t["e1"][0], 4),
        "ratio_eager_over_native": round(t["e0"][0] / t["n0"][0], 2),
        "ratio_eager_over_native_clim": round(t["e1"][0] / t["n1"][0], 2),
        "ratio_native_over_copy_rate_floor": round(t["n0"][0] / floor0, 3),
        "ratio_native_over_copy_rate_floor_clim": round(t["n1"][0] / floor1, 3),
        "algorithmic_MB": {"verify": round(2 * nbytes / 1e6, 1),
                           "verify_clim": round(3 * nbytes / 1e6, 1)},
        "copy_rate_GBps_reference": COPY_RATE_GBPS,
        "max_diff_native_vs_eager_over_magnitude": float(f"{diff:.3e}"),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
