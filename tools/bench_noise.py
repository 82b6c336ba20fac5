#!/usr/bin/env python3
"""Time the native random-field fill (msfno_noise_spectral) and a whole sample (fill +
InverseRealSHT) on one GPU against the same quantity in eager torch ops.

Workload: F fields at 721 x 1440 with lmax = mmax = 360 (129,600 complex coefficients, 1 MB
per field), F = 8 x 73 and 32 x 73 by default (an 8- and a 32-member ensemble of the 73
channels), one Matern spectrum per channel.
  native  one msfno_noise_spectral launch into a preallocated buffer; + the inverse
          transform, one call per group of 73 fields (the batch the network's own transforms
          run at)
  eager   what a user of the library without the kernel runs: torch.randn complex64, the
          m = 0 column made real with unit variance, torch.tril, the per-degree scale; + the
          same InverseRealSHT
The two are timed in interleaved pairs (native, eager, native, eager, ...) with device
events after a warm-up, so a drift of the machine hits both alike.  Prints one JSON line per
F: the median milliseconds of each, the median of the per-pair ratios eager / native and
its spread (min, max over the pairs), the bytes the fill writes and their time at the
6.3 TB/s a float4 copy reaches.  There is no CPU fallback: without a GPU it fails.

Usage:  python tools/bench_noise.py [--fields 584 2336] [--pairs 7] [--out FILE.json]
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

COPY_RATE = 6.3e12
DEV = "cuda"


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def pairs(native, eager, n, warm=2):
    """n interleaved (native, eager) timings -> medians, per-pair ratio median and spread."""
    for _ in range(warm):
        native()
        eager()
    torch.cuda.synchronize()
    tn, te = [], []
    for _ in range(n):
        tn.append(once(native))
        te.append(once(eager))
    ratio = [e / v for v, e in zip(tn, te)]
    return {"native_ms": statistics.median(tn), "native_min_max_ms": (min(tn), max(tn)),
            "eager_ms": statistics.median(te), "eager_min_max_ms": (min(te), max(te)),
            "ratio": statistics.median(ratio), "ratio_min_max": (min(ratio), max(ratio))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", type=int, nargs="+", default=[8 * 73, 32 * 73])
    ap.add_argument("--channels", type=int, default=73)
    ap.add_argument("--grid", type=int, nargs=2, default=[721, 1440])
    ap.add_argument("--lmax", type=int, default=360)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from msfno_amd import _native as N
    from msfno_amd.harmonics import GaussianRandomFieldS2, matern_sqrt_eig, unit_variance
    lib = N.lib()
    H, W = args.grid
    L, K = args.lmax, args.channels
    se = torch.stack([unit_variance(matern_sqrt_eig(L, alpha=2.0 + 0.01 * k)) for k in range(K)])
    grf = GaussianRandomFieldS2(H, W, lmax=L, sqrt_eig=se, seed=1).to(DEV)
    tab = grf.table()
    st = N.stream_of(tab.device)
    out = {}
    for F in args.fields:
        if F % K:
            raise SystemExit(f"--fields must be multiples of --channels = {K}, got {F}")
        coeffs = torch.empty(F // K, K, L, L, dtype=torch.complex64, device=DEV)
        draw = [0]

        def native_fill():
            draw[0] += 1
            N.check(lib.msfno_noise_spectral(coeffs.data_ptr(), None, tab.data_ptr(), K, F, 0, L,
                                             L, 0.0, 1.0, 1, draw[0], None, st),
                    "msfno_noise_spectral")
            return coeffs

        def eager_fill():
            xi = torch.randn(F // K, K, L, L, dtype=torch.complex64, device=DEV)
            xi[..., 0] = xi[..., 0].real * 2.0 ** 0.5
            return torch.tril(xi) * tab.unsqueeze(-1)

        def transform(c):
            for member in c:  # K fields per call: the batch the network's transforms run at
                grf.isht(member)

        with torch.no_grad():
            r = {"fill": pairs(native_fill, eager_fill, args.pairs),
                 "sample": pairs(lambda: transform(native_fill()),
                                 lambda: transform(eager_fill()), args.pairs)}
            # the two streams differ; their statistics must not: the mean of |c|^2 / S_l
            # over the degrees l >= 1 (whitened, so that every coefficient counts alike)
            def white_power(c):
                return (c[..., 1:, :].abs().pow(2) / tab[:, 1:, None] ** 2).mean().item()
            r = dict(r, white_power_native_over_eager=white_power(native_fill())
                     / white_power(eager_fill()))
        r["fill_bytes"] = F * L * L * 8
        r["fill_ms_at_6.3TBps"] = r["fill_bytes"] / COPY_RATE * 1e3
        r["fill_fraction_of_copy_rate"] = r["fill_ms_at_6.3TBps"] / r["fill"]["native_ms"]
        out[f"fields={F}"] = r
        print(f"fields={F}", json.dumps(r), flush=True)
        del coeffs
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
