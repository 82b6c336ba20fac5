#!/usr/bin/env python3
"""Time the regional verification sums on one GPU against the unchanged global kernel and
against the same regional sums in eager torch.

Workload: (1, 73, 721, 1440) fp32 fields (303 MB each) under the cosine weights, without and
with a climatology slab for every (b, c), timed with device events after warm-up, the variants
taken in turn within every repetition:
  (g)    msfno_verify_sums, the global kernel: the yardstick.  R latitude bands cost R calls
         of it today; boxes and masks it cannot do at all
  (r1)   msfno_verify_region_sums, one region of all ones
  (r8)   8 latitude bands (one pass)
  (r13)  regions.scorecard: 13 regions, bands and boxes (two passes: 8 + 5 -> 8)
  (r13p) the same 13 with a pix_bits plane (a random land mask in every box)
  (e*)   the regional sums of r1, r8, r13, r13p in eager torch: the weighted terms once, then
         one masked multiply and sum per region and term
Prints one JSON line: per variant the median, min and max milliseconds, the ratio to (g) of
the same repetition set, eager / native, and the achieved GB/s against the bytes the passes
stream (fields once per pass of 8 regions, the plane once per slab and pass) beside the
6.3 TB/s a float4 copy reaches.  There is no CPU fallback: without a GPU it fails.

Usage:  python tools/bench_verify_regions.py [--shape 1 73 721 1440] [--reps 30] [--warmup 3]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

COPY_RATE_GBPS = 6300


def time_interleaved(fns, reps, warmup):
    """{name: (median, min, max) ms}; every repetition runs each variant once, in order."""
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
        out[k] = (statistics.median(t), min(t), max(t))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, default=[1, 73, 721, 1440])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_verify_regions.py needs a GPU (no CPU fallback)")
    from msfno_amd import losses as L
    from msfno_amd import regions as RG
    from msfno_amd import verification as V

    B, C, H, W = args.shape
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    tar = torch.randn(B, C, H, W, device=dev, generator=g)
    prd = tar + 0.3 * torch.randn(B, C, H, W, device=dev, generator=g)
    clim = 0.7 * torch.randn(B, C, H, W, device=dev, generator=g)
    w = L.device_weights("cosine", H, dev)
    w4 = w[None, None, :, None]

    edges = np.linspace(-90.0, 90.0, 9)
    card = RG.scorecard((H, W))
    land = np.random.default_rng(0).random((H, W)) < 0.3
    masked = RG.Regions(card.names, card.row_bits, card.col_bits,
                        np.where(land, np.uint32(0), np.uint32(0xFFFFFFFF)))
    sets = {
        "r1": RG.Regions.boxes((H, W), {"global": (None, None, None, None)}),
        "r8": RG.Regions.bands((H, W), {f"band{k}": [(edges[k], edges[k + 1])]
                                        for k in range(8)}),
        "r13": card,
        "r13p": masked,
    }
    glob = V.Verifier(w, H, W, 2, B, C, device=dev)
    vers = {k: V.RegionalVerifier(w, rg, 2, B, C, device=dev) for k, rg in sets.items()}
    dense = {k: torch.from_numpy(np.stack([rg.mask(n) for n in rg.names])).to(dev).float()
             for k, rg in sets.items()}

    def eager(key, with_clim):
        d = prd - tar
        terms = [w4.expand_as(d), w4 * d * d, w4 * d, w4 * d.abs()]
        if with_clim:
            pa, ta = prd - clim, tar - clim
            terms += [w4 * pa * pa, w4 * ta * ta, w4 * pa * ta]
        out = torch.zeros(B, C, len(sets[key]), 7, device=dev)
        for r, m in enumerate(dense[key]):
            for k, x in enumerate(terms):
                out[:, :, r, k] = (x * m).sum(dim=(-1, -2))
        return out

    result = {
        "tool": "bench_verify_regions", "shape": [B, C, H, W], "weights": "cosine",
        "reps": args.reps, "warmup": args.warmup,
        "timing": "device events, per call, variants interleaved",
        "copy_rate_GBps_reference": COPY_RATE_GBPS,
        "regions": {k: len(rg) for k, rg in sets.items()},
    }
    nbytes = 4 * B * C * H * W
    for with_clim in (False, True):
        c = clim if with_clim else None
        slot = int(with_clim)
        fns = {"g": lambda: glob.update(slot, prd, tar, c)}
        for k in sets:
            fns[k] = lambda k=k: vers[k].update(slot, prd, tar, c)
        for k in sets:
            fns["e" + k[1:]] = lambda k=k: eager(k, with_clim)
        # native and eager must agree before their times are compared (fp32 eager sums of
        # non-negative terms: 1e-4 relative; the global column: bitwise the global kernel)
        for fn in list(fns.values())[:1 + len(sets)]:
            fn()
        torch.cuda.synchronize()
        diff = 0.0
        for k in sets:
            e, n = eager(k, with_clim), vers[k].sums[slot]
            idx = [0, 1, 3] + ([4, 5] if with_clim else [])
            diff = max(diff, float(((n - e)[..., idx].abs()
                                    / e[..., idx].abs().clamp(min=1e-30)).max()))
        assert diff < 1e-4, diff
        for k in ("r1", "r13"):
            assert torch.equal(vers[k].sums[slot][:, :, 0, 1:], glob.sums[slot]), k

        t = time_interleaved(fns, args.reps, args.warmup)
        fields = (3 if with_clim else 2) * nbytes
        res = {"global_ms": [round(v, 4) for v in t["g"]],
               "global_GBps": round(fields / t["g"][0] / 1e6, 1),
               "max_diff_native_vs_eager_relative": float(f"{diff:.3e}")}
        for k, rg in sets.items():
            passes = (len(rg) + 7) // 8
            streamed = passes * (fields + (nbytes if rg.pix_bits is not None else 0))
            res[k] = {
                "ms_median_min_max": [round(v, 4) for v in t[k]],
                "ratio_over_global": round(t[k][0] / t["g"][0], 3),
                "ratio_over_R_global_calls": round(t[k][0] / (len(rg) * t["g"][0]), 3),
                "eager_ms_median_min_max": [round(v, 3) for v in t["e" + k[1:]]],
                "ratio_eager_over_native": round(t["e" + k[1:]][0] / t[k][0], 1),
                "passes": passes, "streamed_MB": round(streamed / 1e6, 1),
                "streamed_GBps": round(streamed / t[k][0] / 1e6, 1),
                "fraction_of_copy_rate": round(streamed / t[k][0] / 1e6 / COPY_RATE_GBPS, 3),
            }
        result["clim" if with_clim else "no_clim"] = res
    print(json.dumps(result))


if __name__ == "__main__":
    main()
