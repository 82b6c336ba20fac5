#!/usr/bin/env python3
"""Time the native regridder (msfno_amd/regrid.py, csrc/regrid.hip) on one GPU against a device
copy of the same bytes and against the same operator in eager torch, and end to end through
``Rollout.export``.

Kernel cases on (1, 73, 721, 1440) fp32 fields, 300 + N(0, 1):
  (a) conservative to 121 x 240 (WeatherBench's 1.5 degree grid with poles)
  (b) conservative to the 120 x 240 Gauss grid
  (c) sst_input of 28 fields to 180 x 360: the 4 x 4 block mean with NaN skipped (a third of
      the points NaN in patches) and the per-field affine
Each against
  copy    ``dst.copy_(src)`` of (input + output) / 2 bytes: it moves the bytes the regridder
          has to move (the input read once, the output written once), so native / copy is the
          share of the achievable stream that the kernel reaches
  eager   the same operator as eager torch ops on the same tensors: two dense fp32 matmuls
          (Wlat @ x, then @ Wlon.T) and, for (c), nan_to_num, isnan, the two products for
          numerator and denominator, the division, the fill and the affine
Device events; the sides alternate in one process, pair by pair, after one warm round.
  (d) end to end steps/s of the 12-block network (config 3 of bench.py, HIP graph) over
      --steps steps: Rollout.export(regrid=) to 121 x 240 through the writer ring, against the
      strided window (every sixth point) through the ring and against the whole-field export.
Prints one JSON line per case: (median, min, max) milliseconds of each side over the pairs, the
(median, min, max) of the per-pair ratios to the native side, the algorithmic bytes, and the
largest difference between native and eager.  There is no CPU fallback: without a GPU it fails.

Usage:  python tools/bench_regrid.py [--pairs 7] [--reps 10] [--steps 12] [--no-net] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "modulated-spherical-fourier-neural-operator_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

DEV = "cuda"


def timed(fn, reps):
    """ms per call over reps calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def stats(ts):
    return statistics.median(ts), min(ts), max(ts)


def paired(sides, pairs, reps):
    """{name: fn} alternating; one warm round first.  (median, min, max) ms of each side and
    of the per-pair ratio of every later side to the first."""
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in sides}
    for _ in range(pairs):
        for k, fn in sides.items():
            ts[k].append(timed(fn, reps))
    first = next(iter(sides))
    out = {f"{k}_ms": stats(v) for k, v in ts.items()}
    for k in list(sides)[1:]:
        out[f"{k}_over_{first}"] = stats([b / a for a, b in zip(ts[first], ts[k])])
    return out


def copy_pair(nbytes):
    src = torch.empty(nbytes // 8, dtype=torch.float32, device=DEV).normal_()
    return src, torch.empty_like(src)


def bench_kernels(args, out):
    from msfno_amd import regrid as G
    S, H, W = args.shape
    g = torch.Generator(device=DEV).manual_seed(0)
    x = 300 + torch.randn(1, S, H, W, device=DEV, generator=g)

    def linear_case(name, R):
        Wlat, Wlon = (torch.from_numpy(m).float().to(DEV) for m in R.dense())
        WlonT = Wlon.t().contiguous()
        y = torch.empty((1, S) + R.out_shape, device=DEV)
        nbytes = (x.numel() + y.numel()) * 4
        src, cpy = copy_pair(nbytes)
        eager = lambda: torch.matmul(torch.matmul(Wlat, x), WlonT)
        res = paired({"native": lambda: R(x, out=y), "copy": lambda: cpy.copy_(src),
                      "eager": eager}, args.pairs, args.reps)
        res["bytes"] = nbytes
        res["native_GBps"] = nbytes / res["native_ms"][0] / 1e6
        res["fraction_of_copy"] = res["copy_ms"][0] / res["native_ms"][0]
        res["taps"] = [R.lat.taps, R.lon.taps]
        res["max_abs_diff_vs_eager"] = (R(x) - eager()).abs().max().item()
        out[name] = res
        print(name, json.dumps(res), flush=True)

    with torch.no_grad():
        src_grid = G.Grid(H, W)
        linear_case("(a) conservative to 121 x 240", G.Regridder(src_grid, G.Grid(121, 240)))
        linear_case("(b) conservative to 120 x 240 Gauss",
                    G.Regridder(src_grid, G.Grid(120, 240, "legendre-gauss")))

        T = args.sst_fields
        sst = 290 + torch.randn(1, T, H, W, device=DEV, generator=g)
        land = torch.rand(H // 16 + 1, W // 16 + 1, device=DEV, generator=g) < 1 / 3
        land = land.repeat_interleave(16, 0).repeat_interleave(16, 1)[:H, :W].roll((5, 3), (0, 1))
        sst[:, :, land] = float("nan")
        means = 288 + torch.randn(1, T, 1, 1, device=DEV, generator=g)
        stds = 1 + torch.rand(1, T, 1, 1, device=DEV, generator=g)
        R = G.Regridder((H, W), method=G.block_mean(4, 4))
        Wlat, Wlon = (torch.from_numpy(m).float().to(DEV) for m in R.dense())
        WlonT = Wlon.t().contiguous()

        def eager_sst():
            v = (~torch.isnan(sst)).float()
            num = torch.matmul(torch.matmul(Wlat, torch.nan_to_num(sst, nan=0.0)), WlonT)
            den = torch.matmul(torch.matmul(Wlat, v), WlonT)
            y = torch.where(den > 0, num / den, torch.full_like(num, float("nan")))
            return (y - means) / stds

        nbytes = (sst.numel() + T * R.out_shape[0] * R.out_shape[1]) * 4
        src, cpy = copy_pair(nbytes)
        res = paired({"native": lambda: G.sst_input(sst, 4, means, stds),
                      "copy": lambda: cpy.copy_(src), "eager": eager_sst}, args.pairs, args.reps)
        res["bytes"] = nbytes
        res["native_GBps"] = nbytes / res["native_ms"][0] / 1e6
        res["fraction_of_copy"] = res["copy_ms"][0] / res["native_ms"][0]
        a, b = G.sst_input(sst, 4, means, stds), eager_sst()
        res["nan_cells_agree"] = bool((torch.isnan(a) == torch.isnan(b)).all().item())
        res["nan_cells"] = int(torch.isnan(a).sum().item())
        res["max_abs_diff_vs_eager"] = torch.nan_to_num(a - b, nan=0.0).abs().max().item()
        name = f"(c) sst_input of {T} fields to {R.out_shape[0]} x {R.out_shape[1]}"
        out[name] = res
        print(name, json.dumps(res), flush=True)


def bench_rollout(args, out):
    from msfno_amd import export as X
    from msfno_amd import regrid as G
    from msfno_amd.rollout import Rollout
    from msfno_amd.sfno import FourierNeuralOperatorNet_Filmed
    S, H, W = args.shape
    torch.manual_seed(1)
    net = FourierNeuralOperatorNet_Filmed("cpu", None, film_layers=1, advanced_logging=False,
                                          model_depth=None, img_size=(H, W), in_chans=S,
                                          out_chans=S, embed_dim_sfno=256, num_layers=12,
                                          filter_type="non-linear", spectral_layers=3).eval().to(DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    x0 = torch.randn(1, S, H, W, generator=g, device=DEV)
    film = 0.1 * torch.randn(1, 2, 1, 256, generator=g, device=DEV)
    r = Rollout(net, film=film, scale=1.0, graph=True)
    null = lambda step, packed: None
    R = G.Regridder(G.Grid(H, W), G.Grid(121, 240))
    s6 = X.Selection(lat=slice(None, None, 6), lon=slice(None, None, 6))
    coarse = (1, S) + R.out_shape
    sides = {}

    def exporting(w, regrid=None):
        def go():
            r.export(x0, args.steps, w, normalised_input=True, regrid=regrid)
            w.flush()
        return go

    def dropped():
        for _, y in r.run(x0, args.steps, normalised_input=True):
            pass

    sides["export_u16_regrid"] = exporting(X.ForecastWriter(coarse, sink=null, device=DEV), R)
    sides["export_u16_stride6"] = exporting(
        X.ForecastWriter(x0.shape, selection=s6, sink=null, device=DEV))
    sides["export_u16_whole"] = exporting(X.ForecastWriter(x0.shape, sink=null, device=DEV))
    sides["outputs_dropped"] = dropped
    ts = {k: [] for k in sides}
    with torch.no_grad():
        for fn in sides.values():                    # one warm round (the capture is in it)
            fn()
        torch.cuda.synchronize()
        for _ in range(args.pairs):
            for k, fn in sides.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts[k].append(args.steps / (time.perf_counter() - t0))
    res = {f"{k}_steps_per_s": stats(v) for k, v in ts.items()}
    for k in list(sides)[1:]:
        res[f"{k}_over_export_u16_regrid"] = stats(
            [b / a for a, b in zip(ts["export_u16_regrid"], ts[k])])
    res["steps_per_sample"] = args.steps
    out["(d) rollout end to end"] = res
    print("(d) rollout end to end", json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[73, 721, 1440])
    ap.add_argument("--sst-fields", type=int, default=28)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--no-net", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {}
    bench_kernels(args, out)
    torch.cuda.empty_cache()
    if not args.no_net:
        bench_rollout(args, out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
