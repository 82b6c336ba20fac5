#!/usr/bin/env python3
"""Time the native statistics over time (msfno_amd/timestats.py, csrc/timestats.hip) on one GPU
against a device copy of the same bytes and against the same recurrence in eager torch, and end
to end through ``Rollout.verify_maps``.

Kernel cases on (B, 73, 721, 1440) fp32 fields, 300 + N(0, 1), at B = 1 and B = 8:
  (a) the FIELD update (2 planes and the count): B + 6 planes of traffic
  (b) the ERROR update with a climatology (8 planes and the count): 3 B + 18 planes
  (c) the merge of two ERROR states with anomalies: 27 planes (B does not enter)
Each against
  copy    ``dst.copy_(src)`` of half the bytes the call moves (read once, written once): it
          moves the same number of bytes, so copy / native is the share of the achievable
          stream that the kernel reaches
  eager   the same recurrence as eager in-place torch ops on the same state tensors, one
          batch element after the other
Device events; the sides alternate in one process, pair by pair, after one warm round.
  (d) end to end: a --steps step ``Rollout.verify_maps`` (with a climatology) of the 12-block
      network (config 3 of bench.py, HIP graph) against ``Rollout.verify`` and against the
      rollout alone, in seconds per rollout, and the update's own time per scored step from (b).
Prints one JSON line per case: (median, min, max) milliseconds of each side over the pairs, the
(median, min, max) of the per-pair ratios to the native side, and the algorithmic bytes.  There
is no CPU fallback: without a GPU it fails.

Usage:  python tools/bench_timestats.py [--pairs 7] [--reps 5] [--steps 12] [--no-net] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "modulated-spherical-fourier-neural-operator_amd"),
          os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from bench_regrid import copy_pair, paired, stats  # noqa: E402

DEV = "cuda"


def eager_field(x, n, mean, m2):
    for b in range(x.shape[0]):
        n += 1
        delta = x[b] - mean
        mean += delta / n
        m2 += delta * (x[b] - mean)


def eager_error(p, t, c, n, q):
    """q = the 8 planes; c (B, S, H, W)."""
    for b in range(p.shape[0]):
        n += 1
        d = p[b] - t[b]
        delta = d - q[0]
        q[0] += delta / n
        q[1] += delta * (d - q[0])
        q[2] += (d.abs() - q[2]) / n
        pa, ta = p[b] - c[b], t[b] - c[b]
        dpa = pa - q[3]
        q[3] += dpa / n
        q[4] += dpa * (pa - q[3])
        dta = ta - q[5]
        q[5] += dta / n
        q[6] += dta * (ta - q[5])
        q[7] += dpa * (ta - q[5])


def eager_merge(na, qa, nb, qb):
    n = na + nb
    f = nb / n
    g = na * f
    for m, v in ((0, 1), (3, 4), (5, 6)):
        delta = qb[m] - qa[m]
        if m == 3:
            dpa = delta
        qa[m] += delta * f
        qa[v] += qb[v] + delta * delta * g
    qa[7] += qb[7] + dpa * delta * g
    qa[2] += (qb[2] - qa[2]) * f
    na.copy_(n)


def bench_kernels(args, out):
    from msfno_amd import timestats as T
    S, H, W = args.shape
    plane = S * H * W * 4
    g = torch.Generator(device=DEV).manual_seed(0)
    per_step = {}
    for B in args.batches:
        t = 300 + torch.randn(B, S, H, W, device=DEV, generator=g)
        p = t + 0.3 * torch.randn(B, S, H, W, device=DEV, generator=g)
        c = 300 + 0.7 * torch.randn(S, H, W, device=DEV, generator=g)
        cb = c.expand(B, S, H, W)

        def case(name, nbytes, native, eager):
            src, cpy = copy_pair(nbytes)
            res = paired({"native": native, "copy": lambda: cpy.copy_(src), "eager": eager},
                         args.pairs, args.reps)
            res["bytes"] = nbytes
            res["native_GBps"] = nbytes / res["native_ms"][0] / 1e6
            res["fraction_of_copy"] = res["copy_ms"][0] / res["native_ms"][0]
            out[name] = res
            print(name, json.dumps(res), flush=True)
            del src, cpy
            torch.cuda.empty_cache()
            return res

        with torch.no_grad():
            fs = T.FieldStats(S, H, W, device=DEV)
            n = torch.zeros(S, H, W, device=DEV)
            q = torch.zeros(8, S, H, W, device=DEV)
            case(f"(a) FIELD update, B = {B}", (B + 6) * plane, lambda: fs.update(t),
                 lambda: eager_field(t, n, q[0], q[1]))
            del fs
            em = T.ErrorMaps(S, H, W, anomalies=True, device=DEV)
            em.update(p, t, clim=c)
            res = case(f"(b) ERROR update with a climatology, B = {B}", (3 * B + 18) * plane,
                       lambda: em.update(p, t, clim=c), lambda: eager_error(p, t, cb, n, q))
            per_step[B] = res["native_ms"]
            if B == args.batches[0]:
                other = T.ErrorMaps(S, H, W, anomalies=True, device=DEV)
                other.update(t, p, clim=c)
                nb = torch.ones(S, H, W, device=DEV)
                qb = torch.randn(8, S, H, W, device=DEV, generator=g)
                n.fill_(1.0)
                case("(c) merge of two ERROR states with anomalies", 27 * plane,
                     lambda: em.merge(other), lambda: eager_merge(n, q, nb, qb))
                del other, nb, qb
            del em, n, q
            torch.cuda.empty_cache()
    return per_step


def bench_rollout(args, out, per_step):
    from msfno_amd import timestats as T
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
    clim = torch.randn(S, H, W, generator=g, device=DEV)
    truths = [(torch.randn(1, S, H, W, generator=g, device=DEV), clim) for _ in range(args.steps)]
    maps = T.LeadTimeMaps(args.steps, S, H, W, anomalies=True, device=DEV)

    def alone():
        for _, y in r.run(x0, args.steps, normalised_input=True):
            pass

    sides = {
        "verify": lambda: r.verify(x0, truths, args.steps, normalised_input=True),
        "verify_maps": lambda: r.verify_maps(x0, truths, args.steps, maps=maps,
                                             normalised_input=True),
        "rollout_alone": alone,
    }
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
                ts[k].append((time.perf_counter() - t0) * 1e3)
    res = {f"{k}_ms_per_rollout": stats(v) for k, v in ts.items()}
    res["maps_minus_verify_ms_per_step"] = stats(
        [(b - a) / args.steps for a, b in zip(ts["verify"], ts["verify_maps"])])
    res["update_ms_per_scored_step"] = per_step.get(1)
    res["steps"] = args.steps
    out["(d) rollout end to end"] = res
    print("(d) rollout end to end", json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[73, 721, 1440])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--no-net", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {}
    per_step = bench_kernels(args, out)
    torch.cuda.empty_cache()
    if not args.no_net:
        bench_rollout(args, out, per_step)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
