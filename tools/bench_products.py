#!/usr/bin/env python3
"""Time the native ensemble products and threshold counts on one GPU against the same results
in eager torch.

Workload: M members of (1, 73, 721, 1440) fp32 fields (303 MB each), 300 + N(0, 1), against a
300.5 + N(0, 1) truth, random latitude weights:
  products         mean + std + three quantiles (0.1, 0.5, 0.9) + two thresholds (300.0, 301.0):
                   ensemble.products, one pass, reads M fields and writes 7
  threshold sums   four thresholds (299.0, 300.0, 300.7, 302.0): ensemble.threshold_sums into
                   preallocated buffers, reads M + 1 fields
  the same results as eager torch ops on the same tensors: sort along the member axis and a
  lerp, mean, std, comparisons, and one masked sum per bin: what a user of the library
  without these kernels runs
Device events; the two sides alternate in one process, pair by pair, after one warm pair.
Prints one JSON line per M and case: (median, min, max) milliseconds of each side over the
pairs, the (median, min, max) of the per-pair ratio eager / native, the algorithmic bytes,
their time at the 6.3 TB/s a float4 copy reaches and the fraction of it that the native side
achieves, and the largest difference between the two sides.  There is no CPU fallback: without
a GPU it fails.

Usage:  python tools/bench_products.py [--members 8 32] [--pairs 7] [--out FILE.json]
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
LEVELS = (0.1, 0.5, 0.9)
PROB_THR = (300.0, 301.0)
SUM_THR = (299.0, 300.0, 300.7, 302.0)


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    return statistics.median(ts), min(ts), max(ts)


def paired(native, eager, pairs):
    """The two sides alternating; one warm pair first."""
    native()
    eager()
    torch.cuda.synchronize()
    tn, te = [], []
    for _ in range(pairs):
        tn.append(once(native))
        te.append(once(eager))
    return {"native_ms": stats(tn), "eager_ms": stats(te),
            "eager_over_native": stats([e / n for n, e in zip(tn, te)])}


def eager_products(ens, thr):
    """(mean, std, (3, ...) quantiles, (2, ...) prob)"""
    M = ens.shape[0]
    srt = ens.sort(dim=0).values
    qs = []
    for q in LEVELS:
        pos = q * (M - 1)
        lo = min(int(pos), M - 1)
        hi = min(lo + 1, M - 1)
        qs.append(torch.lerp(srt[lo], srt[hi], pos - lo))
    del srt
    prob = [(ens > t).float().mean(dim=0) for t in thr]
    return ens.mean(dim=0), ens.std(dim=0), torch.stack(qs), torch.stack(prob)


def eager_threshold_sums(ens, tar, w, thr):
    """(1, S, nt, 2, M + 1)"""
    M = ens.shape[0]
    wv = w[:, None]
    per_t = []
    for t in thr:
        k = (ens > t).sum(dim=0)
        o = tar > t
        rows = [[(wv * (k == r)).sum(dim=(-1, -2)) for r in range(M + 1)],
                [(wv * ((k == r) & o)).sum(dim=(-1, -2)) for r in range(M + 1)]]
        per_t.append(torch.stack([torch.stack(r, dim=-1) for r in rows], dim=-2))
    return torch.stack(per_t, dim=-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--shape", type=int, nargs=3, default=[73, 721, 1440])
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from msfno_amd import ensemble as E
    S, H, W = args.shape
    n = S * H * W
    g = torch.Generator(device=DEV).manual_seed(0)
    w = torch.rand(H, device=DEV, generator=g) + 0.1
    tar = 300.5 + torch.randn(1, S, H, W, device=DEV, generator=g)
    pthr = torch.tensor(PROB_THR, device=DEV).expand(S, len(PROB_THR)).contiguous()
    sthr = torch.tensor(SUM_THR, device=DEV).expand(1, S, len(SUM_THR)).contiguous()
    out = {}
    for M in args.members:
        ens = 300 + torch.randn(M, 1, S, H, W, device=DEV, generator=g)
        with torch.no_grad():
            r = paired(lambda: E.products(ens, quantiles=LEVELS, thresholds=pthr),
                       lambda: eager_products(ens, PROB_THR), args.pairs)
            got = E.products(ens, quantiles=LEVELS, thresholds=pthr)
            want = eager_products(ens, PROB_THR)
            r["max_abs_diff_vs_eager"] = {
                k: (a - b).abs().max().item()
                for k, a, b in zip(("mean", "std", "quantiles", "prob"),
                                   (got.mean, got.std, got.quantiles, got.prob), want)}
            del got, want
            r["bytes"] = (M + 2 + len(LEVELS) + len(PROB_THR)) * n * 4
            r["stream_ms_at_6.3TBps"] = r["bytes"] / COPY_RATE * 1e3
            r["fraction_of_stream"] = r["stream_ms_at_6.3TBps"] / r["native_ms"][0]
            out[f"products M={M}"] = r
            print(f"products M={M}", json.dumps(r), flush=True)

            counts = torch.empty(1, S, len(SUM_THR), 2, M + 1, device=DEV)
            ws = E.threshold_workspace(M, 1, S, len(SUM_THR), H, W, DEV)
            r = paired(lambda: E._threshold_launch(ens, tar, w, sthr, counts, ws),
                       lambda: eager_threshold_sums(ens, tar, w, SUM_THR), args.pairs)
            E._threshold_launch(ens, tar, w, sthr, counts, ws)
            ref = eager_threshold_sums(ens, tar, w, SUM_THR)
            r["max_rel_diff_vs_eager"] = ((ref - counts).abs() / ref.clamp(min=1e-30)).max().item()
            del ref
            r["bytes"] = (M + 1) * n * 4
            r["stream_ms_at_6.3TBps"] = r["bytes"] / COPY_RATE * 1e3
            r["fraction_of_stream"] = r["stream_ms_at_6.3TBps"] / r["native_ms"][0]
            out[f"threshold_sums M={M}"] = r
            print(f"threshold_sums M={M}", json.dumps(r), flush=True)
        del ens
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
