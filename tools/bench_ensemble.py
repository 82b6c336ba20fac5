#!/usr/bin/env python3
"""Time the native ensemble verification sums and the CRPS gradient on one GPU against the
same sums in eager torch.

Workload: M members of (1, 73, 721, 1440) fp32 fields (303 MB each) against one truth,
300 + N(0, 1) against 300.5 + N(0, 1), random latitude weights; device events, warm, the
median of the runs:
  msfno_ens_sums with and without the rank histogram   reads (M + 1) fields
  msfno_ens_crps_backward                              reads M + 1, writes M fields
  the same five sums (and the rank counts) as eager torch ops on the same tensors: the
  member mean, the |.| mean, a loop over i of (x_i - x_{i+1..}) for the pair sums, one
  masked sum per rank: what a user of the library without these kernels runs
  at M = 8, eager autograd of abs - gini / (M (M - 1)) (forward + backward; at M = 32 its
  saved pair tensors would take 150 GB)
Prints one JSON line per M: (median, min, max) milliseconds, the algorithmic bytes, their
time at the 6.3 TB/s a float4 copy reaches, and the largest relative difference between
the native and the eager sums.  There is no CPU fallback: without a GPU it fails.

Usage:  python tools/bench_ensemble.py [--members 8 32] [--out FILE.json]
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


def timed(fn, warm=3, runs=9):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def eager_sums(ens, tar, w, hist):
    M = ens.shape[0]
    wv = w[:, None]
    d = ens - tar
    dbar = d.mean(dim=0)
    res = [(wv * dbar * dbar).sum(dim=(-1, -2)), (wv * dbar).sum(dim=(-1, -2)),
           (wv * d.abs().mean(dim=0)).sum(dim=(-1, -2))]
    del d
    g = torch.zeros_like(tar)
    q = torch.zeros_like(tar)
    for i in range(M - 1):
        p = ens[i:i + 1] - ens[i + 1:]
        g += p.abs().sum(dim=0)
        q += (p * p).sum(dim=0)
    res += [(wv * g).sum(dim=(-1, -2)), (wv * q).sum(dim=(-1, -2))]
    h = None
    if hist:
        rank = (ens < tar).sum(dim=0)
        h = torch.stack([(wv * (rank == r)).sum(dim=(-1, -2)) for r in range(M + 1)], dim=-1)
    return torch.stack(res, dim=-1), h


def eager_forward_backward(ens, tar, w):
    M = ens.shape[0]
    x = ens.detach().requires_grad_()
    gini = 0
    for i in range(M - 1):
        gini = gini + (x[i:i + 1] - x[i + 1:]).abs().sum(dim=0)
    loss = (w[:, None] * ((x - tar).abs().mean(dim=0) - gini / (M * (M - 1)))).sum()
    loss.backward()
    return x.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--shape", type=int, nargs=3, default=[73, 721, 1440])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from msfno_amd import _native as N
    from msfno_amd import ensemble as E
    lib = N.lib()
    S, H, W = args.shape
    n = S * H * W
    w = torch.rand(H, device=DEV) + 0.1
    tar = 300.5 + torch.randn(1, S, H, W, device=DEV)
    out = {}
    for M in args.members:
        ens = 300 + torch.randn(M, 1, S, H, W, device=DEV)
        ws = E.workspace(M, 1, S, H, W, DEV)
        sums = torch.empty(1, S, 5, device=DEV)
        hist = torch.empty(1, S, M + 1, device=DEV)
        g = torch.ones(S, device=DEV)
        st = N.stream_of(ens.device)

        def native_sums(h):
            N.check(lib.msfno_ens_sums(ens.data_ptr(), n, tar.data_ptr(), w.data_ptr(),
                                       sums.data_ptr(), h, M, S, H, W, ws.data_ptr(), ws.numel(),
                                       st), "msfno_ens_sums")

        r = {"sums_hist_ms": timed(lambda: native_sums(hist.data_ptr())),
             "sums_nohist_ms": timed(lambda: native_sums(None))}
        dens = torch.empty(M, 1, S, H, W, device=DEV)
        r["backward_ms"] = timed(lambda: N.check(lib.msfno_ens_crps_backward(
            ens.data_ptr(), n, tar.data_ptr(), w.data_ptr(), g.data_ptr(), 1.0 / (M * (M - 1)),
            dens.data_ptr(), n, M, S, H, W, st), "msfno_ens_crps_backward"))
        del dens
        r["bytes_read_fwd"] = (M + 1) * n * 4
        r["bytes_bwd"] = (2 * M + 1) * n * 4
        r["stream_fwd_ms_at_6.3TBps"] = r["bytes_read_fwd"] / COPY_RATE * 1e3
        r["stream_bwd_ms_at_6.3TBps"] = r["bytes_bwd"] / COPY_RATE * 1e3
        with torch.no_grad():
            r["eager_sums_nohist_ms"] = timed(lambda: eager_sums(ens, tar, w, False), 1, 3)
            r["eager_sums_hist_ms"] = timed(lambda: eager_sums(ens, tar, w, True), 1, 3)
            es, eh = eager_sums(ens, tar, w, True)
            native_sums(hist.data_ptr())
            torch.cuda.synchronize()
            # the non-negative sums: eager torch forms them from differences too
            r["max_rel_diff_vs_eager_nonneg"] = (
                (es[..., 2:] - sums[..., 2:]).abs() / es[..., 2:].abs()).max().item()
            r["hist_max_rel_diff_vs_eager"] = (
                (eh - hist).abs() / eh.clamp(min=1e-30)).max().item()
            del es, eh
        if M <= 8:
            r["eager_fwd_bwd_ms"] = timed(lambda: eager_forward_backward(ens, tar, w), 1, 3)
        out[f"M={M}"] = r
        print(f"M={M}", json.dumps(r), flush=True)
        del ens
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
