#!/usr/bin/env python3
"""Time the vector spherical harmonic transforms against the scalar ones on one GPU.

At 721 x 1440, lmax 360, bc = 15 (the model's 15 wind pairs), device events after warm-up,
the two sides alternating within every repetition of one process:
  (a) RealVectorSHT on (15, 2, 721, 1440)          vs  four RealSHT calls on (15, 721, 1440)
  (b) InverseRealVectorSHT on (15, 2, 360, 361)    vs  four InverseRealSHT calls on (15, 360, 361)
A vector transform is two scalar transforms of 30 fields each plus its streaming kernels
(the combine on the spectra; the pack on the spectra and the add over the grid), so four
scalar calls of 15 fields are the same Legendre and FFT work without them.  Expected from
the byte counts: (a) within 1.1x, (b) within 1.3x.
Prints one JSON line and writes it to profiles/vector/bench_vector_sht.json: median / min
milliseconds per side and the ratio of the medians.  There is no CPU fallback.

Usage:  python tools/bench_vector_sht.py [--grid 721 1440] [--lmax 360] [--bc 15]
        [--reps 300] [--warmup 10] [--out PATH]
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


def time_pair_ms(fa, fb, reps, warmup):
    """Median and min milliseconds of fa and of fb, run alternately."""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for e0, e1, e2 in ev:
        e0.record()
        fa()
        e1.record()
        fb()
        e2.record()
    torch.cuda.synchronize()
    ta = [e0.elapsed_time(e1) for e0, e1, _ in ev]
    tb = [e1.elapsed_time(e2) for _, e1, e2 in ev]
    return (statistics.median(ta), min(ta)), (statistics.median(tb), min(tb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, nargs=2, default=[721, 1440])
    ap.add_argument("--lmax", type=int, default=360)
    ap.add_argument("--bc", type=int, default=15)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "vector",
                                                  "bench_vector_sht.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_vector_sht.py needs a GPU (no CPU fallback)")
    from msfno_amd import harmonics as H

    nlat, nlon = args.grid
    lmax, mmax, bc = args.lmax, args.lmax + 1, args.bc
    dev = torch.device("cuda", 0)
    kw = dict(lmax=lmax, mmax=mmax, grid="equiangular")
    vsht = H.RealVectorSHT(nlat, nlon, **kw).float().to(dev)
    ivsht = H.InverseRealVectorSHT(nlat, nlon, **kw).float().to(dev)
    sht = H.RealSHT(nlat, nlon, **kw).float().to(dev)
    isht = H.InverseRealSHT(nlat, nlon, **kw).float().to(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    v = torch.randn(bc, 2, nlat, nlon, device=dev, generator=gen)
    x = [torch.randn(bc, nlat, nlon, device=dev, generator=gen) for _ in range(4)]

    with torch.no_grad():
        st = vsht(v)
        c = [sht(xi) for xi in x]
        fwd = time_pair_ms(lambda: vsht(v), lambda: [sht(xi) for xi in x], args.reps,
                           args.warmup)
        inv = time_pair_ms(lambda: ivsht(st), lambda: [isht(ci) for ci in c], args.reps,
                           args.warmup)

    def side(t):
        return {"median_ms": round(t[0], 4), "min_ms": round(t[1], 4)}

    res = {"device": torch.cuda.get_device_name(0), "nlat": nlat, "nlon": nlon, "lmax": lmax,
           "mmax": mmax, "bc": bc, "reps": args.reps,
           "forward": {"vector": side(fwd[0]), "four_scalar": side(fwd[1]),
                       "ratio": round(fwd[0][0] / fwd[1][0], 4), "expected_within": 1.1},
           "inverse": {"vector": side(inv[0]), "four_scalar": side(inv[1]),
                       "ratio": round(inv[0][0] / inv[1][0], 4), "expected_within": 1.3}}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
