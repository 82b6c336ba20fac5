#!/usr/bin/env python3
"""Time the native power spectrum and the spectral loss on one GPU.

Kernel level, (73, 721, 721) complex64 coefficients (303 MB), device events after warm-up:
  (a) msfno_spectrum_power           reads the coefficients: 304 MB algorithmic
  (b) msfno_spectrum_power_backward  reads them, writes as much: 607 MB algorithmic
  (c) the same formula as eager torch ops on the same tensor (what a user of the
      reference's losses.py runs after the transform), forward and forward + backward
Loss level, 1 x 73 x 721 x 1440 fields, lmax 721:
  (d) spectral_l2loss_sphere(relative=True)(...).backward() end to end (two forward
      transforms, two spectra, one adjoint transform)
Prints one JSON line and writes it to profiles/spectral_loss/bench_spectral_loss.json:
median / min milliseconds, achieved GB/s against the algorithmic bytes beside the
6.3 TB/s copy rate, and the ratios to the eager formula.  There is no CPU fallback.

Usage:  python tools/bench_spectral_loss.py [--coeffs 73 721 721] [--reps 30] [--warmup 5]
        [--no-loss] [--out PATH]
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


def time_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = [a.elapsed_time(b) for a, b in ev]
    return statistics.median(t), min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--coeffs", type=int, nargs=3, default=[73, 721, 721])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-loss", action="store_true", help="skip the end-to-end loss")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "spectral_loss",
                                                  "bench_spectral_loss.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_spectral_loss.py needs a GPU (no CPU fallback)")
    from msfno_amd import _native as N
    from msfno_amd import losses as L
    from msfno_amd.harmonics import RealSHT

    n, lmax, mmax = args.coeffs
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    c = torch.view_as_complex(torch.randn(n, lmax, mmax, 2, device=dev, generator=gen))
    g = torch.rand(n, lmax, device=dev, generator=gen) + 0.5
    power = torch.empty(n, lmax, device=dev)
    dc = torch.empty_like(c)
    lib = N.lib()
    stream = N.stream_of(dev)

    def fwd():
        N.check(lib.msfno_spectrum_power(c.data_ptr(), power.data_ptr(), n, lmax, mmax, stream))

    def bwd():
        N.check(lib.msfno_spectrum_power_backward(c.data_ptr(), g.data_ptr(), dc.data_ptr(), n,
                                                  lmax, mmax, stream))

    ce = c.clone().requires_grad_()

    def eager_power(x):
        a = torch.view_as_real(x)
        a = a[..., 0] ** 2 + a[..., 1] ** 2
        return a[..., :, 0] + 2 * torch.sum(a[..., :, 1:], dim=-1)

    def eager_fwd():
        with torch.no_grad():
            eager_power(c)

    def eager_fwd_bwd():
        ce.grad = None
        eager_power(ce).backward(g)

    # the two must agree before their times are compared
    fwd()
    bwd()
    eager_fwd_bwd()
    ref = eager_power(c.detach())
    perr = ((power - ref).abs() / ref).max().item()
    derr = ((torch.view_as_real(dc) - torch.view_as_real(ce.grad)).abs().max()
            / torch.view_as_real(ce.grad).abs().max()).item()
    assert perr < 1e-4 and derr < 1e-6, (perr, derr)

    a_med, a_min = time_ms(fwd, args.reps, args.warmup)
    b_med, b_min = time_ms(bwd, args.reps, args.warmup)
    e_med, e_min = time_ms(eager_fwd, args.reps, args.warmup)
    f_med, f_min = time_ms(eager_fwd_bwd, args.reps, args.warmup)
    ce.grad = None
    nbytes = 8 * n * lmax * mmax
    out = {
        "tool": "bench_spectral_loss", "coeffs": [n, lmax, mmax], "reps": args.reps,
        "warmup": args.warmup, "timing": "device events, per call",
        "spectrum_power_ms": round(a_med, 4), "spectrum_power_ms_min": round(a_min, 4),
        "spectrum_power_GBps": round((nbytes + 4 * n * lmax) / a_med / 1e6, 1),
        "spectrum_power_backward_ms": round(b_med, 4),
        "spectrum_power_backward_ms_min": round(b_min, 4),
        "spectrum_power_backward_GBps": round((2 * nbytes + 4 * n * lmax) / b_med / 1e6, 1),
        "eager_fwd_ms": round(e_med, 4), "eager_fwd_ms_min": round(e_min, 4),
        "eager_fwd_bwd_ms": round(f_med, 4), "eager_fwd_bwd_ms_min": round(f_min, 4),
        "ratio_eager_fwd_over_native_fwd": round(e_med / a_med, 2),
        "ratio_eager_fwd_bwd_over_native_fwd_bwd": round(f_med / (a_med + b_med), 2),
        "algorithmic_MB": {"spectrum_power": round((nbytes + 4 * n * lmax) / 1e6, 1),
                           "spectrum_power_backward": round((2 * nbytes + 4 * n * lmax) / 1e6, 1)},
        "copy_rate_GBps_reference": 6300,
        "power_max_rel_diff_native_vs_eager": float(f"{perr:.3e}"),
        "grad_max_rel_diff_native_vs_eager": float(f"{derr:.3e}"),
    }
    del ce, dc, power, ref

    if not args.no_loss:
        B, C, H, W, LM = 1, 73, 721, 1440, 721
        sht = RealSHT(H, W, lmax=LM, mmax=W // 2 + 1).float().to(dev)
        tar = torch.randn(B, C, H, W, device=dev, generator=gen)
        prd = (tar + 0.3 * torch.randn(B, C, H, W, device=dev, generator=gen)).requires_grad_()

        def loss_step():
            prd.grad = None
            L.spectral_l2loss_sphere(sht, prd, tar, relative=True).backward()

        l_reps, l_warmup = max(20, args.reps // 2), 3
        l_med, l_min = time_ms(loss_step, l_reps, l_warmup)
        out.update({"loss_reps": l_reps, "loss_warmup": l_warmup,
                    "loss": "spectral_l2loss_sphere(relative=True), forward + backward",
                    "loss_shape": [B, C, H, W], "loss_lmax": LM, "loss_mmax": W // 2 + 1,
                    "loss_fwd_bwd_ms": round(l_med, 4), "loss_fwd_bwd_ms_min": round(l_min, 4)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
