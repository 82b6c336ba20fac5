#!/usr/bin/env python3
"""Time the forecast export on one GPU: the native 16-bit packing against a device copy of its
algorithmic bytes and against the same encoding in eager torch, and a rollout that leaves the
device through ``Rollout.export`` against the parent's only way out, ``y.cpu()`` per step.

Workload: (1, 73, 721, 1440) fp32 fields (303 MB), 300 + N(0, 1).
  (a) whole      msfno_pack16 on the whole field into preallocated buffers.  Algorithmic bytes:
                 2 x 303 MB read (range pass, pack pass) + 152 MB written.  Its pair partner is
                 a float4 device copy that moves as many bytes (copy_ of half of them).
  (b) stride 6   msfno_pack16 on the window lat[::6], lon[::6] (121 x 240 of every field).
                 Algorithmic bytes: 2 x 4 B read + 2 B written per selected point; the copy of
                 as many bytes is its partner.  (The hardware fetches whole cache lines of the
                 121 touched rows: 73 x 121 x 1440 x 4 B = 51 MB a pass.)
  (c) eager      the same encoding as eager torch ops on the same tensor: amin / amax, frexp for
                 the exponent, subtract, ldexp, round, clamp and the conversion to 16 bits; the
                 partner of (a) in a second pairing.
  (e) one slab   msfno_pack16 on one (721, 1440) slab (4 MB: the pack pass finds it in L2) times
                 73, against (a): meant to show what the second read of a 303 MB field costs;
                 measured, it is three launches on a 4 MB problem, a latency figure.
  (d) end to end steps/s of the 12-block network (config 3 of bench.py, HIP graph) over
                 ``--steps`` steps per sample: ``for i, y in rollout.run(...): y.cpu()``, against
                 Rollout.export with u16 on the whole field, u16 at stride 6 and f32 on the
                 whole field (each with the final flush inside the timed window), and against
                 the rollout that drops its outputs.  The variants alternate sample by sample.
Device events for (a)-(c), (e), each sample ``--reps`` calls; a host clock around work that ends
in a synchronise for (d).  The sides of a pairing alternate in one process after one warm
round.  Prints one JSON line per case: (median, min, max) of each side over the pairs and of the
per-pair ratio.  There is no CPU fallback: without a GPU it fails.

Usage:  python tools/bench_export.py [--pairs 7] [--reps 10] [--steps 12] [--no-net]
                                     [--out FILE.json]
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

COPY_RATE = 6.3e12
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


def eager_pack(x):
    """(ref, exp2, q) of x (1, S, H, W) as eager torch ops; q as int16 holding q - 32768 (this
    torch has no 16-bit unsigned arithmetic on the device)."""
    lo = x.amin(dim=(-1, -2), keepdim=True)
    hi = x.amax(dim=(-1, -2), keepdim=True)
    d = hi - lo
    m, e = torch.frexp(d)
    E = torch.where(d == 0, torch.zeros_like(e),
                    torch.where(m <= 65535.0 / 65536.0, e - 16, e - 15).clamp(min=-126))
    v = torch.ldexp(x - lo, -E).round().clamp(0, 65535)
    return lo, E, (v - 32768).to(torch.int16)


def bench_kernels(args, out):
    from msfno_amd import export as X
    S, H, W = args.shape
    g = torch.Generator(device=DEV).manual_seed(0)
    x = 300 + torch.randn(1, S, H, W, device=DEV, generator=g)
    n = S * H * W

    def case(name, sel, x=x, scale=1):
        r = (sel or X.Selection()).resolve(x.shape)
        dst = X.empty_packed(r.out_shape, DEV, sel)
        ws = X.workspace(r.out_shape, DEV)
        npts = r.out_shape[1] * r.out_shape[2] * r.out_shape[3]
        nbytes = npts * 10
        src = torch.empty(nbytes // 8, dtype=torch.float32, device=DEV).normal_()
        cpy = torch.empty_like(src)
        res = paired({"native": lambda: X.pack(x, sel, out=dst, ws=ws),
                      "copy": lambda: cpy.copy_(src)}, args.pairs, args.reps)
        res["bytes"] = nbytes
        res["stream_ms_at_6.3TBps"] = nbytes / COPY_RATE * 1e3
        res["fraction_of_stream"] = res["stream_ms_at_6.3TBps"] / res["native_ms"][0]
        res["scale"] = scale
        out[name] = res
        print(name, json.dumps(res), flush=True)
        return dst, ws

    with torch.no_grad():
        dst, ws = case("(a) pack16 whole field", None)
        case("(b) pack16 stride-6 window",
             X.Selection(lat=slice(None, None, 6), lon=slice(None, None, 6)))
        case("(e) pack16 one slab (x S for the field)", None, x=x[:, :1].contiguous(), scale=S)
        res = paired({"native": lambda: X.pack(x, None, out=dst, ws=ws),
                      "eager": lambda: eager_pack(x)}, args.pairs, max(1, args.reps // 3))
        lo, E, q = eager_pack(x)
        X.pack(x, None, out=dst, ws=ws)
        nq = dst.q.view(torch.int16).to(torch.int32) & 0xFFFF
        res["eager_differs"] = {"ref": int((lo.view(-1) != dst.ref.view(-1)).sum().item()),
                                "exp2": int((E.view(-1) != dst.exp2.view(-1)).sum().item()),
                                "q": int((nq != q.to(torch.int32) + 32768).sum().item())}
        out["(c) pack16 against eager torch"] = res
        print("(c) pack16 against eager torch", json.dumps(res), flush=True)
        # the decode, for the archive replay
        y = torch.empty(1, S, H, W, device=DEV)
        src = torch.empty(n * 6 // 8, dtype=torch.float32, device=DEV).normal_()
        cpy = torch.empty_like(src)
        res = paired({"native": lambda: X.unpack(dst, out=y), "copy": lambda: cpy.copy_(src)},
                     args.pairs, args.reps)
        res["bytes"] = n * 6
        out["unpack16 whole field"] = res
        print("unpack16 whole field", json.dumps(res), flush=True)


def bench_rollout(args, out):
    from msfno_amd import export as X
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
    s6 = X.Selection(lat=slice(None, None, 6), lon=slice(None, None, 6))
    writers = {"export_u16_whole": X.ForecastWriter(x0.shape, sink=null, device=DEV),
               "export_u16_stride6": X.ForecastWriter(x0.shape, selection=s6, sink=null, device=DEV),
               "export_f32_whole": X.ForecastWriter(x0.shape, encoding="f32", sink=null, device=DEV)}

    def cpu_per_step():
        for _, y in r.run(x0, args.steps, normalised_input=True):
            y.cpu()

    def dropped():
        for _, y in r.run(x0, args.steps, normalised_input=True):
            pass

    def exporting(w):
        def go():
            r.export(x0, args.steps, w, normalised_input=True)
            w.flush()
        return go

    sides = {"cpu_per_step": cpu_per_step}
    sides.update({k: exporting(w) for k, w in writers.items()})
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
        res[f"{k}_over_cpu_per_step"] = stats([b / a for a, b in zip(ts["cpu_per_step"], ts[k])])
    res["steps_per_sample"] = args.steps
    with torch.no_grad():
        last = [y for _, y in r.run(x0, args.steps, normalised_input=True)][-1]
    res["outputs_finite"] = bool(torch.isfinite(last).all().item())
    res["host_bytes_per_step"] = {"cpu_per_step": S * H * W * 4, "export_u16_whole": S * H * W * 2,
                                  "export_u16_stride6": S * 121 * 240 * 2 if (H, W) == (721, 1440)
                                  else None, "export_f32_whole": S * H * W * 4}
    out["(d) rollout end to end"] = res
    print("(d) rollout end to end", json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[73, 721, 1440])
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
