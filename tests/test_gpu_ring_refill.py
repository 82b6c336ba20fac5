"""The MFMA kernels that refill an LDS ring by LDS-DMA while they compute
(csrc/gemm_x6c.hip: the spectral-MLP layers; csrc/mlp_fused_h.hip: the fused block
MLP; csrc/skip_h.hip: the two inner-skip kernels; csrc/x3h_tile.h: X3hRing, the ring and its
counted wait for the block MLP and the one-tile skip).  The spectral layers and the persistent skip issue
a refill piece by piece between the MFMA groups of a step, the block MLP and the
one-tile skip as one burst behind the step's first MFMAs; either way what orders a piece
against the reads of its ring slot is a counted s_waitcnt and a barrier, so a miscount
shows up as a result that is wrong at some sizes or differs from run to run.  Every
case therefore

  * is compared with the same computation in fp64 on the CPU, the error bounded by
    twice the error of the fp32 CPU evaluation of the same data (the bar of
    tests/test_gpu_x3h.py), and
  * runs three times on the same inputs in one process, the three outputs bit-equal.

Sizes: the smallest at which the loops take each of their paths.
  spectral chain  C = 8, 16, 32, 64: hidden K = 16 .. 128, that is 1, 2, 4 and 8 k-tiles
                  of 16 (one tile: no refill at all; two: prologue only; four: the first
                  count at which a stage is refilled while the ring wraps); 33 x 64 with
                  lmax 24 gives several column tiles with a ragged last one, 13 x 26 with
                  lmax 12 a single one.  Once with MSFNO_X3C_BM64=0 (the 128-row,
                  three-stage kernel) and once with the switch unset (the 64-row,
                  two-stage kernel takes these small grids), each in a child process:
                  the switch is read once per process.
  block MLP       C = 256, H = 512 (the only fused shape), P = 4, 64, 68, 212 pixels: one
                  partial 64-pixel tile, one full, one full + a 4-pixel tail, three
                  full + a 20-pixel tail; B = 1, 2; with and without the residual.
                  mlp_fused_h_kernel is reached through the block forward only (no entry
                  point of its own; msfno_mlp_forward_affine runs the general fused MLP
                  of mlp_gen_h.hip and answers MSFNO_EUNSUPPORTED at 256 -> 512 -> 256), so
                  these cases run a whole C = 256 block on a grid of P points.
  inner skip      msfno_conv1x1, C = 256: P = 212 (the persistent kernel, P % 4 == 0)
                  and P = 210 (one tile per workgroup), B = 2: four 128-pixel tiles on at
                  least four workgroups, one tile each.  The persistent kernel's loop over
                  tiles runs with B = 3, P = 260 on ONE workgroup (MSFNO_SKIP_GRID=0): nine
                  tiles, the next tile's x through the ring, the scale tables reloaded at
                  two field boundaries, each field ending on a 4-pixel tile, the tail's
                  dummy groups.
References: oracle/sfno_ref.py (layers.py:536-639 SpectralAttentionS2, :145-178 MLP,
sfnonet.py:359-393 the block).
"""
import functools
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    _repo = os.path.dirname(HERE)
    for _d in (HERE, _repo, os.path.join(_repo, "modulated-spherical-fourier-neural-operator_amd")):
        sys.path.insert(0, _d)

import numpy as np  # noqa: E402
import pytest  # noqa: E402
import torch  # noqa: E402

from oracle import sfno_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bar(got, want64, want32, what):
    """error vs fp64 within 2x of the fp32 CPU evaluation's (tests/test_gpu_x3h.py)"""
    e = (got.double() - want64).abs().max().item()
    e32 = (want32.double() - want64).abs().max().item()
    ymax = max(want64.abs().max().item(), 1.0)
    print(f"{what}: max-abs vs fp64  gpu {e:.3e}  cpu-fp32 {e32:.3e}  (|y|max {ymax:.3f})")
    assert e < max(2.0 * e32, 1e-6 * ymax), (what, e, e32)


def _thrice(f):
    """f() three times; the first result, and whether all three are bit-equal"""
    ys = [f() for _ in range(3)]
    return ys[0], all(torch.equal(ys[0], y) for y in ys[1:])


# ---- spectral chain ------------------------------------------------------------------

# (C, nlat, nlon, lmax)
SPEC_CASES = [(C, *grid) for grid in ((33, 64, 24), (13, 26, 12)) for C in (8, 16, 32, 64)]
SPEC_IDS = [f"C{c[0]}_{c[1]}x{c[2]}_l{c[3]}" for c in SPEC_CASES]
SPEC_B = 2


def _spec_inputs(case, dtype=torch.float32):
    C, nlat, nlon, lmax = case
    cfg = sfno_ref.BlockCfg(filter_type="non-linear")
    p = sfno_ref.make_block_params(C, lmax, lmax + 1, cfg, seed=3 + C, randomize_affine=True)
    g = torch.Generator().manual_seed(100 + C + nlat)
    # the chain is positively homogeneous and its initial weights (0.02 randn) shrink a
    # unit input to 3e-4 (C = 8) .. 3e-2 (C = 64): scale the input so the output is O(1)
    # and the bar's floor, 1e-6 max(1, |y|), is a relative bound
    x = torch.randn(SPEC_B, C, nlat, nlon, generator=g) * (3000.0 * (8.0 / C) ** 2)
    return cfg, {k: v.to(dtype) if v.is_floating_point() else v for k, v in p.items()}, x.to(dtype)


@functools.lru_cache(maxsize=None)
def _spec_ref(case, dtype):
    C, nlat, nlon, lmax = case
    _, p, x = _spec_inputs(case, dtype)
    sht, isht = sfno_ref.make_transforms(nlat, nlon, lmax, lmax + 1, dtype=dtype)
    ws = [p[f"filter_layer.filter.w.{i}"] for i in range(3)]
    with torch.no_grad():
        return sfno_ref.spectral_attention_s2(x, sht, isht, ws, p["filter_layer.filter.wout"]).double()


def _block(C, cfg, p, nlat, nlon, lmax, mmax, grid="equiangular"):
    from functools import partial

    from msfno_amd.harmonics import InverseRealSHT, RealSHT
    from msfno_amd.sfno import FourierNeuralOperatorBlock_Filmed
    sht = RealSHT(nlat, nlon, lmax=lmax, mmax=mmax, grid=grid).float()
    isht = InverseRealSHT(nlat, nlon, lmax=lmax, mmax=mmax, grid=grid).float()
    sht.weights = sht.weights * 1e5
    isht.pct = isht.pct / 1e5
    norm = partial(torch.nn.InstanceNorm2d, num_features=C, eps=1e-6, affine=True,
                   track_running_stats=False)
    blk = FourierNeuralOperatorBlock_Filmed(sht, isht, C, filter_type=cfg.filter_type,
                                            mlp_ratio=2.0, norm_layer=(norm, norm),
                                            inner_skip=cfg.inner_skip, outer_skip=cfg.outer_skip,
                                            mlp_mode="distributed", spectral_layers=3)
    blk.load_state_dict(p, strict=False)
    return blk.eval().to(DEV)


def _spec_gpu(case):
    C, nlat, nlon, lmax = case
    cfg, p, x = _spec_inputs(case)
    blk = _block(C, cfg, p, nlat, nlon, lmax, lmax + 1)
    xd = x.to(DEV)
    with torch.no_grad():
        return _thrice(lambda: blk.filter_layer(xd).cpu())


@functools.lru_cache(maxsize=None)
def _spec_child(bm64):
    """every spectral case in one child process: {id: (output, repeatable)}"""
    import tempfile
    env = dict(os.environ)
    env.pop("MSFNO_X3C_BM64", None)
    if bm64 is not None:
        env["MSFNO_X3C_BM64"] = bm64
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "spec.npz")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, cwd=HERE,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        z = np.load(out)
        same = json.loads(str(z["same"]))
        return {i: (torch.from_numpy(z[i]), same[i]) for i in SPEC_IDS}


@pytest.mark.parametrize("bm64", ["0", None], ids=["rows128_3stage", "rows64_2stage"])
@pytest.mark.parametrize("case", SPEC_CASES, ids=SPEC_IDS)
def test_spectral_chain(case, bm64):
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    cid = SPEC_IDS[SPEC_CASES.index(case)]
    got, same = _spec_child(bm64)[cid]
    assert same, f"{cid}: three runs on the same input differ"
    _bar(got, _spec_ref(case, torch.float64), _spec_ref(case, torch.float32), cid)


# ---- block MLP -----------------------------------------------------------------------

# P -> (nlat, nlon): Gauss-Legendre grids of P points, lmax = mmax = 2 (17 and 53 rows:
# the longitude FFT takes no prime factor above 13)
MLP_GRIDS = {4: (2, 2), 64: (4, 16), 68: (17, 4), 212: (53, 4)}
MLP_C = 256


def _mlp_block_inputs(P, B, resid, dtype=torch.float32):
    nlat, nlon = MLP_GRIDS[P]
    cfg = sfno_ref.BlockCfg(filter_type="non-linear", outer_skip="identity" if resid else None)
    p = sfno_ref.make_block_params(MLP_C, 2, 2, cfg, seed=17, randomize_affine=True)
    g = torch.Generator().manual_seed(1000 + P + B)
    x = torch.randn(B, MLP_C, nlat, nlon, generator=g)
    gamma = 0.2 * torch.randn(B, MLP_C, generator=g)
    beta = 0.2 * torch.randn(B, MLP_C, generator=g)
    p = {k: v.to(dtype) if v.is_floating_point() else v for k, v in p.items()}
    return cfg, p, x.to(dtype), gamma.to(dtype), beta.to(dtype)


def _mlp_block_ref(P, B, resid, dtype):
    nlat, nlon = MLP_GRIDS[P]
    cfg, p, x, gamma, beta = _mlp_block_inputs(P, B, resid, dtype)
    sht, isht = sfno_ref.make_transforms(nlat, nlon, 2, 2, grid="legendre-gauss", dtype=dtype)
    with torch.no_grad():
        return sfno_ref.block_forward(p, x, sht, isht, cfg, gamma, beta, 0.7).double()


@pytest.mark.parametrize("resid", [True, False], ids=["resid", "noresid"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("P", sorted(MLP_GRIDS))
def test_block_mlp(P, B, resid):
    nlat, nlon = MLP_GRIDS[P]
    cfg, p, x, gamma, beta = _mlp_block_inputs(P, B, resid)
    blk = _block(MLP_C, cfg, p, nlat, nlon, 2, 2, grid="legendre-gauss")
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    with torch.no_grad():
        got, same = _thrice(lambda: blk(xd, gd, bd, 0.7).cpu())
    assert same, "three runs on the same input differ"
    _bar(got, _mlp_block_ref(P, B, resid, torch.float64), _mlp_block_ref(P, B, resid, torch.float32),
         f"block P={P} B={B} resid={resid}")


# ---- inner skip ----------------------------------------------------------------------

def _inner_skip(B, P):
    """msfno_conv1x1 at C = 256 three times: (inputs x, w, b on the CPU, output, repeatable)"""
    from msfno_amd import _native as N
    C = MLP_C
    g = torch.Generator().manual_seed(P)
    x = torch.randn(B, C, P, generator=g)
    w = torch.randn(C, C, generator=g) / C ** 0.5
    b = 0.1 * torch.randn(C, generator=g)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    ws = torch.empty(N.lib().msfno_conv1x1_workspace_size(B, C, C), dtype=torch.uint8, device=DEV)

    def run():
        out = torch.empty(B, C, P, device=DEV)
        N.check(N.lib().msfno_conv1x1(wd.data_ptr(), bd.data_ptr(), xd.data_ptr(), out.data_ptr(),
                                      B, C, C, P, ws.data_ptr(), ws.numel(), N.stream_of(xd.device)),
                "conv1x1")
        return out.cpu()

    got, same = _thrice(run)
    return x, w, b, got, same


def _inner_skip_bar(x, w, b, got, what):
    want64 = torch.einsum("oi,bip->bop", w.double(), x.double()) + b.double()[None, :, None]
    want32 = torch.einsum("oi,bip->bop", w, x) + b[None, :, None]
    _bar(got, want64, want32, what)


@pytest.mark.parametrize("P", [212, 210], ids=["skip_hp_P212", "skip_h_P210"])
def test_inner_skip(P):
    x, w, b, got, same = _inner_skip(2, P)
    assert same, "three runs on the same input differ"
    _inner_skip_bar(x, w, b, got, f"conv1x1 P={P}")


def test_inner_skip_one_workgroup_many_tiles(monkeypatch):
    """skip_hp_kernel's loop over tiles: B = 3, P = 260 is nine 128-pixel tiles (128, 128, 4
    per field), and MSFNO_SKIP_GRID=0 (read on every call) makes launch_skip_h ask for
    max(1, 0) = 1 workgroup, which walks all nine: x of tiles 1..8 arrives through the ring,
    the scale tables are reloaded at two field boundaries, the last tile issues dummy groups.
    The one-tile kernel (MSFNO_SKIP_P=0, also read on every call) forms every output from the
    same products in the same order, and the two kernels agreed bit for bit on this input
    before they shared csrc/x3h_tile.h, so that is asserted too."""
    monkeypatch.setenv("MSFNO_SKIP_GRID", "0")
    x, w, b, got, same = _inner_skip(3, 260)
    assert same, "three runs on the same input differ"
    _inner_skip_bar(x, w, b, got, "conv1x1 B=3 P=260, one workgroup")
    monkeypatch.setenv("MSFNO_SKIP_P", "0")
    _, _, _, one_tile, same = _inner_skip(3, 260)
    assert same, "skip_h_kernel: three runs on the same input differ"
    assert torch.equal(got, one_tile), "skip_hp_kernel and skip_h_kernel differ"


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    import conftest  # noqa: F401  (puts the package on sys.path)
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    res = {i: _spec_gpu(c) for i, c in zip(SPEC_IDS, SPEC_CASES)}
    np.savez(sys.argv[1], same=json.dumps({i: s for i, (_, s) in res.items()}),
             **{i: y.numpy() for i, (y, _) in res.items()})
