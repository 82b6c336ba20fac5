"""The Legendre kernels over depth, ragged tiles and dispatch edges (legendre_cases.py has
the cases, their fp64 references and the measures; test_legendre_cases_host.py the
conditions that give the bars their meaning).

Which kernel a case reaches follows csrc/plan.cpp:

* stand-alone RealSHT (msfno_sht_forward -> legendre_fwd): always legendre_x3_kernel, the
  tiled one, 128 rows x 64 columns, ceil(K / 32) k-tiles with K = Ke (even problems) or Ko
  (odd ones); x3f needs norm0's statistics and is never taken here.
* stand-alone InverseRealSHT (msfno_sht_inverse -> legendre_inv -> ensure_desc3):
  legendre_x3r_kernel when every problem has K <= X3R_KMAX degrees of one parity and
  N = Ke <= X3R_NMAX columns, body NK = ceil(K / 32), x3r_zero for K = 0; otherwise
  legendre_x3_kernel for all problems of the launch.
* a block with norm0 (run_spectral): forward legendre_x3f_kernel when x3f_usable, that is
  a symmetric table and Ke <= X3F_KMAX, body KS = ceil(K / 32) per problem; otherwise the
  tiled kernel on the fp32 slab.  The inverse as for the stand-alone transform.

Every stand-alone call goes through the C ABI with a workspace of exactly the size the
library asks for, filled with 0xFF bytes (NaN as floats and as fp16 pairs), a guard behind
it, and an output pre-filled with NaN: a pad that leaks, an element left unwritten or a
store past the workspace fails the case.

Measured on an MI355X (worst (m, parity) block of the forward result, worst Fourier column
of the inverse one, in units of 1e-7; bar 20, the fp32 restatement of the reference on the
same inputs reaches 7.7):

  dense, lmax 20, mmax 5, nlat 129 .. 769 (15 depths)   forward 1.6 .. 2.8   inverse 1.4 .. 2.2
  grid,  lmax 20, mmax 5, nlat 129, 449, 673            forward 1.9 .. 2.5   inverse 1.5 .. 2.0
  nlat 257, lmax 130, 200, 290, 384, 386 (mmax 3)       forward 1.5 .. 1.9   inverse 1.7 .. 3.0
  nlat 129, R = 2, 130, 258, 282; lmax 3 < mmax 5       forward 1.5 .. 2.6   inverse 1.5 .. 2.3
  nlat 449, all 17 orders, R = 150                      forward 2.1          inverse 3.2
  nlat 2047 / 2049 (lmax 8, mmax 3)                     forward 4.2 / 3.8    inverse 1.6 / 1.6

Block cases (max-abs error against the fp64 oracle / e32, the fp32 oracle's own distance;
bar 8): 0.73 .. 1.38 over all 31 cases, the largest at nlat 767 (x3f KS 12, non-linear);
non-linear 5.5e-7 .. 2.2e-6 absolute, linear 1.5e-6 .. 3.5e-6, the non-linear grid twin
2.5e-8.  MSFNO_X3F_NS=2 gives the same figures to every printed digit (the ring depth does
not change the order of the sums).  The forward refuses no channel count: C = 12 and 20
give R = 264 and 280, no multiples of 16.

Found by this sweep (every inverse case with an odd number of spectrum values, bc nlat mmax;
the column m = mmax - 1 was off by 0.78 of its maximum): the codelet inverse FFT
(fft_c2r_dma_kernel) stages the spectrum in 16-B chunks and clamped the last chunk so that
the last row's last bin was replaced by the bin two before it.  Fixed in csrc/fft.hip.
"""
import json
import os
import subprocess
import sys
from functools import partial

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":             # the MSFNO_X3F_NS=2 child: no conftest sets the path
    for _p in (HERE, os.path.dirname(HERE),
               os.path.join(os.path.dirname(HERE), "modulated-spherical-fourier-neural-operator_amd")):
        sys.path.insert(0, _p)

import legendre_cases as L  # noqa: E402
from workspace_guard import guard_intact as _guard_intact, guarded as _guarded  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- stand-alone transforms through the C ABI ---------------------------------------
def _module(cls, c):
    """The native transform of `c`: its own equiangular table ("grid"), or the dense
    symmetric one installed as test_asymmetric_table_uses_general_layout installs one."""
    from msfno_amd import harmonics as H
    mod = getattr(H, cls)(c.nlat, L.NLON, lmax=c.lmax, mmax=c.mmax, grid="equiangular").float()
    if c.kind == "dense":
        if cls == "RealSHT":
            mod.weights = L.table(c, False).float()
        else:
            mod.pct = L.table(c, True).float()
    return mod.to(DEV)


def _sht(mod, arg, fill=0xFF):
    """msfno_sht_forward / msfno_sht_inverse of `arg` on `mod`'s plan: workspace bytes
    `fill`, output pre-filled with NaN, guard checked."""
    from msfno_amd import _native as N
    inverse = mod._inverse
    plan = mod._plan(arg.device)
    lead = arg.shape[:-2]
    bc = 1
    for n in lead:
        bc *= n
    nbytes = N.lib().msfno_sht_workspace_size(plan.handle, bc)
    assert nbytes > 0
    ws = _guarded(nbytes, fill)
    if inverse:
        out = torch.full((*lead, mod.nlat, mod.nlon), float("nan"), device=DEV)
        fn = N.lib().msfno_sht_inverse
    else:
        out = torch.full((*lead, mod.lmax, mod.mmax, 2), float("nan"), device=DEV)
        fn = N.lib().msfno_sht_forward
    N.check(fn(plan.handle, arg.data_ptr(), out.data_ptr(), bc, ws.data_ptr(), nbytes,
               N.stream_of(arg.device)), "sht")
    _guard_intact(ws, nbytes)
    return out if inverse else torch.view_as_complex(out)


def _inverse_kernel(c):
    fits = L.nk(c.lmax) <= L.X3R_KMAX // 32 and L.ke(c.nlat) <= L.X3R_NMAX
    return f"x3r NK<={L.nk(c.lmax)} nch {-(-L.ke(c.nlat) // L.X3R_CHUNK)}" if fits else "tiled x3"


def _check_forward(c, got):
    want = L.forward_reference(c)
    assert got.shape == want.shape and got.dtype == torch.complex64
    assert torch.isfinite(torch.view_as_real(got)).all()
    err = L.forward_block_errors(got, want, c)
    worst = max(err, key=err.get)
    print(f"forward {L.case_id(c)} (tiled x3, {L.ks(L.ke(c.nlat))} k-tiles): worst block "
          f"(m, parity) = {worst} {err[worst]:.2e}")
    assert err[worst] < L.GPU_BAR, err
    # structural zeros l < m, and whole columns m >= lmax, are written, and exact
    l_lt_m = torch.arange(c.lmax)[:, None] < torch.arange(c.mmax)[None, :]
    assert (got[..., l_lt_m] == 0).all()


def _check_inverse(c, got):
    want = L.inverse_reference(c)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert torch.isfinite(got).all()
    col = L.inverse_column_errors(got, want, c)
    print(f"inverse {L.case_id(c)} ({_inverse_kernel(c)}): worst column "
          f"m = {col.argmax().item()} {col.max().item():.2e}")
    assert col.max().item() < L.GPU_BAR, col
    # the columns without a degree (m >= lmax) hold nothing
    rest = torch.fft.rfft(got.double(), norm="forward")[..., min(c.mmax, c.lmax):]
    assert rest.abs().max().item() < L.GPU_BAR * want.abs().max().item()


@pytest.mark.parametrize("case", L.CASES, ids=L.IDS)
def test_forward_matches_definition(case):
    """legendre_x3_kernel (every stand-alone forward): ceil(Ke / 32) = 3 .. 13, 33 k-tiles
    with a last one of 1 .. 32 latitudes, 1 .. 4 column tiles of 64 with a ragged last one
    (N = lpe = 8 .. 200), 1 .. 3 row tiles of 128 with 2 or 26 rows in the last."""
    got = _sht(_module("RealSHT", case), L.forward_input(case).to(DEV)).cpu()
    _check_forward(case, got)


@pytest.mark.parametrize("case", L.CASES, ids=L.IDS)
def test_inverse_matches_definition(case):
    """legendre_x3r_kernel, bodies NK 1 .. 6 and x3r_zero, column chunks nch = 3, 4, 5, ..
    32 with a last chunk of 1 .. 32 columns, 1 .. 3 row tiles; legendre_x3_kernel where
    K = 193 > X3R_KMAX (lmax 386) or N = 1025 > X3R_NMAX (nlat 2049)."""
    a = L.inverse_input(case)
    assert a[..., 0, 0].imag.abs().min() > 0
    got = _sht(_module("InverseRealSHT", case), a.to(DEV)).cpu()
    _check_inverse(case, got)


def test_sht_workspace_holds_anything_and_is_not_overrun():
    """The ragged case (Ke = 65, R = 130, lmax 3 < mmax 5) in both directions: the result on
    a workspace of 0xFF bytes is bit-identical to the one on a zero-filled workspace (both
    with a NaN-filled output and an intact guard; the parity is the sweep's)."""
    c = L.RAGGED
    for cls, arg in (("RealSHT", L.forward_input(c)), ("InverseRealSHT", L.inverse_input(c))):
        mod, arg = _module(cls, c), arg.to(DEV)
        dirty, clean = _sht(mod, arg, 0xFF), _sht(mod, arg, 0x00)
        if cls == "RealSHT":
            dirty, clean = torch.view_as_real(dirty), torch.view_as_real(clean)
        assert torch.isfinite(dirty).all()
        assert torch.equal(dirty.view(torch.int32), clean.view(torch.int32)), cls


# ---- the block's spectral path ---------------------------------------------------------
def _block(c):
    from msfno_amd.harmonics import InverseRealSHT, RealSHT
    from msfno_amd.sfno import FourierNeuralOperatorBlock_Filmed
    sht = RealSHT(c.nlat, L.NLON, lmax=c.lmax, mmax=c.mmax, grid="equiangular").float()
    isht = InverseRealSHT(c.nlat, L.NLON, lmax=c.lmax, mmax=c.mmax, grid="equiangular").float()
    if c.kind == "dense":
        sht.weights = L.table(c, False).float()
        isht.pct = L.table(c, True).float()
    norm = partial(torch.nn.InstanceNorm2d, num_features=c.C, eps=1e-6, affine=True,
                   track_running_stats=False)
    blk = FourierNeuralOperatorBlock_Filmed(sht, isht, c.C, filter_type=c.filter, mlp_ratio=2.0,
                                            norm_layer=(norm, norm), inner_skip=None,
                                            outer_skip=None, mlp_mode="none", spectral_layers=3)
    missing, unexpected = blk.load_state_dict(L.block_params(c), strict=False)
    assert not unexpected, unexpected
    assert all(k.endswith((".weights", ".pct")) for k in missing), missing
    assert not hasattr(blk, "inner_skip") and not hasattr(blk, "mlp")
    return blk.eval().to(DEV)


def _forward_kernel(c):
    if L.ke(c.nlat) > L.X3F_KMAX:
        return "tiled x3"
    R = 2 * c.B * c.C
    tiles = -(-R // L.X3F_RB)
    last = R - (tiles - 1) * L.X3F_RB
    return (f"x3f KS {L.ks(L.ke(c.nlat))}/{L.ks(L.ko(c.nlat))} R {R}: {tiles} row tiles, the "
            f"last of {last / L.X3F_CHUNK:g} chunks")


def _block_error(c):
    """(max-abs error of blk.global_conv(x, x) against the fp64 oracle, the case's bar)."""
    x = L.block_input(c).to(DEV)
    with torch.no_grad():
        got = _block(c).global_conv(x, x).cpu()
    want = L.block_reference(c)
    assert got.shape == want.shape and torch.isfinite(got).all()
    return (got.double() - want).abs().max().item(), L.block_bar(c)


@pytest.mark.parametrize("case", L.BLOCK_CASES, ids=L.BLOCK_IDS)
def test_block_spectral_path_matches_oracle(case):
    """norm0 -> filter -> (GELU) -> norm1 of a block without skips and MLP.  Forward:
    legendre_x3f_kernel, bodies KS 2 .. 12 (even and odd problems of an odd nlat differ),
    1 .. 3 row tiles of X3F_RB, 1 .. 16 chunks of 16 rows with a half-empty last one, 1 .. 4
    column tiles; legendre_x3_kernel at nlat 769.  Inverse: legendre_x3r_kernel, NK 1 .. 6,
    legendre_x3_kernel at lmax 386."""
    err, bar = _block_error(case)
    e32 = L.block_e32(case)
    print(f"block {L.block_id(case)} ({_forward_kernel(case)}): max-abs {err:.2e} = "
          f"{err / e32:.2f} e32, bar {bar:.2e}")
    assert err <= bar, (err, bar, err / e32)


def _global_conv_abi(blk, x, fill):
    from msfno_amd import _native as N
    fwd, inv = blk._transforms()
    pf, pi = fwd._plan(x.device), inv._plan(x.device)
    d, keep = blk.native_desc()        # no prepared-weight cache: the images live in ws
    B = x.shape[0]
    nbytes = N.lib().msfno_block_workspace_size(d, pf.handle, pi.handle, B)
    assert nbytes > 0
    ws = _guarded(nbytes, fill)
    out = torch.full((B, blk.embed_dim_sfno, inv.nlat, inv.nlon), float("nan"), device=DEV)
    N.check(N.lib().msfno_block_global_conv(d, pf.handle, pi.handle, x.data_ptr(), x.data_ptr(),
                                            out.data_ptr(), B, ws.data_ptr(), nbytes,
                                            N.stream_of(x.device)), "global_conv")
    _guard_intact(ws, nbytes)
    del keep
    return out


@pytest.mark.parametrize("case", L.BLOCK_RAGGED, ids=L.block_id)
def test_block_workspace_holds_anything_and_is_not_overrun(case):
    """msfno_block_global_conv at Ke = 65, R = 264 / 280 and lmax 4 < mmax 5: on a workspace
    of 0xFF bytes the result is finite, within the block bar, and bit-identical to the one on
    a zero-filled workspace; the guard behind the workspace is untouched."""
    blk, x = _block(case), L.block_input(case).to(DEV)
    dirty, clean = _global_conv_abi(blk, x, 0xFF), _global_conv_abi(blk, x, 0x00)
    assert torch.isfinite(dirty).all()
    err = (dirty.cpu().double() - L.block_reference(case)).abs().max().item()
    bar = L.block_bar(case)
    print(f"block ABI {L.block_id(case)}: max-abs {err:.2e} bar {bar:.2e}")
    assert err <= bar, (err, bar)
    assert torch.equal(dirty.view(torch.int32), clean.view(torch.int32))


# ---- MSFNO_X3F_NS=2: the two-stage ring, read once per process --------------------------
def _variant_errors():
    return {L.block_id(c): _block_error(c) for c in L.BLOCK_VARIANT_CASES}


def test_x3f_two_stage_ring_on_every_depth_and_row_count():
    """legendre_x3f_kernel<2> (MSFNO_X3F_NS=2: chunk j + 1 is issued into the stage chunk
    j - 1 just left) on the depth and row cases, in one child process; same bar."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)],
                       env=dict(os.environ, MSFNO_X3F_NS="2"), cwd=HERE, capture_output=True,
                       text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-2000:]
    errs = json.loads(r.stdout.strip().splitlines()[-1])
    assert sorted(errs) == sorted(L.block_id(c) for c in L.BLOCK_VARIANT_CASES)
    for k, (err, bar) in errs.items():
        print(f"NS=2 {k}: max-abs {err:.2e} bar {bar:.2e}")
    bad = {k: v for k, v in errs.items() if not v[0] <= v[1]}
    assert not bad, bad


if __name__ == "__main__":
    print(json.dumps(_variant_errors()))
