"""The longitude FFT on grid widths without a compiled codelet (csrc/fft.hip GenericFFT:
stockham_pass_pp, radices 4, 2, 3, 5, 7, 11, 13, under fft_r2c_rows_kernel /
fft_c2r_rows_kernel), against the fp64 references of fft_size_cases.py, in both directions
and for both references; the widths the fallback must refuse; the inverse Legendre
dispatch boundary K = X3R_KMAX on such a grid; the block, plain and latitude-band sharded,
on such grids; and two more adjoint plans.

Metric of the parity tests (fft_size_cases.column_errors): over m < mmax, the maximum over
column m of |got - want| divided by the maximum over column m of |want|, plus the global
measure of test_gpu_parity.py.  Bar: 2e-6 per column, the transform bar of
test_gpu_parity.py; test_fft_sizes_host.py shows that an exact fp32 implementation stays
under a quarter of it on the same inputs.

Measured on an MI355X, worst per-column error in units of 1e-7, with the fp32 restatement's
error on the same inputs in parentheses.  No size needed a bar taken from the restatement:
the worst, 8.3e-7 (inverse, 13 x 13), is 2.4 times under 2e-6; the two-pass prime sizes
(11 x 11, 13 x 13) and the four-pass 1820 run at up to 2.9 times the restatement, as the
Horner butterflies' R - 1 chained complex products per output would have it.

  nlon mmax |  forward grid     forward dense  |  inverse grid     inverse dense
    14    8 |   2.3 (2.0)       2.8 (2.1)     |   2.2 (1.4)       2.6 (1.3)
    22   12 |   2.7 (2.0)       2.9 (1.9)     |   3.0 (2.6)       2.8 (1.6)
    28   15 |   2.9 (2.0)       2.3 (2.3)     |   2.7 (1.6)       2.4 (1.6)
    63   32 |   3.6 (2.6)       3.2 (2.1)     |   2.3 (2.8)       2.8 (1.8)
    98   50 |   4.3 (2.2)       3.4 (2.2)     |   3.7 (2.3)       3.3 (2.1)
   242  122 |   4.7 (2.5)       4.1 (2.8)     |   5.4 (2.8)       5.1 (2.9)
   338  170 |   6.8 (3.1)       6.0 (2.5)     |   8.3 (2.9)       5.6 (2.5)
   308  155 |   4.4 (2.5)       4.6 (3.4)     |   5.3 (3.1)       3.7 (2.2)
   364  183 |   5.0 (3.6)       5.0 (2.7)     |   6.1 (3.4)       4.3 (2.2)
   256  129 |   4.7 (4.0)       3.4 (2.4)     |   3.4 (3.4)       3.0 (2.4)
   720  361 |   4.3 (4.1)       3.2 (2.7)     |   4.2 (3.7)       3.7 (2.7)
   770  386 |   5.2 (3.5)       4.7 (3.0)     |   5.7 (3.3)       4.4 (2.6)
   891  446 |   5.4 (4.1)       4.5 (3.0)     |   4.3 (3.9)       3.9 (2.7)
  1820  911 |   6.5 (4.0)       5.4 (3.6)     |   7.4 (3.8)       6.0 (3.1)
   308   52 |   3.6 (2.4)       4.1 (2.4)     |   4.0 (1.8)       3.1 (1.4)
    63   11 |   2.1 (2.1)       1.9 (3.0)     |   2.4 (1.4)       1.9 (1.2)

Other figures of the same run: Legendre boundary 9 x 770, global error 2.2e-7 .. 3.8e-7;
block max-abs 2.4e-7 (|y| <= 4.6), its global_conv 1.2e-6 .. 1.4e-6 (|z| <= 5.4); sharded
against unsharded 6.0e-8; adjoint plans 1.3e-7 .. 2.2e-7.

What the tests catch, tried on scratch builds of fft.hip (each against this whole file):
the `case 7` arm of GenericFFT::run not running its radix-7 pass (56 tests fail), the
prime butterfly's root not conjugated under INV (42), stockham_pass_pp striding its
butterflies by 128 lanes instead of 64 (33), the inverse's `k2 == H` Nyquist clause
removed (25: every even width with mmax = nlon / 2 + 1 and the 386, 386 boundary case).
"""
from functools import partial

import pytest
import torch

import fft_size_cases as F
from oracle import sfno_ref
from oracle import sht_ref as S
from test_gpu_sht_autograd import _err, _forward_problem, _inverse_problem, _mine

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _module(cls, case, kind):
    """The native transform of `case`; for the dense reference with the synthetic table in
    place of its own, as test_asymmetric_table_uses_general_layout installs one."""
    from msfno_amd import harmonics as H
    mod = getattr(H, cls)(case.nlat, case.nlon, lmax=case.mmax, mmax=case.mmax,
                          grid="equiangular").float()
    if kind == "dense":
        if cls == "RealSHT":
            mod.weights = F.dense_table(case, False).float()
        else:
            mod.pct = F.dense_table(case, True).float()
    return mod.to(DEV)


@pytest.mark.parametrize("kind", F.KINDS)
@pytest.mark.parametrize("case", F.CASES, ids=F.IDS)
def test_forward_matches_reference(case, kind):
    want = F.forward_reference(case, kind)
    got = _module("RealSHT", case, kind)(F.forward_input(case).to(DEV)).cpu()
    assert got.shape == want.shape and got.dtype == torch.complex64
    col = F.column_errors(got, want, case, False).max().item()
    tot = F.rel(got.to(torch.complex128), want)
    ref = F.column_errors(F.fp32_forward(case, kind), want, case, False).max().item()
    print(f"forward {kind} nlon {case.nlon} mmax {case.mmax}: per-column {col:.2e} "
          f"overall {tot:.2e} (fp32 restatement per-column {ref:.2e})")
    assert col < F.GPU_BAR and tot < F.GPU_BAR, (col, tot)
    # structural zeros l < m are exact
    l = torch.arange(case.mmax)[:, None]
    m = torch.arange(case.mmax)[None, :]
    assert (got[..., l < m] == 0).all()


@pytest.mark.parametrize("kind", F.KINDS)
@pytest.mark.parametrize("case", F.CASES, ids=F.IDS)
def test_inverse_matches_reference(case, kind):
    want = F.inverse_reference(case, kind)
    a = F.inverse_input(case, kind)
    nyq = case.nlon // 2 if case.nlon % 2 == 0 and case.mmax > case.nlon // 2 else 0
    assert a[..., 0, 0].imag.abs().min() > 0 and a[..., nyq, nyq].imag.abs().min() > 0
    got = _module("InverseRealSHT", case, kind)(a.to(DEV)).cpu()
    assert got.shape == want.shape and got.dtype == torch.float32
    col = F.column_errors(got, want, case, True).max().item()
    tot = F.rel(got.double(), want)
    ref = F.column_errors(F.fp32_inverse(case, kind), want, case, True).max().item()
    print(f"inverse {kind} nlon {case.nlon} mmax {case.mmax}: per-column {col:.2e} "
          f"overall {tot:.2e} (fp32 restatement per-column {ref:.2e})")
    assert col < F.GPU_BAR and tot < F.GPU_BAR, (col, tot)


# ---- refusals ----------------------------------------------------------------------
def _small_transform_still_works():
    nlat, nlon = 7, 28
    from msfno_amd.harmonics import InverseRealSHT, RealSHT
    g = torch.Generator().manual_seed(nlon)
    x = torch.randn(2, nlat, nlon, generator=g)
    want = S.RealSHT(nlat, nlon)(x.double())
    got = RealSHT(nlat, nlon).float().to(DEV)(x.to(DEV)).cpu()
    assert F.rel(got.to(torch.complex128), want) < F.GPU_BAR
    a = torch.view_as_complex(torch.randn(2, nlat, nlon // 2 + 1, 2, generator=g))
    want = S.InverseRealSHT(nlat, nlon)(a.to(torch.complex128))
    got = InverseRealSHT(nlat, nlon).float().to(DEV)(a.to(DEV)).cpu()
    assert F.rel(got.double(), want) < F.GPU_BAR


# 34 = 2.17 and 1822 = 2.911: a prime factor above 13.  1001 = 7.11.13 (odd: H = 1001,
# 72072 B of LDS) and 1848 (H = 924 = 4.3.7.11, 66528 B): over the fallback's 64 KiB.
@pytest.mark.parametrize("nlon", [34, 1822, 1001, 1848])
@pytest.mark.parametrize("cls", ["RealSHT", "InverseRealSHT"])
def test_unsupported_width_is_refused(cls, nlon):
    """NotImplementedError no later than the first call, from a check on the host (plan
    creation for the prime factor, the launcher's LDS check for the size: no FFT kernel is
    launched), and the device is as usable afterwards as before."""
    from msfno_amd import harmonics as H
    nlat, lmax, mmax = 7, 7, nlon // 2 + 1
    g = torch.Generator().manual_seed(nlon)
    if cls == "RealSHT":
        arg = torch.randn(2, nlat, nlon, generator=g)
    else:
        arg = torch.view_as_complex(torch.randn(2, lmax, mmax, 2, generator=g))
    with pytest.raises(NotImplementedError):
        mod = getattr(H, cls)(nlat, nlon, lmax=lmax, mmax=mmax, grid="equiangular").float()
        mod.to(DEV)(arg.to(DEV))
    torch.cuda.synchronize()
    _small_transform_still_works()
    torch.cuda.synchronize()


# ---- Legendre dispatch boundary on a generic grid -------------------------------------
# equiangular 9 x 770 (H = 385): lmax 384 folds to K = 192 = X3R_KMAX degrees per parity,
# the register-resident inverse kernel; lmax 386 to K = 193, the tiled one
@pytest.mark.parametrize("lmax,mmax", [(384, 385), (386, 386)])
def test_legendre_dispatch_boundary(lmax, mmax):
    from msfno_amd.harmonics import InverseRealSHT, RealSHT
    nlat, nlon = 9, 770
    g = torch.Generator().manual_seed(lmax)
    a = torch.view_as_complex(torch.randn(*F.LEAD, lmax, mmax, 2, generator=g))
    want = S.InverseRealSHT(nlat, nlon, lmax=lmax, mmax=mmax)(a.to(torch.complex128))
    got = InverseRealSHT(nlat, nlon, lmax=lmax, mmax=mmax).float().to(DEV)(a.to(DEV)).cpu()
    e = F.rel(got.double(), want)
    print(f"inverse 9x770 lmax {lmax} mmax {mmax}: {e:.2e}")
    assert e < F.GPU_BAR
    x = torch.randn(*F.LEAD, nlat, nlon, generator=g)
    want = S.RealSHT(nlat, nlon, lmax=lmax, mmax=mmax)(x.double())
    got = RealSHT(nlat, nlon, lmax=lmax, mmax=mmax).float().to(DEV)(x.to(DEV)).cpu()
    e = F.rel(got.to(torch.complex128), want)
    print(f"forward 9x770 lmax {lmax} mmax {mmax}: {e:.2e}")
    assert e < F.GPU_BAR
    ll = torch.arange(lmax)[:, None]
    mm = torch.arange(mmax)[None, :]
    assert (got[..., ll < mm] == 0).all()


# ---- the block on non-codelet grids ---------------------------------------------------
# row statistics inside the generic forward FFT (norm0) and skip add (+ GELU for the
# linear filter) + row statistics inside the generic inverse FFT.
# (filter, nlat, nlon, B); lmax = nlat, mmax = lmax + 1.  15 x 63: odd nlon, a pixel count
# that is no multiple of 4
C = 8
BLOCK_CASES = [("non-linear", 19, 308, 2), ("linear", 15, 63, 1), ("non-linear", 23, 720, 1)]


def _block_case(filter_type, nlat, nlon, B, seed=11):
    cfg = sfno_ref.BlockCfg(filter_type=filter_type, inner_skip="linear", outer_skip="identity",
                            has_mlp=True, spectral_layers=3)
    p = sfno_ref.make_block_params(C, nlat, nlat + 1, cfg, seed=seed, randomize_affine=True)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, C, nlat, nlon, generator=g)
    gamma = 0.2 * torch.randn(B, C, generator=g)
    beta = 0.2 * torch.randn(B, C, generator=g)
    return cfg, p, x, gamma, beta


def _block(cfg, p, nlat, nlon):
    from msfno_amd.harmonics import InverseRealSHT, RealSHT
    from msfno_amd.sfno import FourierNeuralOperatorBlock_Filmed
    sht = RealSHT(nlat, nlon, lmax=nlat, mmax=nlat + 1, grid="equiangular").float()
    isht = InverseRealSHT(nlat, nlon, lmax=nlat, mmax=nlat + 1, grid="equiangular").float()
    sht.weights = sht.weights * 1e5
    isht.pct = isht.pct / 1e5
    norm = partial(torch.nn.InstanceNorm2d, num_features=C, eps=1e-6, affine=True,
                   track_running_stats=False)
    blk = FourierNeuralOperatorBlock_Filmed(sht, isht, C, filter_type=cfg.filter_type,
                                            mlp_ratio=2.0, norm_layer=(norm, norm),
                                            inner_skip="linear", outer_skip="identity",
                                            mlp_mode="distributed", spectral_layers=3)
    blk.load_state_dict(p, strict=False)
    return blk.eval().to(DEV)


@pytest.mark.parametrize("case", BLOCK_CASES, ids=lambda c: f"{c[0]}_{c[1]}x{c[2]}_B{c[3]}")
def test_block_on_generic_grid_matches_oracle(case):
    filter_type, nlat, nlon, B = case
    cfg, p, x, gamma, beta = _block_case(*case)
    blk = _block(cfg, p, nlat, nlon)
    with torch.no_grad():
        y = blk(x.to(DEV), gamma.to(DEV), beta.to(DEV), 0.7).cpu()
        sht, isht = sfno_ref.make_transforms(nlat, nlon, nlat, nlat + 1)
        want = sfno_ref.block_forward(p, x, sht, isht, cfg, gamma, beta, 0.7)
        # the block up to norm1 as well: the outer identity skip and the small MLP weights
        # leave the FFT-derived statistics little weight in y itself
        z = blk.global_conv(x.to(DEV), x.to(DEV)).cpu()
        want_z = sfno_ref.global_conv(p, x, x, sht, isht, cfg)
    err = (y - want).abs().max().item()
    err_z = (z - want_z).abs().max().item()
    print(f"{case}: max-abs {err:.3e} |y|max {want.abs().max():.3f}; "
          f"global_conv max-abs {err_z:.3e} |z|max {want_z.abs().max():.3f}")
    assert err < 1e-4 * max(1.0, want.abs().max().item())
    assert err_z < 1e-4 * max(1.0, want_z.abs().max().item())


def test_sharded_block_on_generic_grid_matches_unsharded():
    from msfno_amd.sfno import LatBandBlock, LocalGroup
    case, world = BLOCK_CASES[0], 2
    cfg, p, x, gamma, beta = _block_case(*case)
    blk = _block(cfg, p, case[1], case[2])
    x, gamma, beta = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    with torch.no_grad():
        y1 = blk(x, gamma, beta, 0.7)
        shards = [LatBandBlock(blk, r, world) for r in range(world)]
        gens = [s.stages(s.take(x), gamma, beta, 0.7) for s in shards]
        y = LatBandBlock.assemble(shards, LocalGroup.run(gens))
    err = (y - y1).abs().max().item()
    print(f"sharded {case}: max-abs vs unsharded {err:.3e}")
    assert err < 2e-5


# ---- adjoint plans on generic grids ---------------------------------------------------
# 9 x 28 with mmax 15: the Nyquist column takes the factor-1 branch of adjoint_table
ADJOINT_CASES = [("equiangular", 9, 28, 9, 15), ("equiangular", 9, 63, 9, 10)]
ADJOINT_IDS = ["-".join(map(str, c)) for c in ADJOINT_CASES]


@pytest.mark.parametrize("case", ADJOINT_CASES, ids=ADJOINT_IDS)
def test_forward_transform_backward_on_generic_grid(case):
    x, g, want = _forward_problem(case)
    xg = x.to(DEV).requires_grad_()
    _mine("RealSHT", case)(xg).backward(g.to(DEV))
    e = _err(xg.grad.cpu().double(), want)
    print(f"RealSHT backward {case}: {e:.3e}")
    assert e <= 2e-6, e


@pytest.mark.parametrize("case", ADJOINT_CASES, ids=ADJOINT_IDS)
def test_inverse_transform_backward_on_generic_grid(case):
    a, g, want = _inverse_problem(case)
    ag = a.to(DEV).requires_grad_()
    _mine("InverseRealSHT", case)(ag).backward(g.to(DEV))
    e = _err(ag.grad.cpu().to(torch.complex128), want)
    print(f"InverseRealSHT backward {case}: {e:.3e}")
    assert e <= 2e-6, e
