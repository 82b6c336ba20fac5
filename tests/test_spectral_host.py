"""CPU-side checks of the spectral losses and the power spectrum (msfno_amd/losses.py,
msfno_amd/harmonics/spectrum.py, csrc/spectrum.hip): the committed fixtures
(tests/golden/spectral_loss/, written by make_golden_spectral_losses.py from the
reference's own functions in fp64) agree with the torch restatement
(tests/spectral_util.py), the fixture set is complete, the C-ABI additions are declared,
exported and bound, and the Python entry points refuse CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

import spectral_util as SU
from conftest import REPO

FIXTURES = SU.fixture_files()


@pytest.mark.parametrize("path", FIXTURES, ids=SU.fixture_id)
def test_restatement_regenerates_fixture(path):
    f = SU.load_fixture(path)
    p = f["prd"].clone().requires_grad_()
    v = SU.loss(f["fn"], SU.oracle_sht(f), p, f["tar"], f["relative"], f["squared"])
    v.backward()
    assert torch.isfinite(f["loss"]) and torch.isfinite(f["grad"]).all()
    assert abs(v.item() - f["loss"].item()) <= 1e-12 * abs(f["loss"].item())
    # relative per (b, c) slab: the channel scales span seven decades
    err = (p.grad - f["grad"]).abs().amax(dim=(-1, -2))
    ref = f["grad"].abs().amax(dim=(-1, -2))
    assert (ref > 0).all()
    assert (err <= 1e-12 * ref).all(), (err / ref).max().item()


def test_fixture_set_is_complete():
    """l2 and spectral: relative x squared; h1: squared only; at the five shapes."""
    seen, total = set(), 0
    for path in FIXTURES:
        f = SU.load_fixture(path)
        size = os.path.getsize(path)
        assert size <= 576 * 1000, path
        total += size
        assert f["loss"].dtype == torch.float64 and f["grad"].dtype == torch.float64
        assert f["grad"].shape == f["prd"].shape == f["tar"].shape
        B, C = f["prd"].shape[:2]
        seen.add(((B, C, f["nlat"], f["nlon"], f["lmax"], f["mmax"], f["grid"]), f["fn"],
                  f["relative"], f["squared"]))
    want = {(s, fn, rel, sq) for s in SU.SHAPES for fn, rel, sq in SU.VARIANTS}
    assert len(want) == 50 and seen == want and len(FIXTURES) == 50
    assert total <= 4 * 1000 * 1000


def test_spectrum_symbols_declared_exported_and_bound():
    from msfno_amd import _native as N
    hdr = open(os.path.join(REPO, "include", "msfno.h")).read()
    bound = {n for n, _, _ in N.SIGNATURES}
    for s in ("msfno_spectrum_power", "msfno_spectrum_power_backward"):
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(N.lib(), s), s
        assert s in bound, s
    assert N.lib().msfno_abi_version() == 6


def test_spectrum_entry_points_refuse_bad_arguments_before_any_launch():
    """MSFNO_EINVAL for null pointers, extents below 1 and coefficient pointers off the
    8-byte grid; checked on host pointers that no kernel may touch."""
    from msfno_amd import _native as N
    lib = N.lib()
    buf = (ctypes.c_double * 16)()
    p = ctypes.addressof(buf)
    assert p % 8 == 0
    assert lib.msfno_spectrum_power(None, p, 1, 2, 2, None) == N.MSFNO_EINVAL
    assert lib.msfno_spectrum_power(p, None, 1, 2, 2, None) == N.MSFNO_EINVAL
    for bad in ((0, 2, 2), (1, 0, 2), (1, 2, 0), (-1, 2, 2)):
        assert lib.msfno_spectrum_power(p, p, *bad, None) == N.MSFNO_EINVAL
        assert lib.msfno_spectrum_power_backward(p, p, p, *bad, None) == N.MSFNO_EINVAL
    # coefficient pointers off the 8-byte grid of a complex tensor
    assert lib.msfno_spectrum_power(p + 4, p, 1, 2, 2, None) == N.MSFNO_EINVAL
    assert lib.msfno_spectrum_power_backward(p + 4, p, p, 1, 2, 2, None) == N.MSFNO_EINVAL
    assert lib.msfno_spectrum_power_backward(p, p, p + 4, 1, 2, 2, None) == N.MSFNO_EINVAL
    assert lib.msfno_spectrum_power_backward(None, p, p, 1, 2, 2, None) == N.MSFNO_EINVAL
    assert lib.msfno_spectrum_power_backward(p, None, p, 1, 2, 2, None) == N.MSFNO_EINVAL
    assert lib.msfno_spectrum_power_backward(p, p, None, 1, 2, 2, None) == N.MSFNO_EINVAL


def test_python_entry_points_import_and_refuse_cpu_tensors():
    from msfno_amd import harmonics as H
    from msfno_amd import losses as L
    with pytest.raises(ValueError):
        H.power_spectrum(torch.zeros(2, 3, 4, dtype=torch.complex64))
    sht = H.RealSHT(5, 12, lmax=5, mmax=7)
    x = torch.zeros(1, 2, 5, 12)
    for fn in (L.spectral_l2loss_sphere, L.spectral_loss_sphere, L.h1loss_sphere):
        with pytest.raises(ValueError):
            fn(sht, x, x)
    with pytest.raises(NotImplementedError):
        L.h1loss_sphere(sht, x, x, relative=True)
