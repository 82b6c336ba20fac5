"""CPU-side checks of the sphere-weighted losses (msfno_amd/losses.py, csrc/loss.hip):
the committed fixtures (tests/golden/loss/, written by make_golden_losses.py from the
reference's own classes in fp64) agree with the torch restatement (tests/loss_util.py),
the host weight vectors agree with the reference's, and the C-ABI additions are declared,
exported and bound."""
import os
import re

import numpy as np
import pytest
import torch

import loss_util as LU
from conftest import REPO

FIXTURES = LU.fixture_files()
SHAPES = ("2x3x5x12", "2x5x33x64")


def _cases():
    out = []
    for path in FIXTURES:
        prd, tar, cases = LU.load_fixture(path)
        for c in cases:
            out.append(pytest.param(path, c, id=f"{os.path.basename(path)[:-4]}-{c['reduction']}"))
    return out


def test_fixture_set_is_complete():
    """Three classes, relative x squared for the L2 pair, two reductions, two shapes."""
    seen = set()
    for path in FIXTURES:
        prd, tar, cases = LU.load_fixture(path)
        assert os.path.getsize(path) <= 576 * 1000
        # the inputs are fp32 values
        assert torch.equal(prd, prd.float().double()) and torch.equal(tar, tar.float().double())
        for c in cases:
            seen.add(("x".join(map(str, prd.shape)), c["cls"], c["relative"], c["squared"],
                      c["reduction"]))
    want = set()
    for s in SHAPES:
        for red in ("mean", "sum"):
            want.add((s, "CosineMSELoss", False, False, red))
            for cls in ("L2Sphere", "L2Sphere_noSine"):
                for rel in (True, False):
                    for sq in (True, False):
                        want.add((s, cls, rel, sq, red))
    assert seen == want


@pytest.mark.parametrize("path,c", _cases())
def test_restatement_regenerates_fixture(path, c):
    prd, tar, _ = LU.load_fixture(path)
    v, g = LU.loss_and_grad(c["cls"], prd, tar, c["reduction"], c["relative"], c["squared"],
                            c["eps"] or 1e-4)
    assert abs(v.item() - c["loss"].item()) <= 1e-12 * abs(c["loss"].item())
    # relative per (b, c) slab: the channel scales span seven decades
    err = (g - c["grad"]).abs().amax(dim=(-1, -2))
    ref = c["grad"].abs().amax(dim=(-1, -2))
    assert (err <= 1e-12 * ref).all(), (err / ref).max().item()


@pytest.mark.parametrize("path,c", _cases())
def test_sphere_weights_match_reference(path, c):
    from msfno_amd.losses import sphere_weights
    H = c["w"].numel()
    w = sphere_weights(LU.KIND_OF[c["cls"]], H, c["eps"] or 1e-4)
    assert w.dtype == np.float64 and w.shape == (H,)
    assert np.abs(w - c["w"].numpy()).max() < 1e-13
    assert (LU.weights(LU.KIND_OF[c["cls"]], H, c["eps"] or 1e-4) - c["w"]).abs().max() < 1e-13


def test_sphere_weights_uniform_and_unknown():
    from msfno_amd.losses import sphere_weights
    assert np.array_equal(sphere_weights("uniform", 7), np.ones(7))
    with pytest.raises(ValueError):
        sphere_weights("lobatto", 7)


def test_loss_workspace_size_positive_and_monotone():
    from msfno_amd import _native as N
    f = N.lib().msfno_loss_workspace_size
    base = (73, 721, 1440)
    assert f(*base) > 0 and f(1, 1, 1) > 0
    for axis in range(3):
        prev = 0
        for v in (1, 2, 3, 7, 28, 29, 64, 65, 73, 128, 721, 1024, 1025, 2047, 2048, 2049, 5000):
            a = list(base)
            a[axis] = v
            cur = f(*a)
            assert cur > 0 and cur >= prev, (axis, v, cur, prev)
            prev = cur
    assert f(0, 721, 1440) == 0 and f(73, -1, 1440) == 0


def test_loss_entry_points_refuse_bad_arguments_before_any_launch():
    """MSFNO_EINVAL for null pointers / non-positive sizes, MSFNO_EWORKSPACE for a short
    workspace; checked on host pointers that no kernel may touch."""
    import ctypes
    from msfno_amd import _native as N
    lib = N.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    assert lib.msfno_loss_sums(None, p, p, p, 1, 2, 2, p, 1 << 20, None) == N.MSFNO_EINVAL
    assert lib.msfno_loss_sums(p, p, p, p, 0, 2, 2, p, 1 << 20, None) == N.MSFNO_EINVAL
    assert lib.msfno_loss_sums(p, p, p, p, 1, 2, 2, None, 1 << 20, None) == N.MSFNO_EINVAL
    assert lib.msfno_loss_sums(p, p, p, p, 1, 2, 2, p, 8, None) == N.MSFNO_EWORKSPACE
    assert lib.msfno_loss_backward(p, p, p, None, p, 1, 2, 2, None) == N.MSFNO_EINVAL
    assert lib.msfno_loss_backward(p, p, p, p, p, 1, 2, -3, None) == N.MSFNO_EINVAL


def test_loss_symbols_declared_exported_and_bound():
    from msfno_amd import _native as N
    hdr = open(os.path.join(REPO, "include", "msfno.h")).read()
    bound = {n for n, _, _ in N.SIGNATURES}
    for s in ("msfno_loss_workspace_size", "msfno_loss_sums", "msfno_loss_backward"):
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(N.lib(), s), s
        assert s in bound, s
    assert N.lib().msfno_abi_version() == 6


def test_reduction_none_and_target_gradient_are_refused():
    from msfno_amd import losses as L
    for cls in (L.L2Sphere, L.L2Sphere_noSine, L.CosineMSELoss):
        with pytest.raises(NotImplementedError):
            cls(reduction="none")
    with pytest.raises(ValueError):
        L.L2Sphere_noSine(relative=True, squared=True, reduction="mean")(
            torch.zeros(1, 1, 4, 8), torch.zeros(1, 1, 4, 8))
    with pytest.raises(NotImplementedError):
        L.weighted_sums(torch.zeros(1, 1, 4, 8), torch.zeros(1, 1, 4, 8, requires_grad=True),
                        torch.ones(4))


def test_constructor_defaults_match_reference():
    from msfno_amd import losses as L
    for cls in (L.L2Sphere, L.L2Sphere_noSine):
        m = cls()
        assert (m.relative, m.squared, m.reduction) == (True, False, "sum")
        cls(relative=False, squared=True, reduction="mean", dampening=0.5)  # ignored argument
    m = L.CosineMSELoss()
    assert (m.reduction, m.eps) == ("mean", 1e-4)
