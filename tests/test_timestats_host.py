"""Host-side checks of the statistics over time (msfno_amd/timestats.py): the error bounds
of tests/timestats_util.py hold for the recurrence in fp32 on the CPU on every input family
the GPU tests use (so the bounds themselves do not fail) and catch the naive sum-of-squares
form; the hour-of-year bins follow the reference's rule; and wrong arguments raise before any
native call."""
import datetime as dt

import numpy as np
import pytest
import torch

import timestats_util as TU


def _t(x):
    return torch.from_numpy(np.asarray(x))


@pytest.mark.parametrize("family", TU.FAMILIES)
@pytest.mark.parametrize("shape,updates", TU.CASES + [((1, 2, 3, 2731), 500)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fp32_recurrence_is_inside_the_bounds(shape, updates, family):
    p, t, c = (TU.flat(x) for x in TU.problem(shape, updates, family))
    # FIELD without and with a climatology
    for name, a32, a64 in (("field", t, t.double()), ("field-clim", t - c, t.double() - c.double())):
        n, mean, m2, lo, hi = TU.field32(a32.numpy())
        TU.check_moments(_t(n), _t(mean), _t(m2), a64, None, name)
        assert np.array_equal(lo, a32.numpy().min(0)) and np.array_equal(hi, a32.numpy().max(0))
    # ERROR with a climatology
    n, q = TU.error32(p.numpy(), t.numpy(), c.numpy())
    p64, t64, c64 = p.double(), t.double(), c.double()
    TU.check_moments(_t(n), _t(q[0]), _t(q[1]), p64 - t64, None, "error d")
    TU.assert_within(_t(q[2]), (p64 - t64).abs().mean(0),
                     TU.mean_bound(_t(n), TU.amax(p64 - t64)), "error mean_abs")
    TU.check_moments(_t(n), _t(q[3]), _t(q[4]), p64 - c64, None, "error pa")
    TU.check_moments(_t(n), _t(q[5]), _t(q[6]), t64 - c64, None, "error ta")
    TU.check_cov(_t(q[7]), p64 - c64, t64 - c64, None, "error")


def test_fp32_recurrence_with_missing_updates_is_inside_the_bounds():
    p, t, c = (TU.flat(x) for x in TU.problem((2, 3, 5, 7), 3, "300"))
    g = torch.Generator().manual_seed(5)
    valid = torch.rand(t.shape, generator=g) > 0.3
    valid[:, 0, 0, 0] = False                       # a pixel that never counts
    n, mean, m2, _, _ = TU.field32(t.numpy(), valid.numpy())
    TU.check_moments(_t(n), _t(mean), _t(m2), t.double(), valid, "field")
    assert n[0, 0, 0] == 0 and mean[0, 0, 0] == 0 and m2[0, 0, 0] == 0


@pytest.mark.parametrize("n", [2, 7, 64, 500])
def test_naive_sum_of_squares_breaks_the_variance_bound_at_300(n):
    g = torch.Generator().manual_seed(n)
    a = (300.0 + torch.randn(n, 4099, generator=g)).float()
    cnt, _, var64 = TU.moments64(a)
    bound = TU.var_bound(cnt, TU.amax(a), var64)
    naive = _t(TU.naive_var32(a.numpy())).double()
    _, _, m2, _, _ = TU.field32(a.numpy())
    assert ((_t(m2).double() / n - var64).abs() <= bound).all()
    broken = ((naive - var64).abs() > bound).double().mean().item()
    assert broken > 0.5, f"the naive form broke the bound on only {broken:.0%} of the pixels"


def test_hour_of_year_bin_follows_the_reference_rule():
    from msfno_amd.timestats import Climatology, hour_of_year_bin
    assert Climatology.hour_of_year_bin is hour_of_year_bin
    step = dt.timedelta(hours=6)
    for year, nsteps in ((2019, 1460), (2020, 1464)):
        t0 = dt.datetime(year, 1, 1)
        bins = [hour_of_year_bin(t0 + k * step) for k in range(nsteps)]
        kept = [b for b in bins if b is not None]
        assert kept == list(range(1460)), year
        none = [k for k, b in enumerate(bins) if b is None]
        assert none == ([] if year == 2019 else [236, 237, 238, 239])
        assert hour_of_year_bin(dt.datetime(year, 3, 1, 0)) == 236
        assert hour_of_year_bin(dt.datetime(year, 12, 31, 18)) == 1459
    assert hour_of_year_bin(dt.datetime(1900, 3, 1)) == 236      # not a leap year
    assert hour_of_year_bin(dt.datetime(2000, 2, 29, 12)) is None
    assert hour_of_year_bin(dt.datetime(2021, 1, 2, 12), step_hours=12) == 3
    with pytest.raises(ValueError):
        hour_of_year_bin(dt.datetime(2021, 1, 1, 3))
    with pytest.raises(ValueError):
        hour_of_year_bin(dt.datetime(2021, 1, 1), step_hours=5)


class _NoNative:
    """Stands in for the library: any native call fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"native call {name} after a wrong argument")


@pytest.fixture
def no_native(monkeypatch):
    from msfno_amd import _native as N
    monkeypatch.setattr(N, "_lib", _NoNative())


def test_wrong_arguments_raise_before_any_native_call(no_native):
    from msfno_amd import timestats as T
    C, H, W = 2, 3, 4
    fs = T.FieldStats(C, H, W, device="cpu")
    em = T.ErrorMaps(C, H, W, device="cpu")
    ea = T.ErrorMaps(C, H, W, anomalies=True, device="cpu")
    cl = T.Climatology(5, C, H, W, device="cpu")
    x = torch.zeros(2, C, H, W)
    with pytest.raises(ValueError, match="GPU"):          # a CPU tensor
        fs.update(x)
    with pytest.raises(ValueError, match="GPU"):
        em.update(x, x)
    with pytest.raises(ValueError, match=r"\(C, H, W\)"):  # a wrong shape
        fs.update(torch.zeros(2, C, H, W + 1))
    with pytest.raises(ValueError, match=r"\(C, H, W\)"):
        em.update(torch.zeros(C + 1, H, W), torch.zeros(C + 1, H, W))
    with pytest.raises(ValueError, match="anomalies=True"):  # a climatology without the planes
        em.update(x, x, clim=torch.zeros(C, H, W))
    with pytest.raises(ValueError, match="climatology"):     # and the planes without one
        ea.update(x, x)
    with pytest.raises(ValueError, match="one entry per batch element"):
        cl.update(x, [0, 1, 2])
    with pytest.raises(ValueError, match="bin"):
        cl.update(x, [0, 5])
    with pytest.raises(ValueError, match="minmax"):
        fs.min
    with pytest.raises(ValueError):
        T.FieldStats(0, H, W, device="cpu")
    with pytest.raises(ValueError, match="device states"):
        fs.merge(T.FieldStats(C, H, W, device="cpu"))
    with pytest.raises(ValueError, match="same class"):
        em.merge(ea)


def test_fresh_state_and_accessors_on_the_host():
    from msfno_amd import timestats as T
    fs = T.FieldStats(2, 3, 4, minmax=True, device="cpu")
    assert fs.K == 4 and int(fs.count.sum()) == 0
    assert torch.isinf(fs._planes[2]).all() and (fs._planes[2] > 0).all()
    assert torch.isinf(fs._planes[3]).all() and (fs._planes[3] < 0).all()
    for m in (fs.mean, fs.var(), fs.std, fs.min, fs.max):
        assert torch.isnan(m).all()
    # a state dict round trip keeps the bits; the accessors follow the formulas
    fs._count.fill_(4)
    fs._planes[0].fill_(2.0)
    fs._planes[1].fill_(12.0)
    other = T.FieldStats(2, 3, 4, minmax=True, device="cpu").load_state_dict(fs.state_dict())
    assert torch.equal(other._count, fs._count) and torch.equal(other._planes, fs._planes)
    assert (other.mean == 2).all() and (other.var() == 3).all() and (other.var(ddof=1) == 4).all()
    assert torch.isnan(other.var(ddof=4)).all()
    with pytest.raises(ValueError, match="state dict"):
        T.FieldStats(2, 3, 4, device="cpu").load_state_dict(fs.state_dict())
    lt = T.LeadTimeMaps(3, 2, 3, 4, anomalies=True, device="cpu")
    assert len(lt) == 3 and lt[1].K == 8 and lt[1]._planes.stride(0) == 3 * 2 * 3 * 4
    lt[1]._count.fill_(1)
    assert int(lt._count.sum()) == 2 * 3 * 4 and int(lt[0].count.sum()) == 0
