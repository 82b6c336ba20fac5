"""Restatements of the statistics over time (msfno_amd/timestats.py, csrc/timestats.hip),
written from the formulas: the two-pass mean, variance and covariance over the valid updates
in fp64 (torch), and the same streaming recurrence in fp32 on the CPU (numpy, no fused
multiply-add), plus the error bounds and the shared problems of the tests.

Per pixel, over its N valid updates, with A = max |a| over them, sigma^2 the fp64 variance
and eps = 2^-23:

    |mean - mean64|        <= N eps A
    |m2 / N - sigma^2|     <= eps (8 A sigma + N sigma^2)
    |c_pt / N - cov64|     <= eps (8 (A_pa sigma_ta + A_ta sigma_pa) / 2 + N sigma_pa sigma_ta)
    mean_abs as the mean

These are rounding bounds of the recurrence.  The covariance bound is the variance bound's
form: a relative perturbation eps of pa (of size A_pa) moves the covariance by at most
eps A_pa sigma_ta, and likewise for ta, so A sigma becomes the mean of the two cross terms
(A sigma itself where pa = ta) under the same constant, and sigma^2 becomes
sigma_pa sigma_ta.  The inputs' own subtraction (a = x - c in fp32, relative eps / 2 of a) is
inside the A sigma term's margin.
"""
import functools

import numpy as np
import torch

EPS = 2.0 ** -23

SHAPES = [(1, 1, 1, 1), (1, 1, 1, 3), (2, 3, 5, 7), (3, 2, 4, 8), (1, 2, 3, 2731)]
# (shape, updates): 1 and 3 calls everywhere, 64 on the odd-phase shape only
CASES = [(s, u) for s in SHAPES for u in (1, 3)] + [((2, 3, 5, 7), 64)]
FAMILIES = ("300", "scales")


@functools.lru_cache(maxsize=None)
def problem(shape, updates, family):
    """(p, t, c): fp32 (updates, B, S, H, W) forecasts, truths and climatologies (one slab
    per (call, b, s)), shared and never modified.  "300": 300 +- 1 fields; "scales": the
    channel scales 1e-3 .. 1e4 of verify_util.problem."""
    B, S, H, W = shape
    g = torch.Generator().manual_seed(4000 + updates + 7 * B + 10 * S + 100 * H + W
                                      + FAMILIES.index(family))
    full = (updates,) + shape
    if family == "300":
        t = 300.0 + torch.randn(full, generator=g)
        p = t + 0.3 * torch.randn(full, generator=g)
        c = 300.0 + 0.7 * torch.randn(full, generator=g)
    else:
        scale = torch.logspace(-3, 4, S)[None, None, :, None, None] if S > 1 \
            else torch.ones(1, 1, 1, 1, 1)
        t = (torch.randn(full, generator=g) + 0.5) * scale
        p = t + 0.3 * scale * torch.randn(full, generator=g)
        c = (torch.randn(full, generator=g) * 0.7 + 0.5) * scale
    return p.float(), t.float(), c.float()


def flat(x):
    """(updates, B, S, H, W) -> (N = updates B, S, H, W): the order the updates are applied
    in."""
    return x.reshape((-1,) + tuple(x.shape[2:]))


def moments64(a, valid=None, b=None):
    """(n, mean, var) of ``a`` (N, ...) over the valid updates per pixel, two-pass in fp64;
    with ``b`` also (mean_b, var_b, cov).  n == 0 gives NaN."""
    a = a.double()
    valid = torch.ones_like(a, dtype=torch.bool) if valid is None else valid
    zero = torch.zeros((), dtype=torch.float64)
    n = valid.sum(0)
    nf = n.double()

    def mv(x):
        mean = torch.where(valid, x, zero).sum(0) / nf
        dev = torch.where(valid, x - mean, zero)
        return mean, dev, (dev * dev).sum(0) / nf

    mean, dev, var = mv(a)
    if b is None:
        return n, mean, var
    mb, devb, varb = mv(b.double())
    return n, mean, var, mb, varb, (dev * devb).sum(0) / nf


def amax(a, valid=None):
    """A = max |a| over the valid updates per pixel (0 where there is none)."""
    a = a.double().abs()
    if valid is not None:
        a = torch.where(valid, a, torch.zeros((), dtype=torch.float64))
    return a.max(0).values


def mean_bound(n, A):
    return n.double() * EPS * A


def var_bound(n, A, var):
    return EPS * (8.0 * A * var.sqrt() + n.double() * var)


def cov_bound(n, A_a, var_a, A_b, var_b):
    sa, sb = var_a.sqrt(), var_b.sqrt()
    return EPS * (8.0 * 0.5 * (A_a * sb + A_b * sa) + n.double() * sa * sb)


def assert_within(got, want, bound, what):
    """|got - want| <= bound wherever want is a number; prints the worst ratio first."""
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    ok = ~torch.isnan(want)
    err = (got - want).abs()[ok]
    bnd = bound[ok]
    assert not torch.isnan(got[ok]).any(), f"{what}: NaN where the reference has a number"
    if err.numel() == 0:
        return
    worst = (err / bnd.clamp(min=1e-300)).max().item() if (bnd > 0).any() else 0.0
    print(f"{what}: worst error / bound = {worst:.3g}")
    assert (err <= bnd).all(), f"{what}: error {err.max().item():.3e} exceeds the bound " \
                               f"(worst ratio {worst:.3g})"


def check_moments(count, mean, m2, a, valid, what):
    """count exact, mean and m2 / n within the bounds against fp64 of the values ``a``."""
    n, mean64, var64 = moments64(a, valid)
    A = amax(a, valid)
    assert torch.equal(torch.as_tensor(count).to(torch.int64), n), f"{what}: count"
    has = n > 0
    nn = n.clamp(min=1).double()
    assert_within(torch.where(has, mean.double(), torch.full_like(mean64, float("nan"))),
                  mean64, mean_bound(n, A), f"{what} mean")
    assert_within(torch.where(has, m2.double() / nn, torch.full_like(var64, float("nan"))),
                  var64, var_bound(n, A, var64), f"{what} m2/n")


def check_cov(c_pt, pa, ta, valid, what):
    n, _, va, _, vb, cov = moments64(pa, valid, ta)
    nn = n.clamp(min=1).double()
    got = torch.where(n > 0, c_pt.double() / nn, torch.full_like(cov, float("nan")))
    assert_within(got, cov, cov_bound(n, amax(pa, valid), va, amax(ta, valid), vb),
                  f"{what} c_pt/n")


# ---- the recurrence in fp32 on the CPU -------------------------------------------------------
def _welford32(n, mean, m2, a, ok):
    """One step for the pixels ``ok``; returns the old mean."""
    f32 = np.float32
    fn = (n + 1).astype(f32)
    delta = (a - mean).astype(f32)
    new_mean = (mean + (delta / fn).astype(f32)).astype(f32)
    new_m2 = (m2 + (delta * (a - new_mean).astype(f32)).astype(f32)).astype(f32)
    old = mean.copy()
    mean[ok] = new_mean[ok]
    m2[ok] = new_m2[ok]
    return old


def field32(a, valid=None):
    """(n, mean, m2, lo, hi) of the FIELD recurrence over ``a`` (N, ...) fp32."""
    a = np.asarray(a, dtype=np.float32)
    shape = a.shape[1:]
    n = np.zeros(shape, np.int64)
    mean, m2 = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    lo, hi = np.full(shape, np.inf, np.float32), np.full(shape, -np.inf, np.float32)
    for k in range(a.shape[0]):
        ok = np.ones(shape, bool) if valid is None else np.asarray(valid[k])
        _welford32(n, mean, m2, a[k], ok)
        lo[ok] = np.fmin(lo, a[k])[ok]
        hi[ok] = np.fmax(hi, a[k])[ok]
        n[ok] += 1
    return n, mean, m2, lo, hi


def error32(p, t, c=None, valid=None):
    """(n, planes) of the ERROR recurrence: planes [mean_d, m2_d, mean_abs] and with ``c``
    [mean_pa, m2_pa, mean_ta, m2_ta, c_pt] behind them."""
    f32 = np.float32
    p, t = np.asarray(p, f32), np.asarray(t, f32)
    shape = p.shape[1:]
    K = 3 if c is None else 8
    n = np.zeros(shape, np.int64)
    q = [np.zeros(shape, f32) for _ in range(K)]
    for k in range(p.shape[0]):
        ok = np.ones(shape, bool) if valid is None else np.asarray(valid[k])
        fn = (n + 1).astype(f32)
        d = (p[k] - t[k]).astype(f32)
        _welford32(n, q[0], q[1], d, ok)
        q[2][ok] = (q[2] + ((np.abs(d) - q[2]).astype(f32) / fn).astype(f32)).astype(f32)[ok]
        if c is not None:
            ck = np.asarray(c[k], f32)
            pa, ta = (p[k] - ck).astype(f32), (t[k] - ck).astype(f32)
            pa_old = _welford32(n, q[3], q[4], pa, ok)
            _welford32(n, q[5], q[6], ta, ok)
            step = ((pa - pa_old).astype(f32) * (ta - q[5]).astype(f32)).astype(f32)
            q[7][ok] = (q[7] + step).astype(f32)[ok]
        n[ok] += 1
    return n, q


def naive_var32(a):
    """sum x^2 - (sum x)^2 / n, all in fp32, over n: what this feature does not do."""
    a = np.asarray(a, np.float32)
    s = np.zeros(a.shape[1:], np.float32)
    s2 = np.zeros(a.shape[1:], np.float32)
    for k in range(a.shape[0]):
        s = (s + a[k]).astype(np.float32)
        s2 = (s2 + (a[k] * a[k]).astype(np.float32)).astype(np.float32)
    n = np.float32(a.shape[0])
    return ((s2 - (s * s / n).astype(np.float32)).astype(np.float32) / n).astype(np.float32)
