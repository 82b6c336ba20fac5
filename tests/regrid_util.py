"""The fp64 restatement of msfno_amd/regrid.py's operator and its derived error bound, shared
by test_regrid_host.py and test_gpu_regrid.py.

The operator is ``y = Wlat @ x @ Wlon.T`` per slab, (Wlat, Wlon) = ``Regridder.dense()``, and
in normalised mode ``num / den`` with ``num = Wlat @ (v x) @ Wlon.T``, ``den = Wlat @ v @
Wlon.T``, v = mask * (x is not NaN), and ``fill`` where ``den <= 0`` or ``den < min_valid``.

Bound.  The kernel sums at most K = taps_lat + taps_lon terms per output in two sequential
fp32 chains, over fp32-rounded weights:
    linear       |y - y64| <= (K + 4) 2^-24 (|Wlat| |x| |Wlon|^T)
    normalised   |y - y64| <= 2 (K + 4) 2^-24 mag / den,   mag = |Wlat| |v x| |Wlon|^T
element-wise, the right-hand sides formed in fp64."""
import numpy as np

EPS = 2.0 ** -24


def field(shape, seed, kind="offset"):
    """fp32 slabs: 300 + N(0, 1) (the case that punishes a sum not formed carefully) or
    N(0, 1)."""
    g = np.random.default_rng(seed)
    x = g.standard_normal(shape)
    return (300.0 + x if kind == "offset" else x).astype(np.float32)


def taps(R):
    return R.lat.taps + R.lon.taps


def apply64(Wlat, Wlon, x):
    """Wlat @ x @ Wlon.T over the leading dimensions of x, in fp64."""
    return np.matmul(np.matmul(Wlat, np.asarray(x, dtype=np.float64)), Wlon.T)


def linear(R, x):
    """(y64, bound) of the linear mode for x (..., H, W) without NaN."""
    Wlat, Wlon = R.dense()
    y = apply64(Wlat, Wlon, x)
    mag = apply64(np.abs(Wlat), np.abs(Wlon), np.abs(np.asarray(x, dtype=np.float64)))
    return y, (taps(R) + 4) * EPS * mag


def normalised(R, x, mask=None, skip_nan=False, min_valid=0.0, fill=np.nan):
    """(y64, bound, den, valid) of the normalised mode; y64 holds ``fill`` and the bound 0
    where the output is not valid."""
    Wlat, Wlon = R.dense()
    x = np.asarray(x, dtype=np.float64)
    v = np.ones_like(x)
    if mask is not None:
        v = v * np.asarray(mask, dtype=np.float64)
    if skip_nan:
        v = v * ~np.isnan(x)
    vx = np.where(v != 0, x, 0.0) * v
    num = apply64(Wlat, Wlon, vx)
    den = apply64(Wlat, Wlon, v)
    mag = apply64(np.abs(Wlat), np.abs(Wlon), np.abs(vx))
    valid = (den > 0) & (den >= min_valid)
    safe = np.where(valid, den, 1.0)
    y = np.where(valid, num / safe, fill)
    return y, np.where(valid, 2 * (taps(R) + 4) * EPS * mag / safe, 0.0), den, valid


def check(name, got, want, bound):
    """Every output within its bound (NaN where and only where the restatement has NaN);
    returns the worst error / bound."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{name}: NaN pattern differs"
    err = np.abs(np.where(nan, 0.0, got) - np.where(nan, 0.0, want))
    b = np.where(nan, 0.0, bound)
    ratio = float((err / np.maximum(b, 1e-300)).max()) if err.size else 0.0
    print(f"{name}: worst error / bound {ratio:.3f}")
    assert (err <= b).all(), (name, ratio)
    return ratio


def emulate32(R, x):
    """The linear mode as a sequential fp32 sum without FMA, taps in index order, latitude
    stage then longitude stage: what the kernel's order gives at its least favourable."""
    x = np.asarray(x, dtype=np.float32)
    la, lo = R.lat, R.lon
    mid = np.zeros(x.shape[:-2] + (la.n_out, x.shape[-1]), dtype=np.float32)
    for j in range(la.n_out):
        acc = np.zeros(x.shape[:-2] + (x.shape[-1],), dtype=np.float32)
        for a in range(int(la.count[j])):
            t = (la.w[j, a] * x[..., int(la.start[j]) + a, :]).astype(np.float32)
            acc = t if a == 0 else (acc + t).astype(np.float32)
        mid[..., j, :] = acc
    out = np.zeros(x.shape[:-2] + (la.n_out, lo.n_out), dtype=np.float32)
    for i in range(lo.n_out):
        acc = np.zeros(mid.shape[:-1], dtype=np.float32)
        for b in range(int(lo.count[i])):
            t = (lo.w[i, b] * mid[..., (int(lo.start[i]) + b) % lo.n_in]).astype(np.float32)
            acc = t if b == 0 else (acc + t).astype(np.float32)
        out[..., i] = acc
    return out


def dense_from_tables(start, count, w, n_in):
    """The fp64 matrix a table stands for (of the fp32 weights the kernel reads)."""
    W = np.zeros((len(start), n_in))
    for j in range(len(start)):
        for a in range(int(count[j])):
            W[j, (int(start[j]) + a) % n_in] += float(w[j, a])
    return W


def nan_reach(R, r, c):
    """The boolean (H', W') map of the outputs whose counted taps cover source point (r, c)."""
    la, lo = R.lat, R.lon
    rows = np.array([0 <= r - int(la.start[j]) < int(la.count[j]) for j in range(la.n_out)])
    cols = np.array([(c - int(lo.start[i])) % lo.n_in < int(lo.count[i])
                     for i in range(lo.n_out)])
    return rows[:, None] & cols[None, :]
