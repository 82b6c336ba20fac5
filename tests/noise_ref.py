"""Numpy reference of the random-field stream of csrc/noise.hip: a
Philox4x32-10 and the coefficient formula, in fp64 (the reference) or with every function
evaluated in float32 (the yardstick of the GPU test's tolerance).

    key      (seed & 0xffffffff, seed >> 32)
    counter  (l P + p, f, draw & 0xffffffff, draw >> 32),  P = ceil(mmax / 2), p = m // 2
    words    (w0, w1) -> m = 2p, (w2, w3) -> m = 2p + 1
    u        ((w >> 9) + 0.5) 2^-23
    r = sqrt(-2 ln u_a), z0 = r cos(2 pi u_b), z1 = r sin(2 pi u_b)
    xi       (z0, 0) for m = 0, (z0, z1) / sqrt(2) for 1 <= m <= l, 0 for m > l
    out      a prev + b sqrt_eig[(field0 + i) % K][l] xi, exactly 0 for m > l
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: four broadcastable arrays (or ints), key: two ints -> (..., 4) uint32."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK) for x in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def words(seed, draw, fields, lmax, mmax):
    """(len(fields), lmax, P, 4) uint32: the Philox blocks of the global fields `fields`."""
    P = (mmax + 1) // 2
    f = np.asarray(fields, dtype=np.uint64)[:, None, None]
    c0 = (np.arange(lmax, dtype=np.uint64)[:, None] * np.uint64(P)
          + np.arange(P, dtype=np.uint64)[None, :])[None]
    return philox4x32_10((c0, f, draw & MASK, (draw >> 32) & MASK),
                         (seed & MASK, (seed >> 32) & MASK))


def xi(seed, draw, fields, lmax, mmax, dtype=np.float64):
    """(re, im), each (len(fields), lmax, mmax) of `dtype`, every function evaluated in it."""
    w = words(seed, draw, fields, lmax, mmax)
    n, _, P, _ = w.shape
    t = dtype
    u = ((w >> np.uint32(9)).astype(t) + t(0.5)) * t(2.0 ** -23)   # exact in fp32 and fp64
    ua = u[..., 0::2].reshape(n, lmax, 2 * P)[..., :mmax]
    ub = u[..., 1::2].reshape(n, lmax, 2 * P)[..., :mmax]
    r = np.sqrt(t(-2.0) * np.log(ua))
    ang = t(2.0 * np.pi) * ub
    z0, z1 = r * np.cos(ang), r * np.sin(ang)
    assert z0.dtype == t and z1.dtype == t
    l = np.arange(lmax)[:, None]
    m = np.arange(mmax)[None, :]
    h = t(np.sqrt(0.5))
    re = np.where(m == 0, z0, np.where(m <= l, z0 * h, t(0)))
    im = np.where((m >= 1) & (m <= l), z1 * h, t(0))
    return re.astype(t), im.astype(t)


def spectral(seed, draw, n, field0, lmax, mmax, sqrt_eig, a=0.0, b=1.0, prev=None,
             dtype=np.float64):
    """(n, lmax, mmax) complex (complex128, or complex64 for float32) of the stream:
    a prev + b sqrt_eig[(field0 + i) % K] xi, zero where m > l.  `sqrt_eig` (K, lmax) holds
    the fp32 values the kernel reads; `a`, `b` the fp32 values it is passed."""
    t = dtype
    fields = np.arange(field0, field0 + n)
    re, im = xi(seed, draw, fields, lmax, mmax, t)
    se = np.asarray(sqrt_eig, dtype=np.float32).reshape(-1, lmax)
    s = t(np.float32(b)) * se[fields % se.shape[0]].astype(t)[:, :, None]
    re, im = s * re, s * im
    if prev is not None:
        inside = np.arange(mmax)[None, :] <= np.arange(lmax)[:, None]
        pa = t(np.float32(a))
        re = np.where(inside, pa * prev.real.astype(t) + re, t(0))
        im = np.where(inside, pa * prev.imag.astype(t) + im, t(0))
    out = np.empty(re.shape, dtype=np.complex64 if t is np.float32 else np.complex128)
    out.real, out.imag = re, im
    return out


def degree_power_ratio(c, sqrt_eig):
    """mean over fields of (|c_l0|^2 + 2 sum_{m >= 1} |c_lm|^2) / ((2l + 1) S_l), l >= 1."""
    p = np.abs(c[..., 0]) ** 2 + 2.0 * (np.abs(c[..., 1:]) ** 2).sum(-1)
    l = np.arange(c.shape[-2])
    S = np.asarray(sqrt_eig, dtype=np.float64) ** 2
    return (p.mean(0)[1:]) / ((2 * l[1:] + 1) * S[1:])


def degree_power_sigma(nfields, lmax):
    """The standard deviation of that ratio: (2l + 1) S_l is the mean of a S_l / 2-scaled
    chi-square with 2l + 1 degrees of freedom, so the mean over nfields has relative
    deviation sqrt(2 / (nfields (2l + 1)))."""
    l = np.arange(1, lmax)
    return np.sqrt(2.0 / (nfields * (2 * l + 1)))


# the statistics test (GPU and host): 256 fields at lmax = mmax = 16 from this seed, whose
# reference stream stays within 4 deviations (test_noise_host checks that)
STAT_SEED, STAT_FIELDS, STAT_LMAX = 2024, 256, 16
