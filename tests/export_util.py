"""The numpy fp32 restatement of the 16-bit export encoding (csrc/pack.hip, include/msfno.h):
range over the selection, E, q, decode.  It is the expected value of the export tests, compared
with ==.  Every operation is a numpy float32 operation (IEEE, round to nearest even)."""
import numpy as np

F32 = np.float32


def select(x, slab=None, win=None):
    """The selected points of x (S, H, W): (S_out, nlat_out, nlon_out), a copy."""
    x = np.asarray(x)
    if slab is not None:
        x = x[np.asarray(slab, dtype=np.int64)]
    if win is not None:
        lat0, lat_step, nlat_out, lon0, lon_step, nlon_out = win
        x = x[:, lat0:lat0 + (nlat_out - 1) * lat_step + 1:lat_step,
              lon0:lon0 + (nlon_out - 1) * lon_step + 1:lon_step]
    return np.ascontiguousarray(x, dtype=F32)


def exponent(d):
    """E of the fp32 range d >= 0: 0 where d == 0, else the smallest integer with
    d <= 65535 * 2^E (exact integer arithmetic: python ints and fractions), at least -126."""
    from fractions import Fraction
    d = F32(d)
    if d == 0:
        return 0
    fd = Fraction(float(d))                 # exact
    m, e = np.frexp(np.float64(d))          # d = m 2^e, 0.5 <= m < 1: a first guess
    E = int(e) - 17
    while fd > 65535 * Fraction(2) ** E:
        E += 1
    while fd <= 65535 * Fraction(2) ** (E - 1):
        E -= 1
    return max(E, -126)


def encode(x):
    """(ref (S,) fp32, exp2 (S,) int32, q (S, H, W) uint16) of the slabs x (S, H, W) fp32."""
    x = np.ascontiguousarray(x, dtype=F32)
    S = x.shape[0]
    ref = np.empty(S, F32)
    exp2 = np.empty(S, np.int32)
    q = np.empty(x.shape, np.uint16)
    for s in range(S):
        lo, hi = x[s].min(), x[s].max()
        d = F32(hi - lo)
        E = exponent(d)
        ref[s], exp2[s] = lo, E
        t = (x[s] - lo).astype(F32)
        v = np.rint(np.ldexp(t, -E).astype(F32))
        q[s] = np.clip(v, 0, 65535).astype(np.uint16)
    return ref, exp2, q


def pack(x, slab=None, win=None):
    return encode(select(x, slab, win))


def decode(q, ref, exp2):
    """xhat = fl32(ref + fl32(q) * 2^E), ref and exp2 of shape q.shape[:-2]."""
    q = np.asarray(q, dtype=np.uint16)
    r = np.asarray(ref, dtype=F32)[..., None, None]
    e = np.asarray(exp2, dtype=np.int32)[..., None, None]
    return (r + np.ldexp(q.astype(F32), e).astype(F32)).astype(F32)


def ulp32(v):
    """The spacing of fp32 at |v| (fp64 array in, fp64 out)."""
    return np.spacing(np.abs(np.asarray(v)).astype(F32)).astype(np.float64)


def bound(x, ref, exp2, xhat):
    """The derived round-trip bound per point, in fp64:
    2^(E-1) + ulp32(d)/2 + ulp32(max |xhat|)/2 (the rounding of q, of x - R and of the decode's
    add), d and max |xhat| per slab."""
    x = np.asarray(x, dtype=np.float64)
    S = x.shape[0]
    out = np.empty(S)
    for s in range(S):
        d = F32(F32(x[s].max()) - F32(x[s].min()))
        out[s] = (2.0 ** (int(exp2[s]) - 1) + ulp32(d) / 2
                  + ulp32(np.abs(np.asarray(xhat[s], dtype=np.float64)).max()) / 2)
    return out[:, None, None]


def slabs(shape, seed=0, kind="field"):
    """Test slabs (S, H, W) fp32: 300 + N(0, 1) ("field") or N(0, 1) 1e-3 ("small")."""
    g = np.random.default_rng(seed)
    n = g.standard_normal(shape).astype(F32)
    return (F32(300) + n).astype(F32) if kind == "field" else (n * F32(1e-3)).astype(F32)


def edge_slabs():
    """(name, slab (1, H, W) fp32, expected E or None, expected max q or None) of the edges of
    the encoding."""
    out = []
    out.append(("constant", np.full((1, 3, 5), 287.25, F32), 0, 0))
    for k in (-20, 0, 7):
        top = F32(65535.0 * 2.0 ** k)
        a = np.zeros((1, 2, 6), F32)
        a[0, 1, 3] = top
        a[0, 0, 2] = F32(0.25) * top
        out.append((f"65535*2^{k}", a, k, 65535))
        b = a.copy()
        b[0, 1, 3] = np.nextafter(top, F32(np.inf), dtype=F32)
        out.append((f"nextafter(65535*2^{k})", b, k + 1, None))
    t = np.zeros((1, 2, 4), F32)
    t[0, 0] = [0.0, 0.5, 1.5, 2.5]
    t[0, 1] = [65534.5, 65535.0, 3.0, 7.0]
    out.append(("ties", t, 0, 65535))
    g = np.random.default_rng(3)
    out.append(("negative", (-250 - 40 * g.random((1, 4, 9))).astype(F32), None, None))
    out.append(("1e30", (1e30 * (g.random((1, 4, 9)) - 0.5)).astype(F32), None, None))
    out.append(("1e-30", (1e-30 * (g.random((1, 4, 9)) - 0.5)).astype(F32), None, None))
    # d far below 65535 * 2^-126: the clamp E = -126 acts (subnormal and small normal ranges)
    out.append(("clamp subnormal", (F32(1e-40) * g.integers(0, 9, (1, 3, 7))).astype(F32),
                -126, None))
    # multiples of 2^-126 up to 30000: the unclamped E is -127; with -126 every q is the multiple
    c = g.integers(0, 30000, (1, 3, 7))
    c[0, 0, 0], c[0, 2, 6] = 0, 30000
    out.append(("clamp normal", (F32(2.0 ** -126) * c).astype(F32), -126, 30000))
    return out
