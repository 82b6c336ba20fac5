"""Legendre-stage shape sweep: the cases and their CPU references, shared by
test_legendre_cases_host.py and test_gpu_legendre_shapes.py.

The Legendre stage is a family of kernels and template bodies picked by shape
(csrc/plan.cpp ensure_desc3, x3f_usable; csrc/legendre_x3.hip):

  legendre_x3_kernel   tiled, X3D_BM rows x X3D_BN columns, k-tiles of X3D_BK: the forward
                       transform of a stand-alone RealSHT, and every fallback;
  legendre_x3r_kernel  inverse, register-resident A: one body per NK = ceil(K / 32) <= 6
                       (K the degrees of one parity, <= X3R_KMAX), columns N = Ke <=
                       X3R_NMAX in chunks of 32 through a 3-stage ring, X3D_BM rows a tile;
  legendre_x3f_kernel  forward inside a block with norm0, register-resident B: one body per
                       KS = ceil(K / 32) <= 12 (K = Ke or Ko <= X3F_KMAX latitudes of a
                       hemisphere), X3F_RB rows a tile in chunks of X3F_CHUNK through a
                       3-stage ring (2 with MSFNO_X3F_NS=2), X3D_BN columns a tile.

Ke = ceil(nlat / 2) is the folded latitude count of the even problems, Ko = nlat // 2 that
of the odd ones.  The constants below are csrc/common.h's: when one of them changes, the
cases that name it want revisiting.

Tables.  "dense": a seeded r = randn(mmax, lmax, nlat) made equatorially symmetric,
t = (r + s flip(r, -1)) / 2 with s = (-1)^(l - m), zero where l < m: it satisfies
check_symmetry_kernel's rule exactly (also after .float()), so the folded layout and the
register-resident kernels run, and every entry of every tile is O(1).  Forward tables are
scaled by nlat^-1/2 to keep the coefficients O(1).  The expected result is the transform's
definition in fp64 (fft_size_cases._forward / _inverse).  "grid": the equiangular
quadrature tables of oracle.sht_ref on an odd nlat, a true quadrature table at the same
depth.

Error measures.  Forward: per (m, parity) block of the (..., l, m) result, max |got - want|
over the block / max |want| over the block, every block with at least one degree
(forward_block_errors).  Inverse: per Fourier column m of the output
(fft_size_cases.column_errors), columns m >= lmax (no degree) skipped.  Nothing else is
excluded.  Bar: fft_size_cases.GPU_BAR per block or column; the fp32 restatement of the
reference stays under FP32_BAR = GPU_BAR / 2 (test_legendre_cases_host.py).

Inverse inputs are random phases of unit modulus on every degree l >= m (zero below), so
every k of every NK body carries the same weight.

Block cases compare FourierNeuralOperatorBlock_Filmed.global_conv of a block without inner
skip, MLP or outer skip (norm0 -> filter -> (GELU) -> norm1: the spectral path alone) with
oracle.sfno_ref.global_conv in fp64.  Bar (block_bar): min(1e-4 max(1, |want|max),
BLOCK_E32_FACTOR e32) with e32 the max-abs distance of the same oracle run in fp32."""
import functools
from collections import namedtuple

import torch

import fft_size_cases as F
from oracle import sfno_ref
from oracle import sht_ref as S

# csrc/common.h
X3D_BM, X3D_BN, X3D_BK = 128, 64, 32     # tiled kernel; X3D_BM also x3r's row tile
X3R_KMAX, X3R_NMAX = 192, 1024
X3F_KMAX, X3F_RB = 384, 256
X3F_CHUNK = 16                            # rows per ring stage of x3f (legendre_x3.hip)
X3R_CHUNK = 32                            # columns per ring stage of x3r

NLON = 32                                 # a compiled FFT codelet
GPU_BAR = F.GPU_BAR
FP32_BAR = GPU_BAR / 2
BLOCK_E32_FACTOR = 8
MUTATION = 1.001                          # host condition: one block scaled by this ...
MUTATION_MARGIN = 4                       # ... moves the oracle by this many bars


def ke(nlat):
    return (nlat + 1) // 2


def ko(nlat):
    return nlat // 2


def ks(k):
    """The x3f body (and the tiled kernel's k-tile count) of a K-latitude problem."""
    return -(-k // X3D_BK)


def nk(lmax, m=0):
    """The x3r body of order m's even problem: its K = ceil((lmax - m) / 2) degrees."""
    return -(-((max(lmax - m, 0) + 1) // 2) // 32)


# ---- stand-alone transforms ----------------------------------------------------------
Case = namedtuple("Case", "nlat lmax mmax lead kind")


def _c(nlat, lmax=20, mmax=5, lead=(1, 3), kind="dense"):
    return Case(nlat, lmax, mmax, lead, kind)


# depth: nlat -> Ke (KS); R = 6 rows
DEPTH_NLAT = [
    129,    # Ke 65 = 32.2 + 1 (KS 3, 31 pad columns), Ko 64 (KS 2); x3r nch 3, last chunk 1 column
    191,    # Ke 96 = 32.3 (KS 3, no pad), Ko 95; x3r nch 3 exactly
    192,    # Ke = Ko = 96, no equator row
    225,    # Ke 113 (KS 4), Ko 112; x3r nch 4: the first reuse of ring stage 0
    257,    # Ke 129 = 32.4 + 1 (KS 5), Ko 128 (KS 4); x3r nch 5
    320,    # Ke = Ko = 160 = 32.5 (KS 5)
    353,    # Ke 177 (KS 6), Ko 176
    417,    # Ke 209 (KS 7), Ko 208
    449,    # Ke 225 = 32.7 + 1 (KS 8), Ko 224 (KS 7)
    545,    # Ke 273 (KS 9), Ko 272
    609,    # Ke 305 (KS 10), Ko 304
    673,    # Ke 337 (KS 11), Ko 336
    767,    # Ke 384 = X3F_KMAX = 32.12 (KS 12), Ko 383
    768,    # Ke = Ko = 384
    769,    # Ke 385: the first that leaves x3f for the tiled kernel (13 k-tiles)
]
assert sorted({ks(ke(n)) for n in DEPTH_NLAT}) == list(range(3, 14))
assert ke(767) == X3F_KMAX and ke(769) == X3F_KMAX + 1
GRID_NLAT = (129, 449, 673)              # real-grid twins (odd nlat)

DEGREE_NLAT = 257
# lmax -> K = le(m = 0): 65, 100, 145, 192 = X3R_KMAX (NK 3, 4, 5, 6), 193 (tiled fallback);
# forward N = lpe: 2, 2, 3, 3, 4 column tiles of X3D_BN, the last one ragged
DEGREE_LMAX = [130, 200, 290, 2 * X3R_KMAX, 2 * X3R_KMAX + 2]
assert [nk(l) for l in DEGREE_LMAX] == [3, 4, 5, 6, 7]

# rows R = 2 bc: 2, 130 and 258 (a second and a third X3D_BM-row tile with 2 rows), 282 (> 256,
# no multiple of 16)
ROW_LEADS = [(1,), (65,), (129,), (3, 47)]

RAGGED = _c(129, lmax=3, mmax=5, lead=(65,))

CASES = (
    [_c(n) for n in DEPTH_NLAT]
    + [_c(n, kind="grid") for n in GRID_NLAT]
    + [_c(DEGREE_NLAT, lmax=l, mmax=3) for l in DEGREE_LMAX]
    + [_c(DEGREE_NLAT, lmax=130, mmax=3, kind="grid")]
    # lmax < mmax: columns 3, 4 without a degree; m = lmax - 1 = 2 has one even degree and an
    # odd problem with K = 0 (x3r_zero); Ke 65 (no multiple of 16), R = 130
    + [RAGGED]
    + [_c(129, lmax=12, lead=l) for l in ROW_LEADS]
    # all 17 orders of the grid width (Nyquist column), lmax < mmax, 150 rows
    + [_c(449, lmax=12, mmax=NLON // 2 + 1, lead=(75,))]
    # Ke 1024 = X3R_NMAX, the largest the inverse register kernel takes, and 1025, the first
    # it leaves to the tiled kernel
    + [_c(2 * X3R_NMAX - 1, lmax=8, mmax=3), _c(2 * X3R_NMAX + 1, lmax=8, mmax=3)]
    # the smallest grid with an odd count of spectrum values, bc nlat mmax = 3.9.5 (as in every
    # case above with lead (1, 3), odd nlat and mmax 5): the codelet inverse FFT stages its
    # input in 16-B chunks and once lost the last row's last bin of such a spectrum
    + [_c(9, lmax=5, mmax=5, lead=(3,))]
)


def case_id(c):
    lead = "x".join(map(str, c.lead))
    return f"{c.kind}-{c.nlat}-l{c.lmax}-m{c.mmax}-b{lead}"


IDS = [case_id(c) for c in CASES]
assert len(set(IDS)) == len(IDS)


def _seed(c, salt):
    return 1000003 * salt + 4099 * c.nlat + 17 * c.lmax + c.mmax


def symmetric_table(mmax, lmax, nlat, seed, scale=1.0):
    """fp64 (mmax, lmax, nlat): (r + s flip(r)) / 2, s = (-1)^(l - m), zero where l < m."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(mmax, lmax, nlat, generator=g, dtype=torch.float64)
    d = torch.arange(lmax)[None, :] - torch.arange(mmax)[:, None]            # l - m, [m, l]
    s = (1.0 - 2.0 * (d % 2)).to(torch.float64)[:, :, None]
    t = 0.5 * (r + s * r.flip(-1))
    t[d < 0] = 0.0
    return t * scale


def is_symmetric(t):
    """check_symmetry_kernel's rule with tolerance zero, on the table as given."""
    mmax, lmax, nlat = t.shape
    d = torch.arange(lmax)[None, :] - torch.arange(mmax)[:, None]
    s = (1.0 - 2.0 * (d % 2)).to(t.dtype)[:, :, None]
    h = nlat // 2
    return bool((t.flip(-1)[..., :h] == s * t[..., :h]).all())


@functools.lru_cache(maxsize=None)
def table(c, inverse):
    """The fp64 (mmax, lmax, nlat) table of case `c` (stand-alone or block)."""
    if c.kind == "grid":
        if inverse:
            return S.InverseRealSHT(c.nlat, NLON, lmax=c.lmax, mmax=c.mmax, grid="equiangular").pct
        return S.RealSHT(c.nlat, NLON, lmax=c.lmax, mmax=c.mmax, grid="equiangular").weights
    if inverse:
        return symmetric_table(c.mmax, c.lmax, c.nlat, _seed(c, 5))
    return symmetric_table(c.mmax, c.lmax, c.nlat, _seed(c, 3), c.nlat ** -0.5)


@functools.lru_cache(maxsize=None)
def forward_input(c):
    g = torch.Generator().manual_seed(_seed(c, 1))
    return torch.randn(*c.lead, c.nlat, NLON, generator=g)


@functools.lru_cache(maxsize=None)
def inverse_input(c):
    """(..., lmax, mmax) complex64, unit modulus where l >= m, zero elsewhere; the imaginary
    parts at m = 0 (and at the Nyquist column) are not zero: irfft ignores them."""
    g = torch.Generator().manual_seed(_seed(c, 2))
    a = torch.view_as_complex(torch.randn(*c.lead, c.lmax, c.mmax, 2, generator=g))
    a = a / a.abs()
    return a * (torch.arange(c.lmax)[:, None] >= torch.arange(c.mmax)[None, :])


@functools.lru_cache(maxsize=None)
def forward_reference(c):
    """fp64 (..., lmax, mmax) complex128; computed once, shared, never modified."""
    return F._forward(forward_input(c).double(), table(c, False), c.mmax)


@functools.lru_cache(maxsize=None)
def inverse_reference(c):
    """fp64 (..., nlat, nlon)."""
    return F._inverse(inverse_input(c).to(torch.complex128), table(c, True), NLON)


def fp32_forward(c):
    return F._forward(forward_input(c), table(c, False).float(), c.mmax)


def fp32_inverse(c):
    return F._inverse(inverse_input(c), table(c, True).float(), NLON)


def forward_blocks(c):
    """[(m, parity)] of every block of the forward result with at least one degree."""
    return [(m, p) for m in range(min(c.mmax, c.lmax)) for p in (0, 1) if m + p < c.lmax]


def forward_block_errors(got, want, c):
    """{(m, parity): max |got - want| over the block / max |want| over the block}."""
    got, want = got.to(torch.complex128), want.to(torch.complex128)
    return {(m, p): ((got[..., m + p::2, m] - want[..., m + p::2, m]).abs().max().item()
                     / want[..., m + p::2, m].abs().max().item())
            for m, p in forward_blocks(c)}


def inverse_column_errors(got, want, c):
    """(min(mmax, lmax),) tensor: fft_size_cases.column_errors of the columns with a degree."""
    return F.column_errors(got, want, c, True)[:min(c.mmax, c.lmax)]


# ---- the block's spectral path -------------------------------------------------------
BlockCase = namedtuple("BlockCase", "filter nlat lmax mmax B C kind")
NL, LIN = "non-linear", "linear"


def _b(i, nlat, lmax=12, mmax=5, B=1, C=8, kind="dense"):
    return BlockCase((NL, LIN)[i % 2], nlat, lmax, mmax, B, C, kind)


# x3f KS 3 .. 12 and the fallback at nlat 769; R = 2 B C = 16: one ring stage
BLOCK_DEPTH = [_b(i, n) for i, n in enumerate(DEPTH_NLAT)]
# R = 32, 48 (nch 2, 3: the ring's first wrap), 264 (a second X3F_RB-row tile of half a
# chunk), 280 (one chunk and a half), 520 (a third tile); C = 12 and 20 give 2 B C % 16 = 8
BLOCK_ROWS = [_b(0, 129, B=2), _b(1, 129, B=3), _b(0, 129, B=11, C=12), _b(1, 129, B=7, C=20),
              _b(0, 129, B=13, C=20)]
assert [2 * c.B * c.C for c in BLOCK_ROWS] == [32, 48, 264, 280, 520]
# N = lpe = 65, 100, 145: 2 and 3 ragged X3D_BN-column tiles of x3f; x3r NK 3, 4, 5, then NK 6
# and the tiled inverse
BLOCK_DEGREES = [_b(i, DEGREE_NLAT, lmax=l, mmax=3) for i, l in enumerate(DEGREE_LMAX)]
# both filters on both tables at one shape: R = 272 = X3F_RB + one chunk
BLOCK_TWINS = [BlockCase(f, 449, 12, 5, 17, 8, k) for k in ("dense", "grid") for f in (NL, LIN)]
# the workspace test's: Ke 65 (no multiple of 16), R = 264 and 280, lmax < mmax
BLOCK_RAGGED = [BlockCase(NL, 129, 4, 5, 11, 12, "dense"), BlockCase(LIN, 129, 4, 5, 7, 20, "dense")]
BLOCK_CASES = BLOCK_DEPTH + BLOCK_ROWS + BLOCK_DEGREES + BLOCK_TWINS + BLOCK_RAGGED
# the x3f launches that differ under MSFNO_X3F_NS=2 (ring depth): depth and rows
BLOCK_VARIANT_CASES = BLOCK_DEPTH + BLOCK_ROWS


def block_id(c):
    return f"{c.filter}-{c.kind}-{c.nlat}-l{c.lmax}-m{c.mmax}-B{c.B}-C{c.C}"


BLOCK_IDS = [block_id(c) for c in BLOCK_CASES]
assert len(set(BLOCK_IDS)) == len(BLOCK_IDS)


def nlon_of(c):
    """The grid width of a block case: NLON, unless the case has a field of its own
    (fft_codelet_cases.py)."""
    return getattr(c, "nlon", NLON)


def block_cfg(c):
    """No inner skip, MLP or outer skip, unless the case has fields `skip` / `mlp`
    (fft_codelet_cases.py)."""
    return sfno_ref.BlockCfg(filter_type=c.filter, inner_skip=getattr(c, "skip", None),
                             outer_skip=None, has_mlp=getattr(c, "mlp", False),
                             spectral_layers=3)


FILTER_TO_SKIP = 2.0                      # standard deviation of the filter's output / the skip's


@functools.lru_cache(maxsize=None)
def block_params(c):
    p = sfno_ref.make_block_params(c.C, c.lmax, c.mmax, block_cfg(c), seed=_seed(c, 7) % 9973,
                                   randomize_affine=True)
    if block_cfg(c).inner_skip is not None:
        _balance_filter(c, p)
    return p


def _balance_filter(c, p):
    """Scales the filter's last (linear) weight by a power of two so that the filter's output
    has about FILTER_TO_SKIP times the standard deviation of the inner skip's (per channel,
    means removed).  With the initialisation's 0.02-weights the filter adds between 0.002 and
    17 times the skip, depending on filter, width and depth: where it adds next to nothing,
    no error of the transforms reaches the block's output."""
    cfg = block_cfg(c)
    q = {k: (v.double() if v.is_floating_point() else v) for k, v in p.items()}
    x = block_input(c).double()
    sht = _Transform(table(c, False), False, c.mmax, None, nlon_of(c))
    isht = _Transform(table(c, True), True, c.mmax, nlon=nlon_of(c))
    with torch.no_grad():
        xn = sfno_ref.instance_norm(x, q["norm0.weight"], q["norm0.bias"], cfg.eps)
        if c.filter == NL:
            name = "filter_layer.filter.wout"
            ws = [q[f"filter_layer.filter.w.{i}"] for i in range(cfg.spectral_layers)]
            f = sfno_ref.spectral_attention_s2(xn, sht, isht, ws, q[name])
        else:
            name = "filter_layer.filter.w"
            f = sfno_ref.spectral_conv_s2(xn, sht, isht, q[name], q["filter_layer.filter.ii"],
                                          q["filter_layer.filter.jj"])
        s = x
        if cfg.inner_skip == "linear":
            s = sfno_ref.conv1x1(x, q["inner_skip.weight"], q["inner_skip.bias"])
    dev = lambda t: (t - t.mean((-2, -1), keepdim=True)).std().item()
    p[name] = p[name] * 2.0 ** round(torch.log2(torch.tensor(FILTER_TO_SKIP * dev(s) / dev(f))).item())


@functools.lru_cache(maxsize=None)
def block_input(c):
    g = torch.Generator().manual_seed(_seed(c, 11) + c.B)
    x = torch.randn(c.B, c.C, c.nlat, nlon_of(c), generator=g)
    if getattr(c, "wave1", 0.0):
        # a zonal-wavenumber-1 wave, its profile in latitude half even, half odd about the
        # equator, its amplitude 0.5 .. 1.5 wave1 by channel: order 1 holds a fixed share of
        # the field's energy however many orders the grid has (every other order keeps its
        # O(1) weight), so MUTATED_BIN stays visible at mmax of several hundred
        phi = 2.0 * torch.pi * torch.arange(nlon_of(c)) / nlon_of(c)
        amp = (0.5 + torch.rand(c.B, c.C, 1, 1, generator=g)) * c.wave1
        prof = 0.5 + torch.linspace(-1.0, 1.0, c.nlat)[:, None]
        x = x + amp * prof * torch.cos(phi + 0.3)
        # ... and a second wave of the same amplitude at a high order (fft_codelet_cases.py:
        # in the last KiB or two of spectrum that the inverse FFT stages per row)
        if getattr(c, "wave_hi", 0):
            x = x + amp * prof.flip(0) * torch.cos(c.wave_hi * phi + 1.1)
    if getattr(c, "offset", False):
        # every channel's mean 30 .. 100 standard deviations from zero, either sign
        u = torch.rand(c.C, generator=g)
        sign = 1.0 - 2.0 * (torch.arange(c.C) % 2)
        x = x + (sign * (30.0 + 70.0 * u))[None, :, None, None]
    return x


class _Transform:
    """A transform of the oracle by its definition on a given table (the oracle's own
    modules would build a max(lmax, mmax)^2 nlat recurrence table first)."""

    def __init__(self, tab, inverse, mmax, mutate=None, nlon=NLON):
        self.inverse, self.mmax, self.mutate, self.nlon = inverse, mmax, mutate, nlon
        self.weights = self.pct = tab

    def __call__(self, x):
        if self.inverse:
            return F._inverse(x, self.pct, self.nlon)
        a = F._forward(x, self.weights, self.mmax)
        if self.mutate is not None:
            m, p = self.mutate
            a = a.clone()
            if p is None:                 # the whole Fourier bin m
                a[0, :, :, m] *= MUTATION
            else:
                a[0, :, m + p::2, m] *= MUTATION
        return a


def _oracle(c, dtype, mutate=None):
    p = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in block_params(c).items()}
    x = block_input(c).to(dtype)
    sht = _Transform(table(c, False).to(dtype), False, c.mmax, mutate, nlon_of(c))
    isht = _Transform(table(c, True).to(dtype), True, c.mmax, nlon=nlon_of(c))
    cfg = block_cfg(c)
    with torch.no_grad():
        if cfg.has_mlp:                   # the whole block, no FiLM (fft_codelet_cases.py)
            return sfno_ref.block_forward(p, x, sht, isht, cfg)
        return sfno_ref.global_conv(p, x, x, sht, isht, cfg)


@functools.lru_cache(maxsize=None)
def block_reference(c):
    """fp64 (B, C, nlat, nlon) global_conv (block_forward for a case with an MLP) of the
    oracle."""
    return _oracle(c, torch.float64)


@functools.lru_cache(maxsize=None)
def block_e32(c):
    """max-abs distance of the oracle in fp32 (tables, parameters, input) from fp64."""
    return (_oracle(c, torch.float32).double() - block_reference(c)).abs().max().item()


def block_bar(c):
    flat = 1e-4 * max(1.0, block_reference(c).abs().max().item())
    return min(flat, BLOCK_E32_FACTOR * block_e32(c))


MUTATED_BLOCK = (1, 1)                    # (m, parity): the odd degrees of order 1, batch element 0


MUTATED_BIN = (1, None)                   # all degrees of order 1 (the FFT's bin 1), batch element 0


def block_mutation_shift(c, block=MUTATED_BLOCK):
    """How far the fp64 oracle moves when one (m, parity) block of batch element 0's forward
    coefficients is scaled by MUTATION."""
    return (_oracle(c, torch.float64, block) - block_reference(c)).abs().max().item()
