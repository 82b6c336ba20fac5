"""Spectral-MLP shape sweep: the cases, their CPU references and the fault-injected oracle,
shared by test_spectral_mlp_cases_host.py and test_gpu_spectral_mlp.py.

The complex MLP of the non-linear filter (SpectralAttentionS2: `layers` hidden layers
C -> Hs -> ... -> Hs with ComplexReLU(real), then the output layer Hs -> C, the same weights at
every (l, m) mode) is dispatched by shape in csrc/block_fwd.cpp run_filter:

  "3m"  C <= Hs: Gauss three-multiplication complex GEMMs, gemm_x3c (the x3h engine, the
        default) or gemm_x6c (MSFNO_SPEC_X3H=0) of csrc/gemm_x6c.hip: tiles of X6C_BM rows
        (64 where tiles_m tiles_n B < BM64_TILES) x X6C_BN columns, k-tiles of X6C_BK;
        activations ping-pong between Sb (even layers) and Sc (odd layers); a chain whose
        fixed x3h scales would drain more than X3H_RANGE_BITS of fp16 range takes gemm_x6c;
  "4m"  C > Hs, or MSFNO_SPEC_3M=0: the real-ified [[Wr, -Wi], [Wi, Wr]] GEMMs, layer 0
        through gemm_dense (C > Hs: fp32 rows in, planes and periodic ReLU out) or the
        split-input gemm_x6p (C <= Hs), later layers through gemm_x6p.

The columns of every GEMM are the Tp padded modes of SpecLayout (csrc/plan.cpp): per order
m the even degrees l = m, m + 2, ... in round8 slots, then the odd ones.

A case is (C, factor, layers, nlat, nlon, lmax, mmax, B) with Hs = int(factor C).  Weights
are seeded normals of standard deviation ci^-1/2 on real and imaginary part (the chain
neither vanishes nor overflows at eight layers), x is seeded randn, one seed per field so
that a batch is a prefix of a larger one.  want64 is oracle.sfno_ref.spectral_attention_s2 on
fp64 transforms and weights, want32 the same in fp32; the GPU bar is _bar of
test_gpu_ring_refill.py.  `chain` restates the oracle with one fault injected
(test_spectral_mlp_cases_host.py: without a fault it equals the oracle bit for bit, with one
it misses the bar by MUTATION_MARGIN)."""
import functools
import math
from collections import namedtuple

import torch

from oracle import sfno_ref

# ---- csrc constants: move the cases with them ------------------------------------------
X6C_BM, X6C_BN, X6C_BK = 128, 128, 16    # csrc/gemm_x6c.hip:33
X3C_BM64 = 64                            # gemm_x3c's small-grid row tile (gemm_x6c.hip:795, 809)
BM64_TILES = 2 * 256                     # tiles_m tiles_n B below this: 64-row tiles (gemm_x6c.hip:794, 808)
SPEC_PAD = 8                             # SpecLayout::build rounds each parity's degrees to 8 (plan.cpp:23-24)
MAX_LAYERS = 8                           # check_pair (block_fwd.cpp:293); SpecWeightsX6p::w[9],
#                                          DenseWs::spec[9], BlockBufs::Wexp[9] hold layers + 1 images
X3H_RANGE_BITS = 16.5                    # spec_x3h_range_ok (block_fwd.cpp:228)
MUTATION_MARGIN = 4                      # a fault moves the oracle by this many bars


def cdiv(a, b):
    return -(-a // b)


def round_up(a, b):
    return cdiv(a, b) * b


Layout = namedtuple("Layout", "T Tp ldT off Lpe Lp")


@functools.lru_cache(maxsize=None)
def spec_layout(lmax, mmax):
    """SpecLayout::build (csrc/plan.cpp:11-31) without an m-set mask."""
    T = Tp = 0
    off, Lpe, Lp = [], [], []
    for m in range(mmax):
        l = max(lmax - m, 0)
        Lpe.append(round_up((l + 1) // 2, SPEC_PAD))
        Lp.append(Lpe[m] + round_up(l // 2, SPEC_PAD))
        off.append(Tp)
        T += l
        Tp += Lp[m]
    return Layout(T, Tp, round_up(max(Tp, 8), 8), tuple(off), tuple(Lpe), tuple(Lp))


def column_modes(lmax, mmax):
    """[(l, m) or None] of the Tp columns (spec_col_inv, csrc/spectral.hip:923-930)."""
    L = spec_layout(lmax, mmax)
    cols = []
    for m in range(mmax):
        for u in range(L.Lp[m]):
            j = 2 * u if u < L.Lpe[m] else 2 * (u - L.Lpe[m]) + 1
            cols.append((m + j, m) if m + j < lmax else None)
    assert len(cols) == L.Tp
    return cols


def k_tiles(ci):
    return cdiv(ci, X6C_BK)              # gemm_x6c.hip:757 KT


def row_tiles(co, bm=X6C_BM):
    return round_up(co, X6C_BM) // bm    # gemm_x6c.hip:778 (Mp / 128), :795 (Mp / 64)


def col_tiles(Tp):
    return cdiv(Tp, X6C_BN)              # gemm_x6c.hip:779


def bm64(co, Tp, B):
    """gemm_x3c takes the 64-row kernels (gemm_x6c.hip:794, 808; default switches)."""
    return row_tiles(co) * col_tiles(Tp) * B < BM64_TILES


def chain_of(C, Hs):
    return "3m" if C <= Hs else "4m"     # block_fwd.cpp:312 (and :369 split_l0)


def x3h_range_bits(C, Hs, layers):
    """What spec_x3h_range_ok (block_fwd.cpp:230-234) compares with X3H_RANGE_BITS:
    log2(ci) / 2 + 1 bits of fp16 range per hidden layer."""
    return sum(0.5 * math.log2(C if l == 0 else Hs) + 1.0 for l in range(layers))


def engine_of(C, Hs, layers):
    """The engine of the chain at default switches: "x3h" (gemm_x3c), "x6c" (gemm_x6c) or,
    on the 4M chain, "x6p" (gemm_dense / gemm_x6p)."""
    if chain_of(C, Hs) == "4m":
        return "x6p"
    return "x3h" if x3h_range_bits(C, Hs, layers) <= X3H_RANGE_BITS else "x6c"


# ---- the cases --------------------------------------------------------------------------
Case = namedtuple("Case", "C factor layers nlat nlon lmax mmax B")
G13 = (13, 26, 12, 13)                   # Tp 184: two column tiles, the last of 56
G25 = (25, 50, 24, 25)                   # Tp 496: four column tiles, the last of 112


def _c(C=16, factor=2, layers=3, grid=G13, B=2):
    return Case(C, factor, layers, *grid, B)


def _tp128_pair():
    """The first (lmax, mmax <= lmax + 1) below lmax 32 whose Tp is a multiple of X6C_BN, if
    any: (9, 8), Tp 128 (none has mmax = lmax + 1)."""
    for lmax in range(2, 32):
        for mmax in range(2, lmax + 2):
            if spec_layout(lmax, mmax).Tp % X6C_BN == 0:
                return lmax, mmax
    return None


TP128 = _tp128_pair()

DEPTH = [_c(layers=n) for n in (
    1,      # layer 0 feeds the output layer straight from Sb
    2,      # Sb then Sc: one swap
    4,      # the profile stage clamp ST_SPEC_L0 + min(l, 3) acts (l = 3)
    5,      # 17 range bits: the first depth at hidden 32 that leaves x3h for gemm_x6c
    8,      # MAX_LAYERS: nine images fill w[9] / spec[9] / Wexp[9]; 27.5 range bits
)] + [
    _c(C=40, layers=4),   # 16.1 range bits: the last x3h chain under X3H_RANGE_BITS; Hs 80
    _c(C=64, layers=5),   # hidden 128: 22 bits (x3h measured 64 x the fp32 oracle's error here)
]
HIDDEN = [
    _c(C=24, factor=0.5),   # Hs 12 < C: the 4M chain, layer 0 through gemm_dense; ci 12 (k-tail 12)
    _c(C=24, factor=1),     # Hs = C: the boundary of C <= Hs, still 3M
    _c(C=24, factor=1.5),   # Hs 36: ragged k-tile of 4, 36 rows
    _c(C=16, factor=3),     # Hs 48: three k-tiles
]
CHAIN_4M = [
    _c(C=136, factor=0.5),            # Hs 68: layer 0 136 -> 68 on gemm_dense, two row tiles out
    _c(C=24, factor=0.5, layers=1),   # gemm_dense feeds the output layer
    _c(C=24, factor=0.5, layers=4),   # three gemm_x6p hidden layers behind it
]
RAGGED = [
    _c(C=4),      # a quarter of one k-tile; Hs 8
    _c(C=20),     # ci 20: k-tail 4; Hs 40: k-tail 8
    _c(C=72),     # ci 72: k-tail 8; Hs 144: a second row tile of 16 (64-row tiles: a third)
    _c(C=136),    # output layer: a second row tile with 8 rows; Hs 272: a third row tile of 16
]
COLUMNS = [
    _c(grid=(13, 26, 3, 4)),      # Tp 40 < 64
    _c(grid=(13, 26, 8, 9)),      # Tp 120: one ragged tile
    #                               (Tp 184, two tiles: every G13 case)
    _c(grid=G25),                 # Tp 496: four tiles, the last of 112
    _c(grid=(13, 26, 5, 9)),      # mmax > lmax + 1: orders 5 .. 8 without a degree
    _c(grid=(13, 26, 12, 6)),     # mmax < lmax: Tp 96
] + ([_c(grid=(13, 26, *TP128))] if TP128 and TP128[0] <= 12 else [])   # one exact tile
BATCH = [_c(B=1), _c(B=3)]
# every layer (64 -> 128 -> 128 -> 64) has one 128-row tile and four column tiles:
# tiles_m tiles_n B = 508 (64-row kernels) and 512 = BM64_TILES (128-row kernels)
BOUNDARY = [_c(C=64, layers=2, grid=G25, B=127), _c(C=64, layers=2, grid=G25, B=128)]

CASES = DEPTH + HIDDEN + CHAIN_4M + RAGGED + COLUMNS + BATCH + BOUNDARY


def case_id(c):
    return f"C{c.C}-f{c.factor}-L{c.layers}-{c.nlat}x{c.nlon}-l{c.lmax}-m{c.mmax}-B{c.B}"


IDS = [case_id(c) for c in CASES]
assert len(set(IDS)) == len(IDS)


def by_id(cid):
    return CASES[IDS.index(cid)]


# the subsets of the workspace and the engine tests
DEEPEST, LAST_X3H = DEPTH[4], DEPTH[5]
assert DEEPEST.layers == MAX_LAYERS
WORKSPACE_CASES = [DEPTH[0], DEEPEST, HIDDEN[0], RAGGED[1]]
# (LAST_X3H: the deepest chain that the gemm_x3c switches reach; DEEPEST runs on gemm_x6c)
ENGINE_CASES = [DEPTH[0], DEEPEST, LAST_X3H, HIDDEN[0], HIDDEN[1], RAGGED[1], RAGGED[3]]
ENGINES = [
    {"MSFNO_SPEC_X3H": "0"},
    {"MSFNO_SPEC_3M": "0"},
    {"MSFNO_SPEC_X6": "0"},
    {"MSFNO_GEMM": "f32"},
    {"MSFNO_X3C_BM64": "0"},
    {"MSFNO_X3C_BM64": "2"},
    {"MSFNO_X3C_L0_BM64": "0"},
]


def hidden(c):
    return int(c.factor * c.C)           # SpectralAttentionS2.hidden_size


def layer_dims(c):
    """[(ci, co)] of the layers + 1 GEMMs."""
    Hs = hidden(c)
    return [(c.C if l == 0 else Hs, c.C if l == c.layers else Hs) for l in range(c.layers + 1)]


def layout(c):
    return spec_layout(c.lmax, c.mmax)


def tile_products(c):
    """tiles_m tiles_n B of every layer at the 128-row tiles (what gemm_x3c compares with
    BM64_TILES)."""
    return [row_tiles(co) * col_tiles(layout(c).Tp) * c.B for _, co in layer_dims(c)]


# ---- inputs and references ----------------------------------------------------------------
def _seed(c):
    return 7919 * c.C + 131 * hidden(c) + 17 * c.layers + 3 * c.lmax + c.mmax


@functools.lru_cache(maxsize=None)
def weights(c):
    """([w_0 .. w_{layers-1}], wout), fp32 (ci, co, 2) each."""
    g = torch.Generator().manual_seed(_seed(c))
    ws = [torch.randn(ci, co, 2, generator=g) * ci ** -0.5 for ci, co in layer_dims(c)]
    return ws[:-1], ws[-1]


@functools.lru_cache(maxsize=None)
def _field(seed, b, shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(1000003 * (b + 1) + seed))


def input_of(c):
    """fp32 (B, C, nlat, nlon): field b does not depend on B."""
    return torch.stack([_field(_seed(c), b, (c.C, c.nlat, c.nlon)) for b in range(c.B)])


@functools.lru_cache(maxsize=None)
def _transforms(nlat, nlon, lmax, mmax, dtype):
    return sfno_ref.make_transforms(nlat, nlon, lmax, mmax, dtype=dtype)


def _oracle(c, dtype):
    ws, wout = weights(c)
    sht, isht = _transforms(c.nlat, c.nlon, c.lmax, c.mmax, dtype)
    with torch.no_grad():
        return sfno_ref.spectral_attention_s2(input_of(c).to(dtype), sht, isht,
                                              [w.to(dtype) for w in ws], wout.to(dtype)).double()


@functools.lru_cache(maxsize=None)
def want64(c):
    """fp64 (B, C, nlat, nlon); computed once, shared, never modified."""
    return _oracle(c, torch.float64)


@functools.lru_cache(maxsize=None)
def want32(c):
    return _oracle(c, torch.float32)


# ---- the oracle with one fault ------------------------------------------------------------
Fault = namedtuple("Fault", "kind layer")


def faults(c):
    """Every fault of the module docstring that case `c` can show: a k-tail needs
    ci % 16 != 0, a row tail co % 64 != 0, a skipped or stale layer a square neighbour, a
    column tail a second column tile."""
    dims, out = layer_dims(c), []
    for l, (ci, co) in enumerate(dims):
        if ci % X6C_BK:
            out.append(Fault("ktail", l))
        if co % X3C_BM64:
            out.append(Fault("rowtail", l))
        if 1 <= l < c.layers:
            out.append(Fault("skip", l))
        if l < c.layers:
            out.append(Fault("relu_imag", l))
        # layer l + 1 reads the buffer layer l read (layer l - 1's output): Sb / Sc parity
        if l + 1 <= c.layers and ci == co:
            out.append(Fault("stale", l))
        if col_tiles(layout(c).Tp) > 1:
            out.append(Fault("coltail", l))
    return out


@functools.lru_cache(maxsize=None)
def _coefficients(c):
    sht, _ = _transforms(c.nlat, c.nlon, c.lmax, c.mmax, torch.float64)
    with torch.no_grad():
        return torch.view_as_real(sht(input_of(c).double()))


def _last_tile_mask(c):
    """(lmax, mmax) bool: the modes whose column lies in the last column tile."""
    Tp = layout(c).Tp
    mask = torch.zeros(c.lmax, c.mmax, dtype=torch.bool)
    for t, lm in enumerate(column_modes(c.lmax, c.mmax)):
        if lm is not None and t >= X6C_BN * (col_tiles(Tp) - 1):
            mask[lm] = True
    return mask


def chain(c, fault=None):
    """spectral_attention_s2 of case `c` in fp64, layer by layer with the oracle's own
    contraction and activation, `fault` (a Fault, or None) injected."""
    ws, wout = weights(c)
    _, isht = _transforms(c.nlat, c.nlon, c.lmax, c.mmax, torch.float64)
    mats = [w.double() for w in ws] + [wout.double()]
    ins = [_coefficients(c)]             # ins[l]: what layer l reads, (B, ci, lmax, mmax, 2)
    with torch.no_grad():
        for l, w in enumerate(mats):
            ci, co = w.shape[:2]
            x = ins[l]
            hit = fault is not None and fault.layer == l
            if fault is not None and fault.kind == "stale" and fault.layer + 1 == l:
                x = ins[l - 1]
            if hit and fault.kind == "ktail":
                x = x.clone()
                x[:, ci - ci % X6C_BK:] = 0
            if hit and fault.kind == "skip":
                ins.append(x)
                continue
            y = sfno_ref.compl_mul2d_fwd_c(x, w)
            if l < c.layers:
                y = torch.view_as_real(sfno_ref.complex_relu_real(torch.view_as_complex(y)))
                if hit and fault.kind == "relu_imag":
                    y = y.clamp_min(0.0)
            if hit and fault.kind == "rowtail":
                y = y.clone()
                y[:, co - co % X3C_BM64:] = 0
            if hit and fault.kind == "coltail":
                y = y * (~_last_tile_mask(c))[None, None, :, :, None]
            ins.append(y)
        return isht(torch.view_as_complex(ins[-1].contiguous())).double()
