"""The fragment-order planes of the spectral MLP (csrc/gemm_x6c.hip): a hidden layer stores
its MFMA accumulators as they stand, [tn][kt][matrix-plane][cb][lane][8], the next layer
reads them back as B fragments, and its weight image carries the permutation of the
contraction index that this implies (x6c_kperm: k position kp of k-tile kt is channel
16 kt + pi(kp)).  The sweep of test_gpu_spectral_mlp.py says that something is wrong; this
file says which index.

Weights that move no channel: layers = 2, w0 the identity C -> Hs (1 + 0i on the diagonal,
hidden channels >= C zero), w1 = diag(d_k) with d_k = 1 + k / Hs, distinct, positive and
real, wout the identity on the first C rows.  Output channel c is then d_c times the twice
rectified input channel c and nothing else, so

  * a wrong pi, or t (the two k-tiles of a 32-row block), or kt (the k-tile of a row block)
    sends channel c through another d_k, or to another channel, or to a zero row: an O(1)
    error in the channels of one k-tile position;
  * a wrong cb (the 32-column block of a tile) or tn moves columns: an O(1) error in the
    modes (l, m) of those columns.

Every case is held to the fp64 oracle (oracle.sfno_ref.spectral_attention_s2) at the bar of
the sweep (_bar of test_gpu_ring_refill.py).  A failure names the worst output channel and,
from the fp64 forward transform of the error field, the worst mode with its column, column
tile, 32-column block and lane.

Shapes, the smallest at which each index can go wrong (G13: Tp 184, a ragged second column
tile; G25: Tp 496, four column tiles, every cb):
  C 16, Hs 48, B 1   three k-tiles: t = 1 of the second 32-row block is pad
  C 72, Hs 144, B 2  a second 128-row tile (kt 8); 64-row tiles: a third
  C 16, Hs 32, B 1   one full 32-row block, both t; on G13 and on G25
At default switches these grids take the x3h engine on 64-row tiles; one child process each
runs the same cases on the 128-row, three-stage kernels (MSFNO_X3C_BM64=0) and on the x6
engine (MSFNO_SPEC_X3H=0): the switches are read once per process."""
import functools
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    _repo = os.path.dirname(HERE)
    for _d in (HERE, _repo, os.path.join(_repo, "modulated-spherical-fourier-neural-operator_amd")):
        sys.path.insert(0, _d)

import numpy as np  # noqa: E402
import pytest  # noqa: E402
import torch  # noqa: E402

import spectral_mlp_cases as M  # noqa: E402
from oracle import sfno_ref  # noqa: E402
from test_gpu_ring_refill import _bar  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = [
    M.Case(16, 3, 2, *M.G13, 1),
    M.Case(72, 2, 2, *M.G13, 2),
    M.Case(16, 2, 2, *M.G13, 1),
    M.Case(16, 2, 2, *M.G25, 1),
]
IDS = [M.case_id(c) for c in CASES]
SWITCHES = [{}, {"MSFNO_X3C_BM64": "0"}, {"MSFNO_SPEC_X3H": "0"}]
SWITCH_IDS = ["default", "rows128", "x6"]


@functools.lru_cache(maxsize=None)
def _weights(c):
    """([w0, w1], wout), fp32 (ci, co, 2): identity, diag(1 + k / Hs), identity."""
    C, Hs = c.C, M.hidden(c)
    w0 = torch.zeros(C, Hs, 2)
    w0[torch.arange(C), torch.arange(C), 0] = 1.0
    w1 = torch.zeros(Hs, Hs, 2)
    w1[torch.arange(Hs), torch.arange(Hs), 0] = 1.0 + torch.arange(Hs, dtype=torch.float32) / Hs
    wout = torch.zeros(Hs, C, 2)
    wout[torch.arange(C), torch.arange(C), 0] = 1.0
    return [w0, w1], wout


@functools.lru_cache(maxsize=None)
def _want(c, dtype):
    """the oracle in `dtype`, as fp64; computed once, shared, never modified"""
    ws, wout = _weights(c)
    sht, isht = M._transforms(c.nlat, c.nlon, c.lmax, c.mmax, dtype)
    with torch.no_grad():
        return sfno_ref.spectral_attention_s2(M.input_of(c).to(dtype), sht, isht,
                                              [w.to(dtype) for w in ws], wout.to(dtype)).double()


def _gpu(c):
    from msfno_amd.harmonics import InverseRealSHT, RealSHT
    from msfno_amd.sfno.sfnonet import SpectralFilterLayer
    sht = RealSHT(c.nlat, c.nlon, lmax=c.lmax, mmax=c.mmax, grid="equiangular").float()
    isht = InverseRealSHT(c.nlat, c.nlon, lmax=c.lmax, mmax=c.mmax, grid="equiangular").float()
    sht.weights = sht.weights * 1e5      # as oracle.sfno_ref.make_transforms
    isht.pct = isht.pct / 1e5
    f = SpectralFilterLayer(sht, isht, c.C, filter_type="non-linear", hidden_size_factor=c.factor,
                            spectral_layers=c.layers).filter
    ws, wout = _weights(c)
    assert f.hidden_size == M.hidden(c) and len(f.w) == len(ws)
    with torch.no_grad():
        for p, w in zip(f.w, ws):
            p.copy_(w)
        f.wout.copy_(wout)
    f = f.eval().to(DEV)
    with torch.no_grad():
        return f(M.input_of(c).to(DEV)).cpu()


def _where(c, got):
    """the worst channel of the output error, and the worst mode of its fp64 forward
    transform with the place of that mode's column in the tiled planes"""
    err = got.double() - _want(c, torch.float64)
    per_c = err.abs().amax(dim=(0, 2, 3))
    ch = int(per_c.argmax())
    sht, _ = M._transforms(c.nlat, c.nlon, c.lmax, c.mmax, torch.float64)
    with torch.no_grad():
        spec = sht(err).abs().amax(dim=(0, 1))           # (lmax, mmax)
    l, m = divmod(int(spec.argmax()), spec.shape[1])
    cols = M.column_modes(c.lmax, c.mmax)
    col = cols.index((l, m)) if (l, m) in cols else -1
    Hs = M.hidden(c)
    return (f"worst channel {ch} (k-tile {ch // 16}, position {ch % 16}; d = {1 + ch / Hs:.4f}; "
            f"error {per_c[ch].item():.3e}); worst mode l {l} m {m}: column {col} = column tile "
            f"{col // M.X6C_BN}, 32-column block {col % M.X6C_BN // 32}, lane {col % 32} (+ 32 h)")


@functools.lru_cache(maxsize=None)
def _outputs(switch_id):
    """{case id: output} under the switches; the default ones in this process, the others
    in one child process each"""
    env_add = SWITCHES[SWITCH_IDS.index(switch_id)]
    if not env_add:
        return {i: _gpu(c) for i, c in zip(IDS, CASES)}
    import tempfile
    env = {k: v for k, v in os.environ.items() if k not in {k2 for e in SWITCHES for k2 in e}}
    env.update(env_add)
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "frag.npz")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, cwd=HERE,
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-3000:]
        z = np.load(out)
        return {i: torch.from_numpy(z[i]) for i in IDS}


@pytest.mark.parametrize("switch_id", SWITCH_IDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_identity_chain_keeps_every_channel_and_column(case, switch_id):
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    got = _outputs(switch_id)[M.case_id(case)]
    want64, want32 = _want(case, torch.float64), _want(case, torch.float32)
    assert got.shape == want64.shape
    what = f"{M.case_id(case)} [{switch_id}]"
    try:
        assert torch.isfinite(got).all(), what
        _bar(got, want64, want32, what)
    except AssertionError as e:
        raise AssertionError(f"{e}\n{what}: {_where(case, torch.nan_to_num(got))}") from None


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    import conftest  # noqa: F401  (puts the package on sys.path)
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    np.savez(sys.argv[1], **{i: _gpu(c).numpy() for i, c in zip(IDS, CASES)})
