"""Regional and masked verification on the GPU (csrc/verify_regions.hip through
msfno_amd/verification.py, msfno_amd/regions.py and Rollout.verify) against the fp64
restatement on dense boolean membership (tests/verify_regions_util.py).

Kernel level: msfno_verify_region_sums at the shapes of tests/test_gpu_verify.py, for R = 1, 2,
8, 9 (the first with a second pass), 13 and 32 (bit 31) regions, each without a climatology,
with one for every slab and with the mixed map; outputs and workspace pre-filled with NaN, the
workspace exactly the advertised size in front of a guard.
  n, se, ae, pa2, ta2: 1e-5 relative; err, cross: 1e-5 of their magnitude sums -- the chain of
        a sum is that of msfno_verify_sums (a lane's share of a row plus one weighted add per
        row it visits, csrc/row_reduce.h; out-of-region pixels add an exact 0), so the bound
        tests/test_gpu_verify.py derives is unchanged.  Measured worst error / magnitude
        sum over the kernel cases: 1.9e-7.
Three bitwise contracts: a region of all ones has the six sums of msfno_verify_sums; a
region's sums do not move when NaN, +Inf or -Inf is written outside it (or, under skip_nan,
at skipped pixels); a missing truth is a cleared pix_bits bit.
Driver level: Rollout.verify(regions=) on the small fixture network against fp64 scoring of
run()'s outputs, 1e-3 of the magnitude sums, as tests/test_gpu_verify.py."""
import numpy as np
import pytest
import torch

import verify_regions_util as RU
import verify_util as VU
import workspace_guard as WG

pytestmark = pytest.mark.gpu
DEV = "cuda"

KERNEL_SHAPES = [(1, 1, 1, 1), (1, 1, 2, 8), (1, 2, 7, 9), (2, 3, 5, 12), (3, 7, 121, 250),
                 (1, 1, 3, 4100), (1, 73, 45, 90), (1, 2, 721, 1440)]
_ids = lambda s: "x".join(map(str, s))  # noqa: E731


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _tables(regions, device=DEV):
    return regions.tables(device)


def _rsums(prd, tar, w, tables, R, clim=None, slab=None, skip_nan=False, ws=None):
    """msfno_verify_region_sums on device tensors (any 16-byte phase); a NaN-filled output,
    and a NaN-filled workspace of exactly the advertised size in front of a guard unless a
    workspace is handed in."""
    from msfno_amd import _native as N
    B, C, H, W = prd.shape
    lib = N.lib()
    nbytes = lib.msfno_verify_regions_workspace_size(B * C, H, W, R)
    assert nbytes > 0 and nbytes % 4 == 0
    if ws is None:
        ws = WG.guarded(nbytes, 0xFF)
        assert torch.isnan(ws[:nbytes].view(torch.float32)).all()
    row, col, pix = tables
    sums = _nan(B, C, R, 7)
    N.check(lib.msfno_verify_region_sums(
        prd.data_ptr(), tar.data_ptr(), w.data_ptr(), N.ptr(clim), N.ptr(slab), row.data_ptr(),
        col.data_ptr(), N.ptr(pix), R, int(skip_nan), sums.data_ptr(), B * C, H, W,
        ws.data_ptr(), nbytes, N.stream_of(prd.device)), "msfno_verify_region_sums")
    WG.guard_intact(ws, nbytes)
    return sums, ws


def _gsums(prd, tar, w, clim=None, slab=None):
    """msfno_verify_sums: the unchanged global kernel."""
    from msfno_amd import _native as N
    B, C, H, W = prd.shape
    lib = N.lib()
    nbytes = lib.msfno_verify_workspace_size(B * C, H, W)
    ws = _nan(nbytes // 4)
    sums = _nan(B, C, 6)
    N.check(lib.msfno_verify_sums(prd.data_ptr(), tar.data_ptr(), w.data_ptr(), N.ptr(clim),
                                  N.ptr(slab), sums.data_ptr(), B * C, H, W, ws.data_ptr(),
                                  nbytes, N.stream_of(prd.device)), "msfno_verify_sums")
    return sums


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_sums(tag, got, want, tol=1e-5):
    """Every entry within tol of its magnitude sum (the sum itself for the non-negative
    ones, so that is tol relative); an exact zero where the magnitude sum is zero."""
    want, mag = want
    got = got.cpu().double()
    assert torch.isfinite(got).all(), tag
    assert torch.equal(want[..., RU.NONNEG], mag[..., RU.NONNEG])
    err = (got - want).abs()
    worst = (err / mag.clamp(min=1e-300)).max().item()
    print(f"{tag}: sums max err / magnitude sum {worst:.3e}")
    assert (err <= tol * mag).all(), (tag, worst)
    return worst


def _device_map(slab):
    return None if slab is None else torch.tensor(slab, dtype=torch.int32, device=DEV)


def _plus_zero(x):
    """every element is +0 (not -0)"""
    return bool((x.contiguous().view(torch.int32) == 0).all())


@pytest.mark.parametrize("R", RU.R_VALUES)
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=_ids)
def test_region_sums_kernel(shape, R):
    B, C, H, W = shape
    prd, tar, clim, w, _ = VU.problem(shape)
    regions, member = RU.region_problem(H, W, R)
    tb = _tables(regions)
    assert (tb[2] is None) == (R < 5)                  # both forms of pix_bits are covered
    p, t, wd, cd = prd.to(DEV), tar.to(DEV), w.to(DEV), clim.to(DEV)
    for name, rows, slab in VU.slab_maps(B, C):
        stack = None if rows is None else cd[rows].contiguous()
        sd = _device_map(slab)
        got, ws = _rsums(p, t, wd, tb, R, stack, sd)
        _check_sums(f"{shape} R={R} {name}", got, RU.want(shape, R, name))
        # every workspace word read was written by the call
        again, _ = _rsums(p, t, wd, tb, R, stack, sd, ws=ws)
        assert _bits_equal(got, again), name
        # region 0 is all ones: bitwise the six sums of the global kernel, beside the others
        assert _bits_equal(got[:, :, 0, 1:], _gsums(p, t, wd, stack, sd)), name
        if R > 1:
            assert _plus_zero(got[:, :, 1]), name      # the empty region: seven +0
        if name == "none":
            assert _plus_zero(got[..., 4:])
        if name == "mixed":
            miss = (torch.tensor(slab).reshape(B, C) < 0).to(DEV)
            assert _plus_zero(got[miss][..., 4:])


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=_ids)
def test_one_global_region_is_bitwise_the_global_kernel(shape):
    """One region with all bits set, skip_nan = 0 and 1 (nothing is missing): sums 1..6 are
    those of msfno_verify_sums, n is nlon sum(w)."""
    from msfno_amd.regions import Regions
    B, C, H, W = shape
    prd, tar, clim, w, _ = VU.problem(shape)
    p, t, wd, cd = prd.to(DEV), tar.to(DEV), w.to(DEV), clim.to(DEV)
    glob = Regions.boxes((H, W), {"global": (None, None, None, None)}) if H > 1 else \
        Regions(("global",), np.ones(H, np.uint32), np.ones(W, np.uint32))
    ones = Regions(("global",), np.full(H, 0xFFFFFFFF, np.uint32),
                   np.full(W, 0xFFFFFFFF, np.uint32), np.full((H, W), 0xFFFFFFFF, np.uint32))
    n = W * w.double().sum()
    for name, rows, slab in VU.slab_maps(B, C):
        stack = None if rows is None else cd[rows].contiguous()
        sd = _device_map(slab)
        base = _gsums(p, t, wd, stack, sd)
        for rg in (glob, ones):
            for skip in (False, True):
                got, _ = _rsums(p, t, wd, _tables(rg), 1, stack, sd, skip_nan=skip)
                assert _bits_equal(got[:, :, 0, 1:], base), (name, skip)
                assert ((got[:, :, 0, 0].cpu().double() - n).abs() <= 1e-5 * n).all()


def _shifted(t, k):
    """A contiguous device copy of the 4-byte tensor t that starts k words past a 16-byte
    boundary."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=DEV)
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * k
    return v


POISON = (float("nan"), float("inf"), float("-inf"))


def _poison(x, where, seed):
    """x with NaN, +Inf and -Inf (one third each) written where ``where`` holds."""
    g = torch.Generator().manual_seed(seed)
    kind = torch.randint(0, 3, x.shape, generator=g)
    vals = torch.tensor(POISON, dtype=x.dtype)[kind]
    return torch.where(where.expand(x.shape), vals, x)


@pytest.mark.parametrize("kt", [0, 1], ids=["vector", "scalar"])
def test_region_independence(kt):
    """A region's sums are bit-identical when everything outside it is NaN, +Inf or -Inf in
    prd, tar and clim.  13 x 37 slabs off the 16-byte grid: every column is a scalar head, a
    float4 body and a scalar tail in some row; whole rows and (for the empty region and the
    single pixel) whole slabs are poisoned.  Then, under skip_nan, the same at the skipped
    pixels."""
    shape = (2, 3, 13, 37)
    B, C, H, W = shape
    R = 13
    prd, tar, clim, w, _ = VU.problem(shape)
    regions, member = RU.region_problem(H, W, R)
    tb = _tables(regions)
    wd = w.to(DEV)
    slab = list(range(B * C))
    sd = _device_map(slab)

    def run(p, t, c, skip=False, with_clim=True):
        return _rsums(_shifted(p, 0), _shifted(t, kt), wd, tb, R,
                      _shifted(c, 0) if with_clim else None, sd if with_clim else None,
                      skip_nan=skip)[0]

    for with_clim in (False, True):
        base = run(prd, tar, clim, with_clim=with_clim)
        assert torch.isfinite(base).all()
        for r in (1, 2, 3, 4, 5, 8, R - 1):
            out = ~member[r]
            assert out.any() and (r == 1 or member[r].any())
            assert out.all(dim=1).any() or r not in (1, 2, 3, 5)   # a whole row outside
            got = run(_poison(prd, out, 10 + r), _poison(tar, out, 20 + r),
                      _poison(clim, out, 30 + r), with_clim=with_clim)
            assert _bits_equal(got[:, :, r], base[:, :, r]), (with_clim, r)
            # and the poison is seen where it belongs: the global region is not finite
            assert not torch.isfinite(got[:, :, 0, 1]).any()
            assert _bits_equal(got[:, :, 0, 0], base[:, :, 0, 0])   # n counts pixels
        # skip_nan: missing truths on 30 % of the pixels, a whole row and (without a
        # climatology) a whole slab; a poisoned climatology pixel is itself skipped where it
        # is NaN, so with one the missing set is common to the slabs
        g = torch.Generator().manual_seed(7)
        if with_clim:
            miss = (torch.rand(H, W, generator=g) < 0.3)
            miss[4] = True
            miss = miss.expand(shape)
        else:
            miss = (torch.rand(shape, generator=g) < 0.3)
            miss[:, :, 4] = True
            miss[1, 2] = True
        holes = torch.where(miss, torch.tensor(float("nan")), tar)
        base = run(prd, holes, clim, skip=True, with_clim=with_clim)
        assert torch.isfinite(base).all() and (with_clim or _plus_zero(base[1, 2]))
        got = run(_poison(prd, miss, 41), holes, _poison(clim, miss[0, 0], 42), skip=True,
                  with_clim=with_clim)
        assert _bits_equal(got, base), with_clim


@pytest.mark.parametrize("R", [2, 9])
def test_missing_value_is_a_mask(R):
    """skip_nan sums with NaN truths at a pixel set X are bitwise the sums of regions whose
    pix_bits exclude X, on inputs that are finite there (R = 2: the regions have no pix_bits
    of their own)."""
    from msfno_amd.regions import Regions
    shape = (2, 3, 13, 37)
    B, C, H, W = shape
    prd, tar, clim, w, _ = VU.problem(shape)
    regions, member = RU.region_problem(H, W, R)
    g = torch.Generator().manual_seed(11)
    X = torch.rand(H, W, generator=g) < 0.3
    X[6] = True
    pix = regions.pix_bits if regions.pix_bits is not None else \
        np.full((H, W), 0xFFFFFFFF, np.uint32)
    masked = Regions(regions.names, regions.row_bits, regions.col_bits,
                     np.where(X.numpy(), np.uint32(0), pix))
    holes = torch.where(X.expand(shape), torch.tensor(float("nan")), tar)
    p, wd, cd = prd.to(DEV), w.to(DEV), clim.to(DEV)
    sd = _device_map(list(range(B * C)))
    for stack, sl in ((None, None), (cd, sd)):
        a, _ = _rsums(p, holes.to(DEV), wd, _tables(regions), R, stack, sl, skip_nan=True)
        b, _ = _rsums(p, tar.to(DEV), wd, _tables(masked), R, stack, sl)
        assert torch.isfinite(a).all() and _bits_equal(a, b)
        want = RU.sums(prd.double(), tar.double(), w.double(), member & ~X,
                       None if stack is None else clim.double(), None if sl is None else
                       list(range(B * C)))
        _check_sums(f"missing = mask R={R}", a, want)


def test_skip_nan_against_the_restatement():
    """NaN truths on about 30 % of the pixels plus one all-NaN row and one all-NaN slab, NaN
    in the climatology of the slabs that have one."""
    from msfno_amd import verification as V
    shape = (3, 7, 121, 250)
    B, C, H, W = shape
    R = 13
    prd, tar, clim, w, _ = VU.problem(shape)
    regions, member = RU.region_problem(H, W, R)
    g = torch.Generator().manual_seed(3)
    miss = torch.rand(shape, generator=g) < 0.3
    miss[:, :, 17] = True
    miss[2, 4] = True
    holes = torch.where(miss, torch.tensor(float("nan")), tar)
    cmiss = torch.rand(clim.shape, generator=g) < 0.1
    choles = torch.where(cmiss, torch.tensor(float("nan")), clim)
    p, t, wd = prd.to(DEV), holes.to(DEV), w.to(DEV)
    for name, rows, slab in VU.slab_maps(B, C):
        stack = None if rows is None else choles[rows].contiguous()
        got = V.region_sums(p, t, wd, regions, None if stack is None else stack.to(DEV), slab,
                            skip_nan=True)
        assert got.shape == (B, C, R, 7)
        want = RU.sums(prd.double(), holes.double(), w.double(), member,
                       None if stack is None else stack.double(), slab, skip_nan=True)
        _check_sums(f"skip_nan {name}", got, want)
        assert _plus_zero(got[2, 4])                                # the all-NaN slab
        sc = V.finish_regions(got)
        for k in VU.NAMES:
            assert torch.isnan(getattr(sc, k)[2, 4]).all(), k
        has = torch.ones(B, C, dtype=torch.bool) if slab is None else \
            torch.tensor(slab).reshape(B, C) >= 0
        ref = RU.scores(want[0], has & (slab is not None))
        live = ~torch.isnan(ref["mse"])
        assert torch.equal(torch.isnan(sc.mse.cpu()), ~live)
        assert ((sc.mse.cpu().double() - ref["mse"])[live].abs() <= 3e-5 * ref["mse"][live]).all()
        assert torch.equal(torch.isnan(sc.acc.cpu()), torch.isnan(ref["acc"]))
        ok = ~torch.isnan(ref["acc"])
        assert ((sc.acc.cpu().double() - ref["acc"])[ok].abs() <= 3e-5).all()
    # without skip_nan a missing truth shows: the global region is NaN
    raw = V.region_sums(p, t, wd, regions)
    assert torch.isnan(raw[:, :, 0, 1]).all() and _plus_zero(raw[:, :, 1])


@pytest.mark.parametrize("kp,kt,kc,kcol,kpix",
                         [(1, 1, 1, 1, 1), (3, 3, 3, 3, 3), (2, 2, 2, 0, 3), (0, 2, 0, 1, 3),
                          (2, 2, 1, 2, 2), (0, 0, 0, 1, 0)])
def test_region_sums_on_views_off_the_16_byte_grid(kp, kt, kc, kcol, kpix):
    """prd, tar, clim, col_bits and pix_bits each at their own phase of the 16-byte grid: all
    equal, the vector path with 16-byte loads of the bit tables; the fields equal and the
    tables elsewhere, the float4 body with scalar table loads; the fields mixed, the scalar
    path ((2, 2, 1, ...): vector without a climatology, scalar with one)."""
    shape = (3, 7, 121, 250)
    R = 13
    prd, tar, clim, w, _ = VU.problem(shape)
    regions, _ = RU.region_problem(shape[2], shape[3], R)
    row, col, pix = _tables(regions)
    tb = (row, _shifted(col, kcol), _shifted(pix, kpix))
    p, t, c = _shifted(prd, kp), _shifted(tar, kt), _shifted(clim, kc)
    wd = w.to(DEV)
    got, _ = _rsums(p, t, wd, tb, R)
    _check_sums(f"phase {kp},{kt},-,{kcol},{kpix} none", got, RU.want(shape, R, "none"))
    assert _bits_equal(got[:, :, 0, 1:], _gsums(p, t, wd))
    sd = _device_map(list(range(21)))
    got, _ = _rsums(p, t, wd, tb, R, c, sd)
    _check_sums(f"phase {kp},{kt},{kc},{kcol},{kpix} full", got, RU.want(shape, R, "full"))
    assert _bits_equal(got[:, :, 0, 1:], _gsums(p, t, wd, c, sd))
    # the phase of the bit tables changes how they are loaded, never a sum
    same, _ = _rsums(p, t, wd, (row, col, pix), R, c, sd)
    assert _bits_equal(got, same)


@pytest.mark.parametrize("world", [2, 3])
def test_band_local_region_sums_add_up_to_the_whole_field(world):
    """A latitude-band rank passes its own rows, w[rows], clim[..., rows, :] and
    regions.rows(rows); the ranks' (B, C, R, 7) sums add up to the whole field's."""
    from msfno_amd import verification as V
    from msfno_amd.sfno.latband import band_partition, local_rows
    shape = (1, 3, 91, 180)
    R = 13
    prd, tar, clim, w, _ = VU.problem(shape)
    regions, _ = RU.region_problem(shape[2], shape[3], R)
    p, t, wd, cd = prd.to(DEV), tar.to(DEV), w.to(DEV), clim.to(DEV)
    row_start, _ = band_partition(world, shape[2], 45, 46)
    total = torch.zeros(1, 3, R, 7, dtype=torch.float64)
    seen = []
    for rank in range(world):
        rows = local_rows(world, rank, shape[2], row_start)
        seen += rows
        idx = torch.tensor(rows, device=DEV)
        total += V.region_sums(p[:, :, idx], t[:, :, idx], wd[idx], regions.rows(rows),
                               cd[:, idx]).cpu().double()
    assert sorted(seen) == list(range(shape[2]))
    _check_sums(f"world {world} bands", total, RU.want(shape, R, "full"))
    _check_sums(f"world {world} whole", V.region_sums(p, t, wd, regions, cd),
                RU.want(shape, R, "full"))


def _verifier_problem(R=9):
    shape = (2, 3, 5, 12)
    prd, tar, clim, w, _ = VU.problem(shape)
    regions, _ = RU.region_problem(5, 12, R)
    return shape, R, regions, prd.to(DEV), tar.to(DEV), clim.to(DEV).view(shape), w


def test_regional_verifier_update_captures_in_a_graph():
    from msfno_amd import verification as V
    (B, C, H, W), R, regions, sp, st, sc, w = _verifier_problem()
    sp, st, sc = sp.clone(), st.clone(), sc.clone()
    ver = V.RegionalVerifier(w, regions, 2, B, C, device=DEV)
    assert ver.sums.shape == (2, B, C, R, 7) and torch.isnan(ver.sums).all()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ver.update(0, sp, st, sc)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ver.update(0, sp, st, sc)
    sp.copy_(1.7 * sp + 0.25)
    st.copy_(0.5 * st - 0.125)
    sc.copy_(0.75 * sc + 0.5)
    ver.sums.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    ver.update(1, sp, st, sc)
    assert _bits_equal(ver.sums[0], ver.sums[1])
    _, member = RU.region_problem(H, W, R)
    _check_sums("graph replay", ver.sums[0],
                RU.sums(sp.cpu().double(), st.cpu().double(), w.double(), member,
                        sc.cpu().double().view(B * C, H, W), list(range(B * C))))


def test_regional_verifier_update_does_not_synchronise():
    from msfno_amd import verification as V
    (B, C, H, W), R, regions, p, t, c, w = _verifier_problem()
    ver = V.RegionalVerifier(w, regions, 3, B, C, skip_nan=True, device=DEV)
    slab = _device_map(VU.slab_maps(B, C)[2][2])
    stack = c[0].flip(0).contiguous()      # sample 0's slabs in reversed channel order
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ver.update(0, p, t)
        ver.update(1, p, t, c)
        ver.update(2, p, t, stack, slab)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for k, name in enumerate(("none", "full", "mixed")):
        _check_sums(f"slot {k}", ver.sums[k], RU.want((B, C, H, W), R, name))
    got = ver.scores(batch_mean=True)
    assert got.mse.shape == (3, C, R) and torch.isnan(got.acc[0]).all()
    assert torch.isnan(got.mse[:, :, 1]).all() and torch.isfinite(got.mse[:, :, 0]).all()
    ver.update(0, p, t.cpu(), c.cpu())     # host truths are copied over
    assert _bits_equal(ver.sums[0], ver.sums[1])


def test_refusals_of_the_python_layer():
    from msfno_amd import verification as V
    from msfno_amd.regions import Regions
    from msfno_amd.rollout import Rollout
    x = torch.zeros(1, 2, 4, 8, device=DEV)
    w = torch.ones(4, device=DEV)
    rg = Regions.boxes((4, 8), {"all": (None, None, None, None), "north": (0, 90, None, None)})
    other = Regions.boxes((5, 8), {"all": (None, None, None, None)})
    assert V.region_sums(x, x, w, rg).shape == (1, 2, 2, 7)
    with pytest.raises(ValueError):
        V.region_sums(x.cpu(), x.cpu(), w.cpu(), rg)                   # no CPU path
    with pytest.raises(ValueError, match="grid"):
        V.region_sums(x, x, w, other)
    with pytest.raises(ValueError):
        V.region_sums(x, x, w, "all")
    with pytest.raises(ValueError):
        V.region_sums(x, x, torch.ones(5, device=DEV), rg)             # one weight per row
    with pytest.raises(ValueError, match="requires grad"):
        V.region_sums(x, x.clone().requires_grad_(), w, rg)
    with pytest.raises(ValueError):
        V.region_sums(x, x, w, rg, None, [0, 1])                       # a map without a clim
    with pytest.raises(ValueError):
        V.RegionalVerifier("uniform", rg, 1, 1, 2, device=DEV).update(0, x[:, :1], x[:, :1])
    with pytest.raises(IndexError):
        V.RegionalVerifier("cosine", rg, 1, 1, 2, device=DEV).update(1, x, x)
    with pytest.raises(ValueError):
        V.RegionalVerifier(torch.ones(5), rg, 1, 1, 2, device=DEV)

    class Whole:
        world = 1

    class Sharded:
        world = 2

    with pytest.raises(ValueError, match="grid"):
        Rollout(Whole(), graph=False).verify(x, [x], 1, regions=other)
    with pytest.raises(ValueError, match="skip_nan"):
        Rollout(Whole(), graph=False).verify(x, [x], 1, skip_nan=True)
    with pytest.raises(ValueError, match="verifier"):
        Rollout(Whole(), graph=False).verify(
            x, [x], 1, regions=rg, verifier=V.Verifier("uniform", 4, 8, 1, 1, 2, device=DEV))
    with pytest.raises(NotImplementedError, match=r"regions\.rows\(rows\)"):
        Rollout(Sharded(), graph=False).verify(x, [x], 1, regions=rg)


# ---- the driver: Rollout.verify(regions=) on the small fixture network -----------------------

@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_rollout_verify_regions_on_the_fixture_network(graph):
    """5 steps, every = 2: steps 0, 2, 4 are scored per region, against fp64 scoring of the
    outputs of run(); then once through a regridder, with the regions of the destination
    grid and missing truths."""
    from msfno_amd import regrid as G
    from msfno_amd import verification as V
    from msfno_amd.losses import sphere_weights
    from test_gpu_verify import _rollout
    r, x0, stds = _rollout(graph)
    B, C, H, W = x0.shape
    R = 9
    regions, member = RU.region_problem(H, W, R)
    outs = [o.clone() for _, o in r.run(x0, 5)]
    scored = [0, 2, 4]
    truths = [(outs[i].flip(2).roll(W // 2, 3) + (k + 1) * stds).contiguous()
              for k, i in enumerate(scored)]
    clim = (0.5 * (outs[1][0] + outs[3][0].flip(1))).contiguous()          # (C, H, W)
    got = r.verify(x0, ((t, clim) for t in truths), 5, every=2, weights="cosine",
                   regions=regions)
    assert all(v.shape == (3, B, C, R) for v in got)
    w64 = torch.from_numpy(sphere_weights("cosine", H))
    has = torch.ones(B, C, dtype=torch.bool)
    for k, i in enumerate(scored):
        want = RU.sums(outs[i].cpu().double(), truths[k].cpu().double(), w64, member,
                       clim.cpu().double(), list(range(C)) * B)
        ref = RU.scores(want[0], has)
        live = ~torch.isnan(ref["mse"])
        assert torch.equal(torch.isnan(got.mse[k].cpu()), ~live)
        # mse = se / n: se within 1e-3 of itself, n within 1e-5
        assert ((got.mse[k].cpu().double() - ref["mse"])[live].abs()
                <= 1.1e-3 * ref["mse"][live]).all()
    # the raw sums through a verifier of one's own
    ver = V.RegionalVerifier("cosine", regions, 3, B, C, device=DEV)
    r.verify(x0, ((t, clim) for t in truths), 5, every=2, verifier=ver, regions=regions)
    for k, i in enumerate(scored):
        want = RU.sums(outs[i].cpu().double(), truths[k].cpu().double(), w64, member,
                       clim.cpu().double(), list(range(C)) * B)
        _check_sums(f"step {i}", ver.sums[k], want, tol=1e-3)
    # regridded: regions, truths and weights are those of the destination grid
    Ho, Wo = max(H // 3, 2), max(W // 3, 2)
    Rg = G.Regridder(G.Grid(H, W), G.Grid(Ho, Wo))
    dst, dmember = RU.region_problem(Ho, Wo, 5)
    rec, run = [], r.run

    def recording(*args, **kwargs):
        for i, y in run(*args, **kwargs):
            rec.append(y.clone())
            yield i, y

    r.run = recording
    g = torch.Generator().manual_seed(3)
    coarse = [torch.randn(B, C, Ho, Wo, generator=g) for _ in range(2)]
    coarse[1][:, :, 0, ::2] = float("nan")
    ver = V.RegionalVerifier("cosine", dst, 2, B, C, skip_nan=True, device=DEV)
    sc = r.verify(x0, [c.to(DEV) for c in coarse], 3, every=2, regrid=Rg, regions=dst,
                  verifier=ver)
    assert len(rec) == 3 and tuple(sc.rmse.shape) == (2, B, C, 5)
    wo = torch.from_numpy(sphere_weights("cosine", Ho))
    for k, i in enumerate((0, 2)):
        want = RU.sums(Rg(rec[i]).cpu().double(), coarse[k].double(), wo, dmember,
                       skip_nan=True)
        _check_sums(f"regrid step {i}", ver.sums[k], want, tol=1e-3)
    with pytest.raises(ValueError, match="grid"):
        r.verify(x0, coarse, 3, every=2, regrid=Rg, regions=regions)
