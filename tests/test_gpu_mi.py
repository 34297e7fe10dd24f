"""The mutual-information cost on the GPU: csrc/sim_mi.hip against tests/mi_ref.py (the numpy restatement of the header's
"Mutual information" section), and register(similarity='mi') on the tilted scene of tests/drr_ref.py.

Bars.  hist: equal to the model's int64, bit for bit (integers).  cost: 1e-11 absolute -- at most 4096 terms of magnitude
<= 1/e, a few-ulp log and a reordered float64 sum stay below 1e-12; ten times that.  The table ell: 1e-13 absolute (|log| <= 30,
one ulp of which is 3.6e-15; the kernel's log and numpy's may each be an ulp or two off).  d_moving: exact zeros where the
definition says so, and two checks elsewhere.  (i) Against the kernel's own table: d_moving is float32(-(s / n) (ell[a + 1][b] -
ell[a][b])) of the table dfl_sim_mi_bwd wrote, bit for bit -- one float32 rounding of a float64 value and nothing else.  (ii) Against
the model: |got - want| <= 2^-21 max|want| + (s / n) 4 TABLE_BAR per view.  The second term is the reference's own error: both
sides difference two table entries that each carry a log error of a few 1e-15.  Without it the bound cannot be met where the
true derivative is zero and `want` itself is nothing but that rounding noise -- the constant view: max|want| = 1.7e-18 at 45 x 61,
bins (5, 13), against a kernel value that differs from it by as much -- and it changes nothing elsewhere: on the other views it is
below 1e-6 of the first term.  Registration: the bin count and
the bar of tests/golden/floors/mi.json (tests/mi_floor.py: the model alone ends at 0.079 px with 16 bins, so the bar is
reg_floor.PIXEL_BAR = 0.25 px).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'examples'))
import drr_ref as D  # noqa: E402
import mi_floor as MF  # noqa: E402
import mi_ref as M  # noqa: E402
import reg_ref as R  # noqa: E402
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, drr, preprocess as pp, register as reg  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
SIZES = R.SIM_SIZES + ((1, 1), (2, 1031), (300, 9))
BINS = ((8, 8), (32, 32), (64, 64), (2, 2), (5, 13), (64, 2))
COST_BAR, ADJ_BAR, TABLE_BAR = 1e-11, 2.0 ** -21, 1e-13
_CACHE = {}


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _images(H, W):
    """(fixed, moving [6], (lo, hi)) of a size: reg_ref.sim_images and the range of tests/mi_floor.py; shared, never written to."""
    if (H, W) not in _CACHE:
        fixed, moving = R.sim_images(H, W)
        _CACHE[H, W] = fixed, moving, MF.sim_range(moving)
    return _CACHE[H, W]


def _check_adjoint(got, want, ell, fbin, m, lo, hi, Bm, what):
    """got float32 [H, W] against the model's float64 `want` and against the table `ell` [Bm, Bf] the kernel wrote."""
    on = fbin != M.SKIP
    zero = ~on | ~((m > lo) & (m < hi))
    assert not got[zero].any() and not want[zero].any(), what
    n = int(on.sum())
    if n == 0:
        return 0.0
    s, _ = M.scale(lo, hi, Bm)
    a, _, _ = M.weights(m, lo, hi, Bm)
    b = np.where(on, fbin, 0).astype(np.int64)
    own = np.where(zero, 0.0, -(float(s) / n) * (ell[a + 1, b] - ell[a, b])).astype(np.float32)
    assert np.array_equal(got, own), (what, float(np.abs(got - own).max()))
    top, floor = float(np.abs(want).max()), float(s) / n * 4.0 * TABLE_BAR
    err = float(np.abs(got.astype(np.float64) - want).max())
    assert err <= ADJ_BAR * top + floor, (what, err, top, floor)
    return err / top if top > 1e6 * floor else 0.0


# ---- 1. histogram, cost and adjoint against the model ------------------------------------------------------------------
@pytest.mark.parametrize('mask_name', ['none', 'ragged', 'empty'])
@pytest.mark.parametrize('size', SIZES)
def test_hist_cost_and_adjoint_match_the_model(size, mask_name):
    H, W = size
    fixed, moving, (lo, hi) = _images(H, W)
    mask = R.sim_masks(H, W)[mask_name]
    d_fixed, d_mask, d_moving = _dev(fixed), None if mask is None else _dev(mask), _dev(moving)
    worst_c = worst_g = 0.0
    for Bf, Bm in BINS:
        sim = reg.MISimilarity(d_fixed, d_mask, views=6, bins=(Bf, Bm), moving_range=(lo, hi))
        fbin, info = M.prepare(fixed, mask, Bf)
        assert np.array_equal(sim.fbin.cpu().numpy(), fbin) and sim.info.cpu().numpy().tolist() == info.tolist(), (Bf, Bm)
        got_t = sim.cost(d_moving)
        assert got_t.dtype == torch.float64 and tuple(got_t.shape) == (6,) and got_t.is_cuda
        hist = sim.hist.cpu().numpy()
        want_h = np.stack([M.hist(v, fbin, lo, hi, Bf, Bm) for v in moving])
        assert hist.dtype == np.int64 and torch.equal(sim.hist.cpu(), torch.from_numpy(want_h)), (Bf, Bm)
        assert (hist.sum((1, 2)) == M.UNIT * int(info[0])).all()
        want_c = np.array([-M.mi(h) for h in want_h])
        worst_c = max(worst_c, float(np.abs(got_t.cpu().numpy() - want_c).max()))
        assert np.abs(got_t.cpu().numpy() - want_c).max() <= COST_BAR, (Bf, Bm)
        if info[0] == 0:
            assert (got_t == 0.0).all()
        else:
            assert abs(got_t[2].item()) <= COST_BAR                 # the constant view
        # the adjoint: the cost bits of the forward entry point, the same histogram, the model's table and gradient
        cost2, adj = sim.cost_and_adjoint(d_moving)
        assert torch.equal(cost2, got_t) and torch.equal(sim.hist.cpu(), torch.from_numpy(want_h))
        assert adj.dtype == torch.float32 and tuple(adj.shape) == (6, H, W)
        ell = sim.ell.cpu().numpy()
        np.testing.assert_allclose(ell, np.stack([M.table(h) for h in want_h]), rtol=0, atol=TABLE_BAR)
        adj = adj.cpu().numpy()
        for v in range(6):
            worst_g = max(worst_g, _check_adjoint(adj[v], M.adjoint(moving[v], fbin, lo, hi, Bf, Bm), ell[v], fbin, moving[v], lo, hi, Bm, (Bf, Bm, v)))
    print('MI %d x %d mask %s: %d counted; over %d bin pairs the largest |cost error| %.3e (bar %.0e), adjoint error %.3e of the largest entry '
          '(bar %.3e; views whose gradient is rounding noise aside)' % (H, W, mask_name, int(info[0]), len(BINS), worst_c, COST_BAR, worst_g, ADJ_BAR))


# ---- 2. edge values ----------------------------------------------------------------------------------------------------
def test_edge_values_in_one_image():
    lo, hi, Bf, Bm = np.float32(1.0), np.float32(3.0), 4, 5           # s = 2: x = 2 (m - 1)
    edge = [lo, hi, 0.5, -1e30, 7.0, 1e30, np.nan, np.inf, -np.inf, 1.5, 2.0, 2.5,     # the ends, beyond them, NaN, inf, integer x
            1.0 + 0.99995 / 2, np.nextafter(hi, np.float32(0)), np.nextafter(lo, np.float32(9)), 1.3, 2.71]   # q = 4096; next to the ends
    m = np.array([edge + edge[::-1]], np.float32)
    H, W = m.shape
    fixed = np.arange(W, dtype=np.float32)[None] % 7
    fixed[0, 5] = np.nan                                              # one pixel that is not counted
    a, _, q = M.weights(m, lo, hi, Bm)
    assert q.max() == M.UNIT and q.min() == 0 and a.max() == Bm - 2 and (q[0, [9, 10, 11]] == 0).all() and a[0, [9, 10, 11]].tolist() == [1, 2, 3]
    assert q[0, 12] == M.UNIT and a[0, 12] == 0
    sim = reg.MISimilarity(_dev(fixed), None, views=2, bins=(Bf, Bm), moving_range=(lo, hi))
    fbin, info = M.prepare(fixed, None, Bf)
    assert np.array_equal(sim.fbin.cpu().numpy(), fbin) and info[0] == W - 1
    mv = _dev(np.concatenate([m, m[:, ::-1]])[:, None].reshape(2, H, W))
    cost, adj = sim.cost_and_adjoint(mv)
    want = np.stack([M.hist(v, fbin, lo, hi, Bf, Bm) for v in mv.cpu().numpy()])
    assert torch.equal(sim.hist.cpu(), torch.from_numpy(want)) and int(want[0].sum()) == M.UNIT * (W - 1)
    assert np.abs(cost.cpu().numpy() - [-M.mi(h) for h in want]).max() <= COST_BAR
    for v in range(2):
        mm = mv[v].cpu().numpy()
        _check_adjoint(adj[v].cpu().numpy(), M.adjoint(mm, fbin, lo, hi, Bf, Bm), sim.ell[v].cpu().numpy(), fbin, mm, lo, hi, Bm, v)
    assert adj[0].any() and adj[0, 0, 0].item() == 0.0 and adj[0, 0, 1].item() == 0.0 and adj[0, 0, 5].item() == 0.0


# ---- 3. the 64-bit path ------------------------------------------------------------------------------------------------
def test_a_bin_beyond_32_bits():
    H, W = 1024, 1025
    n = H * W
    assert M.UNIT * n > 2 ** 32
    fixed = torch.full((H, W), 2.0, device=DEV)
    sim = reg.MISimilarity(fixed, None, views=3, bins=(8, 32), moving_range=(0.0, 31.0))
    assert sim.info.cpu().numpy().tolist() == [n, 2.0, 2.0, 0.0] and not sim.fbin.any()
    mv = torch.full((3, H, W), 5.0, device=DEV)
    mv[1] = 5.25                                                     # a quarter of every pixel in the next bin
    want = np.zeros((3, 32, 8), np.int64)
    want[0, 5, 0] = want[2, 5, 0] = M.UNIT * n
    want[1, 5, 0], want[1, 6, 0] = 3072 * n, 1024 * n
    one = sim.cost(mv[:1])
    assert torch.equal(sim.hist[:1].cpu(), torch.from_numpy(want[:1])) and one.item() == 0.0
    three = sim.cost(mv)
    assert torch.equal(sim.hist.cpu(), torch.from_numpy(want)) and (three == 0.0).all()


# ---- 4. batch independence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [(45, 61), (2, 1031)])
def test_a_view_has_the_same_bits_alone_and_in_any_batch(size):
    H, W = size
    fixed, moving, (lo, hi) = _images(H, W)
    seven = np.concatenate([moving, (moving[4:5] * np.float32(0.5) + moving[5:6] * np.float32(0.5))])
    order = [3, 6, 0, 5, 1, 4, 2]
    sim = reg.MISimilarity(_dev(fixed), _dev(R.sim_masks(H, W)['ragged']), views=7, bins=(32, 16), moving_range=(lo, hi))
    mv = _dev(seven)
    cost, adj = sim.cost_and_adjoint(mv)
    hist = sim.hist.clone()
    again, adj2 = sim.cost_and_adjoint(mv)
    assert torch.equal(again, cost) and torch.equal(adj2, adj) and torch.equal(sim.hist, hist)
    assert torch.equal(sim.cost(mv), cost) and torch.equal(sim.hist, hist)
    pc, pa = sim.cost_and_adjoint(mv[order].contiguous())
    assert torch.equal(pc, cost[order]) and torch.equal(pa, adj[order]) and torch.equal(sim.hist, hist[order])
    for v in range(7):
        c1, a1 = sim.cost_and_adjoint(mv[v:v + 1].clone())
        assert torch.equal(c1, cost[v:v + 1]) and torch.equal(a1, adj[v:v + 1]) and torch.equal(sim.hist[0], hist[v]), v


# ---- 5. a bank ---------------------------------------------------------------------------------------------------------
def test_bank_void_views_and_the_others():
    H, W = 17, 70
    fixed, moving, (lo, hi) = _images(H, W)
    bank = np.stack([fixed, np.float32(2) - fixed[::-1].copy(), np.sqrt(fixed + np.float32(1))]).astype(np.float32)
    masks = np.stack([np.full((H, W), 1, np.uint8), R.sim_masks(H, W)['ragged'], R.sim_masks(H, W)['empty']])
    sim = reg.MISimilarity(_dev(bank), _dev(masks), views=6, bins=16)
    singles = [reg.MISimilarity(_dev(bank[f]), _dev(masks[f]), views=6, bins=16, moving_range=(lo, hi)) for f in range(3)]
    mv = _dev(moving)
    assert torch.isnan(sim.cost(mv)).all() and not sim.hist.any()           # no range yet: every view is void
    sim.set_range(lo, hi)
    for f in range(3):
        assert torch.equal(sim.fbin[f], singles[f].fbin) and torch.equal(sim.info[f], singles[f].info)
    want = [singles[f].cost_and_adjoint(mv) + (singles[f].hist.clone(),) for f in range(3)]
    # fixed_of on the device is not checked: entries outside [0, F) are void views
    fixed_of = torch.tensor([0, -1, 3, 1], dtype=torch.int32, device=DEV)
    cost, adj = sim.cost_and_adjoint(mv[:4], fixed_of)
    assert torch.isnan(cost[1:3]).all() and not adj[1:3].any() and not sim.hist[1:3].any() and not sim.ell[1:3].any()
    for v, f in ((0, 0), (3, 1)):
        assert torch.equal(cost[v], want[f][0][v]) and torch.equal(adj[v], want[f][1][v]) and torch.equal(sim.hist[v], want[f][2][v])
    assert torch.equal(sim.cost(mv[:4], fixed_of)[[0, 3]], cost[[0, 3]])
    with pytest.raises(nat.DflError, match='fixed_of holds'):
        sim.cost(mv[:4], [0, -1, 3, 1])                                     # a sequence is checked on the host
    # one image with hi == lo and one with NaN in its range: their views are void, image 2's are not
    sim.set_range(torch.tensor([[float(lo), float(lo)], [float('nan'), float(hi)], [float(lo), float(hi)]], device=DEV))
    which = [0, 2, 1, 2, 0, 1]
    cost, adj = sim.cost_and_adjoint(mv, which)
    for v, f in enumerate(which):
        if f == 2:
            assert torch.equal(cost[v], want[2][0][v]) and torch.equal(adj[v], want[2][1][v]) and torch.equal(sim.hist[v], want[2][2][v])
        else:
            assert torch.isnan(cost[v]) and not adj[v].any() and not sim.hist[v].any()
    assert torch.equal(sim.cost(mv)[:1].isnan(), torch.tensor([True], device=DEV))      # fixed_of None: image 0
    with pytest.raises(nat.DflError, match='mi_range'):
        sim.set_range(np.array([[0, 1], [1, 1], [0, 2]]))
    with pytest.raises(nat.DflError, match='moving range'):
        sim.set_range(torch.zeros((2, 2), device=DEV))
    with pytest.raises(nat.DflError, match='single image'):
        singles[0].cost(mv, [0] * 6)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    H, W = 45, 61
    fixed, moving, (lo, hi) = _images(H, W)
    sim = reg.MISimilarity(_dev(fixed), None, views=6, bins=8, moving_range=(lo, hi))
    mv = _dev(moving)
    L = nat.lib()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    S = -7
    cost = torch.full((6,), float(S), dtype=torch.float64, device=DEV)
    hist = torch.full((6, 8, 8), S, dtype=torch.int64, device=DEV)
    ell = torch.full((6, 8, 8), float(S), dtype=torch.float64, device=DEV)
    adj = torch.full((6, H, W), float(S), device=DEV)
    fbin = torch.full((H, W), 77, dtype=torch.uint8, device=DEV)
    info = torch.full((4,), float(S), dtype=torch.float64, device=DEV)
    common = dict(moving=mv.data_ptr(), fbin=sim.fbin.data_ptr(), info=sim.info.data_ptr(), mrange=sim.mrange.data_ptr(), fixed_of=None,
                  hist=hist.data_ptr(), cost=cost.data_ptr(), V=6, H=H, W=W, F=1, Bf=8, Bm=8)
    bad = [dict(moving=None), dict(fbin=None), dict(info=None), dict(mrange=None), dict(hist=None), dict(cost=None), dict(H=0), dict(W=-1),
           dict(H=65536, W=32768), dict(V=0), dict(V=65536), dict(F=0), dict(F=65536), dict(F=40000, H=300, W=300), dict(Bf=1), dict(Bf=65),
           dict(Bm=1), dict(Bm=65)]
    for kw in bad:
        a = nat.SimMiArgs(**dict(common, **kw))
        assert L.dfl_sim_mi(C.addressof(a), stream) == -1 and b'dfl_sim_mi:' in L.dfl_last_error(), (kw, L.dfl_last_error())
    for kw in bad + [dict(ell=None), dict(d_moving=None)]:
        a = nat.SimMiBwdArgs(**dict(dict(common, ell=ell.data_ptr(), d_moving=adj.data_ptr()), **kw))
        assert L.dfl_sim_mi_bwd(C.addressof(a), stream) == -1 and b'dfl_sim_mi_bwd' in L.dfl_last_error(), (kw, L.dfl_last_error())
    for kw in (dict(fixed=None), dict(fbin=None), dict(info=None), dict(H=0), dict(W=0), dict(H=65536, W=32768), dict(Bf=1), dict(Bf=65)):
        a = nat.SimMiPrepareArgs(**dict(dict(fixed=sim.fixed.data_ptr(), mask=None, fbin=fbin.data_ptr(), info=info.data_ptr(), H=H, W=W, Bf=8), **kw))
        assert L.dfl_sim_mi_prepare(C.addressof(a), stream) == -1 and b'dfl_sim_mi_prepare' in L.dfl_last_error(), (kw, L.dfl_last_error())
    torch.cuda.synchronize()
    assert (cost == S).all() and (hist == S).all() and (ell == S).all() and (adj == S).all() and (fbin == 77).all() and (info == S).all()
    a = nat.SimMiBwdArgs(**dict(common, ell=ell.data_ptr(), d_moving=adj.data_ptr()))       # the same block, unchanged, runs
    assert L.dfl_sim_mi_bwd(C.addressof(a), stream) == 0
    want_c, want_a = sim.cost_and_adjoint(mv)
    assert torch.equal(cost, want_c) and torch.equal(adj, want_a) and torch.equal(hist, sim.hist) and torch.equal(ell, sim.ell)
    with pytest.raises(nat.DflError, match='views'):
        sim.cost(torch.zeros((7, H, W), device=DEV))
    with pytest.raises(nat.DflError, match='GPU'):
        sim.cost(torch.zeros((1, H, W)))
    with pytest.raises(nat.DflError, match='the mask'):
        reg.MISimilarity(_dev(fixed), _dev(np.ones((H, W + 1), np.uint8)))
    with pytest.raises(nat.DflError, match='mi_range'):
        sim.set_range(1.0, 1.0)


# ---- 7. registration ---------------------------------------------------------------------------------------------------
def _scene():
    if 'scene' not in _CACHE:
        import reg_floor as FL
        S = D.scene('tilted')
        _CACHE['scene'] = S, drr.Volume(_dev(S['mu']), _dev(S['lab'])), _dev(FL.fixed_image(S).astype(np.float32))
    return _CACHE['scene']


def _geom(S, poses):
    named = dict(zip(drr.POSES, poses))
    return drr.Geometry(S['K'], S['E'], named, S['I2P'], np.eye(3), drr.default_objects(S['E'], named, S['I2P']),
                        drr.Grid(S['Q'], S['rows'], S['cols']))


def test_register_recovers_the_pelvis_with_mutual_information():
    """The tilted scene from reg_ref.THETA_START (every centre at least 10 px off), bins and bar from mi.json: the model alone
    ends at 0.079 px with 16 bins, the bar is 0.25 px.  GPU: see the printed line."""
    S, vol, fixed = _scene()
    bins, bar = MF.registration()
    geom = _geom(S, S['poses'])
    ctr = R.volume_centre(S)
    assert R.centre_distances(S, S['poses'][0], reg.pose_delta(R.THETA_START, ctr) @ S['poses'][0]).min() >= 10
    kw = dict(moving=(0, 1, 2), theta0=R.THETA_START, popsize=MF.POPSIZE, sigma0=MF.SIGMA0, step_mm=MF.STEP_MM, seed=MF.SEED, similarity='mi',
              mi_bins=bins)
    res = reg.register(vol, geom, fixed, generations=MF.GENERATIONS, **kw)
    dist = R.centre_distances(S, S['poses'][0], res.pose)
    print('MI, %d bins, pelvis from the offset: centres %s px (bar %.3f), cost %.6f -> %.6f, %d renders, theta %s'
          % (bins, ' '.join('%.4f' % d for d in dist), bar, res.cost[0], res.final_cost, res.renders, np.round(res.theta, 3).tolist()))
    assert res.renders == 1 + 16 * 80 + 1 and res.cost.shape == (80,) and res.levels == [(None, 80, 45, 61)]
    assert dist.max() <= bar, dist
    assert res.final_cost < res.cost[0] < 0
    # the run repeats bit for bit; a fixed image under another intensity mapping is registered as well as the first
    a = reg.register(vol, geom, fixed, generations=6, **kw)
    b = reg.register(vol, geom, fixed, generations=6, **kw)
    assert a.theta.tobytes() == b.theta.tobytes() and a.cost.tobytes() == b.cost.tobytes() and a.final_cost == b.final_cost
    # refine: the adjoint exists, and the finish never costs more than the CMA-ES mean
    fine = reg.register(vol, geom, fixed, generations=6, refine=10, **kw)
    assert fine.theta_cma.tobytes() == a.theta.tobytes() and len(fine.refine_cost) >= 1 and fine.refine_cost[0] == a.final_cost
    assert fine.final_cost <= a.final_cost and fine.gradient_evaluations >= 1
    print('MI refine: cost at the CMA-ES mean %.9f, after %d accepted steps %.9f (%d gradient evaluations)'
          % (a.final_cost, len(fine.refine_cost) - 1, fine.final_cost, fine.gradient_evaluations))
    # a given range takes no render; a start with nothing in view is refused
    given = reg.register(vol, geom, fixed, generations=2, mi_range=(0.0, 2.0), **kw)
    assert given.renders == 16 * 2 + 1
    with pytest.raises(nat.DflError, match='nothing is in view'):
        reg.register(vol, geom, fixed, generations=2, **dict(kw, theta0=(0, 0, 0, 4000.0, 0, 0)))


@pytest.mark.parametrize('kw', [dict(generations=5), dict(generations=3, refine=3), dict(generations=3, max_views=16, mi_bins=(8, 24))])
def test_register_many_has_the_bytes_of_register(kw):
    from test_gpu_register_many import _problems, _same_bytes
    vol, geoms, fixed, theta0, _ = _problems()
    kw = dict(dict(mi_bins=16), **kw, popsize=8, step_mm=1.0, similarity='mi')
    got = reg.register_many(vol, geoms, fixed, theta0=theta0, **kw)
    kw.pop('max_views', None)
    assert len(got) == 3 and len({r.theta.tobytes() for r in got}) == 3
    for i in range(3):
        one = reg.register(vol, geoms[i], fixed[i], theta0=theta0[i], **kw)
        _same_bytes(got[i], one, i)
        assert one.renders == 1 + 8 * kw['generations'] + one.gradient_evaluations + 1
        if kw.get('refine'):
            assert one.final_cost <= one.refine_cost[0] and one.gradient_evaluations >= 1


def test_example_end_to_end(tmp_path, capsys):
    import register_2d3d as cli
    from test_gpu_register import CROP, SPEC, _write_container
    S = D.scene('tilted')
    path = os.path.join(str(tmp_path), 'full.h5')
    _write_container(path, 1)
    prefix = os.path.join(str(tmp_path), 'run')
    bins, bar = MF.registration()
    assert cli.main([path, SPEC, '0', '--out', prefix, '--crop', str(CROP), '--ds-factor', '1', '--offset', '2,-1.5,2.5,4,-3,15',
                     '--seed', '0', '--mi-bins', str(bins), '--refine', '5']) == 0
    out = capsys.readouterr().out
    with capsys.disabled():
        print(out)
    z = np.load(prefix + '_reg.npz')
    assert z['cost'].shape == (80,) and z['cost'][-1] < z['cost'][0] < 0                 # -MI, not 1 - NCC
    vals = {ln.split(' = ')[0]: float(ln.split(' = ')[1].split()[0]) for ln in out.strip().split('\n') if ' = ' in ln}
    assert vals['start largest reprojection distance'] >= 10
    assert vals['final largest reprojection distance'] <= bar
    assert 'refinement cost' in out and os.path.getsize(prefix + '_reg.png') > 0
    H, W = pp.out_size(S['rows'], S['cols'], CROP, 1)
    assert (H, W) == (41, 57)
