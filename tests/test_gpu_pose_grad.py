"""The gradient path of dfl_amd.register on the GPU: dfl_sim_gradncc_bwd and dfl_drr_pose_grad against tests/grad_ref.py
(the numpy float64 restatement of DESIGN.md section 19), the chain to the six pose parameters, and the quasi-Newton
finish of register().

Bars: 8 x the floors of tests/golden/floors/pose_grad.json -- the largest |float32 model - float64 model| of the same
numbers (tests/grad_floor.py; both sides the model, never the kernel), as fractions of the largest entry.  The
refinements must pass the bars of tests/test_gpu_register.py (0.25 px, twice the model's cost at the truth); the
models alone, with the product's own bfgs, end at 0.088 px (refinement only) -- pose_grad.json.
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
import grad_floor as GF  # noqa: E402
import grad_ref as G  # noqa: E402
import reg_floor as FL  # noqa: E402
import reg_ref as R  # noqa: E402
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, drr, h5lite, png, preprocess as pp, register as reg  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
_CACHE = {}


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                 # a copy: the shared scene arrays are read-only


# ---- 1. the adjoint of the similarity ----------------------------------------------------------------------------------
@pytest.mark.parametrize('mask_name', ['none', 'ragged', 'empty'])
@pytest.mark.parametrize('size', R.SIM_SIZES)
def test_adjoint_matches_the_model(size, mask_name):
    H, W = size
    fixed, moving = R.sim_images(H, W)
    mask = R.sim_masks(H, W)[mask_name]
    _, want = G.sim_adjoint(moving, fixed, mask)
    bars, sum_bars = GF.adjoint_bars(H, W, mask_name)
    sim = reg.Similarity(_dev(fixed), None if mask is None else _dev(mask), views=6)
    mv = _dev(moving)
    cost, d = sim.cost_and_adjoint(mv)
    assert cost.dtype == torch.float64 and tuple(cost.shape) == (6,) and d.dtype == torch.float32 and tuple(d.shape) == (6, H, W)
    assert torch.equal(cost, sim.cost(mv))                        # the forward's bits
    got = d.cpu().numpy()
    n = int(R.counted(H, W, mask).sum())
    for v in range(6):
        scale = float(np.abs(want[v]).max())
        err, tot = float(np.abs(got[v] - want[v]).max()), abs(float(got[v].astype(np.float64).sum()))
        print('adjoint %d x %d mask %s view %d: largest |adjoint| %.3e, |error| %.3e (bar %.3e), |sum| %.3e (bar %.3e)'
              % (H, W, mask_name, v, scale, err, bars[v] * scale, tot, sum_bars[v] * scale))
        # exactly 0: the constant image, no or one counted pixel (a variance is 0).  The fixed image and its negation
        # (ncc = +-1 is an extremum: the two terms cancel) give 0 or rounding dust in the model; where the model, and with
        # it the floor, is exactly 0 the kernel has to give exactly 0 too
        assert scale == 0.0 if v == 2 or n < 2 else scale < 1e-15 if v < 2 else scale > 1e-10
        if scale == 0.0:
            assert not got[v].any()
        else:
            assert err <= bars[v] * scale and tot <= sum_bars[v] * scale
    # equal bits: a second run, view 4 alone, a permuted batch
    assert torch.equal(sim.cost_and_adjoint(mv)[1], d)
    assert torch.equal(sim.cost_and_adjoint(mv[4:5].clone())[1], d[4:5])
    c2, d2 = sim.cost_and_adjoint(mv[[5, 0, 4]].contiguous())
    assert torch.equal(d2, d[[5, 0, 4]]) and torch.equal(c2, cost[[5, 0, 4]])


# ---- 2. forces and moments ---------------------------------------------------------------------------------------------
def _volume(kind):
    if kind not in _CACHE:
        S = D.scene(kind)
        _CACHE[kind] = (S, drr.Volume(_dev(S['mu']), _dev(S['lab'])), drr.Grid(S['Q'], S['rows'], S['cols']))
    return _CACHE[kind]


def _inputs(kind, view, step, pattern):
    key = (kind, view, step, pattern)
    if key not in _CACHE:
        _CACHE[key] = GF.moment_inputs(*key)
    return _CACHE[key]


@pytest.mark.parametrize('step', [0.5, 1.0])
@pytest.mark.parametrize('view', [0, 1])
@pytest.mark.parametrize('kind', ['tilted', 'aligned'])
def test_moments_match_the_model(kind, view, step):
    S, vol, grid = _volume(kind)
    doc = GF.load()['moments']
    mine = drr.pack(vol, np.array(D.scene_views(S))[view][None], list(D.MASKS), grid, 'trilinear', True)
    for pattern in ('adjoint', 'sines'):
        recs, d_att, zeroed, piv = _inputs(kind, view, step, pattern)
        assert mine[0].tobytes() == recs.tobytes()                # the kernel's own float32 records
        assert zeroed <= 0.01                                     # rays on which N may legitimately differ by one
        want = np.array(doc[GF.moment_key(kind, view, step, pattern)]['moments'])
        bar = GF.moment_bar(kind, view, step, pattern)
        got_t = drr.pose_gradient(vol, mine, grid, _dev(d_att)[None], piv[None], step)
        assert got_t.dtype == torch.float64 and tuple(got_t.shape) == (1, 3, 12) and got_t.is_cuda
        got = got_t.cpu().numpy()[0]
        print('moments %s view %d step %.1f %s: largest entry %.4e, |error| %.3e (bar %.3e), %.3f %% of the rays zeroed'
              % (kind, view, step, pattern, np.abs(want).max(), np.abs(got - want).max(), bar, 100 * zeroed))
        assert np.abs(got - want).max() <= bar
        assert torch.equal(drr.pose_gradient(vol, mine, grid, _dev(d_att)[None], None, step), got_t)       # the default pivots; equal bits
    # known answers, with the sines
    d_t = _dev(d_att)[None]
    assert not drr.pose_gradient(vol, mine, grid, torch.zeros_like(d_t), piv[None], step).cpu().numpy().any()
    hollow = mine.copy()
    hollow['box_hi'][0, 1] = hollow['box_lo'][0, 1] - 1
    h = drr.pose_gradient(vol, hollow, grid, d_t, piv[None], step)
    assert not h[0, 1].cpu().numpy().any() and torch.equal(h[0, [0, 2]], got_t[0, [0, 2]])
    # moving the pivot by p changes Mom by -F (x) p.  Both sides are within the bar of their float64 values, for which
    # this is an identity, and F's own error enters times |p|: (2 + |p|_1) bars
    p = np.array([1.0, -0.5, 0.75], np.float32)
    moved = drr.pose_gradient(vol, mine, grid, d_t, (piv + p)[None], step).cpu().numpy()[0]
    assert np.array_equal(moved[:, :3], got[:, :3])
    assert np.abs(moved[:, 3:].reshape(3, 3, 3) - (got[:, 3:].reshape(3, 3, 3) - got[:, :3, None] * p[None, None, :])).max() <= (2 + np.abs(p).sum()) * bar
    # a view alone equals the same view in a batch, bit for bit
    other = _inputs(kind, 1 - view, step, 'sines')
    order = [view, 1 - view]
    both = drr.pose_gradient(vol, np.stack([recs, other[0]]), grid, _dev(np.stack([d_att, other[1]])), np.stack([piv, other[3]]), step)
    assert torch.equal(both[0:1], got_t), order


# ---- 3. the gradient with respect to the pose parameters ---------------------------------------------------------------
def _scene():
    """(S, volume, fixed on the device, the model's cost at the true pose): shared, never written to."""
    if 'scene' not in _CACHE:
        S, vol, _ = _volume('tilted')
        _CACHE['scene'] = (S, vol, _dev(FL.fixed_image(S).astype(np.float32)), FL.truth_cost(S))
    return _CACHE['scene']


def _geom(S, poses):
    named = dict(zip(drr.POSES, poses))
    return drr.Geometry(S['K'], S['E'], named, S['I2P'], np.eye(3), drr.default_objects(S['E'], named, S['I2P']),
                        drr.Grid(S['Q'], S['rows'], S['cols']))


def test_theta_gradient_matches_the_model():
    S, vol, fixed, _ = _scene()
    doc = GF.load()['theta']
    th = np.array(doc['theta'])
    assert np.array_equal(th, GF.THETA_FRACTION * np.array(R.THETA_START))
    geom, ctr, I2P = _geom(S, S['poses']), R.volume_centre(S), S['I2P']
    back = np.linalg.inv(I2P)
    Dm = reg.pose_delta(th, ctr)
    c2is = np.stack([back @ Dm @ I2P @ ob.c2i for ob in geom.objects])[None]
    xis = (back[None] @ reg.pose_delta_jacobians(th, ctr)[0] @ (np.linalg.inv(Dm) @ I2P)[None])[None]
    assert np.abs(xis[0] - G.xi(th, ctr, I2P, reg.pose_deltas)).max() <= 1e-8
    level = reg._Level(vol, geom.grid, fixed, None, 1, FL.STEP_MM)
    cost, grad = level.costs_and_grads(c2is, [ob.mask for ob in geom.objects], xis, [0, 1, 2])
    want = np.array(doc['gradient'])
    bar = GF.BAR_FACTOR * doc['floor'] * np.abs(want).max()
    print('theta gradient at %.1f x the start: kernel %s, model %s, |error| %.3e (bar %.3e); cost %.6f (model %.6f)'
          % (GF.THETA_FRACTION, np.round(grad[0], 6).tolist(), np.round(want, 6).tolist(), np.abs(grad[0] - want).max(), bar, cost[0], doc['cost']))
    assert cost.shape == (1,) and grad.shape == (1, 6) and grad.dtype == np.float64
    assert np.abs(grad[0] - want).max() <= bar
    assert cost[0] == level.costs(c2is, [ob.mask for ob in geom.objects])[0]
    # an object that does not move contributes nothing: the three single-object gradients add up to the whole
    parts = sum(level.costs_and_grads(c2is, [ob.mask for ob in geom.objects], xis, [n])[1] for n in range(3))
    assert np.abs(parts - grad).max() <= 1e-12 * np.abs(grad).max()


# ---- 4., 5. the quasi-Newton finish ------------------------------------------------------------------------------------
def _model_cost(S, poses):
    return float(R.cost(R.render_poses(S, poses, 'trilinear', 0.5), FL.fixed_image(S)))


def _check_pelvis(S, res, final_poses, truth, what):
    dist = R.centre_distances(S, S['poses'][0], res.pose)
    cost = _model_cost(S, final_poses)
    print('%s: centres %s px (bar %.2f), model cost of the found pose %.6f (at the truth %.6f, bar %.6f), kernel cost %.6f -> %.6f, '
          '%d renders, %d gradient evaluations, theta %s'
          % (what, ' '.join('%.4f' % d for d in dist), FL.PIXEL_BAR, cost, truth, FL.COST_FACTOR * truth, res.refine_cost[0], res.final_cost,
             res.renders, res.gradient_evaluations, np.round(res.theta, 3).tolist()))
    assert dist.max() <= FL.PIXEL_BAR, dist
    assert cost <= FL.COST_FACTOR * truth, cost


def test_refinement_alone():
    """generations=0, refine=30 from the offset tests/grad_floor.py settled on (0.15 x THETA_START, 1.98 px off: from
    0.3 x the models alone end at 0.17 px, above half the bar).  The models alone end at 0.088 px and a cost of 0.002426.
    GPU: centres 0.036 0.045 0.042 0.081 0.021 0.113 px, model cost of the found pose 0.002417, kernel cost 0.159064 ->
    0.002487 in 34 gradient evaluations."""
    S, vol, fixed, truth = _scene()
    doc = GF.load()['refinement']['refine_only']
    assert max(doc['final_px']) <= FL.PIXEL_BAR / 2 and doc['final_cost_step_0_5'] <= FL.COST_FACTOR * truth
    theta0 = np.array(doc['theta0'])
    assert np.allclose(theta0, GF.REFINE_START * np.array(R.THETA_START) / 2 ** doc['halvings'], rtol=1e-15)
    geom = _geom(S, S['poses'])
    res = reg.register(vol, geom, fixed, theta0=theta0, generations=0, refine=GF.REFINE, refine_tol=GF.REFINE_TOL, step_mm=FL.STEP_MM)
    start = R.centre_distances(S, S['poses'][0], reg.pose_delta(theta0, R.volume_centre(S)) @ S['poses'][0])
    print('refinement alone starts %s px off' % ' '.join('%.4f' % d for d in start))
    _check_pelvis(S, res, res.poses, truth, 'refinement alone')
    assert res.cost.shape == (0,) and np.array_equal(res.theta_cma, theta0)
    assert len(res.refine_cost) >= 2 and (np.diff(res.refine_cost) <= 0).all() and res.final_cost == res.refine_cost[-1]
    assert res.gradient_evaluations <= 2 * GF.REFINE + 1 and res.renders == res.gradient_evaluations + 1
    again = reg.register(vol, geom, fixed, theta0=theta0, generations=0, refine=GF.REFINE, refine_tol=GF.REFINE_TOL, step_mm=FL.STEP_MM)
    assert again.theta.tobytes() == res.theta.tobytes() and again.refine_cost.tobytes() == res.refine_cost.tobytes()


def test_refinement_after_cma_es():
    """GPU: centres 0.60 0.81 0.61 1.26 1.55 0.47 px -> 0.10 0.20 0.09 0.08 0.45 0.44 px, kernel cost 0.074756 -> 0.026869 in 34
    gradient evaluations (the models alone: 1.55 -> 0.45 px, 0.0748 -> 0.0271: pose_grad.json)."""
    S, vol, fixed, truth = _scene()
    geom = _geom(S, S['poses'])
    kw = dict(theta0=R.THETA_START, popsize=16, generations=GF.CMA_GENERATIONS, sigma0=2.0, step_mm=FL.STEP_MM, seed=0)
    today = reg.register(vol, geom, fixed, **kw)
    plain = reg.register(vol, geom, fixed, refine=0, **kw)
    assert plain.theta.tobytes() == today.theta.tobytes() and plain.cost.tobytes() == today.cost.tobytes()
    assert plain.final_cost == today.final_cost and plain.renders == today.renders == 16 * GF.CMA_GENERATIONS + 1
    assert plain.gradient_evaluations == 0 and plain.refine_cost.shape == (0,) and plain.theta_cma.tobytes() == plain.theta.tobytes()
    res = reg.register(vol, geom, fixed, refine=GF.REFINE, **kw)
    assert res.theta_cma.tobytes() == today.theta.tobytes() and res.cost.tobytes() == today.cost.tobytes()
    assert res.refine_cost[0] == today.final_cost and res.final_cost <= today.final_cost
    assert (np.diff(res.refine_cost) <= 0).all() and res.renders == today.renders + res.gradient_evaluations
    ctr = R.volume_centre(S)
    before = R.centre_distances(S, S['poses'][0], reg.pose_delta(res.theta_cma, ctr) @ S['poses'][0])
    after = R.centre_distances(S, S['poses'][0], res.pose)
    print('%d generations, then refinement: centres %s px -> %s px, kernel cost %.6f -> %.6f in %d gradient evaluations'
          % (GF.CMA_GENERATIONS, ' '.join('%.4f' % d for d in before), ' '.join('%.4f' % d for d in after), today.final_cost, res.final_cost,
             res.gradient_evaluations))


# ---- 6. refusals launch nothing ----------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    L = nat.lib()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    # the adjoint
    H, W = 45, 61
    fixed, moving = R.sim_images(H, W)
    sim = reg.Similarity(_dev(fixed), None, views=6)
    mv = _dev(moving)
    need = L.dfl_sim_gradncc_bwd_scratch_doubles(6, H, W)
    assert need == 6 * 6 * 6 + 4 * 6
    out = torch.full((6,), -7.0, dtype=torch.float64, device=DEV)
    scratch = torch.full((need,), -7.0, dtype=torch.float64, device=DEV)
    d_moving = torch.full((6, H, W), -7.0, device=DEV)

    def bwd(**k):
        return nat.SimGradnccBwdArgs(**dict(dict(moving=mv.data_ptr(), fx=sim.fx.data_ptr(), fy=sim.fy.data_ptr(), counted=sim.counted.data_ptr(),
                                                 totals=sim.totals.data_ptr(), scratch=scratch.data_ptr(), cost=out.data_ptr(),
                                                 d_moving=d_moving.data_ptr(), scratch_doubles=need, V=6, H=H, W=W), **k))

    for kw, word in ((dict(moving=None), b'required'), (dict(fx=None), b'required'), (dict(fy=None), b'required'),
                     (dict(counted=None), b'required'), (dict(totals=None), b'required'), (dict(scratch=None), b'required'),
                     (dict(cost=None), b'required'), (dict(d_moving=None), b'required'), (dict(H=2), b'3 x 3'), (dict(W=2), b'3 x 3'),
                     (dict(V=0), b'65535'), (dict(V=65536), b'65535'), (dict(scratch_doubles=need - 1), b'scratch')):
        a = bwd(**kw)
        assert L.dfl_sim_gradncc_bwd(C.addressof(a), stream) == -1 and word in L.dfl_last_error(), (kw, L.dfl_last_error())
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (scratch == -7.0).all() and (d_moving == -7.0).all()
    a = bwd()                                                     # the same block, unchanged, runs
    assert L.dfl_sim_gradncc_bwd(C.addressof(a), stream) == 0
    want_c, want_d = sim.cost_and_adjoint(mv)
    assert torch.equal(out, want_c) and torch.equal(d_moving, want_d)
    # the pose gradient
    S, vol, grid = _volume('tilted')
    recs, d_att, _, piv = _inputs('tilted', 0, 1.0, 'sines')
    d_objs = torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(-1)).to(DEV)
    d_t, p_t = _dev(d_att), _dev(piv)
    need = L.dfl_drr_pose_grad_scratch_doubles(1, 3, grid.H, grid.W)
    assert need == 3 * 3 * 4 * 12
    grad = torch.full((1, 3, 12), -7.0, dtype=torch.float64, device=DEV)
    scratch = torch.full((need,), -7.0, dtype=torch.float64, device=DEV)
    nz, ny, nx = vol.shape

    def pg(**k):
        return nat.DrrPoseGradArgs(**dict(dict(mu=vol.mu.data_ptr(), labels=vol.labels.data_ptr(), objects=d_objs.data_ptr(), d_att=d_t.data_ptr(),
                                               pivots=p_t.data_ptr(), grad=grad.data_ptr(), scratch=scratch.data_ptr(), scratch_doubles=need,
                                               qscale=(nat.f32 * 9)(*grid.Q.astype(np.float32).reshape(-1)), nx=nx, ny=ny, nz=nz, H=grid.H,
                                               W=grid.W, views=1, n_obj=3, interp=nat.DRR_TRILINEAR, step_mm=1.0), **k))

    for kw, word in ((dict(mu=None), b'required'), (dict(labels=None), b'required'), (dict(objects=None), b'required'),
                     (dict(d_att=None), b'required'), (dict(pivots=None), b'required'), (dict(grad=None), b'required'),
                     (dict(scratch=None), b'required'), (dict(nx=0), b'bad sizes'), (dict(H=0), b'bad sizes'), (dict(views=0), b'bad sizes'),
                     (dict(n_obj=0), b'bad sizes'), (dict(views=65536, scratch_doubles=1 << 40), b'65535'), (dict(interp=nat.DRR_EXACT), b'trilinear'),
                     (dict(step_mm=0.0), b'step_mm'), (dict(scratch_doubles=need - 1), b'scratch')):
        a = pg(**kw)
        assert L.dfl_drr_pose_grad(C.addressof(a), stream) == -1 and word in L.dfl_last_error(), (kw, L.dfl_last_error())
    torch.cuda.synchronize()
    assert (grad == -7.0).all() and (scratch == -7.0).all()
    a = pg()
    assert L.dfl_drr_pose_grad(C.addressof(a), stream) == 0
    assert torch.equal(grad, drr.pose_gradient(vol, recs[None], grid, d_t[None], piv[None], 1.0))
    # Python
    with pytest.raises(nat.DflError, match='GPU'):
        drr.pose_gradient(vol, recs[None], grid, torch.zeros((1, grid.H, grid.W)), None, 1.0)
    with pytest.raises(nat.DflError, match='d_att'):
        drr.pose_gradient(vol, recs[None], grid, d_t[None, :40], None, 1.0)
    with pytest.raises(nat.DflError, match='pivots'):
        drr.pose_gradient(vol, recs[None], grid, d_t[None], piv, 1.0)
    with pytest.raises(nat.DflError, match='GPU'):
        sim.cost_and_adjoint(torch.zeros((1, H, W)))
    with pytest.raises(nat.DflError, match='adjoint'):
        reg.PatchSimilarity(_dev(fixed), None, views=1).cost_and_adjoint(mv[:1])
    geom = _geom(S, S['poses'])
    with pytest.raises(nat.DflError, match='patch'):
        reg.register(vol, geom, _scene()[2], generations=1, refine=2, similarity='patch')
    with pytest.raises(nat.DflError, match='refine'):
        reg.register(vol, geom, _scene()[2], generations=1, refine=-1)


# ---- 7. the example, end to end ----------------------------------------------------------------------------------------
SPEC, CROP = '17-1882', 2


def _write_container(path, rot180):
    """The tilted scene as a full-resolution file (the construction of tests/test_gpu_register.py): vol, vol-seg,
    vol-landmarks, proj-params and one projection whose image is the model's own exact rendering on the full detector
    grid, with the three poses in reverse order."""
    S = D.scene('tilted')
    poses = S['poses'][::-1]
    recs = D.pack([D.c2i(S['I2P'], P, S['E']) for P in poses], D.MASKS, S['Q'], S['lab'])
    att, plen, _ = D.render(S['mu'], S['lab'], recs, S['Q'].astype(np.float32), S['rows'], S['cols'])
    names = pp.LAND_ORDER[:6]
    pts = R.centres_phys(S).astype(np.float32)
    cam = (S['E'] @ np.linalg.inv(poses[0])) @ np.concatenate([pts.astype(np.float64), np.ones((6, 1))], 1).T
    uv = S['K'] @ cam[:3]
    uv = (uv / uv[2])[:2]
    with h5lite.File(path, 'w') as f:
        f['proj-params/intrinsic'] = S['K']
        f['proj-params/extrinsic'] = S['E']
        f['proj-params/num-rows'] = np.int64(S['rows'])
        f['proj-params/num-cols'] = np.int64(S['cols'])
        for grp, px in ((SPEC + '/vol/', S['hu']), (SPEC + '/vol-seg/image/', S['lab'])):
            f[grp + 'pixels'] = px
            f[grp + 'dir-mat'] = np.eye(3)
            f[grp + 'spacing'] = np.array([0.8, 0.75, 1.1])
            f[grp + 'origin'] = S['I2P'][:3, 3]
        for l, name in enumerate(names):
            f[SPEC + '/vol-landmarks/' + name] = pts[l]
        pfx = SPEC + '/projections/000/'
        f[pfx + 'image/pixels'] = (1000.0 * np.exp(-att)).astype(np.float32)
        f[pfx + 'gt-seg/pixels'] = D.label_map(plen)
        for l, name in enumerate(names):
            f[pfx + 'gt-landmarks/' + name] = uv[:, l].astype(np.float32)
        for k, P in zip(drr.POSES, poses):
            f[pfx + 'gt-poses/' + k] = P
        f[pfx + 'rot-180-for-up'] = np.int64(rot180)
    return poses


def test_example_end_to_end_with_refine(tmp_path, capsys):
    import register_2d3d as cli
    path = os.path.join(str(tmp_path), 'full.h5')
    _write_container(path, 1)
    prefix = os.path.join(str(tmp_path), 'run')
    args = [path, SPEC, '0', '--out', prefix, '--crop', str(CROP), '--ds-factor', '1', '--offset', '2,-1.5,2.5,4,-3,15', '--seed', '0',
            '--generations', '20']
    assert cli.main(args + ['--refine', '10']) == 0
    out = capsys.readouterr().out
    with capsys.disabled():
        print(out)
    line = [ln for ln in out.split('\n') if ln.startswith('pelvis: refinement cost')]
    assert len(line) == 1
    words = line[0].split()
    before, after, evals = float(words[3]), float(words[5]), int(words[7])
    assert after <= before and 1 <= evals
    z = np.load(prefix + '_reg.npz')
    assert z['cost'].shape == (20,) and z['theta'].shape == (6,) and png.read(prefix + '_reg.png').ndim == 3
    vals = {ln.split(' = ')[0]: float(ln.split(' = ')[1].split()[0]) for ln in out.strip().split('\n') if ' = ' in ln}
    assert vals['final largest reprojection distance'] < vals['start largest reprojection distance']
    # without --refine nothing of it is printed, and the patch similarity refuses it on the command line
    assert cli.main(args[:-2] + ['--generations', '2']) == 0
    assert 'refinement' not in capsys.readouterr().out
    assert cli.main(args + ['--refine', '10', '--similarity', 'patch']) == 1
