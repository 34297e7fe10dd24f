"""The gradient path of dfl_amd.register without a GPU: the numpy models of tests/grad_ref.py against central differences
of the models of the cost (tests/reg_ref.py), the Jacobians of pose_delta, the quasi-Newton iteration, the committed
floors against a fresh run of the models, and the refusals at the C ABI and in Python."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
import drr_ref as D  # noqa: E402
import grad_floor as GF  # noqa: E402
import grad_ref as G  # noqa: E402
import reg_floor as FL  # noqa: E402
import reg_ref as R  # noqa: E402
from dfl_amd import _native as nat, drr, register as reg  # noqa: E402


# ---- the models --------------------------------------------------------------------------------------------------------
def test_model_gradient_against_central_differences_of_the_model_cost():
    """The frozen-sampling gradient against differences of the real cost (whose N, t0 and t1 move with the pose) at
    0.2 x THETA_START, h = 0.1, step 1 mm.  Measured: relative difference 0.0221, cosine 0.99990."""
    S = D.scene('tilted')
    fixed = FL.fixed_image(S)
    th = GF.THETA_FRACTION * np.array(R.THETA_START)
    cost, g = G.model_cost_and_grad(S, S['poses'], (0, 1, 2), fixed, reg.pose_deltas, 1.0)(th)
    fn = R.model_cost_fn(S, S['poses'], (0, 1, 2), fixed, reg.pose_deltas, 1.0)
    h = 0.1
    f = fn(np.concatenate([th[None] + h * np.eye(6), th[None] - h * np.eye(6)]))
    cd = (f[:6] - f[6:]) / (2 * h)
    rel = float(np.linalg.norm(g - cd) / np.linalg.norm(cd))
    cos = float(g @ cd / (np.linalg.norm(g) * np.linalg.norm(cd)))
    print('model gradient against central differences: relative difference %.4f, cosine %.5f' % (rel, cos))
    assert cost == fn(th[None])[0]
    assert rel <= 0.05 and cos >= 0.999
    # the committed gradient is this one
    doc = GF.load()['theta']
    np.testing.assert_allclose(g, doc['gradient'], rtol=1e-9, atol=1e-14)
    assert abs(cost - doc['cost']) <= 1e-12


def test_model_adjoint_against_central_differences_on_single_pixels():
    """rtol 1e-6 of the largest |adjoint|: the border pixels' own entries are a thousand times smaller than the largest
    and a difference of two costs resolves them no better.  Measured: 1e-9 in the interior."""
    fixed, moving = (a.astype(np.float64) for a in R.sim_images(45, 61))
    mask = R.sim_masks(45, 61)['ragged']
    for m in (None, mask):
        cost, d = G.sim_adjoint(moving[4], fixed, m)
        assert cost == R.cost(moving[4], fixed, m)
        big = float(np.abs(d).max())
        h = 1e-4
        for r, c in ((0, 0), (10, 20), (44, 60), (22, 1), (23, 30), (5, 59), (1, 1)):
            e = np.zeros((45, 61))
            e[r, c] = h
            num = (R.cost(moving[4] + e, fixed, m) - R.cost(moving[4] - e, fixed, m)) / (2 * h)
            assert abs(d[r, c] - num) <= 1e-6 * big, (r, c, d[r, c], num)
    # the Sobel kernels sum to 0, so does the adjoint; an image that cannot correlate has none
    assert abs(d.sum()) <= 1e-12 * big * d.size
    assert not G.sim_adjoint(np.full((45, 61), 0.7), fixed)[1].any()
    assert not G.sim_adjoint(moving[4], fixed, R.sim_masks(45, 61)['empty'])[1].any()
    assert not G.sim_adjoint(moving[4][:3, :3], fixed[:3, :3])[1].any()
    c, d6 = G.sim_adjoint(moving, fixed)
    assert c.shape == (6,) and d6.shape == (6, 45, 61) and np.array_equal(d6[4], G.sim_adjoint(moving[4], fixed)[1])


def test_model_moments_known_answers():
    S = D.scene('tilted')
    recs, d_att, zeroed, piv = GF.moment_inputs('tilted', 1, 1.0, 'sines')
    q = S['Q'].astype(np.float32)
    args = (S['mu'], S['lab'], recs, q, S['rows'], S['cols'])
    m = G.pose_moments(*args, d_att, piv, 1.0)
    assert zeroed <= 0.01 and m.shape == (3, 12) and np.abs(m).min() > 0
    assert not G.pose_moments(*args, np.zeros_like(d_att), piv, 1.0).any()
    p = np.array([3.0, -2.0, 5.0], np.float32)
    moved = G.pose_moments(*args, d_att, piv + p, 1.0)
    want = m[:, 3:].reshape(3, 3, 3) - m[:, :3, None] * p[None, None, :]
    assert np.array_equal(moved[:, :3], m[:, :3]) and np.abs(moved[:, 3:].reshape(3, 3, 3) - want).max() <= 1e-12 * np.abs(m).max()
    hollow = recs.copy()
    hollow['box_hi'][1] = hollow['box_lo'][1] - 1
    mh = G.pose_moments(S['mu'], S['lab'], hollow, q, S['rows'], S['cols'], d_att, piv, 1.0)
    assert not mh[1].any() and np.array_equal(mh[[0, 2]], m[[0, 2]])
    # the chain: a pure shift along axis a (Xi = e_a e_4^T) picks F[a] of the moving objects alone
    Xi = np.zeros((6, 4, 4))
    for a in range(3):
        Xi[a, a, 3] = 1.0
    assert np.array_equal(G.chain(m, piv, Xi, (0, 2))[:3], m[0, :3] + m[2, :3])
    assert np.array_equal(drr.box_pivots(recs[None])[0], piv) and piv.dtype == np.float32


# ---- the Jacobians of pose_delta ---------------------------------------------------------------------------------------
def test_pose_delta_jacobians():
    ctr = np.array([3.0, -5.0, 100.0])
    thetas = np.array([[0.0] * 6, list(R.THETA_START), [0.3, -1.2, 2.0, 1.0, 2.0, 3.0], [1e-4, 0.0, -2e-4, 0.0, 1.0, 0.0]])
    J = reg.pose_delta_jacobians(thetas, ctr)
    assert J.shape == (4, 6, 4, 4) and J.dtype == np.float64
    for k in range(4):
        for i in range(3):                                        # a translation parameter: exactly its own unit column
            want = np.zeros((4, 4))
            want[i, 3] = 1.0
            assert np.array_equal(J[k, 3 + i], want)
        assert not J[k, :, 3].any()
    for i in range(3):                                            # at theta = 0: rot_unit hat(e_i), about the centre
        E = reg._hat(np.eye(3)[i])
        assert np.array_equal(J[0, i, :3, :3], reg.ROT_UNIT * E) and np.allclose(J[0, i, :3, 3], -reg.ROT_UNIT * E @ ctr, rtol=0, atol=1e-15)
    h = 1e-5
    for k in range(4):
        num = np.stack([(reg.pose_delta(thetas[k] + h * e, ctr) - reg.pose_delta(thetas[k] - h * e, ctr)) / (2 * h) for e in np.eye(6)])
        assert np.abs(J[k] - num).max() <= 1e-8, k
    assert np.abs(reg.pose_delta_jacobians(thetas[1], ctr, rot_unit=0.01)[0, :3] * 2 - reg.pose_delta_jacobians(
        thetas[1] * [0.5, 0.5, 0.5, 1, 1, 1], ctr, rot_unit=0.02)[0, :3]).max() <= 1e-12


# ---- the quasi-Newton iteration ----------------------------------------------------------------------------------------
def test_bfgs_on_an_ill_conditioned_quadratic():
    scale = 10.0 ** (np.arange(6) * 6 / 5)                       # condition 1e6: the quadratic of the CMA-ES test
    target = np.array([1.0, -2.0, 0.5, 3.0, -1.0, 0.25])
    calls = []

    def fun(x):
        calls.append(x.copy())
        return float((((x - target) ** 2) * scale).sum()), 2 * scale * (x - target)

    a = reg.bfgs(fun, np.full(6, 3.0), 100, 1e-12)
    # it ends when a trial step is shorter than min_step = 1e-6, and a quasi-Newton step is the distance to the minimum
    assert np.abs(a.x - target).max() <= 1e-6 and a.f <= 1e-12 * a.trace[0]
    assert a.evaluations == len(calls) and len(a.trace) == a.iterations + 1 and (np.diff(a.trace) <= 0).all()
    assert a.evaluations <= 4 * a.iterations + 1
    g0 = 2 * scale * (3.0 - target)
    assert np.allclose(calls[1], calls[0] - g0 / np.linalg.norm(g0))          # the first trial step is min(1, 1 / |g|) long
    b = reg.bfgs(fun, np.full(6, 3.0), 100, 1e-12)
    assert a.x.tobytes() == b.x.tobytes() and a.trace.tobytes() == b.trace.tobytes()
    # the iteration limit, and a step shorter than tol ends it
    assert reg.bfgs(fun, np.full(6, 3.0), 3, 1e-12).iterations == 3
    assert reg.bfgs(fun, np.full(6, 3.0), 100, 1e-2).iterations < a.iterations
    assert reg.bfgs(fun, target, 5, 1e-12).iterations == 0        # a zero gradient
    # a cost that is not finite, or larger, is a rejected step
    def walled(x):
        f, g = fun(x)
        return (np.nan, g) if x[0] < 0.9 else (f, g)

    w = reg.bfgs(walled, np.full(6, 3.0), 100, 1e-12)
    assert np.isfinite(w.trace).all() and (np.diff(w.trace) <= 0).all() and w.x[0] >= 0.9
    with pytest.raises(nat.DflError, match='finite'):
        reg.bfgs(lambda x: (np.inf, x), np.ones(6))


# ---- the committed floors ----------------------------------------------------------------------------------------------
def test_the_committed_floors_are_the_models():
    doc = GF.load()
    assert doc['bar_factor'] == GF.BAR_FACTOR == 8.0
    now = GF.adjoint_floors()
    assert sorted(now) == sorted(doc['adjoint']) and len(now) == 9
    for key, e in now.items():
        want = doc['adjoint'][key]
        np.testing.assert_allclose(e['scale'], want['scale'], rtol=1e-6, atol=0)
        for name in ('floor', 'sum_floor'):
            assert np.allclose(e[name], want[name], rtol=0.05, atol=1e-18), (key, name, e[name], want[name])
        assert e['scale'][2] == 0.0 and (not key.startswith('3x3') and not key.endswith('empty') or not any(e['scale']))
    assert sorted(doc['moments']) == sorted(GF.moment_key(*c) for c in GF.MOMENT_CASES) and len(doc['moments']) == 16
    for case in (('tilted', 1, 1.0, 'adjoint'), ('aligned', 0, 0.5, 'sines')):
        key, e = GF.moment_case(case)
        want = doc['moments'][key]
        np.testing.assert_allclose(e['moments'], want['moments'], rtol=1e-9, atol=1e-12 * want['scale'])
        assert abs(e['floor'] - want['floor']) <= 0.05 * want['floor'] and e['zeroed_rays'] == want['zeroed_rays'] <= 0.01
    assert all(e['zeroed_rays'] <= 0.01 and 0 < e['floor'] < 0.01 for e in doc['moments'].values())
    # the refinement cases solved by the models alone sit inside the GPU test's bars
    r, truth = doc['refinement'], FL.load()['cost_at_truth_step_0.5']
    one = r['refine_only']
    assert max(one['final_px']) <= FL.PIXEL_BAR / 2 and one['final_cost_step_0_5'] <= FL.COST_FACTOR * truth and one['halvings'] == len(one['tried']) - 1
    assert all(max(t['final_px']) > FL.PIXEL_BAR / 2 for t in one['tried'][:-1])
    assert np.allclose(one['theta0'], GF.REFINE_START * np.array(R.THETA_START) / 2 ** one['halvings'])
    for c in (one, r['cma_then_refine']):
        assert (np.diff(c['refine_cost']) <= 0).all() and c['gradient_evaluations'] <= 2 * GF.REFINE + 1
        assert max(c['final_px']) < max(c['start_px'])


# ---- the C ABI and Python ----------------------------------------------------------------------------------------------
def test_struct_mirrors_and_size_functions():
    L = nat.lib()
    for cls, size in ((nat.SimGradnccBwdArgs, 88), (nat.DrrPoseGradArgs, 136)):
        assert L.dfl_sizeof(nat._SIZEOF_ORDER.index(cls)) == C.sizeof(cls) == size
    for fn in ('dfl_sim_gradncc_bwd', 'dfl_sim_gradncc_bwd_scratch_doubles', 'dfl_drr_pose_grad', 'dfl_drr_pose_grad_scratch_doubles'):
        assert fn in nat.EXPORTS and hasattr(L, fn)
    assert L.dfl_sim_gradncc_bwd_scratch_doubles(1, 3, 3) == 6 + 4 and L.dfl_sim_gradncc_bwd_scratch_doubles(6, 45, 61) == 6 * 6 * 6 + 24
    assert L.dfl_sim_gradncc_bwd_scratch_doubles(32, 180, 180) == L.dfl_sim_scratch_doubles(32, 180, 180) + 4 * 32
    for bad in ((0, 45, 61), (65536, 45, 61), (1, 2, 61), (1, 45, 2), (-1, 45, 61), (1, 65536, 65536), (65535, 1 << 20, 16)):
        assert L.dfl_sim_gradncc_bwd_scratch_doubles(*bad) == -1 and b'dfl_sim_gradncc_bwd_scratch_doubles' in L.dfl_last_error(), bad
    assert L.dfl_drr_pose_grad_scratch_doubles(1, 1, 1, 1) == 12 and L.dfl_drr_pose_grad_scratch_doubles(2, 3, 45, 61) == 2 * 3 * 3 * 4 * 12
    assert L.dfl_drr_pose_grad_scratch_doubles(32, 3, 180, 180) == 32 * 3 * 12 * 12 * 12
    for bad in ((0, 3, 45, 61), (65536, 3, 45, 61), (1, 0, 45, 61), (1, 3, 0, 61), (1, 3, 45, 0), (1, 3, 65536, 65536), (65535, 64, 4096, 4096)):
        assert L.dfl_drr_pose_grad_scratch_doubles(*bad) == -1 and b'dfl_drr_pose_grad_scratch_doubles' in L.dfl_last_error(), bad


def test_c_abi_refuses_bad_arguments():
    """Every refusal comes back as -1 with a message, before anything is launched."""
    L = nat.lib()
    P = 4096                                                  # never dereferenced: the checks come first

    def bwd(**k):
        return nat.SimGradnccBwdArgs(**dict(dict(moving=P, fx=P, fy=P, counted=P, totals=P, scratch=P, cost=P, d_moving=P,
                                                 scratch_doubles=6 * 6 * 6 + 24, V=6, H=45, W=61), **k))

    for kw, word in ((dict(moving=None), b'required'), (dict(fx=None), b'required'), (dict(fy=None), b'required'),
                     (dict(counted=None), b'required'), (dict(totals=None), b'required'), (dict(scratch=None), b'required'),
                     (dict(cost=None), b'required'), (dict(d_moving=None), b'required'), (dict(H=2), b'3 x 3'), (dict(W=2), b'3 x 3'),
                     (dict(V=0), b'65535'), (dict(V=65536, scratch_doubles=1 << 40), b'65535'), (dict(scratch_doubles=6 * 6 * 6 + 23), b'scratch'),
                     (dict(scratch_doubles=6 * 6 * 6), b'scratch'), (dict(V=7), b'scratch'), (dict(H=51), b'scratch'),
                     (dict(H=65536, W=65536, scratch_doubles=1 << 40), b'too large')):
        a = bwd(**kw)
        assert L.dfl_sim_gradncc_bwd(C.addressof(a), None) == -1, kw
        assert word in L.dfl_last_error() and b'dfl_sim_gradncc_bwd' in L.dfl_last_error(), (kw, L.dfl_last_error())
    assert L.dfl_sim_gradncc_bwd(None, None) == -1 and b'null' in L.dfl_last_error()

    def pg(**k):
        return nat.DrrPoseGradArgs(**dict(dict(mu=P, labels=P, objects=P, d_att=P, pivots=P, grad=P, scratch=P, scratch_doubles=3 * 3 * 4 * 12,
                                               qscale=(nat.f32 * 9)(*range(9)), nx=37, ny=45, nz=53, H=45, W=61, views=1, n_obj=3,
                                               interp=nat.DRR_TRILINEAR, step_mm=1.0), **k))

    for kw, word in ((dict(mu=None), b'required'), (dict(labels=None), b'required'), (dict(objects=None), b'required'),
                     (dict(d_att=None), b'required'), (dict(pivots=None), b'required'), (dict(grad=None), b'required'),
                     (dict(scratch=None), b'required'), (dict(nx=0), b'bad sizes'), (dict(ny=-1), b'bad sizes'), (dict(nz=0), b'bad sizes'),
                     (dict(H=0), b'bad sizes'), (dict(W=0), b'bad sizes'), (dict(views=0), b'bad sizes'), (dict(n_obj=0), b'bad sizes'),
                     (dict(nx=2048, ny=2048, nz=512), b'2^31'), (dict(views=65536, scratch_doubles=1 << 40), b'65535'),
                     (dict(H=65536, W=65536, scratch_doubles=1 << 40), b'too large'), (dict(interp=nat.DRR_EXACT), b'trilinear'),
                     (dict(interp=2), b'trilinear'), (dict(step_mm=0.0), b'step_mm'), (dict(step_mm=-1.0), b'step_mm'),
                     (dict(step_mm=float('inf')), b'step_mm'), (dict(step_mm=float('nan')), b'step_mm'),
                     (dict(scratch_doubles=3 * 3 * 4 * 12 - 1), b'scratch'), (dict(views=2), b'scratch'), (dict(W=65), b'scratch')):
        a = pg(**kw)
        assert L.dfl_drr_pose_grad(C.addressof(a), None) == -1, kw
        assert word in L.dfl_last_error() and b'dfl_drr_pose_grad' in L.dfl_last_error(), (kw, L.dfl_last_error())
    assert L.dfl_drr_pose_grad(None, None) == -1 and b'null' in L.dfl_last_error()


def test_python_refusals_without_a_gpu():
    S = D.scene('tilted')
    recs = D.pack(D.scene_views(S)[0], D.MASKS, S['Q'], S['lab'], True, 'trilinear')[None]
    grid = drr.Grid(S['Q'], S['rows'], S['cols'])
    with pytest.raises(nat.DflError, match='drr.Volume'):
        drr.pose_gradient(object(), recs, grid, torch.zeros((1, 45, 61)))
    # patch + refine, a bad refine, and CPU tensors are refused before anything touches a device
    with pytest.raises(nat.DflError, match='patch'):
        reg.register(None, None, None, similarity='patch', refine=3)
    for bad in (-1, 1.5, True):
        with pytest.raises(nat.DflError, match='refine'):
            reg.register(None, None, None, refine=bad)
    with pytest.raises(nat.DflError, match='refine'):
        reg.register(None, None, None, refine=2, refine_tol=-1.0)
    with pytest.raises(nat.DflError, match='drr.Volume'):
        reg.register(object(), None, torch.zeros((45, 61)), refine=3)
    for name in ('pose_delta_jacobians', 'bfgs', 'BfgsResult'):
        assert name in reg.__all__
    assert 'pose_gradient' in drr.__all__ and 'box_pivots' in drr.__all__
