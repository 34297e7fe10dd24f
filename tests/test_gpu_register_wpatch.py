"""The weighted patch gradient-NCC and the patch adjoint on the GPU: dfl_sim_patch_weights and
dfl_sim_patch_eval (csrc/sim_patch.hip) against tests/patch_grad_ref.py, and whole registrations of the tilted scene of
tests/drr_ref.py under the weighted patch cost, refined on its adjoint.

Bars: 8 x the floors of tests/golden/floors/register_wpatch.json -- the largest |float32 model - float64 model| of the
weighted cost and, per weighting and view, of the adjoint as a fraction of the view's largest |adjoint| (views 0, 1 and 3
sit at an extremum: the scale of view 4), for the same size, (radius, stride), mask and min_count (tests/patch_grad_floor.py;
both sides the model, never the kernel).  A floor of 0 means exact equality: a cost of exactly 1, an adjoint of exact zeros.

Registration bars (reg_ref.centre_distances, pixels): E and F 0.25 px (reg_floor.PIXEL_BAR; the models alone end within
half of it), G twice the largest distance the model alone ends at.
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
import patch_grad_floor as GF  # noqa: E402
import patch_grad_ref as PG  # noqa: E402
import patch_ref as PT  # noqa: E402
import reg_floor as FL  # noqa: E402
import reg_ref as R  # noqa: E402
import test_gpu_register_many as MANY  # noqa: E402  (its scenes, problems and containers; nothing of it is collected here)
import test_gpu_register_patch as PATCH  # noqa: E402
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, drr, register as reg  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
_CACHE = {}
FIXED_OF = MANY.FIXED_OF


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                 # a copy: the shared arrays are read-only


def _floors():
    if 'floors' not in _CACHE:
        _CACHE['floors'] = GF.load()
    return _CACHE['floors']


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _eval_args(sim, moving, scratch, cost, d_moving=None, weighted=False, fixed_of=None, over=()):
    """A dfl_sim_patch_eval block from the buffers of a PatchSimilarity or PatchSimilarityBank."""
    a = dict(moving=moving.data_ptr(), fx=sim.fx.data_ptr(), fy=sim.fy.data_ptr(), counted=sim.counted.data_ptr(), ptotals=sim.ptotals.data_ptr(),
             pflags=sim.pflags.data_ptr(), pcount=sim.pcount.data_ptr(), pweights=sim.pweights.data_ptr() if weighted else None,
             pwsum=sim.pwsum.data_ptr() if weighted else None, fixed_of=None if fixed_of is None else fixed_of.data_ptr(),
             scratch=scratch.data_ptr(), cost=cost.data_ptr(), d_moving=None if d_moving is None else d_moving.data_ptr(),
             scratch_doubles=scratch.numel(), V=int(moving.shape[0]), H=sim.H, W=sim.W, rho=sim.radius, stride=sim.stride, F=getattr(sim, 'F', 1))
    a.update(over)                                                # fields a refusal test replaces
    return nat.SimPatchEvalArgs(**a)


def _eval(sim, moving, bwd, weighted=False, fixed_of=None):
    """dfl_sim_patch_eval through nat.call on fresh buffers: (cost [V], d_moving [V, H, W] or None)."""
    V = int(moving.shape[0])
    need = nat.lib().dfl_sim_patch_eval_scratch_doubles(V, sim.H, sim.W, sim.radius, sim.stride, int(bwd))
    scratch = torch.empty(need, dtype=torch.float64, device=DEV)
    cost = torch.empty(V, dtype=torch.float64, device=DEV)
    d = torch.full((V, sim.H, sim.W), float('nan'), device=DEV) if bwd else None
    nat.call('dfl_sim_patch_eval', _eval_args(sim, moving, scratch, cost, d, weighted, fixed_of), _stream())
    return cost, d


# ---- 1. the kernels against the model ----------------------------------------------------------------------------------
@pytest.mark.parametrize('mask_name', ['none', 'ragged', 'empty'])
@pytest.mark.parametrize('case', PG.cases(), ids=lambda c: '%dx%d-r%d-s%d' % c)
def test_weighted_patch_similarity_and_both_adjoints_match_the_model(case, mask_name):
    H, W, rho, stride = case
    fixed, moving = R.sim_images(H, W)
    mask = R.sim_masks(H, W)[mask_name]
    d_fixed, d_mask, d_moving = _dev(fixed), None if mask is None else _dev(mask), _dev(moving)
    PR, PC = PT.grid(H, W, rho, stride)
    for mc in sorted({1, PT.default_min_count(rho)}):
        rec = _floors()['similarity'][GF.key(H, W, rho, stride, mask_name, mc)]
        want, bar = np.array(rec['cost']), GF.cost_bar(H, W, rho, stride, mask_name, mc)
        sim = reg.PatchSimilarity(d_fixed, d_mask, views=6, radius=rho, stride=stride, min_count=mc, weight='variance')
        plain = reg.PatchSimilarity(d_fixed, d_mask, views=6, radius=rho, stride=stride, min_count=mc)
        assert sim.entry == 'dfl_sim_patch_eval' and plain.entry == 'dfl_sim_patch_gradncc' and sim.patches == PR * PC
        # the weights against the model with float32 gradients
        w, tot = PG.weights(fixed, mask, rho, stride, mc, np.float32)
        got_w, got_tot = sim.pweights.cpu().numpy(), sim.pwsum.cpu().numpy()
        flags = sim.pflags.cpu().numpy()
        assert got_w.shape == (PR * PC, 2) and np.array_equal(got_w > 0, np.stack([flags & 1, flags >> 1 & 1], 1).astype(bool))
        assert np.abs(got_w - w).max() <= 1e-12 * w.max() and np.abs(got_tot - tot).max() <= 1e-12 * w.max()
        assert np.array_equal(got_tot > 0, sim.pcount.cpu().numpy() > 0)
        # the weighted cost
        got_t = sim.cost(d_moving)
        got = got_t.cpu().numpy()
        print('weighted patch gradient-NCC %d x %d, radius %d stride %d (%d x %d patches), mask %s, min_count %d: cost %s, max |error| %.3e '
              '(bar %.3e)' % (H, W, rho, stride, PR, PC, mask_name, mc, ' '.join('%.6g' % c for c in got), float(np.abs(got - want).max()), bar))
        if rec['floor'] == 0.0:
            assert (got == 1.0).all()
        else:
            assert np.abs(got - want).max() <= bar
            assert abs(got[0]) <= bar and abs(got[1] - 2) <= bar and got[2] == 1.0
        # the adjoint of either weighting: the weighted one through the class, the uniform one through the C entry point
        terms = PG.patch_terms(moving, fixed, mask, rho, stride, mc)
        c_w, d_w = sim.cost_and_adjoint(d_moving)
        c_u, d_u = _eval(plain, d_moving, True)
        assert torch.equal(c_w, got_t) and torch.equal(c_u, plain.cost(d_moving))         # the forward's bits, with and without d_moving
        assert d_w.dtype == torch.float32 and tuple(d_w.shape) == (6, H, W)
        for weight, d_got in (('variance', d_w), ('uniform', d_u)):
            _, d_want = PG.adjoint(moving, fixed, mask, rho, stride, mc, np.float64, weight, terms)
            bars, scale = GF.adjoint_bars(H, W, rho, stride, mask_name, mc, weight)
            err = np.abs(d_got.cpu().numpy().astype(np.float64) - d_want).max((1, 2))
            print('   adjoint (%s): max |error| / scale %s (bars %s)' % (weight, ' '.join('%.2e' % (e / s if s > 0 else e) for e, s in zip(err, scale)),
                                                                           ' '.join('%.2e' % (b / s if s > 0 else b) for b, s in zip(bars, scale))))
            assert (err <= bars).all(), (weight, err, bars)
            assert not d_got[2].any()                             # the constant image: exact zeros
        # equal bits: a second run, view 4 alone, a permuted batch
        for again in (sim.cost_and_adjoint(d_moving), ):
            assert torch.equal(again[0], c_w) and torch.equal(again[1], d_w)
        one = sim.cost_and_adjoint(d_moving[4:5].clone())
        assert torch.equal(one[0], c_w[4:5]) and torch.equal(one[1], d_w[4:5])
        perm = sim.cost_and_adjoint(d_moving[[5, 0, 4]].contiguous())
        assert torch.equal(perm[0], c_w[[5, 0, 4]]) and torch.equal(perm[1], d_w[[5, 0, 4]])
        # one patch that covers the whole interior is the global cost and the global adjoint, each within its own bar of its model
        if (H, W, rho) == (9, 9, 3) and mc == 1:
            import grad_ref as G
            glob_c, glob_d = reg.Similarity(d_fixed, d_mask, views=6).cost_and_adjoint(d_moving)
            _, g64 = G.sim_adjoint(moving, fixed, mask)           # the global floors have no 9 x 9 case: measured here, the same way
            _, g32 = G.sim_adjoint(moving, fixed, mask, dtype=np.float32)
            gbars = FL.BAR_FACTOR * np.abs(g32.astype(np.float64) - g64).max((1, 2))
            glob_bar = FL.BAR_FACTOR * float(np.abs(R.cost(moving, fixed, mask, np.float32) - R.cost(moving, fixed, mask)).max())
            assert PR == PC == 1 and np.abs(got - glob_c.cpu().numpy()).max() <= bar + glob_bar
            diff = np.abs(d_w.cpu().numpy().astype(np.float64) - glob_d.cpu().numpy().astype(np.float64)).max((1, 2))
            wbars, _ = GF.adjoint_bars(H, W, rho, stride, mask_name, mc, 'variance')
            assert (diff <= wbars + gbars).all(), (diff, wbars, gbars)


def test_eval_has_the_bits_of_the_existing_entry_points():
    """With pweights, fixed_of and d_moving all NULL: dfl_sim_patch_gradncc; with fixed_of: dfl_sim_patch_bank_gradncc."""
    for H, W, rho, stride in ((45, 61, 3, 2), (9, 300, 1, 1), (17, 70, 7, 8)):
        fixed, masks, moving = MANY._bank_inputs(H, W)
        mc = 5 if rho == 1 else None
        bank = reg.PatchSimilarityBank(fixed, MANY._mask_bank(masks, H, W), 7, rho, stride, mc)
        of = torch.tensor(FIXED_OF, dtype=torch.int32, device=DEV)
        c, _ = _eval(bank, moving, False, fixed_of=of)
        assert torch.equal(c, bank.cost(moving, FIXED_OF))
        c_b, d_b = _eval(bank, moving, True, fixed_of=of)
        assert torch.equal(c_b, c) and torch.isfinite(d_b).all()
        for f in range(3):
            single = reg.PatchSimilarity(fixed[f], masks[f], 7, rho, stride, mc)
            c1, _ = _eval(single, moving, False)
            assert torch.equal(c1, single.cost(moving))
            c2, d2 = _eval(single, moving, True)
            assert torch.equal(c2, c1)
            mine = [v for v, g in enumerate(FIXED_OF) if g == f]
            assert torch.equal(d_b[mine], d2[mine]) and torch.equal(c_b[mine], c1[mine])      # the uniform adjoint: bank against single


@pytest.mark.parametrize('H,W,rho,stride,F', [(45, 61, 3, 2, 3), (17, 70, 1, 4, 3), (19, 1538, 3, 2, 2)])
def test_weighted_bank_has_the_bits_of_the_single_image_calls(H, W, rho, stride, F):
    """F = 3, V = 7; 19 x 1538: 6 x 1536 x 8 = 73728 bytes of dynamic LDS in the forward, 97 tiles across in the adjoint."""
    fixed, masks, moving = MANY._bank_inputs(H, W, F)
    fixed_of = [f % F for f in FIXED_OF]
    bank = reg.PatchSimilarityBank(fixed, MANY._mask_bank(masks, H, W), 7, rho, stride, 1, weight='variance')
    assert bank.entry == 'dfl_sim_patch_eval' and tuple(bank.pweights.shape) == (F, bank.patches, 2) and tuple(bank.pwsum.shape) == (F, 2)
    cost, d = bank.cost_and_adjoint(moving, fixed_of)
    assert torch.equal(cost, bank.cost(moving, fixed_of)) and cost.dtype == torch.float64 and tuple(d.shape) == (7, H, W)
    single = [reg.PatchSimilarity(fixed[f], masks[f], 7, rho, stride, 1, weight='variance') for f in range(F)]
    for f in range(F):
        assert torch.equal(bank.pweights[f], single[f].pweights) and torch.equal(bank.pwsum[f], single[f].pwsum)
    for v, f in enumerate(fixed_of):
        c1, d1 = single[f].cost_and_adjoint(moving[v:v + 1])
        assert torch.equal(cost[v:v + 1], c1) and torch.equal(d[v:v + 1], d1), (v, f)
    assert d[3].any()
    perm = [6, 2, 0, 4]
    c2, d2 = bank.cost_and_adjoint(moving[perm].contiguous(), [fixed_of[v] for v in perm])
    assert torch.equal(c2, cost[perm]) and torch.equal(d2, d[perm])
    if W == 1538:                                                 # the cost within its bar of the model, measured here for this size
        f_np, m_np = fixed[0].cpu().numpy(), moving[[0, 4]].cpu().numpy()
        c64 = PG.cost(m_np, f_np, None, rho, stride, 1)
        c32 = PG.cost(m_np, f_np, None, rho, stride, 1, np.float32)
        got = single[0].cost(moving[[0, 4]].contiguous()).cpu().numpy()
        print('19 x 1538: weighted cost %s, model %s, floor %.3e' % (got, c64, np.abs(c32 - c64).max()))
        assert np.abs(got - c64).max() <= FL.BAR_FACTOR * np.abs(c32 - c64).max()


def test_out_of_range_views_cost_nan_and_get_zero_planes():
    H, W = 45, 61
    fixed, masks, moving = MANY._bank_inputs(H, W)
    mv = moving[[4, 5, 0, 3]].contiguous()
    for F in (3, 2):
        bad = torch.tensor([0, -1, F, 1], dtype=torch.int32, device=DEV)
        bank = reg.PatchSimilarityBank(fixed[:F], MANY._mask_bank(masks[:F], H, W), 4, 3, 2, weight='variance')
        held = [t.clone() for t in (bank.fx, bank.ptotals, bank.pflags, bank.pcount, bank.pweights, bank.pwsum)]
        good = bank.cost_and_adjoint(mv[[0, 3]].contiguous(), [0, 1])
        for weighted in (True, False):
            cost, d = _eval(bank, mv, True, weighted, bad)
            assert torch.isnan(cost[1:3]).all() and torch.isfinite(cost[[0, 3]]).all()
            assert not d[1:3].any() and not torch.signbit(d[1:3]).any() and d[0].any()
            if weighted:
                assert torch.equal(cost[[0, 3]], good[0]) and torch.equal(d[[0, 3]], good[1])
        cost, d = bank.cost_and_adjoint(mv, bad)
        assert torch.isnan(cost[1:3]).all() and torch.equal(cost[[0, 3]], good[0]) and torch.equal(d[[0, 3]], good[1]) and not d[1:3].any()
        assert torch.isnan(bank.cost(mv, bad)[1:3]).all()
        assert all(torch.equal(a, b) for a, b in zip(held, (bank.fx, bank.ptotals, bank.pflags, bank.pcount, bank.pweights, bank.pwsum)))


def test_refusals_launch_nothing():
    L = nat.lib()
    H, W, rho, stride = 45, 61, 3, 2
    fixed, masks, moving = MANY._bank_inputs(H, W)
    bank = reg.PatchSimilarityBank(fixed, MANY._mask_bank(masks, H, W), 7, rho, stride, weight='variance')
    of = torch.tensor(FIXED_OF, dtype=torch.int32, device=DEV)
    need = L.dfl_sim_patch_eval_scratch_doubles(7, H, W, rho, stride, 1)
    assert need == 7 * 19 * 2 + 4 * 7 * 19 * 27
    out = torch.full((7,), -7.0, dtype=torch.float64, device=DEV)
    scratch = torch.full((need,), -7.0, dtype=torch.float64, device=DEV)
    d = torch.full((7, H, W), -7.0, device=DEV)
    for kw, word in ((dict(moving=None), b'required'), (dict(pcount=None), b'required'), (dict(cost=None), b'required'),
                     (dict(pweights=None), b'come together'), (dict(pwsum=None), b'come together'), (dict(F=0), b'bank'), (dict(F=65536), b'bank'),
                     (dict(H=2), b'3 x 3'), (dict(V=0), b'65535'), (dict(rho=0), b'radius'), (dict(stride=0), b'stride'), (dict(rho=22), b'does not fit'),
                     (dict(scratch_doubles=need - 1), b'scratch'), (dict(scratch_doubles=7 * 19 * 2), b'scratch'), (dict(stride=1), b'scratch')):
        a = _eval_args(bank, moving, scratch, out, d, True, of, kw)
        assert L.dfl_sim_patch_eval(C.addressof(a), _stream()) == -1 and word in L.dfl_last_error(), (kw, L.dfl_last_error())
    pw = torch.full((bank.patches, 2), -7.0, dtype=torch.float64, device=DEV)
    ps = torch.full((2,), -7.0, dtype=torch.float64, device=DEV)
    for kw in (dict(ptotals=None), dict(pflags=None), dict(pweights=None), dict(pwsum=None), dict(P=0)):
        a = nat.SimPatchWeightsArgs(**dict(dict(ptotals=bank.ptotals.data_ptr(), pflags=bank.pflags.data_ptr(), pweights=pw.data_ptr(),
                                                pwsum=ps.data_ptr(), P=bank.patches), **kw))
        assert L.dfl_sim_patch_weights(C.addressof(a), _stream()) == -1
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (scratch == -7.0).all() and (d == -7.0).all() and (pw == -7.0).all() and (ps == -7.0).all()
    a = _eval_args(bank, moving, scratch, out, d, True, of)       # the same block, unchanged, runs
    assert L.dfl_sim_patch_eval(C.addressof(a), _stream()) == 0
    want = bank.cost_and_adjoint(moving, FIXED_OF)
    assert torch.equal(out, want[0]) and torch.equal(d, want[1])
    single = reg.PatchSimilarity(fixed[0], None, 7, rho, stride)
    with pytest.raises(nat.DflError, match='adjoint'):
        single.cost_and_adjoint(moving)
    with pytest.raises(nat.DflError, match='views'):
        reg.PatchSimilarity(fixed[0], None, 6, rho, stride, weight='variance').cost_and_adjoint(moving)


# ---- 2. registrations --------------------------------------------------------------------------------------------------
def _run(name, fixed=None, **kw):
    """register() with lambda 16, seed 0, step 1 mm and the patches of the model runs; cached."""
    if name not in _CACHE:
        S, vol, scene_fixed = PATCH._scene()
        args = dict(theta0=R.THETA_START, popsize=FL.POPSIZE, sigma0=2.0, step_mm=FL.STEP_MM, seed=FL.SEED, similarity='patch',
                    patch_radius=GF.RHO, patch_stride=GF.STRIDE, patch_weight='variance')
        args.update(kw)
        res = reg.register(vol, PATCH._geom(S), scene_fixed if fixed is None else fixed, **args)
        dist = R.centre_distances(S, S['poses'][0], res.pose)
        print('%s: centres %s px, cost %.6f -> %.6f, %d renders, %d gradient evaluations'
              % (name, ' '.join('%.4f' % d for d in dist), res.cost[0] if len(res.cost) else float('nan'), res.final_cost, res.renders,
                 res.gradient_evaluations))
        _CACHE[name] = (res, dist)
    return _CACHE[name]


def test_case_e_the_weighted_cost_recovers_the_offset():
    res, dist = _run('E', generations=GF.GENERATIONS)
    assert res.renders == 16 * 80 + 1 and res.cost.shape == (80,)
    assert dist.max() <= FL.PIXEL_BAR, dist


def test_case_f_the_quasi_newton_finish_alone():
    model = _floors()['registration']['F']
    res, dist = _run('F', theta0=np.array(model['theta0']), generations=0, refine=GF.REFINE)
    assert res.cost.shape == (0,) and res.gradient_evaluations >= 2
    assert len(res.refine_cost) >= 2 and res.refine_cost[-1] < res.refine_cost[0] and res.final_cost <= res.refine_cost[0]
    assert np.array_equal(res.theta_cma, np.array(model['theta0']))
    assert dist.max() <= FL.PIXEL_BAR, dist


def test_case_g_a_textured_projection():
    """No patch of the textured image drops out: the uniform patch cost at the true pose is a third, the weighted one small."""
    S, _, _ = PATCH._scene()
    model = _floors()['registration']
    tex = _dev(GF.textured_fixed(S).astype(np.float32))
    res, dist = _run('G', fixed=tex, generations=GF.GENERATIONS)
    uni, dist_u = _run('G_uniform', fixed=tex, generations=GF.GENERATIONS, patch_weight='uniform')
    bar = GF.MODEL_FACTOR * max(model['G']['final_px'])
    print('G: the model alone ends at %.4f px (weighted) and %.4f px (uniform); here %.4f and %.4f'
          % (max(model['G']['final_px']), max(model['G_uniform']['final_px']), dist.max(), dist_u.max()))
    assert dist.max() <= bar, (dist, bar)
    assert res.final_cost < uni.final_cost / 5


def test_patch_weight_uniform_is_the_call_without_it():
    S, vol, fixed = PATCH._scene()
    geom = PATCH._geom(S)
    for kw in (dict(similarity='patch'), dict(), dict(refine=2)):
        plain = reg.register(vol, geom, fixed, theta0=R.THETA_START, generations=4, seed=3, **kw)
        named = reg.register(vol, geom, fixed, theta0=R.THETA_START, generations=4, seed=3, patch_weight='uniform', **kw)
        for field in ('theta', 'cost', 'pose', 'delta', 'refine_cost', 'theta_cma'):
            assert getattr(named, field).tobytes() == getattr(plain, field).tobytes(), field
        assert named.final_cost == plain.final_cost and named.renders == plain.renders
    weighted = reg.register(vol, geom, fixed, theta0=R.THETA_START, generations=4, seed=3, similarity='patch', patch_weight='variance')
    assert weighted.cost.tobytes() != plain.cost.tobytes()
    # levels work as for the patch cost, and the finish runs on the last level's grid
    raw = _dev((1000.0 * np.exp(-FL.fixed_image(S))).astype(np.float32))
    res = reg.register(vol, geom, raw, theta0=R.THETA_START, levels=[(2, 4), (1, 4)], similarity='patch', patch_weight='variance', refine=2)
    assert res.levels == [(2, 4, 23, 31), (1, 4, 45, 61)] and res.gradient_evaluations >= 1 and np.isfinite(res.refine_cost).all()


@pytest.mark.parametrize('name,kw', [('weighted', dict(generations=4, refine=3)), ('weighted_two_chunks', dict(generations=4, refine=3, max_views=16))])
def test_register_many_has_the_bytes_of_register(name, kw):
    vol, geoms, fixed, theta0, _ = MANY._problems()
    kw = dict(kw, popsize=8, step_mm=1.0, similarity='patch', patch_weight='variance')
    got = reg.register_many(vol, geoms, fixed, theta0=theta0, **kw)
    kw.pop('max_views', None)
    for i in range(3):
        one = reg.register(vol, geoms[i], fixed[i], theta0=theta0[i], **kw)
        print('%s problem %d: final cost %.6f, %d renders, %d gradient evaluations' % (name, i, one.final_cost, one.renders, one.gradient_evaluations))
        MANY._same_bytes(got[i], one, (name, i))
    assert len({r.theta.tobytes() for r in got}) == 3 and all(r.gradient_evaluations >= 1 for r in got)


# ---- 3. the examples, end to end ---------------------------------------------------------------------------------------
def test_examples_end_to_end(tmp_path, capsys):
    import register_2d3d as one
    import register_specimen as many
    path = os.path.join(str(tmp_path), 'full.h5')
    PATCH._write_container(path, 1)
    prefix = os.path.join(str(tmp_path), 'run')
    tail = ['--crop', str(PATCH.CROP), '--ds-factor', '1', '--similarity', 'patch', '--patch-weight', 'variance', '--refine', '2', '--gt-lands',
            '--generations', '5']
    assert one.main([path, PATCH.SPEC, '0', '--out', prefix] + tail) == 0
    out = capsys.readouterr().out
    assert 'refinement cost' in out
    z = np.load(prefix + '_reg.npz')
    assert z['cost'].shape == (5,) and np.isfinite(z['theta']).all() and 0 < float(z['similarity_cost']) < 1
    path2 = os.path.join(str(tmp_path), 'many.h5')
    MANY._write_container(path2)
    assert many.main([path2, MANY.SPEC, '--out', prefix + 'm', '--projs', '0,1'] + tail) == 0
    capsys.readouterr()
    zm = np.load(prefix + 'm_reg.npz')
    assert zm['registered'].tolist() == [1, 1] and np.isfinite(zm['theta']).all()
