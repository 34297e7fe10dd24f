"""The patch-wise gradient-NCC and the landmark term on the GPU: csrc/sim_patch.hip against
tests/patch_ref.py, and whole registrations of the tilted scene of tests/drr_ref.py under the patch cost.

Similarity bars: 8 x the floors of tests/golden/floors/register_patch.json -- the largest |float32-gradient model -
float64 model| of the cost for the same size, (radius, stride), mask and min_count (tests/patch_floor.py; both sides
the model, never the kernel).  A floor of 0 (no patch counts) means the kernel has to give exactly 1.

Registration bars (reg_ref.centre_distances, pixels): A and B 0.25 px (reg_floor.PIXEL_BAR); C and D twice the largest
distance the model alone ends at (register_patch.json: CMA-ES paths may part where fp32 rendering swaps two near-equal
candidates), and C also nearer than the same run without the landmark term.
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
import patch_floor as PF  # noqa: E402
import patch_ref as PT  # noqa: E402
import reg_floor as FL  # noqa: E402
import reg_ref as R  # noqa: E402
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, drr, h5lite, png, preprocess as pp, register as reg  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
_CACHE = {}


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                 # a copy: the shared arrays are read-only


def _floors():
    if 'floors' not in _CACHE:
        _CACHE['floors'] = PF.load()
    return _CACHE['floors']


# ---- 1. the kernels against the model ----------------------------------------------------------------------------------
@pytest.mark.parametrize('mask_name', ['none', 'ragged', 'empty'])
@pytest.mark.parametrize('case', PT.cases(), ids=lambda c: '%dx%d-r%d-s%d' % c)
def test_patch_similarity_matches_the_model(case, mask_name):
    H, W, rho, stride = case
    fixed, moving = R.sim_images(H, W)
    mask = R.sim_masks(H, W)[mask_name]
    d_fixed, d_mask, d_moving = _dev(fixed), None if mask is None else _dev(mask), _dev(moving)
    PR, PC = PT.grid(H, W, rho, stride)
    for mc in (1, PT.default_min_count(rho)):
        rec = _floors()['similarity'][PF.key(H, W, rho, stride, mask_name, mc)]
        want, bar = np.array(rec['cost']), FL.BAR_FACTOR * rec['floor']
        sim = reg.PatchSimilarity(d_fixed, d_mask, views=6, radius=rho, stride=stride, min_count=None if mc > 1 else 1)
        assert (sim.radius, sim.stride, sim.min_count, sim.patches) == (rho, stride, mc, PR * PC)
        got_t = sim.cost(d_moving)
        assert got_t.dtype == torch.float64 and tuple(got_t.shape) == (6,) and got_t.is_cuda
        got = got_t.cpu().numpy()
        print('patch gradient-NCC %d x %d, radius %d stride %d (%d x %d patches), mask %s, min_count %d (%d / %d count): cost %s, '
              'max |error| %.3e (bar %.3e)' % (H, W, rho, stride, PR, PC, mask_name, mc, rec['count_x'], rec['count_y'],
                                               ' '.join('%.6g' % c for c in got), float(np.abs(got - want).max()), bar))
        # what dfl_sim_patch_prepare left, against the model with float32 gradients: flags and counts exactly
        totals, flags, _ = PT.fixed_patches(fixed, mask, rho, stride, mc, np.float32)
        assert np.array_equal(sim.pflags.cpu().numpy(), flags)
        assert sim.pcount.cpu().numpy().tolist() == [int((flags & 1).sum()), int((flags >> 1 & 1).sum())] == [rec['count_x'], rec['count_y']]
        pt = sim.ptotals.cpu().numpy()
        assert pt.shape == (PR * PC, 5) and np.array_equal(pt[:, 0], totals[:, 0])
        assert (np.abs(pt - totals) <= 1e-12 * np.abs(totals).max(1, keepdims=True)).all()
        # the model, and the known answers
        if rec['floor'] == 0.0:
            assert rec['count_x'] == rec['count_y'] == 0 and (got == 1.0).all()
        else:
            assert np.abs(got - want).max() <= bar
            assert abs(got[0]) <= bar and abs(got[1] - 2) <= bar and got[2] == 1.0 and abs(got[3] - got[0]) <= bar
        # equal bits: a second run, view 4 alone, a permuted batch, another object
        assert torch.equal(sim.cost(d_moving), got_t)
        assert torch.equal(sim.cost(d_moving[4:5].clone()), got_t[4:5])
        assert torch.equal(sim.cost(d_moving[[5, 0, 4]].contiguous()), got_t[[5, 0, 4]])
        again = reg.PatchSimilarity(d_fixed, d_mask, views=1, radius=rho, stride=stride, min_count=mc)
        assert torch.equal(again.cost(d_moving[5:6].clone()), got_t[5:6])
        # one patch that covers the whole interior is the global cost, each within its own bar of the model
        if (H, W, rho) == (9, 9, 3) and mc == 1:
            glob = reg.Similarity(d_fixed, d_mask, views=6).cost(d_moving).cpu().numpy()
            glob_bar = FL.BAR_FACTOR * float(np.abs(R.cost(moving, fixed, mask, np.float32) - R.cost(moving, fixed, mask)).max())
            assert PR == PC == 1 and np.abs(R.cost(moving, fixed, mask) - want).max() <= 1e-15
            assert np.abs(got - glob).max() <= bar + glob_bar, (got, glob)


def test_patch_similarity_refusals_launch_nothing():
    H, W, rho, stride = 45, 61, 3, 2
    fixed, moving = R.sim_images(H, W)
    sim = reg.PatchSimilarity(_dev(fixed), None, views=6, radius=rho, stride=stride)
    mv = _dev(moving)
    L = nat.lib()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    need = L.dfl_sim_patch_scratch_doubles(6, H, W, rho, stride)
    P = L.dfl_sim_patch_count(H, W, rho, stride)
    assert need == 6 * 19 * 2 == sim.pscratch.numel() and P == 19 * 27 == sim.patches
    out = torch.full((6,), -7.0, dtype=torch.float64, device=DEV)
    scratch = torch.full((need,), -7.0, dtype=torch.float64, device=DEV)

    def args(**k):
        return nat.SimPatchGradnccArgs(**dict(dict(moving=mv.data_ptr(), fx=sim.fx.data_ptr(), fy=sim.fy.data_ptr(),
                                                   counted=sim.counted.data_ptr(), ptotals=sim.ptotals.data_ptr(), pflags=sim.pflags.data_ptr(),
                                                   pcount=sim.pcount.data_ptr(), scratch=scratch.data_ptr(), cost=out.data_ptr(),
                                                   scratch_doubles=need, V=6, H=H, W=W, rho=rho, stride=stride), **k))

    for kw, word in ((dict(moving=None), b'required'), (dict(ptotals=None), b'required'), (dict(pflags=None), b'required'),
                     (dict(pcount=None), b'required'), (dict(scratch=None), b'required'), (dict(cost=None), b'required'),
                     (dict(H=2), b'3 x 3'), (dict(V=0), b'65535'), (dict(V=65536), b'65535'), (dict(rho=0), b'radius'),
                     (dict(stride=0), b'stride'), (dict(rho=22), b'does not fit'), (dict(scratch_doubles=need - 1), b'scratch'),
                     (dict(stride=1), b'scratch')):
        a = args(**kw)
        assert L.dfl_sim_patch_gradncc(C.addressof(a), stream) == -1 and word in L.dfl_last_error(), (kw, L.dfl_last_error())
    ptotals = torch.full((P, 5), -7.0, dtype=torch.float64, device=DEV)
    pflags = torch.full((P,), 77, dtype=torch.uint8, device=DEV)
    pcount = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    for kw, word in ((dict(fx=None), b'required'), (dict(pcount=None), b'required'), (dict(W=2), b'3 x 3'), (dict(rho=0), b'radius'),
                     (dict(stride=-1), b'stride'), (dict(min_count=0), b'min_count'), (dict(rho=30), b'does not fit')):
        a = nat.SimPatchPrepareArgs(**dict(dict(fx=sim.fx.data_ptr(), fy=sim.fy.data_ptr(), counted=sim.counted.data_ptr(),
                                                ptotals=ptotals.data_ptr(), pflags=pflags.data_ptr(), pcount=pcount.data_ptr(), H=H, W=W,
                                                rho=rho, stride=stride, min_count=25), **kw))
        assert L.dfl_sim_patch_prepare(C.addressof(a), stream) == -1 and word in L.dfl_last_error(), (kw, L.dfl_last_error())
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (scratch == -7.0).all() and (ptotals == -7.0).all() and (pflags == 77).all() and (pcount == -7).all()
    a = args()                                                    # the same block, unchanged, runs
    assert L.dfl_sim_patch_gradncc(C.addressof(a), stream) == 0
    assert torch.equal(out, sim.cost(mv))
    with pytest.raises(nat.DflError, match='does not fit'):
        reg.PatchSimilarity(_dev(fixed[:16]), radius=7)
    with pytest.raises(nat.DflError, match='DFL_SIM_PATCH_MAX_W'):
        reg.PatchSimilarity(torch.zeros((9, nat.SIM_PATCH_MAX_W + 1), device=DEV), radius=1)
    with pytest.raises(nat.DflError, match='views'):
        sim.cost(torch.zeros((7, H, W), device=DEV))
    with pytest.raises(nat.DflError, match='GPU'):
        sim.cost(torch.zeros((1, H, W)))


def test_the_widest_image():
    """DFL_SIM_PATCH_MAX_W columns: the column sums of a band take 6 x 1536 doubles of LDS, above the 64 KB a kernel gets
    without asking.  A ramp along the columns is compared with itself, its negation and a constant."""
    H, W = 19, nat.SIM_PATCH_MAX_W
    rng = np.random.default_rng(3)
    fixed = (np.arange(W, dtype=np.float32)[None] * np.float32(0.01)) ** 2 + rng.standard_normal((H, W)).astype(np.float32)
    sim = reg.PatchSimilarity(_dev(fixed), None, views=3, radius=7, stride=4)
    got = sim.cost(_dev(np.stack([fixed, -fixed, np.full((H, W), np.float32(2.5))]))).cpu().numpy()
    assert sim.patches == 1 * 381 and sim.pcount.cpu().numpy().tolist() == [381, 381]
    want = PT.cost(np.stack([fixed, -fixed]), fixed, None, 7, 4, dtype=np.float32)
    assert abs(got[0]) <= 1e-12 and abs(got[1] - 2) <= 1e-12 and got[2] == 1.0 and np.abs(got[:2] - want).max() <= 1e-12


# ---- 2. registrations --------------------------------------------------------------------------------------------------
def _scene():
    """(S, volume, fixed on the device): shared, never written to."""
    if 'scene' not in _CACHE:
        S = D.scene('tilted')
        _CACHE['scene'] = (S, drr.Volume(_dev(S['mu']), _dev(S['lab'])), _dev(FL.fixed_image(S).astype(np.float32)))
    return _CACHE['scene']


def _geom(S):
    named = dict(zip(drr.POSES, S['poses']))
    return drr.Geometry(S['K'], S['E'], named, S['I2P'], np.eye(3), drr.default_objects(S['E'], named, S['I2P']),
                        drr.Grid(S['Q'], S['rows'], S['cols']))


def _run(name, fixed=None, **kw):
    """register() from reg_ref.THETA_START with lambda 16, seed 0, step 1 mm and the patches of the model runs; cached."""
    if name not in _CACHE:
        S, vol, scene_fixed = _scene()
        args = dict(theta0=R.THETA_START, popsize=FL.POPSIZE, sigma0=2.0, step_mm=FL.STEP_MM, seed=FL.SEED, similarity='patch',
                    patch_radius=PF.RHO, patch_stride=PF.STRIDE)
        args.update(kw)
        res = reg.register(vol, _geom(S), scene_fixed if fixed is None else fixed, **args)
        dist = R.centre_distances(S, S['poses'][0], res.pose)
        print('%s: centres %s px, cost %.6f -> %.6f (similarity %.6f + landmarks %.6f), %d renders'
              % (name, ' '.join('%.4f' % d for d in dist), res.cost[0], res.final_cost, res.similarity_cost, res.landmark_cost, res.renders))
        _CACHE[name] = (res, dist)
    return _CACHE[name]


def test_defaults_give_the_bits_of_a_call_without_the_new_arguments():
    S, vol, fixed = _scene()
    geom = _geom(S)
    X, x2d = PF.landmarks(S)
    plain = reg.register(vol, geom, fixed, theta0=R.THETA_START, generations=6, seed=3)
    named = reg.register(vol, geom, fixed, theta0=R.THETA_START, generations=6, seed=3, similarity='global', patch_radius=3, patch_stride=9)
    zero = reg.register(vol, geom, fixed, theta0=R.THETA_START, generations=6, seed=3, landmarks=(X, x2d), landmark_weight=0)
    for other in (named, zero):
        for field in ('theta', 'cost', 'pose', 'delta'):
            assert getattr(other, field).tobytes() == getattr(plain, field).tobytes(), field
        assert other.final_cost == plain.final_cost == plain.similarity_cost and other.landmark_cost == 0.0 and other.renders == plain.renders
    patch = reg.register(vol, geom, fixed, theta0=R.THETA_START, generations=6, seed=3, similarity='patch')
    assert patch.cost.tobytes() != plain.cost.tobytes()
    again = reg.register(vol, geom, fixed, theta0=R.THETA_START, generations=6, seed=3, similarity='patch', patch_radius=7, patch_stride=4,
                         patch_min_count=113)
    assert again.cost.tobytes() == patch.cost.tobytes() and again.theta.tobytes() == patch.theta.tobytes()


def test_case_a_the_patch_cost_recovers_the_offset():
    """The model alone: 10.9 .. 12.7 px -> 0.007 .. 0.028 px, cost 0.851 -> 0.00381 (register_patch.json)."""
    res, dist = _run('A', generations=PF.LONG)
    assert res.renders == 16 * 80 + 1 and res.cost.shape == (80,) and res.levels == [(None, 80, 45, 61)]
    assert dist.max() <= FL.PIXEL_BAR, dist
    assert res.landmark_cost == 0.0 and res.final_cost == res.similarity_cost and res.cost[0] > 0.5
    model = _floors()['registration']['A']
    assert res.final_cost <= FL.COST_FACTOR * model['cost_at_truth']


def test_case_b_the_landmark_term():
    """The model alone ends at 0.10 .. 0.14 px: the landmarks are 1.3 px off and pull."""
    S, _, _ = _scene()
    X, x2d = PF.landmarks(S)
    assert np.isnan(x2d[:, R.LAND_MISSING]).all() and np.isnan(x2d).sum() == 2
    res, dist = _run('B', generations=PF.LONG, landmarks=(X, x2d), landmark_weight=PF.LAND_WEIGHT)
    assert dist.max() <= FL.PIXEL_BAR, dist
    want = reg.landmark_penalty(_geom(S), res.pose, X, x2d, PF.LAND_WEIGHT)[0]
    assert abs(res.landmark_cost - want) <= 1e-12 and abs(want - PT.landmark_penalty(S, res.pose, X, x2d, PF.LAND_WEIGHT)[0]) <= 1e-12
    assert res.final_cost == res.similarity_cost + res.landmark_cost and 0.005 < res.landmark_cost < 0.05
    assert res.cost[0] > 1.0                                      # eleven pixels off: the term alone is above 1


def test_case_c_the_landmark_term_after_thirty_generations():
    """The model alone: 0.11 .. 0.30 px with the term, 0.08 .. 1.16 px without."""
    S, _, _ = _scene()
    X, x2d = PF.landmarks(S)
    with_term, dist = _run('C', generations=PF.SHORT, landmarks=(X, x2d), landmark_weight=PF.LAND_WEIGHT)
    without, dist0 = _run('A_short', generations=PF.SHORT)
    bar = PF.MODEL_FACTOR * max(_floors()['registration']['C']['final_px'])
    assert dist.max() <= bar, (dist, bar)
    assert dist.max() < dist0.max(), (dist, dist0)


def test_case_d_a_foreign_structure():
    """The fixed image plus a bar the CT does not hold.  The model alone: 0.10 .. 0.41 px (global cost: 0.06 .. 0.63 px)."""
    S, _, _ = _scene()
    res, dist = _run('D', fixed=_dev(PF.foreign_fixed(S).astype(np.float32)), generations=PF.LONG)
    bar = PF.MODEL_FACTOR * max(_floors()['registration']['D']['final_px'])
    assert dist.max() <= bar, (dist, bar)


def test_coarse_to_fine_levels():
    S, vol, fixed = _scene()
    geom = _geom(S)
    raw = _dev((1000.0 * np.exp(-FL.fixed_image(S))).astype(np.float32))
    res = reg.register(vol, geom, raw, theta0=R.THETA_START, levels=[(2, 20), (1, 20)], popsize=16, sigma0=2.0, seed=0, similarity='patch')
    assert res.levels == [(2, 20, 23, 31), (1, 20, 45, 61)] and res.cost.shape == (40,) and res.renders == 16 * 40 + 1
    dist = R.centre_distances(S, S['poses'][0], res.pose)
    print('two levels, patch cost: centres %s px, cost %.6f -> %.6f' % (' '.join('%.4f' % d for d in dist), res.cost[0], res.final_cost))
    assert dist.max() <= 1.0
    with pytest.raises(nat.DflError, match='level 1 .factor 4. has a grid of 12 x 16, too small for one patch of side 15'):
        reg.register(vol, geom, raw, levels=[(2, 2), (4, 2)], similarity='patch')
    small = reg.register(vol, geom, raw, theta0=R.THETA_START, levels=[(4, 2)], similarity='patch', patch_radius=3, patch_stride=1)
    assert small.levels == [(4, 2, 12, 16)] and np.isfinite(small.cost).all()
    with pytest.raises(nat.DflError, match='does not fit'):
        reg.register(vol, geom, fixed, generations=1, similarity='patch', patch_radius=22)
    masked = reg.register(vol, geom, fixed, theta0=R.THETA_START, generations=2, similarity='patch', mask=_dev(R.sim_masks(45, 61)['ragged']))
    plain = reg.register(vol, geom, fixed, theta0=R.THETA_START, generations=2, similarity='patch')
    assert np.isfinite(masked.cost).all() and masked.cost[0] != plain.cost[0]


# ---- 3. the example, end to end ----------------------------------------------------------------------------------------
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


def test_example_end_to_end(tmp_path, capsys):
    import register_2d3d as cli
    S = D.scene('tilted')
    path = os.path.join(str(tmp_path), 'full.h5')
    _write_container(path, 1)
    prefix = os.path.join(str(tmp_path), 'run')
    assert cli.main([path, SPEC, '0', '--out', prefix, '--crop', str(CROP), '--ds-factor', '1', '--similarity', 'patch', '--landmark-weight',
                     '0.01', '--gt-lands', '--generations', '40', '--sigma', '1.0']) == 0
    out = capsys.readouterr().out
    with capsys.disabled():
        print(out)
    H, W = pp.out_size(S['rows'], S['cols'], CROP, 1)
    z = np.load(prefix + '_reg.npz')
    assert z['poses'].shape == (3, 4, 4) and z['cost'].shape == (40,) and z['theta'].shape == (6,) and z['lands'].shape == (2, 6)
    assert png.read(prefix + '_reg.png').shape == (H, 3 * W, 3)
    assert z['similarity_cost'].shape == () and z['landmark_cost'].shape == ()
    # the gt-landmarks are where the true pose projects the 3D landmarks, so the start is exact (start_lands are the 2D
    # landmarks to the float32 they are stored in) and the saved term is the weight times the mean squared distance
    vals = {ln.split(' = ')[0]: float(ln.split(' = ')[1].split()[0]) for ln in out.strip().split('\n') if ' = ' in ln}
    assert vals['start largest reprojection distance'] <= 1e-3
    d = z['lands'] - z['start_lands']
    dmax = float(np.hypot(*d).max())                              # start_lands stand in for the 2D landmarks: 1e-3 px per coordinate
    assert abs(float(z['landmark_cost']) - 0.01 * float((d * d).sum(0).mean())) <= 0.01 * (2 * dmax * 2e-3 + 4e-6)
    assert 0 < float(z['similarity_cost']) < 1 and float(z['landmark_cost']) >= 0 and z['cost'][-1] < z['cost'][0]
    if float(z['landmark_cost']) > 0:
        assert 'pelvis: similarity %.6f, landmark term %.6f' % (float(z['similarity_cost']), float(z['landmark_cost'])) in out
    # the same run with the global cost and no landmark term differs, and saves zeros for the term
    assert cli.main([path, SPEC, '0', '--out', prefix + '2', '--crop', str(CROP), '--ds-factor', '1', '--gt-lands', '--generations', '3']) == 0
    capsys.readouterr()
    z2 = np.load(prefix + '2_reg.npz')
    assert float(z2['landmark_cost']) == 0.0 and z2['cost'].shape == (3,) and float(z2['similarity_cost']) > 0
