"""The outline cost on the GPU: dfl_sim_outline (csrc/sim_outline.hip) against tests/outline_ref.py, the numpy float64
restatement of DESIGN.md section 26, and registrations of the tilted scene of tests/drr_ref.py on it.

The kernel gets distance maps made by labels.edt on the device; the reference works from the label maps copied to the
host, by brute force (surface_ref.sites, dist2_to), and the device's distance maps are held against its own.
Bars: counts are exact.  Sums and cost: |got - want| <= H W 2^-52 |want| -- any order of adding n <= H W non-negative doubles
is within (n - 1) 2^-53 relative of the exact sum, for the kernel and for numpy each.  Costs the definition makes 0 or 1 are
exactly that.

Registration bars: every ellipsoid centre, projected under the true and under the found pelvis pose, within twice the
largest distance tests/golden/floors/outline.json records for the case (tests/outline_floor.py: the model alone, with the
product's optimiser).  Twice, because the float32 render flips near-tie boundary pixels and the two CMA-ES trajectories
part; the cost cannot resolve less than a pixel.
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
import labels_ref as LR  # noqa: E402
import outline_floor as FL  # noqa: E402
import outline_ref as O  # noqa: E402
import reg_ref as R  # noqa: E402
import surface_ref as SR  # noqa: E402
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, drr, h5lite, labels, png, preprocess as pp, register as reg  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
_CACHE = {}
# 33 x 130 = 4290 pixels: four full chunks of DFL_SIM_OUTLINE_CHUNK = 1024 and a ragged fifth of 194
SIZES = ((45, 61), (5, 7), (1, 9), (33, 130))
# the union of the pelvis labels, two single labels, then a set the views alone hold (8), one the fixed maps alone hold (9)
# and one that neither holds (10)
SETS6 = ((1, 2, 3, 4), (5,), (6,), (8,), (9,), (10,))
CAPS = (1.5, 5.0, 1000.0)             # below most distances, equal to some (d2 = 25), far above all


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _scene():
    if 'scene' not in _CACHE:
        S = D.scene('tilted')
        _CACHE['scene'] = (S, drr.Volume(_dev(S['mu']), _dev(S['lab'])))
    return _CACHE['scene']


def _geom(S, poses):
    named = dict(zip(drr.POSES, poses))
    return drr.Geometry(S['K'], S['E'], named, S['I2P'], np.eye(3), drr.default_objects(S['E'], named, S['I2P']),
                        drr.Grid(S['Q'], S['rows'], S['cols']))


def _scene_labels(poses_list):
    """uint8 [n, 45, 61] on the device: the label maps the GPU renders for the tilted scene under every [3 poses]."""
    S, vol = _scene()
    objs = [_geom(S, poses).objects for poses in poses_list]
    return drr.render(vol, objs, _geom(S, S['poses']).grid, 'exact')[2]


def _maps(H, W):
    """(views uint8 [3, H, W], fixed uint8 [2, H, W]) on the host, shared and never written to.  45 x 61: the scene's own
    label maps at the true and the perturbed poses, rendered on the GPU.  Else blobs and patterns.  Label 8 is stamped into
    views 0 and 1 alone, label 9 into the fixed maps alone, 40 (in no set) into both; view 2 is fixed map 0."""
    if (H, W) not in _CACHE:
        if (H, W) == (45, 61):
            S, _ = _scene()
            lab = _scene_labels([S['poses'], D.perturbed(S)]).cpu().numpy()
            views, fixed = np.stack([lab[0], lab[1], lab[0]]), np.stack([lab[0], lab[1]])      # views 0 and 1 meet the other pose's map
        else:
            b = LR.blobs(3, H, W, seed=7)
            views = np.stack([b[0], LR.pattern('random_sparse', H, W, labels.TILE), b[1]])
            fixed = np.stack([b[1], LR.pattern('checkerboard', H, W, labels.TILE) if H * W < 100 else b[2]])
        views, fixed = views.copy(), fixed.copy()
        views[:2, H // 2:H // 2 + 3, 1:4] = 8
        fixed[:, 0:2, W - 3:W] = 9
        views[0, H - 1, W // 2:] = 40
        fixed[1, 0, :W // 3] = 40
        views[2] = fixed[0]
        for a in (views, fixed):
            a.setflags(write=False)
        _CACHE[(H, W)] = views, fixed
    return _CACHE[(H, W)]


def _want(H, W, sets, cap, fixed_of):
    key = ('want', H, W, sets, cap, tuple(fixed_of))
    if key not in _CACHE:
        views, fixed = _maps(H, W)
        _CACHE[key] = O.cost_stack(views, fixed, sets, cap, fixed_of)
    return _CACHE[key]


def _close(got, want, HW):
    return bool((np.abs(got - want) <= HW * 2.0 ** -52 * np.abs(want)).all())


# ---- 1. the kernel against the model -----------------------------------------------------------------------------------
@pytest.mark.parametrize('sets', [SETS6, ((1, 2, 3, 4),)], ids=['S6', 'S1'])
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_outline_matches_the_model(size, sets):
    H, W = size
    views, fixed = _maps(H, W)
    fixed_of = [1, 0, 0]                                        # a permuted bank; view 2 is fixed map 0 itself
    d_views, d_fixed = _dev(views), _dev(fixed)
    sim = reg.OutlineSimilarity(d_fixed, [list(s) for s in sets], views=3, cap=CAPS[0])
    assert sim.F == 2 and sim.S == len(sets) and sim.scratch.numel() == 4 * 3 * len(sets) * -(-H * W // nat.SIM_OUTLINE_CHUNK)
    # the distance maps the kernel reads are the model's own
    assert np.array_equal(sim.d2_fixed.cpu().numpy(), np.stack([O.d2_stack(f, sets) for f in fixed]))
    for cap in CAPS:
        sim.cap = cap
        n_want, s_want, c_want = _want(H, W, sets, cap, fixed_of)
        got_t = sim.cost(d_views, fixed_of)
        assert got_t.dtype == torch.float64 and tuple(got_t.shape) == (3,) and got_t.is_cuda
        got, n_got, s_got = got_t.cpu().numpy(), sim.counts.cpu().numpy(), sim.sums.cpu().numpy()
        if cap == CAPS[0]:
            assert np.array_equal(sim.d2_moving.cpu().numpy(), np.stack([O.d2_stack(m, sets) for m in views]))
        err = np.abs(got - c_want) / np.maximum(np.abs(c_want), 1e-300)
        print('outline %d x %d, %d sets, cap %g: cost %s, largest relative error %.3e (bar %.3e)'
              % (H, W, len(sets), cap, ' '.join('%.6g' % c for c in got), float(err.max()), H * W * 2.0 ** -52))
        assert n_got.dtype == np.int32 and np.array_equal(n_got, n_want)
        assert _close(s_got, s_want, H * W) and _close(got, c_want, H * W)
        # the same map on both sides: exactly 0 (exactly 1 where it holds none of the sets, which the tiny sizes may do)
        assert got[2] == c_want[2] == (0.0 if n_want[2].any() else 1.0) and (s_got[2] == 0.0).all()
        assert ((got >= 0.0) & (got <= 1.0)).all() and got[0] > 0.0
        one_sided = (n_want > 0).sum(-1) == 1
        assert (s_got[one_sided] == 0.0).all() and (s_got[(n_want == 0).all(-1)] == 0.0).all()
        # equal bits: a second run, a view alone, the views permuted
        assert torch.equal(sim.cost(d_views, fixed_of), got_t)
        assert torch.equal(sim.cost(d_views[1:2].clone(), fixed_of[1:2]), got_t[1:2])
        assert torch.equal(sim.cost(d_views[[2, 0, 1]].contiguous(), [fixed_of[k] for k in (2, 0, 1)]), got_t[[2, 0, 1]])
    # one fixed map and one view (V = 1, F = 1, fixed_of NULL) gives the bank's bits
    alone = reg.OutlineSimilarity(d_fixed[1].clone(), [list(s) for s in sets], views=1, cap=CAPS[2])
    assert torch.equal(alone.cost(d_views[0:1].clone()), got_t[0:1])
    # a fixed_of entry outside the bank (a device tensor is not checked on the host): NaN for that view alone
    wild = sim.cost(d_views, torch.tensor([1, 2, 0], dtype=torch.int32, device=DEV)).cpu().numpy()
    assert np.isnan(wild[1]) and wild[0] == got[0] and wild[2] == got[2]
    assert (sim.counts[1] == 0).all() and (sim.sums[1] == 0).all() and np.array_equal(sim.counts[0].cpu().numpy(), n_want[0])


def test_costs_the_definition_makes_exact():
    """Sets that only one side holds cost exactly 1, sets that neither holds leave 1.0, a cap equal to the largest distance
    truncates nothing."""
    H, W = 33, 130
    views, fixed = _maps(H, W)
    d_views, d_fixed = _dev(views), _dev(fixed)
    for sets, want in (([[8]], [1.0, 1.0, 1.0]), ([[9]], [1.0, 1.0, 0.0]), ([[10]], [1.0, 1.0, 1.0]), ([[8], [10]], [1.0, 1.0, 1.0])):
        sim = reg.OutlineSimilarity(d_fixed[0].clone(), sets, views=3, cap=4.0)
        assert sim.cost(d_views).cpu().tolist() == want, sets
        assert (sim.sums == 0).all()
    est, gt = SR.shifted_rectangles()                            # the farthest pair is exactly 5 apart: d2 = 25, cap 5
    sim = reg.OutlineSimilarity(_dev(gt), 1, views=2, cap=5.0)
    c5 = sim.cost(_dev(np.stack([est, gt])))
    s5 = sim.sums.clone()
    assert (O.d2_stack(gt, [(1,)])[0][SR.sites(est, (1,), True)] == 25).any()
    assert sim.counts.cpu().tolist() == [[[74, 74]], [[74, 74]]] and float(c5[1]) == 0.0
    assert _close(c5[:1].cpu().numpy(), np.array([3.1027798811266067 / 5.0]), 40 * 50)
    sim.cap = 50.0
    c50 = sim.cost(_dev(np.stack([est, gt])))
    assert _close(c50[:1].cpu().numpy(), np.array([3.1027798811266067 / 50.0]), 40 * 50) and float(c50[1]) == 0.0
    assert torch.equal(sim.sums, s5)                             # min(sqrt(25), 5) is 5 itself
    sim.cap = 2.0
    assert sim.cost(_dev(est[None])).cpu().tolist() == [(140.0 / 74 + 140.0 / 74) / 4.0] and sim.sums[0].cpu().tolist() == [[140.0, 140.0]]


def test_outline_refusals_launch_nothing():
    H, W = 33, 130
    views, fixed = _maps(H, W)
    sets = [list(s) for s in SETS6]
    sim = reg.OutlineSimilarity(_dev(fixed), sets, views=3, cap=16.0)
    want = sim.cost(_dev(views), [1, 0, 0]).clone()
    counts_want, sums_want = sim.counts.clone(), sim.sums.clone()
    L = nat.lib()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    need = L.dfl_sim_outline_scratch_doubles(3, 6, H, W)
    assert need == 4 * 3 * 6 * 5 == sim.scratch.numel()
    out = torch.full((3,), -7.0, dtype=torch.float64, device=DEV)
    sums = torch.full((3, 6, 2), -7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((3, 6, 2), -7, dtype=torch.int32, device=DEV)
    scratch = torch.full((need,), -7.0, dtype=torch.float64, device=DEV)
    fixed_of = torch.tensor([1, 0, 0], dtype=torch.int32, device=DEV)

    def args(**k):
        return nat.SimOutlineArgs(**dict(dict(d2_moving=sim.d2_moving.data_ptr(), d2_fixed=sim.d2_fixed.data_ptr(), fixed_of=fixed_of.data_ptr(),
                                              counts=counts.data_ptr(), sums=sums.data_ptr(), cost=out.data_ptr(), scratch=scratch.data_ptr(),
                                              scratch_doubles=need, cap=16.0, V=3, F=2, S=6, H=H, W=W, reserved=0), **k))

    for kw, word in ((dict(d2_moving=None), b'required'), (dict(d2_fixed=None), b'required'), (dict(counts=None), b'required'),
                     (dict(sums=None), b'required'), (dict(cost=None), b'required'), (dict(scratch=None), b'required'),
                     (dict(V=0), b'65535'), (dict(V=65536), b'65535'), (dict(F=0), b'fixed maps'), (dict(S=0), b'label sets'),
                     (dict(S=32), b'label sets'), (dict(H=0), b'bad sizes'), (dict(W=-1), b'bad sizes'), (dict(H=46342, W=2), b'does not fit'),
                     (dict(cap=0.0), b'cap'), (dict(cap=float('inf')), b'cap'), (dict(cap=float('nan')), b'cap'),
                     (dict(scratch_doubles=need - 1), b'scratch')):
        a = args(**kw)
        assert L.dfl_sim_outline(C.addressof(a), stream) == -1 and word in L.dfl_last_error(), (kw, L.dfl_last_error())
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (sums == -7.0).all() and (counts == -7).all() and (scratch == -7.0).all()
    a = args()                                                    # the same block, unchanged, runs
    assert L.dfl_sim_outline(C.addressof(a), stream) == 0
    assert torch.equal(out, want) and torch.equal(counts, counts_want) and torch.equal(sums, sums_want)
    with pytest.raises(nat.DflError, match='views'):
        sim.cost(torch.zeros((4, H, W), dtype=torch.uint8, device=DEV))
    with pytest.raises(nat.DflError, match='GPU'):
        sim.cost(torch.zeros((1, H, W), dtype=torch.uint8))
    with pytest.raises(nat.DflError, match='moving label maps'):
        sim.cost(torch.zeros((1, H, W + 1), dtype=torch.uint8, device=DEV))
    with pytest.raises(nat.DflError, match='dtype'):
        sim.cost(torch.zeros((1, H, W), device=DEV))
    with pytest.raises(nat.DflError, match='0 .. 1'):
        sim.cost(_dev(views), [0, 2, 0])
    with pytest.raises(nat.DflError, match='cap'):
        reg.OutlineSimilarity(_dev(fixed), sets, cap=0.0)
    with pytest.raises(nat.DflError, match='label'):
        reg.OutlineSimilarity(_dev(fixed), [[1], [32]])
    with pytest.raises(nat.DflError, match='single map'):
        reg.OutlineSimilarity(_dev(fixed[0]), sets).cost(_dev(views[:1]), [0])


# ---- 2. registrations of the tilted scene ------------------------------------------------------------------------------
def _segmentation():
    """The model's label map at the true poses, on the device."""
    if 'seg' not in _CACHE:
        _CACHE['seg'] = _dev(FL.fixed_seg(D.scene('tilted')))
    return _CACHE['seg']


@pytest.mark.parametrize('case', ['near', 'far'])
def test_pelvis_recovers_on_the_outlines(case):
    """near: the model alone ends 0.27 px off at the most, far: 0.58 px (outline.json); the bars are twice that.  GPU: see
    the printed line."""
    S, vol = _scene()
    st, bar = FL.SETTINGS[case], FL.bar(case)
    geom = _geom(S, S['poses'])
    start = R.centre_distances(S, S['poses'][0], reg.pose_delta(st['theta0'], R.volume_centre(S)) @ S['poses'][0])
    if case == 'far':
        assert start.min() > 20, start
    res = reg.register(vol, geom, None, moving=(0, 1, 2), theta0=st['theta0'], popsize=FL.POPSIZE, generations=st['generations'],
                       sigma0=st['sigma0'], seed=FL.SEED, similarity='outline', segmentation=_segmentation(), outline_cap=FL.CAP)
    dist = R.centre_distances(S, S['poses'][0], res.pose)
    print('outline %s: centres %s -> %s px (bar %.3f), cost %.6f -> %.6f (the model: %.6f -> %.6f), %d renders, theta %s'
          % (case, ' '.join('%.2f' % d for d in start), ' '.join('%.4f' % d for d in dist), bar, res.cost[0], res.final_cost,
             FL.load()['registration'][case]['cost_first_generation'], FL.load()['registration'][case]['final_cost'], res.renders,
             np.round(res.theta, 3).tolist()))
    assert res.renders == 16 * st['generations'] + 1 and res.cost.shape == (st['generations'],) and len(res.poses) == 3
    assert res.similarity_cost == res.final_cost and res.landmark_cost == 0.0 and 0.0 <= res.final_cost <= 1.0
    assert dist.max() <= bar, dist


def test_the_truth_costs_exactly_nothing():
    """The view rendered at the true poses, against a segmentation rendered on the GPU at the same poses."""
    S, vol = _scene()
    geom = _geom(S, S['poses'])
    seg = _scene_labels([S['poses']])[0].clone()
    res = reg.register(vol, geom, None, generations=0, similarity='outline', segmentation=seg, outline_cap=16.0)
    assert res.final_cost == 0.0 and res.similarity_cost == 0.0 and res.renders == 1 and res.cost.shape == (0,)
    off = reg.register(vol, geom, None, theta0=R.THETA_START, generations=0, similarity='outline', segmentation=seg, outline_cap=16.0)
    assert 0.3 < off.final_cost < 0.8                            # the model: 0.554 at this start (outline.json)
    # the landmark term adds on the host; chosen sets are taken; a run repeats bit for bit
    X = R.centres_phys(S)
    x2d = drr.project_points(geom, X)
    kw = dict(theta0=R.THETA_START, generations=3, seed=2, similarity='outline', segmentation=seg, outline_cap=16.0)
    a, b = reg.register(vol, geom, None, **kw), reg.register(vol, geom, None, **kw)
    assert a.theta.tobytes() == b.theta.tobytes() and a.cost.tobytes() == b.cost.tobytes()
    with_lands = reg.register(vol, geom, None, landmarks=(X, x2d), landmark_weight=0.01, **kw)
    assert with_lands.landmark_cost > 0.0 and with_lands.final_cost == with_lands.similarity_cost + with_lands.landmark_cost
    union = reg.register(vol, geom, None, outline_sets=[[1, 2, 3, 4], [5], [6]], **kw)
    assert np.isfinite(union.cost).all() and union.cost.tobytes() != a.cost.tobytes()
    with pytest.raises(nat.DflError, match='segmentation'):
        reg.register(vol, geom, None, similarity='outline', segmentation=seg[:-1].contiguous())
    with pytest.raises(nat.DflError, match='GPU'):
        reg.register(vol, geom, None, similarity='outline', segmentation=seg.cpu())


# ---- the example, end to end -------------------------------------------------------------------------------------------
SPEC = '17-1882'


def _write_inputs(folder):
    """The tilted scene as a full-resolution file, as tests/test_gpu_register.py builds its own (vol, vol-seg,
    vol-landmarks, proj-params and one projection whose image is the model's exact rendering on the full detector grid),
    and a results file whose 'nn-segs' row 0 is the model's label map at the true poses."""
    S = D.scene('tilted')
    poses = S['poses']
    att = D.model('tilted', 'exact', 0)[0]
    names = pp.LAND_ORDER[:6]
    pts = R.centres_phys(S).astype(np.float32)
    uv = R.project(S, poses[0], pts.astype(np.float64))
    path = os.path.join(folder, 'full.h5')
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
        f[pfx + 'gt-seg/pixels'] = FL.fixed_seg(S)
        for l, name in enumerate(names):
            f[pfx + 'gt-landmarks/' + name] = uv[:, l].astype(np.float32)
        for k, P in zip(drr.POSES, poses):
            f[pfx + 'gt-poses/' + k] = P
        f[pfx + 'rot-180-for-up'] = np.int64(0)
    segs = os.path.join(folder, 'out.npz')
    np.savez(segs, **{'nn-segs': FL.fixed_seg(S)[None]})
    return path, segs


def test_two_stages_through_the_example(tmp_path, capsys):
    """two_stage of outline.json through examples/register_outline.py: the far start, 60 generations on the outlines, 40 on
    the gradient-NCC.  Every centre within the `far` bar after either stage."""
    import register_outline as cli
    S = D.scene('tilted')
    path, segs = _write_inputs(str(tmp_path))
    prefix = os.path.join(str(tmp_path), 'run')
    far = FL.SETTINGS['far']
    common = [path, SPEC, '0', segs, 'nn-segs', '--crop', '0', '--ds-factor', '1']
    assert cli.main(common + ['--out', prefix, '--offset', ','.join(repr(t) for t in far['theta0']), '--outline-generations',
                              str(far['generations']), '--outline-sigma', str(far['sigma0']), '--outline-cap', str(FL.CAP), '--generations',
                              str(FL.SECOND['generations']), '--sigma', str(FL.SECOND['sigma0']), '--seed', '0']) == 0
    out = capsys.readouterr().out
    with capsys.disabled():
        print(out)
    z = np.load(prefix + '_reg.npz')
    for key in ('start_poses', 'poses', 'cost', 'theta', 'similarity_cost', 'landmark_cost', 'start_lands', 'lands', 'land_names', 'outline_poses',
                'outline_cost'):
        assert key in z.files, key
    assert z['poses'].shape == (3, 4, 4) and z['outline_poses'].shape == (3, 4, 4) and z['start_poses'].shape == (3, 4, 4)
    assert z['outline_cost'].shape == (far['generations'],) and z['cost'].shape == (FL.SECOND['generations'],)
    assert png.read(prefix + '_reg.png').shape == (S['rows'], 3 * S['cols'], 3)
    bar = FL.bar('far')
    d_start, d_outline, d_final = (R.centre_distances(S, S['poses'][0], P) for P in (z['start_poses'][0], z['outline_poses'][0], z['poses'][0]))
    print('two stages: centres %s -> %s -> %s px (bar %.3f)' % tuple([' '.join('%.3f' % d for d in dd) for dd in (d_start, d_outline, d_final)] + [bar]))
    assert d_start.min() > 20 and d_outline.max() <= bar and d_final.max() <= bar
    vals = {ln.split(' = ')[0]: float(ln.split(' = ')[1].split()[0]) for ln in out.strip().split('\n') if ' = ' in ln}
    assert vals['start largest reprojection distance'] > 20 and vals['final largest reprojection distance'] <= bar + 1e-3
    assert 'outline: cost' in out and 'gradient-NCC: cost' in out and 'outline rotation error' in vals
    # the way in without landmarks: the poses of an earlier run; and too few landmarks name it
    assert cli.main(common + ['--out', prefix + '2', '--start-npz', prefix + '_reg.npz', '--outline-generations', '2', '--generations', '2',
                              '--outline-cap', '16', '--clean']) == 0
    z2 = np.load(prefix + '2_reg.npz')
    assert np.array_equal(z2['start_poses'], z['poses']) and z2['outline_cost'].shape == (2,)
    capsys.readouterr()
    csv = os.path.join(str(tmp_path), 'lands.csv')
    with open(csv, 'w') as f:
        f.write('pat,proj,land,row,col,time\n' + ''.join('%s,0,%d,10.0,%d.0,0.1\n' % (SPEC, l, 10 + 5 * l) for l in range(3)))
    assert cli.main(common + ['--lands-csv', csv]) == 1
    assert '--start-npz' in capsys.readouterr().out
