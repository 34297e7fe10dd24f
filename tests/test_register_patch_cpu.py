"""The patch-wise gradient-NCC and the landmark term of dfl_amd.register on the CPU: the numpy
model tests/patch_ref.py on its known answers, the committed floors of tests/patch_floor.py, the condition on the test
inputs that keeps kernel and model agreed about which patches count, the C ABI of csrc/sim_patch.hip (struct mirrors
and refusals: nothing is launched), landmark_penalty by hand, register()'s new refusals and the example's command line.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'examples'))

import drr_ref as D  # noqa: E402
import patch_floor as PF  # noqa: E402
import patch_ref as PT  # noqa: E402
import reg_floor as FL  # noqa: E402
import reg_ref as R  # noqa: E402
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, drr, register as reg  # noqa: E402


# ---- the model ---------------------------------------------------------------------------------------------------------
def test_model_known_answers():
    """3 fixed + 2 is reg_ref.sim_images' float32 image: its rounding leaves 6e-14 with the default patches and up to
    2e-11 with the small overlapping ones (weak patches weigh as much as strong ones), so the 1e-12 is asked of the
    default patches, and of every case for the same image taken in float64, which is affine exactly."""
    for H, W in ((45, 61), (17, 70)):
        fixed, moving = R.sim_images(H, W)
        c = PT.cost(moving, fixed)                               # radius 7, stride 4
        assert abs(c[0]) <= 1e-15 and abs(c[1] - 2) <= 1e-15 and c[2] == 1.0 and abs(c[3]) <= 1e-12, c
        assert 1e-4 < c[4] < 0.1 and 0.1 < c[5] < 1.0
        assert (PT.cost(moving, fixed, R.sim_masks(H, W)['empty'], 3, 2, 1) == 1.0).all()
        assert (PT.cost(moving, fixed, R.sim_masks(H, W)['empty']) == 1.0).all()
        assert PT.cost(moving[4], fixed) == c[4]
    for H, W, rho, s in PT.cases():
        fixed, moving = R.sim_images(H, W)
        c = PT.cost(np.stack([fixed, -fixed, moving[2], 3.0 * fixed.astype(np.float64) + 2.0]), fixed, None, rho, s, 1)
        assert abs(c[0]) <= 1e-15 and abs(c[1] - 2) <= 1e-15 and c[2] == 1.0 and abs(c[3]) <= 1e-12, (H, W, rho, s, c)
    # one patch that covers the whole interior is section 16's cost
    fixed, moving = R.sim_images(9, 9)
    assert PT.grid(9, 9, 3, 1) == (1, 1)
    for name, mask in R.sim_masks(9, 9).items():
        for mc in (1, 25):
            got, want = PT.cost(moving, fixed, mask, 3, 1, mc), R.cost(moving, fixed, mask)
            if int(R.counted(9, 9, mask).sum()) >= mc:
                assert np.abs(got - want).max() <= 1e-15, (name, mc)
            else:
                assert (got == 1.0).all()
    # a zero fixed image: no patch counts
    assert PT.cost(moving, np.zeros((9, 9), np.float32), None, 1, 1, 1).tolist() == [1.0] * 6


def test_patch_grid_by_hand():
    assert PT.grid(45, 61, 3, 2) == (19, 27)                      # (43 - 7) // 2 + 1, (59 - 7) // 2 + 1
    assert (19 - 1) * 2 + 7 == 43 and (27 - 1) * 2 + 7 == 59      # the patches reach the last interior row and column
    assert PT.grid(17, 70, 7, 8) == (1, 7)                        # (15 - 15) // 8 + 1, (68 - 15) // 8 + 1
    assert (7 - 1) * 8 + 15 == 63 < 68                            # five trailing interior columns are not used
    where = list(PT._patches(17, 70, 7, 8))
    assert len(where) == 7 and where[-1] == (slice(0, 15), slice(48, 63))
    assert PT.grid(9, 300, 1, 1) == (5, 296) and PT.grid(9, 9, 3, 2) == (1, 1) and PT.grid(9, 9, 2, 5) == (1, 1)
    for bad in ((9, 9, 4, 1), (45, 16, 7, 1), (45, 61, 0, 1), (45, 61, 1, 0)):
        with pytest.raises(ValueError):
            PT.grid(*bad)
    assert len(PT.cases()) == 14 and (9, 9, 7, 8) not in PT.cases() and (9, 300, 7, 8) not in PT.cases()
    # the unused trailing columns do not reach the cost
    fixed, moving = R.sim_images(17, 70)
    changed = moving.copy()
    changed[:, :, 65:] += 1.0                                     # interior columns j >= 63 are columns c >= 64; Sobel reaches c + 1
    assert PT.cost(changed, fixed, None, 7, 8).tolist() == PT.cost(moving, fixed, None, 7, 8).tolist()


def test_min_count_drops_thinned_patches():
    fixed, _ = R.sim_images(17, 70)
    ragged = R.sim_masks(17, 70)['ragged']
    t1, f1, _ = PT.fixed_patches(fixed, ragged, 3, 2, 1)
    t24, f24, _ = PT.fixed_patches(fixed, ragged, 3, 2, 24)
    assert t1.shape == (5 * 31, 5) and np.array_equal(t1, t24)
    assert int((f1 != 0).sum()) == 99 and int((f24 != 0).sum()) == 72
    assert ((f24 != 0) <= (t24[:, 0] >= 24)).all() and ((f1 != 0) <= (t1[:, 0] >= 1)).all()
    assert int((t1[:, 0] >= 24).sum()) < int((t1[:, 0] >= 1).sum())
    # totals by hand for one patch
    on = R.counted(17, 70, ragged)
    gx, gy = R.sobel(fixed)
    a, b = 2, 11
    sel = on[4:11, 22:29]
    x = gx[4:11, 22:29][sel]
    np.testing.assert_allclose(t1[a * 31 + b, :3], [sel.sum(), x.sum(), (x * x).sum()], rtol=1e-14)
    assert PT.default_min_count(3) == 25 and PT.default_min_count(7) == 113 and PT.default_min_count(1) == 5


def test_the_committed_floors_are_the_models():
    doc = PF.load()
    assert doc['bar_factor'] == FL.BAR_FACTOR == 8.0 and doc['patch'] == {'radius': 7, 'stride': 4}
    now = PF.sim_floors()
    assert sorted(now) == sorted(doc['similarity']) and len(now) == 14 * 3 * 2
    for key, e in now.items():
        want = doc['similarity'][key]
        assert (e['count_x'], e['count_y'], e['patches']) == (want['count_x'], want['count_y'], want['patches']), key
        np.testing.assert_allclose(e['cost'], want['cost'], atol=1e-12)
        assert abs(e['floor'] - want['floor']) <= 0.05 * want['floor'] + 1e-18, (key, e['floor'], want['floor'])
    assert now[PF.key(45, 61, 3, 2, 'none', 1)]['cost'][:3] == [0.0, 2.0, 1.0]
    assert all(c == 1.0 for k in now if '/empty/' in k for c in now[k]['cost'])
    assert all(now[k]['floor'] == 0.0 and now[k]['count_x'] == 0 for k in now if '/empty/' in k)
    # a floor of 0 (the kernel then has to give exactly 1) only where no patch counts
    assert all((e['floor'] == 0.0) == (e['count_x'] == 0 and e['count_y'] == 0) for e in now.values())
    assert all(c == 1.0 for e in now.values() if e['floor'] == 0.0 for c in e['cost'])
    floors = [e['floor'] for e in now.values() if e['floor'] > 0]
    assert len(floors) >= 48 and 1e-10 < min(floors) and max(floors) < 1e-6, (min(floors), max(floors))
    # the registration cases solved by the model alone sit inside the GPU test's bars
    r = doc['registration']
    assert sorted(r) == ['A', 'A_short', 'B', 'C', 'D', 'D_global']
    assert min(r['A']['start_px']) >= 10 and max(r['A']['final_px']) <= FL.PIXEL_BAR / 4
    assert r['A']['final_cost'] <= 1.05 * r['A']['cost_at_truth'] and r['A']['cost_first_generation'] > 0.5
    assert abs(r['A']['cost_at_truth'] - 0.00381) <= 1e-5
    assert max(r['B']['final_px']) <= FL.PIXEL_BAR / 1.5 and r['B']['landmark_weight'] == PF.LAND_WEIGHT == 0.01
    assert (r['C']['generations'], r['A_short']['generations'], r['A']['generations']) == (PF.SHORT, PF.SHORT, PF.LONG) == (30, 30, 80)
    # case C: after 30 generations the landmark term has the model nearer than the patch cost alone
    assert max(r['C']['final_px']) < 0.3 < 1.0 < max(r['A_short']['final_px'])
    # case D: the foreign bar costs the patch cost less than the global one
    assert r['D']['similarity'] == 'patch' and r['D_global']['similarity'] == 'global'
    assert max(r['D']['final_px']) < 0.45 < 0.6 < max(r['D_global']['final_px'])
    assert all(r[k]['theta'] and r[k]['popsize'] == 16 and r[k]['seed'] == 0 and r[k]['sigma0'] == 2.0 for k in r)


def test_no_patch_of_the_test_inputs_sits_at_the_variance_threshold():
    """A condition on the inputs: the kernel decides with one-pass float64 sums of float32 gradients, the model with
    two passes, and they agree about which patches count as long as no live patch has a variance ratio near 2^-40."""
    lo, hi = PT.BAND
    assert lo == 2.0 ** -44 and hi == 2.0 ** -36 and lo < R.VAR_EPS < hi
    inputs = [(R.sim_images(H, W)[0], mask, rho, s) for H, W, rho, s in PT.cases() for mask in R.sim_masks(H, W).values()]
    S = D.scene('tilted')
    inputs += [(FL.fixed_image(S).astype(np.float32), None, PF.RHO, PF.STRIDE), (PF.foreign_fixed(S).astype(np.float32), None, PF.RHO, PF.STRIDE)]
    seen = 0
    for fixed, mask, rho, s in inputs:
        for dtype in (np.float64, np.float32):
            totals, _, ratios = PT.fixed_patches(fixed, mask, rho, s, 1, dtype)      # min_count 1: every patch that can live
            live = ratios[totals[:, 0] >= 1]
            assert not ((live >= lo) & (live <= hi)).any(), (fixed.shape, rho, s, live[(live >= lo) & (live <= hi)])
            seen += live.size
    assert seen > 10000


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_struct_mirrors_match_the_library():
    L = nat.lib()
    for cls, size in ((nat.SimPatchPrepareArgs, 72), (nat.SimPatchGradnccArgs, 104)):
        assert L.dfl_sizeof(nat._SIZEOF_ORDER.index(cls)) == C.sizeof(cls) == size
    k = nat._SIZEOF_ORDER.index(nat.SimPatchPrepareArgs)
    assert nat._SIZEOF_ORDER[k + 1] is nat.SimPatchGradnccArgs and nat._SIZEOF_ORDER[-1] is nat.OptimPackArgs
    for fn in ('dfl_sim_patch_prepare', 'dfl_sim_patch_gradncc', 'dfl_sim_patch_count', 'dfl_sim_patch_scratch_doubles'):
        assert fn in nat.EXPORTS and hasattr(L, fn)
    header = open(os.path.join(ROOT, 'include', 'dfl_hip.h')).read()
    for line in ('int dfl_sim_patch_prepare(const dfl_sim_patch_prepare_args* a, dfl_stream_t stream);',
                 'int dfl_sim_patch_gradncc(const dfl_sim_patch_gradncc_args* a, dfl_stream_t stream);',
                 'int64_t dfl_sim_patch_count(int32_t H, int32_t W, int32_t rho, int32_t stride);',
                 'int64_t dfl_sim_patch_scratch_doubles(int32_t V, int32_t H, int32_t W, int32_t rho, int32_t stride);',
                 '#define DFL_SIM_PATCH_MAX_W %d' % nat.SIM_PATCH_MAX_W):
        assert line in header, line
    assert nat.SIM_PATCH_MAX_W >= 1538
    assert L.dfl_sim_patch_count(45, 61, 3, 2) == 19 * 27 and L.dfl_sim_patch_count(17, 70, 7, 8) == 7
    assert L.dfl_sim_patch_count(9, 9, 3, 1) == 1 and L.dfl_sim_patch_count(9, 300, 1, 1) == 5 * 296
    assert L.dfl_sim_patch_count(180, 180, 7, 4) == 41 * 41 and L.dfl_sim_patch_count(1538, 1538, 7, 4) == 381 * 381
    assert L.dfl_sim_patch_scratch_doubles(6, 45, 61, 3, 2) == 6 * 19 * 2 and L.dfl_sim_patch_scratch_doubles(32, 180, 180, 7, 4) == 32 * 41 * 2
    assert L.dfl_sim_patch_scratch_doubles(65535, 9, 9, 3, 1) == 65535 * 2
    for H, W, rho, s in PT.cases():
        PR, PC = PT.grid(H, W, rho, s)
        assert L.dfl_sim_patch_count(H, W, rho, s) == PR * PC and L.dfl_sim_patch_scratch_doubles(3, H, W, rho, s) == 3 * PR * 2
    for bad, word in (((2, 61, 1, 1), b'3 x 3'), ((45, 2, 1, 1), b'3 x 3'), ((45, 61, 0, 1), b'radius'), ((45, 61, 1, 0), b'stride'),
                      ((9, 9, 4, 1), b'does not fit'), ((45, 16, 7, 1), b'does not fit'), ((45, 1539, 3, 2), b'DFL_SIM_PATCH_MAX_W'),
                      ((65536, 65536, 1, 1), b'too large'), ((45, 61, 1 << 30, 1), b'does not fit')):
        assert L.dfl_sim_patch_count(*bad) == -1 and word in L.dfl_last_error() and b'dfl_sim_patch_count' in L.dfl_last_error(), bad
        assert L.dfl_sim_patch_scratch_doubles(1, *bad) == -1 and b'dfl_sim_patch_scratch_doubles' in L.dfl_last_error(), bad
    for V in (0, 65536, -1):
        assert L.dfl_sim_patch_scratch_doubles(V, 45, 61, 3, 2) == -1 and b'65535' in L.dfl_last_error()


def test_c_abi_refuses_bad_arguments():
    """Every refusal comes back as -1 with a message, before anything is launched."""
    L = nat.lib()
    P = 4096                                                  # never dereferenced: the checks come first

    def prep(**k):
        return nat.SimPatchPrepareArgs(**dict(dict(fx=P, fy=P, counted=P, ptotals=P, pflags=P, pcount=P, H=45, W=61, rho=3, stride=2,
                                                   min_count=25), **k))

    sizes = ((dict(H=2), b'3 x 3'), (dict(W=2), b'3 x 3'), (dict(H=0), b'3 x 3'), (dict(H=65536, W=65536), b'too large'),
             (dict(rho=0), b'radius'), (dict(rho=-3), b'radius'), (dict(stride=0), b'stride'), (dict(stride=-1), b'stride'),
             (dict(rho=22), b'does not fit'), (dict(H=8), b'does not fit'), (dict(W=8), b'does not fit'),
             (dict(W=nat.SIM_PATCH_MAX_W + 1), b'DFL_SIM_PATCH_MAX_W'))
    for kw, word in tuple((dict(**{f: None}), b'required') for f in ('fx', 'fy', 'counted', 'ptotals', 'pflags', 'pcount')) + sizes + \
            ((dict(min_count=0), b'min_count'), (dict(min_count=-5), b'min_count')):
        a = prep(**kw)
        assert L.dfl_sim_patch_prepare(C.addressof(a), None) == -1, kw
        assert word in L.dfl_last_error() and b'dfl_sim_patch_prepare' in L.dfl_last_error(), (kw, L.dfl_last_error())
    assert L.dfl_sim_patch_prepare(None, None) == -1 and b'null' in L.dfl_last_error()

    def sim(**k):
        return nat.SimPatchGradnccArgs(**dict(dict(moving=P, fx=P, fy=P, counted=P, ptotals=P, pflags=P, pcount=P, scratch=P, cost=P,
                                                   scratch_doubles=6 * 19 * 2, V=6, H=45, W=61, rho=3, stride=2), **k))

    fields = ('moving', 'fx', 'fy', 'counted', 'ptotals', 'pflags', 'pcount', 'scratch', 'cost')
    for kw, word in tuple((dict(**{f: None}), b'required') for f in fields) + sizes + \
            ((dict(V=0), b'65535'), (dict(V=65536, scratch_doubles=1 << 40), b'65535'), (dict(scratch_doubles=6 * 19 * 2 - 1), b'scratch'),
             (dict(V=7), b'scratch'), (dict(H=47), b'scratch'), (dict(stride=1), b'scratch'), (dict(scratch_doubles=0), b'scratch')):
        a = sim(**kw)
        assert L.dfl_sim_patch_gradncc(C.addressof(a), None) == -1, kw
        assert word in L.dfl_last_error() and b'dfl_sim_patch_gradncc' in L.dfl_last_error(), (kw, L.dfl_last_error())
    assert L.dfl_sim_patch_gradncc(None, None) == -1 and b'null' in L.dfl_last_error()


# ---- the landmark term -------------------------------------------------------------------------------------------------
def _geom(S, crop=0, factor=1, rot180=False):
    G, (H, W) = drr.training_grid(S['rows'], S['cols'], crop, factor, rot180)
    poses = dict(zip(drr.POSES, S['poses']))
    return drr.Geometry(S['K'], S['E'], poses, S['I2P'], G, drr.default_objects(S['E'], poses, S['I2P']),
                        drr.Grid(-np.linalg.inv(S['K']) @ G, H, W))


@pytest.mark.parametrize('crop,factor,rot180', [(0, 1, False), (3, 2, True)])
def test_landmark_penalty_by_hand(crop, factor, rot180):
    S = D.scene('tilted')
    geom = _geom(S, crop, factor, rot180)
    X = R.centres_phys(S)
    P = S['poses'][0]
    off = np.array([[3.0, 0.0, -1.0, 2.0, 0.0, 0.5], [4.0, 1.0, 0.0, -2.0, 0.0, 0.5]])
    x2d = drr.project_points(geom, X) + off
    # at the pose the points were projected with, the distances are the offsets: mean of 25, 1, 1, 8, 0, 0.5
    got = reg.landmark_penalty(geom, P, X, x2d, 0.5)
    assert got.shape == (1,) and abs(got[0] - 0.5 * 35.5 / 6) <= 1e-9
    x2d[:, 3] = np.nan                                            # the landmark of squared distance 8 was not found
    assert abs(reg.landmark_penalty(geom, P[None], X, x2d, 0.5)[0] - 0.5 * 27.5 / 5) <= 1e-9
    x2d[0, 0] = np.inf                                            # one coordinate is enough to drop a column
    assert abs(reg.landmark_penalty(geom, P, X, x2d, 2.0)[0] - 2.0 * 2.5 / 4) <= 1e-9
    # a batch: every pose on its own, against project_points pose by pose
    ctr = R.volume_centre(S)
    poses = reg.pose_deltas(np.array([[0] * 6, R.THETA_START, [0.5, 0, 0, 0, 1, 0]], np.float64), ctr) @ P[None]
    got = reg.landmark_penalty(geom, poses, X, x2d, 0.01)
    use = np.isfinite(x2d).all(0)
    for n in range(3):
        d = drr.project_points(reg.with_pelvis_pose(geom, poses[n]), X)[:, use] - x2d[:, use]
        assert abs(got[n] - 0.01 * (d ** 2).sum(0).mean()) <= 1e-12 * max(got[n], 1.0)
    assert got[1] > 10 * max(got[0], got[2]) and got.min() > 0   # eleven pixels off against about one
    if factor == 1 and not rot180:
        np.testing.assert_allclose(got, PT.landmark_penalty(S, poses, X, x2d, 0.01), rtol=1e-12)
    # weight 0: exact zeros, of the batch's length
    zero = reg.landmark_penalty(geom, poses, X, x2d, 0.0)
    assert zero.shape == (3,) and zero.dtype == np.float64 and not zero.any() and not np.signbit(zero).any()
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(nat.DflError, match='weight'):
            reg.landmark_penalty(geom, P, X, x2d, bad)
    with pytest.raises(nat.DflError, match='usable'):
        reg.landmark_penalty(geom, P, X, np.full((2, 6), np.nan), 1.0)
    with pytest.raises(nat.DflError, match='expected'):
        reg.landmark_penalty(geom, P, X, x2d[:, :5], 1.0)


# ---- register ----------------------------------------------------------------------------------------------------------
def test_register_refuses_before_it_touches_the_gpu():
    """The new arguments are checked first: none of these calls gets as far as asking for device tensors."""
    S = D.scene('tilted')
    geom = _geom(S)
    X = R.centres_phys(S)
    x2d = drr.project_points(geom, X)
    for kw, word in ((dict(similarity='ssd'), 'similarity'), (dict(similarity=None), 'similarity'),
                     (dict(similarity='patch', patch_radius=0), 'radius'), (dict(similarity='patch', patch_radius=2.5), 'radius'),
                     (dict(similarity='patch', patch_stride=0), 'stride'), (dict(similarity='patch', patch_min_count=0), 'min_count'),
                     (dict(landmark_weight=-0.5), 'landmark_weight'), (dict(landmark_weight=float('nan')), 'landmark_weight'),
                     (dict(landmarks=(X, x2d), levels=[(1, 2)]), 'levels'), (dict(landmarks=(X, x2d), moving=(1,)), 'pelvis'),
                     (dict(landmarks=(X, x2d), moving=(1, 2), landmark_weight=1.0), 'pelvis'),
                     (dict(landmarks=(X, np.full((2, 6), np.nan))), 'usable'), (dict(landmarks=(X, x2d[:, :4])), 'expected'),
                     (dict(landmarks=X), 'landmarks')):
        with pytest.raises(nat.DflError, match=word):
            reg.register(None, geom, None, **kw)
    with pytest.raises(nat.DflError, match='Volume'):               # and with good ones the earlier checks come as before
        reg.register(None, geom, None, similarity='patch', landmarks=(X, x2d), landmark_weight=0.01)
    import torch
    with pytest.raises(nat.DflError, match='GPU'):
        reg.PatchSimilarity(torch.zeros(45, 61))
    with pytest.raises(nat.DflError, match='radius'):
        reg.PatchSimilarity(torch.zeros(45, 61), radius=0)
    assert reg._patch_params(7, 4, None) == (7, 4, 113) and reg._patch_params(3, 2, 24) == (3, 2, 24)
    for name in ('PatchSimilarity', 'landmark_penalty'):
        assert name in reg.__all__


# ---- the example -------------------------------------------------------------------------------------------------------
def test_command_line(capsys):
    import register_2d3d as cli
    base = ['f.h5', '17-1882', '3', '--gt-lands']
    assert cli.parse_similarity(base) == (base, {'--similarity': 'global', '--patch-radius': 7, '--patch-stride': 4, '--landmark-weight': None})
    rest, o = cli.parse_similarity(['f.h5', '--similarity', 'patch', '17-1882', '--patch-radius', '5', '3', '--landmark-weight', '0.01',
                                    '--gt-lands', '--patch-stride', '2', '--seed', '4'])
    assert rest == ['f.h5', '17-1882', '3', '--gt-lands', '--seed', '4']
    assert o == {'--similarity': 'patch', '--patch-radius': 5, '--patch-stride': 2, '--landmark-weight': 0.01}
    assert cli.parse(rest)[1]['--seed'] == 4
    for bad in (['--similarity'], ['--similarity', 'local'], ['--patch-radius', '0'], ['--patch-radius', 'x'], ['--patch-stride', '0'],
                ['--patch-stride', '1.5'], ['--landmark-weight', '-1'], ['--landmark-weight', 'nan'], ['--landmark-weight']):
        assert cli.parse_similarity(base + bad) is None, bad
        assert cli.main(base + bad) == 1, bad
        out = capsys.readouterr().out
        assert out.startswith('Usage: ') and '--lands-csv FILE | --gt-lands | --offset' in out
        assert out.rstrip().endswith('[--seed 0] [--similarity global|patch] [--patch-radius 7] [--patch-stride 4] [--landmark-weight 0]')
    # the landmark term uses the landmarks that gave the start: not with --offset; the old refusals print the new text too
    for bad in (['f.h5', '17-1882', '0', '--offset', '0,0,0,0,0,0', '--landmark-weight', '0.01'],
                ['f.h5', '17-1882', '0', '--offset', '0,0,0,0,0,0', '--similarity', 'patch', '--landmark-weight', '0'],
                ['f.h5', '17-1882', '0', '--similarity', 'patch'], ['f.h5', '17-1882', '0', '--gt-lands', '--what']):
        assert cli.main(bad) == 1, bad
        assert '--landmark-weight 0]' in capsys.readouterr().out
    doc = cli.__doc__
    assert '--similarity patch' in doc and '--landmark-weight' in doc and 'similarity_cost' in doc
