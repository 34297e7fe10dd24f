"""Similarity against a bank of fixed images and register_many on the GPU.

Everything here is an identity of bits, so there is no tolerance: a view scored against image f of a bank has the bits
the single-image entry point gives it against that image, and problem i of register_many has the bytes of the register()
call that defines it.  The accuracy of those bits is held by tests/test_gpu_register.py, tests/test_gpu_register_patch.py
and tests/test_gpu_pose_grad.py.
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
import reg_ref as R  # noqa: E402
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, drr, h5lite, preprocess as pp, register as reg  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
_CACHE = {}
FIXED_OF = [2, 0, 1, 1, 0, 2, 0]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                 # a copy: the shared arrays are read-only


def _bank_inputs(H, W, F=3):
    """(fixed [F, H, W], masks [F] of uint8 [H, W] or None, moving [7, H, W]) on the device: the fixed image of
    reg_ref.sim_images and its two rendered views as fixed images, under the masks none, ragged and empty; the six moving
    images and the fixed image itself as views."""
    key = ('bank', H, W, F)
    if key not in _CACHE:
        fixed, moving = R.sim_images(H, W)
        m = R.sim_masks(H, W)
        _CACHE[key] = (_dev(np.stack([fixed, moving[5], moving[4]][:F])), [None if k is None else _dev(k) for k in (m['none'], m['ragged'], m['empty'])][:F],
                       _dev(np.concatenate([moving, fixed[None]])))
    return _CACHE[key]


def _mask_bank(masks, H, W):
    """uint8 [F, H, W]: a bank has a mask for every image or for none; no mask is a mask of non-zero bytes."""
    return torch.stack([torch.full((H, W), 255, dtype=torch.uint8, device=DEV) if m is None else m for m in masks])


# ---- 1. the bank forward, global ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', R.SIM_SIZES)
def test_bank_cost_has_the_bits_of_similarity(size):
    H, W = size
    fixed, masks, moving = _bank_inputs(H, W)
    bank = reg.SimilarityBank(fixed, _mask_bank(masks, H, W), views=7)
    got = bank.cost(moving, FIXED_OF)
    assert got.dtype == torch.float64 and tuple(got.shape) == (7,)
    single = [reg.Similarity(fixed[f], masks[f], views=7) for f in range(3)]
    want = torch.cat([single[f].cost(moving[v:v + 1]) for v, f in enumerate(FIXED_OF)])
    print('bank %d x %d: costs %s' % (H, W, got.cpu().numpy().tolist()))
    assert torch.equal(got, want)
    assert torch.equal(want, torch.stack([single[f].cost(moving)[v] for v, f in enumerate(FIXED_OF)]))      # ... in any batch
    # the planes and totals of image f are those of Similarity(fixed[f], masks[f])
    for f in range(3):
        assert torch.equal(bank.fx[f], single[f].fx) and torch.equal(bank.fy[f], single[f].fy) and torch.equal(bank.counted[f], single[f].counted)
        assert torch.equal(bank.totals[f], single[f].totals)
    # a permuted batch, one view alone, a device tensor as fixed_of: the same bits per view
    perm = [5, 0, 6, 2, 4, 1, 3]
    assert torch.equal(bank.cost(moving[perm].contiguous(), [FIXED_OF[v] for v in perm]), got[perm])
    for v in (1, 4):
        assert torch.equal(bank.cost(moving[v:v + 1].clone(), [FIXED_OF[v]]), got[v:v + 1])
    assert torch.equal(bank.cost(moving, torch.tensor(FIXED_OF, dtype=torch.int32, device=DEV)), got)
    # every view against every image: V does not matter, nor do the other entries
    for f in range(3):
        assert torch.equal(bank.cost(moving, [f] * 7), single[f].cost(moving))
    # one image, no masks: Similarity itself
    one = reg.SimilarityBank(fixed[:1], None, views=7)
    assert torch.equal(one.cost(moving, [0] * 7), single[0].cost(moving))
    # the host check of a sequence
    with pytest.raises(nat.DflError, match='0 .. 2'):
        bank.cost(moving, [0, 1, 2, 3, 0, 0, 0])
    with pytest.raises(nat.DflError, match='one per view'):
        bank.cost(moving, [0, 1])
    with pytest.raises(nat.DflError, match='int32'):
        bank.cost(moving, torch.zeros(7, dtype=torch.int64, device=DEV))


# ---- 2. the bank adjoint -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', R.SIM_SIZES)
def test_bank_adjoint_has_the_bits_of_similarity(size):
    H, W = size
    fixed, masks, moving = _bank_inputs(H, W)
    bank = reg.SimilarityBank(fixed, _mask_bank(masks, H, W), views=7)
    cost, d = bank.cost_and_adjoint(moving, FIXED_OF)
    assert cost.dtype == torch.float64 and tuple(cost.shape) == (7,) and d.dtype == torch.float32 and tuple(d.shape) == (7, H, W)
    assert torch.equal(cost, bank.cost(moving, FIXED_OF))
    for v, f in enumerate(FIXED_OF):
        c1, d1 = reg.Similarity(fixed[f], masks[f], views=1).cost_and_adjoint(moving[v:v + 1])
        assert torch.equal(cost[v:v + 1], c1) and torch.equal(d[v:v + 1], d1), (v, f)
    assert size == (3, 3) or (d[3] != 0).any()                    # not an identity of zeros (view 5's image has the empty mask)
    perm = [3, 6, 0, 5]
    c2, d2 = bank.cost_and_adjoint(moving[perm].contiguous(), [FIXED_OF[v] for v in perm])
    assert torch.equal(c2, cost[perm]) and torch.equal(d2, d[perm])


# ---- 3. the patch bank -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W,rho,stride,F', [(45, 61, 3, 2, 3), (45, 61, 1, 1, 3), (9, 300, 3, 2, 3), (19, 1538, 3, 2, 2)])
def test_patch_bank_cost_has_the_bits_of_patch_similarity(H, W, rho, stride, F):
    """9 x 300: the threads pass over the columns twice; 19 x 1538: 6 x 1536 x 8 = 73728 bytes of dynamic LDS, above 64 KB."""
    fixed, masks, moving = _bank_inputs(H, W, F)
    fixed_of = [f % F for f in FIXED_OF]
    min_count = 5 if rho == 1 else None
    bank = reg.PatchSimilarityBank(fixed, _mask_bank(masks, H, W), 7, rho, stride, min_count)
    got = bank.cost(moving, fixed_of)
    single = [reg.PatchSimilarity(fixed[f], masks[f], 7, rho, stride, min_count) for f in range(F)]
    want = torch.cat([single[f].cost(moving[v:v + 1]) for v, f in enumerate(fixed_of)])
    print('patch bank %d x %d rho %d stride %d: costs %s' % (H, W, rho, stride, got.cpu().numpy().tolist()))
    assert torch.equal(got, want) and got.dtype == torch.float64
    for f in range(F):
        assert torch.equal(bank.ptotals[f], single[f].ptotals) and torch.equal(bank.pflags[f], single[f].pflags)
        assert torch.equal(bank.pcount[f], single[f].pcount)
        assert torch.equal(bank.cost(moving, [f] * 7), single[f].cost(moving))
    perm = [6, 2, 0, 4]
    assert torch.equal(bank.cost(moving[perm].contiguous(), [fixed_of[v] for v in perm]), got[perm])
    with pytest.raises(nat.DflError, match='adjoint'):
        bank.cost_and_adjoint(moving, fixed_of)


# ---- 4. fixed_of outside [0, F) ----------------------------------------------------------------------------------------
def test_out_of_range_views_cost_nan_and_the_others_keep_their_bits():
    H, W = 45, 61
    fixed, masks, moving = _bank_inputs(H, W)
    mv = moving[[4, 5, 0, 3]].contiguous()
    for F in (3, 2):
        bad = torch.tensor([0, -1, F, 1], dtype=torch.int32, device=DEV)
        bank = reg.SimilarityBank(fixed[:F], _mask_bank(masks[:F], H, W), views=4)
        patch = reg.PatchSimilarityBank(fixed[:F], _mask_bank(masks[:F], H, W), 4, 3, 2)
        held = [t.clone() for t in (bank.fx, bank.fy, bank.counted, bank.totals, patch.fx, patch.fy, patch.counted, patch.ptotals, patch.pflags,
                                    patch.pcount)]
        good = bank.cost_and_adjoint(mv[[0, 3]].contiguous(), [0, 1])
        good_patch = patch.cost(mv[[0, 3]].contiguous(), [0, 1])
        for cost in (bank.cost(mv, bad), patch.cost(mv, bad)):
            assert torch.isnan(cost[1:3]).all() and torch.isfinite(cost[[0, 3]]).all()
        assert torch.equal(bank.cost(mv, bad)[[0, 3]], good[0]) and torch.equal(patch.cost(mv, bad)[[0, 3]], good_patch)
        cost, d = bank.cost_and_adjoint(mv, bad)
        assert torch.isnan(cost[1:3]).all() and torch.equal(cost[[0, 3]], good[0])
        assert not d[1:3].any() and not torch.signbit(d[1:3]).any() and torch.equal(d[[0, 3]], good[1]) and d[0].any()
        now = (bank.fx, bank.fy, bank.counted, bank.totals, patch.fx, patch.fy, patch.counted, patch.ptotals, patch.pflags, patch.pcount)
        assert all(torch.equal(a, b) for a, b in zip(held, now))


# ---- 5. refusals launch nothing ----------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    L = nat.lib()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    H, W = 45, 61
    fixed, masks, moving = _bank_inputs(H, W)
    bank = reg.SimilarityBank(fixed, _mask_bank(masks, H, W), views=7)
    patch = reg.PatchSimilarityBank(fixed, _mask_bank(masks, H, W), 7, 3, 2)
    of = torch.tensor(FIXED_OF, dtype=torch.int32, device=DEV)
    need = L.dfl_sim_gradncc_bwd_scratch_doubles(7, H, W)
    pneed = L.dfl_sim_patch_scratch_doubles(7, H, W, 3, 2)
    out = torch.full((7,), -7.0, dtype=torch.float64, device=DEV)
    scratch = torch.full((max(need, pneed),), -7.0, dtype=torch.float64, device=DEV)
    d_moving = torch.full((7, H, W), -7.0, device=DEV)
    shared = dict(moving=moving.data_ptr(), fixed_of=of.data_ptr(), scratch=scratch.data_ptr(), cost=out.data_ptr(), V=7, H=H, W=W, F=3)
    planes = dict(fx=bank.fx.data_ptr(), fy=bank.fy.data_ptr(), counted=bank.counted.data_ptr())

    def fwd(**k):
        return nat.SimBankGradnccArgs(**dict(dict(shared, totals=bank.totals.data_ptr(), scratch_doubles=need, **planes), **k))

    def bwd(**k):
        return nat.SimBankGradnccBwdArgs(**dict(dict(shared, totals=bank.totals.data_ptr(), d_moving=d_moving.data_ptr(), scratch_doubles=need, **planes), **k))

    def pat(**k):
        return nat.SimPatchBankGradnccArgs(**dict(dict(shared, fx=patch.fx.data_ptr(), fy=patch.fy.data_ptr(), counted=patch.counted.data_ptr(),
                                                       ptotals=patch.ptotals.data_ptr(), pflags=patch.pflags.data_ptr(), pcount=patch.pcount.data_ptr(),
                                                       scratch_doubles=pneed, rho=3, stride=2), **k))

    common = ((dict(moving=None), b'required'), (dict(fx=None), b'required'), (dict(scratch=None), b'required'), (dict(cost=None), b'required'),
              (dict(fixed_of=None), b'fixed_of'), (dict(F=0), b'bank'), (dict(F=65536), b'bank'), (dict(H=2), b'3 x 3'), (dict(V=0), b'65535'),
              (dict(V=65536), b'65535'), (dict(scratch_doubles=5), b'scratch'))
    for make, entry, more in ((fwd, 'dfl_sim_bank_gradncc', ((dict(totals=None), b'required'),)),
                              (bwd, 'dfl_sim_bank_gradncc_bwd', ((dict(d_moving=None), b'required'), (dict(scratch_doubles=need - 1), b'scratch'))),
                              (pat, 'dfl_sim_patch_bank_gradncc', ((dict(pcount=None), b'required'), (dict(rho=0), b'radius'), (dict(stride=0), b'stride'),
                                                                   (dict(scratch_doubles=pneed - 1), b'scratch')))):
        for kw, word in common + more:
            a = make(**kw)
            assert getattr(L, entry)(C.addressof(a), stream) == -1 and word in L.dfl_last_error(), (entry, kw, L.dfl_last_error())
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (scratch == -7.0).all() and (d_moving == -7.0).all()
    # the same blocks, unchanged, run
    a = bwd()
    assert L.dfl_sim_bank_gradncc_bwd(C.addressof(a), stream) == 0
    want_c, want_d = bank.cost_and_adjoint(moving, FIXED_OF)
    assert torch.equal(out, want_c) and torch.equal(d_moving, want_d)
    a = pat()
    assert L.dfl_sim_patch_bank_gradncc(C.addressof(a), stream) == 0
    assert torch.equal(out, patch.cost(moving, FIXED_OF))
    a = fwd()
    assert L.dfl_sim_bank_gradncc(C.addressof(a), stream) == 0
    assert torch.equal(out, want_c)
    with pytest.raises(nat.DflError, match='GPU'):
        bank.cost(torch.zeros((1, H, W)), [0])
    with pytest.raises(nat.DflError, match='masks'):
        reg.SimilarityBank(fixed, _mask_bank(masks, H, W)[:2])


# ---- 6. register_many against register ---------------------------------------------------------------------------------
FIELDS = ('theta', 'cost', 'theta_cma', 'refine_cost', 'final_cost', 'similarity_cost', 'landmark_cost', 'pose', 'renders', 'gradient_evaluations')
TRUE = (0.0, 0.25, -0.15)                                         # the fixed images: the scene moved by these fractions of THETA_FEMUR
START = (0.3, 0.2, 0.1)                                           # the starts: these fractions of THETA_START


def _problems():
    """(volume, geoms [3], fixed [3, H, W], theta0 [3, 6], landmarks [3]): the tilted scene at three true offsets, each
    problem's fixed image the device's own trilinear render of its geometry; shared and never written to."""
    if 'problems' not in _CACHE:
        S = D.scene('tilted')
        vol = drr.Volume(_dev(S['mu']), _dev(S['lab']))
        ctr, X = R.volume_centre(S), R.centres_phys(S)
        geoms, fixed, lands = [], [], []
        for n, t in enumerate(TRUE):
            Dm = reg.pose_delta(t * np.array(R.THETA_FEMUR), ctr)
            named = dict(zip(drr.POSES, [Dm @ P for P in S['poses']]))
            g = drr.Geometry(S['K'], S['E'], named, S['I2P'], np.eye(3), drr.default_objects(S['E'], named, S['I2P']),
                             drr.Grid(S['Q'], S['rows'], S['cols']))
            geoms.append(g)
            fixed.append(drr.render(vol, g.objects, g.grid, interp='trilinear', step_mm=1.0)[0])
            lands.append(None if n == 1 else (X, drr.project_points(g, X) + R.LAND_OFFSETS))
        theta0 = np.array([s * np.array(R.THETA_START) for s in START])
        _CACHE['problems'] = (vol, geoms, torch.stack(fixed).contiguous(), theta0, lands)
    return _CACHE['problems']


def _same_bytes(many, one, what):
    for name in FIELDS:
        a, b = getattr(many, name), getattr(one, name)
        assert type(a) is type(b), (what, name, type(a), type(b))
        if isinstance(a, np.ndarray):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, name, a, b)
        else:
            assert a == b, (what, name, a, b)


@pytest.mark.parametrize('name,kw,with_lands', [
    ('a', dict(generations=6), False),
    ('b', dict(generations=4, refine=4), False),
    ('b_two_chunks', dict(generations=4, refine=4, max_views=16), False),
    ('c', dict(generations=6, similarity='patch', patch_radius=7, patch_stride=4), False),
    ('d', dict(generations=4, refine=3, landmark_weight=0.01), True),
    ('refine_alone', dict(generations=0, refine=3), False)])
def test_register_many_has_the_bytes_of_register(name, kw, with_lands):
    vol, geoms, fixed, theta0, lands = _problems()
    kw = dict(kw, popsize=8, step_mm=1.0)
    many_kw = dict(kw, landmarks=lands) if with_lands else kw
    got = reg.register_many(vol, geoms, fixed, theta0=theta0, **many_kw)
    kw.pop('max_views', None)
    assert len(got) == 3
    for i in range(3):
        one = reg.register(vol, geoms[i], fixed[i], theta0=theta0[i], landmarks=lands[i] if with_lands else None, **kw)
        print('%s problem %d: final cost %.6f, %d renders, %d gradient evaluations, theta %s'
              % (name, i, one.final_cost, one.renders, one.gradient_evaluations, np.round(one.theta, 4).tolist()))
        _same_bytes(got[i], one, (name, i))
        assert got[i].levels == one.levels and np.array_equal(got[i].centre, one.centre) and np.array_equal(got[i].delta, one.delta)
        assert all(np.array_equal(a, b) for a, b in zip(got[i].poses, one.poses))
    assert len({r.theta.tobytes() for r in got}) == 3             # three problems, not one three times
    if with_lands:
        assert got[0].landmark_cost > 0 and got[1].landmark_cost == 0.0 and got[2].landmark_cost > 0
    if kw.get('refine'):
        assert all(r.gradient_evaluations >= 1 and len(r.refine_cost) >= 1 for r in got)


def test_register_many_with_masks_and_start_poses():
    """masks and P0 are per problem too: one more set-up, with both."""
    vol, geoms, fixed, theta0, _ = _problems()
    H, W = geoms[0].size
    masks = _dev(np.stack([np.full((H, W), 255, np.uint8), R.sim_masks(H, W)['ragged'], np.full((H, W), 1, np.uint8)]))
    P0 = np.stack([g.poses[drr.POSES[0]] for g in geoms[::-1]])
    got = reg.register_many(vol, geoms, fixed, theta0=theta0, P0=P0, masks=masks, popsize=8, generations=3, refine=2, seed=5)
    for i in range(3):
        one = reg.register(vol, geoms[i], fixed[i], theta0=theta0[i], P0=P0[i], mask=masks[i], popsize=8, generations=3, refine=2, seed=5)
        _same_bytes(got[i], one, ('masks', i))


@pytest.mark.parametrize('kw', [dict(similarity='global'), dict(similarity='patch', patch_weight='variance')], ids=['global', 'wpatch'])
def test_register_many_of_one_problem_has_the_bytes_of_register(kw):
    """register() and register_many() share one driver; N = 1 holds the bank entry points (F = 1, fixed_of = [0, ...]) against
    the single-image ones at the smallest problem count, search and finish."""
    vol, geoms, fixed, theta0, _ = _problems()
    kw = dict(kw, popsize=16, generations=6, refine=2)
    got = reg.register_many(vol, geoms[2:], fixed[2:], theta0=theta0[2:], **kw)
    one = reg.register(vol, geoms[2], fixed[2], theta0=theta0[2], **kw)
    assert len(got) == 1 and one.gradient_evaluations >= 1
    for name in FIELDS:
        a, b = getattr(got[0], name), getattr(one, name)
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, (name, a, b)


# ---- 7. the example, end to end ----------------------------------------------------------------------------------------
SPEC, CROP = '17-1882', 2


def _write_container(path):
    """The tilted scene as a full-resolution file (the construction of tests/test_gpu_register.py) with four projections
    of the one exact rendering: projections 0, 1 and 2 have six gt-landmarks each, shifted by 0, 0.4 and 0.8 pixels so that
    their start poses differ; projection 3 has three, too few for pnp."""
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
        for p in range(4):
            pfx = SPEC + '/projections/%03d/' % p
            f[pfx + 'image/pixels'] = (1000.0 * np.exp(-att)).astype(np.float32)
            f[pfx + 'gt-seg/pixels'] = D.label_map(plen)
            for l, name in enumerate(names[:3] if p == 3 else names):
                f[pfx + 'gt-landmarks/' + name] = (uv[:, l] + 0.4 * p * np.array([1.0, -0.5])).astype(np.float32)
            for k, P in zip(drr.POSES, poses):
                f[pfx + 'gt-poses/' + k] = P
            f[pfx + 'rot-180-for-up'] = np.int64(1)


def test_example_end_to_end(tmp_path, capsys):
    import register_2d3d as single
    import register_specimen as cli
    path = os.path.join(str(tmp_path), 'full.h5')
    _write_container(path)
    prefix = os.path.join(str(tmp_path), 'run')
    opts = ['--crop', str(CROP), '--ds-factor', '1', '--gt-lands', '--generations', '5', '--refine', '2', '--popsize', '8', '--seed', '1']
    assert cli.main([path, SPEC, '--out', prefix] + opts) == 0
    out = capsys.readouterr().out
    with capsys.disabled():
        print(out)
    assert 'projection 3: left out' in out and '3 of 4 projections registered' in out
    last = out.strip().split('\n')[-1]
    assert last.startswith('rotation error: median ') and 'largest' in last and 'translation error: median ' in last
    lines = open(prefix + '_reg.csv').read().strip().split('\n')
    assert lines[0] == 'proj,start_rot_deg,start_trans_mm,rot_deg,trans_mm,final_cost,renders,gradient_evaluations' and len(lines) == 5
    for p in range(3):
        cells = lines[1 + p].split(',')
        assert len(cells) == 8 and int(cells[0]) == p and np.isfinite([float(c) for c in cells[1:]]).all()
        assert int(cells[6]) == 8 * 5 + int(cells[7]) + 1 and int(cells[7]) >= 1
    assert lines[4] == '3,,,,,,,'
    z = np.load(prefix + '_reg.npz')
    assert z['projs'].tolist() == [0, 1, 2, 3] and z['registered'].tolist() == [1, 1, 1, 0]
    assert z['poses'].shape == (4, 4, 4) and np.isfinite(z['poses'][:3]).all() and np.isnan(z['poses'][3]).all() and np.isnan(z['theta'][3]).all()
    assert len({z['poses'][p].tobytes() for p in range(3)}) == 3
    # projection 1 alone, by the single-projection example at the same settings: the same bytes
    assert single.main([path, SPEC, '1', '--out', prefix + '_one'] + opts) == 0
    capsys.readouterr()
    one = np.load(prefix + '_one_reg.npz')
    assert one['poses'][0].tobytes() == z['poses'][1].tobytes() and one['theta'].tobytes() == z['theta'][1].tobytes()
    assert one['start_poses'][0].tobytes() == z['start_poses'][1].tobytes()
    # --projs selects and orders; a projection the specimen does not have is refused
    assert cli.main([path, SPEC, '--out', prefix + '_sel', '--projs', '2,3'] + opts) == 0
    capsys.readouterr()
    sel = np.load(prefix + '_sel_reg.npz')
    assert sel['projs'].tolist() == [2, 3] and sel['poses'][0].tobytes() == z['poses'][2].tobytes()
    assert cli.main([path, SPEC, '--projs', '4'] + opts) == 1 and cli.main([path, SPEC, '--projs', '3', '--out', prefix + '_none'] + opts) == 1
