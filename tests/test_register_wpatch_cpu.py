"""The weighted patch gradient-NCC and the patch adjoint on the CPU: the numpy model
tests/patch_grad_ref.py on its known answers, by hand and against central differences, the committed floors of
tests/patch_grad_floor.py, the C ABI of dfl_sim_patch_weights / dfl_sim_patch_eval (struct mirrors and refusals: nothing is
launched), the option patch_weight of register() and register_many(), and the examples' --patch-weight.
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
import patch_grad_floor as GF  # noqa: E402
import patch_grad_ref as PG  # noqa: E402
import patch_ref as PT  # noqa: E402
import reg_floor as FL  # noqa: E402
import reg_ref as R  # noqa: E402
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, drr, register as reg  # noqa: E402


# ---- the model ---------------------------------------------------------------------------------------------------------
def test_model_known_answers():
    for H, W in ((45, 61), (17, 70)):
        fixed, moving = R.sim_images(H, W)
        c = PG.cost(moving, fixed)                               # radius 7, stride 4, weighted
        assert abs(c[0]) <= 1e-15 and abs(c[1] - 2) <= 1e-15 and c[2] == 1.0 and abs(c[3]) <= 1e-12, c
        assert 1e-4 < c[4] < 0.1 and 0.1 < c[5] < 1.0
        assert (PG.cost(moving, fixed, R.sim_masks(H, W)['empty'], 3, 2, 1) == 1.0).all()
        assert abs(PG.cost(moving[4], fixed) - c[4]) <= 1e-15    # numpy adds a batch of views in another order than one view
        # the uniform weighting is section 18's cost
        assert np.abs(PG.cost(moving, fixed, None, 3, 2, weight='uniform') - PT.cost(moving, fixed, None, 3, 2)).max() <= 1e-15
    assert len(PG.cases()) == 18 and (17, 70, 1, 4) in PG.cases() and (9, 9, 7, 8) not in PG.cases()
    # one patch that covers the whole interior is section 16's cost, whatever it weighs
    fixed, moving = R.sim_images(9, 9)
    for name, mask in R.sim_masks(9, 9).items():
        got, want = PG.cost(moving, fixed, mask, 3, 1, 1), R.cost(moving, fixed, mask)
        assert np.abs(got - want).max() <= 1e-15, name
    assert PG.cost(moving, np.zeros((9, 9), np.float32), None, 1, 1, 1).tolist() == [1.0] * 6
    with pytest.raises(ValueError):
        PG.shares(fixed, None, 3, 1, 1, np.float64, 'energy')


def test_weights_by_hand():
    """7 x 8, radius 1, stride 2: a 5 x 6 interior with 2 x 2 patches of 3 x 3 pixels; the image is c^2 + 3 r, so
    gx = 16 c and gy = 24 on every interior pixel: every patch has sum (gx - mean)^2 = 3 (256 + 0 + 256) and a flat gy."""
    r, c = np.meshgrid(np.arange(7.0), np.arange(8.0), indexing='ij')
    img = c * c + 3.0 * r
    gx, gy = R.sobel(img)
    assert (gx == 16.0 * c[1:-1, 1:-1]).all() and (gy == 24.0).all()
    assert PT.grid(7, 8, 1, 2) == (2, 2)
    w, tot = PG.weights(img, None, 1, 2, 1)
    assert w.tolist() == [[1536.0, 0.0]] * 4 and tot.tolist() == [6144.0, 0.0]
    assert PG.shares(img, None, 1, 2, 1).tolist() == [[0.25, 0.0]] * 4
    # one mask byte takes the interior pixels (0, 2 .. 4) away.  Patch (0, 0) keeps eight pixels, gx = 16 (3 x), 32 (3 x), 48 (2 x)
    # about their mean 30: 3 x 196 + 3 x 4 + 2 x 324; patch (0, 1) keeps its two lower rows: 2 (256 + 0 + 256)
    mask = np.ones((7, 8), np.uint8)
    mask[0, 4] = 0
    on = R.counted(7, 8, mask)
    assert not on[0, 2:5].any() and on[1:, :].all() and int(on.sum()) == 27
    w, tot = PG.weights(img, mask, 1, 2, 1)
    assert w[:, 0].tolist() == [1248.0, 1024.0, 1536.0, 1536.0] and not w[:, 1].any() and tot.tolist() == [5344.0, 0.0]
    assert PG.shares(img, mask, 1, 2, 1)[:, 0].tolist() == [1248.0 / 5344.0, 1024.0 / 5344.0, 1536.0 / 5344.0, 1536.0 / 5344.0]
    # min_count: patch (0, 1) keeps six pixels and leaves with min_count 7
    w7, tot7 = PG.weights(img, mask, 1, 2, 7)
    assert w7[:, 0].tolist() == [1248.0, 0.0, 1536.0, 1536.0] and tot7[0] == 4320.0
    # weighted cost by hand: X is the weighted mean of the patches' ncc
    mv = img + 0.5 * np.sin(r * c)
    ncc, _, _ = PG.patch_terms(mv[None], img, mask, 1, 2, 1)
    want = 1.0 - 0.5 * float((w[:, 0] * ncc[0, :, 0]).sum() / tot[0])
    assert abs(PG.cost(mv, img, mask, 1, 2, 1) - want) <= 1e-15


def test_texture_quiets_the_background_patches():
    """Section 18's weakness and its remedy: on a fixed image no patch of which is flat, the uniform cost at the true pose
    is a third; weighted by the energy of the fixed gradient it is under a hundredth."""
    fixed, _ = R.sim_images(45, 61)
    tex = PG.textured(fixed)
    uniform, weighted = float(PT.cost(fixed, tex, None, 3, 2)), float(PG.cost(fixed, tex, None, 3, 2))
    assert abs(uniform - 0.3547) <= 1e-4 and abs(weighted - 0.00672) <= 1e-5
    assert weighted < uniform / 20
    _, flags, _ = PT.fixed_patches(tex, None, 3, 2)
    assert (flags == 3).all()                                     # nothing drops out


def test_model_adjoint_against_central_differences():
    doc = GF.load()['finite_differences']
    seen = 0
    for case in (GF.FD_CASE, GF.FD_CASE_DENSE):
        H, W, rho, s, mask_name, mc = case
        mask = R.sim_masks(H, W)[mask_name]
        px = GF.check_pixels(H, W, rho, s, mask)
        cov = np.zeros((H, W), np.int64)
        cov[1:-1, 1:-1] = PG.coverage(H, W, rho, s)
        kinds = {int(cov[r, c]) for r, c in px if 1 <= r < H - 1 and 1 <= c < W - 1}
        assert any(r in (0, H - 1) or c in (0, W - 1) for r, c in px) and len(px) >= 20
        if case == GF.FD_CASE:
            on = np.zeros((H, W), bool)
            on[1:-1, 1:-1] = R.counted(H, W, mask)
            assert 0 in kinds and any(not on[r, c] and 1 <= r < H - 1 and 1 <= c < W - 1 for r, c in px)
        else:
            assert {1, 4, 9} <= kinds
        for weight in PG.WEIGHTS:
            recorded = doc['%s/%s' % (GF.key(*case), weight)]
            assert recorded < 1e-8
            assert GF.fd_error(case, weight) <= 10 * recorded
            seen += len(px)
    assert seen >= 4 * 20


def test_adjoint_is_zero_where_nothing_reaches():
    """Stride 4 with side 3: interior rows and columns 3, 7, ... lie in no patch, and g is 0 there; d_moving still gathers
    from its neighbours.  A view under the empty mask, or a flat one, has an adjoint of exact zeros."""
    fixed, moving = R.sim_images(17, 70)
    cov = PG.coverage(17, 70, 1, 4)
    assert (cov[3] == 0).all() and (cov[:, 3] == 0).all() and cov.max() == 1
    _, d = PG.adjoint(moving, fixed, None, 1, 4, 1)
    assert not d[2].any() and np.abs(d[4]).max() > 0
    _, d = PG.adjoint(moving, fixed, R.sim_masks(17, 70)['empty'], 1, 4, 1)
    assert not d.any()
    # the trailing rows and columns no patch reaches (radius 7, stride 8: interior columns 63 .. 67) get nothing from their own pixels
    _, d = PG.adjoint(moving[4:5], fixed, None, 7, 8)
    assert not d[0, :, 66:].any() and d[0, :, 64].any()


# ---- the committed floors ----------------------------------------------------------------------------------------------
def test_the_committed_floors_are_the_models():
    doc = GF.load()
    assert doc['bar_factor'] == FL.BAR_FACTOR == 8.0 and doc['patch'] == {'radius': 7, 'stride': 4} and doc['band'] == list(PT.BAND)
    sim = doc['similarity']
    assert len(sim) == 18 * 3 * 2 and sorted(sim) == sorted(GF.key(H, W, rho, s, m, mc) for H, W, rho, s in PG.cases()
                                                            for m in ('none', 'ragged', 'empty') for mc in (1, PT.default_min_count(rho)))
    for case in ((9, 9, 3, 2), (17, 70, 1, 4), (17, 70, 7, 8)):                  # recomputed here: a few seconds
        now = GF.floors_of(case)
        for k, e in now.items():
            want = sim[k]
            np.testing.assert_allclose(e['cost'], want['cost'], atol=1e-12)
            np.testing.assert_allclose(e['pwsum'], want['pwsum'], rtol=1e-12)
            assert abs(e['floor'] - want['floor']) <= 0.05 * want['floor'] + 1e-18, (k, e['floor'], want['floor'])
            for w in PG.WEIGHTS:
                np.testing.assert_allclose(e['adjoint'][w]['scale'], want['adjoint'][w]['scale'], rtol=1e-9)
                np.testing.assert_allclose(e['adjoint'][w]['floor'], want['adjoint'][w]['floor'], rtol=0.05, atol=1e-18)
    lo, hi = PT.BAND
    for k, e in sim.items():
        # the input condition, asserted by the floor script for every input: what it recorded lies above the band
        assert all(v is None or v >= hi for pair in e['nearest_ratio_above_band'] for v in pair), k
        assert '/empty/' not in k or e['pwsum'] == [0.0, 0.0]
        if e['pwsum'] == [0.0, 0.0]:                              # no patch counts (the empty mask; the ragged one where it leaves too little)
            assert e['floor'] == 0.0 and e['cost'] == [1.0] * 6
            assert all(f == 0.0 for w in PG.WEIGHTS for f in e['adjoint'][w]['floor'])
        else:
            assert e['cost'][2] == 1.0 and abs(e['cost'][0]) <= 1e-12 and abs(e['cost'][1] - 2) <= 1e-12, k
            for w in PG.WEIGHTS:
                a = e['adjoint'][w]
                assert a['floor'][2] == 0.0 and a['scale'][2] == 0.0, k          # the constant image: exact zeros
                assert a['scale'][0] == a['scale'][1] == a['scale'][3] == a['scale'][4], k
    floors = [e['floor'] for e in sim.values() if e['floor'] > 0]
    assert len(floors) >= 60 and 1e-11 < min(floors) and max(floors) < 1e-5, (min(floors), max(floors))
    # views 4 and 5 (rendered): float32 rounding of the per-pixel arithmetic; view 3 (3 fixed + 2 rounded to float32, near the
    # extremum) up to 2 % of view 4's scale under the uniform weighting, where weak patches weigh as much as strong ones
    adj = [f for e in sim.values() for w in PG.WEIGHTS for f in e['adjoint'][w]['floor'][4:] if f > 0]
    assert 1e-8 < min(adj) and max(adj) < 1e-3, (min(adj), max(adj))
    assert max(f for e in sim.values() for w in PG.WEIGHTS for f in e['adjoint'][w]['floor']) < 0.05
    # the GPU bars are taken from these
    assert GF.cost_bar(45, 61, 3, 2, 'none', 1) == 8.0 * sim[GF.key(45, 61, 3, 2, 'none', 1)]['floor']
    bars, scale = GF.adjoint_bars(45, 61, 3, 2, 'none', 1, 'variance')
    assert bars.shape == (6,) and bars[2] == 0.0 and (bars[[0, 1, 3, 4, 5]] > 0).all() and scale[0] == scale[4]


def test_the_registrations_by_the_models_sit_inside_the_gpu_bars():
    r = GF.load()['registration']
    assert sorted(r) == ['E', 'F', 'G', 'G_uniform']
    for k in ('E', 'G', 'G_uniform'):
        assert (r[k]['generations'], r[k]['popsize'], r[k]['seed'], r[k]['sigma0']) == (80, 16, 0, 2.0) and min(r[k]['start_px']) >= 10
    assert r['E']['patch_weight'] == r['G']['patch_weight'] == r['F']['patch_weight'] == 'variance' and r['G_uniform']['patch_weight'] == 'uniform'
    # E and F: the project's quarter pixel is asked of the GPU provided the models end within half of it
    assert max(r['E']['final_px']) <= FL.PIXEL_BAR / 2
    assert max(r['F']['final_px']) <= FL.PIXEL_BAR / 2 and r['F']['refine'] == 30 and r['F']['refine_cost'][-1] < r['F']['refine_cost'][0]
    assert np.allclose(r['F']['theta0'], GF.REFINE_START * np.array(R.THETA_START) / 2 ** r['F']['halvings'])
    # G: on the textured image the weighted cost is far lower at the truth, and ends no further away than the uniform one
    assert r['G']['cost_at_truth'] < r['G_uniform']['cost_at_truth'] / 10
    assert max(r['G']['final_px']) <= max(r['G_uniform']['final_px'])


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_struct_mirrors_match_the_library():
    L = nat.lib()
    for cls, size in ((nat.SimPatchWeightsArgs, 40), (nat.SimPatchEvalArgs, 136)):
        assert L.dfl_sizeof(nat._SIZEOF_ORDER.index(cls)) == C.sizeof(cls) == size
    k = nat._SIZEOF_ORDER.index(nat.SimGradnccBwdArgs)
    assert nat._SIZEOF_ORDER[k + 1:k + 4] == [nat.SimPatchWeightsArgs, nat.SimPatchEvalArgs, nat.DrrPoseGradArgs]
    assert [f for f, _ in nat.SimPatchWeightsArgs._fields_] == ['ptotals', 'pflags', 'pweights', 'pwsum', 'P']
    assert [f for f, _ in nat.SimPatchEvalArgs._fields_] == ['moving', 'fx', 'fy', 'counted', 'ptotals', 'pflags', 'pcount', 'pweights', 'pwsum',
                                                           'fixed_of', 'scratch', 'cost', 'd_moving', 'scratch_doubles', 'V', 'H', 'W', 'rho',
                                                           'stride', 'F']
    for fn in ('dfl_sim_patch_weights', 'dfl_sim_patch_eval', 'dfl_sim_patch_eval_scratch_doubles'):
        assert fn in nat.EXPORTS and hasattr(L, fn)
    header = open(os.path.join(ROOT, 'include', 'dfl_hip.h')).read()
    mine = [n for n in nat.EXPORTS if n.startswith('dfl_sim_patch_')]
    protos = ['int dfl_sim_patch_bank_gradncc(const dfl_sim_patch_bank_gradncc_args* a, dfl_stream_t stream);',
              'int dfl_sim_patch_weights(const dfl_sim_patch_weights_args* a, dfl_stream_t stream);',
              'int dfl_sim_patch_eval(const dfl_sim_patch_eval_args* a, dfl_stream_t stream);',
              'int dfl_sim_patch_eval_scratch_doubles(int32_t V, int32_t H, int32_t W, int32_t rho, int32_t stride, int32_t bwd);']
    at = [header.index(p) for p in protos]
    assert at == sorted(at) and mine[-4:] == [p.split('(')[0].split()[-1] for p in protos]      # EXPORTS is in header order
    assert L.dfl_sim_patch_eval_scratch_doubles.restype is C.c_int
    for H, W, rho, s in PG.cases():
        PR, PC = PT.grid(H, W, rho, s)
        assert L.dfl_sim_patch_eval_scratch_doubles(3, H, W, rho, s, 0) == 3 * PR * 2 == L.dfl_sim_patch_scratch_doubles(3, H, W, rho, s)
        assert L.dfl_sim_patch_eval_scratch_doubles(3, H, W, rho, s, 1) == 3 * PR * 2 + 4 * 3 * PR * PC
    assert L.dfl_sim_patch_eval_scratch_doubles(32, 180, 180, 7, 4, 1) == 32 * 41 * 2 + 4 * 32 * 41 * 41
    for bad, word in (((2, 61, 1, 1), b'3 x 3'), ((45, 61, 0, 1), b'radius'), ((45, 61, 1, 0), b'stride'), ((9, 9, 4, 1), b'does not fit'),
                      ((45, 1539, 3, 2), b'DFL_SIM_PATCH_MAX_W'), ((65536, 65536, 1, 1), b'too large')):
        for bwd in (0, 1):
            assert L.dfl_sim_patch_eval_scratch_doubles(1, *bad, bwd) == -1
            assert word in L.dfl_last_error() and b'dfl_sim_patch_eval_scratch_doubles' in L.dfl_last_error(), bad
    for V in (0, 65536, -1):
        assert L.dfl_sim_patch_eval_scratch_doubles(V, 45, 61, 3, 2, 1) == -1 and b'65535' in L.dfl_last_error()
    # more than 2^31 - 1 doubles: 1536 x 1536 with every pixel a patch has 2.3 million of them
    assert L.dfl_sim_patch_eval_scratch_doubles(1000, 1538, 1538, 1, 1, 0) == 1000 * 1534 * 2
    assert L.dfl_sim_patch_eval_scratch_doubles(1000, 1538, 1538, 1, 1, 1) == -1 and b'2^31' in L.dfl_last_error()


def test_c_abi_refuses_bad_arguments():
    """Every refusal comes back as -1 with a message, before anything is launched."""
    L = nat.lib()
    P = 4096                                                  # never dereferenced: the checks come first

    def wts(**k):
        return nat.SimPatchWeightsArgs(**dict(dict(ptotals=P, pflags=P, pweights=P, pwsum=P, P=19 * 27), **k))

    for kw, word in tuple((dict(**{f: None}), b'required') for f in ('ptotals', 'pflags', 'pweights', 'pwsum')) + \
            ((dict(P=0), b'patches'), (dict(P=-4), b'patches'), (dict(P=1 << 31), b'patches')):
        a = wts(**kw)
        assert L.dfl_sim_patch_weights(C.addressof(a), None) == -1, kw
        assert word in L.dfl_last_error() and b'dfl_sim_patch_weights' in L.dfl_last_error(), (kw, L.dfl_last_error())
    assert L.dfl_sim_patch_weights(None, None) == -1 and b'null' in L.dfl_last_error()

    fwd, bwd = 6 * 19 * 2, 6 * 19 * 2 + 4 * 6 * 19 * 27

    def ev(**k):
        return nat.SimPatchEvalArgs(**dict(dict(moving=P, fx=P, fy=P, counted=P, ptotals=P, pflags=P, pcount=P, pweights=P, pwsum=P, fixed_of=P,
                                                scratch=P, cost=P, d_moving=P, scratch_doubles=bwd, V=6, H=45, W=61, rho=3, stride=2, F=3), **k))

    sizes = ((dict(H=2), b'3 x 3'), (dict(W=2), b'3 x 3'), (dict(H=65536, W=65536), b'too large'), (dict(rho=0), b'radius'),
             (dict(stride=0), b'stride'), (dict(rho=22), b'does not fit'), (dict(H=8), b'does not fit'),
             (dict(W=nat.SIM_PATCH_MAX_W + 1), b'DFL_SIM_PATCH_MAX_W'))
    required = ('moving', 'fx', 'fy', 'counted', 'ptotals', 'pflags', 'pcount', 'scratch', 'cost')
    cases = tuple((dict(**{f: None}), b'required') for f in required) + sizes + \
        ((dict(pweights=None), b'come together'), (dict(pwsum=None), b'come together'),
         (dict(V=0), b'65535'), (dict(V=65536, scratch_doubles=1 << 40), b'65535'),
         (dict(F=0), b'bank'), (dict(F=65536), b'bank'), (dict(F=800000), b'bank'), (dict(H=1200, W=1200, F=1500, scratch_doubles=1 << 40), b'bank'),
         (dict(scratch_doubles=bwd - 1), b'scratch'), (dict(scratch_doubles=fwd), b'dfl_sim_patch_eval_scratch_doubles'),
         (dict(d_moving=None, scratch_doubles=fwd - 1), b'scratch'), (dict(V=7), b'scratch'), (dict(stride=1), b'scratch'),
         (dict(scratch_doubles=0), b'scratch'),
         (dict(H=16 * 65535 + 1, W=9, rho=1, stride=1 << 20, fixed_of=None, scratch_doubles=1 << 40), b'too tall'))
    for kw, word in cases:
        a = ev(**kw)
        assert L.dfl_sim_patch_eval(C.addressof(a), None) == -1, kw
        assert word in L.dfl_last_error() and b'dfl_sim_patch_eval' in L.dfl_last_error(), (kw, L.dfl_last_error())
    assert L.dfl_sim_patch_eval(None, None) == -1 and b'null' in L.dfl_last_error()
    # the existing entry points refuse as before, with their own names
    a = nat.SimPatchGradnccArgs(moving=P, fx=P, fy=P, counted=P, ptotals=P, pflags=P, pcount=P, scratch=P, cost=P, scratch_doubles=fwd - 1,
                                V=6, H=45, W=61, rho=3, stride=2)
    assert L.dfl_sim_patch_gradncc(C.addressof(a), None) == -1 and b'(dfl_sim_patch_scratch_doubles)' in L.dfl_last_error()


# ---- register ----------------------------------------------------------------------------------------------------------
def _geom(S):
    poses = dict(zip(drr.POSES, S['poses']))
    return drr.Geometry(S['K'], S['E'], poses, S['I2P'], np.eye(3), drr.default_objects(S['E'], poses, S['I2P']), drr.Grid(S['Q'], S['rows'], S['cols']))


def test_register_checks_patch_weight_before_it_touches_the_gpu():
    geom = _geom(D.scene('tilted'))
    for fn, first in ((reg.register, (None, geom, None)), (reg.register_many, (None, [geom], None))):
        for kw, word in ((dict(similarity='patch', patch_weight='energy'), 'patch weight'), (dict(patch_weight=None), 'patch weight'),
                         (dict(patch_weight='variance'), 'global'), (dict(similarity='global', patch_weight='variance', refine=3), 'global'),
                         (dict(similarity='patch', patch_weight='variance', patch_radius=0), 'radius')):
            with pytest.raises(nat.DflError, match=word):
                fn(*first, **kw)
        # the pinned refusal stays: the uniform patch cost with refine, by default and when named
        for kw in (dict(similarity='patch', refine=3), dict(similarity='patch', refine=3, patch_weight='uniform')):
            with pytest.raises(nat.DflError, match='patch') as e:
                fn(*first, **kw)
            assert 'refine' in str(e.value)
        # with the weighted cost the same call gets past the options, as far as the first check on device tensors
        for kw in (dict(similarity='patch', patch_weight='variance', refine=3), dict(similarity='patch', patch_weight='variance'),
                   dict(patch_weight='uniform')):
            with pytest.raises(nat.DflError, match='Volume|GPU'):
                fn(*first, **kw)
    assert reg._cost_options(0, 1e-4, 'patch', 7, 4, None, 0.0) == ((7, 4, 113, 'uniform'), 0.0)
    assert reg._cost_options(5, 1e-4, 'patch', 3, 2, 24, 0.5, 'variance') == ((3, 2, 24, 'variance'), 0.5)
    assert reg._cost_options(5, 1e-4, 'global', 7, 4, None, 0.0, 'uniform') == (None, 0.0)
    import torch
    for cls, img in ((reg.PatchSimilarity, torch.zeros(45, 61)), (reg.PatchSimilarityBank, torch.zeros(2, 45, 61))):
        with pytest.raises(nat.DflError, match='patch weight'):
            cls(img, weight='energy')
        with pytest.raises(nat.DflError, match='GPU'):
            cls(img, weight='variance')
        assert cls.entry in ('dfl_sim_patch_gradncc', 'dfl_sim_patch_bank_gradncc')


# ---- the examples ------------------------------------------------------------------------------------------------------
def test_command_lines(capsys):
    import register_2d3d as one
    import register_specimen as many
    assert one.parse_patch_weight(['a', '--gt-lands']) == (['a', '--gt-lands'], 'uniform')
    assert one.parse_patch_weight(['a', '--patch-weight', 'variance', '--refine', '3']) == (['a', '--refine', '3'], 'variance')
    assert one.parse_patch_weight(['--patch-weight', 'uniform', 'a']) == (['a'], 'uniform')
    for bad in (['a', '--patch-weight'], ['a', '--patch-weight', 'energy'], ['--patch-weight', '--gt-lands']):
        assert one.parse_patch_weight(bad) is None
    assert many.parse_patch_weight is one.parse_patch_weight
    base = ['f.h5', '17-1882', '0', '--gt-lands']
    for cli, line in ((one, base), (many, ['f.h5', '17-1882', '--gt-lands'])):
        for bad in (['--patch-weight'], ['--patch-weight', 'energy'], ['--patch-weight', 'variance'],            # the last: not with global
                    ['--similarity', 'patch', '--refine', '2'], ['--similarity', 'patch', '--patch-weight', 'uniform', '--refine', '2']):
            assert cli.main(line + bad) == 1, bad
            out = capsys.readouterr().out
            assert out.startswith('Usage: ') and '[--patch-weight uniform|variance]' in out and not out.rstrip().endswith('variance]')
        assert '--patch-weight variance' in cli.__doc__
    # understood: the weighted patch cost with --refine gets past the command line
    (path, spec), o = many.parse(['f.h5', 's', '--gt-lands', '--similarity', 'patch', '--refine', '2'], 'variance')
    assert o['--refine'] == 2 and '--patch-weight' not in o
    assert many.parse(['f.h5', 's', '--gt-lands', '--refine', '2'], 'variance') is None
    assert many.parse(['f.h5', 's', '--gt-lands', '--similarity', 'patch', '--refine', '2']) is None
