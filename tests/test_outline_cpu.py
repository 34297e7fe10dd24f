"""The outline cost without a GPU: the numpy model (tests/outline_ref.py) on cases worked out by hand, the C ABI of
csrc/sim_outline.hip (the binding derived from the header and its refusals, which launch nothing), the refusals of
register(similarity='outline') and register_many before anything touches a device, the command line of
examples/register_outline.py, and tests/golden/floors/outline.json against a recomputation.
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
import outline_floor as FL  # noqa: E402
import outline_ref as O  # noqa: E402
import reg_ref as R  # noqa: E402
import surface_ref as SR  # noqa: E402
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, drr, register as reg  # noqa: E402


# ---- the model ---------------------------------------------------------------------------------------------------------
def test_the_model_on_shifted_rectangles():
    """A 15 x 24 rectangle and its copy shifted by (3, 4): 74 boundary pixels each way, no distance above 5.
    Uncapped the cost is ASSD / cap.  With cap 2 every distance of 2 or more counts 2: of the moving rectangle's top row
    (24 pixels) one pixel lies on the fixed boundary and its two neighbours 1 away, of its left column (13) likewise, the
    bottom row (24) and the right column (13) are 3 and 4 away: a = 0 + 2 + 21 * 2 + 0 + 2 + 10 * 2 + 24 * 2 + 13 * 2 = 140,
    and b = 140 by the point symmetry of the pair; c = (140 / 74 + 140 / 74) / 4 = 35 / 37."""
    est, gt = SR.shifted_rectangles()
    for cap in (5.0, 7.5, 32.0):
        counts, sums, c = O.cost(est, gt, [(1,)], cap)
        assert counts.tolist() == [[74, 74]]
        assert c == pytest.approx(3.1027798811266067 / cap, rel=1e-14)
        assert (sums[0, 0] / 74 + sums[0, 1] / 74) / 2 == pytest.approx(3.1027798811266067, rel=1e-14)
    counts, sums, c = O.cost(est, gt, [(1,)], 2.0)
    assert counts.tolist() == [[74, 74]] and sums.tolist() == [[140.0, 140.0]]
    assert c == (140.0 / 74 + 140.0 / 74) / 4.0 and c == pytest.approx(35.0 / 37.0, rel=1e-15)
    # a cap equal to a distance: the farthest pair is exactly 5 apart, so cap 5 truncates nothing
    assert O.cost(est, gt, [(1,)], 5.0)[1].tolist() == O.cost(est, gt, [(1,)], 50.0)[1].tolist()
    # the same map on both sides costs exactly 0, whatever the cap
    assert O.cost(gt, gt, [(1,)], 3.0)[2] == 0.0 and O.cost(gt, gt, [(1,)], 3.0)[1].tolist() == [[0.0, 0.0]]


def test_the_branches_of_the_model():
    est, gt = SR.shifted_rectangles()
    two = est.copy()
    two[0:3, 0:3] = 2                                         # label 2 in the moving map alone
    counts, sums, c = O.cost(two, gt, [(1,), (2,), (3,)], 8.0)
    assert counts.tolist() == [[74, 74], [8, 0], [0, 0]]      # scored; one-sided; not scored
    assert sums[1].tolist() == [0.0, 0.0] and sums[2].tolist() == [0.0, 0.0]
    both = 3.1027798811266067 / 8.0
    assert c == pytest.approx((both + 1.0) / 2.0, rel=1e-14)
    # the fixed map alone holds the set: also 1; a union is one set
    assert O.cost(gt, two, [(2,)], 8.0)[2] == 1.0 and O.cost(gt, two, [(2,)], 8.0)[0].tolist() == [[0, 8]]
    assert O.cost(two, gt, [(1, 2)], 8.0)[0][0, 1] == 74 and O.cost(two, gt, [(1, 2)], 8.0)[0][0, 0] == 74 + 8
    # no set scored: 1.0; values of 32 and more are in no set
    assert O.cost(est, gt, [(3,), (4,)], 8.0)[2] == 1.0
    big = np.where(est == 1, 40, 0).astype(np.uint8)
    assert O.cost(big, big, [(8,)], 8.0)[2] == 1.0 and O.labels_of(0x1e) == (1, 2, 3, 4)
    # from_d2 reads boundary sites off the distance maps alone
    d2m, d2f = O.d2_stack(two, [(1,), (2,)]), O.d2_stack(gt, [(1,), (2,)])
    assert (d2f[1] == O.NONE).all() and ((d2m[0] == 0) == SR.sites(two, (1,), True)).all()
    assert O.from_d2(d2m, d2f, 8.0)[2] == pytest.approx((both + 1.0) / 2.0, rel=1e-14)
    stack = O.cost_stack(np.stack([two, gt]), np.stack([gt, two]), [(1,), (2,)], 8.0, [0, 1])
    assert stack[2][0] == O.cost(two, gt, [(1,), (2,)], 8.0)[2] and stack[2][1] == O.cost(gt, two, [(1,), (2,)], 8.0)[2]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_the_binding_comes_from_the_header():
    assert 'dfl_sim_outline' in nat.EXPORTS and 'dfl_sim_outline_scratch_doubles' in nat.EXPORTS
    assert [(n, t) for n, t in nat.SimOutlineArgs._fields_] == \
        [(n, C.c_void_p) for n in ('d2_moving', 'd2_fixed', 'fixed_of', 'counts', 'sums', 'cost', 'scratch')] + \
        [('scratch_doubles', C.c_int64), ('cap', C.c_double)] + [(n, C.c_int32) for n in ('V', 'F', 'S', 'H', 'W', 'reserved')]
    assert C.sizeof(nat.SimOutlineArgs) == 7 * 8 + 8 + 8 + 6 * 4
    L = nat.lib()
    assert L.dfl_sim_outline.argtypes == [C.c_void_p, C.c_void_p] and L.dfl_sim_outline_scratch_doubles.restype == C.c_int
    assert nat.SIM_OUTLINE_CHUNK == 1024
    assert L.dfl_sim_outline_scratch_doubles(16, 6, 180, 180) == 4 * 16 * 6 * 32
    assert L.dfl_sim_outline_scratch_doubles(3, 1, 33, 130) == 4 * 3 * 1 * 5 and L.dfl_sim_outline_scratch_doubles(1, 31, 1, 9) == 4 * 31
    for bad in ((0, 1, 5, 5), (65536, 1, 5, 5), (1, 0, 5, 5), (1, 32, 5, 5), (1, 1, 0, 5), (1, 1, 5, 0), (1, 1, 46342, 2), (65535, 31, 4000, 4000)):
        assert L.dfl_sim_outline_scratch_doubles(*bad) < 0 and b'dfl_sim_outline_scratch_doubles' in L.dfl_last_error(), bad


def test_c_abi_refuses_bad_arguments():
    """Every refusal comes before the launch and before a pointer is followed: the addresses here are not memory."""
    L = nat.lib()
    fake = 1 << 20

    def args(**k):
        return nat.SimOutlineArgs(**dict(dict(d2_moving=fake, d2_fixed=fake, fixed_of=None, counts=fake, sums=fake, cost=fake, scratch=fake,
                                              scratch_doubles=4 * 2 * 3 * 1, cap=16.0, V=2, F=1, S=3, H=5, W=7, reserved=0), **k))

    for kw, word in ((dict(d2_moving=None), b'required'), (dict(d2_fixed=None), b'required'), (dict(counts=None), b'required'),
                     (dict(sums=None), b'required'), (dict(cost=None), b'required'), (dict(scratch=None), b'required'),
                     (dict(V=0), b'65535'), (dict(V=65536), b'65535'), (dict(F=0), b'fixed maps'), (dict(S=0), b'label sets'),
                     (dict(S=nat.LABEL_MAX_CLASSES + 1), b'label sets'), (dict(H=0), b'bad sizes'), (dict(W=0), b'bad sizes'),
                     (dict(H=46342, W=2, scratch_doubles=1 << 40), b'does not fit'), (dict(cap=0.0), b'cap'), (dict(cap=-1.0), b'cap'),
                     (dict(cap=float('inf')), b'cap'), (dict(cap=float('nan')), b'cap'), (dict(scratch_doubles=23), b'scratch')):
        a = args(**kw)
        assert L.dfl_sim_outline(C.addressof(a), None) == -1 and word in L.dfl_last_error(), (kw, L.dfl_last_error())
    assert L.dfl_sim_outline(None, None) == -1 and b'null args' in L.dfl_last_error()


# ---- register() and register_many() ------------------------------------------------------------------------------------
def _geom(S):
    G, (H, W) = drr.training_grid(S['rows'], S['cols'], 0, 1, False)
    poses = dict(zip(drr.POSES, S['poses']))
    return drr.Geometry(S['K'], S['E'], poses, S['I2P'], G, drr.default_objects(S['E'], poses, S['I2P']), drr.Grid(-np.linalg.inv(S['K']) @ G, H, W))


def test_register_refuses_before_it_touches_the_gpu():
    S = D.scene('tilted')
    g = _geom(S)
    H, W = g.size
    seg = torch.zeros((H, W), dtype=torch.uint8)              # on the CPU
    for kw, word in ((dict(segmentation=None), 'segmentation'), (dict(segmentation=seg[:-1]), 'segmentation'),
                     (dict(segmentation=seg[None]), 'segmentation'), (dict(segmentation=seg.float()), 'segmentation'),
                     (dict(segmentation=np.zeros((H, W), np.uint8)), 'segmentation'),
                     (dict(levels=[(1, 2)]), 'levels'), (dict(mask=torch.ones((H, W), dtype=torch.uint8)), 'mask'),
                     (dict(refine=2), 'refine'), (dict(refine=2), 'outline'), (dict(patch_weight='variance'), 'patch_weight'),
                     (dict(outline_cap=0.0), 'outline_cap'), (dict(outline_cap=float('nan')), 'outline_cap'),
                     (dict(popsize=3), 'Volume'), (dict(), 'Volume')):     # with good arguments the first thing missed is the device volume
        with pytest.raises(nat.DflError, match=word):
            reg.register(None, g, None, **dict(dict(similarity='outline', segmentation=seg), **kw))
    stand_in = object.__new__(drr.Volume)                     # passes for a Volume: the tensor check is reached
    with pytest.raises(nat.DflError, match='segmentation on the GPU'):
        reg.register(stand_in, g, None, similarity='outline', segmentation=seg)
    # an unknown similarity still says so, and the options of the outline belong to it alone
    with pytest.raises(nat.DflError, match='similarity'):
        reg.register(None, g, None, similarity='chamfer')
    with pytest.raises(nat.DflError, match="'outline'"):
        reg.register(None, g, None, similarity='chamfer')
    for kw in (dict(segmentation=seg), dict(outline_sets=[[1]]), dict(similarity='patch', segmentation=seg)):
        with pytest.raises(nat.DflError, match="belong to similarity='outline'"):
            reg.register(None, g, None, **kw)
    with pytest.raises(nat.DflError, match='register_many.*outline'):
        reg.register_many(None, [g, g], torch.zeros((2, H, W)), similarity='outline')
    with pytest.raises(nat.DflError, match='similarity'):
        reg.register_many(None, [g, g], torch.zeros((2, H, W)), similarity='chamfer')
    with pytest.raises(nat.DflError, match='GPU'):
        reg.OutlineSimilarity(seg, [[1]])
    with pytest.raises(nat.DflError, match='GPU'):
        reg.OutlineSimilarity(seg[None], [[1]])
    assert 'OutlineSimilarity' in reg.__all__
    # the default sets: one per label of the moving objects' masks
    assert reg._outline_sets(g, (0, 1, 2), None) == [[1], [2], [3], [4], [5], [6]] and reg._outline_sets(g, (1,), None) == [[5]]
    assert reg._outline_sets(g, (0,), [[1, 2, 3, 4]]) == [[1, 2, 3, 4]]


# ---- the example -------------------------------------------------------------------------------------------------------
def test_command_line(capsys):
    import register_outline as cli
    base = ['f.h5', '17-1882', '3', 'out.h5', 'nn-segs']
    pos, o = cli.parse(base + ['--gt-lands'])
    assert pos == ('f.h5', '17-1882', '3', 'out.h5', 'nn-segs')
    assert o == {'--start-npz': None, '--lands-csv': None, '--offset': None, '--gt-lands': True, '--clean': False, '--outline-generations': 40,
                 '--outline-sigma': 4.0, '--outline-cap': 32.0, '--generations': 40, '--sigma': 1.0, '--out': None, '--crop': 50,
                 '--ds-factor': 8, '--popsize': 16, '--seed': 0, '--step': 1.0}
    _, o = cli.parse(base + ['--start-npz', 'a_reg.npz', '--clean', '--outline-cap', '16', '--outline-generations', '60', '--outline-sigma', '2.5',
                             '--generations', '7', '--sigma', '0.5', '--seed', '4', '--out', 'run'])
    assert (o['--start-npz'], o['--clean'], o['--outline-cap'], o['--outline-generations'], o['--outline-sigma'], o['--generations'], o['--sigma'],
            o['--seed'], o['--out']) == ('a_reg.npz', True, 16.0, 60, 2.5, 7, 0.5, 4, 'run')
    assert cli.parse(base + ['--offset', '1,2,3,4,5,6'])[1]['--offset'] == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    assert cli.parse(base + ['--lands-csv', 'l.csv'])[1]['--lands-csv'] == 'l.csv'
    for bad in ([], ['--gt-lands', '--offset', '0,0,0,0,0,0'], ['--gt-lands', '--start-npz', 'a.npz'], ['--lands-csv', 'l.csv', '--start-npz', 'a.npz'],
                ['--offset', '1,2,3'], ['--start-npz'], ['--gt-lands', '--outline-cap', '0'], ['--gt-lands', '--outline-cap', 'x'],
                ['--gt-lands', '--outline-sigma', '-1'], ['--gt-lands', '--outline-generations', '0'], ['--gt-lands', '--generations', '0'],
                ['--gt-lands', '--sigma', '0'], ['--gt-lands', '--popsize', '3'], ['--gt-lands', '--what'], ['--gt-lands', '--similarity', 'patch'],
                ['--gt-lands', 'extra'], ['--gt-lands', '--outline-cap', 'nan']):
        assert cli.parse(base + bad) is None, bad
    assert cli.parse(base[:4] + ['--gt-lands']) is None and cli.parse(['f.h5', 's', 'x', 'out.h5', 'nn-segs', '--gt-lands']) is None
    for argv in ([], base, base + ['--gt-lands', '--offset', '0,0,0,0,0,0']):
        assert cli.main(argv) == 1
        out = capsys.readouterr().out
        assert '(--start-npz FILE | --lands-csv FILE | --gt-lands | --offset rx,ry,rz,tx,ty,tz)' in out
        assert out.rstrip().endswith('[--out PREFIX] [--crop 50] [--ds-factor 8] [--popsize 16] [--seed 0] [--step 1.0]')
    doc = cli.__doc__
    assert '--start-npz' in doc and 'outline_poses' in doc and 'outline_cost' in doc and '--clean' in doc


# ---- the committed floors ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['near', 'far'])
def test_the_floor_file_matches_a_recomputation(case):
    doc = FL.load()
    rec, st = doc['registration'][case], FL.SETTINGS[case]
    assert doc['bar_factor'] == FL.BAR_FACTOR == 2.0 and doc['model_bar_pixels'] == FL.MODEL_BAR == 1.0
    assert rec['theta0'] == list(st['theta0']) and rec['sigma0'] == st['sigma0'] and rec['generations'] == st['generations']
    assert rec['cap'] == FL.CAP == 16.0 and rec['popsize'] == 16 and rec['seed'] == 0 and rec['label_sets'] == [list(s) for s in O.DEFAULT_SETS]
    start, truth = FL.start_and_truth_cost(D.scene('tilted'), st['theta0'])
    assert truth == 0.0 and rec['truth_cost'] == 0.0
    assert abs(start - rec['start_cost']) <= 1e-12, (start, rec['start_cost'])
    assert len(rec['final_px']) == 6 and max(rec['final_px']) <= FL.MODEL_BAR and FL.bar(case) == 2.0 * max(rec['final_px'])
    assert rec['final_cost'] < 0.1 * rec['start_cost']
    S = D.scene('tilted')
    np.testing.assert_allclose(rec['start_px'], FL.pelvis_px(S, st['theta0']), rtol=0, atol=1e-9)
    np.testing.assert_allclose(rec['final_px'], FL.pelvis_px(S, rec['theta']), rtol=0, atol=1e-9)


def test_the_floor_file_holds_every_case():
    reg_doc = FL.load()['registration']
    assert sorted(reg_doc) == ['far', 'far_intensity', 'near', 'two_stage']
    assert FL.SETTINGS['far']['theta0'] == tuple(2.5 * t for t in R.THETA_START) and min(reg_doc['far']['start_px']) > 20
    assert reg_doc['far_intensity']['asserted'] is False and reg_doc['far_intensity']['theta0'] == reg_doc['far']['theta0']
    two = reg_doc['two_stage']
    assert two['theta0'] == reg_doc['far']['theta'] and (two['sigma0'], two['generations'], two['seed']) == (1.0, 40, 1)
    assert two['start_px'] == reg_doc['far']['final_px'] and max(two['final_px']) <= FL.bar('far')
