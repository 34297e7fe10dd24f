"""register_many on the CPU: the step-wise optimisers against cma_es and bfgs byte for byte, the C
ABI of the three bank entry points (struct mirrors and refusals with fake pointers: nothing is launched), the refusals of
register_many that come before anything touches a device, the host check of fixed_of and the command line of
examples/register_specimen.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'examples'))

import drr_ref as D  # noqa: E402
import reg_ref as R  # noqa: E402
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, drr, register as reg  # noqa: E402


# ---- the step-wise optimisers ------------------------------------------------------------------------------------------
def test_cma_steps_driven_by_hand_is_cma_es():
    scale = np.array([1.0, 3.0, 0.5, 10.0, 2.0, 0.1])
    target = np.array([0.3, -1.0, 2.0, 0.0, 1.5, -0.7])

    def cost(xs):
        return (((xs - target[None]) * scale[None]) ** 2).sum(1)

    want = reg.cma_es(cost, np.zeros(6), 1.5, 8, 30, 3)
    steps, asked = reg.cma_steps(np.zeros(6), 1.5, 8, 30, 3), 0
    xs = next(steps)
    while True:
        assert xs.shape == (8, 6)
        asked += 1
        try:
            xs = steps.send(cost(xs))
        except StopIteration as stop:
            got = stop.value
            break
    assert asked == 30 and got.evaluations == want.evaluations == 240
    assert got.mean.tobytes() == want.mean.tobytes() and got.trace.tobytes() == want.trace.tobytes() and got.trace.shape == (30,)
    assert got.sigma == want.sigma and got.best_f == want.best_f and got.best_x.tobytes() == want.best_x.tobytes()
    assert want.trace[-1] < want.trace[0]                         # and the search went downhill
    # no generation: the result without a single request
    with pytest.raises(StopIteration) as stop:
        next(reg.cma_steps(np.ones(6), 1.0, 8, 0, 3))
    assert np.array_equal(stop.value.value.mean, np.ones(6)) and stop.value.value.evaluations == 0
    with pytest.raises(nat.DflError, match='popsize'):
        next(reg.cma_steps(np.ones(6), 1.0, 3, 5, 0))


def _functions():
    A = np.diag([1.0, 10.0, 100.0, 1000.0])

    def quadratic(x):
        return 0.5 * float(x @ A @ x), A @ x

    def rosenbrock(x):
        f = float((100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1.0 - x[:-1]) ** 2).sum())
        g = np.zeros_like(x)
        g[:-1] = -400.0 * x[:-1] * (x[1:] - x[:-1] ** 2) - 2.0 * (1.0 - x[:-1])
        g[1:] += 200.0 * (x[1:] - x[:-1] ** 2)
        return f, g

    def walled(x):                                                # not finite beyond a wall: trials are rejected there
        if x[0] < -0.5:
            return np.inf, np.full_like(x, np.nan)
        return float(np.cosh(x).sum()), np.sinh(x)

    return (quadratic, np.full(4, 3.0), 40), (rosenbrock, np.array([-1.2, 1.0, 0.5]), 60), (walled, np.array([2.0, -0.4, 1.0, 0.3, 2.5]), 25)


def test_three_bfgs_in_lockstep_are_three_bfgs():
    cases = _functions()
    want = [reg.bfgs(fun, x0, its, 1e-10) for fun, x0, its in cases]
    assert len({w.evaluations for w in want}) == 3               # they need different numbers of trials
    assert any(w.evaluations > w.iterations + 1 for w in want)    # and some trial was rejected
    rounds = []

    def evaluate(idx, points):
        rounds.append(list(idx))
        return [cases[i][0](x) for i, x in zip(idx, points)]

    got = reg.lockstep([reg.bfgs_steps(x0, its, 1e-10) for _, x0, its in cases], evaluate)
    for g, w in zip(got, want):
        assert g.x.tobytes() == w.x.tobytes() and g.trace.tobytes() == w.trace.tobytes() and g.evaluations == w.evaluations
        assert g.f == w.f and g.iterations == w.iterations
    # one round per evaluation of the longest problem; a finished problem drops out and never comes back
    assert len(rounds) == max(w.evaluations for w in want) and rounds[0] == [0, 1, 2]
    for i, w in enumerate(want):
        assert [i in r for r in rounds] == [True] * w.evaluations + [False] * (len(rounds) - w.evaluations)
    with pytest.raises(nat.DflError, match='replies'):
        reg.lockstep([reg.bfgs_steps(np.ones(2), 3)], lambda idx, pts: [])
    with pytest.raises(nat.DflError, match='not finite'):
        reg.lockstep([reg.bfgs_steps(np.ones(2), 3)], lambda idx, pts: [(np.nan, np.ones(2))])
    assert reg.lockstep([], lambda idx, pts: []) == []


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
BANK = ('SimBankGradnccArgs', 'SimBankGradnccBwdArgs', 'SimPatchBankGradnccArgs')


def test_struct_mirrors_match_the_library():
    L = nat.lib()
    for name, size in zip(BANK, (96, 104, 112)):
        cls = getattr(nat, name)
        assert L.dfl_sizeof(nat._SIZEOF_ORDER.index(cls)) == C.sizeof(cls) == size, name
    k = nat._SIZEOF_ORDER.index(nat.DrrObject)
    assert [c.__name__ for c in nat._SIZEOF_ORDER[k - 3:k]] == list(BANK) and nat._SIZEOF_ORDER[k - 4] is nat.DrrPoseGradArgs
    assert nat._SIZEOF_ORDER[-3:] == [nat.DrrObject, nat.DrrArgs, nat.OptimPackArgs]
    assert L.dfl_sizeof(len(nat._SIZEOF_ORDER)) == -1
    for fn in ('dfl_sim_bank_gradncc', 'dfl_sim_bank_gradncc_bwd', 'dfl_sim_patch_bank_gradncc'):
        assert fn in nat.EXPORTS and hasattr(L, fn)
    for cls in (nat.SimBankGradnccArgs, nat.SimBankGradnccBwdArgs, nat.SimPatchBankGradnccArgs):
        names = [f for f, _ in cls._fields_]
        assert 'fixed_of' in names and names[-1] == 'F' and dict(cls._fields_)['F'] is C.c_int32


def test_c_abi_refuses_bad_arguments():
    """Every refusal comes back as -1 with a message that names the entry point, before anything is launched."""
    L = nat.lib()
    P = 4096                                                      # never dereferenced: the checks come first
    sizes = ((dict(H=2), b'3 x 3'), (dict(W=2), b'3 x 3'), (dict(H=65536, W=65536), b'too large'), (dict(V=0), b'65535'),
             (dict(V=65536, scratch_doubles=1 << 40), b'65535'), (dict(scratch_doubles=0), b'scratch'), (dict(V=8), b'scratch'),
             (dict(fixed_of=None), b'fixed_of'), (dict(F=0), b'bank'), (dict(F=-2), b'bank'), (dict(F=65536), b'bank'),
             (dict(H=1500, W=1500, F=955, scratch_doubles=1 << 40), b'too large'))     # F H W >= 2^31 with every single size good
    assert 955 * 1500 * 1500 >= 1 << 31 > 954 * 1500 * 1500 and 1500 <= nat.SIM_PATCH_MAX_W

    def fwd(**k):
        return nat.SimBankGradnccArgs(**dict(dict(moving=P, fx=P, fy=P, counted=P, totals=P, fixed_of=P, scratch=P, cost=P,
                                                  scratch_doubles=7 * 6 * 6, V=7, H=45, W=61, F=3), **k))

    def bwd(**k):
        return nat.SimBankGradnccBwdArgs(**dict(dict(moving=P, fx=P, fy=P, counted=P, totals=P, fixed_of=P, scratch=P, cost=P, d_moving=P,
                                                     scratch_doubles=7 * 6 * 6 + 4 * 7, V=7, H=45, W=61, F=3), **k))

    def patch(**k):
        return nat.SimPatchBankGradnccArgs(**dict(dict(moving=P, fx=P, fy=P, counted=P, ptotals=P, pflags=P, pcount=P, fixed_of=P, scratch=P,
                                                       cost=P, scratch_doubles=7 * 19 * 2, V=7, H=45, W=61, rho=3, stride=2, F=3), **k))

    for make, entry, fields, more in (
            (fwd, 'dfl_sim_bank_gradncc', ('moving', 'fx', 'fy', 'counted', 'totals', 'scratch', 'cost'), ()),
            (bwd, 'dfl_sim_bank_gradncc_bwd', ('moving', 'fx', 'fy', 'counted', 'totals', 'scratch', 'cost', 'd_moving'),
             ((dict(scratch_doubles=7 * 6 * 6 + 4 * 7 - 1), b'scratch'),)),
            (patch, 'dfl_sim_patch_bank_gradncc', ('moving', 'fx', 'fy', 'counted', 'ptotals', 'pflags', 'pcount', 'scratch', 'cost'),
             ((dict(rho=0), b'radius'), (dict(stride=0), b'stride'), (dict(rho=22), b'does not fit'),
              (dict(W=nat.SIM_PATCH_MAX_W + 1), b'DFL_SIM_PATCH_MAX_W'), (dict(scratch_doubles=7 * 19 * 2 - 1), b'scratch')))):
        fn = getattr(L, entry)
        for kw, word in tuple((dict(**{f: None}), b'required') for f in fields) + sizes + more:
            a = make(**kw)
            assert fn(C.addressof(a), None) == -1, (entry, kw)
            assert word in L.dfl_last_error() and entry.encode() + b':' in L.dfl_last_error(), (entry, kw, L.dfl_last_error())
        assert fn(None, None) == -1 and b'null' in L.dfl_last_error()


# ---- register_many -----------------------------------------------------------------------------------------------------
def _geom(S, poses=None, rot180=False):
    G, (H, W) = drr.training_grid(S['rows'], S['cols'], 0, 1, rot180)
    poses = dict(zip(drr.POSES, S['poses'] if poses is None else poses))
    return drr.Geometry(S['K'], S['E'], poses, S['I2P'], G, drr.default_objects(S['E'], poses, S['I2P']),
                        drr.Grid(-np.linalg.inv(S['K']) @ G, H, W))


def test_register_many_refuses_before_it_touches_the_gpu():
    S = D.scene('tilted')
    g = _geom(S)
    X = R.centres_phys(S)
    x2d = drr.project_points(g, X)
    H, W = g.size
    cpu = torch.zeros((2, H, W))
    other_masks = _geom(S)
    other_masks.objects[1] = drr.Obj(other_masks.objects[1].c2i, (5, 6))
    other_K = _geom(S)
    other_K.K = S['K'] * 1.01
    for kw, word in ((dict(levels=[(1, 2)]), 'levels'), (dict(similarity='patch', refine=2), 'refine'), (dict(refine=-1), 'refine'),
                     (dict(similarity='ssd'), 'similarity'), (dict(similarity='patch', patch_radius=0), 'radius'),
                     (dict(landmark_weight=-1.0), 'landmark_weight'),
                     (dict(theta0=np.zeros((3, 6))), 'theta0'), (dict(theta0=np.zeros(6)), 'theta0'), (dict(P0=np.zeros((1, 4, 4))), 'P0'),
                     (dict(landmarks=[(X, x2d)]), 'landmarks'), (dict(landmarks=(X, x2d, None)), 'landmarks'),
                     (dict(landmarks=[(X, x2d), (X, x2d[:, :4])]), 'expected'), (dict(landmarks=[None, (X, x2d)], moving=(1, 2)), 'pelvis'),
                     (dict(fixed=torch.zeros((3, H, W))), 'fixed'), (dict(masks=torch.zeros((1, H, W), dtype=torch.uint8)), 'masks'),
                     (dict(geoms=[g, _geom(S, rot180=True)]), 'differs'), (dict(geoms=[g, other_masks]), 'differs'),
                     (dict(geoms=[g, other_K]), 'differs'), (dict(geoms=[g, None]), 'Geometry'),
                     (dict(moving=()), 'moving'), (dict(popsize=3), 'population'),
                     (dict(max_views=15), 'max_views'), (dict(max_views=65536), 'max_views'), (dict(max_views=32.0), 'max_views'),
                     (dict(), 'Volume')):                        # and with good arguments the first thing missed is the device volume
        args = dict(dict(geoms=[g, g], fixed=cpu), **kw)
        geoms, fixed = args.pop('geoms'), args.pop('fixed')
        with pytest.raises(nat.DflError, match=word):
            reg.register_many(None, geoms, fixed, **args)
    with pytest.raises(nat.DflError, match='no problem'):
        reg.register_many(None, [], cpu[:0])
    with pytest.raises(nat.DflError, match='one per problem'):
        reg.register_many(None, g, cpu)
    # CPU tensors: a Volume cannot be made without a device, so a stand-in that passes for one reaches the tensor checks
    stand_in = object.__new__(drr.Volume)
    with pytest.raises(nat.DflError, match='GPU'):
        reg.register_many(stand_in, [g, g], cpu)
    with pytest.raises(nat.DflError, match='GPU'):
        reg.SimilarityBank(torch.zeros((2, 45, 61)))
    with pytest.raises(nat.DflError, match='radius'):
        reg.PatchSimilarityBank(torch.zeros((2, 45, 61)), radius=0)
    assert reg.default_max_views(180, 180) == (1 << 30) // (4 * 180 * 180) == 8285 and reg.default_max_views(45, 61) == 65535
    assert reg.default_max_views(1536, 1536) == 113
    for name in ('register_many', 'SimilarityBank', 'PatchSimilarityBank', 'cma_steps', 'bfgs_steps', 'lockstep', 'fixed_of_array'):
        assert name in reg.__all__


def test_fixed_of_is_checked_on_the_host():
    got = reg.fixed_of_array([2, 0, 1, 1, 0, 2, 0], 7, 3)
    assert got.dtype == np.int32 and got.tolist() == [2, 0, 1, 1, 0, 2, 0] and got.flags['C_CONTIGUOUS']
    assert reg.fixed_of_array(np.array([0, 4], np.int64)[::1], 2, 5).tolist() == [0, 4]
    assert reg.fixed_of_array(np.arange(6, dtype=np.uint8)[::2], 3, 5).tolist() == [0, 2, 4]
    for bad, V, F, word in (([0, 3], 2, 3, '0 .. 2'), ([-1, 0], 2, 3, 'holds -1'), ([0, 1], 3, 3, 'one per view'), ([[0, 1]], 2, 3, 'one per view'),
                            ([0.0, 1.0], 2, 3, 'integers'), ([True, False], 2, 3, 'integers'), ([], 1, 3, 'one per view')):
        with pytest.raises(nat.DflError, match=word):
            reg.fixed_of_array(bad, V, F)


# ---- the example -------------------------------------------------------------------------------------------------------
def test_command_line(capsys):
    import register_specimen as cli
    (path, spec), o = cli.parse(['f.h5', '17-1882', '--gt-lands'])
    assert (path, spec) == ('f.h5', '17-1882')
    assert o == {'--out': None, '--crop': 50, '--ds-factor': 8, '--popsize': 16, '--generations': 80, '--seed': 0, '--lands-csv': None,
                 '--projs': None, '--max-views': None, '--gt-lands': True, '--similarity': 'global', '--patch-radius': 7, '--patch-stride': 4,
                 '--landmark-weight': None, '--refine': 0}
    _, o = cli.parse(['--projs', '0,3,7', 'f.h5', '--lands-csv', 'l.csv', '--refine', '12', '17-1882', '--max-views', '64', '--popsize', '32',
                      '--landmark-weight', '0.01', '--out', 'run', '--crop', '2', '--ds-factor', '1', '--generations', '5', '--seed', '4'])
    assert o['--projs'] == [0, 3, 7] and o['--lands-csv'] == 'l.csv' and o['--refine'] == 12 and o['--max-views'] == 64 and o['--popsize'] == 32
    assert (o['--landmark-weight'], o['--out'], o['--crop'], o['--ds-factor'], o['--generations'], o['--seed']) == (0.01, 'run', 2, 1, 5, 4)
    _, o = cli.parse(['f.h5', 's', '--gt-lands', '--similarity', 'patch', '--patch-radius', '5', '--patch-stride', '2', '--generations', '0'])
    assert (o['--similarity'], o['--patch-radius'], o['--patch-stride'], o['--generations']) == ('patch', 5, 2, 0)
    base = ['f.h5', '17-1882', '--gt-lands']
    for bad in (['f.h5', '17-1882'], base + ['--lands-csv', 'l.csv'], ['f.h5', '--gt-lands'], base + ['0'], base + ['--femurs'],
                base + ['--offset', '0,0,0,0,0,0'], base + ['--projs'], base + ['--projs', '1,x'], base + ['--projs', '1,1'],
                base + ['--projs', '-1'], base + ['--popsize', '3'], base + ['--max-views', '8'], base + ['--max-views', '70000'],
                base + ['--refine', '-1'], base + ['--refine', '3', '--similarity', 'patch'], base + ['--similarity', 'local'],
                base + ['--generations', '-1'], base + ['--landmark-weight', 'nan'], base + ['--levels', '2']):
        assert cli.parse(bad) is None, bad
        assert cli.main(bad) == 1, bad
        out = capsys.readouterr().out
        assert out.startswith('Usage: ') and '(--lands-csv FILE | --gt-lands) [--projs 0,3,7]' in out and out.rstrip().endswith('[--max-views N]')
    import register_2d3d
    assert cli.read_lands_csv is register_2d3d.read_lands_csv and cli.pose_errors is register_2d3d.pose_errors
    assert cli.parse_similarity is register_2d3d.parse_similarity and cli.parse_refine is register_2d3d.parse_refine
    assert 'register_many' in cli.__doc__ and '_reg.csv' in cli.__doc__
