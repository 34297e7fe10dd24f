"""The mutual-information cost without a GPU: the numpy model (tests/mi_ref.py) on answers known by hand, the committed
floors (tests/golden/floors/mi.json) against the model, the adjoint against central differences with the bar the floor sets,
the struct mirrors, every refusal of the C ABI (the library loads without a GPU and refuses before it launches), the
refusals of dfl_amd.register and the command line of the two examples.
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
import mi_floor as MF  # noqa: E402
import mi_ref as M  # noqa: E402
import reg_floor as FL  # noqa: E402
import reg_ref as R  # noqa: E402
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, drr, register as reg  # noqa: E402


# ---- the model ---------------------------------------------------------------------------------------------------------
def test_known_answers():
    rng = np.random.default_rng(0)
    two = (rng.random((12, 10)) < 0.5).astype(np.float32)
    two[0, :2] = 0, 1                                             # both levels occur
    n1 = int(two.sum())
    fbin, info = M.prepare(two, None, 2)
    assert info.tolist() == [120.0, 0.0, 1.0, 0.0] and np.array_equal(fbin, two.astype(np.uint8))
    # two identical two-level images: a diagonal histogram; MI = the entropy of the levels, log 2 when they are equally frequent
    h = M.hist(two, fbin, 0.0, 1.0, 2, 2)
    assert h.tolist() == [[4096 * (120 - n1), 0], [0, 4096 * n1]]
    p = n1 / 120.0
    assert abs(M.cost(two, fbin, (0.0, 1.0), 2, 2) + (-p * np.log(p) - (1 - p) * np.log(1 - p))) <= 1e-15
    half = np.zeros((4, 6), np.float32)
    half[:, 3:] = 1
    fb, _ = M.prepare(half, None, 2)
    assert M.cost(half, fb, (0.0, 1.0), 2, 2) == -np.log(2.0)
    assert M.cost(-half, fb, (-1.0, 0.0), 2, 2) == -np.log(2.0)   # any one-to-one mapping of the intensities
    assert abs(M.cost(half, M.prepare(half, None, 64)[0], (0.0, 1.0), 64, 64) + np.log(2.0)) <= 1e-15
    # independent images: every joint entry is the product of its marginals
    rows = np.zeros((4, 6), np.float32)
    rows[2:] = 1
    assert M.hist(rows, fb, 0.0, 1.0, 2, 2).tolist() == [[6 * 4096] * 2] * 2 and M.cost(rows, fb, (0.0, 1.0), 2, 2) == 0.0
    # a constant image, on either side
    assert M.cost(np.full((4, 6), np.float32(0.3)), fb, (0.0, 1.0), 2, 8) == 0.0
    flat, info = M.prepare(np.full((4, 6), np.float32(5)), None, 7)
    assert not flat.any() and info.tolist() == [24.0, 5.0, 5.0, 0.0] and M.cost(half, flat, (0.0, 1.0), 7, 2) == 0.0
    # the Parzen window: a value three quarters of the way between two bins
    h = M.hist(np.full((1, 1), np.float32(0.75)), np.zeros((1, 1), np.uint8), 0.0, 1.0, 2, 2)
    assert h.tolist() == [[1024, 0], [3072, 0]]
    h = M.hist(np.array([[np.nan, -3.0, 9.0, 0.5]], np.float32), np.array([[0, 1, 1, M.SKIP]], np.uint8), 0.0, 2.0, 2, 3)
    assert h.tolist() == [[4096, 4096], [0, 0], [0, 4096]]        # NaN counts as lo, values outside clamp, SKIP is not counted
    # nothing counted, masks, non-finite fixed values, void ranges
    fixed = np.arange(12, dtype=np.float32).reshape(3, 4)
    fixed[0, 0], fixed[2, 3] = np.nan, np.inf
    mask = np.ones((3, 4), np.uint8)
    mask[1] = 0
    fbin, info = M.prepare(fixed, mask, 4)
    assert info.tolist() == [6.0, 1.0, 10.0, 0.0]
    assert fbin.tolist() == [[255, 0, 0, 0], [255] * 4, [3, 3, 3, 255]]
    assert M.prepare(fixed, np.zeros((3, 4), np.uint8), 4)[1].tolist() == [0.0] * 4
    none = M.prepare(fixed, np.zeros((3, 4), np.uint8), 4)[0]
    assert (none == M.SKIP).all() and M.cost(fixed, none, (0.0, 1.0), 4, 4) == 0.0 and not M.adjoint(fixed, none, 0.0, 1.0, 4, 4).any()
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (np.nan, 1.0), (0.0, np.inf), (-3e38, 3e38), (0.0, 1e-45)):
        assert M.scale(lo, hi, 64)[1], (lo, hi)
        assert np.isnan(M.cost(fixed, fbin, (lo, hi), 4, 64)) and not M.hist(fixed, fbin, lo, hi, 4, 64).any()
        assert not M.adjoint(fixed, fbin, lo, hi, 4, 64).any()
    assert not M.scale(0.0, 1.0, 2)[1]


def test_histogram_totals_and_the_unquantised_variant():
    for H, W in R.SIM_SIZES:
        fixed, moving = R.sim_images(H, W)
        lo, hi = MF.sim_range(moving)
        for name, mask in R.sim_masks(H, W).items():
            for Bf, Bm in ((8, 8), (5, 13), (64, 2)):
                fbin, info = M.prepare(fixed, mask, Bf)
                n = int(info[0])
                assert n == int(M.counted(fixed, mask).sum()) == int((fbin != M.SKIP).sum()) and (fbin[fbin != M.SKIP] < Bf).all()
                for v in moving:
                    h = M.hist(v, fbin, lo, hi, Bf, Bm)
                    assert h.dtype == np.int64 and h.shape == (Bm, Bf) and int(h.sum()) == M.UNIT * n and h.min() >= 0
                    hu = M.hist(v, fbin, lo, hi, Bf, Bm, None)
                    assert np.abs(hu - h / M.UNIT).max() <= 0.5 / M.UNIT * max(n, 1)
                    g = M.adjoint(v, fbin, lo, hi, Bf, Bm)
                    assert not g[(fbin == M.SKIP) | ~((v > lo) & (v < hi))].any()


def test_the_committed_floors_are_the_models():
    doc = MF.load()
    assert doc['fd_factor'] == MF.FD_FACTOR == 4.0 and doc['fd_eps'] == MF.FD_EPS and doc['model_bar_pixels'] == MF.MODEL_BAR == 1.0
    now = MF.fd_floors()
    assert sorted(now) == sorted(doc['finite_differences']) == ['17x70', '45x61']
    for key, e in now.items():
        want = doc['finite_differences'][key]
        assert e['inside'] == want['inside'] > 500
        np.testing.assert_allclose([e['central_difference'], e['adjoint_dot_direction']], [want['central_difference'], want['adjoint_dot_direction']],
                                   rtol=1e-9)
        assert want['relative'] <= 2e-5                           # the formula is the derivative: 1.2e-5 and 4e-7
    q = MF.quantisation()
    assert sorted(q) == sorted(doc['quantisation']) and len(q) == 9
    for key, e in q.items():
        want = doc['quantisation'][key]
        assert e['counted'] == want['counted']
        np.testing.assert_allclose(e['cost'], want['cost'], atol=1e-12)
        np.testing.assert_allclose([e['cost_difference'], e['adjoint_difference']], [want['cost_difference'], want['adjoint_difference']],
                                   rtol=1e-6, atol=1e-15)
    assert q['3x3/ragged']['counted'] == 0 and not any(q['3x3/ragged']['cost'])
    # the registration case: the order in which the bin counts were tried, the first that got the model within a pixel, its bar
    r = doc['registration']
    assert r['order'] == list(MF.BINS_TO_TRY) == [16, 8, 32] and sorted(r['tried']) == ['16', '32', '8']
    for b in r['order']:
        t = r['tried'][str(b)]
        assert t['theta0'] == list(R.THETA_START) and min(t['start_px']) >= 10 and t['bins'] == b
    assert r['chosen'] == next(b for b in r['order'] if max(r['tried'][str(b)]['final_px']) <= MF.MODEL_BAR)
    bins, bar = MF.registration()
    assert bins == r['chosen'] and FL.PIXEL_BAR <= bar <= 1.0 and bar >= 2.0 * max(r['tried'][str(bins)]['final_px'])


@pytest.mark.parametrize('size', MF.FD_SIZES)
def test_the_adjoint_is_the_derivative(size):
    """Bar: 4 x the recorded relative distance (mi.json: 1.2e-5 at 45 x 61, 3.9e-7 at 17 x 70).  Without the -log h_a term of the
    table, or with its sign flipped, the same measure is far outside: shown here."""
    bar = MF.fd_bar(*size)
    rel, fd, dot, inside = MF.fd_case(*size)
    dropped, flipped = MF.fd_case(*size, row_term=0.0)[0], MF.fd_case(*size, row_term=-1.0)[0]
    print('%d x %d: central difference %.9g, <adjoint, d> %.9g, relative %.3e (bar %.3e); without -log h_a %.3e, with +log h_a %.3e'
          % (size + (fd, dot, rel, bar, dropped, flipped)))
    assert rel <= bar
    assert dropped > 100 * bar and flipped > 100 * bar


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_struct_mirrors_and_their_place():
    L = nat.lib()
    new = [nat.SimMiPrepareArgs, nat.SimMiArgs, nat.SimMiBwdArgs]
    for cls, size in zip(new, (48, 80, 96)):
        assert L.dfl_sizeof(nat._SIZEOF_ORDER.index(cls)) == C.sizeof(cls) == size
    k = nat._SIZEOF_ORDER.index(nat.ToolsArgs)
    assert nat._SIZEOF_ORDER[k + 1:k + 4] == new and nat._SIZEOF_ORDER[k + 4] is nat.SimPatchPrepareArgs
    assert nat._SIZEOF_ORDER[-3:] == [nat.DrrObject, nat.DrrArgs, nat.OptimPackArgs] and L.dfl_sizeof(len(nat._SIZEOF_ORDER)) == -1
    for fn in ('dfl_sim_mi_prepare', 'dfl_sim_mi', 'dfl_sim_mi_bwd'):
        assert fn in nat.EXPORTS and hasattr(L, fn)
    assert (nat.SIM_MI_UNIT, nat.SIM_MI_MAX_BINS, nat.SIM_MI_SKIP, nat.SIM_MI_INFO) == (M.UNIT, M.MAX_BINS, M.SKIP, 4) == (4096, 64, 255, 4)
    assert nat.SIM_MI_RUN % 256 == 0 and nat.SIM_MI_RUN < 2 ** 19
    assert [n for n, *_ in nat.SimMiArgs._fields_] == ['moving', 'fbin', 'info', 'mrange', 'fixed_of', 'hist', 'cost', 'V', 'H', 'W', 'F', 'Bf', 'Bm']


def test_c_abi_refuses_bad_arguments():
    """Every refusal comes back as -1 with a message that names the entry point, before anything is launched."""
    L = nat.lib()
    P = 4096                                                      # never dereferenced: the checks come first

    def prep(**k):
        return nat.SimMiPrepareArgs(**dict(dict(fixed=P, mask=None, fbin=P, info=P, H=45, W=61, Bf=32), **k))

    for kw, word in ((dict(fixed=None), b'required'), (dict(fbin=None), b'required'), (dict(info=None), b'required'), (dict(H=0), b'bad sizes'),
                     (dict(W=0), b'bad sizes'), (dict(H=-1), b'bad sizes'), (dict(H=65536, W=32768), b'2^31'), (dict(Bf=1), b'bins'),
                     (dict(Bf=65), b'bins'), (dict(Bf=0), b'bins')):
        a = prep(**kw)
        assert L.dfl_sim_mi_prepare(C.addressof(a), None) == -1, kw
        assert word in L.dfl_last_error() and b'dfl_sim_mi_prepare' in L.dfl_last_error(), (kw, L.dfl_last_error())
    assert L.dfl_sim_mi_prepare(None, None) == -1 and b'null' in L.dfl_last_error()

    common = dict(moving=P, fbin=P, info=P, mrange=P, fixed_of=None, hist=P, cost=P, V=6, H=45, W=61, F=1, Bf=32, Bm=32)
    bad = [(dict(moving=None), b'required'), (dict(fbin=None), b'required'), (dict(info=None), b'required'), (dict(mrange=None), b'required'),
           (dict(hist=None), b'required'), (dict(cost=None), b'required'), (dict(H=0), b'bad sizes'), (dict(W=0), b'bad sizes'),
           (dict(H=65536, W=32768), b'2^31'), (dict(V=0), b'65535'), (dict(V=65536), b'65535'), (dict(F=0), b'65535'), (dict(F=65536), b'65535'),
           (dict(F=3, H=32768, W=32768), b'2^31'), (dict(Bf=1), b'Bf'), (dict(Bf=65), b'Bf'), (dict(Bm=1), b'Bm'), (dict(Bm=65), b'Bm')]
    for kw, word in bad:
        a = nat.SimMiArgs(**dict(common, **kw))
        assert L.dfl_sim_mi(C.addressof(a), None) == -1, kw
        assert word in L.dfl_last_error() and b'dfl_sim_mi:' in L.dfl_last_error(), (kw, L.dfl_last_error())
    for kw, word in bad + [(dict(ell=None), b'required'), (dict(d_moving=None), b'required')]:
        a = nat.SimMiBwdArgs(**dict(dict(common, ell=P, d_moving=P), **kw))
        assert L.dfl_sim_mi_bwd(C.addressof(a), None) == -1, kw
        assert word in L.dfl_last_error() and b'dfl_sim_mi_bwd' in L.dfl_last_error(), (kw, L.dfl_last_error())
    assert L.dfl_sim_mi(None, None) == -1 and b'null' in L.dfl_last_error()
    assert L.dfl_sim_mi_bwd(None, None) == -1 and b'null' in L.dfl_last_error()


# ---- Python ------------------------------------------------------------------------------------------------------------
def _geom(S):
    named = dict(zip(drr.POSES, S['poses']))
    return drr.Geometry(S['K'], S['E'], named, S['I2P'], np.eye(3), drr.default_objects(S['E'], named, S['I2P']),
                        drr.Grid(S['Q'], S['rows'], S['cols']))


def test_python_refusals_come_before_any_device():
    S = D.scene('tilted')
    g = _geom(S)
    H, W = S['rows'], S['cols']
    img = torch.zeros(H, W)                                       # on the CPU
    seg = torch.zeros((H, W), dtype=torch.uint8)
    for kw, word in ((dict(patch_weight='variance'), 'patch_weight'), (dict(segmentation=seg), "belong to similarity='outline'"),
                     (dict(outline_sets=[[1]]), "belong to similarity='outline'"), (dict(mi_bins=1), 'mi_bins'), (dict(mi_bins=65), 'mi_bins'),
                     (dict(mi_bins=(8, 1)), 'mi_bins'), (dict(mi_bins=(8, 8, 8)), 'mi_bins'), (dict(mi_bins=8.0), 'mi_bins'),
                     (dict(mi_bins=True), 'mi_bins'), (dict(mi_bins='16'), 'mi_bins'), (dict(mi_range=(1.0, 1.0)), 'mi_range'),
                     (dict(mi_range=(2.0, 1.0)), 'mi_range'), (dict(mi_range=(0.0, float('nan'))), 'mi_range'),
                     (dict(mi_range=(0.0, float('inf'))), 'mi_range'), (dict(mi_range=3.0), 'mi_range'), (dict(mi_range=(1.0, 1.0 + 1e-12)), 'mi_range'),
                     (dict(refine=-1), 'refine'), (dict(landmark_weight=-1.0), 'landmark_weight'),
                     (dict(refine=3, landmarks=(np.zeros((4, 3)), np.zeros((2, 4))), levels=[(1, 2)]), 'levels'),
                     (dict(mi_bins=16, mi_range=(0.0, 2.0), refine=5, mask=torch.ones((H, W), dtype=torch.uint8)), 'Volume')):
        with pytest.raises(nat.DflError, match=word):
            reg.register(None, g, img, **dict(dict(similarity='mi'), **kw))
        many = {k: v for k, v in kw.items() if k not in ('segmentation', 'outline_sets', 'levels', 'mask')}
        if len(many) == len(kw):
            with pytest.raises(nat.DflError, match=word):
                reg.register_many(None, [g, g], torch.zeros((2, H, W)), **dict(dict(similarity='mi'), **many))
    with pytest.raises(nat.DflError, match="belongs to similarity='mi'"):
        reg.register(None, g, img, mi_range=(0.0, 1.0))
    with pytest.raises(nat.DflError, match="belongs to similarity='mi'"):
        reg.register_many(None, [g, g], torch.zeros((2, H, W)), similarity='patch', mi_range=(0.0, 1.0))
    with pytest.raises(nat.DflError, match="'outline' or 'mi'"):
        reg.register(None, g, img, similarity='nmi')
    stand_in = object.__new__(drr.Volume)                         # passes for a Volume: the tensor check is reached
    with pytest.raises(nat.DflError, match='fixed image on the GPU'):
        reg.register(stand_in, g, img, similarity='mi')
    for bad in (img, img.numpy(), img[None]):
        with pytest.raises(nat.DflError, match='GPU'):
            reg.MISimilarity(bad)
    with pytest.raises(nat.DflError, match='mi_bins'):
        reg.MISimilarity(img, bins=1)
    assert 'MISimilarity' in reg.__all__ and reg._mi_bins(16) == (16, 16) and reg._mi_bins((64, 2)) == (64, 2) and reg._mi_bins([5, 13]) == (5, 13)
    assert reg._mi_range(0, 2) == (np.float32(0), np.float32(2))


# ---- the examples ------------------------------------------------------------------------------------------------------
def test_command_line(capsys, monkeypatch):
    import register_2d3d as one
    import register_specimen as many
    assert one.parse_mi_bins(['a', '--gt-lands']) == (['a', '--gt-lands'], None)
    assert one.parse_mi_bins(['a', '--mi-bins', '16', '--refine', '3']) == (['a', '--refine', '3'], 16)
    assert one.parse_mi_bins(['--mi-bins', '2', 'a', '--mi-bins', '64']) == (['a'], 64)
    for bad in (['--mi-bins'], ['a', '--mi-bins', 'x'], ['--mi-bins', '1'], ['--mi-bins', '65'], ['--mi-bins', '8.5']):
        assert one.parse_mi_bins(bad) is None, bad
    assert many.parse_mi_bins is one.parse_mi_bins and many.cost_keywords is one.cost_keywords
    assert one.cost_keywords('global', 'uniform', None) == dict(similarity='global', patch_weight='uniform')
    assert one.cost_keywords('patch', 'variance', None) == dict(similarity='patch', patch_weight='variance')
    assert one.cost_keywords('global', 'uniform', 16) == dict(similarity='mi', mi_bins=16)
    assert one.cost_keywords('patch', 'uniform', 16) is None and one.cost_keywords('global', 'variance', 16) is None
    # what parse_similarity returns and the tail of the usage text are as they were
    assert one.parse_similarity(['a']) == (['a'], {'--similarity': 'global', '--patch-radius': 7, '--patch-stride': 4, '--landmark-weight': None})
    assert one.parse_similarity(['a', '--similarity', 'mi']) is None
    base1, base2 = ['f.h5', '17-1882', '0', '--gt-lands'], ['f.h5', '17-1882', '--gt-lands']
    for cli, base in ((one, base1), (many, base2)):
        for bad in (['--mi-bins'], ['--mi-bins', '1'], ['--mi-bins', '16', '--similarity', 'patch'],
                    ['--mi-bins', '16', '--similarity', 'patch', '--patch-weight', 'variance'], ['--patch-weight', 'variance', '--mi-bins', '16']):
            assert cli.main(base + bad) == 1, bad
            out = capsys.readouterr().out
            assert out.startswith('Usage: ') and '[--mi-bins N]' in out
    assert one.USAGE.endswith('[--landmark-weight 0]') and many.USAGE.endswith('[--max-views N]')
    # a good command line passes the parser: the next thing missed is the GPU
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    for cli, base in ((one, base1), (many, base2)):
        with pytest.raises(nat.DflError, match='no GPU visible'):
            cli.main(base + ['--mi-bins', '16', '--refine', '2'])
        assert not capsys.readouterr().out.startswith('Usage: ')
