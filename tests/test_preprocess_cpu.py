"""dfl_amd.preprocess without a GPU: output sizes, the landmark maps against their numpy restatement and their inverse,
parameter errors in Python and at the C ABI, the ctypes mirrors against dfl_sizeof, the refusal of CPU tensors, the
specimen and landmark orders, and the command line of preprocess_full_res.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import preproc_ref as PR  # noqa: E402
import dfl_amd  # noqa: E402
from dfl_amd import _native as nat, preprocess as pp  # noqa: E402


def test_out_size_of_the_published_detector():
    assert [pp.out_size(1536, 1536, 50, f) for f in (1, 2, 4, 8, 16)] == [(s, s) for s in (1436, 718, 359, 180, 90)]
    assert pp.out_size(1536, 1536) == (180, 180)                      # defaults: crop 50, factor 8
    assert dfl_amd.out_size is pp.out_size


def test_out_size_non_square_with_clipped_boxes():
    assert pp.out_size(53, 70, crop=3, factor=4) == (12, 16)
    assert pp.out_size(53, 70, 3, 4) == PR.out_size(53, 70, 3, 4)


@pytest.mark.parametrize('R,C,crop,f', [(1536, 1536, 50, 8), (53, 70, 3, 4), (200, 232, 50, 3), (64, 64, 0, 1)])
def test_landmark_maps_invert_each_other(R, C, crop, f):
    g = np.random.default_rng(5)
    x = g.uniform(-40.0, max(R, C) + 40.0, size=(4, 2, 14))           # some outside the view
    rot = [0, 1, 1, 0]
    m = pp.map_lands(x, rot, R, C, crop, f)
    assert m.dtype == np.float64 and m.shape == x.shape and np.all(np.isfinite(m))
    np.testing.assert_allclose(m, PR.map_lands(x, rot, R, C, crop, f), rtol=0, atol=1e-9)
    back = pp.unmap_lands(m, rot, R, C, crop, f)
    np.testing.assert_allclose(back, x, rtol=0, atol=1e-9)
    np.testing.assert_allclose(back, PR.unmap_lands(m, rot, R, C, crop, f), rtol=0, atol=1e-9)
    assert np.abs(pp.map_lands(x, [1] * 4, R, C, crop, f) - pp.map_lands(x, [0] * 4, R, C, crop, f)).max() > 1


@pytest.mark.parametrize('f', [1, 2, 3, 8, 16])
def test_box_centres_map_to_pixel_indices(f):
    """The centre of the box of full-resolution pixels that output pixel i covers maps to i exactly."""
    R, C, crop = 1536, 1200, 50
    i = np.array([0, 1, 7, 31], np.float64)
    j = np.array([0, 2, 5, 60], np.float64)
    x = np.stack([crop + f * j + (f - 1) / 2.0, crop + f * i + (f - 1) / 2.0])[None]       # [1, 2, 4]: column, row
    m = pp.map_lands(x, [0], R, C, crop, f)
    assert np.array_equal(m[0, 0], j) and np.array_equal(m[0, 1], i)
    # rotated: the mirrored full-resolution points land in the same boxes
    Rc, Cc = R - 2 * crop, C - 2 * crop
    xr = np.stack([crop + Cc - 1 - (f * j + (f - 1) / 2.0), crop + Rc - 1 - (f * i + (f - 1) / 2.0)])[None]
    mr = pp.map_lands(xr, [1], R, C, crop, f)
    assert np.array_equal(mr[0, 0], j) and np.array_equal(mr[0, 1], i)


def test_parameter_errors():
    for kw in (dict(crop=32), dict(crop=40), dict(factor=0), dict(factor=17), dict(crop=-1)):
        with pytest.raises(nat.DflError):
            pp.out_size(64, 80, **dict(dict(crop=3, factor=4), **kw))
    assert pp.out_size(64, 80, crop=31, factor=16) == (1, 2)
    x = np.zeros((1, 2, 3))
    for fn in (pp.map_lands, pp.unmap_lands):
        with pytest.raises(nat.DflError):
            fn(x, [0], 64, 64, 32, 2)
        with pytest.raises(nat.DflError):
            fn(x, [0], 64, 64, 3, 17)
        with pytest.raises(nat.DflError):
            fn(x, [0, 1], 64, 64, 3, 2)               # one flag per projection
        with pytest.raises(nat.DflError):
            fn(np.zeros((2, 3)), [0, 1], 64, 64, 3, 2)


def test_cpu_tensors_are_refused():
    with pytest.raises(nat.DflError, match='GPU'):
        pp.preprocess_projs(torch.ones(1, 16, 16), [0], crop=1, factor=2)
    with pytest.raises(nat.DflError, match='GPU'):
        pp.preprocess_segs(torch.zeros(1, 16, 16, dtype=torch.uint8), [0], crop=1, factor=2)
    with pytest.raises(nat.DflError, match='GPU'):
        pp.restore_labels(torch.zeros(1, 7, 7, dtype=torch.uint8), [0], 16, 16, crop=1, factor=2)
    with pytest.raises(nat.DflError, match='GPU'):
        pp.preprocess_projs(np.ones((1, 16, 16), np.float32), [0], crop=1, factor=2)


def test_struct_mirrors_match_the_library():
    L = nat.lib()
    for cls in (nat.PreprocProjsArgs, nat.PreprocSegsArgs, nat.RestoreLabelsArgs):
        assert L.dfl_sizeof(nat._SIZEOF_ORDER.index(cls)) == C.sizeof(cls) > 0
    for fn in ('dfl_preproc_projs', 'dfl_preproc_segs', 'dfl_restore_labels'):
        assert fn in nat.EXPORTS and hasattr(L, fn)
    assert nat.PREPROC_MAX_FACTOR == 16


def test_c_abi_refuses_bad_arguments():
    """Every refusal comes back as -1 with a message, before anything is launched."""
    L = nat.lib()
    P = 4096                                          # never dereferenced: the checks come first
    for fn, mk in (('dfl_preproc_projs', lambda **k: nat.PreprocProjsArgs(**dict(dict(pixels=P, rot180=P, out=P, scratch=P, N=1, R=64,
                                                                                    C=80, crop=3, factor=4, log=1,
                                                                                    min_intensity=1.0), **k))),
                   ('dfl_preproc_segs', lambda **k: nat.PreprocSegsArgs(**dict(dict(segs=P, rot180=P, out=P, status=P, N=1, R=64,
                                                                                  C=80, crop=3, factor=4), **k))),
                   ('dfl_restore_labels', lambda **k: nat.RestoreLabelsArgs(**dict(dict(labels=P, rot180=P, out=P, N=1, R=64, C=80,
                                                                                       crop=3, factor=4), **k)))):
        f = getattr(L, fn)
        for kw, word in ((dict(crop=32), b'crop'), (dict(crop=100), b'crop'), (dict(factor=0), b'factor'),
                         (dict(factor=17), b'factor'), (dict(rot180=None), b'required'), (dict(out=None), b'required'),
                         (dict(N=0), b'sizes')):
            a = mk(**kw)
            assert f(C.addressof(a), None) == -1, (fn, kw)
            assert word in L.dfl_last_error() and fn.encode() in L.dfl_last_error(), (fn, kw, L.dfl_last_error())
        assert f(None, None) == -1 and b'null' in L.dfl_last_error()
    a = nat.PreprocProjsArgs(pixels=None, rot180=P, out=P, scratch=P, N=1, R=64, C=80, crop=3, factor=4, log=1, min_intensity=1.0)
    assert L.dfl_preproc_projs(C.addressof(a), None) == -1 and b'required' in L.dfl_last_error()
    a = nat.PreprocProjsArgs(pixels=P, rot180=P, out=P, scratch=P, N=1, R=64, C=80, crop=3, factor=4, log=1, min_intensity=0.0)
    assert L.dfl_preproc_projs(C.addressof(a), None) == -1 and b'min_intensity' in L.dfl_last_error()
    a = nat.PreprocSegsArgs(segs=P, rot180=P, out=P, status=None, N=1, R=64, C=80, crop=3, factor=4)
    assert L.dfl_preproc_segs(C.addressof(a), None) == -1 and b'required' in L.dfl_last_error()


def test_specimen_and_landmark_order():
    ids = list(pp.SPECIMEN_ORDER)
    assert pp.specimen_order(sorted(ids)) == ['17-1882', '18-1109', '18-0725', '18-2799', '18-2800', '17-1905']
    assert pp.specimen_order(['18-2800', '17-1882']) == ['17-1882', '18-2800']           # not the six: sorted
    assert pp.specimen_order(ids + ['99-0001']) == sorted(ids + ['99-0001'])
    assert pp.land_order(reversed(pp.LAND_ORDER)) == pp.LAND_ORDER and len(pp.LAND_ORDER) == 14
    assert pp.land_order(['zz', 'SPS-l', 'FH-r', 'aa']) == ['FH-r', 'SPS-l', 'aa', 'zz']


def test_command_line():
    import preprocess_full_res as cli
    a = cli.parse_args(['in.h5', 'out.h5'])
    assert (a.src, a.dst, a.ds_factor, a.crop, a.specimens, a.no_log, a.min_intensity, a.chunk, a.gzip) == \
        ('in.h5', 'out.h5', 8, 50, None, False, 1.0, 32, False)
    a = cli.parse_args(['in.h5', 'out.h5', '--ds-factor', '2', '--crop', '10', '--specimens', '18-2800,17-1882', '--no-log',
                        '--min-intensity', '0.5', '--chunk', '4', '--gzip'])
    assert (a.ds_factor, a.crop, a.specimens, a.no_log, a.min_intensity, a.chunk, a.gzip) == \
        (2, 10, ['18-2800', '17-1882'], True, 0.5, 4, True)


def test_reference_model_on_a_hand_made_case():
    """preproc_ref itself, on values small enough to do by hand: 4 x 6 image, crop 0, f = 4 -> boxes of 4 x 4 and 4 x 2."""
    img = np.full((1, 4, 6), 4.0)
    img[0, :, 4:] = 1.0
    out = PR.projs(img, [0], 0, 4)
    np.testing.assert_allclose(out[0], [[0.0, np.log(4.0)]], atol=1e-15)
    np.testing.assert_allclose(PR.projs(img, [1], 0, 4)[0], [[np.log(4.0) / 2, 0.0]], atol=1e-15)
    np.testing.assert_allclose(PR.projs(img, [0], 0, 4, log=False)[0], [[4.0, 1.0]], atol=0)
    lab = np.array([[[1, 1, 2, 2, 5, 5], [3, 3, 3, 0, 5, 6], [2, 2, 1, 1, 6, 6], [0, 0, 0, 7, 7, 7]]], np.uint8)
    # first box: 0 x4, 1 x4, 2 x4, 3 x3, 7 x1 -> 0 (smallest of the tie); second: 5 x3, 6 x3, 7 x2 -> 5
    assert PR.segs(lab, [0], 0, 4).tolist() == [[[0, 5]]]
    small = np.array([[[3, 9]]], np.uint8)
    full = PR.restore(small, [0], 4, 6, 0, 4)
    assert full[0, :, :4].tolist() == [[3] * 4] * 4 and full[0, :, 4:].tolist() == [[9] * 2] * 4
    full = PR.restore(small, [1], 4, 6, 0, 4)
    assert full[0, :, 2:].tolist() == [[3] * 4] * 4 and full[0, :, :2].tolist() == [[9] * 2] * 4
    assert np.array_equal(PR.segs(full, [1], 0, 4), small)


@pytest.mark.parametrize('R,C,crop,f', [(53, 70, 3, 4), (40, 96, 8, 3), (64, 64, 0, 16)])
def test_reference_restore_by_repetition_equals_the_loops(R, C, crop, f):
    Ro, Co = PR.out_size(R, C, crop, f)
    small = np.random.default_rng(f).integers(0, 256, size=(2, Ro, Co)).astype(np.uint8)
    assert np.array_equal(PR.restore_fast(small, [1, 0], R, C, crop, f), PR.restore(small, [1, 0], R, C, crop, f))
