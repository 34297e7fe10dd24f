"""The label clean-up without a GPU: the numpy restatement (labels_ref.py) against scipy.ndimage, the command line of
clean_segs.py, its file rewrite, and the C ABI entries in the header."""
import argparse
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, h5lite  # noqa: E402
import clean_segs  # noqa: E402
import labels_ref as LR  # noqa: E402

TILE = (8, 16)          # the patterns scale with the tile they are told: small here, labels.TILE on the GPU
SHAPES = LR.shapes(TILE) + [(11, 13)]
ENTRIES = ['dfl_label_components', 'dfl_label_select_scratch_bytes', 'dfl_label_select', 'dfl_label_dilate']


def _cases():
    return [(name, H, W) for name in LR.PATTERNS for H, W in SHAPES]


@pytest.mark.parametrize('name,H,W', _cases())
def test_restatement_agrees_with_scipy_label(name, H, W):
    ndi = pytest.importorskip('scipy.ndimage')
    seg = LR.pattern(name, H, W, TILE)
    for connectivity, structure in ((4, ndi.generate_binary_structure(2, 1)), (8, np.ones((3, 3), dtype=int))):
        root, area, info = LR.components(seg, connectivity)
        want_root = np.full((H, W), -1, dtype=np.int64)
        want_area = np.zeros((H, W), dtype=np.int64)
        flat = np.arange(H * W).reshape(H, W)
        for v in np.unique(seg):
            lab, n = ndi.label(seg == v, structure=structure)
            for k in range(1, n + 1):                         # canonical name of a scipy component: its smallest flat index
                inside = lab == k
                first = int(flat[inside].min())
                want_root[inside] = first
                want_area.ravel()[first] = int(inside.sum())
        assert np.array_equal(root, want_root)
        assert np.array_equal(area, want_area)
        # info from its definition, per component: border bit and the values around it
        for p in np.flatnonzero(area.ravel() > 0):
            inside = root == p
            grown = ndi.binary_dilation(inside, structure=ndi.generate_binary_structure(2, 1)) & ~inside
            bits = 0
            for v in np.unique(seg[grown]):
                bits |= 1 << min(int(v), 30)
            if inside[0].any() or inside[-1].any() or inside[:, 0].any() or inside[:, -1].any():
                bits |= 1 << 31
            assert int(info.ravel()[p]) == bits, (name, connectivity, p)
        assert not info.ravel()[area.ravel() == 0].any()


@pytest.mark.parametrize('name,H,W', _cases())
def test_restatement_fill_agrees_with_scipy_fill_holes(name, H, W):
    ndi = pytest.importorskip('scipy.ndimage')
    seg = LR.pattern(name, H, W, TILE)
    for v in range(1, LR.NUM_CLASSES):
        one = np.where(seg == v, v, 0).astype(np.uint8)
        out, stats = LR.clean(one[None], keep='all', fill_holes=H * W)
        want = (ndi.binary_fill_holes(one == v) * v).astype(np.uint8)
        assert np.array_equal(out[0], want), (name, v)
        assert int(stats['filled'][0, v]) == int((want != one).sum()) and not stats['removed'].any()


def test_restatement_rules_on_the_patterns_made_for_them():
    H, W = 12, 14
    # the tie: the first of the two equal components in row-major order stays, the other and the speck go
    seg = LR.pattern('tie', H, W, TILE)
    out, stats = LR.clean(seg[None])
    assert out[0, 1, 6] == 1 and out[0, 4, 1] == 0 and out[0, 8, 8] == 0 and int(stats['removed'][0, 1]) == 7
    out, _ = LR.clean(seg[None], keep='all', min_area=5)
    assert out[0, 1, 6] == 1 and out[0, 4, 1] == 1 and out[0, 8, 8] == 0
    # a ring closed only diagonally encloses its hole, at either connectivity of the labels; the 5-pixel hole needs 5
    seg = LR.pattern('diagonal_ring', H, W, TILE)
    for connectivity in (4, 8):
        out, stats = LR.clean(seg[None], connectivity=connectivity, keep='all', fill_holes=4)
        assert out[0, 2, 2] == 2 and out[0, 4, 7] == 0 and int(stats['filled'][0, 2]) == 1
    out, stats = LR.clean(seg[None], keep='all', fill_holes=5)
    assert out[0, 4, 7] == 2 and int(stats['filled'][0, 2]) == 6
    # not filled: two labels around the hole, a pocket at the border, a ring of a value beyond the classes
    for name, hole in (('hole_two_labels', (2, 2)), ('hole_at_border', (0, 2)), ('beyond_classes', (2, 2))):
        seg = LR.pattern(name, H, W, TILE)
        out, _ = LR.clean(seg[None], keep='all', fill_holes=H * W)
        assert out[0][hole] == 0, name
    seg = LR.pattern('hole_at_border', H, W, TILE)
    assert LR.clean(seg[None], keep='all', fill_holes=1)[0][0, 4, 4] == 3
    # values beyond the classes pass through keep='largest' untouched, islands included
    seg = LR.pattern('beyond_classes', H, W, TILE)
    out, stats = LR.clean(seg[None])
    assert np.array_equal(out[0] == 9, seg == 9) and out[0, 6, 1] == 0 and out[0, 8, 3] == 1
    assert int(stats['removed'][0, 1]) == 1


def test_restatement_dilate_is_the_disc():
    ndi = pytest.importorskip('scipy.ndimage')
    seg = LR.pattern('random_sparse', 23, 31, TILE)
    for labels in ((1,), (2, 5)):
        for radius in (0, 1, 3, 7):
            r, c = np.mgrid[-radius:radius + 1, -radius:radius + 1]
            disc = r * r + c * c <= radius * radius
            want = ndi.binary_dilation(np.isin(seg, labels), structure=disc).astype(np.uint8)
            assert np.array_equal(LR.dilate(seg, labels, radius), want)


def test_clean_segs_parser():
    p = clean_segs.build_parser()
    positional = [a.dest for a in p._actions if not a.option_strings]
    assert positional == ['seg_file', 'seg_group', 'out_group']
    args = p.parse_args(['out.h5', 'nn-segs', 'nn-segs-clean'])
    assert vars(args) == dict(seg_file='out.h5', seg_group='nn-segs', out_group='nn-segs-clean', out_file=None, num_classes=7,
                              connectivity=8, keep='largest', min_area=0, fill_holes=0)
    args = p.parse_args(['a.h5', 'g', 'h', '--out-file', 'b.h5', '--num-classes', '5', '--connectivity', '4', '--keep', 'all',
                         '--min-area', '9', '--fill-holes', '16'])
    assert (args.out_file, args.num_classes, args.connectivity, args.keep, args.min_area, args.fill_holes) == \
        ('b.h5', 5, 4, 'all', 9, 16)
    for bad in (['--connectivity', '6'], ['--keep', 'first']):
        with pytest.raises(SystemExit):
            p.parse_args(['a.h5', 'g', 'h'] + bad)


def test_clean_segs_refuses_to_run_without_a_gpu(monkeypatch, tmp_path):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(nat.DflError, match='no GPU'):
        clean_segs.main([str(tmp_path / 'missing.h5'), 'nn-segs', 'nn-segs-clean'])
    from dfl_amd import labels
    host = torch.zeros((4, 4), dtype=torch.uint8)
    for call in (lambda: labels.components(host), lambda: labels.clean(host), lambda: labels.bone_mask(host, 1)):
        with pytest.raises(nat.DflError, match='on the GPU'):
            call()


def test_clean_segs_rewrites_the_file_with_everything_else_unchanged(tmp_path):
    rng = np.random.default_rng(3)
    segs = rng.integers(0, 7, size=(3, 9, 11)).astype(np.uint8)
    heats = rng.random((3, 2, 9, 11)).astype(np.float32)
    path = str(tmp_path / 'out.h5')
    with h5lite.File(path, 'w') as f:
        f.create_dataset('nn-segs', data=segs, chunks=(1, 9, 11), compression='gzip', compression_opts=9)
        f.create_dataset('nn-heats', data=heats, chunks=(1, 1, 9, 11), compression='gzip', compression_opts=9)
        f.create_dataset('times', data=np.arange(3, dtype=np.float64))
        g = f.create_group('land-names')
        g['num-lands'] = np.int64(2)
        g['land-00'] = 'FH-l'
    cleaned = np.where(segs == 3, 0, segs).astype(np.uint8)
    args = argparse.Namespace(seg_file=path, out_file=None, out_group='nn-segs-clean')
    clean_segs._write(args, cleaned)
    clean_segs._write(args, cleaned)                           # again: the old 'nn-segs-clean' is replaced, not doubled
    with h5lite.File(path, 'r') as f:
        assert sorted(f.keys()) == ['land-names', 'nn-heats', 'nn-segs', 'nn-segs-clean', 'times']
        assert np.array_equal(f['nn-segs'][...], segs) and f['nn-segs'].dtype == np.uint8
        assert f['nn-segs']._layout[2] == (1, 9, 11) and f['nn-segs']._filters == [(1, (9,))]
        assert np.array_equal(f['nn-heats'][...], heats) and f['nn-heats'].dtype == np.float32
        assert f['nn-heats']._layout[2] == (1, 1, 9, 11)
        assert np.array_equal(f['times'][...], np.arange(3.0)) and f['times'].dtype == np.float64
        assert int(f['land-names/num-lands'][()]) == 2 and f['land-names/land-00'][()] == b'FH-l'
        new = f['nn-segs-clean']
        assert np.array_equal(new[...], cleaned) and new.dtype == np.uint8 and new.shape == segs.shape
        assert new._layout[2] == (1, 9, 11) and new._filters == [(1, (9,))]
    other = str(tmp_path / 'other.h5')
    clean_segs._write(argparse.Namespace(seg_file=path, out_file=other, out_group='nn-segs-clean'), cleaned)
    with h5lite.File(other, 'r') as f:
        assert f.keys() == ['nn-segs-clean'] and np.array_equal(f['nn-segs-clean'][...], cleaned)
    npz = str(tmp_path / 'out.npz')
    np.savez(npz, **{'nn-segs': segs})
    clean_segs._write(argparse.Namespace(seg_file=npz, out_file=None, out_group='nn-segs-clean'), cleaned)
    z = np.load(npz)
    assert sorted(z.files) == ['nn-segs', 'nn-segs-clean'] and np.array_equal(z['nn-segs-clean'], cleaned)


def test_header_declares_the_label_entries_and_the_binding_follows():
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dfl_hip.h')).read(), flags=re.S)
    at = [re.search(r'\b%s\s*\(' % f, hdr) for f in ENTRIES]
    assert all(at) and [m.start() for m in at] == sorted(m.start() for m in at)
    assert hdr.index('dfl_hard_dice') < at[0].start() < hdr.index('dfl_overlay_batch')     # after the landmark and Dice section
    first = nat.EXPORTS.index(ENTRIES[0])
    assert nat.EXPORTS[first:first + len(ENTRIES)] == ENTRIES
    assert max(v for k, v in vars(nat).items() if k.startswith('OP_') and isinstance(v, int)) == 24     # no new op kind
    from dfl_amd import labels
    assert labels.TILE == (nat.LABEL_TILE_H, nat.LABEL_TILE_W)
    assert dfl_amd.labels is labels and 'labels' in dfl_amd.__all__
    L = nat.lib()
    import ctypes as C
    assert L.dfl_label_dilate.argtypes == [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_int32, C.c_void_p,
                                           C.c_void_p]


def test_label_entries_check_their_arguments_before_any_launch():
    """No GPU is touched: every case is refused on the host (null pointers throughout)."""
    L = nat.lib()
    E = nat.ERR_INVALID_ARG
    assert L.dfl_label_components(None, 1, 8, 8, 5, None, None, None, None) == E
    assert b'connectivity 5' in L.dfl_last_error()
    assert L.dfl_label_components(None, 1, 65536, 32768, 8, None, None, None, None) == E
    assert b'32-bit flat index' in L.dfl_last_error()
    assert L.dfl_label_components(None, 1, 8, 8, 8, None, None, None, None) == E          # in range: the null pointers
    assert b'missing pointer' in L.dfl_last_error()
    for C_ in (1, 32):
        assert L.dfl_label_select(None, None, None, None, 1, 8, 8, C_, 1, 0, 0, None, None, None, None) == E
        assert b'num_classes' in L.dfl_last_error()
        assert L.dfl_label_select_scratch_bytes(1, C_) == E
    assert L.dfl_label_select_scratch_bytes(3, 7) == 3 * 7 * 8
    assert L.dfl_label_select(None, None, None, None, 1, 65536, 32768, 7, 1, 0, 0, None, None, None, None) == E
    assert L.dfl_label_select(None, None, None, None, 1, 8, 8, 7, 2, 0, 0, None, None, None, None) == E
    assert L.dfl_label_dilate(None, 1, 8, 8, 2, 33, None, None) == E
    assert b'radius 33' in L.dfl_last_error()
    assert L.dfl_label_dilate(None, 1, 65536, 32768, 2, 1, None, None) == E
    assert L.dfl_label_dilate(None, 0, 8, 8, 2, 1, None, None) == E
