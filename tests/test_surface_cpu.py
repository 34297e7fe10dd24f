"""The boundary distances without a GPU: the numpy restatement (surface_ref.py) against scipy.ndimage and numpy's own
max / percentile / mean, the known answer of the shifted rectangle, the command line of compute_surface_dist_on_test.py, and
the C ABI entries in the header with their host-side refusals."""
import ctypes as C
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
from dfl_amd import _native as nat  # noqa: E402
import compute_surface_dist_on_test as tool  # noqa: E402
import labels_ref as LR  # noqa: E402
import surface_ref as SR  # noqa: E402

TILE = (8, 16)
SHAPES = LR.shapes(TILE) + [(11, 13)]
SETS = [(1,), (2,), (1, 4), (3, 5, 9)]
ENTRIES = ['dfl_label_edt', 'dfl_label_surface_scratch_bytes', 'dfl_label_surface_stats', 'dfl_label_surface_select']


@pytest.mark.parametrize('name', list(LR.PATTERNS))
def test_restatement_agrees_with_scipy_edt_and_erosion(name):
    ndi = pytest.importorskip('scipy.ndimage')
    four = ndi.generate_binary_structure(2, 1)
    for H, W in SHAPES:
        seg = LR.pattern(name, H, W, TILE)
        for labels in SETS:
            mask = np.isin(seg, labels)
            edge = mask & ~ndi.binary_erosion(mask, structure=four, border_value=0)
            assert np.array_equal(SR.sites(seg, labels, False), mask)
            assert np.array_equal(SR.sites(seg, labels, True), edge), (name, H, W, labels)
            for boundary, site in ((False, mask), (True, edge)):
                got = SR.edt(seg, labels, boundary)
                assert got.dtype == np.int32
                if not site.any():
                    assert (got == SR.NONE).all()
                    continue
                # scipy measures to the nearest ZERO of its input; the squares of its float64 distances round to the integers
                want = np.rint(ndi.distance_transform_edt(~site) ** 2).astype(np.int64)
                assert np.array_equal(got, want), (name, H, W, labels, boundary)


def test_sites_never_hold_values_beyond_31():
    seg = np.array([[40, 40, 1], [40, 8, 1]], dtype=np.uint8)
    assert not SR.sites(seg, (40,), False).any() and (SR.edt(seg, (40,), False) == SR.NONE).all()
    assert np.array_equal(SR.edt(seg, (8, 40), False), [[2, 1, 2], [1, 0, 1]])


def _pairs():
    """(est, gt) images on which every label of 1..6 occurs in some pair: blobs against differently seeded blobs, and
    patterns against each other."""
    blobs_a, blobs_b = LR.blobs(2, 37, 45, seed=3), LR.blobs(2, 37, 45, seed=4)
    out = [(blobs_a[k], blobs_b[k]) for k in range(2)]
    out.append((LR.pattern('random_sparse', 23, 31, TILE), LR.pattern('random_dense', 23, 31, TILE)))
    out.append((LR.pattern('two_u', 23, 31, TILE), LR.pattern('comb', 23, 31, TILE)))
    return out


@pytest.mark.parametrize('percentile', [0.0, 50.0, 95.0, 100.0])
def test_restatement_metrics_agree_with_numpy_on_scipy_distances(percentile):
    ndi = pytest.importorskip('scipy.ndimage')
    four = ndi.generate_binary_structure(2, 1)
    seen = 0
    for est, gt in _pairs():
        got = SR.metrics(est, gt, LR.NUM_CLASSES, spacing=0.7, percentile=percentile)
        for l in range(1, LR.NUM_CLASSES):
            e = (est == l) & ~ndi.binary_erosion(est == l, structure=four, border_value=0)
            g = (gt == l) & ~ndi.binary_erosion(gt == l, structure=four, border_value=0)
            assert got['n_est'][l - 1] == e.sum() and got['n_gt'][l - 1] == g.sum()
            if not e.any() or not g.any():
                want = 0.0 if not e.any() and not g.any() else np.inf
                assert got['hd'][l - 1] == want and got['hdp'][l - 1] == want and got['assd'][l - 1] == want
                continue
            seen += 1
            d0 = ndi.distance_transform_edt(~g)[e]
            d1 = ndi.distance_transform_edt(~e)[g]
            both = np.concatenate([d0, d1])
            assert got['hd'][l - 1] == pytest.approx(0.7 * both.max(), rel=1e-12)
            assert got['hdp'][l - 1] == pytest.approx(0.7 * np.percentile(both, percentile), rel=1e-12, abs=1e-300)
            assert got['assd'][l - 1] == pytest.approx(0.7 * (d0.mean() + d1.mean()) / 2.0, rel=1e-12)
            assert got['mean_est_to_gt'][l - 1] == pytest.approx(0.7 * d0.mean(), rel=1e-12)
            assert got['mean_gt_to_est'][l - 1] == pytest.approx(0.7 * d1.mean(), rel=1e-12)
    assert seen >= 12


def test_shifted_rectangle_known_answer():
    est, gt = SR.shifted_rectangles()
    assert int((gt == 1).sum()) == 15 * 24 and np.array_equal(np.argwhere(est == 1) - np.argwhere(gt == 1), np.full((360, 2), (3, 4)))
    m = SR.metrics(est, gt, 2)
    assert m['n_est'][0] == 74 and m['n_gt'][0] == 74
    assert m['hd'][0] == 5.0
    assert m['hdp'][0] == pytest.approx(4.08001865665148, rel=1e-13)
    assert m['assd'][0] == pytest.approx(3.1027798811266067, rel=1e-13)
    n, max2, total = SR.stats(est, gt, 2)
    assert n.tolist() == [[74, 74]] and max2.tolist() == [[25, 25]]
    assert SR.kth2(est, gt, 1, 147) == 25 and SR.kth2(est, gt, 1, 148) == -1 and SR.kth2(est, gt, 1, -1) == -1


def test_tool_parser():
    p = tool.build_parser()
    positional = [a.dest for a in p._actions if not a.option_strings]
    assert positional == ['ds_path', 'seg_file', 'seg_group', 'csv_out', 'pat_ind']
    import compute_actual_dice_on_test as dice_tool
    assert positional == [a.dest for a in dice_tool.build_parser()._actions if not a.option_strings]
    args = p.parse_args(['data.h5', 'out.h5', 'nn-segs', 'dist.csv', '4'])
    assert vars(args) == dict(ds_path='data.h5', seg_file='out.h5', seg_group='nn-segs', csv_out='dist.csv', pat_ind=4,
                              no_hdr=False, num_classes=7, pixel_mm=1.0, percentile=95.0)
    args = p.parse_args(['d', 's', 'g', 'c', '2', '--no-hdr', '--num-classes', '5', '--pixel-mm', '0.194', '--percentile', '90'])
    assert (args.no_hdr, args.num_classes, args.pixel_mm, args.percentile) == (True, 5, 0.194, 90.0)
    assert tool.header(95.0) == 'pat,proj,label,hd,hd95,assd'
    assert tool.header(90.0) == 'pat,proj,label,hd,hd90,assd' and tool.header(99.5) == 'pat,proj,label,hd,hd99.5,assd'
    with pytest.raises(SystemExit):
        p.parse_args(['d', 's', 'g', 'c', 'four'])


def test_tool_and_module_refuse_to_run_without_a_gpu(monkeypatch, tmp_path):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(nat.DflError, match='no GPU'):
        tool.main([str(tmp_path / 'missing.h5'), str(tmp_path / 'missing2.h5'), 'nn-segs', str(tmp_path / 'o.csv'), '1'])
    assert not os.path.exists(str(tmp_path / 'o.csv'))
    from dfl_amd import labels
    host = torch.zeros((4, 4), dtype=torch.uint8)
    for call in (lambda: labels.edt(host, 1), lambda: labels.surface_distances(host, host)):
        with pytest.raises(nat.DflError, match='on the GPU'):
            call()
    assert 'edt' in labels.__all__ and 'surface_distances' in labels.__all__
    assert labels.SURFACE_CHUNK_BYTES == 256 * 1024 * 1024
    assert 'r * r' in labels.edt.__doc__ and 'bone_mask' in labels.edt.__doc__


def test_label_set_arguments_of_edt():
    from dfl_amd import labels
    assert labels._label_sets(3, 'edt') == ([8], False)
    assert labels._label_sets((1, 4), 'edt') == ([0b10010], False)
    assert labels._label_sets([[1], (2, 5), [31]], 'edt') == ([2, 0b100100, 1 << 31], True)
    assert labels._label_sets([[0]], 'edt') == ([1], True)
    for bad in (32, -1, True, (), [1, 32], [[1], 2], [[1], []], [[1, 40]], 1.5, [[l] for l in range(32)]):
        with pytest.raises(nat.DflError):
            labels._label_sets(bad, 'edt')


def test_header_declares_the_distance_entries_and_the_binding_follows():
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dfl_hip.h')).read(), flags=re.S)
    at = [re.search(r'\b%s\s*\(' % f, hdr).start() for f in ENTRIES]
    assert at == sorted(at)
    assert re.search(r'\bdfl_label_dilate\s*\(', hdr).start() < at[0] and at[-1] < hdr.index('dfl_overlay_batch')
    first = nat.EXPORTS.index('dfl_label_dilate') + 1          # directly after the four clean-up entries, in header order
    assert nat.EXPORTS[first:first + len(ENTRIES)] == ENTRIES
    assert nat.EXPORTS[first + len(ENTRIES)] == 'dfl_overlay_batch'
    L = nat.lib()
    for f in ENTRIES:
        assert getattr(L, f).restype is C.c_int, f
    assert nat.LABEL_EDT_NONE == 2147483647 == SR.NONE
    assert re.search(r'^#define DFL_LABEL_EDT_NONE \d+$', hdr, re.M)
    assert max(v for k, v in vars(nat).items() if k.startswith('OP_') and isinstance(v, int)) == 24     # no new op kind
    assert L.dfl_label_edt.argtypes == [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                        C.c_void_p, C.c_void_p, C.c_void_p]


def test_distance_entries_check_their_arguments_before_any_launch():
    """No GPU is touched: every case is refused on the host (null pointers throughout)."""
    L = nat.lib()
    E = nat.ERR_INVALID_ARG
    err = L.dfl_last_error

    def edt(B=1, H=8, W=8, S=1, boundary=0):
        return L.dfl_label_edt(None, B, H, W, None, S, boundary, None, None, None)
    for kw in (dict(B=0), dict(H=0), dict(W=-1)):
        assert edt(**kw) == E and b'bad sizes' in err()
    # (H-1)^2 + (W-1)^2 >= 2^31 - 1 is refused before anything else: 46341^2 alone, and 32769^2 twice (= 2^31 + 2^17 + 2)
    assert edt(H=46342, W=1, S=0) == E and b'squared distance' in err()
    assert edt(H=32770, W=32770, boundary=7) == E and b'squared distance' in err()
    assert edt(H=46341, W=1, S=0) == E and b'label sets' in err()          # 46340^2 < 2^31 - 1: the shape passes
    for S in (0, 32):
        assert edt(S=S) == E and b'label sets' in err()
    for boundary in (-1, 2):
        assert edt(boundary=boundary) == E and b'boundary' in err()
    assert edt() == E and b'missing pointer' in err()
    words = (C.c_uint32 * 1)(2)
    assert L.dfl_label_edt(None, 1, 8, 8, C.addressof(words), 1, 1, None, None, None) == E and b'missing pointer' in err()

    assert L.dfl_label_surface_scratch_bytes(0, 8, 8, 7) == E and b'bad sizes' in err()
    assert L.dfl_label_surface_scratch_bytes(1, 46342, 1, 7) == E and b'squared distance' in err()
    for C_ in (1, 32):
        assert L.dfl_label_surface_scratch_bytes(1, 8, 8, C_) == E and b'num_classes' in err()
    assert L.dfl_label_surface_scratch_bytes(1 << 20, 8, 8, 31) == E and b'more than an int' in err()
    # the larger of: one record of (C-1) * 2 doubles per 1024 pixels of an image; 256 bins and two state words per (b, l, j)
    assert L.dfl_label_surface_scratch_bytes(3, 180, 180, 7) == max(3 * 32 * 12 * 8, 3 * 12 * (1024 + 8))
    assert L.dfl_label_surface_scratch_bytes(1, 1440, 1440, 7) == max(2025 * 12 * 8, 12 * (1024 + 8))
    assert L.dfl_label_surface_scratch_bytes(1, 1, 1, 2) == 2 * (1024 + 8)

    def stats(B=1, H=8, W=8, C_=7):
        return L.dfl_label_surface_stats(None, None, B, H, W, C_, None, None, None, None, None, None, None)

    def select(B=1, H=8, W=8, C_=7):
        return L.dfl_label_surface_select(None, None, B, H, W, C_, None, None, None, None, None, None)
    for call, name in ((stats, b'dfl_label_surface_stats'), (select, b'dfl_label_surface_select')):
        assert call(B=0) == E and b'bad sizes' in err() and name in err()
        assert call(H=46342, W=1) == E and b'squared distance' in err()
        for C_ in (1, 32):
            assert call(C_=C_) == E and b'num_classes' in err()
        assert call(B=1 << 20, C_=31) == E and b'too large' in err()
        assert call() == E and b'missing pointer' in err() and name in err()
