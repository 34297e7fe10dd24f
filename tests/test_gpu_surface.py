"""The boundary distances on the GPU against their numpy restatement (surface_ref.py): dfl_label_edt bit for bit,
dfl_label_surface_stats and dfl_label_surface_select through their C entries (counts, maxima and order statistics exactly, the
sums within the rounding of a float64 sum), labels.surface_distances against numpy's max / percentile / mean, and
compute_surface_dist_on_test.py end to end.  Every call is made twice and must give the same bytes."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, h5lite, labels  # noqa: E402
import labels_ref as LR  # noqa: E402
import surface_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = labels.TILE
SHAPES = LR.shapes(TILE)
THREE = [(2,), (1, 4), (3, 5, 9)]
C7 = LR.NUM_CLASSES
KEYS = ('hd', 'hdp', 'assd', 'mean_est_to_gt', 'mean_gt_to_est', 'n_est', 'n_gt')


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda', torch.cuda.current_device())


def _np(x):
    if isinstance(x, dict):
        return {k: _np(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return tuple(_np(v) for v in x)
    return x.cpu().numpy() if torch.is_tensor(x) else x


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _twice(fn):
    """fn() run twice on the same input: the results as numpy, identical bytes required."""
    first, second = _np(fn()), _np(fn())
    assert _same(first, second), 'two runs on the same input differ'
    return first


def _put(a, dev):
    return torch.from_numpy(np.array(a, order='C')).to(dev)        # (a copy: the patterns are read-only)


def check_edt(segs_np, dev):
    """labels.edt of a uint8 [B, H, W] stack against the restatement: boundary off and on, one set and three sets at once."""
    segs = _put(segs_np, dev)
    for boundary in (False, True):
        one = _twice(lambda: labels.edt(segs, 1, boundary))
        assert one.dtype == np.int32 and one.shape == segs_np.shape
        assert np.array_equal(one, SR.edt_stack(segs_np, [(1,)], boundary)[:, 0]), boundary
        three = _twice(lambda: labels.edt(segs, THREE, boundary))
        assert three.dtype == np.int32 and three.shape == (segs_np.shape[0], 3) + segs_np.shape[1:]
        assert np.array_equal(three, SR.edt_stack(segs_np, THREE, boundary)), boundary


@pytest.mark.parametrize('H,W', SHAPES)
@pytest.mark.parametrize('name', list(LR.PATTERNS))
def test_edt_pattern(name, H, W):
    check_edt(LR.pattern(name, H, W, TILE)[None], _dev())


def _one_site(H, W, r, c, label=1):
    img = np.zeros((H, W), dtype=np.uint8)
    img[r, c] = label
    return img


@pytest.mark.parametrize('corner', [(0, 0), (0, -1), (-1, 0), (-1, -1)])
def test_edt_single_site_in_a_corner_the_search_runs_its_full_length(corner):
    dev = _dev()
    H, W = 203, 131                       # rows beyond the tile's LDS window in both directions, columns in three tiles
    img = _one_site(H, W, *corner)
    r, c = np.mgrid[0:H, 0:W]
    want = ((r - corner[0] % H) ** 2 + (c - corner[1] % W) ** 2).astype(np.int32)
    for boundary in (False, True):
        got = _twice(lambda: labels.edt(_put(img, dev), 1, boundary))
        assert np.array_equal(got, want) and np.array_equal(got, SR.edt(img, (1,), boundary))


def test_edt_no_site_and_nothing_leaks_across_a_batch():
    dev = _dev()
    H, W = 70, 90
    assert nat.LABEL_EDT_NONE == SR.NONE == 2 ** 31 - 1
    none = _twice(lambda: labels.edt(_put(np.zeros((2, H, W), dtype=np.uint8), dev), [(1,), (0, 2)]))
    assert (none[:, 0] == SR.NONE).all() and (none[:, 1] == 0).all()
    # a site in the last row of the middle image only: were the batch one tall image, the first row of the next image
    # would be at distance 1 and the last row of the one before at distance H
    stack = np.zeros((3, H, W), dtype=np.uint8)
    stack[1, H - 1, 40] = 1
    stack[1, 0, 3] = 1
    for boundary in (False, True):
        got = _twice(lambda: labels.edt(_put(stack, dev), (1, 5), boundary))
        assert (got[0] == SR.NONE).all() and (got[2] == SR.NONE).all()
        assert np.array_equal(got, SR.edt_stack(stack, [(1, 5)], boundary)[:, 0])
    # values of 32 and more are in no set, whatever the word says
    big = np.full((1, 9, 9), 40, dtype=np.uint8)
    assert (_np(labels.edt(_put(big, dev), [[8]])) == SR.NONE).all()


@pytest.mark.parametrize('which', ['first', 'last'])
def test_edt_sites_only_in_the_first_or_the_last_row(which):
    dev = _dev()
    H, W = 157, 75
    img = np.zeros((H, W), dtype=np.uint8)
    img[0 if which == 'first' else H - 1, ::7] = 3
    img[0 if which == 'first' else H - 1, 70:] = 3
    for boundary in (False, True):
        got = _twice(lambda: labels.edt(_put(img, dev), (3,), boundary))
        assert np.array_equal(got, SR.edt(img, (3,), boundary))


@pytest.mark.parametrize('shape', [(1, 4200), (4200, 1)])
def test_edt_and_select_with_all_four_key_bytes_live(shape):
    """One site at the far end of a 4200-pixel row or column: d^2 reaches 4199^2 > 2^24."""
    dev = _dev()
    H, W = shape
    gt = _one_site(H, W, H - 1, W - 1)
    got = _twice(lambda: labels.edt(_put(gt, dev), 1, True))
    want = (np.arange(4199, -1, -1, dtype=np.int64) ** 2).astype(np.int32).reshape(H, W)
    assert np.array_equal(got, want) and np.array_equal(got, SR.edt(gt, (1,), True))
    # est: a line of label 1 from the other end, so that its boundary pixels are the far ones; keys up to 4199^2
    est = np.zeros((H, W), dtype=np.uint8)
    est.reshape(-1)[:3000] = 1
    n, max2, total, kth2 = _raw(est[None], gt[None], 2, lambda N: np.stack([N - 1, N // 2], -1), dev)
    assert n.tolist() == [[[3000, 1]]] and max2.tolist() == [[[4199 ** 2, 1200 ** 2]]]
    assert kth2[0, 0, 0] == 4199 ** 2 == SR.kth2(est, gt, 1, 3000) and kth2[0, 0, 1] == SR.kth2(est, gt, 1, 3001 // 2)
    assert 4199 ** 2 > 2 ** 24


# ---- the C entries of the statistics, called as labels.surface_distances calls them ----------------------------------------
def _raw(est_np, gt_np, C, ranks_of, dev):
    """-> (n, max2, sum, kth2) as numpy, each [B, C-1, 2]; ranks_of(N [B, C-1]) -> the int ranks [B, C-1, 2] to select."""
    def run():
        e, g = _put(est_np, dev), _put(gt_np, dev)
        B, H, W = e.shape
        L = nat.lib()
        words = [1 << l for l in range(1, C)]
        d2g, d2e = labels._edt(g, words, True), labels._edt(e, words, True)
        nbytes = nat.check(L.dfl_label_surface_scratch_bytes(B, H, W, C))
        scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
        n = torch.full((B, C - 1, 2), -7, dtype=torch.int32, device=dev)
        max2 = torch.full_like(n, -7)
        total = torch.full((B, C - 1, 2), -7.0, dtype=torch.float64, device=dev)
        s = torch.cuda.current_stream().cuda_stream
        nat.check(L.dfl_label_surface_stats(e.data_ptr(), g.data_ptr(), B, H, W, C, d2g.data_ptr(), d2e.data_ptr(), n.data_ptr(),
                                            max2.data_ptr(), total.data_ptr(), scratch.data_ptr(), s), 'dfl_label_surface_stats')
        ranks = _put(np.asarray(ranks_of(n.cpu().numpy().sum(-1).astype(np.int64))).astype(np.int32), dev)
        assert ranks.shape == n.shape
        kth2 = torch.full_like(n, -7)
        nat.check(L.dfl_label_surface_select(e.data_ptr(), g.data_ptr(), B, H, W, C, d2g.data_ptr(), d2e.data_ptr(),
                                             ranks.data_ptr(), kth2.data_ptr(), scratch.data_ptr(), s), 'dfl_label_surface_select')
        return n, max2, total, kth2, ranks
    n, max2, total, kth2, ranks = _twice(run)
    # against the restatement: counts, maxima and order statistics exactly, the sums within the rounding of a sum
    for b in range(est_np.shape[0]):
        rn, rmax2, rsum = SR.stats(est_np[b], gt_np[b], C)
        assert np.array_equal(n[b], rn), ('n', b, n[b], rn)
        assert np.array_equal(max2[b], rmax2), ('max2', b, max2[b], rmax2)
        # (n + 2) * 2^-53 relative: the worst case of any order of summation of n non-negative correctly rounded terms
        bound = (rn + 2) * 2.0 ** -53 * rsum
        print('sum: image %d, largest |device - numpy| / bound = %.3f' % (b, float((np.abs(total[b] - rsum) / np.maximum(bound, 1e-300)).max())))
        assert (np.abs(total[b] - rsum) <= bound).all(), ('sum', b, total[b], rsum)
        for l in range(1, C):
            for j in range(2):
                assert kth2[b, l - 1, j] == SR.kth2(est_np[b], gt_np[b], l, int(ranks[b, l - 1, j])), ('kth2', b, l, j)
    return n, max2, total, kth2


def check_surface(est_np, gt_np, dev, C=C7, spacing=1.0, percentile=95.0):
    """labels.surface_distances of a stack against numpy's max / percentile / mean of the restatement's distances."""
    got = _twice(lambda: labels.surface_distances(_put(est_np, dev), _put(gt_np, dev), num_classes=C, spacing=spacing,
                                                  percentile=percentile))
    B = est_np.shape[0]
    assert sorted(got) == sorted(KEYS)
    for k in KEYS:
        assert got[k].shape == (B, C - 1) and got[k].dtype == (np.int32 if k.startswith('n_') else np.float64), k
    for b in range(B):
        rn, rmax2, _ = SR.stats(est_np[b], gt_np[b], C)
        assert np.array_equal(got['n_est'][b], rn[:, 0]) and np.array_equal(got['n_gt'][b], rn[:, 1])
        for l in range(1, C):
            d0, d1 = SR.distances(est_np[b], gt_np[b], l)
            mine = {k: got[k][b, l - 1] for k in KEYS[:5]}
            if d0.size == 0 or d1.size == 0:
                want = 0.0 if d0.size == d1.size else np.inf
                assert all(v == want for v in mine.values()), (b, l, mine)
                continue
            both = np.concatenate([d0, d1])
            assert mine['hd'] == np.sqrt(np.float64(rmax2[l - 1].max())) * spacing, (b, l)
            want = {'hdp': np.percentile(both, percentile) * spacing, 'assd': (d0.mean() + d1.mean()) / 2.0 * spacing,
                    'mean_est_to_gt': d0.mean() * spacing, 'mean_gt_to_est': d1.mean() * spacing}
            for k, w in want.items():
                assert abs(mine[k] - w) <= 1e-12 * abs(w), (k, b, l, mine[k], w)
    ref = SR.metrics_stack(est_np, gt_np, C, spacing, percentile)
    for k in KEYS[:5]:
        fin = np.isfinite(ref[k])
        assert np.array_equal(np.isfinite(got[k]), fin) and np.allclose(got[k][fin], ref[k][fin], rtol=1e-12, atol=0.0), k
    return got


def _stack():
    """[4, 180, 180] of blobs as ground truth and a perturbed copy as the estimate: shifted, speckled, one label wiped out of
    one image of the estimate and one out of both maps of another."""
    gt = LR.blobs(4, 180, 180).copy()
    est = np.roll(gt, (2, -1), axis=(1, 2))
    rng = np.random.default_rng(21)
    noise = rng.random(est.shape)
    est[noise < 0.004] = rng.integers(0, C7, size=int((noise < 0.004).sum()))
    est[0][est[0] == 6] = 0
    est[1][est[1] == 5] = 0
    gt[1][gt[1] == 5] = 0
    gt[2][gt[2] == 2] = 0
    return est, gt


def test_surface_identical_maps_give_zeros():
    dev = _dev()
    seg = LR.blobs(2, 45, 70, seed=9)
    got = check_surface(seg, seg, dev)
    for k in KEYS[:5]:
        assert (got[k] == 0.0).all(), k
    assert np.array_equal(got['n_est'], got['n_gt']) and got['n_est'].sum() > 0


def test_surface_label_absent_in_est_in_gt_and_in_both():
    dev = _dev()
    H, W = 40, 50
    est = np.zeros((1, H, W), dtype=np.uint8)
    gt = np.zeros_like(est)
    est[0, 5:12, 5:12], gt[0, 6:12, 4:12] = 1, 1          # in both
    gt[0, 20:25, 20:30] = 2                               # absent in est
    est[0, 30:33, 30:41] = 3                              # absent in gt
    got = check_surface(est, gt, dev, C=5)                # label 4: absent in both
    assert np.isfinite(got['hd'][0, 0]) and got['hd'][0, 0] > 0
    for k in ('hd', 'hdp', 'assd'):
        assert got[k][0, 1] == np.inf and got[k][0, 2] == np.inf and got[k][0, 3] == 0.0
    assert got['n_est'][0].tolist() == [24, 0, 24, 0] and got['n_gt'][0].tolist() == [24, 26, 0, 0]
    n, max2, total, kth2 = _raw(est, gt, 5, lambda N: np.stack([N - 1, N], -1), dev)
    assert max2[0, 1:].tolist() == [[0, 0]] * 3 and total[0, 1:].tolist() == [[0.0, 0.0]] * 3
    # the union of a label that one map lacks holds NONE for every boundary pixel of the other; rank N is beyond every union
    assert kth2[0, :, 0].tolist() == [max2[0, 0].max(), SR.NONE, SR.NONE, -1] and (kth2[0, :, 1] == -1).all()


def test_surface_shifted_rectangle_known_answer():
    dev = _dev()
    est, gt = SR.shifted_rectangles()
    got = check_surface(est[None], gt[None], dev, C=2)
    assert got['n_est'][0, 0] == 74 and got['n_gt'][0, 0] == 74 and got['hd'][0, 0] == 5.0
    assert abs(got['hdp'][0, 0] - 4.08001865665148) <= 1e-12 * 4.08001865665148
    assert abs(got['assd'][0, 0] - 3.1027798811266067) <= 1e-12 * 3.1027798811266067
    two_d = _np(labels.surface_distances(_put(est, dev), _put(gt, dev), num_classes=2, spacing=0.5))
    assert all(two_d[k].shape == (1,) for k in KEYS) and two_d['hd'][0] == 2.5 and two_d['n_est'][0] == 74
    _raw(est[None], gt[None], 2, lambda N: np.stack([N // 2, np.full_like(N, -1)], -1), dev)


def test_surface_label_touching_the_image_border():
    dev = _dev()
    H, W = 33, 70
    est = np.zeros((1, H, W), dtype=np.uint8)
    gt = np.zeros_like(est)
    gt[0, 0:9, 0:20], est[0, 0:12, 0:17] = 1, 1           # in the corner: the image border is boundary in both
    gt[0, 20:, 60:], est[0, 22:, 58:] = 2, 2
    gt[0, :, 40], est[0, :, 42] = 3, 3                    # a full column, border at both ends
    check_surface(est, gt, dev, C=4)
    _raw(est, gt, 4, lambda N: np.stack([np.zeros_like(N), N - 1], -1), dev)


def test_surface_union_of_one_and_all_keys_equal():
    dev = _dev()
    est = _one_site(20, 20, 5, 5)[None]
    none = np.zeros_like(est)
    # N == 1: one boundary pixel in est, none in gt
    got = check_surface(est, none, dev, C=2)
    assert got['hd'][0, 0] == np.inf and got['n_est'][0, 0] == 1 and got['n_gt'][0, 0] == 0
    n, max2, total, kth2 = _raw(est, none, 2, lambda N: np.stack([N - 1, N], -1), dev)
    assert n.tolist() == [[[1, 0]]] and kth2.tolist() == [[[SR.NONE, -1]]]
    # all keys equal: one pixel each, 3 apart: both directions hold the one distance 3
    gt = _one_site(20, 20, 5, 8)[None]
    for p in (0.0, 50.0, 95.0, 100.0):
        got = check_surface(est, gt, dev, C=2, percentile=p)
        assert got['hd'][0, 0] == 3.0 and got['hdp'][0, 0] == 3.0 and got['assd'][0, 0] == 3.0
    n, max2, total, kth2 = _raw(est, gt, 2, lambda N: np.stack([np.zeros_like(N), N - 1], -1), dev)
    assert kth2.tolist() == [[[9, 9]]] and total.tolist() == [[[3.0, 3.0]]]


@pytest.mark.parametrize('percentile', [0.0, 50.0, 95.0, 100.0])
def test_surface_percentiles(percentile):
    dev = _dev()
    est, gt = _stack()
    check_surface(est[:1, :90, :120], gt[:1, :90, :120], dev, spacing=0.194, percentile=percentile)


def test_surface_realistic_stack_of_blobs():
    dev = _dev()
    est, gt = _stack()
    got = check_surface(est, gt, dev)
    assert got['hd'][0, 5] == np.inf and got['hd'][2, 1] == np.inf and got['hd'][1, 4] == 0.0
    assert np.isfinite(got['hd']).sum() >= 4 * 6 - 3
    _raw(est, gt, C7, lambda N: np.stack([N // 2, np.floor(0.95 * np.maximum(N - 1, 0)).astype(np.int64)], -1), dev)
    check_edt(gt, dev)


def test_surface_in_three_chunks_gives_identical_bytes(monkeypatch):
    """The stack and one more image, five in all: at two images per chunk they go in three chunks, the last one short."""
    dev = _dev()
    est, gt = _stack()
    est, gt = np.concatenate([est, gt[:1]]), np.concatenate([gt, est[3:]])
    e, g = _put(est, dev), _put(gt, dev)
    whole = _np(labels.surface_distances(e, g))
    per_image = 3 * (C7 - 1) * 180 * 180 * 4
    assert labels.SURFACE_CHUNK_BYTES // per_image >= 5
    calls = []
    real = labels._surface_chunk
    monkeypatch.setattr(labels, '_surface_chunk', lambda e_, *a: calls.append(e_.shape[0]) or real(e_, *a))
    monkeypatch.setattr(labels, 'SURFACE_CHUNK_BYTES', 2 * per_image + 5)
    parts = _twice(lambda: labels.surface_distances(e, g))
    assert calls == [2, 2, 1] * 2
    assert _same(parts, whole)
    monkeypatch.setattr(labels, 'SURFACE_CHUNK_BYTES', 1)             # less than one image: one image per chunk
    assert _same(_np(labels.surface_distances(e, g)), whole) and calls[6:] == [1] * 5


def test_python_refusals():
    dev = _dev()
    seg = _put(LR.pattern('random_sparse', 20, 30, TILE), dev)
    for bad in (seg.float(), seg.cpu(), seg[None, None], seg[:0]):
        with pytest.raises(nat.DflError):
            labels.edt(bad, 1)
        with pytest.raises(nat.DflError):
            labels.surface_distances(bad, bad)
    for sets in (32, -1, (), [1, 32], [[1], 2], [[1], []], True):
        with pytest.raises(nat.DflError):
            labels.edt(seg, sets)
    with pytest.raises(nat.DflError):
        labels.edt(seg, 1, boundary=2)
    for kw in (dict(num_classes=1), dict(num_classes=32), dict(spacing=0.0), dict(percentile=101.0), dict(percentile=-1.0)):
        with pytest.raises(nat.DflError):
            labels.surface_distances(seg, seg, **kw)
    with pytest.raises(nat.DflError):
        labels.surface_distances(seg, seg[:10])
    # a view that is not contiguous is read as what it shows
    wide = _put(LR.pattern('random_dense', 20, 60, TILE), dev)
    assert np.array_equal(_np(labels.edt(wide[:, ::2], (2, 3))), SR.edt(np.ascontiguousarray(_np(wide)[:, ::2]), (2, 3), False))


def test_entries_refuse_bad_arguments():
    dev = _dev()
    L = nat.lib()
    E = nat.ERR_INVALID_ARG
    seg = torch.zeros((1, 8, 8), dtype=torch.uint8, device=dev)
    i32 = torch.zeros((4, 6, 8 * 8 + 1), dtype=torch.int32, device=dev)
    f64 = torch.zeros(64, dtype=torch.float64, device=dev)
    scratch = torch.zeros(4096, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    import ctypes
    words = (ctypes.c_uint32 * 1)(2)
    w = ctypes.addressof(words)
    a, b, c, d = (i32[k].data_ptr() for k in range(4))
    sp, fp, sc = seg.data_ptr(), f64.data_ptr(), scratch.data_ptr()
    for S, boundary in ((0, 0), (32, 1), (1, 2), (1, -1)):
        assert L.dfl_label_edt(sp, 1, 8, 8, w, S, boundary, a, b, s) == E
    assert L.dfl_label_edt(sp, 1, 8, 8, None, 1, 0, a, b, s) == E
    assert L.dfl_label_edt(sp, 0, 8, 8, w, 1, 0, a, b, s) == E
    assert L.dfl_label_edt(None, 1, 46342, 1, None, 1, 0, None, None, s) == E and b'squared distance' in L.dfl_last_error()
    for C_ in (1, 32):
        assert L.dfl_label_surface_stats(sp, sp, 1, 8, 8, C_, a, b, c, d, fp, sc, s) == E
        assert L.dfl_label_surface_select(sp, sp, 1, 8, 8, C_, a, b, c, d, sc, s) == E
    assert L.dfl_label_surface_stats(sp, sp, 1, 8, 8, 7, a, b, c, d, fp, None, s) == E
    assert L.dfl_label_surface_stats(sp, sp, 1, 8, 8, 7, a, b, c, d, fp, sc + 4, s) == E and b'aligned' in L.dfl_last_error()
    assert L.dfl_label_surface_select(sp, sp, 1, 8, 8, 7, a, b, None, d, sc, s) == E
    assert L.dfl_label_surface_select(sp, sp, 1, 8, 8, 7, a, b, c, d, sc + 4, s) == E and b'aligned' in L.dfl_last_error()
    assert L.dfl_label_surface_select(None, None, 1, 40000, 40000, 7, None, None, None, None, None, s) == E
    torch.cuda.synchronize()


def test_tool_end_to_end(tmp_path):
    _dev()
    import compute_surface_dist_on_test as tool
    est, gt = _stack()
    est, gt = np.ascontiguousarray(est[:3, :60, :80]), np.ascontiguousarray(gt[:3, :60, :80])
    est[0][est[0] == 6] = 0
    gt[0, 50:55, 60:70] = 6                                # label 6 of projection 0: in gt only
    data, out, csv = str(tmp_path / 'data.h5'), str(tmp_path / 'out.h5'), str(tmp_path / 'dist.csv')
    with h5lite.File(data, 'w') as f:
        f.create_dataset('04/segs', data=gt)
    with h5lite.File(out, 'w') as f:
        f.create_dataset('nn-segs', data=est, chunks=(1, 60, 80), compression='gzip', compression_opts=9)
    tool.main([data, out, 'nn-segs', csv, '4', '--pixel-mm', '0.5'])
    rows = open(csv).read().strip().split('\n')
    ref = SR.metrics_stack(est, gt, C7, spacing=0.5, percentile=95.0)
    assert rows[0] == 'pat,proj,label,hd,hd95,assd' and len(rows) == 1 + 3 * 6
    want = ['4,%d,%d,%.2f,%.2f,%.2f' % (p, l, ref['hd'][p, l - 1], ref['hdp'][p, l - 1], ref['assd'][p, l - 1])
            for p in range(3) for l in range(1, C7)]
    # two decimals of a value that sits on a rounding boundary could differ by the last float64 bit: none does here
    for k in ('hd', 'hdp', 'assd'):
        v = ref[k][np.isfinite(ref[k])] * 100.0
        assert (np.abs(v - np.floor(v) - 0.5) > 1e-9).all(), k
    assert rows[1:] == want
    assert rows[6] == '4,0,6,inf,inf,inf'
    tool.main([data, out, 'nn-segs', csv, '4', '--no-hdr', '--percentile', '50'])
    rows = open(csv).read().strip().split('\n')
    ref50 = SR.metrics_stack(est, gt, C7, percentile=50.0)
    assert len(rows) == 18 and rows[0] == '4,0,1,%.2f,%.2f,%.2f' % (ref50['hd'][0, 0], ref50['hdp'][0, 0], ref50['assd'][0, 0])
