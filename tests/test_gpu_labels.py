"""The label clean-up on the GPU against its numpy restatement (labels_ref.py), bit for bit: dfl_label_components,
dfl_label_select and dfl_label_dilate through dfl_amd.labels, and clean_segs.py end to end.  No tolerances anywhere: every
result is an exact integer and canonical, and every call is made twice and must give the same bytes."""
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

pytestmark = pytest.mark.gpu

TILE = labels.TILE
SHAPES = LR.shapes(TILE)
BIG = SHAPES[-1]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda', torch.cuda.current_device())


def _twice(fn):
    """fn() run twice on the same input: the results (tensors, or tuples / dicts of them) as numpy, identical bytes required."""
    def to_np(x):
        if isinstance(x, dict):
            return {k: to_np(v) for k, v in x.items()}
        if isinstance(x, (tuple, list)):
            return tuple(to_np(v) for v in x)
        return x.cpu().numpy()

    def same(a, b):
        if isinstance(a, dict):
            return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
        if isinstance(a, tuple):
            return len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    first, second = to_np(fn()), to_np(fn())
    assert same(first, second), 'two runs on the same input differ'
    return first


def check_stack(segs_np, dev):
    """Every check of the issue on one uint8 [B, H, W] stack."""
    B, H, W = segs_np.shape
    segs = torch.from_numpy(np.array(segs_np)).to(dev)
    for connectivity in (4, 8):
        root, area, info = _twice(lambda: labels.components(segs, connectivity))
        want = LR.components_stack(segs_np, connectivity)
        assert root.dtype == np.int32 and area.dtype == np.int32 and info.dtype == np.int32
        assert np.array_equal(root, want[0]), 'root, connectivity %d' % connectivity
        assert np.array_equal(area, want[1]), 'area, connectivity %d' % connectivity
        assert np.array_equal(info.view(np.uint32), want[2]), 'info, connectivity %d' % connectivity
        settings = [dict(keep=k, min_area=m) for k in ('largest', 'all') for m in (0, 5)]
        settings += [dict(fill_holes=f) for f in (4, H * W)]          # (fill_holes=0 with the defaults is the first setting)
        for kw in settings:
            out, stats = _twice(lambda: labels.clean(segs, connectivity=connectivity, **kw))
            ref_out, ref_stats = LR.clean(segs_np, connectivity=connectivity, **kw)
            assert out.dtype == np.uint8 and np.array_equal(out, ref_out), (connectivity, kw)
            for key in ('removed', 'filled'):
                assert stats[key].dtype == np.int32 and np.array_equal(stats[key], ref_stats[key]), (connectivity, kw, key)
    for which in ((2,), (1, 4)):
        for dilate in (0, 1, 3, 7):
            mask = _twice(lambda: labels.bone_mask(segs, which, dilate))
            want = np.stack([LR.dilate(s, which, dilate) for s in segs_np])
            assert mask.dtype == np.uint8 and np.array_equal(mask, want), (which, dilate)


@pytest.mark.parametrize('H,W', SHAPES)
@pytest.mark.parametrize('name', list(LR.PATTERNS))
def test_pattern(name, H, W):
    check_stack(LR.pattern(name, H, W, TILE)[None], _dev())


def test_batch_of_three_images_nothing_leaks_across():
    H, W = BIG
    # the comb fills its last row, the serpentine its first: were the batch one tall image, they would touch (both label 3 here)
    a = LR.pattern('comb', H, W, TILE)
    b = np.where(LR.pattern('serpentine', H, W, TILE) > 0, 3, 0).astype(np.uint8)
    c = LR.pattern('random_dense', H, W, TILE)
    assert (a[-1] == 3).all() and (b[0] == 3).all()
    check_stack(np.stack([a, b, c]), _dev())


def test_two_dimensional_input_and_the_mask_similarity_takes():
    dev = _dev()
    seg_np = LR.pattern('random_sparse', 37, 70, TILE)
    seg = torch.from_numpy(np.array(seg_np)).to(dev)
    root, area, info = labels.components(seg)
    want = LR.components(seg_np, 8)
    assert root.shape == (37, 70) and np.array_equal(root.cpu().numpy(), want[0]) and np.array_equal(area.cpu().numpy(), want[1])
    out, stats = labels.clean(seg, min_area=3, fill_holes=2)
    ref_out, ref_stats = LR.clean(seg_np[None], min_area=3, fill_holes=2)
    assert out.shape == (37, 70) and np.array_equal(out.cpu().numpy(), ref_out[0])
    assert stats['removed'].shape == (7,) and np.array_equal(stats['removed'].numpy(), ref_stats['removed'][0])
    assert np.array_equal(stats['filled'].numpy(), ref_stats['filled'][0])
    mask = labels.bone_mask(seg, 3, dilate=2)
    assert mask.shape == (37, 70) and mask.dtype == torch.uint8 and mask.is_contiguous()
    from dfl_amd import register
    register.Similarity(torch.rand(37, 70, device=dev), mask)            # the dtype and layout it takes
    # a view that is not contiguous is read as what it shows
    wide = torch.from_numpy(np.array(LR.pattern('random_dense', 37, 140, TILE))).to(dev)
    root2, _, _ = labels.components(wide[:, ::2], 4)
    assert np.array_equal(root2.cpu().numpy(), LR.components(np.ascontiguousarray(wide.cpu().numpy()[:, ::2]), 4)[0])
    for bad in (seg.float(), seg.cpu(), seg[None, None]):
        with pytest.raises(nat.DflError):
            labels.components(bad)
    for kw in (dict(connectivity=5), dict(keep='first'), dict(num_classes=1), dict(num_classes=32), dict(min_area=-1)):
        with pytest.raises(nat.DflError):
            labels.clean(seg, **kw)
    with pytest.raises(nat.DflError):
        labels.components(seg, connectivity=6)
    for args in ((32, 0), (1, 33), ((), 0)):
        with pytest.raises(nat.DflError):
            labels.bone_mask(seg, *args)


def test_realistic_stack_of_blobs():
    check_stack(LR.blobs(4, 180, 180), _dev())


def test_entries_refuse_bad_arguments():
    dev = _dev()
    L = nat.lib()
    E = nat.ERR_INVALID_ARG
    seg = torch.zeros((1, 8, 8), dtype=torch.uint8, device=dev)
    i32 = torch.zeros((3, 8, 8), dtype=torch.int32, device=dev)
    scratch = torch.zeros(64, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    r, a, i = (i32[k].data_ptr() for k in range(3))
    assert L.dfl_label_components(seg.data_ptr(), 1, 8, 8, 5, r, a, i, s) == E
    for C_ in (1, 32):
        assert L.dfl_label_select(seg.data_ptr(), r, a, i, 1, 8, 8, C_, 1, 0, 0, seg.data_ptr(), None, scratch.data_ptr(), s) == E
    assert L.dfl_label_dilate(seg.data_ptr(), 1, 8, 8, 2, 33, seg.data_ptr(), s) == E
    # H * W >= 2^31 with null pointers: refused before any launch
    assert L.dfl_label_components(None, 1, 65536, 32768, 8, None, None, None, s) == E
    assert L.dfl_label_select(None, None, None, None, 1, 46341, 46341, 7, 1, 0, 0, None, None, None, s) == E
    assert L.dfl_label_dilate(None, 1, 32768, 65536, 2, 1, None, s) == E
    torch.cuda.synchronize()


def test_clean_segs_end_to_end(tmp_path, capsys):
    _dev()
    import clean_segs
    import compute_actual_dice_on_test as dice_tool
    rng = np.random.default_rng(7)
    est = LR.blobs(5, 45, 70, seed=9)
    gt = LR.blobs(5, 45, 70, seed=10)
    heats = rng.random((5, 2, 45, 70)).astype(np.float32)
    data, out = str(tmp_path / 'data.h5'), str(tmp_path / 'out.h5')
    with h5lite.File(data, 'w') as f:
        f.create_dataset('04/segs', data=gt)
    with h5lite.File(out, 'w') as f:
        f.create_dataset('nn-segs', data=est, chunks=(1, 45, 70), compression='gzip', compression_opts=9)
        f.create_dataset('nn-heats', data=heats, chunks=(1, 1, 45, 70), compression='gzip', compression_opts=9)
    clean_segs.main([out, 'nn-segs', 'nn-segs-clean', '--min-area', '4', '--fill-holes', '3'])
    lines = capsys.readouterr().out.strip().split('\n')
    want, want_stats = LR.clean(est, min_area=4, fill_holes=3)
    stage1, _ = LR.clean(est, min_area=4)
    root, area, _ = LR.components_stack(est, 8)
    assert len(lines) == 6
    for l, line in zip(range(1, 7), lines):
        comps = int(((area > 0) & (est == l) & (stage1 == 0)).sum())
        assert line == 'label %d: %d components removed, %d pixels removed, %d pixels filled' % (
            l, comps, want_stats['removed'][:, l].sum(), want_stats['filled'][:, l].sum())
    assert want_stats['removed'].sum() > 0 and want_stats['filled'].sum() > 0          # the case exercises both stages
    with h5lite.File(out, 'r') as f:
        assert sorted(f.keys()) == ['nn-heats', 'nn-segs', 'nn-segs-clean']
        got = f['nn-segs-clean']
        assert got.shape == est.shape and got.dtype == np.uint8 and np.array_equal(got[...], want)
        assert f['nn-segs'][...].tobytes() == est.tobytes() and f['nn-heats'][...].tobytes() == heats.tobytes()
    for group in ('nn-segs-clean', 'nn-segs'):
        csv = str(tmp_path / (group + '.csv'))
        dice_tool.main([data, out, group, csv, '4'])
        rows = open(csv).read().strip().split('\n')
        assert rows[0] == 'pat,proj,label,dice' and len(rows) == 1 + 5 * 6
    other = str(tmp_path / 'other.h5')
    clean_segs.main([out, 'nn-segs', 'cleaned', '--out-file', other, '--keep', 'all', '--connectivity', '4'])
    with h5lite.File(other, 'r') as f:
        assert np.array_equal(f['cleaned'][...], LR.clean(est, connectivity=4, keep='all')[0])
