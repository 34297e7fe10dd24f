"""The boundary loss without a GPU: the numpy restatement (boundary_ref.py) against its known answer, against
scipy.ndimage's distance transform through the formula of the paper's code, and against torch.autograd in float64; the C
ABI entries in the header with their host-side refusals; the two flags of train.py."""
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
import boundary_ref as BR  # noqa: E402

ENTRIES = ['dfl_boundary_maps_scratch_bytes', 'dfl_boundary_maps', 'dfl_boundary_loss_scratch_doubles', 'dfl_boundary_loss']
SHAPES = [(5, 7), (1, 9), (9, 1), (33, 130)]


def test_known_answer():
    g = np.array([[[0, 1, 1, 1, 0]]], dtype=np.uint8)
    phi, d2 = BR.maps_of_labels(g, 2)
    assert phi.dtype == np.float32 and phi.shape == (1, 2, 1, 5)
    assert phi[0, 0, 0].tolist() == [0, 1, 2, 1, 0] and phi[0, 1, 0].tolist() == [1, 0, -1, 0, 1]
    assert d2[0, 1, 0].tolist() == [1, 1, 4, 1, 1]
    assert not np.signbit(phi[phi == 0]).any()
    seg = np.full((1, 2, 1, 5), 0.5, dtype=np.float32)
    value, mag, n = BR.term(seg, phi, False)
    assert value == 0.25 and mag == 0.5 * (4 + 3) / 10 and n == 10
    assert BR.term(seg, phi, True)[0] == 0.5 * 1 / 5
    assert np.array_equal(BR.maps(BR.one_hot(g, 2)), phi)


def test_empty_and_whole_image_classes_are_zero_and_ties_take_the_first_maximum():
    g = np.zeros((2, 3, 4), dtype=np.uint8)
    g[1, 1, 2] = 2                                       # image 0: a single class; image 1: one pixel of class 2, none of 1
    phi, _ = BR.maps_of_labels(g, 3)
    assert not phi[0].any() and not phi[1, 1].any() and not np.signbit(phi[phi == 0]).any()
    assert phi[1, 2, 1, 2] == 0 and phi[1, 2, 1, 3] == 1 and phi[1, 2, 0, 0] == np.float32(np.sqrt(5.0))
    assert phi[1, 0, 1, 2] == 1 and phi[1, 0, 0, 0] == np.float32(1.0 - np.sqrt(5.0)) and phi[1, 0, 1, 1] == 0
    t = np.array([0.25, 0.7, 0.7, -1.0], dtype=np.float32).reshape(1, 4, 1, 1)
    assert BR.labels_of(t).tolist() == [[[1]]]
    assert BR.labels_of(np.zeros((1, 4, 1, 1), dtype=np.float32)).tolist() == [[[0]]]


@pytest.mark.parametrize('shape', SHAPES)
def test_restatement_is_one_hot2dist_on_scipy(shape):
    ndi = pytest.importorskip('scipy.ndimage')
    h, w = shape
    seen = 0
    for C_, seed in ((2, 1), (4, 2), (7, 3)):
        g = BR.random_labels(2, C_, h, w, seed)
        phi, _ = BR.maps_of_labels(g, C_)
        for b in range(2):
            for c in range(C_):
                pos = g[b] == c
                if not pos.any() or pos.all():
                    assert not phi[b, c].any()
                    continue
                neg = ~pos
                want = ndi.distance_transform_edt(neg) * neg - (ndi.distance_transform_edt(pos) - 1) * pos
                assert np.array_equal(phi[b, c], want.astype(np.float32)), (shape, C_, b, c)
                assert not np.signbit(phi[b, c][phi[b, c] == 0]).any()
                seen += 1
    assert seen >= 6


def test_gradient_is_autograd_of_the_formula():
    g = BR.random_labels(2, 4, 9, 11, 5)
    phi = BR.maps(BR.one_hot(g, 4))
    rng = np.random.default_rng(0)
    seg = rng.random((2, 4, 9, 11)).astype(np.float32)
    for skip_bg in (False, True):
        s = torch.tensor(seg, dtype=torch.float64, requires_grad=True)
        p = torch.tensor(phi, dtype=torch.float64)
        c0 = 1 if skip_bg else 0
        value = 0.3 * (s[:, c0:] * p[:, c0:]).sum() / BR.count(seg.shape, skip_bg)
        (0.5 * value).backward()
        assert value.item() == pytest.approx(0.3 * BR.term(seg, phi, skip_bg)[0], rel=1e-14)
        assert np.allclose(s.grad.numpy(), BR.grad(phi, skip_bg, beta=0.3, grad_scale=0.5), rtol=1e-14, atol=0.0)
        assert not skip_bg or not s.grad[:, 0].any()


def test_header_declares_the_entries_and_the_binding_follows():
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dfl_hip.h')).read(), flags=re.S)
    at = [re.search(r'\b%s\s*\(' % f, hdr).start() for f in ENTRIES]
    assert at == sorted(at)
    first = nat.EXPORTS.index(ENTRIES[0])
    assert nat.EXPORTS[first:first + len(ENTRIES)] == ENTRIES
    L = nat.lib()
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    assert (L.dfl_boundary_maps_scratch_bytes.restype, L.dfl_boundary_maps_scratch_bytes.argtypes) == (C.c_int, [i32] * 4)
    assert (L.dfl_boundary_maps.restype, L.dfl_boundary_maps.argtypes) == (C.c_int, [vp, i64, i64, i64, i32, i32, i32, i32, vp, vp, vp])
    assert (L.dfl_boundary_loss_scratch_doubles.restype, L.dfl_boundary_loss_scratch_doubles.argtypes) == (C.c_int, [i32] * 3)
    assert (L.dfl_boundary_loss.restype, L.dfl_boundary_loss.argtypes) == (C.c_int, [vp, vp])
    names = [f[0] for f in nat.BoundaryLossArgs._fields_]
    assert names == ['seg', 'phi', 'loss', 'sums', 'grad_scale', 'dseg', 'seg_sN', 'seg_sC', 'seg_sH', 'dseg_sN', 'dseg_sC', 'dseg_sH',
                     'B', 'C', 'h', 'w', 'skip_bg', 'stage', 'accumulate_loss', 'accumulate_grad', 'beta', 'reserved']
    assert C.sizeof(nat.BoundaryLossArgs) == 6 * 8 + 6 * 8 + 8 * 4 + 4 + 4
    assert max(v for k, v in vars(nat).items() if k.startswith('OP_') and isinstance(v, int)) == 24     # no new op kind
    from dfl_amd import boundary
    assert dfl_amd.boundary is boundary and {'boundary', 'DiceBoundaryLoss2D', 'DiceHeatMapBoundaryLoss2D'} <= set(dfl_amd.__all__)
    assert boundary.__all__ == ['signed_distance_maps', 'boundary_term', 'DiceBoundaryLoss2D', 'DiceHeatMapBoundaryLoss2D']
    assert boundary.DiceBoundaryLoss2D().boundary_wgt == 0.01 and boundary.DiceHeatMapBoundaryLoss2D().boundary_wgt == 0.01
    assert boundary.DiceBoundaryLoss2D().skip_bg is True and boundary.DiceHeatMapBoundaryLoss2D().heatmap_wgt == 0.5


def test_maps_entries_check_their_arguments_before_any_launch():
    """No GPU is touched: every case is refused on the host (null pointers throughout, or addresses nothing may follow)."""
    L = nat.lib()
    E = nat.ERR_INVALID_ARG
    err = L.dfl_last_error
    junk = 0x1000                    # an address that is refused before it is followed

    def maps(B=1, C_=7, h=8, w=8, tseg=None, phi=None, scratch=None):
        return L.dfl_boundary_maps(tseg, 64 * C_, 64, 8, B, C_, h, w, phi, scratch, None)
    for call in (maps, lambda **kw: L.dfl_boundary_maps_scratch_bytes(kw.get('B', 1), kw.get('C_', 7), kw.get('h', 8), kw.get('w', 8))):
        for kw in (dict(B=0), dict(h=0), dict(w=-1)):
            assert call(**kw) == E and b'bad sizes' in err()
        for C_ in (1, 0, -3, 32):
            assert call(C_=C_) == E and b'classes' in err()
        assert call(h=46342, w=1) == E and b'squared distance' in err()          # (h-1)^2 alone reaches 2^31 - 1
        assert call(h=32770, w=32770) == E and b'squared distance' in err()
        assert call(h=30000, w=30000) == E and (b'too large' in err() or b'more than an int' in err())   # 16 h w bytes per pair
    assert maps() == E and b'missing pointer' in err()
    assert maps(tseg=junk, phi=junk) == E and b'missing pointer' in err()
    assert maps(tseg=junk, scratch=junk) == E and b'missing pointer' in err()
    assert maps(phi=junk, scratch=junk) == E and b'missing pointer' in err()
    assert maps(tseg=junk, phi=junk, scratch=junk + 4) == E and b'aligned' in err()
    # labels, then the row scratch and the planes of one chunk, each rounded up to 256 bytes
    up = lambda v: (v + 255) // 256 * 256                                       # noqa: E731
    assert L.dfl_boundary_maps_scratch_bytes(3, 7, 33, 130) == up(3 * 4290) + up(3 * 14 * 4291 * 4) + up(3 * 14 * 4290 * 4)
    assert L.dfl_boundary_maps_scratch_bytes(1, 31, 8, 8) == up(64) + up(30 * 65 * 4) + up(30 * 64 * 4)      # 15 pairs a call
    # 8 x 7 x 768^2: three classes of all eight images fit 256 MiB
    assert L.dfl_boundary_maps_scratch_bytes(8, 7, 768, 768) == up(8 * 589824) + up(8 * 6 * 589825 * 4) + up(8 * 6 * 589824 * 4)


def test_loss_entry_checks_its_arguments_before_any_launch():
    L = nat.lib()
    E = nat.ERR_INVALID_ARG
    err = L.dfl_last_error
    junk = 0x1000

    def loss(stage=1, **kw):
        a = nat.BoundaryLossArgs()
        a.B, a.C, a.h, a.w, a.stage, a.beta = 1, 7, 8, 8, stage, 0.01
        for k, v in kw.items():
            setattr(a, k, v)
        return L.dfl_boundary_loss(C.addressof(a), None)
    assert L.dfl_boundary_loss(None, None) == E and b'argument block' in err()
    for kw in (dict(B=0), dict(h=0), dict(w=-1)):
        assert loss(**kw) == E and b'bad sizes' in err()
    for C_ in (1, 0, 32):
        assert loss(C=C_) == E and b'classes' in err()
    assert loss(h=46342, w=1) == E and b'squared distance' in err()
    for stage in (0, 3, -1):
        assert loss(stage=stage, seg=junk, phi=junk, loss=junk, sums=junk, dseg=junk) == E and b'stage' in err()
    for beta in (float('nan'), float('inf')):
        assert loss(beta=beta, seg=junk, phi=junk, loss=junk, sums=junk) == E and b'finite' in err()
    full = dict(seg=junk, phi=junk, loss=junk, sums=junk)
    assert loss() == E and b'missing pointer' in err()
    for leave in full:
        assert loss(**{k: v for k, v in full.items() if k != leave}) == E and b'missing pointer' in err(), leave
    assert loss(stage=2, phi=junk) == E and b'missing pointer' in err()
    assert loss(stage=2, dseg=junk) == E and b'missing pointer' in err()
    for strides in (dict(dseg_sN=448), dict(dseg_sN=448, dseg_sC=64), dict(dseg_sH=8)):
        assert loss(stage=2, phi=junk, dseg=junk, **strides) == E and b'strides' in err()
    # one record per workgroup: a wave per row of an (image, class), four waves, 1024 workgroups at most
    assert L.dfl_boundary_loss_scratch_doubles(1, 2, 1) == 1 and L.dfl_boundary_loss_scratch_doubles(3, 7, 33) == (3 * 7 * 33 + 3) // 4
    assert L.dfl_boundary_loss_scratch_doubles(16, 7, 184) == 1024 and L.dfl_boundary_loss_scratch_doubles(0, 7, 8) == 0


def test_python_entries_refuse_host_tensors():
    from dfl_amd import boundary
    host = torch.zeros((1, 2, 4, 4))
    with pytest.raises(RuntimeError, match='GPU'):
        boundary.signed_distance_maps(host)
    with pytest.raises(RuntimeError, match='GPU'):
        boundary.boundary_term(host, host)
    with pytest.raises(RuntimeError, match='GPU'):
        boundary.DiceBoundaryLoss2D()(host, host)


def test_train_flags():
    import train
    assert train.EXTENSION_FLAGS['boundary_coeff'] is None and train.EXTENSION_FLAGS['boundary_ramp'] == 0
    p = train.build_full_parser()
    a = p.parse_args(['d.h5'])
    assert a.boundary_coeff is None and a.boundary_ramp == 0
    a = p.parse_args(['d.h5', '--boundary-coeff', '0.05', '--boundary-ramp', '12'])
    assert a.boundary_coeff == 0.05 and a.boundary_ramp == 12
    assert p.parse_args(['d.h5', '--boundary-coeff']).boundary_coeff == 0.01          # the default weight
    for bad in (['--boundary-ramp', '-1'], ['--boundary-ramp', '1.5'], ['--boundary-coeff', 'much']):
        with pytest.raises(SystemExit):
            p.parse_args(['d.h5'] + bad)
    with pytest.raises(SystemExit):                         # the reference's own parser knows neither
        train.build_parser().parse_args(['d.h5', '--boundary-coeff', '0.01'])
    assert 'resum' in [x for x in p._actions if x.dest == 'boundary_coeff'][0].help
    assert train.CHECKPOINT_KEYS == ['epoch', 'model-state-dict', 'optim-type', 'optimizer-state-dict', 'scheduler-state-dict', 'loss',
                                     'best-valid-loss', 'save-best-valid', 'num-classes', 'depth', 'init-feats-exp', 'batch-norm',
                                     'padding', 'no-max-pool', 'pad-img-size', 'batch-size', 'data-aug', 'opt-nesterov',
                                     'opt-momentum', 'opt-wgt-decay', 'num-lands', 'heat-coeff', 'use-dice-valid', 'unet-use-res',
                                     'unet-block-depth', 'lrs-meth', 'lrs-num-epochs', 'lrs-growth-factor', 'lrs-max-num-restarts',
                                     'lrs-save-restart-net-prefix', 'lrs-save-after-n-restarts', 'lrs-num-restarts', 'lrs-patience',
                                     'lrs-cooldown', 'checkpoint-freq', 'train-idx', 'valid-idx']
    assert not any('boundary' in k for k in train.Settings.from_args(p.parse_args(['d.h5', '--boundary-coeff', '0.1'])))
    # the weight of 0-based epoch e: B * min(1, (e + 1) / E), B itself without a ramp
    assert [train.boundary_weight(0.02, 4, e) for e in (0, 1, 3, 9)] == [0.005, 0.01, 0.02, 0.02]
    assert train.boundary_weight(0.02, 0, 0) == 0.02 and train.boundary_weight(0.02, 1, 0) == 0.02
