"""The cross-entropy / focal term without a GPU: the numpy restatement (ce_ref.py) against its known answers, against
torch.nn.functional.nll_loss and against torch.autograd in float64; the C ABI entries in the header with their host-side
refusals; balanced_class_weights; the three flags of train.py."""
import ctypes as C
import math
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
import ce_ref as CR  # noqa: E402

ENTRIES = ['dfl_ce_loss_scratch_doubles', 'dfl_ce_loss']
LN2 = math.log(2.0)


def _one(s, t=1.0):
    """A single pixel of two channels: (s, t) in channel 0, (1 - s, 0) in channel 1."""
    seg = np.array([s, 1.0 - s], dtype=np.float64).reshape(1, 2, 1, 1)
    tgt = np.array([t, 0.0], dtype=np.float64).reshape(1, 2, 1, 1)
    return seg, tgt


def test_known_answers():
    seg, tgt = _one(0.5)
    assert CR.EPS == float(np.float32(2.0) ** -100) == float.fromhex('0x1p-100')
    assert CR.value(seg, tgt) == pytest.approx(LN2, rel=1e-15)
    assert CR.value(seg, tgt, gamma=2.0) == pytest.approx(0.25 * LN2, rel=1e-15)
    assert CR.value(seg, tgt, class_weights=(3.0, 1.0)) == pytest.approx(3 * LN2, rel=1e-15)
    # N counts pixels, not elements: three pixels of two channels, every element a target
    seg3 = np.full((1, 2, 1, 3), 0.5)
    assert CR.count(seg3.shape) == 3
    assert CR.value(seg3, np.ones((1, 2, 1, 3))) == pytest.approx(6 * LN2 / 3, rel=1e-15)
    assert np.allclose(CR.grad(seg3, np.ones((1, 2, 1, 3)), lam=0.5), -0.5 / 3 / 0.5, rtol=1e-15, atol=0)
    # s = 0 at a target: the clamp; the gradient is the formula at EPS, not zero
    seg, tgt = _one(0.0)
    for gamma in (0.0, 1.0, 2.0, 5.0):
        assert CR.value(seg, tgt, gamma=gamma) == pytest.approx(100 * LN2 * (1 - CR.EPS) ** gamma, rel=1e-15)
        want = -0.7 * ((1 - CR.EPS) ** gamma / CR.EPS - gamma * (1 - CR.EPS) ** (gamma - 1) * math.log(CR.EPS))
        got = CR.grad(seg, tgt, gamma=gamma, lam=0.7)
        assert got[0, 0, 0, 0] == pytest.approx(want, rel=1e-15) and got[0, 0, 0, 0] < -2.0 ** 99
        assert got[0, 1, 0, 0] == 0.0 and not np.signbit(got[0, 1, 0, 0])
        assert CR.grad(*_one(CR.EPS / 2), gamma=gamma, lam=0.7)[0, 0, 0, 0] == got[0, 0, 0, 0]
    # s = 1 at a target
    seg, tgt = _one(1.0, t=2.0)
    for gamma in (0.0, 1.0, 2.0, 5.0):
        v = CR.value(seg, tgt, class_weights=(3.0, 1.0), gamma=gamma)
        assert v == 0.0 and not np.signbit(v)
        g = CR.grad(seg, tgt, class_weights=(3.0, 1.0), gamma=gamma, lam=0.7)[0, 0, 0, 0]
        assert g == (pytest.approx(-0.7 * 3.0 * 2.0 / 1, rel=1e-15) if gamma == 0 else 0.0)
    # elements with w t == 0: exactly +0, whatever s is (no logarithm)
    seg = np.array([0.0, np.nan], dtype=np.float64).reshape(1, 2, 1, 1)
    tgt = np.array([1.0, 0.0]).reshape(1, 2, 1, 1)
    assert CR.value(seg, tgt, class_weights=(0.0, 1.0)) == 0.0
    assert not CR.grad(seg, tgt, class_weights=(0.0, 1.0)).any()
    for bad in (0.5, -1.0, 8.5):
        with pytest.raises(AssertionError):
            CR.value(seg, tgt, gamma=bad)


def test_gamma_zero_is_nll_loss_of_the_log_probabilities():
    shape = (2, 5, 7, 9)
    seg = CR.softmax_noise(shape, 3)
    g, t = CR.one_hot_labels(shape, 4)
    logp = torch.log(torch.tensor(seg, dtype=torch.float64))
    lab = torch.tensor(g)
    want = torch.nn.functional.nll_loss(logp, lab, reduction='mean').item()
    assert CR.value(seg, t) == pytest.approx(want, rel=1e-14)
    w = (0.5, 2.0, 0.0, 1.25, 3.0)
    want = torch.nn.functional.nll_loss(logp, lab, weight=torch.tensor(w, dtype=torch.float64), reduction='sum').item() / CR.count(shape)
    assert CR.value(seg, t, class_weights=w) == pytest.approx(want, rel=1e-14)


@pytest.mark.parametrize('gamma', [0.0, 1.0, 2.0, 5.0])
def test_gradient_is_autograd_of_the_formula(gamma):
    shape = (2, 4, 5, 6)
    seg = CR.softmax_noise(shape, 5)
    _, t = CR.one_hot_labels(shape, 6)
    t[0, :, 1, 1] = (0.25, 0.5, 0.0, 0.25)                        # a soft target
    seg[1, 2, 0, 0], t[1, :, 0, 0] = 1.0, (0, 0, 1, 0)            # s = 1 at a target
    seg[1, 3, 0, 1], t[1, :, 0, 1] = CR.EPS, (0, 0, 0, 1)         # s = EPS at a target
    w = (0.5, 2.0, 0.0, 1.25)
    s = torch.tensor(seg, dtype=torch.float64, requires_grad=True)
    tt, ww = torch.tensor(t, dtype=torch.float64), torch.tensor(w, dtype=torch.float64).reshape(1, 4, 1, 1)
    sc = torch.clamp(s, CR.EPS, 1.0)
    value = 0.3 * (-(ww * tt) * (1 - sc) ** gamma * torch.log(sc)).sum() / CR.count(shape)
    (0.5 * value).backward()
    assert value.item() == pytest.approx(0.3 * CR.value(seg, t, w, gamma), rel=1e-14)
    got = CR.grad(seg, t, w, gamma, lam=0.3, grad_scale=0.5)
    assert np.allclose(s.grad.numpy(), got, rtol=1e-12, atol=0.0)
    assert not got[(t * np.asarray(w, dtype=np.float32).reshape(1, 4, 1, 1)) == 0].any()


def test_header_declares_the_entries_and_the_binding_follows():
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dfl_hip.h')).read(), flags=re.S)
    at = [re.search(r'\b%s\s*\(' % f, hdr).start() for f in ['dfl_boundary_loss'] + ENTRIES + ['dfl_get_math_mode']]
    assert at == sorted(at)                                           # after the boundary block
    first = nat.EXPORTS.index(ENTRIES[0])
    assert nat.EXPORTS[first - 1] == 'dfl_boundary_loss' and nat.EXPORTS[first:first + 2] == ENTRIES
    L = nat.lib()
    i32, vp = C.c_int32, C.c_void_p
    assert (L.dfl_ce_loss_scratch_doubles.restype, L.dfl_ce_loss_scratch_doubles.argtypes) == (C.c_int, [i32] * 3)
    assert (L.dfl_ce_loss.restype, L.dfl_ce_loss.argtypes) == (C.c_int, [vp, vp])
    fields = nat.CeLossArgs._fields_
    assert [f[0] for f in fields] == ['seg', 'tseg', 'loss', 'sums', 'grad_scale', 'dseg', 'seg_sN', 'seg_sC', 'seg_sH',
                                      'tseg_sN', 'tseg_sC', 'tseg_sH', 'dseg_sN', 'dseg_sC', 'dseg_sH', 'B', 'C', 'h', 'w', 'stage',
                                      'accumulate_loss', 'accumulate_grad', 'lambda', 'gamma', 'class_wgt']
    assert fields[-1][1] is C.c_float * 32 and dict(fields)['lambda'] is C.c_float and dict(fields)['gamma'] is C.c_float
    assert C.sizeof(nat.CeLossArgs) == 6 * 8 + 9 * 8 + 7 * 4 + 2 * 4 + 32 * 4 + 4          # (4: the tail padding of 8-byte members)
    assert nat.CeLossArgs not in nat._SIZEOF_ORDER and nat._SIZEOF_ORDER[-1] is nat.OptimPackArgs
    assert max(v for k, v in vars(nat).items() if k.startswith('OP_') and isinstance(v, int)) == 24     # no new op kind
    assert nat.LABEL_MAX_CLASSES == 31
    from dfl_amd import ce
    assert dfl_amd.ce is ce and set(ce.__all__) <= set(dfl_amd.__all__) and 'ce' in dfl_amd.__all__
    assert ce.__all__ == ['cross_entropy_term', 'balanced_class_weights', 'DiceCELoss2D', 'DiceHeatMapCELoss2D']
    d, dh = ce.DiceCELoss2D(), ce.DiceHeatMapCELoss2D()
    assert (d.skip_bg, d.ce_wgt, d.gamma, d.class_weights, d.boundary_wgt) == (True, 1.0, 0.0, None, 0.0)
    assert (dh.skip_bg, dh.heatmap_wgt, dh.ce_wgt, dh.gamma, dh.class_weights, dh.boundary_wgt) == (True, 0.5, 1.0, 0.0, None, 0.0)


def test_entry_checks_its_arguments_before_any_launch():
    """No GPU is touched: every case is refused on the host (null pointers, or addresses nothing may follow)."""
    L = nat.lib()
    E = nat.ERR_INVALID_ARG
    err = L.dfl_last_error
    junk = 0x1000
    s1 = dict(seg=junk, tseg=junk, loss=junk, sums=junk)
    s2 = dict(seg=junk, tseg=junk, dseg=junk)

    def loss(stage=1, weights=None, **kw):
        a = nat.CeLossArgs()
        a.B, a.C, a.h, a.w, a.stage = 1, 7, 8, 8, stage
        setattr(a, 'lambda', 1.0)
        for c in range(32):
            a.class_wgt[c] = 1.0
        for c, v in (weights or {}).items():
            a.class_wgt[c] = v
        for k, v in kw.items():
            setattr(a, k, v)
        return L.dfl_ce_loss(C.addressof(a), None)
    assert L.dfl_ce_loss(None, None) == E and b'argument block' in err()
    for kw in (dict(B=0), dict(h=0), dict(w=-1), dict(B=-2)):
        assert loss(**dict(s1, **kw)) == E and b'bad sizes' in err(), kw
    for C_ in (1, 0, -3, 32):
        assert loss(**dict(s1, C=C_)) == E and b'C = ' in err() and b'classes' in err()
    for stage in (0, 3, -1):
        assert loss(stage=stage, **dict(s1, dseg=junk)) == E and b'stage' in err()
    for bad in (float('nan'), float('inf'), -float('inf')):
        assert loss(**dict(s1, **{'lambda': bad})) == E and b'lambda' in err() and b'finite' in err()
        assert loss(**dict(s1, gamma=bad)) == E and b'gamma' in err() and b'finite' in err()
    for gamma in (0.5, 0.999, -1.0, 1e-30, 8.5):
        assert loss(**dict(s1, gamma=gamma)) == E and b'gamma' in err(), gamma
        assert loss(stage=2, **dict(s2, gamma=gamma)) == E and b'gamma' in err(), gamma
    for c, bad in ((0, -1.0), (6, float('nan')), (3, float('inf')), (6, -1e-30)):
        assert loss(weights={c: bad}, **s1) == E and b'class_wgt[%d]' % c in err()
    assert loss() == E and b'missing pointer' in err()
    for leave in s1:
        assert loss(**{k: v for k, v in s1.items() if k != leave}) == E and b'missing pointer' in err() and leave.encode() in err(), leave
    for leave in s2:
        assert loss(stage=2, **{k: v for k, v in s2.items() if k != leave}) == E and b'missing pointer' in err() and leave.encode() in err(), leave
    for strides in (dict(dseg_sN=448), dict(dseg_sN=448, dseg_sC=64), dict(dseg_sH=8), dict(dseg_sC=64, dseg_sH=8)):
        assert loss(stage=2, **dict(s2, **strides)) == E and b'strides' in err() and b'dseg' in err()
    # one record per workgroup: a wave per row of an (image, class), four waves, 1024 workgroups at most
    assert L.dfl_ce_loss_scratch_doubles(1, 2, 1) == 1 and L.dfl_ce_loss_scratch_doubles(3, 7, 33) == (3 * 7 * 33 + 3) // 4
    assert L.dfl_ce_loss_scratch_doubles(3, 7, 200) == 1024 and L.dfl_ce_loss_scratch_doubles(0, 7, 8) == 0


def test_python_entries_refuse_host_tensors():
    from dfl_amd import ce
    host = torch.zeros((1, 2, 4, 4))
    with pytest.raises(RuntimeError, match='GPU'):
        ce.cross_entropy_term(host, host)
    with pytest.raises(RuntimeError, match='GPU'):
        ce.DiceCELoss2D()(host, host)
    with pytest.raises(RuntimeError, match='GPU'):
        ce.DiceCELoss2D(ce_wgt=0.0)(host, host)
    with pytest.raises(RuntimeError, match='GPU'):
        ce.DiceHeatMapCELoss2D(boundary_wgt=0.01)((host, host), (host, host))


def test_balanced_class_weights():
    f = dfl_amd.balanced_class_weights
    assert f((6, 3, 0, 3)) == (0.5, 1.0, 0.0, 1.0)
    assert f([5, 5]) == (1.0, 1.0) and f((0, 0, 0)) == (0.0, 0.0, 0.0)
    assert f(torch.tensor([1, 3])) == (2.0, 2.0 / 3.0)
    w = f((10 ** 9, 1, 7))
    assert w == ((10 ** 9 + 8) / (3 * 10 ** 9), (10 ** 9 + 8) / 3, (10 ** 9 + 8) / 21)
    with pytest.raises(ValueError):
        f((3, -1))
    with pytest.raises(ValueError):
        f(())


def test_train_flags(capsys):
    import train
    E = train.EXTENSION_FLAGS
    assert E['ce_coeff'] is None and E['focal_gamma'] == 0.0 and E['class_weights'] is None
    assert E['boundary_coeff'] is None and E['boundary_ramp'] == 0
    p = train.build_full_parser()
    a = p.parse_args(['d.h5'])
    assert a.ce_coeff is None and a.focal_gamma == 0.0 and a.class_weights is None
    a = train.parse_args(['d.h5'])
    assert a.ce_coeff is None and a.focal_gamma == 0.0 and a.class_weights is None and a.boundary_coeff is None
    assert train.parse_args(['d.h5', '--ce-coeff']).ce_coeff == 1.0                      # the default weight
    a = train.parse_args(['d.h5', '--num-classes', '3', '--ce-coeff', '0.5', '--focal-gamma', '2', '--class-weights', '1,0,2.5'])
    assert (a.ce_coeff, a.focal_gamma, a.class_weights) == (0.5, 2.0, (1.0, 0.0, 2.5))
    a = train.parse_args(['d.h5', '--ce-coeff', '--class-weights', 'balanced', '--focal-gamma', '8', '--boundary-coeff'])
    assert (a.ce_coeff, a.focal_gamma, a.class_weights, a.boundary_coeff) == (1.0, 8.0, 'balanced', 0.01)
    for bad in (['--focal-gamma', '2'], ['--class-weights', 'balanced'], ['--class-weights', '1,1'],      # without --ce-coeff
                ['--ce-coeff', '--focal-gamma', '0.5'], ['--ce-coeff', '--focal-gamma', '9'], ['--ce-coeff', '--focal-gamma', '-1'],
                ['--ce-coeff', '--focal-gamma', 'nan'], ['--ce-coeff', '--focal-gamma', 'sharp'], ['--ce-coeff', 'much'],
                ['--ce-coeff', 'inf'], ['--ce-coeff', '--num-classes', '3', '--class-weights', '1,1'],        # a wrong count
                ['--ce-coeff', '--num-classes', '3', '--class-weights', '1,1,1,1'], ['--ce-coeff', '--class-weights', '1,-1'],
                ['--ce-coeff', '--class-weights', '1,x'], ['--ce-coeff', '--class-weights', '1,inf'], ['--ce-coeff', '--class-weights', '']):
        with pytest.raises(SystemExit):
            train.parse_args(['d.h5'] + bad)
        assert 'error' in capsys.readouterr().err, bad
    for flag in (['--ce-coeff', '1'], ['--focal-gamma', '2'], ['--class-weights', 'balanced']):          # the reference's own parser
        with pytest.raises(SystemExit):
            train.build_parser().parse_args(['d.h5'] + flag)
    for dest in ('ce_coeff', 'focal_gamma', 'class_weights'):
        assert 'give it again when resuming' in ' '.join([x for x in p._actions if x.dest == dest][0].help.split())
    assert train.CHECKPOINT_KEYS == ['epoch', 'model-state-dict', 'optim-type', 'optimizer-state-dict', 'scheduler-state-dict', 'loss',
                                     'best-valid-loss', 'save-best-valid', 'num-classes', 'depth', 'init-feats-exp', 'batch-norm',
                                     'padding', 'no-max-pool', 'pad-img-size', 'batch-size', 'data-aug', 'opt-nesterov',
                                     'opt-momentum', 'opt-wgt-decay', 'num-lands', 'heat-coeff', 'use-dice-valid', 'unet-use-res',
                                     'unet-block-depth', 'lrs-meth', 'lrs-num-epochs', 'lrs-growth-factor', 'lrs-max-num-restarts',
                                     'lrs-save-restart-net-prefix', 'lrs-save-after-n-restarts', 'lrs-num-restarts', 'lrs-patience',
                                     'lrs-cooldown', 'checkpoint-freq', 'train-idx', 'valid-idx']
    s = train.Settings.from_args(train.parse_args(['d.h5', '--ce-coeff', '0.3', '--focal-gamma', '2', '--class-weights', 'balanced']))
    assert 'ce' not in s and not any(k.startswith('ce-') or w in k for k in s for w in ('focal', 'gamma', 'class-w', 'entropy'))
