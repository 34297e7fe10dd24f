"""train.py with the cross-entropy / focal term, end to end on the GPU: the toy file and command of
test_gpu_boundary_train.py, one short epoch with --ce-coeff / --focal-gamma / --class-weights (log line, the printed balanced
weights, finite minibatch losses, the checkpoint's keys unchanged), and the same command without the flags (the existing
loss, no such line, a smaller first minibatch loss)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dfl_amd  # noqa: E402
from test_entrypoints_cpu import CHECKPOINT_KEYS  # noqa: E402
from test_gpu_entrypoints import NC, make_file, run  # noqa: E402

pytestmark = pytest.mark.gpu

_RUNS = {}


def _train(tmp_path_factory, extra):
    """(output, minibatch losses, checkpoint, data file) of one epoch; a command runs once per session of this file."""
    key = tuple(extra)
    if key not in _RUNS:
        cwd = str(tmp_path_factory.mktemp('ce_train'))
        make_file(os.path.join(cwd, 'data.npz'))
        out = run('train.py', ['data.npz', '--train-pats', '1', '--valid-pats', '2', '--num-classes', str(NC), '--unet-img-dim', '48',
                               '--batch-size', '4', '--unet-num-lvls', '3', '--unet-init-feats-exp', '3', '--unet-batch-norm',
                               '--unet-padding', '--unet-no-max-pool', '--nesterov', '--init-lr', '0.05', '--checkpoint-net', 'ck.pt',
                               '--best-net', 'best.pt', '--train-loss-txt', 'tl.txt', '--valid-loss-txt', 'vl.txt',
                               '--max-num-epochs', '1', '--seed', '1'] + list(extra), cwd)
        losses = [float(x) for x in open(os.path.join(cwd, 'tl.txt')).read().split()]
        ck = torch.load(os.path.join(cwd, 'ck.pt'), map_location='cpu', weights_only=False)
        _RUNS[key] = (out, losses, ck, os.path.join(cwd, 'data.npz'))
    return _RUNS[key]


def _loss_lines(out):
    return [ln.strip() for ln in out.split('\n') if ln.strip().startswith('loss:')]


def _check_run(out, losses, ck):
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses)           # 8 images / batch 4
    assert list(ck.keys()) == CHECKPOINT_KEYS and ck['epoch'] == 1
    assert 'Exiting - maximum number of epochs performed!' in out


def test_one_epoch_with_the_cross_entropy_term_alone(tmp_path_factory):
    out, losses, ck, _ = _train(tmp_path_factory, ['--ce-coeff'])
    assert _loss_lines(out) == ['loss: Dice + cross-entropy (weight 1.0, gamma 0.0, class weights none)']
    assert 'class weights (' not in out
    _check_run(out, losses, ck)


@pytest.mark.parametrize('more', [[], ['--use-lands'], ['--use-lands', '--boundary-coeff', '0.01']],
                         ids=['dice', 'dice and heat maps', 'dice, heat maps and boundary'])
def test_one_epoch_with_the_balanced_focal_term(tmp_path_factory, more):
    out, losses, ck, data = _train(tmp_path_factory, ['--ce-coeff', '0.5', '--focal-gamma', '2', '--class-weights', 'balanced'] + more)
    middle = ''
    if '--use-lands' in more:
        middle += ' + heat-map NCC (weight 0.5)'
    if '--boundary-coeff' in more:
        middle += ' + boundary distance (weight 0.01, ramp 0)'
    assert _loss_lines(out) == ['loss: Dice' + middle + ' + cross-entropy (weight 0.5, gamma 2.0, class weights balanced)']
    # the weights: the label pixels of the whole training set (specimen 1), before augmentation
    counts = np.bincount(np.load(data)['01/segs'].reshape(-1), minlength=NC)
    want = dfl_amd.balanced_class_weights(counts.tolist())
    assert len(want) == NC and all(w > 0 for w in want) and want[0] < 1 < max(want[1:])
    assert 'class weights (balanced): ' + ', '.join('{:.6g}'.format(v) for v in want) in out
    _check_run(out, losses, ck)


def test_the_term_raises_the_first_minibatch_loss_and_no_flag_means_the_existing_loss(tmp_path_factory):
    out, losses, ck, _ = _train(tmp_path_factory, [])
    assert _loss_lines(out) == ['loss: Dice']
    assert 'cross-entropy' not in out and 'class weights' not in out and 'boundary' not in out
    _check_run(out, losses, ck)
    _, with_ce, _, _ = _train(tmp_path_factory, ['--ce-coeff'])           # (weight 1; the run of the first test)
    print('first minibatch loss', losses[0], 'with --ce-coeff 1', with_ce[0])
    assert with_ce[0] > losses[0]                       # the same initialisation and batch (--seed), and CE > 0
