"""train.py with the boundary-distance term, end to end on the GPU: the toy file of test_gpu_entrypoints.py, one short epoch
with --boundary-coeff / --boundary-ramp (log line, finite minibatch losses, the checkpoint's keys unchanged), and the same
command without the flags (the existing loss, no such line)."""
import math
import os

import pytest
import torch

from test_entrypoints_cpu import CHECKPOINT_KEYS
from test_gpu_entrypoints import NC, make_file, run

pytestmark = pytest.mark.gpu


def _train(tmp_path, extra):
    cwd = str(tmp_path)
    make_file(os.path.join(cwd, 'data.npz'))
    out = run('train.py', ['data.npz', '--train-pats', '1', '--valid-pats', '2', '--num-classes', str(NC), '--unet-img-dim', '48',
                           '--batch-size', '4', '--unet-num-lvls', '3', '--unet-init-feats-exp', '3', '--unet-batch-norm',
                           '--unet-padding', '--unet-no-max-pool', '--nesterov', '--init-lr', '0.05', '--checkpoint-net', 'ck.pt',
                           '--best-net', 'best.pt', '--train-loss-txt', 'tl.txt', '--valid-loss-txt', 'vl.txt',
                           '--max-num-epochs', '1', '--seed', '1'] + extra, cwd)
    losses = [float(x) for x in open(os.path.join(cwd, 'tl.txt')).read().split()]
    ck = torch.load(os.path.join(cwd, 'ck.pt'), map_location='cpu', weights_only=False)
    return out, losses, ck


@pytest.mark.parametrize('lands', [False, True], ids=['dice', 'dice and heat maps'])
def test_one_epoch_with_the_boundary_term(tmp_path, lands):
    out, losses, ck = _train(tmp_path, ['--boundary-coeff', '0.01', '--boundary-ramp', '2'] + (['--use-lands'] if lands else []))
    if lands:
        assert 'loss: Dice + heat-map NCC (weight 0.5) + boundary distance (weight 0.01, ramp 2)' in out
    else:
        assert 'loss: Dice + boundary distance (weight 0.01, ramp 2)' in out
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses)           # 8 images / batch 4
    assert list(ck.keys()) == CHECKPOINT_KEYS and ck['epoch'] == 1
    assert 'Exiting - maximum number of epochs performed!' in out


@pytest.mark.parametrize('lands', [False, True], ids=['dice', 'dice and heat maps'])
def test_one_epoch_without_the_flags_is_the_existing_loss(tmp_path, lands):
    out, losses, ck = _train(tmp_path, ['--use-lands'] if lands else [])
    lines = [ln.strip() for ln in out.split('\n') if ln.strip().startswith('loss:')]
    assert lines == (['loss: Dice + heat-map NCC (weight 0.5)'] if lands else ['loss: Dice'])
    assert 'boundary' not in out
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses)
    assert list(ck.keys()) == CHECKPOINT_KEYS
