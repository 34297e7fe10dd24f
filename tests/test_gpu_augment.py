"""Device-side random augmentation (dfl_augment_batch behind dfl_amd.DeviceAugment): explicit-parameter parity against
the fixtures of the numpy restatement (tests/golden/aug_*.npz, tools/gen_aug_golden.py), the Philox noise field, the
rows left alone, the sampler through get_dataset, and train.py --data-aug end to end."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dfl_amd
from dfl_amd import dataset as D
from conftest import ROOT, load_golden
import aug_ref as A

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FIXTURES = ['aug_46_p0', 'aug_46_p1', 'aug_192_p0', 'aug_192_p2', 'aug_37x53_p3']


def _dataset(g, land_rule='reference', prob=0.5):
    W, pad = int(g['W']), int(g['pad'])
    ds = D.DeviceDataSet(torch.from_numpy(g['projs']).unsqueeze(1), torch.from_numpy(g['segs']), torch.from_numpy(g['lands']),
                         proj_pad_dim=W + 2 * pad if pad else 0, num_classes=int(g['C']), device=DEV)
    assert ds.extra_pad == pad
    ds.augment = D.DeviceAugment(0, prob=prob, land_rule=land_rule)
    return ds


@pytest.mark.parametrize('name', FIXTURES)
def test_explicit_parameters_match_restatement(name):
    g = load_golden(name)
    H, W, C, L = int(g['H']), int(g['W']), int(g['C']), int(g['L'])
    prms = A.load_params(g)
    n = len(prms)
    for rule in ('reference', 'in_view'):
        ds = _dataset(g, rule)
        probe = {}
        x, m, l, h = ds._prepare(list(range(n)), aug_params=prms, probe=probe)
        torch.cuda.synchronize()
        assert probe['rows'] == list(range(n))
        np.testing.assert_allclose(l.cpu().numpy(), g['lands_' + rule], rtol=0, atol=1e-4)
        if rule == 'in_view':
            continue
        lev = probe['levels'].cpu().numpy().astype(np.int32)
        want = g['levels'].astype(np.int32)
        diff = np.abs(lev - want)
        assert diff.max() <= 1, (name, int(diff.max()))
        assert (diff == 0).mean() >= 0.999, (name, float((diff == 0).mean()))
        # where the level agrees, the standardised projection agrees (the statistics see the whole image)
        xs = x[:, 0].cpu().numpy()
        same = diff == 0
        assert np.abs(xs - g['x'])[same].max() <= 1e-5, name
        # labels / one-hot masks, except at sources within 1e-6 of an integer
        labels = g['labels']
        mm = m.cpu().numpy()
        ok = ~g['near']
        for c in range(C):
            assert np.array_equal(mm[:, c][ok], (labels == c)[ok].astype(np.float32)), (name, c)
        assert np.array_equal(mm.sum(1)[ok], (labels != 255)[ok].astype(np.float32))
        # heat maps of the transformed landmarks (every finite one, dataset.py:313)
        hh = h.cpu().numpy()[:, :, 0]
        lw = g['lands_reference']
        Yg, Xg = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing='ij')
        for i in range(n):
            for k in range(L):
                if np.isfinite(lw[i, 0, k]):
                    want_h = np.exp(((Xg - lw[i, 0, k]) ** 2 + (Yg - lw[i, 1, k]) ** 2) / np.float32(-2 * 2.5 ** 2)) / np.float32(2 * math.pi * 2.5 ** 2)
                    np.testing.assert_allclose(hh[i, k], want_h, rtol=1e-4, atol=1e-7)
                else:
                    assert not hh[i, k].any()


def test_erase_boxes_at_exact_rows_and_columns():
    g = load_golden('aug_46_p0')
    prms = A.load_params(g)
    i = [k for k, p in enumerate(prms) if p['flags'] == A.ERASE][0]
    base = dict(prms[i], flags=0)
    ds = _dataset(g)
    x0 = ds._prepare([i], aug_params=[base])[0][0, 0]
    ds.do_norm_01_scale = False
    r0 = ds._prepare([i], aug_params=[base])[0][0, 0].cpu().numpy()
    r1 = ds._prepare([i], aug_params=[prms[i]])[0][0, 0].cpu().numpy()
    inside = np.zeros(r0.shape, bool)
    for (a, b, nr, nc, _) in prms[i]['boxes']:
        inside[a:a + nr, b:b + nc] = True
    assert np.array_equal(r0[~inside], r1[~inside])
    assert (r0[inside] != r1[inside]).mean() > 0.99
    assert x0.shape == r0.shape


def test_noise_field_matches_philox_restatement():
    g = load_golden('aug_192_p0')
    H, W = int(g['H']), int(g['W'])
    prm = dict(A.load_params(g)[0], flags=A.NOISE, boxes=[])
    ds = _dataset(g)
    runs = []
    for _ in range(2):
        probe = {}
        ds._prepare([0], aug_params=[prm], probe=probe)
        runs.append(probe['noise'][0].cpu().numpy())
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32))          # same key: same bits
    want = A.normals(prm['noise_key'], np.arange(H * W)).reshape(H, W)
    assert np.abs(runs[0] - want).max() <= 1e-5
    # the residual the noise step adds to the normalised image: mean 0, std sigma (5 standard errors)
    r = runs[0].astype(np.float64).ravel() * prm['sigma']
    assert abs(r.mean()) < 5 * prm['sigma'] / math.sqrt(r.size)
    assert abs(r.std() - prm['sigma']) < 5 * prm['sigma'] / math.sqrt(2 * r.size)


def test_rows_left_alone_are_bit_identical_to_prep():
    g = load_golden('aug_46_p1')
    prms = A.load_params(g)
    ds = _dataset(g)
    plain = D.DeviceDataSet(torch.from_numpy(g['projs']).unsqueeze(1), torch.from_numpy(g['segs']), torch.from_numpy(g['lands']),
                            proj_pad_dim=int(g['W']) + 2, num_classes=int(g['C']), device=DEV)
    mixed = [prms[0], None, prms[2]]
    got = ds._prepare([0, 1, 2], aug_params=mixed)
    ref = plain._prepare([0, 1, 2])
    for a, b in zip(got, ref):
        assert torch.equal(a[1], b[1])
        assert not torch.equal(a[0], b[0])
    # prob = 0: the sampler augments nothing and every tensor equals augment=None's
    ds0 = _dataset(g, prob=0.0)
    for a, b in zip(ds0._prepare([2, 0, 1]), plain._prepare([2, 0, 1])):
        assert torch.equal(a, b)


def _container(tmp_path, n_per_pat=(10, 6), H=44, W=44, L=3, NC=4):
    gen = torch.Generator().manual_seed(5)
    d = {'land-names/num-lands': np.int64(L)}
    for l in range(L):
        d['land-names/land-%02d' % l] = np.array('L%d' % l)
    Y, X = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing='ij')
    for pat, n in enumerate(n_per_pat, 1):
        projs = 0.1 * torch.randn(n, H, W, generator=gen)
        segs = torch.zeros(n, H, W, dtype=torch.uint8)
        lands = torch.zeros(n, 2, L)
        for i in range(n):
            for c in range(1, NC):
                cx, cy = float(torch.rand(1, generator=gen)) * 24 + 10, float(torch.rand(1, generator=gen)) * 24 + 10
                mk = ((X - cx) / 6) ** 2 + ((Y - cy) / 5) ** 2 <= 1
                segs[i][mk] = c
                projs[i][mk] += 0.4 * c
                lands[i, :, min(c - 1, L - 1)] = torch.tensor([cx, cy])
        d['%02d/projs' % pat], d['%02d/segs' % pat], d['%02d/lands' % pat] = projs.numpy(), segs.numpy(), lands.numpy()
    path = str(tmp_path / 'data.npz')
    np.savez(path, **d)
    return path


def test_get_dataset_augments_the_training_split_only(tmp_path):
    path = _container(tmp_path)
    aug = dfl_amd.DeviceAugment(1, prob=1.0)
    tr, va, ti, vi = D.get_dataset(path, [1, 2], 4, pad_img_dim=48, train_valid_split=0.75, augment=aug)
    assert tr.augment is aug and va.augment is None
    plain = D.get_dataset(path, [1, 2], 4, pad_img_dim=48)
    x, m, l, h = next(tr.batches(4))
    assert x.shape == (4, 1, 48, 48) and m.shape == (4, 4, 44, 44) and l.shape == (4, 2, 3) and h.shape == (4, 3, 1, 44, 44)
    want = plain._prepare(ti[:4])
    assert not torch.equal(x, want[0])
    vx = next(va.batches(len(vi)))[0]
    assert torch.equal(vx, plain._prepare(vi)[0])
    # the same epoch draws the same augmentation, the next epoch another one
    again = tr._prepare(list(range(4)))[0]
    assert torch.equal(again, x)
    aug.set_epoch(1)
    assert not torch.equal(tr._prepare(list(range(4)))[0], x)
    with pytest.raises(NotImplementedError, match='augment='):
        D.get_dataset(path, [1], 4, data_aug=True)


def _run(args, cwd):
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + os.path.join(ROOT, 'tests') + os.pathsep + env.get('PYTHONPATH', '')
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


RECORDER = r'''
import sys, torch, numpy as np
sys.argv = sys.argv[1:]
import train
from dfl_amd import dataset as D
seen = {}
orig = D.DeviceDataSet._prepare
def rec(self, idx, *a, **k):
    out = orig(self, idx, *a, **k)
    if self.augment is not None:
        for r, i in enumerate(idx):
            seen[(self.augment.epoch, int(i))] = [None if t is None else t[r].cpu().numpy() for t in out]
    return out
D.DeviceDataSet._prepare = rec
train.main(sys.argv[1:])
np.savez(OUT, **{'%d_%d_%d' % (e, i, j): v for (e, i), vs in seen.items() for j, v in enumerate(vs) if v is not None})
'''


def test_train_data_aug_two_epochs_and_resume(tmp_path):
    from test_entrypoints_cpu import CHECKPOINT_KEYS
    path = _container(tmp_path)
    common = [path, '--train-pats', '1', '--valid-pats', '2', '--num-classes', '4', '--unet-img-dim', '48',
              '--batch-size', '4', '--unet-num-lvls', '3', '--unet-init-feats-exp', '3', '--unet-batch-norm', '--unet-padding',
              '--unet-no-max-pool', '--use-lands', '--nesterov', '--wgt-decay', '1e-4', '--data-aug', '--seed', '1',
              '--checkpoint-net', 'ck.pt', '--best-net', 'best.pt', '--train-loss-txt', 'tl.txt', '--valid-loss-txt', 'vl.txt']
    full, part = tmp_path / 'full', tmp_path / 'part'
    full.mkdir()
    part.mkdir()
    for d, epochs in ((full, 2), (part, 1)):
        (d / 'rec.py').write_text('OUT = %r\n' % str(d / 'seen.npz') + RECORDER)
        out = _run([str(d / 'rec.py'), 'train.py'] + common + ['--max-num-epochs', str(epochs)], str(d))
        assert 'augmentation: DeviceAugment(seed=1, prob=0.5' in out and 'seed 1 (from --seed)' in out
    ck = torch.load(str(full / 'ck.pt'), map_location='cpu', weights_only=False)
    assert list(ck.keys()) == CHECKPOINT_KEYS and ck['data-aug'] is True and ck['epoch'] == 2
    losses = [float(v) for v in (full / 'tl.txt').read_text().split()]
    assert losses and all(math.isfinite(v) for v in losses)
    # resume the one-epoch run for its second epoch: the epoch-1 items are prepared bit for bit as in the full run
    _run([str(part / 'rec.py'), 'train.py'] + common + ['--max-num-epochs', '2'], str(part))
    a, b = np.load(str(full / 'seen.npz')), np.load(str(part / 'seen.npz'))
    keys = [k for k in a.files if k.startswith('1_')]
    assert len(keys) >= 4 * 8
    for k in keys:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
