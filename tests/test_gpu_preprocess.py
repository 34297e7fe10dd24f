"""dfl_amd.preprocess on the GPU (csrc/preproc.hip) against tests/preproc_ref.py, the numpy float64 restatement of the
arithmetic: projections within 2e-5, labels and restored labels bit for bit; a constant image that must come out as
exactly 0; constructed ties; the refusal of a label above 15; one case at the published detector size; and the command
line end to end -- full-resolution container -> preprocess_full_res.py -> loader -> one train.py epoch.

The bar of 2e-5 for projections: values are at most log 65535 = 11.1, where one fp32 ulp is 9.5e-7; a sequential fp32
sum of the 256 terms of a 16 x 16 box stays within 8.8e-6 of float64, and a 1-ulp logarithm adds about 1e-6."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
import preproc_ref as PR  # noqa: E402
import dfl_amd  # noqa: E402
from dfl_amd import _native as nat, h5lite, preprocess as pp  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
TOL = 2e-5
SHAPES = [(53, 70, 3), (64, 64, 0), (200, 232, 50)]             # rows, columns, crop
FACTORS = [1, 2, 3, 4, 8, 16]
ROT = [0, 1, 0]
_CACHE = {}


def _inputs(R, C):
    """A batch of 3: uint16 and float32 intensities with zeros and values below min_intensity, and 7 labels in blobs."""
    key = ('in', R, C)
    if key not in _CACHE:
        g = np.random.default_rng(1000 * R + C)
        u16 = g.integers(0, 65536, size=(3, R, C)).astype(np.uint16)
        u16[g.random((3, R, C)) < 0.05] = 0
        f32 = (g.random((3, R, C)) * np.float32(4000.0)).astype(np.float32)
        f32[g.random((3, R, C)) < 0.05] = 0.0
        f32[g.random((3, R, C)) < 0.05] *= np.float32(1e-4)       # below min_intensity = 1
        coarse = g.integers(0, 7, size=(3, -(-R // 5), -(-C // 5))).astype(np.uint8)
        lab = np.repeat(np.repeat(coarse, 5, 1), 5, 2)[:, :R, :C].copy()
        speck = g.random((3, R, C)) < 0.1
        lab[speck] = g.integers(0, 7, size=int(speck.sum())).astype(np.uint8)
        _CACHE[key] = (u16, f32, lab)
    return _CACHE[key]


def _ref(kind, R, C, crop, f, **kw):
    key = (kind, R, C, crop, f) + tuple(sorted(kw.items()))
    if key not in _CACHE:
        u16, f32, lab = _inputs(R, C)
        if kind == 'u16' or kind == 'f32':
            _CACHE[key] = PR.projs(u16 if kind == 'u16' else f32, ROT, crop, f, **kw)
        else:
            _CACHE[key] = PR.segs(lab, ROT, crop, f)
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- projections -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f', FACTORS)
@pytest.mark.parametrize('R,C,crop', SHAPES)
@pytest.mark.parametrize('kind', ['u16', 'f32'])
def test_projections_match_the_reference(kind, R, C, crop, f):
    u16, f32, _ = _inputs(R, C)
    out = pp.preprocess_projs(_dev(u16 if kind == 'u16' else f32), ROT, crop=crop, factor=f)
    assert out.dtype == torch.float32 and out.is_cuda and tuple(out.shape) == (3,) + PR.out_size(R, C, crop, f)
    ref = _ref(kind, R, C, crop, f)
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
    print('preprocess_projs %s %dx%d crop %d f %d: max |error| %.3e' % (kind, R, C, crop, f, err))
    assert np.all(np.isfinite(out.cpu().numpy())) and float(out.min()) >= 0.0
    assert err <= TOL, err


@pytest.mark.parametrize('f', [5, 6, 7, 9, 10, 11, 12, 13, 14, 15])
def test_the_other_factors(f):
    """Every factor is its own kernel instantiation: the ones the lists above leave out, on the smallest shape."""
    R, C, crop = SHAPES[0]
    u16, f32, lab = _inputs(R, C)
    for px in (u16, f32):
        out = pp.preprocess_projs(_dev(px), ROT, crop=crop, factor=f)
        assert float(np.abs(out.cpu().numpy().astype(np.float64) - PR.projs(px, ROT, crop, f)).max()) <= TOL
    seg = pp.preprocess_segs(_dev(lab), ROT, crop=crop, factor=f)
    assert np.array_equal(seg.cpu().numpy(), PR.segs(lab, ROT, crop, f))
    full = pp.restore_labels(seg, ROT, R, C, crop=crop, factor=f)
    assert np.array_equal(full.cpu().numpy(), PR.restore(seg.cpu().numpy(), ROT, R, C, crop, f))


@pytest.mark.parametrize('f', [1, 3, 8])
def test_projections_without_log_and_with_another_floor(f):
    R, C, crop = SHAPES[0]
    _, f32, _ = _inputs(R, C)
    # log=False under the same bar: intensities up to 16, where one fp32 ulp (9.5e-7) is that of the largest line integral
    low = (f32 * np.float32(16.0 / 4000.0)).astype(np.float32)
    out = pp.preprocess_projs(_dev(low), ROT, crop=crop, factor=f, log=False)
    assert float(np.abs(out.cpu().numpy().astype(np.float64) - PR.projs(low, ROT, crop, f, log=False)).max()) <= TOL
    # and at any magnitude the result is the fp64 box mean rounded to fp32 (uint16 input, values up to 65535)
    u16 = _inputs(R, C)[0]
    out = pp.preprocess_projs(_dev(u16), ROT, crop=crop, factor=f, log=False)
    ref = PR.projs(u16, ROT, crop, f, log=False)
    assert float((np.abs(out.cpu().numpy().astype(np.float64) - ref) / np.maximum(np.abs(ref), 1e-30)).max()) <= 2.0 ** -23
    out = pp.preprocess_projs(_dev(f32), ROT, crop=crop, factor=f, min_intensity=37.5)
    ref = PR.projs(f32, ROT, crop, f, min_intensity=37.5)
    assert float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max()) <= TOL


@pytest.mark.parametrize('f', FACTORS)
@pytest.mark.parametrize('value', [1234.567, 0.25, 65535.0])
def test_a_constant_image_is_exactly_zero(value, f):
    R, C, crop = SHAPES[0]
    img = torch.full((2, R, C), value, dtype=torch.float32, device=DEV)
    out = pp.preprocess_projs(img, [0, 1], crop=crop, factor=f)
    assert torch.count_nonzero(out).item() == 0
    if value >= 1 and float(value).is_integer():
        out = pp.preprocess_projs(img.to(torch.uint16), [1, 0], crop=crop, factor=f)
        assert torch.count_nonzero(out).item() == 0


def test_the_border_does_not_reach_the_output():
    """The brightest pixels sit in the cropped border: they must not set I0, and rotation must not pull them in."""
    R, C, crop = 64, 80, 5
    g = np.random.default_rng(9)
    img = (g.random((2, R, C)) * 100 + 1).astype(np.float32)
    ref = PR.projs(img, [0, 1], crop, 4)
    img2 = img.copy()
    img2[:, :crop] = img2[:, -crop:] = 60000.0
    img2[:, :, :crop] = img2[:, :, -crop:] = 60000.0
    out = pp.preprocess_projs(_dev(img2), [0, 1], crop=crop, factor=4)
    assert float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max()) <= TOL


# ---- labels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f', FACTORS)
@pytest.mark.parametrize('R,C,crop', SHAPES)
def test_labels_match_the_reference(R, C, crop, f):
    _, _, lab = _inputs(R, C)
    out = pp.preprocess_segs(_dev(lab), ROT, crop=crop, factor=f)
    assert out.dtype == torch.uint8 and out.is_cuda
    assert np.array_equal(out.cpu().numpy(), _ref('seg', R, C, crop, f))


def test_ties_go_to_the_smallest_label():
    # f = 2: every box holds two labels twice, the larger one first in memory
    lab = np.zeros((1, 4, 6), np.uint8)
    lab[0, 0:2, 0:2] = [[3, 1], [1, 3]]
    lab[0, 0:2, 2:4] = [[15, 15], [0, 0]]
    lab[0, 0:2, 4:6] = [[9, 8], [9, 8]]
    lab[0, 2:4, 0:2] = [[14, 15], [15, 14]]
    lab[0, 2:4, 2:4] = [[7, 7], [2, 2]]
    lab[0, 2:4, 4:6] = [[5, 4], [4, 5]]
    want = np.array([[[1, 0, 8], [14, 2, 4]]], np.uint8)
    assert np.array_equal(PR.segs(lab, [0], 0, 2), want)
    assert np.array_equal(pp.preprocess_segs(_dev(lab), [0], crop=0, factor=2).cpu().numpy(), want)
    assert np.array_equal(pp.preprocess_segs(_dev(lab), [1], crop=0, factor=2).cpu().numpy(), want[:, ::-1, ::-1])
    # f = 3: three labels three times each
    lab = np.zeros((1, 3, 6), np.uint8)
    lab[0, :, 0:3] = [[6, 4, 2], [6, 4, 2], [6, 4, 2]]
    lab[0, :, 3:6] = [[13, 13, 13], [11, 12, 11], [12, 11, 12]]
    want = np.array([[[2, 11]]], np.uint8)
    assert np.array_equal(PR.segs(lab, [0], 0, 3), want)
    assert np.array_equal(pp.preprocess_segs(_dev(lab), [0], crop=0, factor=3).cpu().numpy(), want)
    # f = 16: a box of one label only (256 of it), and a 128 / 128 tie
    lab = np.zeros((1, 16, 32), np.uint8)
    lab[0, :, :16] = 15
    lab[0, :8, 16:] = 7
    lab[0, 8:, 16:] = 3
    assert np.array_equal(pp.preprocess_segs(_dev(lab), [0], crop=0, factor=16).cpu().numpy(), [[[15, 3]]])


@pytest.mark.parametrize('f', [1, 4, 16])
def test_a_label_above_15_is_refused(f):
    R, C, crop = SHAPES[0]
    _, _, lab = _inputs(R, C)
    lab = lab.copy()
    lab[1, 20, 33] = 16
    with pytest.raises(nat.DflError, match='15'):
        pp.preprocess_segs(_dev(lab), ROT, crop=crop, factor=f)
    lab[1, 20, 33] = 255
    with pytest.raises(nat.DflError, match='15'):
        pp.preprocess_segs(_dev(lab), ROT, crop=crop, factor=f)
    lab[1, 20, 33] = 15
    out = pp.preprocess_segs(_dev(lab), ROT, crop=crop, factor=f)
    assert np.array_equal(out.cpu().numpy(), PR.segs(lab, ROT, crop, f))


# ---- restore -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f', FACTORS)
@pytest.mark.parametrize('R,C,crop', SHAPES + [(40, 96, 8)])      # 96 and 64 columns: the 16-byte store path
def test_restore_matches_the_reference_and_inverts(R, C, crop, f):
    Ro, Co = PR.out_size(R, C, crop, f)
    g = np.random.default_rng(R + 7 * f)
    small = g.integers(0, 256, size=(3, Ro, Co)).astype(np.uint8)       # restore copies labels: any byte
    out = pp.restore_labels(_dev(small), ROT, R, C, crop=crop, factor=f)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (3, R, C)
    ref = PR.restore(small, ROT, R, C, crop, f)
    assert np.array_equal(out.cpu().numpy(), ref)
    if crop:
        o = out.cpu().numpy()
        assert not o[:, :crop].any() and not o[:, -crop:].any() and not o[:, :, :crop].any() and not o[:, :, -crop:].any()
    small = small & 15
    back = pp.preprocess_segs(pp.restore_labels(_dev(small), ROT, R, C, crop=crop, factor=f), ROT, crop=crop, factor=f)
    assert np.array_equal(back.cpu().numpy(), small)


# ---- the published detector size ---------------------------------------------------------------------------------------
def test_full_size_projections_and_labels():
    R = C = 1536
    g = np.random.default_rng(77)
    img = (g.random((2, R, C), dtype=np.float32) * np.float32(30000.0)).astype(np.float32)
    img[g.random((2, R, C)) < 0.02] = 0.0
    coarse = g.integers(0, 7, size=(2, R // 12, C // 12)).astype(np.uint8)
    lab = np.repeat(np.repeat(coarse, 12, 1), 12, 2)
    rot = [0, 1]
    out = pp.preprocess_projs(_dev(img), rot)                           # defaults: crop 50, factor 8
    assert tuple(out.shape) == (2, 180, 180)
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - PR.projs(img, rot, 50, 8)).max())
    print('preprocess_projs 1536 x 1536 f 8: max |error| %.3e' % err)
    assert err <= TOL, err
    seg = pp.preprocess_segs(_dev(lab), rot)
    assert np.array_equal(seg.cpu().numpy(), PR.segs(lab, rot, 50, 8))
    full = pp.restore_labels(seg, rot, R, C).cpu().numpy()
    assert np.array_equal(full, PR.restore_fast(seg.cpu().numpy(), rot, R, C, 50, 8))
    assert np.array_equal(pp.preprocess_segs(_dev(full), rot).cpu().numpy(), seg.cpu().numpy())


# ---- end to end --------------------------------------------------------------------------------------------------------
E2E_R, E2E_C, E2E_CROP, E2E_F = 200, 232, 50, 2
SPECS = [('18-2800', 3), ('17-1882', 2)]                                # not the README's six: sorted -> 17-1882 is 01


def _write_full_res(path):
    g = np.random.default_rng(2020)
    names = list(pp.LAND_ORDER)
    data = {}
    with h5lite.File(path, 'w') as f:
        f['proj-params/num-cols'] = np.int64(E2E_C)
        f['proj-params/num-rows'] = np.int64(E2E_R)
        for s, (spec, n) in enumerate(SPECS):
            imgs, segs, rots, lands = [], [], [], []
            for p in range(n):
                pfx = '%s/projections/%03d/' % (spec, p)
                img = (g.random((E2E_R, E2E_C)) * 20000.0).astype(np.float32)
                img[g.random((E2E_R, E2E_C)) < 0.03] = 0.0
                coarse = g.integers(0, 7, size=(E2E_R // 8, E2E_C // 8)).astype(np.uint8)
                seg = np.repeat(np.repeat(coarse, 8, 0), 8, 1)
                rot = (p + s) % 2
                # integer pixel centres inside the crop window (mapped: k / 2 - 0.25, never half-way between two pixels)
                la = np.stack([g.integers(E2E_CROP + 8, E2E_C - E2E_CROP - 8, size=14),
                               g.integers(E2E_CROP + 8, E2E_R - E2E_CROP - 8, size=14)]).astype(np.float64)
                if s == 1 and p == 1:
                    la[:, 5] = (E2E_C + 40.0, -12.0)                   # one landmark outside the view
                f.create_dataset(pfx + 'image/pixels', data=img, chunks=(E2E_R, E2E_C), compression='gzip')
                f.create_dataset(pfx + 'gt-seg/pixels', data=seg, chunks=(E2E_R, E2E_C), compression='gzip')
                for l in reversed(range(14)):
                    v = la[:, l].astype(np.float32)
                    f[pfx + 'gt-landmarks/' + names[l]] = v if l % 2 else v.reshape(2, 1)
                f[pfx + 'rot-180-for-up'] = np.int64(rot)
                imgs.append(img)
                segs.append(seg)
                rots.append(rot)
                lands.append(la)
            data[spec] = (np.stack(imgs), np.stack(segs), rots, np.stack(lands))
    return data


def _run(script, args, cwd):
    p = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    return p.stdout


def test_command_line_to_loader_to_training(tmp_path):
    from dfl_amd import dataset
    cwd = str(tmp_path)
    data = _write_full_res(os.path.join(cwd, 'full.h5'))
    out = _run('preprocess_full_res.py', ['full.h5', 'pre.h5', '--ds-factor', str(E2E_F), '--chunk', '2'], cwd)
    Ro, Co = PR.out_size(E2E_R, E2E_C, E2E_CROP, E2E_F)
    lines = out.strip().split('\n')
    assert lines == ['17-1882 -> 01: 2 projections, %d x %d' % (Ro, Co), '18-2800 -> 02: 3 projections, %d x %d' % (Ro, Co)]
    pre = os.path.join(cwd, 'pre.h5')
    assert dataset.get_num_lands_from_dataset(pre) == 14
    assert dataset.get_land_names_from_dataset(pre) == pp.LAND_ORDER
    want = {}
    with h5lite.File(pre, 'r') as f:
        assert sorted(f.keys()) == ['01', '02', 'land-names']
        for grp, spec in (('01', '17-1882'), ('02', '18-2800')):
            imgs, segs, rots, lands = data[spec]
            projs = f[grp + '/projs'][()]
            assert projs.dtype == np.float32 and f[grp + '/segs'][()].dtype == np.uint8 and f[grp + '/lands'][()].dtype == np.float32
            assert float(np.abs(projs.astype(np.float64) - PR.projs(imgs, rots, E2E_CROP, E2E_F)).max()) <= TOL
            assert np.array_equal(f[grp + '/segs'][()], PR.segs(segs, rots, E2E_CROP, E2E_F))
            ml = PR.map_lands(lands, rots, E2E_R, E2E_C, E2E_CROP, E2E_F)
            assert np.array_equal(f[grp + '/lands'][()], ml.astype(np.float32)) and f[grp + '/lands'].shape == (len(rots), 2, 14)
            want[grp] = (PR.segs(segs, rots, E2E_CROP, E2E_F), ml)
    # the loader: masks are the one-hot labels, every heat map peaks on the pixel the mapped landmark rounds to
    ds = dataset.get_dataset(pre, [1, 2], num_classes=7, pad_img_dim=68, device=DEV)
    seg_all = np.concatenate([want['01'][0], want['02'][0]])
    land_all = np.concatenate([want['01'][1], want['02'][1]])
    assert len(ds) == 5
    outside = 0
    for i in range(5):
        x, masks, lands, heats = ds[i][:4]
        assert tuple(x.shape) == (1, Ro + 2, Co + 2)                    # 66 columns padded to 68
        assert np.array_equal(masks.argmax(0).cpu().numpy(), seg_all[i]) and float(masks.sum(0).min()) == 1.0
        for l in range(14):
            cx, cy = land_all[i, :, l]
            h = heats[l].reshape(Ro, Co)
            if 0 <= cx <= Co - 1 and 0 <= cy <= Ro - 1:
                r, c = divmod(int(h.argmax()), Co)
                assert (r, c) == (int(round(cy)), int(round(cx))), (i, l, (r, c), (cy, cx))
                assert abs(float(lands[0, l]) - cx) < 1e-4 and abs(float(lands[1, l]) - cy) < 1e-4
            else:
                outside += 1
                assert not torch.isfinite(lands[:, l]).any() and float(h.abs().max()) == 0.0
    assert outside == 1
    # the entry point the file is for: one epoch of a depth-2 toy network
    out = _run('train.py', ['pre.h5', '--train-pats', '2', '--valid-pats', '1', '--num-classes', '7', '--unet-img-dim', '68',
                            '--batch-size', '3', '--unet-num-lvls', '2', '--unet-init-feats-exp', '3', '--unet-batch-norm',
                            '--unet-padding', '--unet-no-max-pool', '--use-lands', '--init-lr', '0.05', '--max-num-epochs', '1',
                            '--checkpoint-net', 'ck.pt', '--train-loss-txt', 'tl.txt', '--valid-loss-txt', 'vl.txt',
                            '--no-save-best-valid', '--seed', '3'], cwd)
    assert 'Exiting - maximum number of epochs performed!' in out
    tl = [float(v) for v in open(os.path.join(cwd, 'tl.txt')).read().split('\n')[:-1]]
    assert len(tl) == 1 and np.isfinite(tl[0])


# ---- convert_file: orders, overrides and refusals ----------------------------------------------------------------------
def _tiny_full_res(path, specs, names, drop=None, dtypes=None, bad_shape=None, R=24, C=28):
    """A full-resolution container of R x C projections; drop = (specimen, projection, landmark) left out."""
    g = np.random.default_rng(11)
    data = {}
    with h5lite.File(path, 'w') as f:
        f['proj-params/num-cols'] = np.int64(C)
        f['proj-params/num-rows'] = np.int64(R)
        for spec, n in specs:
            for p in range(n):
                pfx = '%s/projections/%03d/' % (spec, p)
                shape = (R, C + 2) if bad_shape == (spec, p) else (R, C)
                dt = (dtypes or {}).get((spec, p), np.float32)
                img = g.integers(0, 5000, size=shape).astype(dt)
                seg = g.integers(0, 7, size=shape).astype(np.uint8)
                f.create_dataset(pfx + 'image/pixels', data=img, chunks=shape, compression='gzip')
                f.create_dataset(pfx + 'gt-seg/pixels', data=seg, chunks=shape, compression='gzip')
                la = g.uniform(0, 20, size=(len(names), 2))
                for l, name in enumerate(names):
                    if drop != (spec, p, name):
                        f[pfx + 'gt-landmarks/' + name] = la[l].astype(np.float32)
                f[pfx + 'rot-180-for-up'] = np.int64(p % 2)
                data[(spec, p)] = (img, seg, p % 2, la.astype(np.float32))
    return data


def test_convert_file_overrides_and_refusals(tmp_path):
    from dfl_amd import dataset
    cwd = str(tmp_path)
    names = ['zz-extra', 'GSN-r', 'FH-l', 'aa-extra']
    specs = [('18-2800', 2), ('17-1882', 1), ('99-0001', 2)]
    data = _tiny_full_res(os.path.join(cwd, 'full.h5'), specs, names, dtypes={('18-2800', 1): np.uint16})
    # --specimens gives the numbering, --gzip compresses, f = 3 and crop 2 leave clipped boxes; the uint16 projection
    # shares a chunk with a float one
    out = _run('preprocess_full_res.py', ['full.h5', 'pre.h5', '--ds-factor', '3', '--crop', '2', '--specimens',
                                          '99-0001,18-2800', '--gzip', '--chunk', '8'], cwd)
    assert out.strip().split('\n') == ['99-0001 -> 01: 2 projections, 7 x 8', '18-2800 -> 02: 2 projections, 7 x 8']
    pre = os.path.join(cwd, 'pre.h5')
    assert dataset.get_land_names_from_dataset(pre) == ['FH-l', 'GSN-r', 'aa-extra', 'zz-extra']   # the reference's, then sorted
    order = [names.index(n) for n in ['FH-l', 'GSN-r', 'aa-extra', 'zz-extra']]
    with h5lite.File(pre, 'r') as f:
        assert sorted(f.keys()) == ['01', '02', 'land-names']
        for grp, spec in (('01', '99-0001'), ('02', '18-2800')):
            imgs, segs, rots, las = zip(*[data[(spec, p)] for p in range(2)])
            ref = PR.projs(np.stack([im.astype(np.float64) for im in imgs]), rots, 2, 3)
            assert float(np.abs(f[grp + '/projs'][()].astype(np.float64) - ref).max()) <= TOL
            assert np.array_equal(f[grp + '/segs'][()], PR.segs(np.stack(segs), rots, 2, 3))
            lands = np.stack(las).transpose(0, 2, 1)[:, :, order]
            assert np.array_equal(f[grp + '/lands'][()], PR.map_lands(lands, rots, 24, 28, 2, 3).astype(np.float32))
    # land_names overrides the order and the selection; specimens default to sorted ids (not the README's six)
    done = pp.convert_file(os.path.join(cwd, 'full.h5'), os.path.join(cwd, 'pre2.h5'), factor=2, crop=0, land_names=['GSN-r', 'FH-l'],
                           device=DEV)
    assert [(s, k, n) for s, k, n, _ in done] == [('17-1882', 1, 1), ('18-2800', 2, 2), ('99-0001', 3, 2)]
    assert dataset.get_land_names_from_dataset(os.path.join(cwd, 'pre2.h5')) == ['GSN-r', 'FH-l']
    # refusals: they name what is wrong
    with pytest.raises(nat.DflError, match='no specimen 00-0000'):
        pp.convert_file(os.path.join(cwd, 'full.h5'), os.path.join(cwd, 'x.h5'), specimens=['00-0000'], crop=2, device=DEV)
    _tiny_full_res(os.path.join(cwd, 'drop.h5'), specs, names, drop=('18-2800', 1, 'GSN-r'))
    with pytest.raises(nat.DflError, match='specimen 18-2800, projection 001 has no landmark GSN-r'):
        pp.convert_file(os.path.join(cwd, 'drop.h5'), os.path.join(cwd, 'x.h5'), crop=2, factor=3, device=DEV)
    _tiny_full_res(os.path.join(cwd, 'shape.h5'), specs, names, bad_shape=('99-0001', 0))
    with pytest.raises(nat.DflError, match='proj-params say'):
        pp.convert_file(os.path.join(cwd, 'shape.h5'), os.path.join(cwd, 'x.h5'), crop=2, factor=3, device=DEV)
