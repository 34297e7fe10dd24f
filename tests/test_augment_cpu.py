"""Host side of the device augmentation (no GPU): the numpy restatement's warp against PIL itself, the geometry of the
maps, the sampler's distributions and seeding, the tap bounds, and the Philox4x32-10 generator."""
import math

import numpy as np
import pytest

import dfl_amd
from dfl_amd import dataset as D
import aug_ref as A

IDENT = dict(angle=0.0, translate=(0.0, 0.0), scale=1.0, shear=(0.0, 0.0))


def _random_map(rng, W, H):
    prm = dict(angle=rng.uniform(-5, 5), translate=(rng.uniform(-5, 5), rng.uniform(-5, 5)), scale=rng.uniform(0.9, 1.1),
               shear=(rng.uniform(-1, 1), rng.uniform(-1, 1)))
    return A.inverse_affine_matrix((W * 0.5, H * 0.5), prm['angle'], prm['translate'], prm['scale'], prm['shear'])


def test_bilinear_and_nearest_models_match_pil():
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(0)
    n = bad_bl = bad_nn = 0
    far = []
    for _ in range(20):
        H, W = (int(v) for v in rng.integers(20, 80, 2))
        img = rng.integers(0, 256, (H, W), dtype=np.uint8)
        m = _random_map(rng, W, H)
        ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
        pil = np.asarray(Image.fromarray(img).transform((W, H), Image.AFFINE, data=tuple(m), resample=Image.BILINEAR))
        bad_bl += int((A.pil_bilinear(img, m, xs, ys) != pil).sum())
        pil = np.asarray(Image.fromarray(img).transform((W, H), Image.AFFINE, data=tuple(m), resample=Image.NEAREST))
        diff = A.pil_nearest(img, m, xs, ys) != pil
        sx, sy = A.source_coords(m, xs, ys)
        dist = np.minimum(np.abs(sx - np.round(sx)), np.abs(sy - np.round(sy)))
        far += list(dist[diff])
        bad_nn += int(diff.sum())
        n += H * W
    assert bad_bl == 0                                    # every pixel, border rules included
    # PIL's nearest runs in 16.16 fixed point: the floor model differs only next to integer source coordinates
    assert bad_nn <= 1e-3 * n and (not far or max(far) < 1e-3), (bad_nn, n, max(far) if far else None)


def test_dot_at_landmark_lands_on_the_warped_landmark():
    H = W = 64
    proj = np.zeros((H, W), np.float32)
    lx, ly = 30.0, 25.0
    proj[int(ly), int(lx)] = 1.0
    proj[int(ly) + 1, int(lx) + 1] = 1.0
    seg = np.zeros((H, W), np.uint8)
    lands = np.array([[lx + 0.5], [ly + 0.5]], np.float32)   # the centre of the 2x2 bright block
    prm = dict(flags=0, angle=4.0, translate=(6.0, -3.0), scale=1.07, shear=(0.5, -0.8), boxes=[])
    o = A.augment_item(proj, seg, lands, prm, 0, 4, land_rule='in_view', standardize=False)
    lev = o['levels'].astype(np.float64)
    yy, xx = np.nonzero(lev > 0)
    w = lev[yy, xx]
    cx, cy = (xx * w).sum() / w.sum(), (yy * w).sum() / w.sum()
    assert np.isfinite(o['lands']).all()
    assert abs(cx - o['lands'][0, 0]) < 1.0 and abs(cy - o['lands'][1, 0]) < 1.0


def test_pure_translation_moves_content_by_t():
    rng = np.random.default_rng(1)
    H = W = 40
    proj = rng.random((H, W)).astype(np.float32)
    proj[0, 0], proj[-1, -1] = 0.0, 1.0                   # min / max fixed: the quantisation is that of the input
    prm = dict(IDENT, flags=0, translate=(3.0, -2.0), boxes=[])
    o = A.augment_item(proj, None, None, prm, 0, 2, standardize=False)
    q = (proj * np.float32(255)).astype(np.uint8)
    assert np.array_equal(o['levels'][5:-5, 5:-5], q[7:-3, 2:-8])   # out[y, x] = in[y + 2, x - 3]


def test_identity_reproduces_the_quantised_input():
    rng = np.random.default_rng(2)
    H, W, pad = 30, 34, 2
    proj = (rng.random((H, W)) * 500 + 20).astype(np.float32)
    prm = dict(IDENT, flags=0, boxes=[])
    o = A.augment_item(proj, rng.integers(0, 3, (H, W)).astype(np.uint8), None, prm, pad, 3, standardize=False)
    mn, mx = proj.min(), proj.max()
    q = (((proj - mn) / np.float32(mx - mn)) * np.float32(255)).astype(np.uint8)
    assert np.array_equal(o['levels'], np.pad(q, pad, 'reflect'))


def test_sampler_distributions():
    n, H, W = 20000, 192, 192
    ps = D.DeviceAugment(11).draw(n, H, W)
    aug = [p for p in ps if p is not None]

    def within(count, total, prob):
        return abs(count - total * prob) <= 5 * math.sqrt(total * prob * (1 - prob))
    assert within(len(aug), n, 0.5)
    m = len(aug)
    assert within(sum(1 for p in aug if p['flags'] & A.INVERT), m, 0.5)
    erased = [p for p in aug if p['flags'] & A.ERASE]
    assert within(len(erased), m, 0.25)
    counts = np.bincount([len(p['boxes']) for p in erased], minlength=6)
    assert counts[0] == 0 and all(within(counts[k], len(erased), 0.2) for k in range(1, 6))
    for p in aug:
        assert p['flags'] & A.NOISE and p['flags'] & A.GAMMA
        assert 0.005 <= p['sigma'] <= 0.01 and 0.7 <= p['gamma'] <= 1.3 and -5 <= p['angle'] <= 5
        assert 0.9 <= p['scale'] <= 1.1 and all(-1 <= s <= 1 for s in p['shear'])
        assert math.hypot(*p['translate']) <= 20.0
        for (r0, c0, nr, nc, key) in p['boxes']:
            assert 0 < nr <= H and 0 < nc <= W and 0 <= r0 <= H - nr and 0 <= c0 <= W - nc and 0 <= key < 1 << 64
    for key, lo, hi in (('sigma', 0.005, 0.01), ('gamma', 0.7, 1.3), ('angle', -5, 5), ('scale', 0.9, 1.1)):
        v = np.array([p[key] for p in aug])
        sd = (hi - lo) / math.sqrt(12)
        assert abs(v.mean() - (lo + hi) / 2) <= 5 * sd / math.sqrt(m), key
    t = np.array([p['translate'] for p in aug])
    mag = np.hypot(t[:, 0], t[:, 1])
    assert abs(mag.mean() - 10.0) <= 5 * (20 / math.sqrt(12)) / math.sqrt(m)
    # direction uniform on the circle: Kolmogorov-Smirnov against U(-pi, pi)
    ang = np.sort(np.arctan2(t[:, 1], t[:, 0]))
    cdf = (ang + math.pi) / (2 * math.pi)
    k = np.arange(1, m + 1)
    ks = max((k / m - cdf).max(), (cdf - (k - 1) / m).max())
    assert ks < 1.63 / math.sqrt(m)                       # 1 % level
    # box sides: round(N(0,1) 0.15 n + 0.15 n), truncated to (0, n]: the mean of the accepted sides
    sides = np.array([b[2] for p in erased for b in p['boxes']], np.float64)
    mu, s = 0.15 * H, 0.15 * H
    z = np.random.default_rng(0).standard_normal(400000) * s + mu
    z = np.round(z)
    z = z[(z > 0) & (z <= H)]
    assert abs(sides.mean() - z.mean()) <= 5 * z.std() / math.sqrt(len(sides))


def test_sampler_seeding_epochs_and_ranks():
    a, b = D.DeviceAugment(5), D.DeviceAugment(5)
    assert a.draw(300, 64, 64) == b.draw(300, 64, 64)
    assert a.params([3, 1, 7], 300, 64, 64) == [b.draw(300, 64, 64)[i] for i in (3, 1, 7)]
    a.set_epoch(1)
    assert a.draw(300, 64, 64) != b.draw(300, 64, 64)
    b.set_epoch(1)
    assert a.draw(300, 64, 64) == b.draw(300, 64, 64)
    assert D.DeviceAugment(5, rank=1).draw(300, 64, 64) != D.DeviceAugment(5, rank=0).draw(300, 64, 64)
    assert D.DeviceAugment(6).draw(300, 64, 64) != D.DeviceAugment(5).draw(300, 64, 64)
    assert all(p is None for p in D.DeviceAugment(5, prob=0.0).draw(300, 64, 64))
    with pytest.raises(ValueError):
        D.DeviceAugment(5, land_rule='nearby')


def test_table_maps_match_the_restatement():
    rng = np.random.default_rng(3)
    for (H, W, pad) in ((46, 46, 0), (184, 184, 4), (37, 53, 3)):
        for has_seg in (True, False):
            prm = dict(flags=15, sigma=0.007, gamma=1.1, angle=rng.uniform(-5, 5), translate=tuple(rng.uniform(-14, 14, 2)),
                       scale=rng.uniform(0.9, 1.1), shear=tuple(rng.uniform(-1, 1, 2)), noise_key=12345,
                       boxes=[(1, 2, 3, 4, 99)])
            it = D.DeviceAugment.item(prm, 2, H, W, pad, has_seg)
            img, seg, land = A.maps(H, W, pad, prm, has_seg)
            np.testing.assert_allclose(np.array(it.img_map), img, rtol=0, atol=1e-12)
            np.testing.assert_allclose(np.array(it.seg_map), seg, rtol=0, atol=1e-12)
            np.testing.assert_allclose(np.array(it.land_map), land, rtol=0, atol=1e-12)
            assert it.row == 2 and it.flags == 15 and it.n_box == 1 and list(it.box[0]) == [1, 2, 3, 4] and it.box_key[0] == 99
    with pytest.raises(ValueError):
        D.DeviceAugment.item(dict(prm, boxes=[(0, 0, 500, 4, 1)]), 0, 46, 46, 0, True)


def _corners():
    for ang in (-5.0, 5.0):
        for sx in (-1.0, 1.0):
            for sy in (-1.0, 1.0):
                for s in (0.9, 1.1):
                    for k in range(16):
                        th = 2 * math.pi * k / 16
                        yield dict(angle=ang, shear=(sx, sy), scale=s, translate=(20 * math.cos(th), 20 * math.sin(th)))


def test_taps_inside_the_padded_image_at_the_corners_of_the_parameter_box():
    # the paper preset (184 x 184 images padded to 192) and 192 x 192: PIL's border rules never apply
    for H, pad in ((184, 4), (192, 0), (192, 2)):
        assert all(A.taps_inside(H, H, pad, p) for p in _corners()), H
    # small images: the warp reaches past the reflect padding, where PIL's rules (fill 0, clamped taps) hold -- the
    # kernel and the restatement implement them, and the fixtures at 46 x 46 cover them
    assert not all(A.taps_inside(46, 46, 0, p) for p in _corners())


def test_philox_known_answers_and_box_muller():
    # Random123 known-answer vectors of philox4x32 with 10 rounds
    assert [int(v) for v in A.philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert [int(v) for v in A.philox4x32_10(*([0xffffffff] * 6))] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert [int(v) for v in A.philox4x32_10(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)] == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    z = A.normals(0x0123456789abcdef, np.arange(200000)).astype(np.float64)
    se = 1 / math.sqrt(z.size)
    assert abs(z.mean()) < 5 * se and abs(z.std() - 1) < 5 * se and np.isfinite(z).all()
    assert not np.array_equal(A.normals(1, np.arange(16)), A.normals(2, np.arange(16)))


def test_data_aug_keyword_still_refuses_and_points_to_augment():
    with pytest.raises(NotImplementedError, match='augment=DeviceAugment'):
        D.get_dataset('unused.npz', [1], 7, data_aug=True)
    with pytest.raises(TypeError):
        D.get_dataset('unused.npz', [1], 7, augment=object())
    assert dfl_amd.DeviceAugment is D.DeviceAugment
