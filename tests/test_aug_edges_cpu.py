"""The case table of the augmentation edge tests (tests/test_gpu_aug_edges.py runs it through dfl_augment_batch) and what
keeps it honest without a GPU: every border rule of PIL's warp, every reflection depth, every flag combination and every
landmark boundary is in the table, the gamma cases keep their ambiguous quantisation steps rare, and the restatement
(tests/aug_ref.py) still returns the stored arrays of fixture aug_46_p0.

A case: H, W, pad, C, L, flags, warp (affine parameters) or maps (18 explicit doubles), boxes, keys, the image family
('unit': random fp32 with minimum exactly 0 and maximum exactly 1; 'offset': the same times 3 minus 2), the label map
('plain': 0..C-1, 'foreign': with values >= C and 255), the landmarks ('random' or 'edges') and a seed that picks the random
image (for five of the 37 x 53 gamma cases one that keeps the gamma window under 0.5 %: at that size the two pixels that
are exactly 0 and 1 alone, tapped by four output pixels each, are 0.29 %)."""
import math
import zlib

import numpy as np
import pytest

from conftest import load_golden
import aug_ref as A

F32 = np.float32
IDENT = dict(angle=0.0, translate=(0.0, 0.0), scale=1.0, shear=(0.0, 0.0))
K63, K64 = 1 << 63, (1 << 64) - 1
SKEW = dict(angle=33.0, shear=(20.0, -10.0))


def _warp(**kw):
    return dict(IDENT, **kw)


def _case(name, H, W, pad, flags, warp=None, maps=None, C=3, L=3, boxes=(), family=None, labels='plain', lands='random',
          noise_key=0x0123456789abcdef, sigma=0.01, gamma=0.7, seed=0):
    if family is None:
        family = 'unit' if flags & A.GAMMA else 'offset'
    return dict(name=name, H=H, W=W, pad=pad, flags=flags, warp=warp, maps=maps, C=C, L=L, boxes=list(boxes), family=family,
                labels=labels, lands=lands, noise_key=noise_key, sigma=sigma, gamma=gamma, seed=seed)


def _point_maps(H, W, pad, special):
    """Explicit maps around the identity: `special` = {(map index, entry): value} overrides single entries."""
    m = [np.array(v, np.float64) for v in A.maps(H, W, pad, IDENT)]
    for (k, e), v in special.items():
        m[k][e] = v
    return tuple(m)


def _one_point(H, W, pad):
    """An all-zero linear part: every output pixel reads the same source point, every landmark lands on (3, 4)."""
    ch, cw = (H + 1) // 2, (W + 1) // 2
    return (np.array([0, 0, cw + pad + 2.25, 0, 0, ch + pad + 3.75]), np.array([0, 0, cw + 1.5, 0, 0, ch + 2.5]),
            np.array([0, 0, 3.0, 0, 0, 4.0]))


CASES = [
    # the smallest images: pad 4 makes the reflect pad larger than the image
    _case('2x2_p0_identity', 2, 2, 0, 0, _warp(), C=2, L=1, noise_key=0),
    _case('2x2_p4_invert', 2, 2, 4, 1, _warp(), noise_key=1),
    _case('2x3_p0_half_pixel', 2, 3, 0, 2, _warp(translate=(0.5, -0.5)), noise_key=(1 << 32) - 1),
    _case('2x3_p4_integer_shift', 2, 3, 4, 3, _warp(translate=(1.0, -2.0)), noise_key=1 << 32),
    _case('3x2_p0_rot90', 3, 2, 0, 8, _warp(angle=90.0), boxes=[(0, 0, 2, 2, K63), (1, 1, 2, 1, 5)]),
    _case('3x2_p4_fill_strips', 3, 2, 4, 9, _warp(translate=(5.5, -6.25)), boxes=[(2, 3, 5, 4, K64)]),
    # landmark boundaries under the identity map, labels >= C
    _case('5x7_p1_land_edges', 5, 7, 1, 0, _warp(), C=3, L=16, labels='foreign', lands='edges'),
    _case('5x7_p1_all_outside', 5, 7, 1, 10, _warp(translate=(1000.0, 0.0)), boxes=[(0, 0, 3, 3, 9)], noise_key=K63),
    _case('5x7_p1_quarter', 5, 7, 1, 11, _warp(scale=0.25, translate=(0.3, 0.6)), boxes=[(6, 8, 1, 1, 3)], noise_key=K64),
    _case('16x16_p0_quarter', 16, 16, 0, 0, _warp(scale=0.25, translate=(2.3, -1.7)), C=254, labels='foreign'),
    _case('16x16_p0_half', 16, 16, 0, 2, _warp(scale=0.5, translate=(-7.25, 7.75))),
    _case('16x16_p0_zoom4', 16, 16, 0, 1, _warp(scale=4.0, translate=(0.25, 0.75))),
    _case('16x16_p0_skew', 16, 16, 0, 3, _warp(scale=0.5, translate=(3.5, 2.5), **SKEW), L=14),
    # explicit maps: non-finite and huge entries, one source point
    _case('16x16_p0_nan_map', 16, 16, 0, 0, maps=_point_maps(16, 16, 0, {(0, 1): math.nan, (2, 5): math.nan})),
    _case('16x16_p0_inf_map', 16, 16, 0, 8, maps=_point_maps(16, 16, 0, {(1, 2): math.inf, (2, 0): math.inf}),
          boxes=[(3, 3, 4, 4, 77)]),
    _case('16x16_p0_huge_map', 16, 16, 0, 0, maps=_point_maps(16, 16, 0, {(0, 0): 1e300, (2, 4): 1e300})),
    _case('16x16_p0_one_point', 16, 16, 0, 2, maps=_one_point(16, 16, 0)),
    # 37 x 53 pad 4: every border rule of the bilinear warp in one picture
    _case('37x53_p4_skew_quarter', 37, 53, 4, 0, _warp(scale=0.25, translate=(9.5, -14.25), **SKEW), C=5, L=4),
    _case('37x53_p4_rot90', 37, 53, 4, 9, _warp(angle=90.0, translate=(0.5, 0.0)),
          boxes=[(0, 0, 45, 61, 11), (44, 60, 1, 1, 12)]),
    # more than 64 * 256 pixels: a second stride in every statistics slice
    _case('129x128_p0_identity', 129, 128, 0, 0, _warp()),
    _case('129x128_p0_all_steps', 129, 128, 0, 11, _warp(scale=0.5, translate=(30.5, -20.25), **SKEW), C=2, L=14,
          boxes=[(100, 90, 29, 38, 21), (0, 0, 1, 128, 22), (5, 7, 129 - 5, 1, 23)]),
    # gamma: 'unit' images, large enough that the two exact levels (0 and 255) and the window stay rare
    _case('37x53_p4_gamma', 37, 53, 4, 4, _warp(), gamma=0.7, seed=2),
    _case('37x53_p4_gamma_invert', 37, 53, 4, 5, _warp(translate=(3.0, -2.0)), gamma=1.3, seed=7),
    _case('37x53_p4_gamma_noise', 37, 53, 4, 6, _warp(translate=(0.5, 0.5)), gamma=1.3, noise_key=K63 + 1, seed=1),
    _case('129x128_p0_gamma_noise_invert', 129, 128, 0, 7, _warp(scale=0.5, translate=(1.25, -0.75)), gamma=0.7),
    _case('37x53_p4_gamma_erase', 37, 53, 4, 12, _warp(angle=33.0), gamma=0.7, seed=7,
          boxes=[(3, 4, 10, 20, 31), (8, 14, 30, 40, 32)]),
    _case('37x53_p4_gamma_erase_invert', 37, 53, 4, 13, _warp(scale=0.5, translate=(-4.5, 6.25)), gamma=1.3, seed=1,
          boxes=[(0, 0, 45, 61, 33)]),
    _case('129x128_p0_gamma_erase_noise', 129, 128, 0, 14, _warp(angle=90.0), gamma=1.3, boxes=[(64, 64, 65, 64, 34)]),
    _case('37x53_p4_gamma_all_steps', 37, 53, 4, 15, _warp(scale=0.25, translate=(9.5, -14.25), **SKEW), gamma=0.7, C=5, L=4,
          boxes=[(1, 1, 5, 5, 41), (2, 2, 9, 3, 42), (40, 50, 5, 11, 43), (20, 0, 1, 61, 44), (0, 30, 45, 1, 45)]),
]
BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def land_edges(H, W, C):
    """[2, 16] landmarks that sit, under the identity map, exactly on and one float32 step beyond every boundary of the
    two drop rules (reference: x < 0, x > H-1, y < 0, y < C-1; in view: outside [0, W-1] x [0, H-1]), then inf in x only,
    inf in y only, a NaN and -inf."""
    up = lambda v: np.nextafter(F32(v), F32(np.inf))       # noqa: E731
    dn = lambda v: np.nextafter(F32(v), F32(-np.inf))      # noqa: E731
    pts = [(0, C - 1), (dn(0), C - 1), (H - 1, C - 1), (up(H - 1), C - 1), (W - 1, H - 1), (up(W - 1), H - 1), (0, 0), (0, dn(0)),
           (1, H - 1), (1, up(H - 1)), (1, C - 1), (1, dn(C - 1)), (np.inf, 2), (2, np.inf), (np.nan, 2), (-np.inf, 1)]
    return np.array(pts, F32).T.copy()


def build(c):
    """The inputs of a case: proj [H,W] fp32, seg [H,W] uint8, lands [2,L] fp32 and the parameter dict of aug_ref."""
    H, W, C, L = c['H'], c['W'], c['C'], c['L']
    rng = np.random.default_rng(zlib.crc32(c['name'].encode()) + c['seed'])
    proj = rng.random((H, W), dtype=F32)
    proj.flat[int(proj.argmin())] = 0.0
    proj.flat[int(proj.argmax())] = 1.0
    if c['family'] == 'offset':
        proj = proj * F32(3.0) - F32(2.0)
    seg = rng.integers(0, C, (H, W)).astype(np.uint8)
    if c['labels'] == 'foreign':
        k = max(H * W // 8, 1)
        seg.flat[rng.choice(H * W, 3 * k, replace=False)] = np.repeat(np.array([C, 255, min(C + 50, 255)], np.uint8), k)
    if c['lands'] == 'edges':
        lands = land_edges(H, W, C)
        assert lands.shape[1] == L
    else:
        lands = np.stack([rng.uniform(-2, W + 1, L), rng.uniform(-2, H + 1, L)]).astype(F32)
    prm = dict(c['warp'] or IDENT, flags=c['flags'], sigma=c['sigma'], gamma=c['gamma'], noise_key=c['noise_key'],
               boxes=list(c['boxes']), maps=c['maps'])
    return dict(proj=proj, seg=seg, lands=lands, prm=prm)


_MODEL = {}


def model(name, normals_fn=None, **kw):
    """augment_item of a case (raw image, reference rule); with the restated normals it is computed once and shared."""
    c = BY_NAME[name]
    if normals_fn is None and not kw:
        if name not in _MODEL:
            b = build(c)
            _MODEL[name] = A.augment_item(b['proj'], b['seg'], b['lands'], b['prm'], c['pad'], c['C'], standardize=False)
        return _MODEL[name]
    b = build(c)
    kw.setdefault('standardize', False)
    return A.augment_item(b['proj'], b['seg'], b['lands'], b['prm'], c['pad'], c['C'], normals_fn=normals_fn or A.normals, **kw)


# ---- the table ---------------------------------------------------------------------------------------------------------------
def test_images_span_exactly_zero_to_one_and_shapes_are_the_smallest():
    shapes = set()
    for c in CASES:
        p = build(c)['proj']
        lo, hi = (0.0, 1.0) if c['family'] == 'unit' else (-2.0, 1.0)
        assert p.dtype == F32 and p.min() == lo and p.max() == hi and len(np.unique(p)) > 1
        assert c['family'] == 'unit' or not c['flags'] & A.GAMMA
        shapes.add((c['H'], c['W'], c['pad']))
    assert {(2, 2, 0), (2, 2, 4), (2, 3, 0), (2, 3, 4), (3, 2, 0), (3, 2, 4), (5, 7, 1), (16, 16, 0), (37, 53, 4), (129, 128, 0)} == shapes
    assert 129 * 128 > 64 * 256 and max(c['H'] * c['W'] for c in CASES) == 129 * 128 and max(c['L'] for c in CASES) <= 16


def test_every_tap_path_occurs_in_at_least_two_cases():
    hit = {k: [] for k in ('outside', 'dropped', 'clamp_x', 'clamp_y', 'reflect2')}
    for c in CASES:
        rep = A.tap_report(c['H'], c['W'], c['pad'], build(c)['prm'])
        counts = {k: int(v.sum()) for k, v in rep.items()}
        print('TAPS %-32s %s of %d' % (c['name'], counts, rep['outside'].size))
        for k, n in counts.items():
            if n:
                hit[k].append(c['name'])
    for k, names in hit.items():
        assert len(names) >= 2, (k, names)
    # the two configurations the issue names
    rep = A.tap_report(37, 53, 4, build(BY_NAME['37x53_p4_skew_quarter'])['prm'])
    assert all(rep[k].any() for k in ('outside', 'dropped', 'clamp_x', 'clamp_y'))
    rep = A.tap_report(2, 2, 4, build(BY_NAME['2x2_p4_invert'])['prm'])
    assert rep['reflect2'].sum() > 50 and not rep['outside'].any()
    # entirely outside: one affine case and the maps with a non-finite or huge entry
    for name in ('5x7_p1_all_outside', '16x16_p0_nan_map', '16x16_p0_huge_map'):
        c = BY_NAME[name]
        assert A.tap_report(c['H'], c['W'], c['pad'], build(c)['prm'])['outside'].all(), name
        assert not model(name)['levels'].any()
    one = model('16x16_p0_one_point')
    assert len(np.unique(one['levels'])) == 1 and len(np.unique(one['labels'])) == 1


def test_label_255_foreign_labels_and_class_counts():
    with255 = [c['name'] for c in CASES if (model(c['name'])['labels'] == 255).any()]
    assert len(with255) >= 3, with255
    assert (model('16x16_p0_inf_map')['labels'] == 255).all()
    assert {2, 254} <= {c['C'] for c in CASES}
    for name in ('5x7_p1_land_edges', '16x16_p0_quarter'):
        C = BY_NAME[name]['C']
        seg = build(BY_NAME[name])['seg']
        assert (seg == 255).any() and ((seg >= C) & (seg < 255)).any()
        o = model(name)
        assert (o['labels'] >= C).any() and np.array_equal(o['masks'].sum(0), (o['labels'] < C).astype(F32))


def test_every_flag_combination_and_landmark_count():
    assert {c['flags'] for c in CASES} == set(range(16))
    assert 1 in {c['L'] for c in CASES} and max(c['L'] for c in CASES) >= 14
    for c in CASES:
        assert bool(c['boxes']) == bool(c['flags'] & A.ERASE), c['name']


def test_gamma_cases_keep_the_window_rare():
    """A condition on the inputs: at most 0.5 % of the output pixels of a gamma case read a tap whose level two powf may
    truncate differently (aug_ref.gamma_window)."""
    n = 0
    for c in CASES:
        if c['flags'] & A.GAMMA:
            plane, share_src = A.gamma_window(build(c)['proj'], build(c)['prm'], c['pad'])
            print('WINDOW %-32s %d of %d output pixels (%.3f %%), %.3f %% of the source pixels' % (
                c['name'], int(plane.sum()), plane.size, 100 * plane.mean(), 100 * share_src))
            assert plane.mean() <= 0.005, c['name']
            n += 1
    assert n == 8


def test_landmark_edges_sit_on_the_boundaries():
    c = BY_NAME['5x7_p1_land_edges']
    H, W, C = c['H'], c['W'], c['C']
    b = build(c)
    ln = b['lands']
    assert np.array_equal(A.case_maps(H, W, c['pad'], b['prm'])[2], np.array([1.0, 0, 0, 0, 1, 0]))     # the identity, exactly
    xs, ys = list(ln[0]), list(ln[1])
    for v in (0, H - 1, W - 1):
        assert F32(v) in xs and (np.nextafter(F32(v), F32(np.inf)) in xs or np.nextafter(F32(v), F32(-np.inf)) in xs)
    for v in (0, H - 1, C - 1):
        assert F32(v) in ys and (np.nextafter(F32(v), F32(np.inf)) in ys or np.nextafter(F32(v), F32(-np.inf)) in ys)
    assert np.isinf(ln[0, 12]) and np.isfinite(ln[1, 12]) and np.isfinite(ln[0, 13]) and np.isinf(ln[1, 13])
    assert np.isnan(ln).sum() == 1
    kept = {}
    for rule in ('reference', 'in_view', None):
        o = model(c['name'], land_rule=rule)['lands']
        kept[rule] = [bool(np.isfinite(o[:, l]).all()) for l in range(12)]
        # dataset.py:242: a pair with an inf coordinate stays as it is; a NaN is mapped (and stays NaN)
        assert np.array_equal(o[:, [12, 13, 15]].view(np.uint32), ln[:, [12, 13, 15]].view(np.uint32))
        assert np.isnan(o[:, 14]).all()
    t, f = True, False
    assert kept['reference'] == [t, f, t, f, f, f, f, f, t, t, t, f]
    assert kept['in_view'] == [t, f, t, t, t, f, t, f, t, f, t, t]
    assert all(kept[None])


def test_erase_rule_of_the_header():
    full = [(0, 0, 2, 2, 1), (1, 1, 0, 2, 2), (0, 0, 1, 1, 3)]
    assert A.erase_boxes(dict(boxes=full), 4, 4) == full[:1]                 # a non-positive side ends the list
    assert A.erase_boxes(dict(boxes=[(0, 0, 2, 2, 1), (3, 0, 2, 1, 2)]), 4, 4) == [(0, 0, 2, 2, 1)]     # one row too far
    assert A.erase_boxes(dict(boxes=[(0, 0, 4, 4, k) for k in range(7)]), 4, 4) == [(0, 0, 4, 4, k) for k in range(5)]
    assert A.erase_boxes(dict(boxes=[(-1, 0, 1, 1, 1)]), 4, 4) == []


def test_reflection_beyond_one_period_is_numpy_reflect():
    for n in (2, 3, 5):
        i = np.arange(-4 * n, 5 * n)
        want = np.pad(np.arange(n), (4 * n, 4 * n), 'reflect')[i + 4 * n]
        assert np.array_equal(A.reflect_index(i, n), want)


# ---- the restatement has not moved -------------------------------------------------------------------------------------------
def test_restatement_still_returns_fixture_aug_46_p0():
    g = load_golden('aug_46_p0')
    pad, C = int(g['pad']), int(g['C'])
    for i, prm in enumerate(A.load_params(g)):
        o = A.augment_item(g['projs'][i], g['segs'][i], g['lands'][i], prm, pad, C, land_rule='reference')
        o2 = A.augment_item(g['projs'][i], g['segs'][i], g['lands'][i], prm, pad, C, land_rule='in_view')
        assert np.array_equal(o['levels'], g['levels'][i]), i
        assert np.array_equal(o['labels'], g['labels'][i]), i
        assert np.array_equal(o['lands'].view(np.uint32), g['lands_reference'][i].view(np.uint32)), i
        assert np.array_equal(o2['lands'].view(np.uint32), g['lands_in_view'][i].view(np.uint32)), i
