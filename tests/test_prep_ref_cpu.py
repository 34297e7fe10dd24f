"""tests/prep_ref.py -- the float64 models that the kernels of csrc/prep.hip are held against (tests/test_gpu_prep.py) -- against
oracle/ref_cpu.py on random data and against the goldens 'dataset' and 'est_lands'; and the cases the GPU test runs against the
regimes of the launch geometry they are named after.  Runs without a GPU."""
import math

import numpy as np
import pytest
import torch

import prep_ref as PR
from conftest import load_golden
from oracle import ref_cpu as R

# csrc: prep.hip
PREP_NB = 64                    # prep_stats_kernel: statistics slices (workgroups of 256) per image
PREP_WRITE_PER_THREAD = 4       # dfl_prep_batch: ceil(n / (256 * 4)) workgroups ...
PREP_WRITE_CAP = 1024           # ... capped at 1024
LM_SCAN_NB = 64                 # est_lands_scan_kernel: workgroups of 256 per map
LM_SCAN_U = 8                   # ... and loads in flight per thread and trip (constexpr U)
DICE_PER_THREAD = 16            # dfl_hard_dice: ceil(pixels / (256 * 16)) workgroups ...
DICE_CAP = 256                  # ... capped at 256
WG = 256

SLOT = LM_SCAN_NB * WG          # pixels between two unroll slots of a thread:            16384
TRIP = SLOT * LM_SCAN_U         # pixels one trip of the outer loop covers:              131072
F32_EPS = 2.0 ** -23


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def scan_coords(i):
    """(workgroup, thread, unroll slot, outer trip) that reads flat index i in est_lands_scan_kernel."""
    return (i // WG) % LM_SCAN_NB, i % WG, (i // SLOT) % LM_SCAN_U, i // TRIP


# ---------------------------------------------------------------------------------------------------- models vs oracle
@pytest.mark.parametrize('H,W,pad', [(20, 31, 0), (37, 53, 36), (46, 46, 1), (2, 2, 1)])
def test_standardize_is_the_oracles_preprocess_proj(H, W, pad):
    img = PR.prep_images('uniform', 2, H, W)
    for b in range(2):
        x, m, sd = PR.standardize(img[b], pad)
        p = PR.reflect_pad(img[b], pad)
        assert np.array_equal(p, torch.nn.functional.pad(_t(img[b])[None, None], (pad,) * 4, mode='reflect')[0, 0].numpy()
                              if pad else img[b])
        want = R.preprocess_proj(_t(img[b])[None].double(), pad)[0].numpy()          # the oracle's formula in float64
        assert np.abs(x - want).max() <= 1e-12 * np.abs(want).max()
        want32 = R.preprocess_proj(_t(img[b])[None], pad)[0].numpy()                 # and as the oracle runs it
        assert np.abs(x - want32).max() <= 64 * F32_EPS * (np.abs(want32).max() + abs(m) / sd)
        assert abs(m - p.astype(np.float64).mean()) <= 1e-12 * abs(m) and abs(sd - p.astype(np.float64).std(ddof=1)) <= 1e-12 * sd


def test_standardize_of_a_high_offset_image_keeps_its_digits():
    """The two-pass form loses nothing at mean / spread = 10^5; that is what makes it the reference for the one-pass kernel."""
    img = PR.prep_images('offset', 1, 37, 53)[0]
    x, m, sd = PR.standardize(img, 3)
    p = PR.reflect_pad(img, 3).astype(np.float64)
    assert abs(m - 60000.0) < 0.1 and 0.4 < sd < 0.6
    q = p - 60000.0                                             # exact in float64: the same statistics without the offset
    assert abs(sd - q.std(ddof=1)) <= 1e-13 * sd and np.abs(x - (q - q.mean()) / q.std(ddof=1)).max() <= 1e-9


def test_one_hot_and_heat_are_the_oracles():
    g = load_golden('dataset')
    H, W = g['projs'].shape[-2:]
    marked = R.mark_oob_landmarks(_t(g['lands']), H, W)
    for i in range(3):
        x, _, _ = PR.standardize(g['projs'][i], int(g['pad_48_46']))
        assert np.abs(x - g['item%d_p' % i][0]).max() <= 16 * F32_EPS * np.abs(x).max()
        assert np.array_equal(PR.one_hot(g['segs'][i], 7), g['item%d_s' % i])
        maps, e = PR.heat(g['lands'][i], H, W, 2.5)
        want = g['item%d_h' % i][:, 0]
        assert np.abs(maps - want).max() <= 16 * F32_EPS * np.abs(want).max()
        assert np.array_equal(maps.reshape(14, -1).max(1) == 0, np.isinf(marked[i].numpy()).any(0))
        assert np.array_equal(maps.reshape(14, -1).max(1) == 0, want.reshape(14, -1).max(1) == 0)
    labels = PR.prep_labels(2, 20, 31, 7, foreign=(200, 255))
    assert np.array_equal(np.stack([PR.one_hot(l, 7) for l in labels]), R.one_hot_masks(_t(labels).long(), 7).numpy())
    assert (labels >= 7).any() and float(PR.one_hot(labels[0], 7)[:, labels[0] >= 7].max()) == 0.0


@pytest.mark.parametrize('H,W', [(2, 2), (20, 31), (37, 53)])
@pytest.mark.parametrize('sigma', [2.5, 1.0])
def test_heat_view_rule_and_values(H, W, sigma):
    lands, view = PR.prep_lands(3, H, W, 14)
    assert view.sum() == 3 * 6 and (~view).sum() == 3 * 8
    marked = R.mark_oob_landmarks(_t(lands), H, W)
    for b in range(3):
        maps, e = PR.heat(lands[b], H, W, sigma)
        want = R.gaussian_heatmaps(marked[b], H, W, sigma)[:, 0].numpy()
        for l in range(14):
            finite = bool(np.isfinite(lands[b, :, l]).all())
            if view[b, l]:
                assert maps[l].max() > 0 and np.abs(maps[l] - want[l]).max() <= 64 * F32_EPS * want[l].max()
                mx, my = float(lands[b, 0, l]), float(lands[b, 1, l])
                r, c = min(H - 1, 1), W - 1
                assert e[l, r, c] == -((c - mx) ** 2 + (r - my) ** 2) / (2.0 * sigma * sigma)
                full = math.exp(e[l, r, c]) / (2.0 * math.pi * sigma * sigma)
                assert abs(maps[l, r, c] - full) <= 1e-15 * full
            else:
                assert maps[l].max() == 0.0 and e[l].max() == 0.0 and e[l].min() == 0.0
                if finite:                                      # (the oracle's own map is NaN for a NaN landmark: out of its contract)
                    assert want[l].max() == 0.0
    ent = PR.land_entries(H, W)
    assert [PR.in_view(mx, my, H, W) for mx, my, _ in ent] == [ok for _, _, ok in ent]
    # one float32 step outside on each side, and the boundary itself
    assert ent[3][0] < 0 and ent[4][1] < 0 and ent[5][0] > W - 1 and ent[6][1] > H - 1
    assert ent[5][0] - np.float32(W - 1) <= np.spacing(np.float32(W - 1)) and np.signbit(ent[1][0]) and ent[1][0] == 0


def test_est_lands_is_the_oracles_on_the_golden():
    g = load_golden('est_lands')
    labels = [int(v) for v in g['label_for_land']]
    rc, ncc, _, _ = PR.est_lands(g['heats'], g['segs'], labels)
    assert np.array_equal(rc, g['rc_masked'])
    assert np.array_equal(PR.est_lands(g['heats'])[0], g['rc_plain'])
    want, wncc = R.est_landmarks(_t(g['heats']), _t(g['segs']), labels, return_ncc=True)
    assert np.array_equal(rc, want.numpy()) and np.abs(ncc - wncc.numpy()).max() <= 2e-5
    w64 = R.est_landmarks(_t(g['heats']).double(), _t(g['segs']), labels, return_ncc=True)[1]
    assert np.abs(ncc - w64.numpy()).max() <= 64 * F32_EPS          # (the oracle stores its correlations as float32)


@pytest.mark.parametrize('H,W', PR.EST_SHAPES[:4])
def test_est_lands_is_the_oracles_on_the_peak_cases(H, W):
    heats, _ = PR.peak_case(H, W)
    rc, ncc, amp_y, amp_t = PR.est_lands(heats)
    want, wncc = R.est_landmarks(_t(heats).double(), return_ncc=True)
    assert np.array_equal(rc, want.numpy()) and np.abs(ncc - wncc.numpy()).max() <= 64 * F32_EPS
    assert np.isfinite(amp_y).all() and (amp_y >= 1.0).all() and np.allclose(amp_t, amp_t[0, 0]) and 1.0 < amp_t[0, 0] < 20.0


def test_est_lands_is_the_oracles_on_the_masked_case():
    heats, segs, lab = PR.masked_case(64, 80)
    for min_ncc in (PR.EST_MIN_NCC, -2.0):
        rc, ncc, _, _ = PR.est_lands(heats, segs, lab, min_ncc=min_ncc)
        want, wncc = R.est_landmarks(_t(heats).double(), _t(segs), [int(v) for v in lab], min_ncc=min_ncc, return_ncc=True)
        assert np.array_equal(rc, want.numpy()) and np.abs(ncc - wncc.numpy()).max() <= 64 * F32_EPS
    # what the case is there for
    assert (segs[0] == 5).any() and not (segs[1] == 5).any() and not (segs == 9).any()
    assert (segs == 200).any() and (segs == 255).any()
    assert [np.flatnonzero(segs[b].ravel() == 4).tolist() for b in range(2)] == [[64 * 80 - 1]] * 2
    assert (lab < 0).sum() == 2
    l5, l9, l4 = list(lab).index(5), list(lab).index(9), list(lab).index(4)
    assert rc[0, l5].min() >= 0 and rc[1, l5].tolist() == [-1, -1] and ncc[1, l5] == 0.0      # min_ncc = -2: only presence decides
    assert rc[:, l9].max() == -1 and rc[:, l4].tolist() == [[63, 79]] * 2
    assert np.array_equal(PR.est_lands(heats, segs, None)[0], PR.est_lands(heats)[0])
    assert np.array_equal(PR.est_lands(heats, None, lab)[0], PR.est_lands(heats)[0])


def test_hard_dice_is_the_oracles():
    for pixels, B, C, kind in [(70 * 90, 3, 7, 'random'), (70 * 90, 3, 7, 'special'), (70 * 90, 1, 7, 'foreign'), (257, 3, 2, 'random'),
                               (70 * 90, 1, 256, 'random'), (1, 1, 2, 'random')]:
        est, gt = PR.dice_case(pixels, B, C, kind)
        counts, dice = PR.dice_counts(est, gt, C)
        for b in range(B):
            assert dice[b] == R.hard_dice(_t(est[b]), _t(gt[b]), C)
            assert sum(c[0] for c in counts[b]) == int((est[b] < C).sum()) and sum(c[1] for c in counts[b]) == int((gt[b] < C).sum())
            assert all(c[2] <= min(c[0], c[1]) for c in counts[b])
        if kind == 'special':
            assert dice[0][0] == 1.0 and counts[0][1] == [0, 0, 0]                  # label 1: in neither map
            assert dice[0][1] == 0.0 and counts[0][2][0] > 0 and counts[0][2][1] == 0   # label 2: in est only
            assert dice[B - 1] == [1.0] * (C - 1)
        if kind == 'foreign':
            assert all(int(((est == v) & (gt == v)).sum()) > 0 for v in (7, 200, 255))
            assert sum(c[0] for c in counts[0]) < pixels
        if C == 256:
            assert all(c[0] > 0 and c[1] > 0 for c in counts[0])                    # all 768 counters are live


# ---------------------------------------------------------------------------------------------------- the cases' margins
@pytest.mark.parametrize('H,W', PR.EST_SHAPES)
def test_every_landmark_case_is_far_from_the_threshold(H, W):
    """A condition on the inputs: no correlation of a case that runs on the device is within 0.01 of its min_ncc, so acceptance
    cannot hinge on float32 rounding and no case is excused."""
    heats, names = PR.peak_case(H, W, L=3 if H * W > TRIP else None)
    rc, ncc, _, _ = PR.est_lands(heats, min_ncc=PR.EST_MIN_NCC)
    assert np.abs(ncc - PR.EST_MIN_NCC).min() >= 0.01, sorted(zip(np.abs(ncc - PR.EST_MIN_NCC).ravel(), sum(names, [])))[:3]
    accepted = rc[..., 0] >= 0
    assert accepted.any() and (H * W > TRIP or (~accepted).any())
    if H * W <= TRIP:
        for b in range(2):
            for l, name in enumerate(names[b]):
                if name.startswith('corner'):
                    assert accepted[b, l] and ncc[b, l] > 0.99
                if name == 'noise':
                    assert not accepted[b, l] and abs(ncc[b, l]) < 0.5
    if (H, W) == (64, 80):
        mh, ms, ml = PR.masked_case(H, W)
        assert np.abs(PR.est_lands(mh, ms, ml)[1] - PR.EST_MIN_NCC).min() >= 0.01


def test_the_smallest_map_takes_every_window_through_the_reflection():
    H = W = 13
    assert H == PR.LM_R + 1                       # csrc: dfl_est_lands requires H, W > LM_R = 12
    rc = PR.est_lands(PR.peak_case(H, W)[0], min_ncc=-2.0)[0]
    assert rc.min() >= 0 and {tuple(v) for v in rc[0].tolist()} >= {(0, 0), (0, 12), (12, 0), (12, 12), (11, 12)}


# ---------------------------------------------------------------------------------------------------- the cases' regimes
def test_scan_shapes_lie_in_the_three_regimes():
    hw = [h * w for h, w in PR.EST_SHAPES]
    # empty workgroups: fewer pixels than one slot, and fewer than 64 workgroups' worth in the smaller maps
    assert all(n <= SLOT for n in hw[:4]) and 13 * 13 < WG and math.ceil(64 * 80 / WG) < LM_SCAN_NB
    # partly filled unroll: more than one slot, less than a trip, and the last slot itself only partly covered
    assert SLOT < hw[4] <= TRIP and hw[4] % SLOT != 0 and hw[4] // SLOT < LM_SCAN_U - 1
    # second trip of the outer loop, which itself ends inside the first unroll slot
    assert TRIP < hw[5] < TRIP + SLOT


def test_argmax_cases_sit_where_their_names_say():
    for (H, W) in [(64, 80), (150, 200), (300, 440)]:
        heats, want = PR.argmax_case(H, W)
        hw = H * W
        assert np.isfinite(heats).all()
        for b in range(2):
            for l, (name, k) in enumerate(want[b]):
                m = heats[b, l].ravel()
                top = np.flatnonzero(m == m.max())
                assert top[0] == k, name
                if name.startswith('unique'):
                    assert top.tolist() == [k]
                elif name.startswith('tie'):
                    assert len(top) == 2 and m[top[0]].tobytes() == m[top[1]].tobytes()
                elif name == 'all-negative':
                    assert m.max() < 0
                elif '0' in name and 'before' in name:
                    assert len(top) == 2 and m.max() == 0 and np.signbit(m[top[0]]) != np.signbit(m[top[1]])
                    assert np.signbit(m[top[0]]) == name.startswith('-0')
                elif name == 'subnormal':
                    assert 0 < m.min() and m.max() < 2.0 ** -126 and len(top) == 1
                else:
                    raise AssertionError(name)
        names = [n for n, _ in want[0]]
        assert ('unique@16384' in names) == (hw > SLOT) and ('unique@131072' in names) == (hw > TRIP)
        assert ('tie unroll slots' in names) == (hw > SLOT + 300) and ('tie outer trips' in names) == (hw > TRIP + 300)
    assert len(PR.argmax_case(300, 440)[1][0]) == 8 + 4 + 1 + 2 + 1
    ties = {n: (scan_coords(i), scan_coords(j)) for n, i, j in PR.TIES}
    assert all(i < j for _, i, j in PR.TIES)
    a, b = ties['tie workgroups']
    assert a[0] != b[0] and a[2:] == b[2:]
    a, b = ties['tie neighbouring workgroups']
    assert b[0] == a[0] + 1 and (a[1], b[1]) == (WG - 1, 0) and a[2:] == b[2:]
    a, b = ties['tie unroll slots']
    assert a[:2] == b[:2] and a[3] == b[3] and a[2] != b[2]
    a, b = ties['tie outer trips']
    assert a[:3] == b[:3] and a[3] != b[3]
    # the boundaries the unique maxima straddle
    assert scan_coords(255)[0] + 1 == scan_coords(256)[0] and scan_coords(16383)[2] + 1 == scan_coords(16384)[2]
    assert scan_coords(131071)[3] + 1 == scan_coords(131072)[3] and scan_coords(131071)[:3] == (LM_SCAN_NB - 1, WG - 1, LM_SCAN_U - 1)


def test_prep_shapes_lie_in_their_regimes():
    n = [(H + 2 * p) * (W + 2 * p) for _, H, W, p in PR.PREP_SHAPES]
    assert n[0] == 16 < WG                                               # less than one workgroup
    assert [p for _, H, W, p in PR.PREP_SHAPES if p == H - 1] == [1, 36]  # the largest legal reflect, square and not
    assert all(n_ <= PREP_NB * WG for n_ in n[:3]) and n[3] > PREP_NB * WG      # the statistics loop's second trip
    # second pass of the write kernel: past what the capped grid covers at 4 pixels a thread; masks and heats (H * W pixels) too
    _, H, W, p = PR.PREP_BIG
    assert p == 0 and H * W > PREP_WRITE_CAP * WG * PREP_WRITE_PER_THREAD
    assert math.ceil(n[3] / (WG * PREP_WRITE_PER_THREAD)) < PREP_WRITE_CAP    # every other shape runs the uncapped grid


def test_dice_sizes_lie_in_their_regimes():
    px = PR.DICE_PIXELS
    assert px[:4] == [1, 255, 257, 6300] and all(p_ % WG for p_ in px)
    assert math.ceil(px[3] / (WG * DICE_PER_THREAD)) == 2                # more than one workgroup, below the cap
    assert px[4] > DICE_CAP * DICE_PER_THREAD * WG and px[4] - DICE_CAP * DICE_PER_THREAD * WG == 257   # the stride loop's second trip
    assert 3 * 256 > WG                                                  # C = 256: more than one LDS counter per thread
