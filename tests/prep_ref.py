"""float64 models of the three entry points of csrc/prep.hip -- dfl_prep_batch, dfl_est_lands, dfl_hard_dice -- as
include/dfl_hip.h states them ("GPU-side input pipeline", "Landmark extraction", "Hard Dice"), in numpy only, and the
builders of the cases that tests/test_gpu_prep.py runs on the device (tests/test_prep_ref_cpu.py vouches for the same
inputs on the CPU: the models against oracle/ref_cpu.py and the goldens, the cases against the regimes they are named
after).

Inputs are taken at their stored precision (float32 pixels, landmarks and sigma, uint8 labels); everything after that is
float64, or Python integers for the counts.  Heat maps handed to est_lands are finite by contract: NaN and +-inf heat
values are out of scope here (the device treats them as "no candidate"; nothing states what the reference scripts do
with them) and no builder of this module produces one."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
LM_T, LM_R = 25, 12             # the template's side and the reflect border of the window (est_lands_csv.py:96-124)
LM_N = LM_T * LM_T


# ---------------------------------------------------------------------------------------------------- input pipeline
def reflect_pad(img, pad):
    """[H][W] -> [H + 2 pad][W + 2 pad], mirrored about the border pixels without repeating them (pad < H, W)."""
    img = np.asarray(img)
    H, W = img.shape
    assert 0 <= pad < H and pad < W
    rows = np.abs(np.arange(-pad, H + pad))
    rows = np.where(rows >= H, 2 * (H - 1) - rows, rows)
    cols = np.abs(np.arange(-pad, W + pad))
    cols = np.where(cols >= W, 2 * (W - 1) - cols, cols)
    return img[rows[:, None], cols[None, :]]


def standardize(img, pad):
    """-> (x, m, sd): (p - m) / sd of the padded image p, m its mean and sd its unbiased standard deviation, two passes."""
    p = reflect_pad(np.asarray(img, dtype=F32), pad).astype(F64)
    n = p.size
    m = math.fsum(p.ravel()) / n
    sd = math.sqrt(math.fsum(((p - m) ** 2).ravel()) / (n - 1))
    return (p - m) / sd, m, sd


def one_hot(labels, C):
    """[H][W] labels -> float32 [C][H][W]; a label >= C is in no channel."""
    labels = np.asarray(labels)
    return (labels[None] == np.arange(C).reshape(C, 1, 1)).astype(F32)


def in_view(mx, my, H, W):
    """Both coordinates finite and inside [0, W-1] x [0, H-1], bounds included (-0.0 >= 0 holds)."""
    mx, my = float(mx), float(my)
    return math.isfinite(mx) and math.isfinite(my) and 0.0 <= mx <= W - 1 and 0.0 <= my <= H - 1


def heat(lands, H, W, sigma):
    """lands [2][L] (row 0 = column x, row 1 = row y) -> (maps [L][H][W], e [L][H][W]): exp(e) / (2 pi sigma^2) with
    e = -((x - mx)^2 + (y - my)^2) / (2 sigma^2); an all-zero map (and e = 0) for a landmark that is not in view."""
    lands = np.asarray(lands, dtype=F32)
    L = lands.shape[1]
    s2 = float(F32(sigma)) ** 2
    Y, X = np.meshgrid(np.arange(H, dtype=F64), np.arange(W, dtype=F64), indexing='ij')
    maps, es = np.zeros((L, H, W), F64), np.zeros((L, H, W), F64)
    for l in range(L):
        mx, my = lands[0, l], lands[1, l]
        if in_view(mx, my, H, W):
            es[l] = -((X - float(mx)) ** 2 + (Y - float(my)) ** 2) / (2.0 * s2)
            maps[l] = np.exp(es[l]) / (2.0 * math.pi * s2)
    return maps, es


# ---------------------------------------------------------------------------------------------------- landmark extraction
def template(sigma):
    s2 = float(F32(sigma)) ** 2
    d = np.arange(LM_T, dtype=F64) - LM_R
    return np.exp(-(d[None, :] ** 2 + d[:, None] ** 2) / (2.0 * s2)) / (2.0 * math.pi * s2)


def ncc_2d(t, y):
    """ncc.py:12-38 in float64: standard deviations over N - 1, the product over N sd_t sd_y + 1e-8.  -> (ncc, sd_t, sd_y)"""
    N = t.size
    tz, yz = t - t.sum() / N, y - y.sum() / N
    sd_t, sd_y = math.sqrt((tz * tz).sum() / (N - 1)), math.sqrt((yz * yz).sum() / (N - 1))
    return float((tz * yz).sum() / (N * (sd_t * sd_y) + 1.0e-8)), sd_t, sd_y


def est_lands(heats, segs=None, label_for_land=None, sigma=2.5, min_ncc=0.9):
    """heats float32 [B][L][H][W] -> (rowcol int [B][L][2], ncc [B][L], amp_y [B][L], amp_t [B][L]).
    arg-max on the float32 values with exact comparison (-0.0 == +0.0, ties to the lowest flat index) over the pixels whose label
    is label_for_land[l] (all of them when segs or label_for_land is None or the entry is negative); nothing eligible -> (-1, -1),
    ncc 0.  Else ncc_2d(template, 25 x 25 window of the map reflect-padded by 12) in float64; the location is kept iff
    not (ncc < min_ncc).  amp_y = max|y| / sd_y of the window and amp_t = max|t| / sd_t of the template (inf for a constant
    window) are what the error bound of a float32 evaluation is written in."""
    heats = np.asarray(heats)
    assert heats.dtype == F32 and bool(np.isfinite(heats).all())
    B, L, H, W = heats.shape
    assert H > LM_R and W > LM_R
    t = template(sigma)
    rowcol = np.full((B, L, 2), -1, np.int64)
    ncc, amp_y, amp_t = np.zeros((B, L)), np.zeros((B, L)), np.zeros((B, L))
    for b in range(B):
        for l in range(L):
            flat = heats[b, l].ravel()
            want = -1 if (segs is None or label_for_land is None) else int(label_for_land[l])
            idx = np.arange(flat.size) if want < 0 else np.flatnonzero(np.asarray(segs[b]).ravel() == want)
            if idx.size == 0:
                continue
            best = idx[int(np.argmax(flat[idx]))]           # numpy: the first of equal maxima; -0.0 == +0.0
            r, c = int(best) // W, int(best) % W
            y = reflect_pad(heats[b, l], LM_R)[r:r + LM_T, c:c + LM_T].astype(F64)
            v, sd_t, sd_y = ncc_2d(t, y)
            ncc[b, l] = v
            amp_y[b, l] = float(np.abs(y).max()) / sd_y if sd_y > 0 else math.inf
            amp_t[b, l] = float(t.max()) / sd_t
            if not v < float(F32(min_ncc)):
                rowcol[b, l] = (r, c)
    return rowcol, ncc, amp_y, amp_t


# ---------------------------------------------------------------------------------------------------- hard Dice
def dice_counts(est, gt, C):
    """[B][n] labels -> (counts [B][C][3] of Python integers (|est == l|, |gt == l|, |both|), dice [B][C-1] for l = 1..C-1)."""
    est, gt = np.asarray(est), np.asarray(gt)
    counts, dice = [], []
    for b in range(est.shape[0]):
        e, g = est[b].ravel().astype(np.int64), gt[b].ravel().astype(np.int64)
        ne = np.bincount(e, minlength=256)
        ng = np.bincount(g, minlength=256)
        nb = np.bincount(e[e == g], minlength=256)
        counts.append([[int(ne[l]), int(ng[l]), int(nb[l])] for l in range(C)])
        dice.append([2.0 * c[2] / (c[0] + c[1]) if c[0] + c[1] > 0 else 1.0 for c in counts[-1][1:]])
    return counts, dice


# ==================================================================================================== case builders
def rng(seed):
    return np.random.default_rng(seed)


# ---- dfl_prep_batch
PREP_SHAPES = [(1, 2, 2, 1), (3, 20, 31, 0), (2, 37, 53, 36), (2, 130, 127, 3), (1, 1025, 1025, 0)]   # (B, H, W, pad)
PREP_BIG = PREP_SHAPES[-1]


def prep_images(kind, B, H, W, seed=11):
    """float32 [B][H][W]: 'uniform' 100..3100; 'offset' 60000 + N(0, 0.5), a 16-bit detector image whose mean is 10^5 spreads;
    'scaled' uniform images whose means differ by 1000 x from one image to the next."""
    g = rng(seed + 1000 * H + W)
    if kind == 'uniform':
        return (g.random((B, H, W)) * 3000.0 + 100.0).astype(F32)
    if kind == 'offset':
        return (60000.0 + 0.5 * g.standard_normal((B, H, W))).astype(F32)
    assert kind == 'scaled'
    return ((g.random((B, H, W)) * 3.0 + 0.1) * (1000.0 ** np.arange(B)).reshape(B, 1, 1)).astype(F32)


def prep_labels(B, H, W, C, foreign=(), seed=12):
    """uint8 [B][H][W] over 0..C-1, every label present where the image has the room; `foreign` labels (>= C) on some pixels."""
    g = rng(seed + 1000 * H + W + C)
    lab = g.integers(0, C, (B, H, W)).astype(np.uint8)
    flat = lab.reshape(B, -1)
    for b in range(B):
        for k, v in enumerate(foreign):
            flat[b, (3 + 7 * k + b)::11] = v
    return lab


def land_entries(H, W):
    """(mx, my, in view) for the fourteen landmark forms: on the boundary of the view, one float32 step outside it on each of
    its four sides, sub-pixel, and not finite in one or both coordinates."""
    w1, h1 = F32(W - 1), F32(H - 1)
    up, dn, inf, nan = F32(np.inf), F32(-np.inf), F32(np.inf), F32(np.nan)
    sx, sy = F32(0.37 * (W - 1)), F32(0.61 * (H - 1))
    ent = [(F32(0.0), F32(0.0), True), (F32(-0.0), F32(-0.0), True), (w1, h1, True),
           (np.nextafter(F32(0.0), dn), sy, False), (sx, np.nextafter(F32(0.0), dn), False),
           (np.nextafter(w1, up), sy, False), (sx, np.nextafter(h1, up), False),
           (sx, sy, True), (inf, inf, False), (dn, sy, False), (nan, sy, False), (sx, inf, False),
           (w1, F32(-0.0), True), (F32(0.25 * (W - 1)), F32(0.5 * (H - 1)), True)]
    assert len(ent) == 14
    return ent


def prep_lands(B, H, W, L, start=0):
    """float32 [B][2][L] and bool [B][L] (in view): the forms of land_entries, rotated from one image to the next."""
    ent = land_entries(H, W)
    lands, view = np.zeros((B, 2, L), F32), np.zeros((B, L), bool)
    for b in range(B):
        for l in range(L):
            mx, my, ok = ent[(start + 5 * b + l) % 14]
            lands[b, 0, l], lands[b, 1, l], view[b, l] = mx, my, ok
    return lands, view


# ---- dfl_est_lands
EST_SHAPES = [(13, 13), (13, 40), (40, 13), (64, 80), (150, 200), (300, 440)]
EST_MIN_NCC = 0.9
EST_SIGMA = 2.5


def peak_positions(H, W):
    """(name, row, col) of the peaks: the four corners, the rows / columns where the 25 x 25 window first and last touches the
    border (11, 12, H-13, H-12), interior-near-border positions, a sub-pixel peak, and None for noise only."""
    return [('corner00', 0, 0), ('corner0W', 0, W - 1), ('cornerH0', H - 1, 0), ('cornerHW', H - 1, W - 1),
            ('r11c12', 11, 12), ('rH-13cW-12', H - 13, W - 12), ('r12c11', 12, min(11, W - 1)), ('rH-12cW-13', H - 12, W - 13),
            ('r5c5', 5, 5), ('r3cmid', 3, W // 2), ('rmidc2', H // 2, 2), ('subpixel', H // 2 + 0.5, W // 2 - 0.25),
            ('noise', None, None)]


def peak_case(H, W, L=None, seed=21):
    """heats float32 [2][L][H][W]: a Gaussian peak (sigma 2.5) per map plus 1e-4 uniform noise; image 1 holds the positions in the
    reverse order and other noise.  L = None: every position; else the first L of (cornerHW, rH-13cW-12, subpixel, ...)."""
    pos = peak_positions(H, W)
    if L is not None:
        order = [3, 5, 11, 4, 12, 0, 1, 2, 6, 7, 8, 9, 10]
        pos = [pos[k] for k in order[:L]]
    g = rng(seed + 1000 * H + W)
    heats = np.zeros((2, len(pos), H, W), F32)
    names = [[], []]
    for b in range(2):
        for l, (name, r, c) in enumerate(pos if b == 0 else pos[::-1]):
            m = 1.0e-4 * g.random((H, W))
            if r is not None:
                m = m + heat(np.array([[c], [r]], F32), H, W, EST_SIGMA)[0][0]
            heats[b, l] = m.astype(F32)
            names[b].append(name)
    return heats, names


# (name, lower flat index, higher flat index) of two equal maxima; tests/test_prep_ref_cpu.py holds them against the scan's constants
TIES = [('tie workgroups', 300, 1000), ('tie neighbouring workgroups', 255, 256), ('tie unroll slots', 300, 300 + 16384),
        ('tie outer trips', 300, 300 + 131072)]


def argmax_case(H, W, seed=31):
    """heats float32 [2][L][H][W] for the placement of the arg-max, and per map (name, expected flat index): a unique maximum
    at each listed flat index that the map has, two equal maxima in different workgroups / unroll slots / outer trips of the scan,
    an all-negative map, zero maxima of either sign, positive subnormals.  Image 1 holds the maps in the reverse order."""
    hw = H * W
    g = rng(seed + hw)
    maps = []
    for k in (0, hw - 1, 255, 256, 16383, 16384, 131071, 131072):
        if k < hw:
            m = g.random(hw).astype(F32)
            m[k] = 2.0
            maps.append(('unique@%d' % k, k, m))
    for name, i, j in TIES:
        if j < hw:
            m = g.random(hw).astype(F32)
            m[i] = m[j] = 2.0
            maps.append((name, i, m))
    m = (-1.0 - g.random(hw)).astype(F32)
    m[hw // 3] = -0.5
    maps.append(('all-negative', hw // 3, m))
    lo, hi = hw // 5, hw - 7
    for name, a, b in (('-0 before +0', -0.0, 0.0), ('+0 before -0', 0.0, -0.0)):
        m = (-1.0 - g.random(hw)).astype(F32)
        m[lo], m[hi] = a, b
        maps.append((name, lo, m))
    m = (g.integers(1, 1 << 20, hw).astype(np.uint32)).view(F32).copy()    # positive subnormals k * 2^-149
    m[hw // 2 + 1] = np.uint32((1 << 22) + 5).view(F32)
    maps.append(('subnormal', hw // 2 + 1, m))
    heats = np.stack([np.stack([m.reshape(H, W) for _, _, m in maps]), np.stack([m.reshape(H, W) for _, _, m in maps[::-1]])])
    want = [[(n, k) for n, k, _ in maps], [(n, k) for n, k, _ in maps[::-1]]]
    return heats, want


def masked_case(H, W, seed=41):
    """-> (heats [2][L][H][W], segs uint8 [2][H][W], label_for_land int32 [L]).  Labels 0..3 everywhere; 5 in image 0 only; 200 and
    255 in both; 4 on the single pixel H*W-1 of both; 9 nowhere.  label_for_land mixes negative, present and absent labels."""
    g = rng(seed + 1000 * H + W)
    label_for_land = np.array([-1, 3, 9, 5, 200, 255, 4, 0, -7], np.int32)
    heats, _ = peak_case(H, W, L=len(label_for_land), seed=seed)
    segs = g.integers(0, 4, (2, H, W)).astype(np.uint8)
    segs[0, H // 4:H // 2, W // 4:W // 2] = 5
    segs[:, 2:H // 3, W // 2:] = 200
    segs[:, H // 2:, 1:W // 3] = 255
    segs[:, H - 1, W - 1] = 4
    return heats, segs, label_for_land


# ---- dfl_hard_dice
DICE_PIXELS = [1, 255, 257, 70 * 90, 256 * 16 * 256 + 257]


def dice_case(pixels, B, C, kind='random', seed=51):
    """(est, gt) uint8 [B][pixels].  'random': labels 0..C-1, every one present when pixels >= C; 'foreign': C = 7 maps that also hold
    7, 200 and 255 in both; 'special': image 0 has label 1 absent from both and label 2 in est only, the last image is identical
    maps."""
    g = rng(seed + pixels + 7 * C + B)
    est = g.integers(0, C, (B, pixels)).astype(np.uint8)
    gt = np.where(g.random((B, pixels)) < 0.7, est, g.integers(0, C, (B, pixels))).astype(np.uint8)
    if pixels >= C:
        est[:, :C] = np.arange(C, dtype=np.uint8)
        gt[:, pixels - C:] = np.arange(C, dtype=np.uint8)
    if kind == 'foreign':
        for k, v in enumerate((7, 200, 255)):
            est[:, (k + 1)::13] = v
            gt[:, (k + 2)::17] = v
            gt[:, (k + 1)::26] = v          # some pixels carry the same foreign label in both maps
    if kind == 'special':
        est[0][est[0] == 1] = 0
        gt[0][gt[0] == 1] = 0
        gt[0][gt[0] == 2] = 0
        gt[B - 1] = est[B - 1]
    return est, gt
