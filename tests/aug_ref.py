"""numpy restatement of one augmented training item of the reference's RandomDataAugDataSet (train_test_code/dataset.py:
107-293) for EXPLICIT parameters, with the per-pixel normals of the device path (Philox4x32-10 + Box-Muller).  The
reference draws its parameters from Python's ``random`` and torch's CPU generator and warps through torchvision + PIL;
given the parameters every step is deterministic, and this file restates those steps in the reference's arithmetic
(fp32 tensor ops, fp64 PIL warp).  tools/gen_aug_golden.py writes the fixtures tests/golden/aug_*.npz from it; the CPU
tests pin its warp against PIL itself.  torchvision is not needed: its affine matrix is restated below, in one place.

Parameters of one item (``prm``): flags (dfl_amd._native.AUG_*), sigma, noise_key, gamma, angle (degrees), translate
(tx, ty) pixels, scale, shear (degrees x, y), boxes [(row, col, rows, cols, key), ...]; optionally maps = (projection
map, label map, landmark map), the 18 doubles of a dfl_augment_item, which replace maps() (then angle, translate, scale
and shear are not read).  tap_report() and gamma_window() say which of PIL's border rules, how much reflection and which
quantisation steps each output pixel of a case meets (tests/test_aug_edges_cpu.py, tests/test_gpu_aug_edges.py)."""
import math

import numpy as np

INVERT, NOISE, GAMMA, ERASE = 1, 2, 4, 8
F32 = np.float32


# ---- torchvision.transforms.functional._get_inverse_affine_matrix (the documented definition) -------------------------
def inverse_affine_matrix(center, angle, translate, scale, shear):
    """Inverse of M = T(translate) C RSS C^-1 with RSS = rotation(angle) with x / y shear, times scale; C = translation
    by center.  Returns the 6 coefficients (a, b, c, d, e, f): source = (a x + b y + c, d x + e y + f)."""
    rot = math.radians(angle)
    sx, sy = math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d, -b, 0.0, -c, a, 0.0]
    m = [v / scale for v in m]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def maps(H, W, pad, prm, has_seg=True):
    """(projection map, label map, landmark map): the first two PIL inverse maps of the padded frames (torchvision's PIL
    path centres them at (width / 2, height / 2)); the third the forward landmark map of dataset.py:211-219, centre
    (shape[-2] / 2 + 0.5, shape[-1] / 2 + 0.5) of the label map (of the cropped projection without labels)."""
    ch, cw = int(math.ceil(H / 2.0)), int(math.ceil(W / 2.0))
    args = (prm['angle'], tuple(prm['translate']), prm['scale'], tuple(prm['shear']))
    Hp, Wp = H + 2 * (ch + pad), W + 2 * (cw + pad)
    img = inverse_affine_matrix((Wp * 0.5, Hp * 0.5), *args)
    seg = inverse_affine_matrix(((W + 2 * cw) * 0.5, (H + 2 * ch) * 0.5), *args)
    sh = (H, W) if has_seg else (H + 2 * pad, W + 2 * pad)
    a = inverse_affine_matrix((sh[0] / 2.0 + 0.5, sh[1] / 2.0 + 0.5), *args)
    land = np.linalg.inv(np.array([a[0:3], a[3:6], [0.0, 0.0, 1.0]]))[:2].reshape(-1)
    return np.array(img), np.array(seg), land


# ---- Philox4x32-10 + Box-Muller ------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32 with 10 rounds (Salmon, Moraes, Dror, Shaw, SC'11), vectorised over uint32 arrays."""
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85
    x = [np.asarray(v, dtype=np.uint64) & np.uint64(0xffffffff) for v in (c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xffffffff, int(k1) & 0xffffffff
    mask = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = M0 * x[0], M1 * x[2]
        x = [(p1 >> np.uint64(32)) ^ x[1] ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ x[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return [v.astype(np.uint32) for v in x]


def normals(key, idx):
    """The device's N(0,1) for 64-bit key and pixel indices idx: counter (idx lo, idx hi, 0, 0), key (key lo, key hi);
    u1 = ((r0 >> 8) + 1) 2^-24, u2 = (r1 >> 8) 2^-24, z = sqrt(-2 ln u1) cos(2 pi u2) in fp32."""
    idx = np.asarray(idx, dtype=np.uint64)
    key = int(key)
    r = philox4x32_10(idx & np.uint64(0xffffffff), idx >> np.uint64(32), 0, 0, key & 0xffffffff, key >> 32)
    u1 = ((r[0] >> np.uint32(8)) + np.uint32(1)).astype(F32) * F32(2.0 ** -24)
    u2 = (r[1] >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)
    return np.sqrt(F32(-2.0) * np.log(u1)) * np.cos(F32(6.2831853071795864769) * u2)


# ---- PIL's 8-bit Image.transform(AFFINE) -----------------------------------------------------------------------------------
def source_coords(m, xs, ys):
    """Source point of the output pixel centres (xs + 0.5, ys + 0.5): PIL's affine_transform, fp64."""
    X, Y = xs + 0.5, ys + 0.5
    return m[0] * X + m[1] * Y + m[2], m[3] * X + m[4] * Y + m[5]


def bilinear_taps(Hs, Ws, m, xs, ys):
    """PIL's bilinear taps at the output pixels (xs, ys) of an Hs x Ws image: (inside, x0, y0, xa, xb, ya, yb, second, dx,
    dy).  x0, y0: floor of source - 0.5; xa, xb, ya the clamped taps; second: the row y0 + 1 exists (else yb = ya and
    the second row is dropped).  Outside the frame (a non-finite source included) the taps are those of source (0, 0)."""
    with np.errstate(invalid='ignore', over='ignore'):
        sx, sy = source_coords(m, xs, ys)
        inside = (sx >= 0) & (sx < Ws) & (sy >= 0) & (sy < Hs)
    sx, sy = np.where(inside, sx, 0.0), np.where(inside, sy, 0.0)
    xi, yi = sx - 0.5, sy - 0.5
    fx, fy = np.floor(xi), np.floor(yi)
    dx, dy = xi - fx, yi - fy
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    xa, xb = np.clip(x0, 0, Ws - 1), np.clip(x0 + 1, 0, Ws - 1)
    ya = np.clip(y0, 0, Hs - 1)
    second = (y0 + 1 >= 0) & (y0 + 1 < Hs)
    yb = np.where(second, y0 + 1, ya)
    return inside, x0, y0, xa, xb, ya, yb, second, dx, dy


def pil_bilinear(img, m, xs, ys):
    """PIL's bilinear_filter8 at the output pixels (xs, ys) of the uint8 image img: outside [0, size) -> 0; taps at
    source - 0.5 clamped to the image, the second row dropped past the last one; the fp64 result truncated."""
    Hs, Ws = img.shape
    inside, x0, y0, xa, xb, ya, yb, second, dx, dy = bilinear_taps(Hs, Ws, m, xs, ys)
    q = img.astype(np.float64)
    v1 = q[ya, xa] + (q[ya, xb] - q[ya, xa]) * dx
    v2 = np.where(second, q[yb, xa] + (q[yb, xb] - q[yb, xa]) * dx, v1)
    v = v1 + (v2 - v1) * dy
    return np.where(inside, v, 0.0).astype(np.int64).astype(np.uint8)


def pil_nearest(img, m, xs, ys, fill=0):
    """Nearest: the pixel holding the source point (floor); outside the image (a non-finite source included) -> fill."""
    Hs, Ws = img.shape
    with np.errstate(invalid='ignore', over='ignore'):
        sx, sy = source_coords(m, xs, ys)
        inside = (sx >= 0) & (sx < Ws) & (sy >= 0) & (sy < Hs)
    sx, sy = np.where(inside, sx, 0.0), np.where(inside, sy, 0.0)
    xi = np.clip(np.floor(sx).astype(np.int64), 0, Ws - 1)
    yi = np.clip(np.floor(sy).astype(np.int64), 0, Hs - 1)
    return np.where(inside, img[yi, xi], fill).astype(img.dtype)


def reflect_index(i, n):
    """numpy 'reflect' padding as an index map, any distance."""
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


# ---- one item -------------------------------------------------------------------------------------------------------------
def _norm(p):
    mn, mx = p.min(), p.max()
    return mn, mx, F32(mx - mn)


def case_maps(H, W, pad, prm, has_seg=True):
    """The three maps of a case as float64 arrays of 6: prm['maps'] when given, else maps()."""
    if prm.get('maps') is not None:
        return tuple(np.array(m, dtype=np.float64) for m in prm['maps'])
    return maps(H, W, pad, prm, has_seg)


def before_gamma(proj, prm, normals_fn=normals):
    """(the fp32 image after invert and noise, the noise normals or None)."""
    p = np.asarray(proj, dtype=F32)
    H, W = p.shape
    z = None
    if prm['flags'] & INVERT:                            # :118-122
        p = p.max() - p
    if prm['flags'] & NOISE:                             # :127-138
        mn, mx, d = _norm(p)
        p = (p - mn) / d
        z = normals_fn(prm['noise_key'], np.arange(H * W)).reshape(H, W)
        p = p + z * F32(prm['sigma'])
        p = p * d + mn
    return p, z


def erase_boxes(prm, Ho, Wo):
    """The boxes the erase step applies: the first five at most, up to the first one that does not fit the Ho x Wo image
    or has a side <= 0 (include/dfl_hip.h: dfl_augment_item.n_box)."""
    out = []
    for (r0, c0, nr, nc, key) in prm['boxes'][:5]:
        if r0 < 0 or c0 < 0 or nr <= 0 or nc <= 0 or r0 + nr > Ho or c0 + nc > Wo:
            break
        out.append((r0, c0, nr, nc, key))
    return out


def augment_item(proj, seg, lands, prm, pad, C, land_rule='reference', heat_sigma=2.5, standardize=True, normals_fn=normals):
    """proj [H,W] fp32, seg [H,W] uint8 labels or None, lands [2,L] fp32 or None.  Returns a dict: x [H+2pad,W+2pad]
    (standardised), levels (the warped 8-bit image, cropped), noise [H,W] (the normals, or None), labels [H,W] (255 =
    outside the warped frame), label_src (source coordinates of the label pixels, for the near-integer exclusion), masks
    [C,H,W], lands [2,L], heats [L,H,W].  normals_fn(key, idx) supplies the normals of the noise plane and of every
    erase box (the device's own, in the tests that hold the rest bit for bit); land_rule None drops no landmark."""
    p, z = before_gamma(proj, prm, normals_fn)
    H, W = p.shape
    flags = prm['flags']
    out = {'noise': z}
    if flags & GAMMA:                                    # :140-151
        mn, mx, d = _norm(p)
        p = (p - mn) / d
        p = np.power(p, F32(prm['gamma']))
        p = p * d + mn
    # affine (:153-248)
    mn, mx, d = _norm(p)
    p = (p - mn) / d
    q = (p * F32(255.0)).astype(np.uint8)                # to_pil_image: mul(255).byte()
    ch, cw = int(math.ceil(H / 2.0)), int(math.ceil(W / 2.0))
    qp = np.pad(q, ((ch + pad, ch + pad), (cw + pad, cw + pad)), 'reflect')
    img_map, seg_map, land_map = case_maps(H, W, pad, prm, seg is not None)
    Ho, Wo = H + 2 * pad, W + 2 * pad
    ys, xs = np.meshgrid(np.arange(Ho) + ch, np.arange(Wo) + cw, indexing='ij')   # the centre crop of the padded frame
    lev = pil_bilinear(qp, img_map, xs.astype(np.float64), ys.astype(np.float64))
    out['levels'] = lev
    p = lev.astype(F32) / F32(255.0)
    p = p * d + mn
    if seg is not None:
        sp = np.pad(np.asarray(seg, dtype=np.uint8), ((ch, ch), (cw, cw)), 'reflect')
        ys, xs = np.meshgrid(np.arange(H) + ch, np.arange(W) + cw, indexing='ij')
        out['labels'] = pil_nearest(sp, seg_map, xs.astype(np.float64), ys.astype(np.float64), fill=255)
        with np.errstate(invalid='ignore', over='ignore'):
            out['label_src'] = source_coords(seg_map, xs.astype(np.float64), ys.astype(np.float64))
        out['masks'] = np.stack([(out['labels'] == c) for c in range(C)]).astype(F32)
    if lands is not None:
        ln = np.array(lands, dtype=F32, copy=True)
        for l in range(ln.shape[1]):
            x, y = float(ln[0, l]), float(ln[1, l])
            if math.isinf(x) or math.isinf(y):           # :242: the pair stays as it is
                continue
            with np.errstate(invalid='ignore', over='ignore'):
                X = land_map[0] * x + land_map[1] * y + land_map[2]
                Y = land_map[3] * x + land_map[4] * y + land_map[5]
            if seg is not None and land_rule == 'reference':        # :245-247 as written: orig_s_shape is (C, H, W)
                drop = X < 0 or X > H - 1 or Y < 0 or Y < C - 1
            elif seg is not None and land_rule == 'in_view':
                drop = X < 0 or X > W - 1 or Y < 0 or Y > H - 1
            else:
                drop = False
            with np.errstate(over='ignore'):
                ln[:, l] = (math.inf, math.inf) if drop else (X, Y)
        out['lands'] = ln
        Yg, Xg = np.meshgrid(np.arange(H, dtype=F32), np.arange(W, dtype=F32), indexing='ij')
        s2 = F32(heat_sigma) * F32(heat_sigma)
        kexp, knorm = F32(1.0) / (s2 * F32(-2.0)), F32(1.0) / (F32(2.0 * math.pi) * s2)
        h = np.zeros((ln.shape[1], H, W), F32)
        for l in range(ln.shape[1]):
            if np.isfinite(ln[0, l]) and np.isfinite(ln[1, l]):
                dx, dy = Xg - ln[0, l], Yg - ln[1, l]
                h[l] = np.exp((dx * dx + dy * dy) * kexp) * knorm
        out['heats'] = h
    if flags & ERASE:                                    # :250-283
        for (r0, c0, nr, nc, key) in erase_boxes(prm, Ho, Wo):
            roi = p[r0:r0 + nr, c0:c0 + nc]
            sig = (roi.max() - roi.min()) * F32(0.2)
            rr, cc = np.meshgrid(np.arange(r0, r0 + nr), np.arange(c0, c0 + nc), indexing='ij')
            z = normals_fn(key, (rr * Wo + cc).reshape(-1)).reshape(nr, nc)
            p[r0:r0 + nr, c0:c0 + nc] = roi + z * sig
    out['raw'] = p.copy()
    if standardize:                                      # :292-293, statistics in fp64 like dfl_prep_batch
        v = p.astype(np.float64)
        m = v.sum() / v.size
        var = max((np.square(v).sum() - v.sum() * m) / (v.size - 1), 0.0)
        with np.errstate(divide='ignore', invalid='ignore'):
            p = (p - F32(m)) * F32(np.float64(1.0) / np.sqrt(np.float64(var)))
    out['x'] = p
    return out


def taps_inside(H, W, pad, prm):
    """True when every bilinear tap of the projection warp and every nearest sample of the label warp lies inside the
    padded image (then PIL's border rules never apply).  The maps are affine: the crop's corner pixels bound them."""
    img_map, seg_map, _ = maps(H, W, pad, prm)
    ch, cw = int(math.ceil(H / 2.0)), int(math.ceil(W / 2.0))
    ok = True
    for m, (h, w), (ph, pw) in ((img_map, (H + 2 * pad, W + 2 * pad), (ch + pad, cw + pad)), (seg_map, (H, W), (ch, cw))):
        xs = np.array([0, w - 1, 0, w - 1], np.float64) + cw
        ys = np.array([0, 0, h - 1, h - 1], np.float64) + ch
        sx, sy = source_coords(m, xs, ys)
        ok &= bool(np.all(sx - 0.5 >= 0) and np.all(sy - 0.5 >= 0) and np.all(sx + 0.5 <= W + 2 * pw - 1) and
                   np.all(sy + 0.5 <= H + 2 * ph - 1))
    return ok


def _proj_taps(H, W, pad, prm):
    """bilinear_taps of the projection warp of a case over its (H+2pad) x (W+2pad) output, and the reflect pads."""
    ch, cw = int(math.ceil(H / 2.0)), int(math.ceil(W / 2.0))
    ph, pw = ch + pad, cw + pad
    ys, xs = np.meshgrid(np.arange(H + 2 * pad) + ch, np.arange(W + 2 * pad) + cw, indexing='ij')
    img_map = case_maps(H, W, pad, prm)[0]
    return bilinear_taps(H + 2 * ph, W + 2 * pw, img_map, xs.astype(np.float64), ys.astype(np.float64)), ph, pw


def tap_report(H, W, pad, prm):
    """Which rule of the projection warp each output pixel meets, as boolean planes [H+2pad, W+2pad]: 'outside' (the
    source is outside the padded frame, or not finite: level 0), and among the others 'dropped' (no row below the first
    taps: the second row is dropped), 'clamp_x' / 'clamp_y' (a tap left or right of / above the frame is clamped) and
    'reflect2' (one of the four taps, taken relative to the unpadded image, lies outside [-(n-1), 2(n-1)]: one mirror
    does not bring it home, the reflection runs beyond one period)."""
    (inside, x0, y0, xa, xb, ya, yb, second, dx, dy), ph, pw = _proj_taps(H, W, pad, prm)
    Wp = W + 2 * pw

    def far(i, n):
        return (i < -(n - 1)) | (i > 2 * (n - 1))
    return {'outside': ~inside, 'dropped': inside & ~second, 'clamp_x': inside & ((x0 < 0) | (x0 + 1 > Wp - 1)),
            'clamp_y': inside & (y0 < 0),
            'reflect2': inside & (far(xa - pw, W) | far(xb - pw, W) | far(ya - ph, H) | far(yb - ph, H))}


def gamma_window(proj, prm, pad, normals_fn=normals):
    """For a case with the gamma flag: the boolean plane [H+2pad, W+2pad] "one of the four taps of this output pixel lies
    in the gamma window", and the share of source pixels in it.  A source pixel is in the window when the float64
    evaluation of its value before the 8-bit truncation, t * 255 (normalise, ^gamma, map back, normalise again), lies
    within w = 255 * 2^-21 * (|mn| + |mx|) / (mx - mn) of an integer, mn / mx the image's range after gamma: there two
    powf of different libraries, each within an ulp or so of the truth, may truncate to different levels."""
    p, _ = before_gamma(proj, prm, normals_fn)
    H, W = p.shape
    nmn, nmx, nd = _norm(p)
    g = np.power((p - nmn) / nd, F32(prm['gamma'])) * nd + nmn
    mn, mx, d = _norm(g)
    v = ((p.astype(np.float64) - float(nmn)) / float(nd)) ** float(F32(prm['gamma'])) * float(nd) + float(nmn)
    t255 = (v - float(mn)) / float(d) * 255.0
    w = 255.0 * 2.0 ** -21 * (abs(float(mn)) + abs(float(mx))) / (float(mx) - float(mn))
    near = np.abs(t255 - np.rint(t255)) <= w
    (inside, x0, y0, xa, xb, ya, yb, second, dx, dy), ph, pw = _proj_taps(H, W, pad, prm)
    nearp = np.pad(near, ((ph, ph), (pw, pw)), 'reflect')
    return inside & (nearp[ya, xa] | nearp[ya, xb] | nearp[yb, xa] | nearp[yb, xb]), float(near.mean())


def heat_arguments(lands, H, W, heat_sigma=2.5):
    """(the fp32 arguments of exp [L,H,W], knorm fp32, finite [L]) of the heat maps of the landmarks lands [2,L], in the
    arithmetic of augment_item: a test compares a kernel's expf against the float64 exp of the same argument."""
    ln = np.asarray(lands, dtype=F32)
    Yg, Xg = np.meshgrid(np.arange(H, dtype=F32), np.arange(W, dtype=F32), indexing='ij')
    s2 = F32(heat_sigma) * F32(heat_sigma)
    kexp, knorm = F32(1.0) / (s2 * F32(-2.0)), F32(1.0) / (F32(2.0 * math.pi) * s2)
    finite = np.isfinite(ln[0]) & np.isfinite(ln[1])
    arg = np.zeros((ln.shape[1], H, W), F32)
    for l in np.nonzero(finite)[0]:
        dx, dy = Xg - ln[0, l], Yg - ln[1, l]
        arg[l] = (dx * dx + dy * dy) * kexp
    return arg, knorm, finite


def load_params(g):
    """The parameter dicts of a fixture (dfl_amd.dataset.DeviceAugment.draw's form)."""
    out = []
    for i in range(len(g['flags'])):
        out.append(dict(flags=int(g['flags'][i]), sigma=float(g['sigma'][i]), gamma=float(g['gamma'][i]),
                        angle=float(g['angle'][i]), translate=tuple(float(v) for v in g['translate'][i]),
                        scale=float(g['scale'][i]), shear=tuple(float(v) for v in g['shear'][i]),
                        noise_key=int(g['noise_key'][i]),
                        boxes=[tuple(int(v) for v in g['boxes'][i, b]) for b in range(int(g['n_box'][i]))]))
    return out
