"""Writes tests/golden/overlay_*.npz and the ellipse stamp table deepfluorolabeling-ipcai2020_amd/data/ellipse_stamps.txt.

Dev-only: needs torch (CPU) and Pillow (the fixtures pin Pillow 12.2), not torchvision or h5py.  The reference's overlay
scripts (train_test_code/overlay_est_ann.py, overlay_est_heat.py, examples_dataset/make_preproc_overlays.py) are restated
here operation by operation in torch fp32 on the CPU; the torchvision calls they make are restated as torchvision 0.x
implements them:
  TF.to_pil_image(float tensor)  -> Image.fromarray(t.mul(255).byte() as HWC)          (truncation)
  TF.to_tensor(8-bit image)      -> torch.from_numpy(array).permute(2, 0, 1).float().div(255)
  utils.save_image(t)            -> make_grid(t, nrow=8, padding=2, pad_value=0).mul(255).add_(0.5).clamp_(0, 255) as uint8
and ImageDraw.ellipse / ImageDraw.line are called exactly as the reference calls them.  Every image is then ALSO computed by
a numpy model of the kernel's own rules (stamp table gather for the ellipses, clipped segments for the crosses), and the two
must agree byte for byte.

Each overlay_*.npz holds the inputs of ONE dfl_amd.overlay.render call (images, optional segs / heats / gt_lands /
est_lands, num_classes, radius, cross, colors, grid) and the expected uint8 output.  overlay_stamps.npz holds the Pillow
stamps of every box (w, h) with 0 <= w, h <= 8 and of |w - h| <= 1 up to 40.

    python tools/gen_overlay_golden.py
"""
import math
import os

import numpy as np
import torch
import PIL
from PIL import Image, ImageDraw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
STAMPS_TXT = os.path.join(ROOT, 'deepfluorolabeling-ipcai2020_amd', 'data', 'ellipse_stamps.txt')

ANN_COLORS = [[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 0.0], [0.0, 1.0, 1.0], [1.0, 0.5, 0.0],
              [0.5, 0.0, 0.5]]                          # overlay_est_ann.py label_colors
PREPROC_COLORS = ANN_COLORS[:6]                         # make_preproc_overlays.py label_colors
STAMP_MAX = 43          # table: every box with max(w, h) <= 8, and |w - h| <= 4 up to this size


# ---- torchvision, restated ------------------------------------------------------------------------------------------
def to_pil_image(t):
    a = t.mul(255).byte()
    a = a.permute(1, 2, 0).numpy()
    return Image.fromarray(a[:, :, 0], 'L') if a.shape[2] == 1 else Image.fromarray(np.ascontiguousarray(a), 'RGB')


def to_tensor(pil):
    a = torch.from_numpy(np.array(pil, np.uint8, copy=True))
    if a.dim() == 2:
        a = a.unsqueeze(-1)
    return a.permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def make_grid(t, nrow=8, padding=2, pad_value=0.0):
    if t.dim() == 3:
        return t
    if t.shape[0] == 1:
        return t[0]
    B, C, H, W = t.shape
    xmaps = min(nrow, B)
    ymaps = int(math.ceil(float(B) / xmaps))
    height, width = H + padding, W + padding
    grid = t.new_full((C, height * ymaps + padding, width * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= B:
                break
            grid[:, y * height + padding:y * height + padding + H, x * width + padding:x * width + padding + W] = t[k]
            k += 1
    return grid


def save_image_bytes(t):
    g = make_grid(t)
    return g.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()


def normalise(img):
    """(img - min) / (max - min); a constant image is defined as 0 (the reference divides 0 by 0)."""
    lo, hi = img.min(), img.max()
    if bool(hi == lo):
        return torch.zeros_like(img)
    return (img - lo) / (hi - lo)


# ---- the reference scripts, restated ----------------------------------------------------------------------------------
def ref_ann(img, seg, num_classes, gt_lands, est_lands, overlay_lands, colors=ANN_COLORS, radius=2, cross=6):
    """overlay_est_ann.py:94-170 for one projection: img [1,H,W] fp32, seg [H,W] or None, gt_lands [2,L] or None,
    est_lands {idx: (col, row)}."""
    img = normalise(img)
    pil = to_pil_image(img).convert('RGB')
    img = to_tensor(pil)
    if seg is not None:
        alpha = 0.35
        for l in range(1, num_classes):
            if l - 1 >= len(colors):
                break
            s_idx = seg == l
            for c in range(3):
                img_c = img[c, :, :]
                img_c[s_idx] = ((1 - alpha) * img_c[s_idx]) + (alpha * colors[l - 1][c])
    if overlay_lands:
        pil = to_pil_image(img)
        draw = ImageDraw.Draw(pil)

        def get_box(x, box_radius=radius):
            return [(x[0] - box_radius, x[1] - box_radius), (x[0] + box_radius, x[1] + box_radius)]
        if gt_lands is not None:
            for l in range(gt_lands.shape[-1]):
                cur = gt_lands[:, l]
                if math.isfinite(cur[0]) and math.isfinite(cur[1]):
                    draw.ellipse(get_box(cur), fill='yellow')
        for _, x in (est_lands or {}).items():
            draw.line([(x[0], x[1] + cross), (x[0], x[1] - cross)], fill='yellow')
            draw.line([(x[0] - cross, x[1]), (x[0] + cross, x[1])], fill='yellow')
        del draw
        img = to_tensor(pil)
    return save_image_bytes(img)


def ref_heat(img, heat):
    """overlay_est_heat.py:55-88 for one projection and landmark."""
    img = normalise(img)
    pil = to_pil_image(img).convert('RGB')
    img = to_tensor(pil)
    heat_base_color = [0.0, 1.0, 0.0]
    heat_min, heat_max = heat.min(), heat.max()
    rng = heat_max - heat_min
    heat = heat - heat_min
    if rng > 1.0e-3:
        heat /= rng
    for c in range(3):
        img[c, :, :] = ((1 - heat) * img[c, :, :]) + (heat * heat_base_color[c])
    return save_image_bytes(img)


def ref_preproc(projs, segs, lands):
    """make_preproc_overlays.py:42-128 for one specimen group: projs [N,H,W] fp32, segs [N,H,W], lands [N,2,L]."""
    N, rows, cols = projs.shape
    box_radius = max(16 * (rows / 1536.0), 3.0)
    out = torch.zeros(N, 3, rows, cols)
    for p in range(N):
        cur = normalise(projs[p])
        pil = to_pil_image(cur.unsqueeze(0)).convert('RGB')
        cur = to_tensor(pil)
        for l in range(1, 7):
            idx = segs[p] == l
            for c in range(3):
                cc = cur[c, :, :]
                cc[idx] = ((1 - 0.35) * cc[idx]) + (0.35 * PREPROC_COLORS[l - 1][c])
        pil = to_pil_image(cur)
        draw = ImageDraw.Draw(pil)
        for l in range(lands.shape[2]):
            x, y = lands[p, 0, l], lands[p, 1, l]
            if (x >= 0) and (y >= 0) and (x < cols) and (y < cols):
                draw.ellipse([(x - box_radius, y - box_radius), (x + box_radius, y + box_radius)], fill='yellow')
        del draw
        out[p] = to_tensor(pil)
    return save_image_bytes(out), box_radius


# ---- Pillow's filled ellipse as a stamp table ---------------------------------------------------------------------------
def pil_stamp(w, h):
    im = Image.new('L', (w + 7, h + 7), 0)
    ImageDraw.Draw(im).ellipse([(3, 3), (3 + w, 3 + h)], fill=255)
    a = np.array(im) > 0
    assert not a[:3].any() and not a[:, :3].any() and not a[4 + h:].any() and not a[:, 4 + w:].any(), (w, h)
    return a[3:4 + h, 3:4 + w]


def stamp_boxes():
    return [(w, h) for w in range(STAMP_MAX + 1) for h in range(STAMP_MAX + 1)
            if max(w, h) <= 8 or abs(w - h) <= 4]


def spans_of(stamp):
    out = []
    for row in stamp:
        nz = np.nonzero(row)[0]
        if nz.size == 0:
            out.append((1, 0))
            continue
        assert nz[-1] - nz[0] + 1 == nz.size, 'a stamp row is not one span'
        out.append((int(nz[0]), int(nz[-1])))
    return out


def write_stamp_table():
    boxes = stamp_boxes()
    lines = ['# Filled-ellipse stamps of Pillow %s ImageDraw.ellipse for integer boxes (0, 0, w, h): one line per box,'
             % PIL.__version__,
             '# "w h" then, for each of the h + 1 rows, the first and last filled column "lo:hi" (1:0 = empty row).',
             '# Written by tools/gen_overlay_golden.py; read by dfl_amd.overlay.']
    for w, h in boxes:
        lines.append('%d %d ' % (w, h) + ' '.join('%d:%d' % s for s in spans_of(pil_stamp(w, h))))
    os.makedirs(os.path.dirname(STAMPS_TXT), exist_ok=True)
    with open(STAMPS_TXT, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return {(w, h): spans_of(pil_stamp(w, h)) for w, h in boxes}


# ---- numpy model of the kernel's marker rules ---------------------------------------------------------------------------
def model_markers(H, W, gt, radius, est, cross, table):
    """Boolean [H, W]: pixels a marker covers.  gt [L,2] (x, y) fp32/fp64, non-finite = none; est [L,2] int, -1 = none."""
    m = np.zeros((H, W), bool)
    if gt is not None:
        r = gt.dtype.type(radius)
        for x, y in gt:
            if not (np.isfinite(x) and np.isfinite(y)):
                continue
            x0, x1, y0, y1 = (math.trunc(float(v)) for v in (x - r, x + r, y - r, y + r))
            spans = table[(x1 - x0, y1 - y0)]
            for j, (lo, hi) in enumerate(spans):
                yy = y0 + j
                if 0 <= yy < H and lo <= hi:
                    a, b = max(x0 + lo, 0), min(x0 + hi, W - 1)
                    if a <= b:
                        m[yy, a:b + 1] = True
    if est is not None:
        for x, y in est:
            if x < 0 or y < 0:
                continue
            if x < W:
                m[max(y - cross, 0):max(min(y + cross, H - 1) + 1, 0), x] = True
            if y < H:
                m[y, max(x - cross, 0):max(min(x + cross, W - 1) + 1, 0)] = True
    return m


def model_render(images, segs, num_classes, heats, gt, radius, est, cross, colors):
    """The kernel's per-pixel rules in numpy fp32 (no grid): uint8 [B,H,W,3]."""
    B, H, W = images.shape
    out = np.zeros((B, H, W, 3), np.uint8)
    k1 = np.float32(1 - 0.35)
    k2 = np.array([[np.float32(0.35 * c) for c in col] for col in colors], np.float32)
    n_tint = min(num_classes - 1, len(colors))
    trunc = gt is not None or est is not None
    for b in range(B):
        x = images[b]
        lo, hi = x.min(), x.max()
        g = np.zeros((H, W), np.uint8) if hi == lo else ((x - lo) / (hi - lo) * np.float32(255)).astype(np.uint8)
        v = np.repeat((g.astype(np.float32) / np.float32(255))[..., None], 3, axis=2)
        if segs is not None:
            for l in range(1, n_tint + 1):
                s = segs[b] == l
                v[s] = k1 * v[s] + k2[l - 1]
        if heats is not None:
            hm = heats[b]
            hl, hh = hm.min(), hm.max()
            h = hm - hl
            if (hh - hl) > np.float32(1e-3):
                h = h / (hh - hl)
            h = h[..., None]
            v = (np.float32(1) - h) * v + h * np.array([0, 1, 0], np.float32)
        if trunc:
            q = np.clip(v * np.float32(255), 0, 255).astype(np.uint8)
        else:
            q = np.clip(v * np.float32(255) + np.float32(0.5), 0, 255).astype(np.uint8)
        mk = model_markers(H, W, None if gt is None else gt[b], radius, None if est is None else est[b], cross, TABLE)
        q[mk] = (255, 255, 0)
        out[b] = q
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------
def make_images(rng, B, H, W, const=False):
    Y, X = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing='ij')
    imgs = np.empty((B, H, W), np.float32)
    for b in range(B):
        imgs[b] = (np.sin(X / (W / 5.0) + b) * np.cos(Y / (H / 3.0)) + 0.3 * rng.standard_normal((H, W))).astype(np.float32)
        imgs[b] = imgs[b] * np.float32(rng.uniform(0.5, 3.0)) + np.float32(rng.uniform(-2, 2))
    if const:
        imgs[:] = np.float32(0.75)
    return imgs


def make_segs(rng, B, H, W, max_label):
    Y, X = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    segs = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        for c in range(1, max_label + 1):
            cx, cy = rng.uniform(0, W), rng.uniform(0, H)
            m = ((X - cx) / (0.3 * W)) ** 2 + ((Y - cy) / (0.25 * H)) ** 2 <= 1
            segs[b][m] = c
    return segs


def make_gt(rng, B, H, W, L):
    """[B, L, 2] fp32 (x, y): fractional positions within 2 px of all four borders, overlapping pairs, non-finite ones."""
    gt = np.empty((B, L, 2), np.float32)
    for b in range(B):
        pts = [(rng.uniform(-0.9, 2.0), rng.uniform(0, H - 1)), (rng.uniform(W - 3.0, W + 0.9), rng.uniform(0, H - 1)),
               (rng.uniform(0, W - 1), rng.uniform(-0.9, 2.0)), (rng.uniform(0, W - 1), rng.uniform(H - 3.0, H + 0.9)),
               (rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5)), (1.2, 0.7), (W - 1.2, H - 0.5), (-1.7, H / 2.0),
               (np.nan, 3.0), (5.0, np.inf), (-np.inf, -np.inf)]
        cx, cy = rng.uniform(4, W - 5), rng.uniform(4, H - 5)
        pts += [(cx, cy), (cx + 1.5, cy + 0.5)]
        while len(pts) < L:
            pts.append((rng.uniform(0, W - 1), rng.uniform(0, H - 1)))
        gt[b] = np.array(pts[:L], np.float32)
    return gt


def make_est(rng, B, H, W, L):
    """[B, L, 2] int32 (col, row), -1 = absent: crosses within 6 px of the borders and overlapping ones."""
    est = np.full((B, L, 2), -1, np.int32)
    for b in range(B):
        pts = [(0, int(rng.integers(0, H))), (W - 1, int(rng.integers(0, H))), (int(rng.integers(0, W)), 0),
               (int(rng.integers(0, W)), H - 1), (3, 4), (W - 4, H - 3), (int(rng.integers(0, W)), int(rng.integers(0, 6)))]
        cx, cy = int(rng.integers(6, W - 6)), int(rng.integers(6, H - 6))
        pts += [(cx, cy), (cx + 3, cy + 2)]
        for k, p in enumerate(pts[:L]):
            if k % 5 != 4 or b == 0:                     # a few absent slots
                est[b, k] = p
    return est


def est_dict(est_b):
    return {l: (int(x), int(y)) for l, (x, y) in enumerate(est_b) if x >= 0 and y >= 0}


def gen_ann(rng, name, B, H, W, seg_max=None, num_classes=7, gt=True, est=True, lands=True, const=False, L=16):
    imgs = make_images(rng, B, H, W, const)
    segs = make_segs(rng, B, H, W, seg_max) if seg_max else None
    g = make_gt(rng, B, H, W, L) if (lands and gt) else None
    e = make_est(rng, B, H, W, 10) if (lands and est) else None
    exp = np.stack([ref_ann(torch.from_numpy(imgs[b]).unsqueeze(0), None if segs is None else torch.from_numpy(segs[b]),
                            num_classes, None if g is None else torch.from_numpy(g[b].T.copy()),
                            None if e is None else est_dict(e[b]), lands) for b in range(B)])
    if lands and g is None:
        g_model = np.full((B, 0, 2), np.nan, np.float32)
    else:
        g_model = g
    mod = model_render(imgs, segs, num_classes, None, g_model, 2, e if (lands or e is not None) else None, 6, ANN_COLORS)
    assert np.array_equal(exp, mod), (name, np.argwhere(exp != mod)[:10])
    d = dict(images=imgs, num_classes=np.int32(num_classes), radius=np.float64(2), cross=np.int32(6),
             colors=np.array(ANN_COLORS, np.float64), grid=np.int32(0), expected=exp)
    if segs is not None:
        d['segs'] = segs
    if lands:
        d['gt_lands'] = g_model
        if e is not None:
            d['est_lands'] = e
    save(name, d)


def gen_heat(rng, name, B, H, W, flat=False):
    imgs = make_images(rng, B, H, W)
    heats = np.empty((B, H, W), np.float32)
    Y, X = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing='ij')
    for b in range(B):
        cx, cy = rng.uniform(0, W), rng.uniform(0, H)
        heats[b] = np.exp(-((X - cx) ** 2 + (Y - cy) ** 2) / np.float32(2 * (W / 8.0) ** 2)).astype(np.float32) * \
            np.float32(rng.uniform(0.01, 0.2)) + np.float32(rng.uniform(-0.01, 0.01))
    if flat:
        heats[0] = np.float32(2e-4) * heats[0] / heats[0].max() + np.float32(0.3)     # range <= 1e-3: not divided
        heats[-1] = np.float32(0.125)                                                   # zero range
    exp = np.stack([ref_heat(torch.from_numpy(imgs[b]).unsqueeze(0), torch.from_numpy(heats[b])) for b in range(B)])
    mod = model_render(imgs, None, 7, heats, None, 2, None, 6, ANN_COLORS)
    assert np.array_equal(exp, mod), (name, np.argwhere(exp != mod)[:10])
    save(name, dict(images=imgs, heats=heats, num_classes=np.int32(7), radius=np.float64(2), cross=np.int32(6),
                    colors=np.array(ANN_COLORS, np.float64), grid=np.int32(0), expected=exp))


def gen_grid(rng, name, B, H, W, L=6):
    projs = make_images(rng, B, H, W) * np.float32(100) + np.float32(500)
    segs = make_segs(rng, B, H, W, 8)
    lands = np.empty((B, 2, L), np.float32)
    for b in range(B):
        lands[b, 0] = rng.uniform(-3, W + 3, L)
        lands[b, 1] = rng.uniform(-3, H + 3, L)
        lands[b, :, 0] = (rng.uniform(0, 1.5), rng.uniform(0, 1.5))
    exp, r = ref_preproc(torch.from_numpy(projs), torch.from_numpy(segs), torch.from_numpy(lands))
    gt = lands.transpose(0, 2, 1).copy()
    x, y = gt[..., 0], gt[..., 1]
    gt[~((x >= 0) & (y >= 0) & (x < W) & (y < W))] = np.nan
    tiles = model_render(projs, segs, 7, None, gt, r, None, 6, PREPROC_COLORS)
    mod = save_image_bytes(torch.from_numpy(tiles).permute(0, 3, 1, 2).float().div(255))
    assert np.array_equal(exp, mod), (name, np.argwhere(exp != mod)[:10])
    save(name, dict(images=projs, segs=segs, gt_lands=gt, lands_raw=lands, num_classes=np.int32(7), radius=np.float64(r),
                    cross=np.int32(6), colors=np.array(PREPROC_COLORS, np.float64), grid=np.int32(1), expected=exp))


def gen_stamps():
    boxes = [(w, h) for w in range(41) for h in range(41) if max(w, h) <= 8 or abs(w - h) <= 1]
    st = np.zeros((len(boxes), 41, 41), np.uint8)
    for k, (w, h) in enumerate(boxes):
        st[k, :h + 1, :w + 1] = pil_stamp(w, h)
    save('overlay_stamps', dict(boxes=np.array(boxes, np.int32), stamps=st))


def save(name, d):
    np.savez_compressed(os.path.join(GOLDEN, name + '.npz'), **d)
    print('wrote', name, {k: getattr(v, 'shape', v) for k, v in d.items() if k != 'expected'})


def check_byte_roundtrip():
    """to_pil_image -> to_tensor -> save_image gives back the byte: the trunc path may quantise once."""
    b = torch.arange(256, dtype=torch.uint8).view(1, 1, 256).expand(3, 1, 256)
    t = to_tensor(Image.fromarray(b.permute(1, 2, 0).numpy().copy(), 'RGB'))
    assert np.array_equal(save_image_bytes(t)[0, :, 0], np.arange(256, dtype=np.uint8))


if __name__ == '__main__':
    assert PIL.__version__.startswith('12.2'), 'the fixtures pin Pillow 12.2 (found %s)' % PIL.__version__
    check_byte_roundtrip()
    TABLE = write_stamp_table()
    rng = np.random.default_rng(20201015)
    gen_ann(rng, 'overlay_ann_184_seg7_lands', 3, 184, 184, seg_max=9, num_classes=7)
    gen_ann(rng, 'overlay_ann_184_noseg_lands', 2, 184, 184)
    gen_ann(rng, 'overlay_ann_184_nolands', 2, 184, 184, seg_max=7, num_classes=7, lands=False)
    gen_ann(rng, 'overlay_ann_46_seg4', 2, 46, 46, seg_max=8, num_classes=4, lands=False)
    gen_ann(rng, 'overlay_ann_46_seg4_gt', 2, 46, 46, seg_max=8, num_classes=4, est=False)
    gen_ann(rng, 'overlay_ann_46_est_only', 2, 46, 46, seg_max=7, gt=False)
    gen_ann(rng, 'overlay_ann_37x53_seg7_lands', 2, 37, 53, seg_max=8, num_classes=7)
    gen_ann(rng, 'overlay_const', 1, 46, 46, seg_max=7, num_classes=7, const=True)
    gen_heat(rng, 'overlay_heat_184', 2, 184, 184)
    gen_heat(rng, 'overlay_heat_46_flat', 2, 46, 46, flat=True)
    gen_heat(rng, 'overlay_heat_37x53', 2, 37, 53)
    gen_grid(rng, 'overlay_grid_48x11', 11, 48, 48)
    gen_stamps()
