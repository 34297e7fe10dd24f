"""Writes tests/golden/aug_*.npz: augmented items for EXPLICIT parameters, computed by the numpy restatement of the
reference's augmentation (tests/aug_ref.py).  torchvision is not needed (its affine matrix is restated there); the CPU
tests pin the restatement's warp against PIL.  Each file: the raw inputs (projs, segs, lands), the parameters (flags,
sigma, gamma, angle, translate, scale, shear, noise_key, boxes + n_box), and per item the outputs: x (standardised),
levels (8-bit warp), labels (255 = outside the warped frame), near (label pixels whose source coordinate lies within 1e-6
of an integer), lands_reference / lands_in_view.

    python tools/gen_aug_golden.py
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import aug_ref as A  # noqa: E402

# name: H, W, pad, C, L, flags of the items (the affine warp always runs; 'identity' = identity affine parameters)
CASES = {
    'aug_46_p0': (46, 46, 0, 4, 3, [15, 'identity', 1, 2, 4, 8]),
    'aug_46_p1': (46, 46, 1, 4, 3, [15, 0, 14]),
    'aug_192_p0': (192, 192, 0, 7, 14, [15, 6]),
    'aug_192_p2': (192, 192, 2, 7, 14, [15, 9]),
    'aug_37x53_p3': (37, 53, 3, 5, 4, [15, 10, 5]),
}


def inputs(rng, n, H, W, C, L):
    Y, X = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing='ij')
    projs = (0.05 * rng.standard_normal((n, H, W)) + 1.0).astype(np.float32)
    segs = np.zeros((n, H, W), np.uint8)
    lands = np.zeros((n, 2, L), np.float32)
    for i in range(n):
        projs[i] += (0.3 * np.sin(X / (W / 3.0) + i) * np.cos(Y / (H / 4.0))).astype(np.float32)
        for c in range(1, C):
            cx, cy = rng.uniform(0.25 * W, 0.75 * W), rng.uniform(0.25 * H, 0.75 * H)
            m = ((X - cx) / (0.15 * W)) ** 2 + ((Y - cy) / (0.12 * H)) ** 2 <= 1
            segs[i][m] = c
            projs[i][m] += np.float32(0.2 * c)
        lands[i, 0] = rng.uniform(0, W - 1, L)
        lands[i, 1] = rng.uniform(0, H - 1, L)
        if L > 2:
            lands[i, :, 0] = (W - 1.5, 2.0)               # near the right edge and the top rows: both rules act
            lands[i, :, 1] = np.inf
    return projs * np.float32(1000.0) + np.float32(50.0), segs, lands


def params(rng, flags, Ho, Wo):
    ident = flags == 'identity'
    flags = 0 if ident else flags
    d = rng.standard_normal(2)
    t = d / np.linalg.norm(d) * rng.random() * 20.0
    prm = dict(flags=flags, sigma=float(rng.uniform(0.005, 0.01)), gamma=float(rng.uniform(0.7, 1.3)),
               angle=0.0 if ident else float(rng.uniform(-5, 5)), translate=(0.0, 0.0) if ident else (float(t[0]), float(t[1])),
               scale=1.0 if ident else float(rng.uniform(0.9, 1.1)),
               shear=(0.0, 0.0) if ident else (float(rng.uniform(-1, 1)), float(rng.uniform(-1, 1))),
               noise_key=int(rng.integers(0, 1 << 63)), boxes=[])
    if flags & A.ERASE:
        mean = np.array([Ho * 0.15, Wo * 0.15], np.float32)
        for _ in range(int(rng.integers(2, 6))):
            while True:
                dims = np.round(rng.standard_normal(2).astype(np.float32) * mean + mean).astype(np.int64)
                if 0 < dims[0] <= Ho and 0 < dims[1] <= Wo:
                    break
            r0, c0 = int(rng.integers(0, Ho - dims[0] + 1)), int(rng.integers(0, Wo - dims[1] + 1))
            prm['boxes'].append((r0, c0, int(dims[0]), int(dims[1]), int(rng.integers(0, 1 << 63))))
        # overlapping boxes: the second one covers part of the first
        r0, c0, nr, nc, _ = prm['boxes'][0]
        prm['boxes'][1] = (r0 + nr // 2, c0 + nc // 2, max(min(nr, Ho - r0 - nr // 2), 1), max(min(nc, Wo - c0 - nc // 2), 1),
                           prm['boxes'][1][4])
    return prm


def main():
    out_dir = os.path.join(ROOT, 'tests', 'golden')
    for name, (H, W, pad, C, L, flag_list) in CASES.items():
        rng = np.random.default_rng(sum(map(ord, name)))
        n = len(flag_list)
        projs, segs, lands = inputs(rng, n, H, W, C, L)
        Ho, Wo = H + 2 * pad, W + 2 * pad
        prms = [params(rng, f, Ho, Wo) for f in flag_list]
        d = dict(projs=projs, segs=segs, lands=lands, H=H, W=W, pad=pad, C=C, L=L)
        d['flags'] = np.array([p['flags'] for p in prms], np.int32)
        for k in ('sigma', 'gamma', 'angle', 'scale'):
            d[k] = np.array([p[k] for p in prms], np.float64)
        d['translate'] = np.array([p['translate'] for p in prms], np.float64)
        d['shear'] = np.array([p['shear'] for p in prms], np.float64)
        d['noise_key'] = np.array([p['noise_key'] for p in prms], np.uint64)
        d['n_box'] = np.array([len(p['boxes']) for p in prms], np.int32)
        boxes = np.zeros((n, 5, 5), np.uint64)
        for i, p in enumerate(prms):
            for b, bx in enumerate(p['boxes']):
                boxes[i, b] = bx
        d['boxes'] = boxes
        xs, levs, labs, nears, lr, li = [], [], [], [], [], []
        for i, p in enumerate(prms):
            o = A.augment_item(projs[i], segs[i], lands[i], p, pad, C, land_rule='reference')
            o2 = A.augment_item(projs[i], segs[i], lands[i], p, pad, C, land_rule='in_view')
            xs.append(o['x'])
            levs.append(o['levels'])
            labs.append(o['labels'])
            sx, sy = o['label_src']
            nears.append((np.abs(sx - np.round(sx)) < 1e-6) | (np.abs(sy - np.round(sy)) < 1e-6))
            lr.append(o['lands'])
            li.append(o2['lands'])
        d.update(x=np.stack(xs), levels=np.stack(levs), labels=np.stack(labs), near=np.stack(nears),
                 lands_reference=np.stack(lr), lands_in_view=np.stack(li))
        path = os.path.join(out_dir, name + '.npz')
        np.savez_compressed(path, **d)
        print('wrote %s (%d items, %d bytes)' % (path, n, os.path.getsize(path)))


if __name__ == '__main__':
    main()
