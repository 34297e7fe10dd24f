"""Times dfl_amd.labels.surface_distances and labels.edt alone on two stacks of blob-shaped label maps against a perturbed
copy -- [110, 180, 180] (a patient's worth at 8x down-sampling) and [8, 1440, 1440] -- and the worst case of the column pass,
a single site in one corner of a 1440 x 1440 image, between device events around each of --reps calls after --warmup calls
(median, min, max).  The host's time for the same: scipy.ndimage.distance_transform_edt per image, label and direction on the
eroded outlines -- a lower bound, the percentile, the means and the copies are left out.  Prints one JSON object; --out also
writes it.

    python tools/bench_surface_dist.py [--reps 20] [--warmup 3] [--host-reps 3] [--out surface_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfl_amd  # noqa: E402,F401
from dfl_amd import labels  # noqa: E402
import labels_ref as LR  # noqa: E402
from bench_labels import events, stack  # noqa: E402

NUM_CLASSES = LR.NUM_CLASSES


def perturbed(gt, seed):
    """The estimate: the ground truth shifted by (2, -1) and speckled."""
    est = np.roll(gt, (2, -1), axis=(1, 2))
    rng = np.random.default_rng(seed)
    noise = rng.random(est.shape)
    est[noise < 0.002] = rng.integers(0, NUM_CLASSES, size=int((noise < 0.002).sum()))
    return np.ascontiguousarray(est)


def host_distances(est, gt, ndi):
    """Per image, label and direction one erosion and one distance transform; -> the largest distance met."""
    four = ndi.generate_binary_structure(2, 1)
    worst = 0.0
    for b in range(est.shape[0]):
        for l in range(1, NUM_CLASSES):
            e, g = est[b] == l, gt[b] == l
            e &= ~ndi.binary_erosion(e, structure=four, border_value=0)
            g &= ~ndi.binary_erosion(g, structure=four, border_value=0)
            if e.any() and g.any():
                worst = max(worst, float(ndi.distance_transform_edt(~g)[e].max()), float(ndi.distance_transform_edt(~e)[g].max()))
    return worst


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_surface_dist needs a GPU')
    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    dev = torch.device('cuda:0')
    sets = [[l] for l in range(1, NUM_CLASSES)]
    res = {'reps': a.reps, 'warmup': a.warmup, 'device': torch.cuda.get_device_name(0), 'chunk_bytes': labels.SURFACE_CHUNK_BYTES,
           'stacks': {}}
    for B, H, W in ((110, 180, 180), (8, 1440, 1440)):
        gt_np = stack(B, H, W, 5)
        est_np = perturbed(gt_np, 6)
        gt, est = torch.from_numpy(gt_np).to(dev), torch.from_numpy(est_np).to(dev)
        out = labels.surface_distances(est, gt)
        fin = torch.isfinite(out['hd'])
        r = {'boundary_pixels_est': int(out['n_est'].sum()), 'boundary_pixels_gt': int(out['n_gt'].sum()),
             'largest_hd': float(out['hd'][fin].max()), 'mean_assd': float(out['assd'][fin].mean()),
             'surface_distances': events(lambda: labels.surface_distances(est, gt), a.reps, a.warmup),
             'edt_six_labels_boundary': events(lambda: labels.edt(gt, sets, True), a.reps, a.warmup),
             'edt_one_set_of_two': events(lambda: labels.edt(gt, (1, 2)), a.reps, a.warmup)}
        if ndi is not None:
            ts = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter()
                worst = host_distances(est_np, gt_np, ndi)
                ts.append((time.perf_counter() - t0) * 1e3)
            r['host_scipy_edt'] = {'median_ms': float(np.median(ts)), 'min_ms': float(np.min(ts)), 'max_ms': float(np.max(ts))}
            r['host_largest_hd_equals_device'] = bool(worst == r['largest_hd'])
        res['stacks']['%dx%dx%d' % (B, H, W)] = r
    # the worst case of the column pass: one site in a corner, every pixel's search runs to the first row
    corner = torch.zeros((1, 1440, 1440), dtype=torch.uint8, device=dev)
    corner[0, 0, 0] = 1
    far = labels.edt(corner, 1)
    assert int(far[0, -1, -1]) == 2 * 1439 ** 2 and int(far.max()) == 2 * 1439 ** 2
    res['corner_site_1x1440x1440'] = {'edt': events(lambda: labels.edt(corner, 1), a.reps, a.warmup)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
