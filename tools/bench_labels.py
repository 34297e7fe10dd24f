"""Times dfl_amd.labels.clean(keep='largest', fill_holes=16) on two stacks of blob-shaped label maps -- [110, 180, 180] (a
patient's worth at 8x down-sampling) and [8, 1440, 1440] -- between device events around each of --reps calls after
--warmup calls (median, min, max), its parts (components at either connectivity, one bone_mask), and the host's time for
the labelling alone: scipy.ndimage.label per image and label with the sizes by np.bincount and the keep-largest assignment,
then one 4-connected labelling of the background per image (the component search of the hole filling; the neighbour test of
the holes is left out, so the host figure is a lower bound of the same work).  Prints one JSON object; --out also writes it.

    python tools/bench_labels.py [--reps 20] [--warmup 3] [--host-reps 3] [--out labels_bench.json]
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
import dfl_amd  # noqa: E402,F401
from dfl_amd import labels  # noqa: E402
import labels_ref as LR  # noqa: E402

NUM_CLASSES = LR.NUM_CLASSES


def stack(B, H, W, seed):
    """Blobs at the scale of 180 x 180 (tests/labels_ref.py: blobs), enlarged to H x W, then speckled again at full size."""
    f = H // 180
    seg = LR.blobs(B, 180, 180, seed=seed)
    if f > 1:
        seg = np.repeat(np.repeat(seg, f, axis=1), f, axis=2)
        rng = np.random.default_rng(seed + 1)
        noise = rng.random(seg.shape)
        seg[noise < 0.002] = rng.integers(0, NUM_CLASSES, size=int((noise < 0.002).sum()))
    assert seg.shape == (B, H, W)
    return np.ascontiguousarray(seg)


def events(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {'median_ms': float(np.median(ts)), 'min_ms': float(np.min(ts)), 'max_ms': float(np.max(ts))}


def host_labelling(segs, ndi):
    eight = np.ones((3, 3), dtype=int)
    out = segs.copy()
    for b in range(segs.shape[0]):
        for l in range(1, NUM_CLASSES):
            lab, n = ndi.label(segs[b] == l, structure=eight)
            if n > 1:
                sizes = np.bincount(lab.ravel())
                sizes[0] = 0
                out[b][(lab > 0) & (lab != sizes.argmax())] = 0
        lab, n = ndi.label(out[b] == 0)
        np.bincount(lab.ravel())
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_labels needs a GPU')
    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    dev = torch.device('cuda:0')
    res = {'reps': a.reps, 'warmup': a.warmup, 'device': torch.cuda.get_device_name(0), 'tile': list(labels.TILE), 'stacks': {}}
    for B, H, W in ((110, 180, 180), (8, 1440, 1440)):
        segs_np = stack(B, H, W, 5)
        segs = torch.from_numpy(segs_np).to(dev)
        cleaned, stats = labels.clean(segs, keep='largest', fill_holes=16)
        r = {'removed_pixels': int(stats['removed'].sum()), 'filled_pixels': int(stats['filled'].sum()),
             'components_8': int((labels.components(segs, 8)[1] > 0).sum()),
             'clean': events(lambda: labels.clean(segs, keep='largest', fill_holes=16), a.reps, a.warmup),
             'components_8_only': events(lambda: labels.components(segs, 8), a.reps, a.warmup),
             'components_4_only': events(lambda: labels.components(segs, 4), a.reps, a.warmup),
             'bone_mask_dilate_7': events(lambda: labels.bone_mask(segs, (1, 2), 7), a.reps, a.warmup),
             'bone_mask_dilate_32': events(lambda: labels.bone_mask(segs, (1, 2), 32), a.reps, a.warmup)}
        if ndi is not None:
            ts = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter()
                host = host_labelling(segs_np, ndi)
                ts.append((time.perf_counter() - t0) * 1e3)
            r['host_scipy_label'] = {'median_ms': float(np.median(ts)), 'min_ms': float(np.min(ts)), 'max_ms': float(np.max(ts))}
            stage1, _ = labels.clean(segs, keep='largest')
            r['host_stage1_equals_device'] = bool(np.array_equal(host, stage1.cpu().numpy()))
        res['stacks']['%dx%dx%d' % (B, H, W)] = r
    # the worst case for the finds: every image one serpentine, a single path half the image long
    snake = torch.from_numpy(np.stack([np.array(LR.serpentine(1440, 1440, labels.TILE))] * 8)).to(dev)
    assert int((labels.components(snake, 4)[1] > 0).sum()) == 8 * (1 + 720)      # per image the path and 720 rows of background
    res['serpentine_8x1440x1440'] = {'components_8_only': events(lambda: labels.components(snake, 8), a.reps, a.warmup),
                                     'components_4_only': events(lambda: labels.components(snake, 4), a.reps, a.warmup)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
