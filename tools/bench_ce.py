"""Times the cross-entropy / focal term (dfl_amd.ce, csrc/ce_loss.hip) at B16 x C7 x 192^2 (the training batch) and
B8 x C7 x 768^2: both stages of dfl_ce_loss -- between device events around each of --reps calls after --warmup calls
(median, min, max), as tools/bench_boundary.py does -- at gamma = 0 (no powf) and gamma = 2, without and with class weights.
Targets are one-hot blob-shaped label maps (tests/labels_ref.py); seg is a soft-max of noise seen through a centre-crop-like
window, and the gradient goes into the same window of a full-size tensor.  Prints one JSON object; --out also writes it.

    python tools/bench_ce.py [--reps 20] [--warmup 3] [--out ce_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, ce  # noqa: E402
import labels_ref as LR  # noqa: E402
from bench_labels import events, stack  # noqa: E402

NUM_CLASSES = LR.NUM_CLASSES


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_ce needs a GPU')
    dev = torch.device('cuda:0')
    res = {'reps': a.reps, 'warmup': a.warmup, 'device': torch.cuda.get_device_name(0), 'shapes': {}}
    for B, side in ((16, 192), (8, 768)):
        Cc, h, w = NUM_CLASSES, side, side
        src = side if side % 180 == 0 else 180 * (side // 180 + 1)
        g_np = stack(B, src, src, 5)[:, :h, :w]
        g = torch.from_numpy(np.ascontiguousarray(g_np)).to(dev)
        target = torch.nn.functional.one_hot(g.long(), Cc).permute(0, 3, 1, 2).float().contiguous()
        out = torch.softmax(torch.randn((B, Cc, h + 8, w + 8), device=dev), dim=1)
        seg = out[..., 4:4 + h, 4:4 + w]                      # what util.center_crop hands to the loss
        counts = np.bincount(g_np.reshape(-1), minlength=Cc)
        loss = torch.zeros((), dtype=torch.float32, device=dev)
        sums = torch.empty(int(nat.lib().dfl_ce_loss_scratch_doubles(B, Cc, h)), dtype=torch.float64, device=dev)
        grad = torch.zeros_like(out)
        st = torch.cuda.current_stream().cuda_stream
        r = {'bytes': {'seg_window': seg.numel() * 4, 'target': target.numel() * 4}}
        for tag, gamma, weights in (('ce', 0.0, None), ('focal_gamma2', 2.0, None),
                                    ('focal_gamma2_balanced', 2.0, ce.balanced_class_weights(counts.tolist()))):
            e = ce._args(seg, target, 1.0, gamma, weights)
            e.loss, e.sums = loss.data_ptr(), sums.data_ptr()
            e.dseg = grad.data_ptr() + 4 * (4 * (w + 8) + 4)
            e.dseg_sN, e.dseg_sC, e.dseg_sH = grad.stride(0), grad.stride(1), grad.stride(2)

            def stage(k, acc, e=e):
                e.stage, e.accumulate_loss, e.accumulate_grad = k, acc, acc
                nat.check(nat.lib().dfl_ce_loss(C.addressof(e), st), 'dfl_ce_loss')
            r[tag] = {'stage1_value': events(lambda: stage(1, 0), a.reps, a.warmup),
                      'stage1_value_accumulate': events(lambda: stage(1, 1), a.reps, a.warmup),
                      'stage2_gradient_write': events(lambda: stage(2, 0), a.reps, a.warmup),
                      'stage2_gradient_accumulate': events(lambda: stage(2, 1), a.reps, a.warmup)}
        res['shapes']['B%dxC%dx%dx%d' % (B, Cc, h, w)] = r
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
