"""Times the boundary loss (dfl_amd.boundary, csrc/boundary.hip) at B16 x C7 x 192^2 (the training batch) and B8 x C7 x 768^2:
dfl_boundary_maps, and both stages of dfl_boundary_loss -- between device events around each of --reps calls after --warmup
calls (median, min, max), as tools/bench_labels.py does.  For the accounting of the maps it also times the distance
transforms alone (labels.edt's entry over the same pairs of label sets, cut into the same chunks of classes), so that
maps - edt = arg-max + combine.  Targets are one-hot blob-shaped label maps (tests/labels_ref.py); seg is a soft-max of noise
seen through a centre-crop-like window.  Prints one JSON object; --out also writes it.

    python tools/bench_boundary.py [--reps 20] [--warmup 3] [--out boundary_bench.json]
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
from dfl_amd import _native as nat, boundary, labels  # noqa: E402
import labels_ref as LR  # noqa: E402
from bench_labels import events, stack  # noqa: E402

NUM_CLASSES = LR.NUM_CLASSES
CHUNK_BYTES = 256 << 20          # csrc/boundary.hip: MAP_CHUNK_BYTES


def classes_per_chunk(B, Cc, h, w):
    pairs = max(1, CHUNK_BYTES // (2 * (2 * h * w + 1) * 4))
    return max(1, min(Cc, 15, pairs // B))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_boundary needs a GPU')
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
        phi = boundary.signed_distance_maps(target)
        CK = classes_per_chunk(B, Cc, h, w)
        sets = [[1 << c, ((1 << Cc) - 1) & ~(1 << c)] for c in range(Cc)]
        chunks = [sum(sets[c0:c0 + CK], []) for c0 in range(0, Cc, CK)]
        rowdist = torch.empty(B * 2 * CK * (h * w + 1), dtype=torch.int32, device=dev)
        d2 = torch.empty((B, 2 * CK, h, w), dtype=torch.int32, device=dev)

        def edt_only():
            for words in chunks:
                labels._edt(g, words, False, rowdist, d2)      # (a shorter last chunk fills the front of d2)
        b = boundary._args(seg, phi, False, 0.01)
        loss = torch.zeros((), dtype=torch.float32, device=dev)
        sums = torch.empty(int(nat.lib().dfl_boundary_loss_scratch_doubles(B, Cc, h)), dtype=torch.float64, device=dev)
        grad = torch.zeros_like(out)
        b.loss, b.sums = loss.data_ptr(), sums.data_ptr()
        b.dseg = grad.data_ptr() + 4 * (4 * (w + 8) + 4)
        b.dseg_sN, b.dseg_sC, b.dseg_sH = grad.stride(0), grad.stride(1), grad.stride(2)
        st = torch.cuda.current_stream().cuda_stream

        def stage(k, acc):
            b.stage, b.accumulate_loss, b.accumulate_grad = k, 0, acc
            nat.check(nat.lib().dfl_boundary_loss(C.addressof(b), st), 'dfl_boundary_loss')
        r = {'classes_per_edt_call': CK, 'edt_calls': len(chunks),
             'maps': events(lambda: boundary.signed_distance_maps(target), a.reps, a.warmup),
             'edt_passes_only': events(edt_only, a.reps, a.warmup),
             'loss_stage1_value': events(lambda: stage(1, 0), a.reps, a.warmup),
             'loss_stage2_gradient_write': events(lambda: stage(2, 0), a.reps, a.warmup),
             'loss_stage2_gradient_accumulate': events(lambda: stage(2, 1), a.reps, a.warmup),
             'bytes': {'phi': phi.numel() * 4, 'seg_window': seg.numel() * 4,
                       'maps_scratch': int(nat.lib().dfl_boundary_maps_scratch_bytes(B, Cc, h, w))}}
        res['shapes']['B%dxC%dx%dx%d' % (B, Cc, h, w)] = r
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
