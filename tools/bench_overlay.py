"""Cost of the result overlays (dfl_amd.overlay.render -> dfl_overlay_batch) on one GPU, beside the host PNG encode.

Cases: 184^2 x 1 and x 16 (the annotation script's size), and 1536^2 x 64 as tiles and as one make_grid canvas (the
preproc example at full resolution): labels, 7 colours, 14 ellipse markers per image.  ms per render by device events;
bytes of the pass = image read twice (min/max, then the pixel pass) + labels + 3 B written = 12 B per pixel.
Run under rocprofv3 --kernel-trace --stats for the per-kernel times.

Prints one JSON line.   python tools/bench_overlay.py [--iters 20]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    args = ap.parse_args()
    from dfl_amd import overlay, png
    g = torch.Generator(device='cuda').manual_seed(0)
    res = {}
    for name, B, S, grid in (('184x1', 1, 184, False), ('184x16', 16, 184, False), ('1536x64', 64, 1536, False),
                             ('1536x64_grid', 64, 1536, True)):
        imgs = torch.rand((B, S, S), device='cuda', generator=g)
        segs = (torch.rand((B, S, S), device='cuda', generator=g) * 8).to(torch.uint8)
        lands = torch.rand((B, 14, 2), device='cuda', generator=g) * S
        r = max(16 * S / 1536.0, 3.0)
        for _ in range(3):
            out = overlay.render(imgs, segs=segs, gt_lands=lands, radius=r, grid=grid)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            out = overlay.render(imgs, segs=segs, gt_lands=lands, radius=r, grid=grid)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.iters
        res[name] = dict(ms=round(ms, 4), bytes=12 * B * S * S, gbps=round(12.0 * B * S * S / ms / 1e6, 1))
        if name == '184x1' or name == '1536x64':
            tile = out[0].cpu().numpy()
            t0 = time.time()
            for _ in range(3):
                png.encode(tile)
            res[name]['png_encode_ms_per_image'] = round((time.time() - t0) / 3 * 1e3, 2)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
