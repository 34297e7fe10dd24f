"""Kernel times of the full-resolution overlays (dfl_amd.overlay.render_full_res -> dfl_fullres_overlay) on one GPU.

Cases: 1536^2 x 16 (one chunk of examples/make_full_res_overlays.py) and 1536^2 x 112 (a whole specimen in one call):
random fp32 images, labels 0..7, 14 landmarks and both texts per image, half of the images rotated; and the plain
resample (dfl_resample_bilinear_u8) of 16 RGB 1536^2 images to 192^2.  Each case runs in a child process under
`rocprofv3 --kernel-trace --stats`; the per-kernel mean times come from its kernel_stats.csv, the ms per call from
device events in the child.  Compulsory bytes of the overlay: the image read twice (min / max, then the render) and the
labels once, 9 B per full-resolution pixel; of the resample: 3 B read per input pixel.

    python tools/bench_fullres_overlay.py [--iters 20] [--out profiles/fullres_overlay_bench.json]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S = 1536
CASES = {'overlay_1536x16': (16, 9), 'overlay_1536x112': (112, 9), 'resample_1536x16_to_192': (16, 3)}


def inner(case, iters):
    import numpy as np
    import torch
    from dfl_amd import overlay
    B, _ = CASES[case]
    g = torch.Generator(device='cuda').manual_seed(0)
    if case.startswith('resample'):
        x = (torch.rand((B, S, S, 3), device='cuda', generator=g) * 256).to(torch.uint8)
        run = lambda: overlay.resize_bilinear(x, (S // 8, S // 8))          # noqa: E731
    else:
        imgs = torch.rand((B, S, S), device='cuda', generator=g)
        segs = (torch.rand((B, S, S), device='cuda', generator=g) * 8).to(torch.uint8)
        rng = np.random.default_rng(0)
        lands = [[('FH-l' if l == 0 else 'FH-r' if l == 1 else 'L%02d' % l, rng.uniform(0, S, 2).astype(np.float32))
                  for l in range(14)] for _ in range(B)]
        args = (imgs, segs, [b % 2 for b in range(B)], lands, [(1, 1)] * B)
        run = lambda: overlay.render_full_res(*args)                        # noqa: E731
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    print('RESULT ' + json.dumps(dict(ms_per_call=round(e0.elapsed_time(e1) / iters, 4))))


def profile(case, iters):
    with tempfile.TemporaryDirectory() as d:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', 'run', '--',
               sys.executable, os.path.abspath(__file__), '--inner', case, '--iters', str(iters)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit('%s failed (%d):\n%s' % (case, r.returncode, (r.stdout + r.stderr)[-3000:]))
        line = [l for l in r.stdout.splitlines() if l.startswith('RESULT ')][-1]
        res = json.loads(line[len('RESULT '):])
        stats = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        if not stats:
            raise SystemExit('%s: rocprofv3 wrote no kernel_stats.csv' % case)
        kernels = {}
        with open(stats[0]) as f:
            for row in csv.DictReader(f):
                name = row['Name']
                if name.startswith(('dfl::', 'void dfl::')) or 'fr_render' in name or 'rs_u8' in name or 'ovl_minmax' in name:
                    key = name.split('(')[0].replace('void ', '').replace('dfl::', '')
                    kernels[key] = dict(calls=int(row['Calls']), mean_us=round(float(row['AverageNs']) / 1e3, 2))
        res['kernels'] = kernels
    B, bpp = CASES[case]
    kernel_ms = sum(k['mean_us'] for k in kernels.values()) / 1e3
    res['compulsory_bytes'] = bpp * B * S * S
    res['kernel_ms'] = round(kernel_ms, 4)
    res['kernel_tbps'] = round(bpp * B * S * S / kernel_ms / 1e9, 3) if kernel_ms > 0 else None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--inner', choices=sorted(CASES))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fullres_overlay_bench.json'))
    args = ap.parse_args()
    if args.inner:
        inner(args.inner, args.iters)
        return
    out = {'tool': 'tools/bench_fullres_overlay.py --iters %d (rocprofv3 --kernel-trace --stats per case; ms per call '
                   'by device events, host work included)' % args.iters,
           'cases': {c: profile(c, args.iters) for c in CASES}}
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
