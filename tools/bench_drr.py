"""Times of the DRR renderer (dfl_amd.drr -> dfl_drr_render, csrc/drr.hip) on one GPU.

A synthetic CT of 384 x 320 x 400 voxels of 0.8 mm with three label blobs (a pelvis-sized one labelled 1 and two
femur-sized ones labelled 5 and 6) under three poses that differ, 800 mm from the source, seen by a 1536 x 1536
detector of 0.194 mm pixels: at factor 1 without crop (2.4 M rays per view, 2 views per launch) and on the training
grid, crop 50 and factor 8 (180 x 180, 32 views per launch); exact and trilinear (step 0.5 mm); tight boxes on and off;
and the 8 x 8-tile thread mapping against the 64 x 1 row mapping, alternating in the same run.

Timed with device events around back-to-back calls of the C entry point (the argument block is built once: no host
work between launches), after a warm-up of every case, `reps` windows of at least --window seconds each; the median is
reported with the spread.  Work is counted from the geometry by code kept here, in float64 on the device: in exact mode
the voxels a ray visits in an object's box (the planes it crosses between entry and exit, plus one); in trilinear mode
the samples (8 voxel reads each).  Rates are that count over the median time.  There is no earlier implementation to
compare against; the outputs of the two mappings are compared bit for bit before anything is timed.

    python tools/bench_drr.py [--window 0.3] [--reps 5] [--out profiles/drr_bench.json]
"""
import argparse
import datetime
import json
import os
import socket
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NX, NY, NZ, SPACING = 384, 320, 400, 0.8
DET, PIXEL_MM, CROP = 1536, 0.194, 50
STEP_MM = 0.5
BLOBS = (((192, 150, 200), (120, 90, 110), 1), ((90, 200, 90), (35, 35, 80), 5), ((294, 200, 90), (35, 35, 80), 6))


def rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    R = np.eye(4)
    i, j = [(1, 2), (0, 2), (0, 1)][axis]
    R[i, i] = R[j, j] = c
    R[i, j], R[j, i] = -s, s
    return R


def phantom(dev):
    """(mu float32, labels uint8) [NZ, NY, NX] on the device, nothing random."""
    import torch
    from dfl_amd import drr
    z, y, x = torch.meshgrid(torch.arange(NZ, device=dev, dtype=torch.float32), torch.arange(NY, device=dev, dtype=torch.float32),
                             torch.arange(NX, device=dev, dtype=torch.float32), indexing='ij')
    lab = torch.zeros((NZ, NY, NX), dtype=torch.uint8, device=dev)
    for ctr, rad, l in BLOBS:
        lab[((x - ctr[0]) / rad[0]) ** 2 + ((y - ctr[1]) / rad[1]) ** 2 + ((z - ctr[2]) / rad[2]) ** 2 < 1] = l
    hu = -1000 + 1000 * torch.exp(-(((x - 192) / 170) ** 2 + ((y - 160) / 140) ** 2 + ((z - 200) / 180) ** 2) ** 2) \
        + 700 * (lab > 0) + 40 * torch.sin(0.09 * x + 0.07 * y + 0.05 * z)
    return drr.hu_to_mu(hu), lab


def poses(n_views):
    """[[C2I per object] per view]: index coordinates <- camera projective frame, every view turned a little more."""
    I2P = np.eye(4)
    I2P[:3, :3] *= SPACING
    I2P[:3, 3] = [-150.0, -120.0, -160.0]
    ctr = (I2P @ np.array([(NX - 1) / 2, (NY - 1) / 2, (NZ - 1) / 2, 1]))[:3]
    out = []
    for v in range(n_views):
        view = []
        for n, (R, shift) in enumerate(((rot(0, 0.5) @ rot(2, 0.3), (3, -4, -800)), (rot(0, 0.6) @ rot(2, 0.25), (6, -2, -790)),
                                        (rot(0, 0.4) @ rot(1, 0.2), (-1, -6, -810)))):
            R = R @ rot(1, 0.02 * v) @ rot(0, -0.015 * v * (n + 1))
            V2C = np.eye(4)                                   # volume physical frame -> camera projective frame
            V2C[:3, :3] = R[:3, :3]
            V2C[:3, 3] = np.array(shift) - R[:3, :3] @ ctr
            view.append(np.linalg.inv(I2P) @ np.linalg.inv(V2C))
        out.append(view)
    return out


def count_work(recs, Q, H, W, interp, dev):
    """Voxels visited (exact) or samples taken (trilinear), summed over views, objects and rays."""
    import torch
    r, c = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing='ij')
    pix = torch.stack([c.reshape(-1), r.reshape(-1), torch.ones(H * W, device=dev, dtype=torch.float64)])
    s = (torch.from_numpy(np.asarray(Q, np.float32).astype(np.float64)).to(dev) @ pix).norm(dim=0)
    total = 0
    for rec in recs.reshape(-1):
        lo = torch.tensor(rec['box_lo'].astype(np.float64), device=dev)[:, None] - 0.5
        hi = torch.tensor(rec['box_hi'].astype(np.float64), device=dev)[:, None] + 0.5
        if bool((hi < lo).any()):
            continue
        o = torch.tensor(rec['o'].astype(np.float64), device=dev)[:, None]
        d = torch.tensor(rec['M'].astype(np.float64).reshape(3, 3), device=dev) @ pix
        ta, tb = (lo - o) / d, (hi - o) / d
        t0 = torch.minimum(ta, tb).amax(0).clamp(min=0.0)
        t1 = torch.maximum(ta, tb).amin(0)
        ok = t1 > t0
        if interp == 'exact':
            v0 = torch.floor(o + t0 * d + 0.5).clamp(min=lo + 0.5, max=hi - 0.5)
            v1 = torch.floor(o + t1 * d + 0.5).clamp(min=lo + 0.5, max=hi - 0.5)
            n = (v1 - v0).abs().sum(0) + 1
        else:
            n = torch.ceil(s * (t1 - t0) / STEP_MM).clamp(min=1.0)
        total += int(n[ok].sum().item())
    return total


def timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=0.3, help='seconds of device work per timed window, at least')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'drr_bench.json'))
    args = ap.parse_args()
    import torch
    from dfl_amd import _native as nat, drr
    if not torch.cuda.is_available():
        raise SystemExit('bench_drr.py needs a GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda', 0)
    mu, lab = phantom(dev)
    vol = drr.Volume(mu, lab)
    f = 1000.0 / PIXEL_MM
    K = np.array([[-f, 0, 767.5], [0, -f, 767.5], [0, 0, 1]])
    stream = torch.cuda.current_stream(dev).cuda_stream
    prop = torch.cuda.get_device_properties(dev)
    res = {'tool': 'tools/bench_drr.py --window %g --reps %d (device events around back-to-back calls; median of the repetitions; '
                   'the two thread mappings alternate)' % (args.window, args.reps),
           'date': datetime.date.today().isoformat(), 'host': socket.gethostname(), 'device': torch.cuda.get_device_name(dev),
           'arch': getattr(prop, 'gcnArchName', ''), 'compute_units': prop.multi_processor_count, 'torch': torch.__version__,
           'hip': torch.version.hip, 'volume': [NX, NY, NZ], 'voxel_mm': SPACING, 'step_mm': STEP_MM,
           'boxes': {str(m): vol.box(drr.label_mask(m)) for m in drr.DEFAULT_MASKS}, 'cases': {}}
    for factor, crop, n_views in ((1, 0, 2), (8, CROP, 32)):
        G, (H, W) = drr.training_grid(DET, DET, crop, factor)
        grid = drr.Grid(-np.linalg.inv(K) @ G, H, W)
        objs = [[drr.Obj(A, m) for A, m in zip(view, drr.DEFAULT_MASKS)] for view in poses(n_views)]
        for interp in ('exact', 'trilinear'):
            for tight in (True, False):
                runs, outs = {}, {}
                for name, mapping in (('tile8x8', 0), ('row64x1', 1)):
                    a, out, keep = drr.render_args(vol, objs, grid, interp=interp, step_mm=STEP_MM, want_plen=False,
                                                   want_labels=interp == 'exact', tight_boxes=tight, mapping=mapping)
                    runs[name] = (lambda a=a: nat.call('dfl_drr_render', a, stream))
                    outs[name] = (out, keep)
                first = {k: timed(fn, 1) for k, fn in runs.items()}                  # warm-up of every case that is timed
                same = all(torch.equal(x, y) for x, y in zip(outs['tile8x8'][0], outs['row64x1'][0]) if x is not None)
                assert same, 'the two mappings must give the same bits'
                iters = {k: max(int(1e3 * args.window / max(timed(fn, 1), 1e-3)) + 1, 1) for k, fn in runs.items()}
                ms = {k: [] for k in runs}
                for _ in range(args.reps):                                           # alternating: one box, one moment
                    for k, fn in runs.items():
                        ms[k].append(timed(fn, iters[k]))
                recs = drr.pack_objects(vol, objs, grid, interp, tight)
                work = count_work(recs, grid.Q, H, W, interp, dev)
                case = {'output': [H, W], 'views_per_launch': n_views, 'rays_per_view': H * W,
                        'work_unit': 'voxels visited' if interp == 'exact' else 'samples (8 voxel reads each)',
                        'work_per_view': work // n_views, 'work_per_ray_and_object': round(work / (n_views * H * W * 3), 1)}
                for k in runs:
                    m = statistics.median(ms[k])
                    case[k] = {'launches_per_window': iters[k], 'first_launch_ms': round(first[k], 3), 'ms_per_view': round(m / n_views, 4),
                               'min_ms_per_view': round(min(ms[k]) / n_views, 4), 'max_ms_per_view': round(max(ms[k]) / n_views, 4),
                               'work_per_second': round(work / m * 1e3, -6)}
                case['row_over_tile'] = round(case['row64x1']['ms_per_view'] / case['tile8x8']['ms_per_view'], 3)
                key = 'f%d/%s/%s' % (factor, interp, 'tight' if tight else 'full')
                res['cases'][key] = case
                print('%-22s %4d x %-4d  %.1f %s per ray and object: 8 x 8 tiles %.4f ms per view (%.3g per second), 64 x 1 rows '
                      '%.4f ms: %.2fx' % (key, H, W, case['work_per_ray_and_object'], case['work_unit'].split(' (')[0],
                                          case['tile8x8']['ms_per_view'], case['tile8x8']['work_per_second'],
                                          case['row64x1']['ms_per_view'], case['row_over_tile']), flush=True)
                del runs, outs
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
