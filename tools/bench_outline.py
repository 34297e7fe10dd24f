"""Times of one optimiser generation of dfl_amd.register(similarity='outline') on one GPU, split into its three parts, and
of the same numbers through labels.surface_distances.

tools/bench_drr.py's phantom (384 x 320 x 400 voxels of 0.8 mm, three label blobs under three poses) on the training grid,
crop 50 and factor 8 (180 x 180), V = 16 candidates per generation, S = 6 label sets ({1} .. {6}); the segmentation is the
exact label map at the phantom's poses and the candidates are drawn around a start 2 units away in every parameter.

  render             dfl_drr_render, exact, tight boxes, 16 views, att and label_map written
  edt                dfl_label_edt of the 16 label maps for the 6 sets, boundary 1 (memset and two kernels)
  outline            dfl_sim_outline on those distance maps (two kernels)
  generation         the three, back to back, as OutlineSimilarity.cost after the render issues them
  surface_distances  labels.surface_distances(views, the segmentation repeated 16 times): the raw directed means of the
                     same boundaries per label, with its own distance transforms of both sides, its reads of counts in the
                     middle and its host tensors at the end (no truncation, no cost)
  register           a whole generation of register(similarity='outline') by the wall clock: with sampling, packing, the
                     upload of the records, the copy of 16 doubles and the CMA-ES update

Device events around each of --reps calls after --warmup calls (argument blocks built once); median, min and max.  Prints one
JSON object; --out also writes it.

    python tools/bench_outline.py [--reps 30] [--warmup 5] [--out outline_bench.json]
"""
import argparse
import datetime
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import bench_drr as B  # noqa: E402
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, drr, labels, register as reg  # noqa: E402
from bench_labels import events  # noqa: E402

FACTOR, VIEWS, CAP = 8, 16, 32.0
SETS = [[l] for l in range(1, 7)]
THETA0 = (2.0, -2.0, 2.0, 2.0, -2.0, 2.0)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--generations', type=int, default=20, help='generations of the wall-clock run of register()')
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_outline.py needs a GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda', 0)
    mu, lab = B.phantom(dev)
    vol = drr.Volume(mu, lab)
    f = 1000.0 / B.PIXEL_MM
    K = np.array([[-f, 0, 767.5], [0, -f, 767.5], [0, 0, 1]])
    G, (H, W) = drr.training_grid(B.DET, B.DET, B.CROP, FACTOR)
    grid = drr.Grid(-np.linalg.inv(K) @ G, H, W)
    I2P = np.eye(4)
    I2P[:3, :3] *= B.SPACING
    I2P[:3, 3] = [-150.0, -120.0, -160.0]
    c2is = B.poses(1)[0]
    objects = [drr.Obj(A, m) for A, m in zip(c2is, drr.DEFAULT_MASKS)]
    poses = {k: I2P @ A for k, A in zip(drr.POSES, c2is)}                             # P = I2P C2I E, E = identity
    geom = drr.Geometry(K, np.eye(4), poses, I2P, G, objects, grid)
    seg = drr.render(vol, objects, grid)[2].clone()
    stream = torch.cuda.current_stream(dev).cuda_stream
    ctr = reg.volume_centre(vol.shape, I2P)
    thetas = np.asarray(THETA0)[None] + 2.0 * np.random.default_rng(0).standard_normal((VIEWS, 6))
    A = np.linalg.inv(I2P)[None] @ reg.pose_deltas(thetas, ctr) @ I2P[None]
    views = [[drr.Obj(A[v] @ ob.c2i, ob.mask) for ob in objects] for v in range(VIEWS)]
    ra, (_, _, maps), keep = drr.render_args(vol, views, grid, interp='exact', want_labels=True)
    sim = reg.OutlineSimilarity(seg, SETS, VIEWS, CAP)
    oa = sim.args(VIEWS)

    def edt():
        labels._edt(maps, sim.words, True, sim.rowdist, sim.d2_moving)

    def outline():
        nat.call('dfl_sim_outline', oa, stream)

    def generation():
        nat.call('dfl_drr_render', ra, stream)
        sim._launch(maps)

    generation()
    cost = sim.out.cpu().numpy()
    assert np.isfinite(cost).all() and (cost > 0).all() and (cost <= 1).all(), cost
    repeated = seg[None].expand(VIEWS, H, W).contiguous()
    sd = labels.surface_distances(maps, repeated)
    # the same boundaries: where a label is in both maps, (a / nM + b / nF) / 2 uncapped is the ASSD
    counts = sim.counts.cpu().numpy()
    assert np.array_equal(counts[..., 0], sd['n_est'].numpy()) and np.array_equal(counts[..., 1], sd['n_gt'].numpy())
    prop = torch.cuda.get_device_properties(dev)
    res = {'tool': 'tools/bench_outline.py --reps %d --warmup %d (device events around each call; median, min, max)' % (a.reps, a.warmup),
           'date': datetime.date.today().isoformat(), 'device': torch.cuda.get_device_name(dev), 'arch': getattr(prop, 'gcnArchName', ''),
           'torch': torch.__version__, 'hip': torch.version.hip, 'volume': [B.NX, B.NY, B.NZ], 'output': [H, W], 'views': VIEWS,
           'label_sets': len(SETS), 'cap': CAP, 'cost_of_the_candidates': [float(c) for c in cost],
           'boundary_pixels_views': int(counts[..., 0].sum()), 'boundary_pixels_segmentation': int(counts[0, :, 1].sum()),
           'bytes_read_by_dfl_sim_outline': 2 * VIEWS * len(SETS) * H * W * 4,
           'render': events(lambda: nat.call('dfl_drr_render', ra, stream), a.reps, a.warmup),
           'edt': events(edt, a.reps, a.warmup), 'outline': events(outline, a.reps, a.warmup),
           'generation': events(generation, a.reps, a.warmup),
           'surface_distances': events(lambda: labels.surface_distances(maps, repeated), a.reps, a.warmup)}
    reg.register(vol, geom, None, theta0=THETA0, popsize=VIEWS, generations=2, similarity='outline', segmentation=seg, outline_cap=CAP)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reg.register(vol, geom, None, theta0=THETA0, popsize=VIEWS, generations=a.generations, similarity='outline', segmentation=seg, outline_cap=CAP)
    res['register_generation_wall_ms'] = (time.perf_counter() - t0) * 1e3 / (a.generations + 1.0 / VIEWS)
    del keep
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f_:
            json.dump(res, f_, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
