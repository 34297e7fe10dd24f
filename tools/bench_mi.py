"""Times of the mutual-information cost (dfl_sim_mi, dfl_sim_mi_bwd) next to the gradient-NCC bank entry
points on one GPU, in one process.

tools/bench_drr.py's phantom (384 x 320 x 400 voxels of 0.8 mm, three label blobs) on the training grid, crop 50 and factor 8
(180 x 180): 16 problems (the phantom under 16 poses, each problem's fixed image its own exact DRR) with lambda = 32 candidates
each, drawn around a start 2 units away in every parameter: V = 512 views against a bank of F = 16 images, bins 32 x 32, the
moving range of every image (0, 1.25 x the largest value of its first candidate).

  render        dfl_drr_render, trilinear, step 1 mm, tight boxes, the 512 views
  mi            dfl_sim_mi on those views (clear, histogram, finish), next to dfl_sim_bank_gradncc
  mi_bwd        dfl_sim_mi_bwd (the same and the adjoint kernel), next to dfl_sim_bank_gradncc_bwd
  generation    one generation of register_many for the 16 problems with each cost, by the wall clock: the difference between a
                run of --generations and one of 2 generations, per generation (it cancels the set-up and the range render)

Device events around back-to-back calls of the C entry points (argument blocks built once) after a warm-up; the two costs are
timed in alternating windows of at least --window seconds, --reps of them each; median, min and max.  Prints one JSON object
and writes it to --out.

    python tools/bench_mi.py [--window 0.3] [--reps 5] [--generations 6] [--out profiles/mi_bench.json]
"""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import bench_drr as B  # noqa: E402

FACTOR, LAMBDA, MANY, BINS, STEP_MM = 8, 32, 16, 32, 1.0
THETA0 = (2.0, -2.0, 2.0, 2.0, -2.0, 2.0)


def alternating(fns, window, reps):
    """{name: median / min / max ms per call} of the functions `fns`, timed in turn, `reps` windows each."""
    iters = {}
    for name, fn in fns.items():
        B.timed(fn, 2)                                              # warm-up
        iters[name] = max(int(1e3 * window / max(B.timed(fn, 1), 1e-3)) + 1, 1)
    ms = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            ms[name].append(B.timed(fn, iters[name]))
    return {name: {'ms': round(statistics.median(v), 4), 'min_ms': round(min(v), 4), 'max_ms': round(max(v), 4), 'calls_per_window': iters[name]}
            for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=0.3, help='seconds of device work per timed window, at least')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--generations', type=int, default=6, help='generations of the longer wall-clock run of register_many')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mi_bench.json'))
    args = ap.parse_args()
    import torch
    from dfl_amd import _native as nat, drr, register as reg
    if not torch.cuda.is_available():
        raise SystemExit('bench_mi.py needs a GPU: a time taken anywhere else says nothing')
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
    geoms, fixed = [], []
    for c2is in B.poses(MANY):
        objects = [drr.Obj(A, m) for A, m in zip(c2is, drr.DEFAULT_MASKS)]
        geoms.append(drr.Geometry(K, np.eye(4), {k: I2P @ A for k, A in zip(drr.POSES, c2is)}, I2P, G, objects, grid))   # P = I2P C2I E
        fixed.append(drr.render(vol, objects, grid, want_labels=False)[0])
    fixed = torch.stack(fixed).contiguous()
    stream = torch.cuda.current_stream(dev).cuda_stream
    prop = torch.cuda.get_device_properties(dev)
    ctr = reg.volume_centre(vol.shape, I2P)
    thetas = np.asarray(THETA0)[None] + 2.0 * np.random.default_rng(0).standard_normal((LAMBDA, 6))
    A = np.linalg.inv(I2P)[None] @ reg.pose_deltas(thetas, ctr) @ I2P[None]
    views = [[drr.Obj(A[v] @ ob.c2i, ob.mask) for ob in g.objects] for g in geoms for v in range(LAMBDA)]
    V = len(views)
    ra, (att, _, _), keep = drr.render_args(vol, views, grid, interp='trilinear', step_mm=STEP_MM, want_labels=False)
    nat.call('dfl_drr_render', ra, stream)
    fixed_of = np.repeat(np.arange(MANY, dtype=np.int32), LAMBDA)
    ncc = reg.SimilarityBank(fixed, None, V)
    mi = reg.MISimilarity(fixed, None, V, BINS)
    top = att.reshape(MANY, LAMBDA, -1)[:, 0].amax(1)
    mi.set_range(torch.stack([torch.zeros_like(top), top * 1.25], 1))
    ncc_cost, mi_cost = ncc.cost(att, fixed_of).cpu().numpy(), mi.cost(att, fixed_of).cpu().numpy()
    assert np.isfinite(ncc_cost).all() and np.isfinite(mi_cost).all() and (mi_cost < 0).all(), (ncc_cost, mi_cost)
    assert int(mi.hist.sum().item()) == V * H * W * nat.SIM_MI_UNIT
    c0, g0 = ncc.cost_and_adjoint(att, fixed_of)
    c1, g1 = mi.cost_and_adjoint(att, fixed_of)
    assert torch.equal(c1.cpu(), torch.from_numpy(mi_cost)) and torch.isfinite(g1).all()
    fo = ncc.fixed_of(fixed_of, V)
    na = ncc._args('dfl_sim_bank_gradncc', att, fo, ncc.scratch, ncc.out)
    nb = ncc._args('dfl_sim_bank_gradncc_bwd', att, fo, ncc.bwd_scratch, c0, g0)
    ma = mi._args('dfl_sim_mi', att, fo, mi.out)
    mb = mi._args('dfl_sim_mi_bwd', att, fo, c1, mi.ell, g1)
    res = {'tool': 'tools/bench_mi.py --window %g --reps %d --generations %d (device events around back-to-back calls, alternating windows; '
                   'wall clock around register_many for a generation; median of the repetitions)' % (args.window, args.reps, args.generations),
           'date': datetime.date.today().isoformat(), 'device': torch.cuda.get_device_name(dev), 'arch': getattr(prop, 'gcnArchName', ''),
           'compute_units': prop.multi_processor_count, 'torch': torch.__version__, 'hip': torch.version.hip, 'volume': [B.NX, B.NY, B.NZ],
           'output': [H, W], 'views': V, 'fixed_images': MANY, 'lambda': LAMBDA, 'bins': [BINS, BINS], 'run_pixels': nat.SIM_MI_RUN,
           'workgroups_of_the_histogram_kernel': V * -(-H * W // nat.SIM_MI_RUN), 'bytes_read_by_the_histogram_kernel': V * H * W * 5,
           'non_zero_bins_per_view_median': int(np.median((mi.hist != 0).sum((1, 2)).cpu().numpy())),
           'mi_cost_range': [float(mi_cost.min()), float(mi_cost.max())]}
    res['render'] = alternating({'render': lambda: nat.call('dfl_drr_render', ra, stream)}, args.window, args.reps)['render']
    res['forward'] = alternating({'dfl_sim_bank_gradncc': lambda: nat.call('dfl_sim_bank_gradncc', na, stream),
                                  'dfl_sim_mi': lambda: nat.call('dfl_sim_mi', ma, stream)}, args.window, args.reps)
    res['adjoint'] = alternating({'dfl_sim_bank_gradncc_bwd': lambda: nat.call('dfl_sim_bank_gradncc_bwd', nb, stream),
                                  'dfl_sim_mi_bwd': lambda: nat.call('dfl_sim_mi_bwd', mb, stream)}, args.window, args.reps)
    res['mi_launch_longer_than_the_render'] = bool(res['forward']['dfl_sim_mi']['ms'] > res['render']['ms'])
    del keep

    def run(generations, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reg.register_many(vol, geoms, fixed, theta0=np.tile(np.asarray(THETA0), (MANY, 1)), popsize=LAMBDA, generations=generations,
                          step_mm=STEP_MM, **kw)
        return (time.perf_counter() - t0) * 1e3

    costs = {'global': dict(similarity='global'), 'mi': dict(similarity='mi', mi_bins=BINS)}
    wall = {name: [] for name in costs}
    for name, kw in costs.items():
        run(2, **kw)                                                # warm-up
    for _ in range(args.reps):
        for name, kw in costs.items():
            wall[name].append((run(args.generations, **kw) - run(2, **kw)) / (args.generations - 2))
    res['register_many_generation_wall_ms'] = {name: {'ms': round(statistics.median(v), 3), 'min_ms': round(min(v), 3), 'max_ms': round(max(v), 3)}
                                               for name, v in wall.items()}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f_:
        json.dump(res, f_, indent=1, sort_keys=True)
        f_.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
