"""Times dfl_amd.mesh on a synthetic 512^3 label volume with four ellipsoidal blobs (labels 1, 2, 5, 6: the labels of
examples/full_res_3d_viz.py), the example's whole GPU half (everything but the file read), and the numpy model
(tests/mesh_ref.py) beside it on a smaller volume.  Prints one JSON object; --out also writes it.

Run under `rocprofv3 --kernel-trace --stats` (a run of its own) for per-kernel times; the JSON carries the bytes each
pass must move so that kernel times can be turned into rates:
  mc_volume_bytes      the compulsory read of the volume by one marching-cubes pass (count and emit each read it once)
  smooth_gather_bytes  per smoothing launch: the CSR row pointers and neighbour ids, one 16-byte position per neighbour
                       entry, the vertex's own T_{n-2} and accumulator (read and written), fixed flag

    python tools/bench_mesh.py [--size 512] [--reps 3] [--model-size 128] [--out mesh_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, 'examples'))
import dfl_amd  # noqa: E402,F401
from dfl_amd import mesh  # noqa: E402

LABELS = [1, 2, 5, 6]


def blobs(n, seed=0):
    """uint8 [n, n, n]: four overlapping-free ellipsoids with a little surface noise."""
    rng = np.random.default_rng(seed)
    vol = np.zeros((n, n, n), np.uint8)
    ax = (np.arange(n, dtype=np.float32) + 0.5) / n
    specs = [(1, (0.3, 0.3, 0.35), (0.2, 0.17, 0.22)), (2, (0.7, 0.3, 0.35), (0.19, 0.18, 0.21)),
             (5, (0.3, 0.72, 0.65), (0.12, 0.2, 0.25)), (6, (0.7, 0.72, 0.65), (0.13, 0.19, 0.26))]
    noise = rng.normal(scale=0.02, size=(n, n)).astype(np.float32)
    for lab, (cx, cy, cz), (rx, ry, rz) in specs:
        for z in range(n):
            dz = ((ax[z] - cz) / rz) ** 2
            if dz > 1:
                continue
            d = ((ax[None, :] - cx) / rx) ** 2 + ((ax[:, None] - cy) / ry) ** 2 + dz + noise
            vol[z][d <= 1] = lab
    return vol


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def events(fn, reps):
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
    return float(np.median(ts))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--model-size', type=int, default=128)
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_mesh needs a GPU')
    import full_res_3d_viz as V
    import mesh_ref as R
    dev = torch.device('cuda:0')
    n = a.size
    vol_h = blobs(n)
    vol = torch.from_numpy(vol_h).to(dev)
    res = {'size': [n, n, n], 'labels': LABELS, 'reps': a.reps, 'device': torch.cuda.get_device_name(0)}
    surfaces = mesh.label_surfaces(vol, LABELS)
    res['vertices'] = [int(v.shape[0]) for v, _ in surfaces]
    res['triangles'] = [int(t.shape[0]) for _, t in surfaces]
    res['label_surfaces_ms'] = timed(lambda: mesh.label_surfaces(vol, LABELS), a.reps)
    res['mc_volume_bytes'] = int(vol.numel())
    v, t = max(surfaces, key=lambda s: s[0].shape[0])
    rp, col, fixed = mesh.neighbours(t, v.shape[0])
    nnz = int(col.numel())
    res['smooth_mesh'] = {'vertices': int(v.shape[0]), 'triangles': int(t.shape[0]), 'neighbour_entries': nnz}
    res['smooth_gather_bytes'] = int(4 * (v.shape[0] + 1) + 4 * nnz + 16 * nnz + v.shape[0] * (16 + 32 + 1))
    res['smooth_ms'] = events(lambda: mesh.smooth(v, t), a.reps)
    res['normals_ms'] = events(lambda: mesh.vertex_normals(v, t), a.reps)
    g = {'volume': vol_h, 'surface_xforms': [np.eye(4)] * 4}
    res['example_gpu_half_ms'] = timed(lambda: V.surfaces_on_gpu(g, dev, log=lambda s: None), a.reps)
    m = a.model_size
    small = blobs(m)
    t0 = time.perf_counter()
    got = mesh.label_surfaces(torch.from_numpy(small).to(dev), LABELS)
    torch.cuda.synchronize()
    t_gpu_small = time.perf_counter() - t0
    t0 = time.perf_counter()
    model = [R.marching_cubes(small, lab) for lab in LABELS]
    t_mc = time.perf_counter() - t0
    k = int(np.argmax([len(p) for p, _, _ in model]))
    xn, _ = R.normalize(model[k][0])
    t0 = time.perf_counter()
    R.smooth(xn, model[k][1])
    t_sm = time.perf_counter() - t0
    same = all(np.array_equal(gt.cpu().numpy(), mt) for (_, gt), (_, mt, _) in zip(got, model))
    res['numpy_model'] = {'size': [m, m, m], 'mc_all_labels_s': t_mc, 'smooth_largest_s': t_sm,
                          'smooth_vertices': int(len(xn)), 'gpu_label_surfaces_first_call_s': t_gpu_small,
                          'gpu_matches_model': bool(same)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
