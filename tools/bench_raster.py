"""Times dfl_amd.raster on tools/bench_mesh.py's synthetic 512^3 scene: the four smoothed blob surfaces with normals, a
1536 x 1536 textured quad behind them (two triangles that cover most of the screen), a ring of instanced spheres and a
few ribbons, drawn at 1920 x 1080 with ssaa 1 and 2.  Prints one JSON object; --out also writes it.

Per ssaa: the milliseconds of one render() between events, the counters, and the bytes each kernel must move at least:
  tris_bytes     the triangle kernel: 12 bytes of indices and three gathered 12-byte positions per triangle
  vis_bytes      the visibility buffer, 8 bytes per sample, written once by the clear and read once by the shade (16)
  shade_bytes    shade: the visibility buffer read, 4 bytes of colour written per sample
  resolve_bytes  resolve: 4 bytes read per sample, 3 written per pixel
Per-kernel times come from runs of their own under `rocprofv3 --kernel-trace --stats` (one ssaa per run, so that the
kernels of the two sizes do not share a row); --kernel-stats SSAA=FILE.csv (repeatable) adds such a run's rs_* rows to the
JSON, each with the rate its compulsory bytes give; --from-json takes the timings of an earlier run instead of
measuring (the merge needs no GPU).

    python tools/bench_raster.py [--size 512] [--reps 5] [--ssaa 1,2] [--out raster_bench.json]
    rocprofv3 --kernel-trace --stats -d rp1 -o s --output-format csv -- python tools/bench_raster.py --ssaa 1
    python tools/bench_raster.py --from-json raster_bench.json --kernel-stats 1=rp1/.../s_kernel_stats.csv --out raster_bench.json
"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'examples'))
import dfl_amd  # noqa: E402,F401
from dfl_amd import mesh, raster  # noqa: E402

W, H, FOV = 1920, 1080, 30.0
COLORS = [(0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 1.0), (1.0, 0.5, 0.0)]


def build_scene(n, dev):
    import bench_mesh as BM
    import full_res_3d_viz as V
    vol = torch.from_numpy(BM.blobs(n)).to(dev)
    meshes, pts = [], []
    for (v, t), rgb in zip(mesh.label_surfaces(vol, BM.LABELS), COLORS):
        xs, undo = mesh.smooth(v, t)
        pos = mesh.transform(xs, undo)
        meshes.append(raster.Mesh(pos, t, normals=mesh.vertex_normals(pos, t), rgb=rgb))
        lo, hi = torch.aminmax(pos, dim=0)
        pts.append(torch.stack([lo, hi]).double().cpu().numpy())
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)           # noqa: E731
    quad = np.array([[-0.2 * n, -0.2 * n, -0.3 * n], [-0.2 * n, 1.2 * n, -0.3 * n], [1.2 * n, 1.2 * n, -0.3 * n], [1.2 * n, -0.2 * n, -0.3 * n]])
    tex = torch.from_numpy(((np.add.outer(np.arange(1536), np.arange(1536)) * 7) % 256).astype(np.uint8)).to(dev)
    meshes.append(raster.Mesh(f32(quad), torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32, device=dev),
                              normals=f32(np.tile([[0, 0, 1.0]], (4, 1))), uv=f32([[0, 0], [0, 1], [1, 1], [1, 0]]), texture=tex))
    sp, st = V.unit_sphere()
    sp, st = f32(sp), torch.from_numpy(st.astype(np.int32)).to(dev)
    for k in range(16):
        M = np.diag([0.02 * n, 0.02 * n, 0.02 * n, 1.0])
        M[:3, 3] = (0.5 * n + 0.45 * n * np.cos(k * np.pi / 8), 0.5 * n + 0.45 * n * np.sin(k * np.pi / 8), 0.9 * n)
        meshes.append(raster.Mesh(sp, st, normals=sp, rgb=(0.5, 0.0, 0.5), matrix=M))
    pts = np.concatenate(pts + [quad])
    eye, target = raster.frame(pts, (0.25, 0.35, -1.0), FOV, W / H, margin=0.8)
    for k in range(4):
        p, q = raster.ribbon((0.5 * n, 0.5 * n, 1.2 * n), quad[k], 0.004 * n, eye)
        meshes.append(raster.Mesh(f32(p), torch.from_numpy(q).to(dev), rgb=(0.0, 1.0, 0.0), unlit=True))
    view = raster.look_at(eye, target, (0, 1, 0))
    d = float(np.linalg.norm(eye - target))
    return meshes, (view, raster.perspective(FOV, W / H, d / 20, d * 4)), d / 20


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
    return float(np.median(ts)), float(np.min(ts))


def kernel_rows(path):
    """{kernel: {calls, average_us, min_us}} of the rs_* rows of a rocprofv3 kernel_stats.csv."""
    out = {}
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            name = row.get('Name', '')
            if 'rs_' in name and '_kernel' in name:
                short = name[name.index('rs_'):].split('(')[0].split('ENS')[0]
                out[short] = {'calls': int(row['Calls']), 'average_us': float(row['AverageNs']) / 1e3, 'min_us': float(row['MinNs']) / 1e3}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--ssaa', default='1,2')
    ap.add_argument('--kernel-stats', action='append', default=[], metavar='SSAA=FILE')
    ap.add_argument('--from-json')
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    if a.from_json:
        with open(a.from_json) as f:
            res = json.load(f)
        return finish(res, a)
    if not torch.cuda.is_available():
        raise SystemExit('bench_raster needs a GPU')
    dev = torch.device('cuda:0')
    meshes, view_proj, near = build_scene(a.size, dev)
    T = sum(int(m.tris.shape[0]) for m in meshes)
    res = {'size': a.size, 'image': [W, H], 'records': len(meshes), 'triangles': T, 'reps': a.reps,
           'device': torch.cuda.get_device_name(0), 'runs': {}}
    for s in [int(t) for t in a.ssaa.split(',')]:
        out = raster.draw(meshes, view_proj, W, H, ssaa=s, near=near, want=('rgb', 'ids', 'counts'))
        S = W * s * H * s
        covered = int((out['ids'] >= 0).sum())
        med, best = events(lambda: raster.render(meshes, view_proj, W, H, ssaa=s, near=near), a.reps)
        res['runs'][str(s)] = {'render_ms_median': med, 'render_ms_min': best, 'counts': out['counts'].cpu().tolist(),
                               'covered_samples': covered, 'samples': S, 'tris_bytes': 48 * T, 'vis_bytes': 16 * S,
                               'shade_bytes': 12 * S, 'resolve_bytes': 4 * S + 3 * W * H,
                               'checksum': int(out['rgb'].to(torch.int64).sum())}
    return finish(res, a)


BYTES_OF = {'rs_clear_kernel': 'vis_bytes', 'rs_tris_kernel': 'tris_bytes', 'rs_shade_kernel': 'shade_bytes',
            'rs_resolve_kernel': 'resolve_bytes'}       # (rs_large_kernel: atomics on covered samples only, no compulsory stream)


def finish(res, a):
    for item in a.kernel_stats:
        s, path = item.split('=', 1)
        rows = kernel_rows(path)
        for name, r in rows.items():
            if name in BYTES_OF:
                r['compulsory_bytes'] = res['runs'][s][BYTES_OF[name]] // (2 if name == 'rs_clear_kernel' else 1)
                r['compulsory_gb_per_s'] = r['compulsory_bytes'] / (r['average_us'] * 1e3)
        res['runs'][s]['kernels'] = rows
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
