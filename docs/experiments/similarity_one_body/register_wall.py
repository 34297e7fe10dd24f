#!/usr/bin/env python3
"""The wall time of one register(generations=20, refine=3) on the scene of tools/bench_register.py: 10 calls after 2 warm-ups.
register() now goes through lockstep; this is what the host pays for that.

    python docs/experiments/similarity_one_body/register_wall.py OUT.json [--tree CHECKOUT]      (default: this tree)
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
tree = os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 and sys.argv[2] == '--tree' else ROOT
sys.path[:0] = [tree, os.path.join(tree, 'tools')]
import torch  # noqa: E402
import bench_drr as B  # noqa: E402
import bench_register as BR  # noqa: E402
from dfl_amd import drr, register as reg  # noqa: E402

assert os.path.realpath(reg.__file__).startswith(os.path.realpath(tree)), reg.__file__
dev = torch.device('cuda', 0)
vol = drr.Volume(*B.phantom(dev))
f = 1000.0 / B.PIXEL_MM
K = np.array([[-f, 0, 767.5], [0, -f, 767.5], [0, 0, 1]])
G, (H, W) = drr.training_grid(B.DET, B.DET, B.CROP, BR.FACTOR)
grid = drr.Grid(-np.linalg.inv(K) @ G, H, W)
I2P = np.eye(4)
I2P[:3, :3] *= B.SPACING
I2P[:3, 3] = [-150.0, -120.0, -160.0]
c2is = B.poses(1)[0]
objects = [drr.Obj(A, m) for A, m in zip(c2is, drr.DEFAULT_MASKS)]
geom = drr.Geometry(K, np.eye(4), {k: I2P @ A for k, A in zip(drr.POSES, c2is)}, I2P, G, objects, grid)
fixed = drr.render(vol, objects, grid, want_labels=False)[0]
ms = []
for call in range(12):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = reg.register(vol, geom, fixed, theta0=BR.THETA0, popsize=BR.LAMBDA, generations=20, step_mm=BR.STEP_MM, refine=3, seed=0)
    ms.append(1e3 * (time.perf_counter() - t0))
out = {'what': 'register(generations=20, refine=3, popsize=%d), wall ms per call, 10 calls after 2 warm-ups' % BR.LAMBDA, 'tree': tree,
       'renders': int(res.renders), 'ms': round(statistics.median(ms[2:]), 4), 'min_ms': round(min(ms[2:]), 4), 'max_ms': round(max(ms[2:]), 4)}
json.dump(out, open(sys.argv[1], 'w'), indent=1)
print(json.dumps(out))
