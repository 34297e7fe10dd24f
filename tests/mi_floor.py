"""What the model of the mutual-information cost does on its own (offline, on the CPU, never the kernel); the result is
committed as tests/golden/floors/mi.json.

(a) The adjoint against central differences: for reg_ref.sim_images at 45 x 61 and 17 x 70, bins 32 x 32, view 5 and a
    random direction restricted to the pixels strictly inside the range, |<adjoint, d> - (c(m + e d) - c(m - e d)) / 2e| /
    |central difference| at e = 1e-6, with the unquantised adjoint (mi_ref.adjoint(unit=None)) and mi_ref.cost64.
    tests/test_mi_cpu.py allows 4 x the recorded value.
(b) Quantisation, informational: the largest |quantised - unquantised| of the cost and of the adjoint per size and mask.
(c) The registration case of tests/test_gpu_mi.py (the tilted scene from reg_ref.THETA_START) run with the product's own
    cma_es and pose_delta but the numpy renderer and this model, for the bin counts 16, 8, 32 in that order: the first
    whose run ends within 1 px at the bone centres is the one the GPU test uses, with max(reg_floor.PIXEL_BAR, 2 x that
    end) as its bar.  A minute or two per bin count; they run side by side.

    python tests/mi_floor.py            # rewrites tests/golden/floors/mi.json
"""
import json
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import drr_ref as D  # noqa: E402
import mi_ref as M  # noqa: E402
import reg_floor as FL  # noqa: E402
import reg_ref as R  # noqa: E402

PATH = os.path.join(HERE, 'golden', 'floors', 'mi.json')
FD_SIZES, FD_BINS, FD_VIEW, FD_EPS, FD_SEED, FD_FACTOR = ((45, 61), (17, 70)), 32, 5, 1e-6, 0, 4.0
BINS_TO_TRY, MODEL_BAR = (16, 8, 32), 1.0
POPSIZE, SEED, STEP_MM, GENERATIONS, SIGMA0 = 16, 0, 1.0, 80, 2.0


def sim_range(moving):
    """The range of the similarity tests: (0, 1.25 x the largest value of the six views)."""
    return M.F32(0), M.F32(M.F32(1.25) * np.asarray(moving, M.F32).max())


def fd_case(H, W, row_term=1.0):
    """(relative distance, central difference, <adjoint, d>, pixels inside) of case (a) at H x W."""
    fixed, moving = R.sim_images(H, W)
    fbin, _ = M.prepare(fixed, None, FD_BINS)
    lo, hi = sim_range(moving)
    m = moving[FD_VIEW]
    inside = (m > lo) & (m < hi)
    d = np.random.default_rng(FD_SEED).standard_normal((H, W)) * inside
    g = M.adjoint(m, fbin, lo, hi, FD_BINS, FD_BINS, None, row_term)
    m64 = m.astype(np.float64)
    fd = (M.cost64(m64 + FD_EPS * d, fbin, lo, hi, FD_BINS, FD_BINS) - M.cost64(m64 - FD_EPS * d, fbin, lo, hi, FD_BINS, FD_BINS)) / (2 * FD_EPS)
    dot = float((g * d).sum())
    return abs(dot - fd) / abs(fd), fd, dot, int(inside.sum())


def fd_floors():
    out = {}
    for H, W in FD_SIZES:
        rel, fd, dot, inside = fd_case(H, W)
        out['%dx%d' % (H, W)] = {'relative': rel, 'central_difference': fd, 'adjoint_dot_direction': dot, 'inside': inside}
    return out


def quantisation():
    out = {}
    for H, W in R.SIM_SIZES:
        fixed, moving = R.sim_images(H, W)
        lo, hi = sim_range(moving)
        for name, mask in R.sim_masks(H, W).items():
            fbin, info = M.prepare(fixed, mask, FD_BINS)
            cq, cu = M.cost(moving, fbin, (lo, hi), FD_BINS, FD_BINS), M.cost(moving, fbin, (lo, hi), FD_BINS, FD_BINS, None)
            ga = max(float(np.abs(M.adjoint(v, fbin, lo, hi, FD_BINS, FD_BINS) - M.adjoint(v, fbin, lo, hi, FD_BINS, FD_BINS, None)).max())
                     for v in moving)
            out['%dx%d/%s' % (H, W, name)] = {'cost': [float(c) for c in cq], 'cost_difference': float(np.abs(cq - cu).max()),
                                              'adjoint_difference': ga, 'counted': int(info[0])}
    return out


def case_offset(bins):
    """The tilted scene from THETA_START with `bins` x `bins`, by the models alone."""
    from dfl_amd import register as reg
    S = D.scene('tilted')
    fixed = FL.fixed_image(S).astype(np.float32)
    fbin, _ = M.prepare(fixed, None, bins)
    ctr = R.volume_centre(S)

    def views(thetas):
        for Dm in reg.pose_deltas(thetas, ctr):
            yield R.render_poses(S, [Dm @ P for P in S['poses']], 'trilinear', STEP_MM).astype(np.float32)

    theta0 = np.array(R.THETA_START)
    lo, hi = M.start_range(next(views(theta0[None])))

    def fn(thetas):
        return np.array([M.cost(v, fbin, (lo, hi), bins, bins) for v in views(thetas)])

    res = reg.cma_es(fn, theta0, SIGMA0, POPSIZE, GENERATIONS, SEED)
    P_start = reg.pose_delta(theta0, ctr) @ S['poses'][0]
    P_end = reg.pose_delta(res.mean, ctr) @ S['poses'][0]
    return bins, {'bins': bins, 'theta0': list(R.THETA_START), 'theta': [float(t) for t in res.mean], 'range': [float(lo), float(hi)],
                  'generations': GENERATIONS, 'sigma0': SIGMA0, 'popsize': POPSIZE, 'seed': SEED,
                  'cost_first_generation': float(res.trace[0]), 'cost_last_generation': float(res.trace[-1]),
                  'cost_at_truth': float(fn(np.zeros((1, 6)))[0]), 'final_cost': float(fn(res.mean[None])[0]),
                  'start_px': [float(d) for d in R.centre_distances(S, S['poses'][0], P_start)],
                  'final_px': [float(d) for d in R.centre_distances(S, S['poses'][0], P_end)]}


def load():
    with open(PATH) as f:
        return json.load(f)


def fd_bar(H, W):
    """FD_FACTOR x the committed relative distance of case (a) at that size."""
    return FD_FACTOR * load()['finite_differences']['%dx%d' % (H, W)]['relative']


def registration():
    """(bins, bar in pixels) of the GPU recovery test, or None when no bin count got the model within MODEL_BAR."""
    doc = load()['registration']
    if doc['chosen'] is None:
        return None
    end = max(doc['tried'][str(doc['chosen'])]['final_px'])
    return int(doc['chosen']), max(FL.PIXEL_BAR, 2.0 * end)


if __name__ == '__main__':
    doc = {'what': '(finite_differences) the relative distance between <unquantised adjoint, d> and central differences of the unquantised '
                   'float64 cost, d restricted to pixels strictly inside the range; (quantisation) largest |quantised - unquantised| of cost '
                   'and adjoint over the six test images per size and mask, bins 32; (registration) the tilted scene from reg_ref.THETA_START '
                   'run with dfl_amd.register.cma_es and pose_delta on the numpy renderer and tests/mi_ref.py per bin count tried: distances '
                   'in pixels between ellipsoid centres projected under the true and the found pose',
           'tool': 'python tests/mi_floor.py', 'numpy': np.__version__, 'fd_factor': FD_FACTOR, 'fd_eps': FD_EPS, 'model_bar_pixels': MODEL_BAR,
           'finite_differences': fd_floors(), 'quantisation': quantisation()}
    with multiprocessing.Pool(len(BINS_TO_TRY)) as pool:
        tried = dict(pool.map(case_offset, BINS_TO_TRY))
    chosen = next((b for b in BINS_TO_TRY if max(tried[b]['final_px']) <= MODEL_BAR), None)
    doc['registration'] = {'order': list(BINS_TO_TRY), 'chosen': chosen, 'tried': {str(b): tried[b] for b in BINS_TO_TRY}}
    os.makedirs(os.path.dirname(PATH), exist_ok=True)
    with open(PATH, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(doc, indent=1, sort_keys=True))
