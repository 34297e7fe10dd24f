"""What the models alone do on the gradient tests (offline, on the CPU, never the kernel); the result is committed as
tests/golden/floors/pose_grad.json.

(a) Adjoint floors: for reg_ref.sim_images, every size and mask, the largest |float32 model - float64 model| of d_moving
    and |sum over the pixels| of the float32 model, per view, both as fractions of the largest |adjoint| of that view
    (the fixed image against itself has an adjoint of rounding size, so the views do not share a floor).
(b) Moment floors: for the cases of tests/test_gpu_pose_grad.py (scene, view, step, adjoint pattern) the largest
    |float32 model - float64 model| of the twelve numbers of every object, as a fraction of the largest entry.
(c) The same for the gradient with respect to the six pose parameters at 0.2 THETA_START.
(d) The refinement cases, run with the product's own bfgs, cma_es and pose_deltas on the numpy models alone.
The GPU bars are BAR_FACTOR x these floors (the factor of tests/reg_floor.py).

    python tests/grad_floor.py            # rewrites tests/golden/floors/pose_grad.json
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
import grad_ref as G  # noqa: E402
import reg_floor as FL  # noqa: E402
import reg_ref as R  # noqa: E402

PATH = os.path.join(HERE, 'golden', 'floors', 'pose_grad.json')
BAR_FACTOR = FL.BAR_FACTOR
MOMENT_CASES = [(kind, view, step, pattern) for kind in ('tilted', 'aligned') for view in (0, 1) for step in (0.5, 1.0)
                for pattern in ('adjoint', 'sines')]
THETA_FRACTION = 0.2                       # (c): the gradient is taken at THETA_FRACTION * THETA_START
REFINE, REFINE_TOL, REFINE_START = 30, 1e-4, 0.3
CMA_GENERATIONS = 25


# ---- (a) ---------------------------------------------------------------------------------------------------------------
def adjoint_floors():
    out = {}
    for H, W in R.SIM_SIZES:
        fixed, moving = R.sim_images(H, W)
        for name, mask in R.sim_masks(H, W).items():
            _, d64 = G.sim_adjoint(moving, fixed, mask)
            _, d32 = G.sim_adjoint(moving, fixed, mask, dtype=np.float32)
            scale = np.abs(d64).max((1, 2))
            live = scale > 0
            err = np.abs(d32 - d64).max((1, 2))
            tot = np.abs(d32.astype(np.float64).sum((1, 2)))
            safe = np.where(live, scale, 1.0)
            out['%dx%d/%s' % (H, W, name)] = {'floor': [float(e) for e in np.where(live, err / safe, 0.0)],
                                              'sum_floor': [float(e) for e in np.where(live, tot / safe, 0.0)],
                                              'scale': [float(s) for s in scale]}
    return out


# ---- (b) ---------------------------------------------------------------------------------------------------------------
def scene_fixed(kind):
    return D.model(kind, 'exact', 0)[0]


def moment_inputs(kind, view, step, pattern):
    """(recs, d_att float32 [H, W] with the near-integer rays zeroed, the fraction of rays zeroed, pivots): what the
    model and the kernel both get."""
    S = D.scene(kind)
    H, W = S['rows'], S['cols']
    recs = D.pack(D.scene_views(S)[view], D.MASKS, S['Q'], S['lab'], True, 'trilinear')
    att, _, frac = D.render(S['mu'], S['lab'], recs, S['Q'].astype(np.float32), H, W, 'trilinear', step_mm=step)
    if pattern == 'adjoint':
        d_att = G.sim_adjoint(att, scene_fixed(kind))[1]
        d_att = d_att / np.abs(d_att).max()
    else:
        rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        d_att = np.sin(0.31 * rr + 0.7) * np.sin(0.23 * cc + 1.1)            # smooth, not zero on the border
    near = D.near_integer(frac)
    d_att = np.where(near, 0.0, d_att).astype(np.float32)
    return recs, d_att, float(near.mean()), G.box_pivots(recs)


def moment_key(kind, view, step, pattern):
    return '%s/view%d/step%.1f/%s' % (kind, view, step, pattern)


def moment_case(case):
    kind, view, step, pattern = case
    S = D.scene(kind)
    recs, d_att, zeroed, piv = moment_inputs(*case)
    q = S['Q'].astype(np.float32)
    m64 = G.pose_moments(S['mu'], S['lab'], recs, q, S['rows'], S['cols'], d_att, piv, step)
    m32 = G.pose_moments(S['mu'], S['lab'], recs, q, S['rows'], S['cols'], d_att, piv, step, dtype=np.float32)
    return moment_key(*case), {'floor': float(np.abs(m32 - m64).max() / np.abs(m64).max()), 'scale': float(np.abs(m64).max()),
                               'zeroed_rays': zeroed, 'moments': m64.tolist()}


# ---- (c) ---------------------------------------------------------------------------------------------------------------
def theta_case(_=None):
    from dfl_amd import register as reg
    S = D.scene('tilted')
    th = THETA_FRACTION * np.array(R.THETA_START)
    out = {}
    for name, dt in (('float64', np.float64), ('float32', np.float32)):
        out[name] = G.model_cost_and_grad(S, S['poses'], (0, 1, 2), FL.fixed_image(S), reg.pose_deltas, FL.STEP_MM, dt)(th)
    g64, g32 = out['float64'][1], out['float32'][1]
    return 'theta', {'theta': th.tolist(), 'cost': out['float64'][0], 'gradient': g64.tolist(),
                     'floor': float(np.abs(g32 - g64).max() / np.abs(g64).max())}


# ---- (d) ---------------------------------------------------------------------------------------------------------------
def _refined(S, theta0, generations):
    from dfl_amd import register as reg
    fixed = FL.fixed_image(S)
    mean, rec = np.asarray(theta0, np.float64), {}
    if generations:
        res = reg.cma_es(R.model_cost_fn(S, S['poses'], (0, 1, 2), fixed, reg.pose_deltas, FL.STEP_MM), mean, 2.0, FL.POPSIZE, generations,
                         FL.SEED)
        mean = res.mean
    fin = reg.bfgs(G.model_cost_and_grad(S, S['poses'], (0, 1, 2), fixed, reg.pose_deltas, FL.STEP_MM), mean, REFINE, REFINE_TOL)
    ctr = R.volume_centre(S)
    px = lambda th: [float(d) for d in R.centre_distances(S, S['poses'][0], reg.pose_delta(th, ctr) @ S['poses'][0])]  # noqa: E731
    final = [reg.pose_delta(fin.x, ctr) @ P for P in S['poses']]
    rec.update(theta0=[float(t) for t in theta0], generations=generations, theta_cma=[float(t) for t in mean], theta=[float(t) for t in fin.x],
               start_px=px(mean), final_px=px(fin.x), refine_cost=[float(c) for c in fin.trace], gradient_evaluations=fin.evaluations,
               iterations=fin.iterations,
               final_cost_step_0_5=float(R.cost(R.render_poses(S, final, 'trilinear', 0.5), fixed)))
    return rec


def case_refine_only(_=None):
    """REFINE_START x THETA_START, halved until the models alone end within half of reg_floor.PIXEL_BAR."""
    S = D.scene('tilted')
    theta, tried = REFINE_START * np.array(R.THETA_START), []
    for halvings in range(4):
        rec = _refined(S, theta, 0)
        rec['halvings'] = halvings
        tried.append(rec)
        if max(rec['final_px']) <= FL.PIXEL_BAR / 2:
            break
        theta = theta / 2
    out = dict(tried[-1])
    out['tried'] = [{k: t[k] for k in ('theta0', 'start_px', 'final_px')} for t in tried]
    return 'refine_only', out


def case_cma_then_refine(_=None):
    return 'cma_then_refine', _refined(D.scene('tilted'), np.array(R.THETA_START), CMA_GENERATIONS)


def _call(job):
    fn, arg = job
    return globals()[fn](arg)


def load():
    with open(PATH) as f:
        return json.load(f)


def adjoint_bars(H, W, mask_name):
    """(bars of d_moving [6], bars of its sum [6]) per view of reg_ref.sim_images, as fractions of the view's largest |adjoint|."""
    e = load()['adjoint']['%dx%d/%s' % (H, W, mask_name)]
    return BAR_FACTOR * np.array(e['floor']), BAR_FACTOR * np.array(e['sum_floor'])


def moment_bar(kind, view, step, pattern):
    """The bar of the twelve numbers in their own units: BAR_FACTOR x floor x the largest entry."""
    e = load()['moments'][moment_key(kind, view, step, pattern)]
    return BAR_FACTOR * e['floor'] * e['scale']


if __name__ == '__main__':
    doc = {'what': '(adjoint, moments, theta) largest |float32 model - float64 model| as a fraction of the largest entry (tests/grad_ref.py); '
                   '(refinement) the cases of tests/test_gpu_pose_grad.py run with dfl_amd.register.bfgs and cma_es on the numpy models: '
                   'distances in pixels between ellipsoid centres projected under the true and the found pose',
           'tool': 'python tests/grad_floor.py', 'numpy': np.__version__, 'bar_factor': BAR_FACTOR, 'adjoint': adjoint_floors(),
           'moments': {}, 'refinement': {}}
    jobs = [('moment_case', c) for c in MOMENT_CASES] + [('theta_case', None), ('case_refine_only', None), ('case_cma_then_refine', None)]
    with multiprocessing.Pool(min(len(jobs), os.cpu_count() or 1, 16)) as pool:
        for name, rec in pool.map(_call, jobs, chunksize=1):
            if name == 'theta':
                doc['theta'] = rec
            elif name in ('refine_only', 'cma_then_refine'):
                doc['refinement'][name] = rec
            else:
                doc['moments'][name] = rec
    os.makedirs(os.path.dirname(PATH), exist_ok=True)
    with open(PATH, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps({k: doc[k] for k in ('theta', 'refinement')}, indent=1, sort_keys=True))
    print({k: (v['floor'], v['zeroed_rays']) for k, v in doc['moments'].items()})
    print({k: (max(v['floor']), max(v['sum_floor'])) for k, v in doc['adjoint'].items()})
