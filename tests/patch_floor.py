"""What the models alone do on the tests of the patch-wise gradient-NCC and of the landmark term (offline, on the CPU,
never the kernel); the result is committed as tests/golden/floors/register_patch.json.  In the manner of
tests/reg_floor.py, whose constants (the factor 8, the pixel bar) hold here too.

(a) Similarity floors: for the test images of tests/test_gpu_register_patch.py (reg_ref.sim_images at patch_ref.SIZES,
    every mask, every (radius, stride) of patch_ref.PARAMS that fits, min_count 1 and the default) the largest
    |float32-gradient model - float64 model| of the cost.  The GPU test allows the kernel 8 x the floor of its case.
(b) The registration cases A to D of the GPU test, run with the product's own cma_es and pose_deltas but the numpy
    renderer and the numpy costs (patch_ref.cost, patch_ref.landmark_penalty).  About three minutes per 80 generations;
    the cases run side by side.

    python tests/patch_floor.py            # rewrites tests/golden/floors/register_patch.json
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
import patch_ref as PT  # noqa: E402
import reg_floor as FL  # noqa: E402
import reg_ref as R  # noqa: E402

PATH = os.path.join(HERE, 'golden', 'floors', 'register_patch.json')
RHO, STRIDE = 7, 4                       # the registrations' patches
LAND_WEIGHT = 0.01                       # per square pixel
SHORT, LONG = 30, 80                     # generations
MODEL_FACTOR = 2.0                       # cases C and D: the GPU run within this many times the model's largest distance


def key(H, W, rho, stride, mask_name, min_count):
    return '%dx%d/r%d_s%d/%s/m%d' % (H, W, rho, stride, mask_name, min_count)


def sim_floors():
    out = {}
    for H, W, rho, stride in PT.cases():
        fixed, moving = R.sim_images(H, W)
        for name, mask in R.sim_masks(H, W).items():
            for mc in (1, PT.default_min_count(rho)):
                c64 = PT.cost(moving, fixed, mask, rho, stride, mc)
                c32 = PT.cost(moving, fixed, mask, rho, stride, mc, dtype=np.float32)
                _, flags, _ = PT.fixed_patches(fixed, mask, rho, stride, mc)
                out[key(H, W, rho, stride, name, mc)] = {'floor': float(np.abs(c32 - c64).max()), 'cost': [float(c) for c in c64],
                                                         'count_x': int((flags & 1).sum()), 'count_y': int((flags >> 1 & 1).sum()),
                                                         'patches': int(flags.size)}
    return out


def sim_bar(H, W, rho, stride, mask_name, min_count):
    """FL.BAR_FACTOR x the committed floor of that case."""
    return FL.BAR_FACTOR * load()['similarity'][key(H, W, rho, stride, mask_name, min_count)]['floor']


def landmarks(S):
    """(X3d [6, 3], x2d [2, 6]) of cases B and C: the projected centres plus reg_ref.LAND_OFFSETS, one column missing."""
    X = R.centres_phys(S)
    x2d = R.project(S, S['poses'][0], X) + R.LAND_OFFSETS
    x2d[:, R.LAND_MISSING] = np.nan
    return X, x2d


def foreign_fixed(S):
    return PT.with_bar(FL.fixed_image(S))


def _run(fixed_of, patch, with_lands, generations):
    """All three bones from reg_ref.THETA_START, sigma0 2, as case 2 of tests/reg_floor.py, under the cost named."""
    from dfl_amd import register as reg
    S = D.scene('tilted')
    fixed, ctr = fixed_of(S), R.volume_centre(S)
    X, x2d = landmarks(S)

    def sim(img):
        return float(PT.cost(img, fixed, None, RHO, STRIDE) if patch else R.cost(img, fixed))

    def fn(thetas):
        Ds = reg.pose_deltas(thetas, ctr)
        out = np.array([sim(R.render_poses(S, [Dm @ P for P in S['poses']], 'trilinear', FL.STEP_MM)) for Dm in Ds])
        if with_lands:
            out = out + PT.landmark_penalty(S, Ds @ S['poses'][0][None], X, x2d, LAND_WEIGHT)
        return out

    res = reg.cma_es(fn, np.array(R.THETA_START), 2.0, FL.POPSIZE, generations, FL.SEED)
    P_start = reg.pose_delta(R.THETA_START, ctr) @ S['poses'][0]
    P_final = reg.pose_delta(res.mean, ctr) @ S['poses'][0]
    return {'theta': [float(t) for t in res.mean], 'generations': generations, 'sigma0': 2.0, 'popsize': FL.POPSIZE, 'seed': FL.SEED,
            'similarity': 'patch' if patch else 'global', 'landmark_weight': LAND_WEIGHT if with_lands else 0.0,
            'cost_first_generation': float(res.trace[0]), 'cost_last_generation': float(res.trace[-1]),
            'final_cost': float(fn(res.mean[None])[0]), 'cost_at_truth': float(fn(np.zeros((1, 6)))[0]),
            'start_px': [float(d) for d in R.centre_distances(S, S['poses'][0], P_start)],
            'final_px': [float(d) for d in R.centre_distances(S, S['poses'][0], P_final)]}


CASES = {'A': (FL.fixed_image, True, False, LONG), 'B': (FL.fixed_image, True, True, LONG),
         'A_short': (FL.fixed_image, True, False, SHORT), 'C': (FL.fixed_image, True, True, SHORT),
         'D': (foreign_fixed, True, False, LONG), 'D_global': (foreign_fixed, False, False, LONG)}


def _call(name):
    return name, _run(*CASES[name])


def load():
    with open(PATH) as f:
        return json.load(f)


if __name__ == '__main__':
    names = [a for a in sys.argv[1:] if a in CASES] or list(CASES)
    doc = {'what': '(similarity) largest |float32-gradient model - float64 model| of the patch-wise gradient-NCC cost over the six test '
                   'images, per size, (radius, stride), mask and min_count (tests/patch_ref.py); (registration) the cases of '
                   'tests/test_gpu_register_patch.py run with dfl_amd.register.cma_es and pose_deltas on the numpy renderer and the '
                   'numpy costs: distances in pixels between ellipsoid centres projected under the true and the found pose',
           'tool': 'python tests/patch_floor.py', 'numpy': np.__version__, 'bar_factor': FL.BAR_FACTOR,
           'bars': {'pixels': FL.PIXEL_BAR, 'model_factor': MODEL_FACTOR}, 'patch': {'radius': RHO, 'stride': STRIDE},
           'similarity': sim_floors(), 'registration': {}}
    if os.path.exists(PATH):                                    # a run of some cases keeps the others
        doc['registration'] = load().get('registration', {})
    if '--floors-only' not in sys.argv[1:]:
        with multiprocessing.Pool(len(names)) as pool:
            for name, rec in pool.map(_call, names):
                doc['registration'][name] = rec
    os.makedirs(os.path.dirname(PATH), exist_ok=True)
    with open(PATH, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(doc['registration'], indent=1, sort_keys=True))
