"""What the models alone do on the registration tests (offline, on the CPU, never the kernel); the result is committed
as tests/golden/floors/register.json.

(a) Similarity floors: for the test images of tests/test_gpu_register.py (reg_ref.sim_images, every size and mask) the
    largest |float32 model - float64 model| of the cost.  The GPU test allows the kernel 8 x the floor of its size and
    mask (the factor of tests/drr_floor.py: it covers FMA contraction and another, legitimate summation order).
(b) The registration cases of the GPU test, run with the product's own cma_es, pose_delta and pnp but the numpy
    renderer and the numpy cost: the check that the inputs are solvable by the model alone, inside the GPU test's bars
    with a margin.  About three minutes per case; the cases run side by side.

    python tests/reg_floor.py            # rewrites tests/golden/floors/register.json
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
import reg_ref as R  # noqa: E402

PATH = os.path.join(HERE, 'golden', 'floors', 'register.json')
BAR_FACTOR = 8.0
POPSIZE, SEED, STEP_MM = 16, 0, 1.0
PIXEL_BAR, FEMUR_BAR, FEMUR_MODEL_BAR, COST_FACTOR = 0.25, 0.5, 0.125, 2.0


def sim_floors():
    out = {}
    for H, W in R.SIM_SIZES:
        fixed, moving = R.sim_images(H, W)
        for name, mask in R.sim_masks(H, W).items():
            c64, c32 = R.cost(moving, fixed, mask), R.cost(moving, fixed, mask, dtype=np.float32)
            out['%dx%d/%s' % (H, W, name)] = {'floor': float(np.abs(c32 - c64).max()), 'cost': [float(c) for c in c64],
                                              'counted': int(R.counted(H, W, mask).sum())}
    return out


class ModelGeom:
    """What dfl_amd.register.pnp reads of a drr.Geometry, for the tilted scene on its full detector grid."""

    def __init__(self, S):
        self.K, self.E, self.G = S['K'], S['E'], np.eye(3)


def fixed_image(S):
    return D.model('tilted', 'exact', 0)[0]


def truth_cost(S):
    """The model's cost at the true pose, trilinear with step 0.5 against the exact fixed image."""
    return float(R.cost(R.render_poses(S, S['poses'], 'trilinear', 0.5), fixed_image(S)))


def landmark_start(S):
    """(x2d with its NaN column, P_init, the pelvis pose pnp returns) of case 3."""
    from dfl_amd import register as reg
    x2d = R.project(S, S['poses'][0], R.centres_phys(S)) + R.LAND_OFFSETS
    x2d[:, R.LAND_MISSING] = np.nan
    P_init = reg.pose_delta(R.THETA_START, R.volume_centre(S)) @ S['poses'][0]
    return x2d, P_init, reg.pnp(ModelGeom(S), R.centres_phys(S), x2d, P_init=P_init)


def _run(S, start_poses, moving, x0, sigma0, generations):
    from dfl_amd import register as reg
    fn = R.model_cost_fn(S, start_poses, moving, fixed_image(S), reg.pose_deltas, STEP_MM)
    res = reg.cma_es(fn, x0, sigma0, POPSIZE, generations, SEED)
    Dm = reg.pose_delta(res.mean, R.volume_centre(S))
    final = [Dm @ P if n in moving else P for n, P in enumerate(start_poses)]
    return res, final, {'theta': [float(t) for t in res.mean], 'generations': generations, 'sigma0': sigma0, 'popsize': POPSIZE,
                        'seed': SEED, 'cost_first_generation': float(res.trace[0]), 'cost_last_generation': float(res.trace[-1]),
                        'final_cost_step_1.0': float(fn(res.mean[None])[0]),
                        'final_cost_step_0.5': float(R.cost(R.render_poses(S, final, 'trilinear', 0.5), fixed_image(S)))}


def case_offset(_=None):
    S = D.scene('tilted')
    from dfl_amd import register as reg
    P_start = reg.pose_delta(R.THETA_START, R.volume_centre(S)) @ S['poses'][0]
    res, final, rec = _run(S, S['poses'], (0, 1, 2), np.array(R.THETA_START), 2.0, 80)
    rec.update(theta0=list(R.THETA_START), start_px=[float(d) for d in R.centre_distances(S, S['poses'][0], P_start)],
               final_px=[float(d) for d in R.centre_distances(S, S['poses'][0], final[0])])
    return 'offset', rec


def case_landmarks(_=None):
    S = D.scene('tilted')
    _, _, P_pnp = landmark_start(S)
    D_start = P_pnp @ np.linalg.inv(S['poses'][0])
    res, final, rec = _run(S, [D_start @ P for P in S['poses']], (0, 1, 2), np.zeros(6), 1.0, 40)
    rec.update(offsets=R.LAND_OFFSETS.tolist(), missing=R.LAND_MISSING,
               start_px=[float(d) for d in R.centre_distances(S, S['poses'][0], P_pnp)],
               final_px=[float(d) for d in R.centre_distances(S, S['poses'][0], final[0])])
    return 'landmarks', rec


def case_femur(_=None):
    """The issue's start offset (0.06 rad, (3, -2, 6) mm), halved until the model ends within FEMUR_MODEL_BAR."""
    S = D.scene('tilted')
    from dfl_amd import register as reg
    X = R.centres_phys(S)[4:5]                                   # the left femur's ellipsoid (label 5)
    theta = np.array(R.THETA_FEMUR)
    tried = []
    for halvings in range(4):
        D_f = reg.pose_delta(theta, R.volume_centre(S))
        start = [S['poses'][0], D_f @ S['poses'][1], S['poses'][2]]
        res, final, rec = _run(S, start, (1,), np.zeros(6), 2.0, 80)
        dist = lambda P: float(np.hypot(*(R.project(S, S['poses'][1], X) - R.project(S, P, X)))[0])  # noqa: E731
        rec.update(theta_start=[float(t) for t in theta], halvings=halvings, start_px=dist(start[1]), final_px=dist(final[1]))
        rec['start_cost_step_1.0'] = float(R.cost(R.render_poses(S, start, 'trilinear', STEP_MM), fixed_image(S)))
        tried.append(rec)
        if rec['final_px'] <= FEMUR_MODEL_BAR:
            break
        theta = theta / 2
    out = dict(tried[-1])
    out['tried'] = [{k: t[k] for k in ('theta_start', 'start_px', 'final_px')} for t in tried]
    return 'femur', out


CASES = {'offset': case_offset, 'landmarks': case_landmarks, 'femur': case_femur}


def _call(name):
    return CASES[name]()


def load():
    with open(PATH) as f:
        return json.load(f)


def sim_bar(H, W, mask_name):
    """BAR_FACTOR x the committed floor of that size and mask."""
    return BAR_FACTOR * load()['similarity']['%dx%d/%s' % (H, W, mask_name)]['floor']


if __name__ == '__main__':
    names = [a for a in sys.argv[1:] if a in CASES] or list(CASES)
    S = D.scene('tilted')
    doc = {'what': '(similarity) largest |float32 model - float64 model| of the gradient-NCC cost over the six test images, per size '
                   'and mask (tests/reg_ref.py); (registration) the cases of tests/test_gpu_register.py run with dfl_amd.register.cma_es, '
                   'pose_delta and pnp on the numpy renderer and the numpy cost: distances in pixels between ellipsoid centres projected '
                   'under the true and the found pose',
           'tool': 'python tests/reg_floor.py', 'numpy': np.__version__, 'bar_factor': BAR_FACTOR,
           'bars': {'pixels': PIXEL_BAR, 'femur_pixels': FEMUR_BAR, 'femur_model_pixels': FEMUR_MODEL_BAR, 'cost_factor': COST_FACTOR},
           'similarity': sim_floors(), 'cost_at_truth_step_0.5': truth_cost(S), 'registration': {}}
    if os.path.exists(PATH):                                    # a run of some cases keeps the others
        doc['registration'] = load().get('registration', {})
    with multiprocessing.Pool(len(names)) as pool:
        for name, rec in pool.map(_call, names):
            doc['registration'][name] = rec
    os.makedirs(os.path.dirname(PATH), exist_ok=True)
    with open(PATH, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(doc, indent=1, sort_keys=True))
