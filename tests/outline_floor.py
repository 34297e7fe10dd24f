"""What the models alone do on the outline registrations of tests/test_gpu_outline.py (offline, on the CPU, never the
kernel); the result is committed as tests/golden/floors/outline.json.

The tilted scene (45 x 61, six ellipsoids), all three objects moving, the product's own cma_es and pose_deltas on the
numpy renderer (drr_ref, exact, label_map) and the numpy outline cost (outline_ref); the fixed input is the model's
label_map at the true poses, for the intensity stages its exact DRR.  Distances are pixels between ellipsoid centres
projected under the true and the found pelvis pose (reg_ref.centre_distances).

    near            THETA_START, sigma 2, 40 generations, cap 16
    far             2.5 x THETA_START, sigma 4, 60 generations, cap 16
    far_intensity   the gradient-NCC alone (global, trilinear, step 1) from the far start: recorded, not asserted
    two_stage       far, then 40 generations of the global gradient-NCC with sigma 1 and seed 1

`near` and `far` are refused when the model's largest final distance exceeds MODEL_BAR: lengthen the run then, not the
bar.  The cases run side by side, a few minutes in all.

    python tests/outline_floor.py            # rewrites tests/golden/floors/outline.json
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
import outline_ref as O  # noqa: E402
import reg_ref as R  # noqa: E402

PATH = os.path.join(HERE, 'golden', 'floors', 'outline.json')
POPSIZE, SEED, STEP_MM, CAP = 16, 0, 1.0, 16.0
MODEL_BAR = 1.0                        # pixels: the largest final distance `near` and `far` may record
BAR_FACTOR = 2.0                       # what the GPU test allows: this times the largest recorded distance of the case
FAR_FACTOR = 2.5
SETTINGS = {'near': dict(theta0=tuple(R.THETA_START), sigma0=2.0, generations=40),
            'far': dict(theta0=tuple(FAR_FACTOR * t for t in R.THETA_START), sigma0=4.0, generations=60)}
SECOND = dict(sigma0=1.0, generations=40, seed=1)


def fixed_seg(S):
    """The model's label map at the true poses."""
    return O.render_labels(S, S['poses'])


def fixed_image(S):
    return D.model('tilted', 'exact', 0)[0]


def pelvis_px(S, theta):
    from dfl_amd import register as reg
    return [float(d) for d in R.centre_distances(S, S['poses'][0], reg.pose_delta(theta, R.volume_centre(S)) @ S['poses'][0])]


def start_and_truth_cost(S, theta0, cap=CAP):
    """(the outline cost at theta0, at theta = 0) of the model: what tests/test_outline_cpu.py recomputes."""
    from dfl_amd import register as reg
    fn = O.model_cost_fn(S, S['poses'], (0, 1, 2), fixed_seg(S), reg.pose_deltas, cap)
    c = fn(np.array([theta0, np.zeros(6)]))
    return float(c[0]), float(c[1])


def _search(fn, x0, sigma0, generations, seed):
    from dfl_amd import register as reg
    res = reg.cma_es(fn, np.asarray(x0, np.float64), sigma0, POPSIZE, generations, seed)
    return res, {'theta': [float(t) for t in res.mean], 'generations': generations, 'sigma0': sigma0, 'popsize': POPSIZE, 'seed': seed,
                 'cost_first_generation': float(res.trace[0]), 'cost_last_generation': float(res.trace[-1]),
                 'final_cost': float(fn(res.mean[None])[0])}


def _outline(name):
    from dfl_amd import register as reg
    S = D.scene('tilted')
    st = SETTINGS[name]
    fn = O.model_cost_fn(S, S['poses'], (0, 1, 2), fixed_seg(S), reg.pose_deltas, CAP)
    res, rec = _search(fn, st['theta0'], st['sigma0'], st['generations'], SEED)
    start, truth = start_and_truth_cost(S, st['theta0'])
    rec.update(theta0=list(st['theta0']), cap=CAP, label_sets=[list(s) for s in O.DEFAULT_SETS], start_cost=start, truth_cost=truth,
               start_px=pelvis_px(S, st['theta0']), final_px=pelvis_px(S, res.mean))
    return res, rec


def _intensity_fn(S):
    from dfl_amd import register as reg
    return R.model_cost_fn(S, S['poses'], (0, 1, 2), fixed_image(S), reg.pose_deltas, STEP_MM)


def case_near(_=None):
    return [('near', _outline('near')[1])]


def case_far(_=None):
    """far, and two_stage from its result."""
    S = D.scene('tilted')
    res, rec = _outline('far')
    fn = _intensity_fn(S)
    res2, rec2 = _search(fn, res.mean, SECOND['sigma0'], SECOND['generations'], SECOND['seed'])
    rec2.update(theta0=[float(t) for t in res.mean], start_cost=float(fn(res.mean[None])[0]), start_px=rec['final_px'],
                final_px=pelvis_px(S, res2.mean))
    return [('far', rec), ('two_stage', rec2)]


def case_far_intensity(_=None):
    S = D.scene('tilted')
    st = SETTINGS['far']
    fn = _intensity_fn(S)
    res, rec = _search(fn, st['theta0'], st['sigma0'], st['generations'], SEED)
    rec.update(theta0=list(st['theta0']), start_cost=float(fn(np.array([st['theta0']]))[0]), start_px=pelvis_px(S, st['theta0']),
               final_px=pelvis_px(S, res.mean), asserted=False)
    return [('far_intensity', rec)]


CASES = {'near': case_near, 'far': case_far, 'far_intensity': case_far_intensity}


def _call(name):
    return CASES[name]()


def load():
    with open(PATH) as f:
        return json.load(f)


def bar(case):
    """BAR_FACTOR x the largest final distance the committed file records for the case, in pixels."""
    return BAR_FACTOR * max(load()['registration'][case]['final_px'])


if __name__ == '__main__':
    names = [a for a in sys.argv[1:] if a in CASES] or list(CASES)
    doc = {'what': 'the outline registrations of tests/test_gpu_outline.py run with dfl_amd.register.cma_es and pose_deltas on the numpy '
                   'renderer (exact, label_map) and the numpy outline cost (tests/outline_ref.py), the intensity stages on the numpy '
                   'gradient-NCC (tests/reg_ref.py): distances in pixels between ellipsoid centres projected under the true and the '
                   'found pelvis pose',
           'tool': 'python tests/outline_floor.py', 'numpy': np.__version__, 'model_bar_pixels': MODEL_BAR, 'bar_factor': BAR_FACTOR,
           'registration': {}}
    if os.path.exists(PATH):                                    # a run of some cases keeps the others
        doc['registration'] = load().get('registration', {})
    with multiprocessing.Pool(len(names)) as pool:
        for recs in pool.map(_call, names):
            for name, rec in recs:
                if name in SETTINGS and max(rec['final_px']) > MODEL_BAR:
                    raise SystemExit('outline_floor: the model ends %s %.3f px off (more than %.1f): lengthen the run, not the bar'
                                     % (name, max(rec['final_px']), MODEL_BAR))
                doc['registration'][name] = rec
    os.makedirs(os.path.dirname(PATH), exist_ok=True)
    with open(PATH, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(doc, indent=1, sort_keys=True))
