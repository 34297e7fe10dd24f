"""What the models alone do on the tests of the weighted patch gradient-NCC and of the patch adjoint (offline, on the
CPU, never the kernel); the result is committed as tests/golden/floors/register_wpatch.json.  In the manner of
tests/patch_floor.py and tests/grad_floor.py, whose constants (the factor 8, the pixel bar, the factor 2 of case D) hold
here too.

(a) Floors, per case = size x (radius, stride) of patch_grad_ref.cases() x mask x min_count (1 and the default), over the
    six images of reg_ref.sim_images: the largest |float32 model - float64 model| of the weighted cost, and per weighting
    and view that of the adjoint as a fraction of the view's largest |adjoint|.  Views 0, 1 and 3 (the fixed image, its
    negation, 3 fixed + 2) sit at an extremum of every patch's ncc: their float64 adjoint is rounding noise, and their
    scale is that of view 4 of the same case.  (The negated image is the third of them: with a = -b the two terms of
    every patch are (alpha - beta)(b - mean b) with alpha = beta.)  A floor of 0 asks the kernel for exact equality.
    The GPU tests allow the kernel BAR_FACTOR x the floor of its case.
(b) The input condition, asserted here for every input and recorded per case: no live patch has the variance ratio of its
    fixed gradient inside patch_ref.BAND, and no (view, patch that counts) that of its moving gradient -- inside the band
    the float32 and the float64 model may decide "the variance is 0" differently.
(c) The adjoint of the float64 model against central differences of its cost at single pixels (CHECK_PIXELS): the largest
    error as a fraction of the largest |adjoint|; tests/test_register_wpatch_cpu.py asserts 10 x this.
(d) The registrations E, F, G of tests/test_gpu_register_wpatch.py with the product's cma_es, bfgs and pose_deltas on the
    numpy renderer, the numpy cost and the numpy gradient (grad_ref.pose_moments and chain).

    python tests/patch_grad_floor.py [--floors-only] [E F G G_uniform]    # rewrites tests/golden/floors/register_wpatch.json
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
import patch_grad_ref as PG  # noqa: E402
import patch_ref as PT  # noqa: E402
import reg_floor as FL  # noqa: E402
import reg_ref as R  # noqa: E402

PATH = os.path.join(HERE, 'golden', 'floors', 'register_wpatch.json')
BAR_FACTOR = FL.BAR_FACTOR
RHO, STRIDE = 7, 4                       # the registrations' patches
GENERATIONS = 80
REFINE, REFINE_TOL, REFINE_START = 30, 1e-4, 0.15
MODEL_FACTOR = 2.0                       # case G: the GPU run within this many times the model's largest distance
EXTREMAL_VIEWS, SCALE_VIEW = (0, 1, 3), 4
FD_CASE = (17, 70, 1, 4, 'ragged', 1)    # (c): pixels in no patch and under the mask ...
FD_CASE_DENSE = (17, 70, 3, 2, 'none', 1)   # ... and pixels covered by 1, 4 and 9 patches
FD_VIEW, FD_STEP = 4, 1e-6                 # the truncation error falls with the square of the step: 1e-8 at 1e-5, 1e-9 here


def key(H, W, rho, stride, mask_name, min_count):
    return '%dx%d/r%d_s%d/%s/m%d' % (H, W, rho, stride, mask_name, min_count)


def in_band(ratios):
    r = np.asarray(ratios, np.float64).reshape(-1)
    return bool(((r > PT.BAND[0]) & (r < PT.BAND[1])).any())


def input_condition(fixed, moving, mask, rho, stride, min_count):
    """Raises when an input breaks (b); returns the ratios nearest to the band from above, (fixed, moving)."""
    near = []
    for dt in (np.float64, np.float32):
        totals, flags, ratios = PT.fixed_patches(fixed, mask, rho, stride, min_count, dt)
        live = totals[:, 0] >= min_count
        _, _, mr = PG.patch_terms(moving, fixed, mask, rho, stride, min_count, dt)
        counts = np.stack([flags & 1, flags >> 1 & 1], 1).astype(bool)
        fr, mr = ratios[live], mr[:, counts]
        if in_band(fr) or in_band(mr):
            raise AssertionError('a variance ratio inside patch_ref.BAND: replace the input, not the band')
        near.append([float(v[v >= PT.BAND[1]].min()) if (v >= PT.BAND[1]).any() else None for v in (fr.reshape(-1), mr.reshape(-1))])
    return near


def floors_of(case):
    H, W, rho, stride = case
    fixed, moving = R.sim_images(H, W)
    out = {}
    for name, mask in R.sim_masks(H, W).items():
        for mc in sorted({1, PT.default_min_count(rho)}):
            near = input_condition(fixed, moving, mask, rho, stride, mc)
            t64 = PG.patch_terms(moving, fixed, mask, rho, stride, mc)
            t32 = PG.patch_terms(moving, fixed, mask, rho, stride, mc, np.float32)
            rec = {'nearest_ratio_above_band': near, 'adjoint': {}}
            for weight in PG.WEIGHTS:
                c64, d64 = PG.adjoint(moving, fixed, mask, rho, stride, mc, np.float64, weight, t64)
                c32, d32 = PG.adjoint(moving, fixed, mask, rho, stride, mc, np.float32, weight, t32)
                scale = np.abs(d64).max((1, 2))
                scale[list(EXTREMAL_VIEWS)] = scale[SCALE_VIEW]
                err = np.abs(d32.astype(np.float64) - d64).max((1, 2))
                rec['adjoint'][weight] = {'floor': [float(e / s) if s > 0 else float(e) for e, s in zip(err, scale)],
                                          'scale': [float(s) for s in scale]}
                if weight == 'variance':
                    rec.update(floor=float(np.abs(c32 - c64).max()), cost=[float(c) for c in c64])
            w, tot = PG.weights(fixed, mask, rho, stride, mc)
            rec.update(pwsum=[float(t) for t in tot], largest_weight=float(w.max()) if w.size else 0.0)
            out[key(H, W, rho, stride, name, mc)] = rec
    return out


# ---- (c) ---------------------------------------------------------------------------------------------------------------
def check_pixels(H, W, rho, stride, mask):
    """At least 20 (r, c): a border pixel, one under the mask, one in no patch, one of every coverage found (so 1, 4 and 9 of
    FD_CASE_DENSE), then a regular lattice."""
    cov = np.zeros((H, W), np.int64)
    cov[1:-1, 1:-1] = PG.coverage(H, W, rho, stride)
    px = [(0, W // 2), (H - 1, 0)]
    if mask is not None:
        rr, cc = np.nonzero(np.asarray(mask) == 0)
        inner = [(r, c) for r, c in zip(rr, cc) if 2 <= r < H - 2 and 2 <= c < W - 2]
        px.append(inner[len(inner) // 2])
    for n in np.unique(cov[2:-2, 2:-2]):
        rr, cc = np.nonzero(cov[2:-2, 2:-2] == n)
        px.append((int(rr[len(rr) // 2]) + 2, int(cc[len(cc) // 2]) + 2))
    px += [(r, c) for r in range(1, H, 5) for c in range(2, W, 11)]
    return [(int(r), int(c)) for r, c in dict.fromkeys(px)]


def fd_error(case, weight):
    """The largest |adjoint - central difference of the cost| over check_pixels as a fraction of the largest |adjoint|, float64 model."""
    H, W, rho, stride, mask_name, mc = case
    fixed, moving = R.sim_images(H, W)
    mask = R.sim_masks(H, W)[mask_name]
    # a patch's ncc does not depend on the scale of a, so it has no derivative where the moving patch is flat (the background of a
    # rendered view): the texture leaves no such patch
    mv = PG.textured(moving[FD_VIEW])
    _, d = PG.adjoint(mv, fixed, mask, rho, stride, mc, np.float64, weight)
    worst = 0.0
    for r, c in check_pixels(H, W, rho, stride, mask):
        hi, lo = mv.copy(), mv.copy()
        hi[r, c] += FD_STEP
        lo[r, c] -= FD_STEP
        fd = (PG.cost(hi, fixed, mask, rho, stride, mc, np.float64, weight) - PG.cost(lo, fixed, mask, rho, stride, mc, np.float64, weight)) / (2 * FD_STEP)
        worst = max(worst, abs(fd - d[r, c]))
    return worst / float(np.abs(d).max())


def fd_floors():
    return {'%s/%s' % (key(*case), w): fd_error(case, w) for case in (FD_CASE, FD_CASE_DENSE) for w in PG.WEIGHTS}


# ---- (d) ---------------------------------------------------------------------------------------------------------------
def textured_fixed(S):
    return PG.textured(FL.fixed_image(S))


def _sim(fixed, weight):
    return lambda img: float(PG.cost(img, fixed, None, RHO, STRIDE, None, np.float64, weight))


def _px(S, theta):
    from dfl_amd import register as reg
    return [float(d) for d in R.centre_distances(S, S['poses'][0], reg.pose_delta(theta, R.volume_centre(S)) @ S['poses'][0])]


def _run_cma(fixed_of, weight):
    """All three bones from reg_ref.THETA_START, sigma0 2, GENERATIONS generations, under the patch cost of that weighting."""
    from dfl_amd import register as reg
    S = D.scene('tilted')
    sim, ctr = _sim(fixed_of(S), weight), R.volume_centre(S)

    def fn(thetas):
        return np.array([sim(R.render_poses(S, [Dm @ P for P in S['poses']], 'trilinear', FL.STEP_MM)) for Dm in reg.pose_deltas(thetas, ctr)])

    res = reg.cma_es(fn, np.array(R.THETA_START), 2.0, FL.POPSIZE, GENERATIONS, FL.SEED)
    return {'theta': [float(t) for t in res.mean], 'generations': GENERATIONS, 'sigma0': 2.0, 'popsize': FL.POPSIZE, 'seed': FL.SEED,
            'patch_weight': weight, 'cost_first_generation': float(res.trace[0]), 'cost_last_generation': float(res.trace[-1]),
            'final_cost': float(fn(res.mean[None])[0]), 'cost_at_truth': float(fn(np.zeros((1, 6)))[0]),
            'start_px': _px(S, np.array(R.THETA_START)), 'final_px': _px(S, res.mean)}


def model_cost_and_grad(S, fixed, weight, pose_deltas):
    """grad_ref.model_cost_and_grad with the patch cost and its adjoint in place of the global ones."""
    ctr, q = R.volume_centre(S), S['Q'].astype(np.float32)

    def fun(theta):
        Dm = pose_deltas(np.asarray(theta, np.float64).reshape(1, 6), ctr)[0]
        recs = D.pack([D.c2i(S['I2P'], Dm @ P, S['E']) for P in S['poses']], D.MASKS, S['Q'], S['lab'], True, 'trilinear')
        att = D.render(S['mu'], S['lab'], recs, q, S['rows'], S['cols'], 'trilinear', step_mm=FL.STEP_MM)[0]
        cost, d_att = PG.adjoint(att, fixed, None, RHO, STRIDE, None, np.float64, weight)
        piv = G.box_pivots(recs)
        grad = G.pose_moments(S['mu'], S['lab'], recs, q, S['rows'], S['cols'], d_att, piv, FL.STEP_MM)
        return float(cost), G.chain(grad, piv, G.xi(theta, ctr, S['I2P'], pose_deltas), (0, 1, 2))

    return fun


def case_F(_=None):
    """generations=0, refine=REFINE from REFINE_START x THETA_START, halved until the models alone end within half of the pixel bar."""
    from dfl_amd import register as reg
    S = D.scene('tilted')
    fun = model_cost_and_grad(S, FL.fixed_image(S), 'variance', reg.pose_deltas)
    theta, tried = REFINE_START * np.array(R.THETA_START), []
    for halvings in range(4):
        fin = reg.bfgs(fun, theta, REFINE, REFINE_TOL)
        rec = {'theta0': [float(t) for t in theta], 'theta': [float(t) for t in fin.x], 'start_px': _px(S, theta), 'final_px': _px(S, fin.x),
               'refine_cost': [float(c) for c in fin.trace], 'gradient_evaluations': fin.evaluations, 'iterations': fin.iterations,
               'halvings': halvings, 'refine': REFINE, 'refine_tol': REFINE_TOL, 'patch_weight': 'variance'}
        tried.append(rec)
        if max(rec['final_px']) <= FL.PIXEL_BAR / 2:
            break
        theta = theta / 2
    out = dict(tried[-1])
    out['tried'] = [{k: t[k] for k in ('theta0', 'start_px', 'final_px')} for t in tried]
    return out


CASES = {'E': lambda: _run_cma(FL.fixed_image, 'variance'), 'F': case_F, 'G': lambda: _run_cma(textured_fixed, 'variance'),
         'G_uniform': lambda: _run_cma(textured_fixed, 'uniform')}


def _call(job):
    kind, arg = job
    if kind == 'floors':
        return kind, floors_of(arg)
    if kind == 'fd':
        return kind, fd_floors()
    return arg, CASES[arg]()


def load():
    with open(PATH) as f:
        return json.load(f)


def cost_bar(H, W, rho, stride, mask_name, min_count):
    """BAR_FACTOR x the committed floor of the weighted cost of that case."""
    return BAR_FACTOR * load()['similarity'][key(H, W, rho, stride, mask_name, min_count)]['floor']


def adjoint_bars(H, W, rho, stride, mask_name, min_count, weight):
    """(bars [6] in the adjoint's own units, one per view of reg_ref.sim_images: BAR_FACTOR x floor x scale; the scales [6])."""
    e = load()['similarity'][key(H, W, rho, stride, mask_name, min_count)]['adjoint'][weight]
    scale = np.array(e['scale'])
    return BAR_FACTOR * np.array(e['floor']) * np.where(scale > 0, scale, 1.0), scale


if __name__ == '__main__':
    names = [a for a in sys.argv[1:] if a in CASES] or list(CASES)
    if '--floors-only' in sys.argv[1:]:
        names = []
    doc = {'what': '(similarity) per size, (radius, stride), mask and min_count: the largest |float32 model - float64 model| of the weighted '
                   'patch gradient-NCC cost over the six test images, and per weighting and view that of the adjoint as a fraction of the '
                   "view's largest |adjoint| (views 0, 1, 3: of view 4's) (tests/patch_grad_ref.py); (finite_differences) the float64 adjoint "
                   'against central differences of the cost; (registration) the cases of tests/test_gpu_register_wpatch.py on the numpy models: '
                   'distances in pixels between ellipsoid centres projected under the true and the found pose',
           'tool': 'python tests/patch_grad_floor.py', 'numpy': np.__version__, 'bar_factor': BAR_FACTOR,
           'bars': {'pixels': FL.PIXEL_BAR, 'model_factor': MODEL_FACTOR}, 'patch': {'radius': RHO, 'stride': STRIDE}, 'band': list(PT.BAND),
           'similarity': {}, 'finite_differences': {}, 'registration': {}}
    if os.path.exists(PATH):                                    # a run of some cases keeps the others
        doc['registration'] = load().get('registration', {})
    jobs = [('case', n) for n in names] + [('fd', None)] + [('floors', c) for c in PG.cases()]
    with multiprocessing.Pool(min(len(jobs), os.cpu_count() or 1, 16)) as pool:
        for kind, rec in pool.imap_unordered(_call, jobs, chunksize=1):
            if kind == 'floors':
                doc['similarity'].update(rec)
            elif kind == 'fd':
                doc['finite_differences'] = rec
            else:
                doc['registration'][kind] = rec
    os.makedirs(os.path.dirname(PATH), exist_ok=True)
    with open(PATH, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(doc['registration'], indent=1, sort_keys=True))
    print(json.dumps(doc['finite_differences'], indent=1, sort_keys=True))
    print({k: (v['floor'], max(v['adjoint']['uniform']['floor']), max(v['adjoint']['variance']['floor'])) for k, v in doc['similarity'].items()})
