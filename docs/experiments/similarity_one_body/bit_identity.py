#!/usr/bin/env python3
"""Did the one similarity body, the one driver and the shared kernel bodies (csrc/sim.h) move a bit?

Three parts, each its own process, every output and every scratch buffer kept:
  abi     the calls of docs/experiments/patch_adjoint/bit_identity.py (that script, unchanged, through runpy; it chains the
          earlier ones), then dfl_sim_patch_weights and dfl_sim_patch_eval on the inputs of tests/test_gpu_register_wpatch.py:
          weighted without and with d_moving and uniform with d_moving, against a bank (F = 3; 2 at 19 x 1538; V = 7) and
          against its image 0 alone (fixed_of NULL).  DFL_LIB_OVERRIDE names the library, as in those scripts.
  python  register() -- global, uniform patch, weighted patch with refine=3, the two levels [(2, 6), (1, 6)], a landmark term
          with refine -- and register_many() with N = 3 in two chunks and in one, on the tests' 45 x 61 scenes with popsize 16
          and 8 generations.  --tree names the checkout whose package is imported (default: this one); every field of the
          tests' FIELDS plus levels and delta is kept.
  --inputs writes what both read with the numpy models alone (no GPU); --compare holds two runs against each other.

  python docs/experiments/similarity_one_body/bit_identity.py --inputs inputs.npz
  DFL_LIB_OVERRIDE=<parent library> python .../bit_identity.py abi inputs.npz parent.npz
  python .../bit_identity.py abi inputs.npz new.npz
  python .../bit_identity.py python inputs.npz parent.py.npz --tree <parent checkout>
  python .../bit_identity.py python inputs.npz new.py.npz
  python .../bit_identity.py --compare parent.npz new.npz         (also holds parent.py.npz against new.py.npz)
"""
import os
import runpy
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
CHAINED = os.path.join(ROOT, 'docs', 'experiments', 'patch_adjoint', 'bit_identity.py')
FIXED_OF = [2, 0, 1, 1, 0, 2, 0]
EVAL_CASES = ((45, 61, 3, 2, 3), (17, 70, 1, 4, 3), (9, 300, 1, 1, 3), (19, 1538, 3, 2, 2))
FIELDS = ('theta', 'cost', 'theta_cma', 'refine_cost', 'final_cost', 'similarity_cost', 'landmark_cost', 'pose', 'renders',
          'gradient_evaluations', 'levels', 'delta')
TRUE, START = (0.0, 0.25, -0.15), (0.3, 0.2, 0.1)                 # tests/test_gpu_register_many.py


def beside(path, tag):
    return (path[:-4] if path.endswith('.npz') else path) + '.%s.npz' % tag


def chained(argv):
    """patch_adjoint/bit_identity.py with this command line; its sys.exit comes back as a status."""
    old = sys.argv
    sys.argv = [CHAINED] + list(argv)
    try:
        runpy.run_path(CHAINED, run_name='__main__')
        return 0
    except SystemExit as e:
        return int(e.code or 0)
    finally:
        sys.argv = old


def differing(path_a, path_b, what):
    a, b = np.load(path_a), np.load(path_b)
    assert sorted(a.files) == sorted(b.files), 'the two runs hold different arrays'
    diff = [k for k in sorted(a.files) if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
    print('%s: %d arrays of %d calls, %d differ' % (what, len(a.files), len({k.rsplit('/', 1)[0] for k in a.files}), len(diff)))
    for k in diff:
        print('  DIFFERS %s' % k)
    return len(diff)


def write_inputs(path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
    status = chained(['--inputs', path])
    import drr_ref as D
    import reg_floor as FL
    import reg_ref as R
    S = D.scene('tilted')
    ctr = R.volume_centre(S)
    from dfl_amd import register as reg                            # host numpy alone: pose_delta
    moved = [[reg.pose_delta(t * np.array(R.THETA_FEMUR), ctr) @ P for P in S['poses']] for t in TRUE]
    fixed_many = np.stack([R.render_poses(S, poses, 'trilinear', 1.0).astype(np.float32) for poses in moved])
    arrays = dict(fixed=FL.fixed_image(S).astype(np.float32), fixed_many=fixed_many, poses_many=np.array(moved), centre=ctr,
                  centres_phys=R.centres_phys(S))
    np.savez(beside(path, 'scene'), **arrays)
    print('%d scene arrays -> %s' % (len(arrays), beside(path, 'scene')))
    return status


def run_abi(inputs, out_path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
    chained([inputs, out_path])                                   # imports dfl_amd from this tree; the library is DFL_LIB_OVERRIDE's
    import torch
    from dfl_amd import _native as nat
    inp = dict(np.load(inputs))
    inp.update(np.load(beside(inputs, 'banks')))
    lib, st, out = nat.lib(), torch.cuda.current_stream().cuda_stream, {}

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def filled(shape, dtype):
        return torch.full(shape, float('nan') if dtype.is_floating_point else 0x2B, dtype=dtype, device='cuda')

    def keep(tag, **tensors):
        torch.cuda.synchronize()
        for name, t in tensors.items():
            out['%s/%s' % (tag, name)] = t.cpu().numpy()

    for H, W, rho, stride, F in EVAL_CASES:
        pre = 'sim' if 'sim/%dx%d/fixed' % (H, W) in inp else 'bank'
        fixed, moving = inp['%s/%dx%d/fixed' % (pre, H, W)], inp['%s/%dx%d/moving' % (pre, H, W)]
        images = dev(np.stack([fixed, moving[5], moving[4]][:F]))
        masks = dev(np.stack([np.full((H, W), 255, np.uint8), inp['%s/%dx%d/mask/ragged' % (pre, H, W)], inp['%s/%dx%d/mask/empty' % (pre, H, W)]][:F]))
        views = dev(np.concatenate([moving, fixed[None]]))
        of = dev(np.array([g % F for g in FIXED_OF], np.int32))
        P = int(lib.dfl_sim_patch_count(H, W, rho, stride))
        fx, fy, counted = filled((F, H, W), torch.float32), filled((F, H, W), torch.float32), filled((F, H, W), torch.uint8)
        totals, ptotals = filled((F, nat.SIM_TOTALS), torch.float64), filled((F, P, nat.SIM_TOTALS), torch.float64)
        pflags, pcount = filled((F, P), torch.uint8), filled((F, 2), torch.int32)
        pweights, pwsum = filled((F, P, 2), torch.float64), filled((F, 2), torch.float64)
        for f in range(F):
            nat.call('dfl_sim_prepare', nat.SimPrepareArgs(fixed=images[f].data_ptr(), mask=masks[f].data_ptr(), fx=fx[f].data_ptr(), fy=fy[f].data_ptr(),
                                                           counted=counted[f].data_ptr(), totals=totals[f].data_ptr(), H=H, W=W), st)
            nat.call('dfl_sim_patch_prepare', nat.SimPatchPrepareArgs(fx=fx[f].data_ptr(), fy=fy[f].data_ptr(), counted=counted[f].data_ptr(),
                                                                      ptotals=ptotals[f].data_ptr(), pflags=pflags[f].data_ptr(),
                                                                      pcount=pcount[f].data_ptr(), H=H, W=W, rho=rho, stride=stride, min_count=1), st)
            nat.call('dfl_sim_patch_weights', nat.SimPatchWeightsArgs(ptotals=ptotals[f].data_ptr(), pflags=pflags[f].data_ptr(),
                                                                      pweights=pweights[f].data_ptr(), pwsum=pwsum[f].data_ptr(), P=P), st)
        tag = 'eval %dx%d radius %d stride %d' % (H, W, rho, stride)
        keep(tag + ' prepared', ptotals=ptotals, pflags=pflags, pcount=pcount, pweights=pweights, pwsum=pwsum)
        for bank in (True, False):
            for weighted, bwd in ((True, False), (True, True), (False, True)):
                need = nat.check(lib.dfl_sim_patch_eval_scratch_doubles(7, H, W, rho, stride, int(bwd)), 'scratch')
                cost, scratch = filled((7,), torch.float64), filled((need,), torch.float64)
                d_moving = filled((7, H, W), torch.float32) if bwd else None
                a = nat.SimPatchEvalArgs(moving=views.data_ptr(), fx=fx.data_ptr(), fy=fy.data_ptr(), counted=counted.data_ptr(),
                                         ptotals=ptotals.data_ptr(), pflags=pflags.data_ptr(), pcount=pcount.data_ptr(),
                                         pweights=pweights.data_ptr() if weighted else None, pwsum=pwsum.data_ptr() if weighted else None,
                                         fixed_of=of.data_ptr() if bank else None, scratch=scratch.data_ptr(), cost=cost.data_ptr(),
                                         d_moving=nat.ptr(d_moving), scratch_doubles=need, V=7, H=H, W=W, rho=rho, stride=stride, F=F if bank else 1)
                nat.call('dfl_sim_patch_eval', a, st)
                kept = dict(cost=cost, scratch=scratch)
                if bwd:
                    kept['d_moving'] = d_moving
                keep('%s %s %s%s' % (tag, 'bank' if bank else 'alone', 'weighted' if weighted else 'uniform', ' bwd' if bwd else ''), **kept)
    np.savez(beside(out_path, 'eval'), **out)
    print('eval: %d arrays of %d calls -> %s' % (len(out), len({k.rsplit('/', 1)[0] for k in out}), beside(out_path, 'eval')))


def run_python(inputs, out_path, tree):
    sys.path[:0] = [tree, os.path.join(tree, 'tests')]
    import torch
    import drr_ref as D
    import reg_ref as R
    from dfl_amd import drr, register as reg
    assert os.path.realpath(reg.__file__).startswith(os.path.realpath(tree)), reg.__file__
    scene = np.load(beside(inputs, 'scene'))
    S = D.scene('tilted')

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def geom(poses):
        named = dict(zip(drr.POSES, poses))
        return drr.Geometry(S['K'], S['E'], named, S['I2P'], np.eye(3), drr.default_objects(S['E'], named, S['I2P']), drr.Grid(S['Q'], S['rows'], S['cols']))

    vol = drr.Volume(dev(S['mu']), dev(S['lab']))
    fixed, raw = dev(scene['fixed']), dev((1000.0 * np.exp(-scene['fixed'].astype(np.float64))).astype(np.float32))
    g, X = geom(S['poses']), scene['centres_phys']
    lands = (X, drr.project_points(g, X) + R.LAND_OFFSETS)
    kw = dict(theta0=R.THETA_START, popsize=16, generations=8, seed=0)
    out = {}

    def keep(tag, res):
        for name in FIELDS:
            out['%s/%s' % (tag, name)] = np.array([[-1 if v is None else v for v in level] for level in res.levels], np.int64) if name == 'levels' \
                else np.asarray(getattr(res, name))

    keep('register global', reg.register(vol, g, fixed, **kw))
    keep('register global refine', reg.register(vol, g, fixed, refine=3, **kw))
    keep('register patch uniform', reg.register(vol, g, fixed, similarity='patch', **kw))
    keep('register patch weighted refine', reg.register(vol, g, fixed, similarity='patch', patch_weight='variance', refine=3, **kw))
    keep('register levels', reg.register(vol, g, raw, levels=[(2, 6), (1, 6)], theta0=R.THETA_START, popsize=16, seed=0))
    keep('register levels weighted refine', reg.register(vol, g, raw, levels=[(2, 6), (1, 6)], theta0=R.THETA_START, popsize=16, seed=0,
                                                          similarity='patch', patch_weight='variance', refine=3))
    keep('register landmarks refine', reg.register(vol, g, fixed, landmarks=lands, landmark_weight=0.01, refine=3, **kw))
    geoms = [geom(list(poses)) for poses in scene['poses_many']]
    theta0 = np.array([s * np.array(R.THETA_START) for s in START])
    many = dict(theta0=theta0, popsize=16, generations=8, seed=0)
    for tag, more in (('two chunks', dict(max_views=32)), ('one chunk', dict()), ('two chunks refine', dict(max_views=32, refine=3)),
                      ('one chunk refine', dict(refine=3)), ('one chunk weighted refine', dict(similarity='patch', patch_weight='variance', refine=3))):
        for i, res in enumerate(reg.register_many(vol, geoms, dev(scene['fixed_many']), **dict(many, **more))):
            keep('register_many %s problem %d' % (tag, i), res)
    np.savez(out_path, **out)
    print('python: %d arrays of %d calls -> %s (package of %s)' % (len(out), len({k.rsplit('/', 1)[0] for k in out}), out_path, tree))


if __name__ == '__main__':
    if sys.argv[1] == '--inputs':
        sys.exit(write_inputs(sys.argv[2]))
    if sys.argv[1] == '--compare':
        a, b = sys.argv[2], sys.argv[3]
        status = chained(['--compare', a, b])
        bad = differing(beside(a, 'eval'), beside(b, 'eval'), 'eval') + differing(beside(a, 'py'), beside(b, 'py'), 'python')
        sys.exit(1 if bad or status else 0)
    if sys.argv[1] == 'abi':
        run_abi(sys.argv[2], sys.argv[3])
    elif sys.argv[1] == 'python':
        run_python(sys.argv[2], sys.argv[3], os.path.abspath(sys.argv[5]) if len(sys.argv) > 5 and sys.argv[4] == '--tree' else ROOT)
    else:
        sys.exit(__doc__)
