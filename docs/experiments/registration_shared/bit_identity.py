#!/usr/bin/env python3
"""Every C entry point of the registration stack on the tests' own seeded inputs; every output goes to an .npz file.  Run once
per library in separate processes and compare byte for byte:
  python docs/experiments/registration_shared/bit_identity.py --inputs inputs.npz          (the numpy models alone: no GPU)
  DFL_LIB_OVERRIDE=<parent library> python docs/experiments/registration_shared/bit_identity.py inputs.npz parent.npz
  python docs/experiments/registration_shared/bit_identity.py inputs.npz new.npz
  python docs/experiments/registration_shared/bit_identity.py --compare parent.npz new.npz
The calls go through dfl_amd._native alone (the ctypes binding), so the run does not depend on which tree's Python
packs records or owns buffers.
  dfl_drr_render      both views of the 'tilted' and 'aligned' scenes of tests/drr_ref.py in one call, tight and full boxes: exact with
                      plen and label_map under both mappings, trilinear with steps 0.5 and 1.0
  dfl_sim_prepare, dfl_sim_gradncc, dfl_sim_gradncc_bwd
                      every size and mask of reg_ref.SIM_SIZES / sim_masks, the six images of reg_ref.sim_images
  dfl_sim_patch_prepare, dfl_sim_patch_gradncc
                      every case of patch_ref.cases() with every mask, min_count 1 and the default
  dfl_drr_pose_grad   the sixteen MOMENT_CASES of tests/grad_floor.py"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

if sys.argv[1] == '--compare':
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    assert sorted(a.files) == sorted(b.files), 'the two runs hold different arrays'
    diff = [k for k in sorted(a.files) if a[k].tobytes() != b[k].tobytes()]
    print('%d arrays of %d calls, %d differ' % (len(a.files), len({k.rsplit('/', 1)[0] for k in a.files}), len(diff)))
    for k in diff:
        x, y = a[k].astype(np.float64), b[k].astype(np.float64)
        print('  DIFFERS %s: largest difference %.3e (largest magnitude %.3e)' % (k, np.nanmax(np.abs(x - y)), np.nanmax(np.abs(x))))
    sys.exit(1 if diff else 0)

if sys.argv[1] == '--inputs':
    import drr_ref as D
    import grad_floor as GF
    import patch_ref as PT
    import reg_ref as R
    inp = {}
    for kind in ('tilted', 'aligned'):
        S = D.scene(kind)
        inp.update({kind + '/mu': S['mu'], kind + '/lab': S['lab'], kind + '/q': S['Q'].astype(np.float32).reshape(-1)})
        for interp in ('exact', 'trilinear'):
            for tight in (True, False):
                inp['%s/recs/%s/%s' % (kind, interp, 'tight' if tight else 'full')] = np.stack(
                    [D.pack(c2is, D.MASKS, S['Q'], S['lab'], tight, interp) for c2is in D.scene_views(S)]).view(np.uint8)
    for H, W in sorted(set(R.SIM_SIZES) | set(PT.SIZES)):
        fixed, moving = R.sim_images(H, W)
        inp.update({'sim/%dx%d/fixed' % (H, W): fixed, 'sim/%dx%d/moving' % (H, W): moving})
        for name, mask in R.sim_masks(H, W).items():
            if mask is not None:
                inp['sim/%dx%d/mask/%s' % (H, W, name)] = mask
    for case in GF.MOMENT_CASES:
        recs, d_att, _, piv = GF.moment_inputs(*case)
        key = 'moment/' + GF.moment_key(*case)
        inp.update({key + '/recs': recs[None].view(np.uint8), key + '/d_att': d_att[None], key + '/pivots': piv[None].astype(np.float32)})
    np.savez(sys.argv[2], **inp)
    print('%d input arrays -> %s' % (len(inp), sys.argv[2]))
    sys.exit(0)

import torch  # noqa: E402

import grad_floor as GF  # noqa: E402
import patch_ref as PT  # noqa: E402
import reg_ref as R  # noqa: E402
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat  # noqa: E402

inp = np.load(sys.argv[1])
lib = nat.lib()
st = torch.cuda.current_stream().cuda_stream
out = {}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nan(shape, dtype=torch.float32):
    """An output buffer nobody has written: NaN, or 0xAB bytes for integers."""
    return torch.full(shape, float('nan'), dtype=dtype, device='cuda') if dtype.is_floating_point else torch.full(shape, 0xAB, dtype=dtype, device='cuda')


def keep(tag, **tensors):
    torch.cuda.synchronize()
    for name, t in tensors.items():
        out['%s/%s' % (tag, name)] = t.cpu().numpy()


def scene_fields(kind, recs, H, W, step):
    mu, lab, objs = dev(inp[kind + '/mu']), dev(inp[kind + '/lab']), dev(recs.reshape(-1))
    nz, ny, nx = mu.shape
    V = recs.shape[0]
    return [mu, lab, objs], dict(mu=mu.data_ptr(), labels=lab.data_ptr(), objects=objs.data_ptr(), qscale=(nat.f32 * 9)(*inp[kind + '/q']),
                                 nx=nx, ny=ny, nz=nz, H=H, W=W, views=V, n_obj=recs.size // (V * C.sizeof(nat.DrrObject)), step_mm=step)


H, W, NL = 45, 61, 7
for kind in ('tilted', 'aligned'):
    for boxes in ('tight', 'full'):
        recs = inp['%s/recs/exact/%s' % (kind, boxes)]
        for mapping in (0, 1):
            alive, f = scene_fields(kind, recs, H, W, 0.5)
            att, plen, lab = nan((2, H, W)), nan((2, NL, H, W)), nan((2, H, W), torch.uint8)
            nat.call('dfl_drr_render', nat.DrrArgs(att=att.data_ptr(), plen=plen.data_ptr(), label_map=lab.data_ptr(), n_labels=NL,
                                                   interp=nat.DRR_EXACT, mapping=mapping, min_len_mm=1.0, **f), st)
            keep('render %s %s exact mapping %d' % (kind, boxes, mapping), att=att, plen=plen, label_map=lab)
            if mapping == 0:                                                  # without plen and label_map: the third kernel
                att = nan((2, H, W))
                nat.call('dfl_drr_render', nat.DrrArgs(att=att.data_ptr(), n_labels=NL, interp=nat.DRR_EXACT, min_len_mm=1.0, **f), st)
                keep('render %s %s exact att alone' % (kind, boxes), att=att)
        recs = inp['%s/recs/trilinear/%s' % (kind, boxes)]
        for step in (0.5, 1.0):
            alive, f = scene_fields(kind, recs, H, W, step)
            att = nan((2, H, W))
            nat.call('dfl_drr_render', nat.DrrArgs(att=att.data_ptr(), n_labels=NL, interp=nat.DRR_TRILINEAR, min_len_mm=1.0, **f), st)
            keep('render %s %s trilinear step %.1f' % (kind, boxes, step), att=att)

for case in GF.MOMENT_CASES:
    kind, view, step, pattern = case
    key = 'moment/' + GF.moment_key(*case)
    alive, f = scene_fields(kind, inp[key + '/recs'], H, W, step)
    d_att, piv = dev(inp[key + '/d_att']), dev(inp[key + '/pivots'])
    need = nat.check(lib.dfl_drr_pose_grad_scratch_doubles(1, 3, H, W), 'scratch')
    grad, scratch = nan((1, 3, 12), torch.float64), nan((need,), torch.float64)
    nat.call('dfl_drr_pose_grad', nat.DrrPoseGradArgs(d_att=d_att.data_ptr(), pivots=piv.data_ptr(), grad=grad.data_ptr(),
                                                      scratch=scratch.data_ptr(), scratch_doubles=need, interp=nat.DRR_TRILINEAR, **f), st)
    keep('pose_grad ' + GF.moment_key(*case), grad=grad, scratch=scratch)


def prepared(tag, H, W, name):
    """dfl_sim_prepare of one size and mask -> (the device tensors, the fields the later calls share)"""
    fixed = dev(inp['sim/%dx%d/fixed' % (H, W)])
    mask = dev(inp['sim/%dx%d/mask/%s' % (H, W, name)]) if name != 'none' else None
    fx, fy, counted, totals = nan((H, W)), nan((H, W)), nan((H, W), torch.uint8), nan((nat.SIM_TOTALS,), torch.float64)
    nat.call('dfl_sim_prepare', nat.SimPrepareArgs(fixed=fixed.data_ptr(), mask=nat.ptr(mask), fx=fx.data_ptr(), fy=fy.data_ptr(),
                                                   counted=counted.data_ptr(), totals=totals.data_ptr(), H=H, W=W), st)
    keep(tag, fx=fx, fy=fy, counted=counted, totals=totals)
    return (fx, fy, counted, totals), dict(fx=fx.data_ptr(), fy=fy.data_ptr(), counted=counted.data_ptr(), H=H, W=W)


for H, W in R.SIM_SIZES:
    moving = dev(inp['sim/%dx%d/moving' % (H, W)])
    V = moving.shape[0]
    for name in ('none', 'ragged', 'empty'):
        tag = 'sim %dx%d %s' % (H, W, name)
        (fx, fy, counted, totals), f = prepared(tag + ' prepare', H, W, name)
        need = int(lib.dfl_sim_scratch_doubles(V, H, W))
        cost, scratch = nan((V,), torch.float64), nan((max(need, 1),), torch.float64)
        nat.call('dfl_sim_gradncc', nat.SimGradnccArgs(moving=moving.data_ptr(), totals=totals.data_ptr(), scratch=scratch.data_ptr(),
                                                       cost=cost.data_ptr(), scratch_doubles=scratch.numel(), V=V, **f), st)
        keep(tag + ' gradncc', cost=cost, scratch=scratch[:need])
        need = nat.check(lib.dfl_sim_gradncc_bwd_scratch_doubles(V, H, W), 'scratch')
        cost, scratch, d_moving = nan((V,), torch.float64), nan((need,), torch.float64), nan((V, H, W))
        nat.call('dfl_sim_gradncc_bwd', nat.SimGradnccBwdArgs(moving=moving.data_ptr(), totals=totals.data_ptr(), scratch=scratch.data_ptr(),
                                                              cost=cost.data_ptr(), d_moving=d_moving.data_ptr(), scratch_doubles=need, V=V,
                                                              **f), st)
        keep(tag + ' gradncc_bwd', cost=cost, scratch=scratch, d_moving=d_moving)

for H, W, rho, stride in PT.cases():
    moving = dev(inp['sim/%dx%d/moving' % (H, W)])
    V = moving.shape[0]
    for name in ('none', 'ragged', 'empty'):
        for mc in (1, PT.default_min_count(rho)):
            tag = 'patch %dx%d radius %d stride %d %s min_count %d' % (H, W, rho, stride, name, mc)
            (fx, fy, counted, totals), f = prepared(tag + ' sim_prepare', H, W, name)
            P = int(lib.dfl_sim_patch_count(H, W, rho, stride))
            need = int(lib.dfl_sim_patch_scratch_doubles(V, H, W, rho, stride))
            assert P > 0 and need > 0, (tag, P, need)
            ptotals, pflags, pcount = nan((P, nat.SIM_TOTALS), torch.float64), nan((P,), torch.uint8), nan((2,), torch.int32)
            f.update(ptotals=ptotals.data_ptr(), pflags=pflags.data_ptr(), pcount=pcount.data_ptr(), rho=rho, stride=stride)
            nat.call('dfl_sim_patch_prepare', nat.SimPatchPrepareArgs(min_count=mc, **f), st)
            keep(tag + ' prepare', ptotals=ptotals, pflags=pflags, pcount=pcount)
            cost, scratch = nan((V,), torch.float64), nan((need,), torch.float64)
            nat.call('dfl_sim_patch_gradncc', nat.SimPatchGradnccArgs(moving=moving.data_ptr(), scratch=scratch.data_ptr(), cost=cost.data_ptr(),
                                                                      scratch_doubles=need, V=V, **f), st)
            keep(tag + ' gradncc', cost=cost, scratch=scratch)

np.savez(sys.argv[2], **out)
print('%d arrays of %d calls -> %s (library: %s)' % (len(out), len({k.rsplit('/', 1)[0] for k in out}), sys.argv[2],
                                                    os.environ.get('DFL_LIB_OVERRIDE', "the tree's own")))
