#!/usr/bin/env python3
"""Did the optional weights and coefficients of the patch kernels move a bit of the existing entry points?

Two parts, every output and every scratch buffer kept:
  1. the calls of docs/experiments/registration_shared/bit_identity.py (that script, unchanged, through runpy): dfl_drr_render,
     dfl_drr_pose_grad, dfl_sim_prepare, dfl_sim_gradncc, dfl_sim_gradncc_bwd, dfl_sim_patch_prepare, dfl_sim_patch_gradncc;
  2. the three bank entry points on the inputs of tests/test_gpu_register_many.py: dfl_sim_bank_gradncc and
     dfl_sim_bank_gradncc_bwd at reg_ref.SIM_SIZES, dfl_sim_patch_bank_gradncc at that file's four patch cases (19 x 1538
     among them), F = 3 (2 at the widest), V = 7, the masks none / ragged / empty.
A library built from the parent commit lacks the three new entry points and has a shorter dfl_sizeof table, which
_native.lib() refuses, so a library named by DFL_LIB_OVERRIDE is loaded here without those two checks, as
docs/experiments/fixed_banks/bit_identity.py does (the structs of the entry points that are called did not change).

  python docs/experiments/patch_adjoint/bit_identity.py --inputs inputs.npz                (numpy models alone: no GPU)
  DFL_LIB_OVERRIDE=<parent library> python docs/experiments/patch_adjoint/bit_identity.py inputs.npz parent.npz
  python docs/experiments/patch_adjoint/bit_identity.py inputs.npz new.npz
  python docs/experiments/patch_adjoint/bit_identity.py --compare parent.npz new.npz
(parent.npz and new.npz hold part 1; part 2 goes to parent.banks.npz and new.banks.npz next to them.)
"""
import ctypes as C
import os
import runpy
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
SHARED = os.path.join(ROOT, 'docs', 'experiments', 'registration_shared', 'bit_identity.py')
FIXED_OF = [2, 0, 1, 1, 0, 2, 0]
PATCH_CASES = ((45, 61, 3, 2, 3), (45, 61, 1, 1, 3), (9, 300, 3, 2, 3), (19, 1538, 3, 2, 2))


def banks_path(path):
    return path[:-4] + '.banks.npz' if path.endswith('.npz') else path + '.banks.npz'


def part_one(argv):
    """registration_shared/bit_identity.py with this command line; its sys.exit (--inputs, --compare) comes back as a status."""
    old = sys.argv
    sys.argv = [SHARED] + list(argv)
    try:
        runpy.run_path(SHARED, run_name='__main__')
        return 0
    except SystemExit as e:
        return int(e.code or 0)
    finally:
        sys.argv = old


if sys.argv[1] == '--compare':
    status = part_one(sys.argv[1:])
    a, b = np.load(banks_path(sys.argv[2])), np.load(banks_path(sys.argv[3]))
    assert sorted(a.files) == sorted(b.files), 'the two runs hold different arrays'
    diff = [k for k in sorted(a.files) if a[k].tobytes() != b[k].tobytes()]
    print('banks: %d arrays of %d calls, %d differ' % (len(a.files), len({k.rsplit('/', 1)[0] for k in a.files}), len(diff)))
    for k in diff:
        print('  DIFFERS %s' % k)
    sys.exit(1 if diff or status else 0)

if sys.argv[1] == '--inputs':
    status = part_one(sys.argv[1:])
    import reg_ref as R
    extra = {}
    for H, W in sorted({(H, W) for H, W, _, _, _ in PATCH_CASES} - set(R.SIM_SIZES)):
        fixed, moving = R.sim_images(H, W)
        extra.update({'bank/%dx%d/fixed' % (H, W): fixed, 'bank/%dx%d/moving' % (H, W): moving})
        for name, mask in R.sim_masks(H, W).items():
            if mask is not None:
                extra['bank/%dx%d/mask/%s' % (H, W, name)] = mask
    np.savez(banks_path(sys.argv[2]), **extra)
    print('%d more input arrays -> %s' % (len(extra), banks_path(sys.argv[2])))
    sys.exit(status)

import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat  # noqa: E402

if os.environ.get('DFL_LIB_OVERRIDE'):
    L = C.CDLL(nat.LIB_PATH)
    missing = [name for name in nat.EXPORTS if not hasattr(L, name)]
    for name in nat.EXPORTS:
        if name not in missing:
            getattr(L, name).restype, getattr(L, name).argtypes = nat._FUNCTIONS[name]
    print('%s lacks %s' % (nat.LIB_PATH, ', '.join(missing) or 'nothing'))
    nat._lib = L
part_one(sys.argv[1:])

import torch  # noqa: E402

import reg_ref as R  # noqa: E402

inp = dict(np.load(sys.argv[1]))
inp.update(np.load(banks_path(sys.argv[1])))
lib = nat.lib()
st = torch.cuda.current_stream().cuda_stream
out = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nan(shape, dtype=torch.float32):
    return torch.full(shape, float('nan'), dtype=dtype, device='cuda') if dtype.is_floating_point else torch.full(shape, 0xAB, dtype=dtype, device='cuda')


def keep(tag, **tensors):
    torch.cuda.synchronize()
    for name, t in tensors.items():
        out['%s/%s' % (tag, name)] = t.cpu().numpy()


def bank_of(H, W, F):
    """The bank of tests/test_gpu_register_many.py: the fixed image and its two rendered views under the masks none, ragged, empty;
    the six moving images and the fixed image as views.  Prepared image by image with dfl_sim_prepare."""
    pre = 'sim' if 'sim/%dx%d/fixed' % (H, W) in inp else 'bank'
    fixed, moving = inp['%s/%dx%d/fixed' % (pre, H, W)], inp['%s/%dx%d/moving' % (pre, H, W)]
    images = dev(np.stack([fixed, moving[5], moving[4]][:F]))
    masks = dev(np.stack([np.full((H, W), 255, np.uint8), inp['%s/%dx%d/mask/ragged' % (pre, H, W)], inp['%s/%dx%d/mask/empty' % (pre, H, W)]][:F]))
    fx, fy, counted, totals = nan((F, H, W)), nan((F, H, W)), nan((F, H, W), torch.uint8), nan((F, nat.SIM_TOTALS), torch.float64)
    for f in range(F):
        nat.call('dfl_sim_prepare', nat.SimPrepareArgs(fixed=images[f].data_ptr(), mask=masks[f].data_ptr(), fx=fx[f].data_ptr(), fy=fy[f].data_ptr(),
                                                       counted=counted[f].data_ptr(), totals=totals[f].data_ptr(), H=H, W=W), st)
    return dev(np.concatenate([moving, fixed[None]])), (fx, fy, counted, totals), dict(fx=fx.data_ptr(), fy=fy.data_ptr(), counted=counted.data_ptr(),
                                                                                         H=H, W=W, F=F)


for H, W in R.SIM_SIZES:
    moving, (fx, fy, counted, totals), f = bank_of(H, W, 3)
    of = dev(np.array(FIXED_OF, np.int32))
    tag = 'bank %dx%d' % (H, W)
    need = int(lib.dfl_sim_scratch_doubles(7, H, W))
    cost, scratch = nan((7,), torch.float64), nan((max(need, 1),), torch.float64)
    nat.call('dfl_sim_bank_gradncc', nat.SimBankGradnccArgs(moving=moving.data_ptr(), totals=totals.data_ptr(), fixed_of=of.data_ptr(),
                                                            scratch=scratch.data_ptr(), cost=cost.data_ptr(), scratch_doubles=scratch.numel(), V=7, **f), st)
    keep(tag + ' gradncc', cost=cost, scratch=scratch[:need])
    need = nat.check(lib.dfl_sim_gradncc_bwd_scratch_doubles(7, H, W), 'scratch')
    cost, scratch, d_moving = nan((7,), torch.float64), nan((need,), torch.float64), nan((7, H, W))
    nat.call('dfl_sim_bank_gradncc_bwd', nat.SimBankGradnccBwdArgs(moving=moving.data_ptr(), totals=totals.data_ptr(), fixed_of=of.data_ptr(),
                                                                   scratch=scratch.data_ptr(), cost=cost.data_ptr(), d_moving=d_moving.data_ptr(),
                                                                   scratch_doubles=need, V=7, **f), st)
    keep(tag + ' gradncc_bwd', cost=cost, scratch=scratch, d_moving=d_moving)

for H, W, rho, stride, F in PATCH_CASES:
    moving, (fx, fy, counted, totals), f = bank_of(H, W, F)
    of = dev(np.array([g % F for g in FIXED_OF], np.int32))
    mc = 5 if rho == 1 else (2 * rho + 1) ** 2 // 2 + 1
    P = int(lib.dfl_sim_patch_count(H, W, rho, stride))
    need = int(lib.dfl_sim_patch_scratch_doubles(7, H, W, rho, stride))
    ptotals, pflags, pcount = nan((F, P, nat.SIM_TOTALS), torch.float64), nan((F, P), torch.uint8), nan((F, 2), torch.int32)
    for k in range(F):
        nat.call('dfl_sim_patch_prepare', nat.SimPatchPrepareArgs(fx=fx[k].data_ptr(), fy=fy[k].data_ptr(), counted=counted[k].data_ptr(),
                                                                  ptotals=ptotals[k].data_ptr(), pflags=pflags[k].data_ptr(), pcount=pcount[k].data_ptr(),
                                                                  H=H, W=W, rho=rho, stride=stride, min_count=mc), st)
    cost, scratch = nan((7,), torch.float64), nan((need,), torch.float64)
    nat.call('dfl_sim_patch_bank_gradncc', nat.SimPatchBankGradnccArgs(moving=moving.data_ptr(), ptotals=ptotals.data_ptr(), pflags=pflags.data_ptr(),
                                                                       pcount=pcount.data_ptr(), fixed_of=of.data_ptr(), scratch=scratch.data_ptr(),
                                                                       cost=cost.data_ptr(), scratch_doubles=need, V=7, rho=rho, stride=stride, **f), st)
    keep('patch bank %dx%d radius %d stride %d' % (H, W, rho, stride), ptotals=ptotals, pflags=pflags, pcount=pcount, cost=cost, scratch=scratch)

np.savez(banks_path(sys.argv[2]), **out)
print('banks: %d arrays of %d calls -> %s' % (len(out), len({k.rsplit('/', 1)[0] for k in out}), banks_path(sys.argv[2])))
