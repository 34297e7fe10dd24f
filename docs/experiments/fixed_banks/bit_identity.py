#!/usr/bin/env python3
"""Did giving the similarity kernels a per-view fixed image move a bit of the existing entry points?

The calls, the inputs and the comparison are docs/experiments/registration_shared/bit_identity.py's: dfl_drr_render,
dfl_drr_pose_grad, dfl_sim_prepare, dfl_sim_gradncc, dfl_sim_gradncc_bwd, dfl_sim_patch_prepare and dfl_sim_patch_gradncc
on the tests' own inputs, every output and every scratch buffer kept.  This script only makes that one run on a library
built from the parent commit: such a library lacks the three bank entry points and has a shorter dfl_sizeof table, which
_native.lib() refuses, so a library named by DFL_LIB_OVERRIDE is loaded here without those two checks (the structs of
the entry points that are called did not change).

  python docs/experiments/fixed_banks/bit_identity.py --inputs inputs.npz                  (numpy models alone: no GPU)
  DFL_LIB_OVERRIDE=<parent library> python docs/experiments/fixed_banks/bit_identity.py inputs.npz parent.npz
  python docs/experiments/fixed_banks/bit_identity.py inputs.npz new.npz
  python docs/experiments/fixed_banks/bit_identity.py --compare parent.npz new.npz
"""
import ctypes as C
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

if not sys.argv[1].startswith('--') and os.environ.get('DFL_LIB_OVERRIDE'):
    import dfl_amd  # noqa: F401
    from dfl_amd import _native as nat
    L = C.CDLL(nat.LIB_PATH)
    missing = [name for name in nat.EXPORTS if not hasattr(L, name)]
    for name in nat.EXPORTS:
        if name not in missing:
            getattr(L, name).restype, getattr(L, name).argtypes = nat._FUNCTIONS[name]
    print('%s lacks %s' % (nat.LIB_PATH, ', '.join(missing) or 'nothing'))
    nat._lib = L
runpy.run_path(os.path.join(ROOT, 'docs', 'experiments', 'registration_shared', 'bit_identity.py'), run_name='__main__')
