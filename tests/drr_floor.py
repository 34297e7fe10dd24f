"""What fp32 can do on the DRR test scenes: the largest |float32 model - float64 model| of att and of plen, for both
scenes and both interpolations, over the two views and the tight boxes the GPU test renders.  Both sides are the numpy
model of tests/drr_ref.py, never the kernel.  Run offline on the CPU; the result is committed as
tests/golden/floors/drr.json, and tests/test_gpu_drr.py allows the kernel 8 x these floors (the margin covers FMA
contraction and a different but legitimate summation order).

Trilinear: a ray whose s (t1 - t0) / step lies within 1e-4 of an integer in the float64 model is left out on both
sides, as in the GPU test: its sample count may differ by one between two precisions.

    python tests/drr_floor.py            # rewrites tests/golden/floors/drr.json
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import drr_ref as D  # noqa: E402

PATH = os.path.join(HERE, 'golden', 'floors', 'drr.json')
BAR_FACTOR = 8.0


def measure():
    out = {}
    for kind in ('tilted', 'aligned'):
        for interp in ('exact', 'trilinear'):
            att = plen = 0.0
            top_att = top_plen = 0.0
            for view in (0, 1):
                a64, p64, frac, _ = D.model(kind, interp, view)
                a32, p32, _, _ = D.model(kind, interp, view, dtype=np.float32)
                keep = ~D.near_integer(frac) if interp == 'trilinear' else np.ones(a64.shape, bool)
                att = max(att, float(np.abs(a32.astype(np.float64) - a64)[keep].max()))
                plen = max(plen, float(np.abs(p32.astype(np.float64) - p64).max()))
                top_att, top_plen = max(top_att, float(a64.max())), max(top_plen, float(p64.max()))
            out['%s/%s' % (kind, interp)] = {'att': att, 'att_largest_value': top_att}
            if interp == 'exact':
                out['%s/%s' % (kind, interp)].update({'plen_mm': plen, 'plen_largest_value_mm': top_plen})
    return out


def load():
    with open(PATH) as f:
        return json.load(f)


def bars(kind, interp):
    """(att bar, plen bar in mm or None): BAR_FACTOR x the committed floors."""
    e = load()['floors'][kind + '/' + interp]
    return BAR_FACTOR * e['att'], BAR_FACTOR * e['plen_mm'] if 'plen_mm' in e else None


if __name__ == '__main__':
    doc = {'what': 'largest |float32 model - float64 model| (tests/drr_ref.py) per scene and interpolation, over views 0 and 1 '
                   'with tight boxes; att in line-integral units, plen in mm',
           'tool': 'python tests/drr_floor.py', 'numpy': np.__version__, 'bar_factor': BAR_FACTOR, 'floors': measure()}
    os.makedirs(os.path.dirname(PATH), exist_ok=True)
    with open(PATH, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(doc, indent=1, sort_keys=True))
