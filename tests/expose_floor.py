"""What fp32 can do on the detector-model test inputs: the largest |float32 model - float64 model| of the intensities
per case (input, blur sigma, noise on / off), over the three views.  Both sides are the numpy model of
tests/expose_ref.py, never the kernel; the normals are those of tests/aug_ref.py under the test's keys.  Run offline on
the CPU; the result is committed as tests/golden/floors/expose.json, and tests/test_gpu_expose.py allows the kernel's
float32 output 8 x these floors (the margin covers FMA contraction, a different but legitimate summation order and an
expf within a couple of ulp).  A floor of 0 asks for equality.

    python tests/expose_floor.py            # rewrites tests/golden/floors/expose.json
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import aug_ref as A  # noqa: E402
import expose_ref as X  # noqa: E402

PATH = os.path.join(HERE, 'golden', 'floors', 'expose.json')
BAR_FACTOR = 8.0


def normals(shape):
    """(z1, z2) float32 [3, R, C] under X.KEYS."""
    n = shape[1] * shape[2]
    z1 = np.stack([A.normals(kq, np.arange(n)).reshape(shape[1:]) for kq, _ in X.KEYS])
    z2 = np.stack([A.normals(ke, np.arange(n)).reshape(shape[1:]) for _, ke in X.KEYS])
    return z1.astype(np.float32), z2.astype(np.float32)


def measure():
    out = {}
    for name, sigma, noise in X.CASES:
        att = X.inputs(name)
        w, _ = X.taps(sigma)
        z1, z2 = normals(att.shape) if noise else (None, None)
        i64 = X.expose(att, w, z1=z1, z2=z2, dtype=np.float64, **X.PARAMS)
        i32 = X.expose(att, w, z1=z1, z2=z2, dtype=np.float32, **X.PARAMS)
        out[X.case_key(name, sigma, noise)] = {'intensity': float(np.abs(i32.astype(np.float64) - i64).max()),
                                               'largest_value': float(np.abs(i64).max())}
    return out


def load():
    with open(PATH) as f:
        return json.load(f)


def bar(name, sigma, noise):
    """BAR_FACTOR x the committed floor of the case."""
    return BAR_FACTOR * load()['floors'][X.case_key(name, sigma, noise)]['intensity']


if __name__ == '__main__':
    doc = {'what': 'largest |float32 model - float64 model| (tests/expose_ref.py) of the detector intensities per input, blur '
                   'sigma and noise on / off, over three views; photons %g, gain %g, electronic sigma %g'
                   % (X.PARAMS['photons'], X.PARAMS['gain'], X.PARAMS['electronic_sigma']),
           'tool': 'python tests/expose_floor.py', 'numpy': np.__version__, 'bar_factor': BAR_FACTOR, 'floors': measure()}
    os.makedirs(os.path.dirname(PATH), exist_ok=True)
    with open(PATH, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(doc, indent=1, sort_keys=True))
