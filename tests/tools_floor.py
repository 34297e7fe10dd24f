"""What float32 can do on the tool test cases: per case the largest |float32 model - float64 model| of sum mu len and of
tool_len, over every view and every pixel.  Both sides are the numpy model of tests/tools_ref.py, never the kernel: the
float32 side carries out the kernel's stated arithmetic step for step.  Run offline on the CPU; the result is committed
as tests/golden/floors/tools.json, and tests/test_gpu_tools.py allows the kernel 8 x these floors against the float64
model (the margin of DESIGN.md sections 15-17: another legitimate order inside a dot product, sqrtf and division within an
ulp).  A floor of 0 asks for equality.  A floor above 0.1 mm would mean the formulation is the naive one
(tests/test_tools_cpu.py holds every floor below that).

    python tests/tools_floor.py            # rewrites tests/golden/floors/tools.json
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tools_ref as T  # noqa: E402

PATH = os.path.join(HERE, 'golden', 'floors', 'tools.json')
BAR_FACTOR = 8.0


def measure():
    out = {}
    for name in T.cases():
        s64, l64 = T.model(name, np.float64)
        s32, l32 = T.model(name, np.float32)
        out[name] = {'att': float(np.abs(s32.astype(np.float64) - s64).max()),
                     'tool_len': float(np.abs(l32.astype(np.float64) - l64).max()),
                     'largest_att': float(s64.max()), 'largest_tool_len': float(l64.max())}
    return out


def load():
    with open(PATH) as f:
        return json.load(f)


def bar(name, what):
    """BAR_FACTOR x the committed floor of the case; what = 'att' or 'tool_len'."""
    return BAR_FACTOR * load()['floors'][name][what]


if __name__ == '__main__':
    doc = {'what': 'largest |float32 model - float64 model| (tests/tools_ref.py) of sum mu len (att) and of tool_len (mm) per '
                   'case, over every view and pixel', 'tool': 'python tests/tools_floor.py', 'numpy': np.__version__,
           'bar_factor': BAR_FACTOR, 'floors': measure()}
    os.makedirs(os.path.dirname(PATH), exist_ok=True)
    with open(PATH, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(doc, indent=1, sort_keys=True))
