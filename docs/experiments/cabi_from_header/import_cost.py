"""Cost of deriving the binding at import: `import dfl_amd._native` (which imports the package, torch included) in fresh
interpreters under `python -X importtime`, parent tree and this tree alternating.  Two figures per run: the whole import, and
the share of dfl_amd._native with what it imports itself (ctypes; now also _cabi, its regular expressions and the parse).

    git archive <parent> dfl_amd.py deepfluorolabeling-ipcai2020_amd include | tar -x -C /tmp/parent
    python docs/experiments/cabi_from_header/import_cost.py /tmp/parent [runs, default 10]
"""
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def once(cwd):
    """(ms of the whole import, ms of dfl_amd._native inside it)"""
    err = subprocess.run([sys.executable, '-X', 'importtime', '-c', 'import dfl_amd._native'], cwd=cwd, check=True,
                         capture_output=True, text=True).stderr
    cum = {m.group(2): int(m.group(1)) / 1e3 for m in re.finditer(r'\|\s*(\d+) \|\s+(\S+)$', err, re.M)}
    first = re.search(r'\|\s*(\d+) \|\s+dfl_amd\._native$', err, re.M)        # the nested line: the module's own import
    return cum['dfl_amd'], int(first.group(1)) / 1e3


def main():
    parent, runs = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 10
    once(parent), once(ROOT)          # file cache, bytecode
    ms = {'parent': [], 'new': []}
    for _ in range(runs):
        ms['parent'].append(once(parent))
        ms['new'].append(once(ROOT))
    med = {}
    for k, v in ms.items():
        whole, native = [a for a, _ in v], [b for _, b in v]
        med[k] = statistics.median(whole), statistics.median(native)
        print('%-6s import dfl_amd: median %7.1f ms (min %7.1f, max %7.1f)   of it dfl_amd._native: median %5.1f ms (min %5.1f, max %5.1f)   %d runs'
              % (k, med[k][0], min(whole), max(whole), med[k][1], min(native), max(native), len(v)))
    print('allowance: 1 %% of the parent\'s import dfl_amd = %.1f ms; dfl_amd._native: new - parent = %+.1f ms; whole import: new - parent = %+.1f ms'
          % (0.01 * med['parent'][0], med['new'][1] - med['parent'][1], med['new'][0] - med['parent'][0]))


if __name__ == '__main__':
    main()
