#!/usr/bin/env python3
"""The table of parent and new times from three rounds each of tools/bench_overlay.py (its JSON line kept as
DIR/bench_overlay_{parent,new}_{1,2,3}.json) and tools/bench_fullres_overlay.py (--out DIR/bench_fullres_{parent,new}_{1,2,3}.json),
run alternately, each run its own process:
    python speed_table.py DIR
Per entry and tree: the median of the three runs and their spread max - min.  The bar:  new median <= parent median * 1.01 +
the larger of the two spreads.  Exit status 1 if an entry misses it."""
import json
import statistics
import sys

d = sys.argv[1]


def load(tool, tree):
    return [json.load(open('%s/bench_%s_%s_%d.json' % (d, tool, tree, k))) for k in (1, 2, 3)]


def entry(runs, path):
    v = []
    for r in runs:
        for p in path:
            r = r[p]
        v.append(r)
    return statistics.median(v), max(v) - min(v)


rows = []
ovl = {t: load('overlay', t) for t in ('parent', 'new')}
for case in ovl['new'][0]:
    rows.append(('render %s, ms per call' % case,) + entry(ovl['parent'], [case, 'ms']) + entry(ovl['new'], [case, 'ms']))
fr = {t: load('fullres', t) for t in ('parent', 'new')}
for case, res in fr['new'][0]['cases'].items():
    rows.append(('%s, ms per call' % case,) + entry(fr['parent'], ['cases', case, 'ms_per_call']) + entry(fr['new'], ['cases', case, 'ms_per_call']))
    for kern in res['kernels']:
        path = ['cases', case, 'kernels', kern, 'mean_us']
        rows.append(('%s `%s`, mean µs' % (case, kern),) + entry(fr['parent'], path) + entry(fr['new'], path))
bad = 0
print('| entry | parent median | parent spread | new median | new spread | limit | |\n|---|---|---|---|---|---|---|')
for name, pm, ps, nm, ns in rows:
    limit = pm * 1.01 + max(ps, ns)
    bad += nm > limit
    print('| %s | %.4f | %.4f | %.4f | %.4f | %.4f | %s |' % (name, pm, ps, nm, ns, limit, 'ok' if nm <= limit else 'SLOWER'))
sys.exit(1 if bad else 0)
