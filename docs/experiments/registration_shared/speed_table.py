#!/usr/bin/env python3
"""The table of parent and new times from two rounds each of tools/bench_register.py and tools/bench_drr.py, run alternately in
one call with --out DIR/bench_{register,drr}_{parent,new}_{1,2}.json:
    python speed_table.py DIR
Per entry and tree: the median of the pooled round medians and the spread max - min over both rounds' windows (for the one
wall-clock figure, which has no windows, the distance of the two rounds).  The bar is the rule of bench_register.py's
patch_generation_check:  new <= parent * 1.01 + the larger of the two spreads.  Exit status 1 if an entry misses it."""
import json
import statistics
import sys

d = sys.argv[1]


def load(tool, tree):
    return [json.load(open('%s/bench_%s_%s_%d.json' % (d, tool, tree, k))) for k in (1, 2)]


def windows(runs, path, ms='ms', lo='min_ms', hi='max_ms'):
    e = []
    for r in runs:
        for p in path:
            r = r[p]
        e.append(r)
    if not isinstance(e[0], dict):
        return statistics.median(e), max(e) - min(e)
    return statistics.median(x[ms] for x in e), max(x[hi] for x in e) - min(x[lo] for x in e)


rows = []
reg = {t: load('register', t) for t in ('parent', 'new')}
for path in (['render'], ['similarity'], ['similarity_patch'], ['generation'], ['generation_patch'], ['gradient_one_view', 'render'],
             ['gradient_one_view', 'adjoint'], ['gradient_one_view', 'pose_gradient'], ['gradient_one_view', 'cost_and_gradient_wall_ms']):
    rows.append(('register ' + '.'.join(path),) + windows(reg['parent'], path) + windows(reg['new'], path))
drr = {t: load('drr', t) for t in ('parent', 'new')}
for case in drr['new'][0]['cases']:
    for mapping in ('tile8x8', 'row64x1'):
        path = ['cases', case, mapping]
        keys = ('ms_per_view', 'min_ms_per_view', 'max_ms_per_view')
        rows.append(('drr %s %s' % (case, mapping),) + windows(drr['parent'], path, *keys) + windows(drr['new'], path, *keys))
bad = 0
print('| entry (ms) | parent median | parent spread | new median | new spread | limit | |\n|---|---|---|---|---|---|---|')
for name, pm, ps, nm, ns in rows:
    limit = pm * 1.01 + max(ps, ns)
    bad += nm > limit
    print('| %s | %.4f | %.4f | %.4f | %.4f | %.4f | %s |' % (name, pm, ps, nm, ns, limit, 'ok' if nm <= limit else 'SLOWER'))
sys.exit(1 if bad else 0)
