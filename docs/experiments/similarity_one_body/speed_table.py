#!/usr/bin/env python3
"""The table of parent and new times from two rounds each of tools/bench_register.py and register_wall.py, run alternately in one
call with --out DIR/bench_register_{parent,new}_{1,2}.json and DIR/register_wall_{parent,new}_{1,2}.json:
    python speed_table.py DIR
Per entry and tree: the median of the two rounds' medians and the spread max - min over both rounds' windows (for a wall-clock
figure without windows, the distance of the two rounds).  The bar is the rule of bench_register.py's patch_generation_check:
new <= parent * 1.01 + the larger of the two spreads.  Exit status 1 if an entry misses it."""
import json
import statistics
import sys

d = sys.argv[1]
ENTRIES = (['render'], ['similarity'], ['similarity_patch'], ['generation'], ['generation_patch'],
           ['gradient_one_view', 'render'], ['gradient_one_view', 'adjoint'], ['gradient_one_view', 'pose_gradient'],
           ['gradient_one_view', 'cost_wall_ms'], ['gradient_one_view', 'cost_and_gradient_wall_ms'],
           ['weighted_patch', 'similarity'], ['weighted_patch', 'adjoint_one_view'],
           ['weighted_patch', 'cost_and_gradient', 'global_wall_ms'], ['weighted_patch', 'cost_and_gradient', 'weighted_patch_wall_ms'],
           ['weighted_patch', 'generation', 'uniform_patch_ms'], ['weighted_patch', 'generation', 'weighted_patch_ms'],
           ['many', 'generation', 'together_ms'], ['many', 'generation', 'one_after_the_other_ms'],
           ['many', 'gradient_round', 'together_ms'], ['many', 'gradient_round', 'one_after_the_other_ms'],
           ['many', 'similarity', 'bank_launch_512_views'], ['many', 'similarity', '16_launches_of_32_views'])


def load(tool, tree):
    return [json.load(open('%s/%s_%s_%d.json' % (d, tool, tree, k))) for k in (1, 2)]


def figure(runs, path):
    """(median, spread) of an entry: a window dict, a number with its *_min_max_ms beside it, or a bare number."""
    med, lo, hi = [], [], []
    for r in runs:
        for p in path[:-1]:
            r = r[p]
        e = r[path[-1]]
        if isinstance(e, dict):
            med.append(e['ms']), lo.append(e['min_ms']), hi.append(e['max_ms'])
        else:
            both = r.get(path[-1].replace('_wall_ms', '_ms').replace('_ms', '_min_max_ms'), [e, e])
            med.append(e), lo.append(both[0]), hi.append(both[1])
    return statistics.median(med), max(hi) - min(lo)


rows = []
reg = {t: load('bench_register', t) for t in ('parent', 'new')}
for path in ENTRIES:
    rows.append(('.'.join(path),) + figure(reg['parent'], path) + figure(reg['new'], path))
wall = {t: load('register_wall', t) for t in ('parent', 'new')}
rows.append(('register(generations=20, refine=3) wall',) + figure([dict(e=w) for w in wall['parent']], ['e']) + figure([dict(e=w) for w in wall['new']], ['e']))
bad = 0
print('| entry (ms) | parent median | parent spread | new median | new spread | limit | |')
print('|---|---|---|---|---|---|---|')
for name, pm, ps, nm, ns in rows:
    limit = pm * 1.01 + max(ps, ns)
    ok = nm <= limit
    bad += not ok
    print('| %s | %.4f | %.4f | %.4f | %.4f | %.4f | %s |' % (name, pm, ps, nm, ns, limit, 'ok' if ok else 'OVER'))
sys.exit(1 if bad else 0)
