"""Timing of two builds of libdfl_hip.so from alternating runs of `python bench.py --full --no-cpu-baseline --no-configs3` in one GPU call:

    python docs/experiments/convs_unified/timing_table.py DIR      # DIR holds bench_parent_<i>.json and bench_new_<i>.json

One row per key: the parent's runs, their min - max range, the new library's runs and median, and whether the median lies within the
parent's range or is faster (every key is a time, except `value`, the headline's images per second, where higher is better)."""
import glob
import json
import os
import statistics
import sys


def last_json(path):
    for line in reversed(open(path).read().splitlines()):
        line = line.strip()
        if line.startswith('{'):
            return json.loads(line)
    raise SystemExit('no JSON line in ' + path)


def find(d, key):
    """First value under `key` anywhere in the result (the forward timings sit in a nested table)."""
    if isinstance(d, dict):
        if key in d:
            return d[key]
        for v in d.values():
            r = find(v, key)
            if r is not None:
                return r
    return None


def rows(r):
    fwd = find(r, 'fwd_ms_per_img') or {}
    out = {'value (headline, higher is better)': r.get('value')}
    out['fwd_ms_per_img.192x192_batch1'] = fwd.get('192x192_batch1')
    lat = fwd.get('192x192_batch1_latency') or {}
    out['192x192_batch1_latency.ms_per_img'] = lat.get('ms_per_img')
    par = fwd.get('192x192_batch1_parity_modes') or {}
    for m in ('fp32', 'bf16x3'):
        v = par.get(m)
        out['192x192_batch1_parity_modes.' + m] = v.get('ms_per_img') if isinstance(v, dict) else v
    for k in sorted(fwd):
        if 'ensemble' in k:
            out[k] = fwd[k]
    return {k: v for k, v in out.items() if isinstance(v, (int, float))}


def main():
    d = sys.argv[1]
    runs = {w: [rows(last_json(p)) for p in sorted(glob.glob(os.path.join(d, 'bench_%s_*.json' % w)))] for w in ('parent', 'new')}
    print('%d parent runs, %d new runs, alternating (parent first)' % (len(runs['parent']), len(runs['new'])))
    bad = 0
    for k in runs['parent'][0]:
        p = [r[k] for r in runs['parent'] if k in r]
        n = [r[k] for r in runs['new'] if k in r]
        med = statistics.median(n)
        higher = k.startswith('value')
        ok = (med >= min(p)) if higher else (med <= max(p))
        bad += 0 if ok else 1
        print('%-42s parent %s  range %.4f - %.4f | new %s  median %.4f  %s' % (
            k, ' '.join('%.4f' % v for v in p), min(p), max(p), ' '.join('%.4f' % v for v in n), med,
            'within the range or faster' if ok else 'OUTSIDE the range'))
    print('RESULT: %s' % ('every key within the parent\'s range or faster' if bad == 0 else '%d keys outside the parent\'s range' % bad))


if __name__ == '__main__':
    main()
