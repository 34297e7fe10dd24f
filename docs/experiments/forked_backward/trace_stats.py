"""Per-step kernel time and busy time from a rocprofv3 kernel-trace CSV.  python trace_stats.py <dir> <bench json line file> <out json>"""
import csv, glob, json, re, sys
from collections import Counter, defaultdict
d, line_file, out = sys.argv[1:4]
files = glob.glob(d + '/**/*kernel_trace.csv', recursive=True)
assert files, 'no kernel trace under ' + d
rows = []
for f in files:
    with open(f) as fh:
        rd = csv.DictReader(fh)
        cols = rd.fieldnames
        cs = [c for c in cols if 'start' in c.lower()][0]
        ce = [c for c in cols if 'end' in c.lower()][0]
        cn = [c for c in cols if 'kernel_name' in c.lower()][0]
        cq = [c for c in cols if 'queue' in c.lower()]
        for r in rd:
            rows.append((int(r[cs]), int(r[ce]), r[cn], r[cq[0]] if cq else ''))
rows.sort()
def short(n):
    n = re.sub(r'^void ', '', n)
    n = re.sub(r'\(.*$', '', n)
    n = re.sub(r'^dfl::', '', n)
    return n[:60]
bench = json.loads([l for l in open(line_file) if l.startswith('{')][-1])
steps, total = bench['steps'], bench['prewarm_steps'] + bench['warmup'] + bench['steps']
cnt = Counter(short(r[2]) for r in rows)
marks = [n for n, c in cnt.items() if c == total]
res = dict(files=len(files), kernels=len(rows), steps_total=total, ms_per_step_reported=bench['ms_per_step'], markers=marks[:4])
if marks:
    m = marks[0]
    at = [r[0] for r in rows if short(r[2]) == m]
    t0, t1 = at[-steps - 1], at[-1]
    sel = [r for r in rows if t0 <= r[0] < t1]
    nst = steps
else:
    sel, nst, t0, t1 = rows, total, rows[0][0], rows[-1][1]
ksum = sum(e - s for s, e, _, _ in sel)
busy, cur_s, cur_e = 0, None, None
for s, e, _, _ in sel:
    if cur_e is None or s > cur_e:
        if cur_e is not None:
            busy += cur_e - cur_s
        cur_s, cur_e = s, e
    else:
        cur_e = max(cur_e, e)
busy += (cur_e - cur_s) if cur_e is not None else 0
ov = defaultdict(int)
active = []
for s, e, n, q in sel:
    active = [a for a in active if a[1] > s]
    for a in active:
        o = min(e, a[1]) - s
        if o > 0:
            ov[tuple(sorted((short(n), short(a[2]))))] += o
    active.append((s, e, n))
fam = defaultdict(lambda: [0, 0])
for s, e, n, _ in sel:
    fam[short(n)][0] += e - s
    fam[short(n)][1] += 1
res.update(steps_measured=nst, wall_ms_per_step=(t1 - t0) / nst / 1e6, kernel_sum_ms_per_step=ksum / nst / 1e6, busy_ms_per_step=busy / nst / 1e6,
           launches_per_step=len(sel) / nst, queues=sorted(set(r[3] for r in sel)),
           overlap_us_per_step={' | '.join(k): round(v / nst / 1e3, 1) for k, v in sorted(ov.items(), key=lambda kv: -kv[1])[:16]},
           family_us_per_step={k: [round(v[0] / nst / 1e3, 1), round(v[1] / nst, 1)] for k, v in sorted(fam.items(), key=lambda kv: -kv[1][0])[:14]})
json.dump(res, open(out, 'w'), indent=1)
print(json.dumps({k: res[k] for k in ('wall_ms_per_step', 'kernel_sum_ms_per_step', 'busy_ms_per_step', 'launches_per_step', 'queues', 'markers')}))
