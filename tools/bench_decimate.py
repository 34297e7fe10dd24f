"""Times dfl_amd.mesh.decimate on tools/bench_mesh.py's synthetic 512^3 volume: decimate(0.25) of the largest smoothed
surface between device events around back-to-back calls (median, min, max), the rounds and the collapses of each, the
first round split into its host part (dfl_mesh_topology, torch.unique / sort / searchsorted, dfl_mesh_csr) and its four
kernel calls, the .glb bytes of the four surfaces and the time of raster.render() on tools/bench_raster.py's scene, both
with and without decimation.  Prints one JSON object; --out also writes it.

The JSON carries, for the first round, the bytes each launch must move at least (`compulsory_bytes`), so that kernel
times from a run of its own under `rocprofv3 --kernel-trace --stats` can be turned into rates; --kernel-stats
RENDER=FILE.csv (repeatable) adds such a run's mesh_* and rs_tris rows under the name RENDER, --from-json takes the timings of an earlier run instead of measuring.

    python tools/bench_decimate.py [--size 512] [--reps 5] [--render both|plain|reduced|none] [--out decimate_bench.json]
    rocprofv3 --kernel-trace --stats -d rp -o s --output-format csv -- python tools/bench_decimate.py --render none
    python tools/bench_decimate.py --from-json decimate_bench.json --kernel-stats none=rp/.../s_kernel_stats.csv --out decimate_bench.json
"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'examples'))
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, gltf, mesh, raster  # noqa: E402

REDUCTION = mesh.REDUCTION


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {'median_ms': float(np.median(ts)), 'min_ms': float(np.min(ts)), 'max_ms': float(np.max(ts))}


def first_round(xs, t, reps):
    """The first round's parts between events, and the bytes its launches must move."""
    V, T = xs.shape[0], t.shape[0]
    s = torch.cuda.current_stream().cuda_stream
    tp = mesh._round_topology(t, V)
    E = tp['edge_u'].numel()
    p = {k: v.data_ptr() for k, v in tp.items()}
    dev = xs.device
    Q = torch.empty((V, 10), dtype=torch.float64, device=dev)
    key, cand = torch.empty(E, dtype=torch.int64, device=dev), torch.empty((E, 3), dtype=torch.float32, device=dev)
    m1, m2 = torch.empty(V, dtype=torch.int64, device=dev), torch.empty(V, dtype=torch.int64, device=dev)
    sel = torch.empty(E, dtype=torch.uint8, device=dev)
    remap, pos_out = torch.empty(V, dtype=torch.int32, device=dev), torch.empty_like(xs)
    tris_out, degen = torch.empty_like(t), torch.empty(T, dtype=torch.uint8, device=dev)
    calls = {
        'dfl_mesh_quadrics': nat.MeshQuadricsArgs(pos=xs.data_ptr(), tris=t.data_ptr(), vt_ptr=p['vt_ptr'], vt_tri=p['vt_tri'],
                                                  Q=Q.data_ptr(), V=V, T=T),
        'dfl_mesh_collapse_keys': nat.MeshCollapseKeysArgs(
            pos=xs.data_ptr(), tris=t.data_ptr(), row_ptr=p['row_ptr'], col=p['col'], use=p['use'], vt_ptr=p['vt_ptr'],
            vt_tri=p['vt_tri'], Q=Q.data_ptr(), edge_u=p['edge_u'], edge_v=p['edge_v'], key=key.data_ptr(), cand=cand.data_ptr(),
            V=V, T=T, E=E),
        'dfl_mesh_collapse_select': nat.MeshCollapseSelectArgs(
            row_ptr=p['row_ptr'], col=p['col'], eid=p['eid'], edge_u=p['edge_u'], edge_v=p['edge_v'], key=key.data_ptr(),
            m1=m1.data_ptr(), m2=m2.data_ptr(), sel=sel.data_ptr(), V=V, E=E)}
    out = {'V': V, 'T': T, 'E': E, 'topology_host_and_csr': events(lambda: mesh._round_topology(t, V), reps)}
    for fn, a in calls.items():
        out[fn] = events(lambda: nat.call(fn, a, s), reps)
    take = sel.clone()
    apply = nat.MeshCollapseApplyArgs(pos=xs.data_ptr(), tris=t.data_ptr(), row_ptr=p['row_ptr'], col=p['col'], eid=p['eid'],
                                      take=take.data_ptr(), cand=cand.data_ptr(), remap=remap.data_ptr(), pos_out=pos_out.data_ptr(),
                                      tris_out=tris_out.data_ptr(), degen=degen.data_ptr(), V=V, T=T, E=E)
    out['dfl_mesh_collapse_apply'] = events(lambda: nat.call('dfl_mesh_collapse_apply', apply, s), reps)

    def compaction():
        keep = remap == torch.arange(V, dtype=torch.int32, device=dev)
        new_id = (torch.cumsum(keep, 0) - 1).to(torch.int32)
        return pos_out[keep].contiguous(), new_id[tris_out[degen == 0].long()].contiguous()
    out['compaction_torch'] = events(compaction, reps)
    out['selected'] = int(sel.sum())
    out['candidates'] = int((key != -1).sum())
    nnz, deg = 2 * E, torch.diff(tp['row_ptr']).long()
    ends = int((deg[tp['edge_u'].long()] + deg[tp['edge_v'].long()]).sum())          # row entries the edge threads walk
    out['compulsory_bytes'] = {
        # per vertex-triangle entry: its id, three indices, three positions; per vertex: two row pointers' worth, Q
        'mesh_quadrics_kernel': 4 * (V + 1) + 3 * T * (4 + 12 + 36) + 80 * V,
        # per edge: its ends, four row pointers, use and col over both rows, two quadrics, two positions, key and cand
        # (the flip loop of the candidates comes on top)
        'mesh_collapse_keys_kernel': E * (8 + 16 + 160 + 24 + 8 + 12) + 8 * ends,
        'mesh_collapse_m1_kernel': 4 * (V + 1) + nnz * (4 + 8) + 8 * V,
        'mesh_collapse_m2_kernel': 4 * (V + 1) + nnz * (4 + 8) + 16 * V,
        'mesh_collapse_flag_kernel': E * (8 + 8 + 16 + 1),
        'mesh_collapse_vertex_kernel': 4 * (V + 1) + nnz * (4 + 1) + V * (12 + 4 + 12),
        'mesh_collapse_tris_kernel': T * (12 + 12 + 12 + 1)}
    return out


def glb_bytes(surfaces):
    sc = gltf.Scene()
    for k, (pos, nrm, tris) in enumerate(surfaces):
        name = 'surface-%d' % k
        sc.node(name, sc.mesh(name, pos.cpu().numpy(), tris.cpu().numpy().astype(np.uint32), sc.material(name, (1.0, 1.0, 1.0)),
                              normals=nrm.cpu().numpy()))
    return len(sc.encode())


def kernel_rows(path):
    out = {}
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            name = row.get('Name', '')
            for tag in ('mesh_quadrics', 'mesh_collapse', 'rs_tris'):
                if tag in name and '_kernel' in name:
                    short = name[name.index(tag):].split('(')[0].split('E2')[0].split('ENS')[0]
                    out[short] = {'calls': int(row['Calls']), 'average_us': float(row['AverageNs']) / 1e3,
                                  'min_us': float(row['MinNs']) / 1e3, 'max_us': float(row['MaxNs']) / 1e3}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--render', default='both', choices=('both', 'plain', 'reduced', 'none'))
    ap.add_argument('--kernel-stats', action='append', default=[], metavar='RENDER=FILE')
    ap.add_argument('--from-json')
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    if a.from_json:
        with open(a.from_json) as f:
            return finish(json.load(f), a)
    if not torch.cuda.is_available():
        raise SystemExit('bench_decimate needs a GPU')
    import bench_mesh as BM
    import bench_raster as BR
    dev = torch.device('cuda:0')
    n = a.size
    vol = torch.from_numpy(BM.blobs(n)).to(dev)
    res = {'size': n, 'reduction': REDUCTION, 'reps': a.reps, 'device': torch.cuda.get_device_name(0)}
    smoothed = [(mesh.smooth(v, t), t) for v, t in mesh.label_surfaces(vol, BM.LABELS)]
    (xs, _), t = max(smoothed, key=lambda s: s[1].shape[0])
    v1, t1, info = mesh.decimate(xs, t, REDUCTION)
    res['largest'] = {'vertices': [int(xs.shape[0]), int(v1.shape[0])], 'triangles': [int(t.shape[0]), int(t1.shape[0])], **info}
    res['largest']['decimate'] = events(lambda: mesh.decimate(xs, t, REDUCTION), a.reps)
    done = [mesh.decimate(xs, t, REDUCTION, max_rounds=k)[2]['collapses'] for k in range(1, info['rounds'] + 1)]
    res['largest']['collapses_per_round'] = [int(d) for d in np.diff([0] + done)]
    res['first_round'] = first_round(xs, t, a.reps)
    fr = res['first_round']
    host = fr['topology_host_and_csr']['median_ms'] + fr['compaction_torch']['median_ms']
    kern = sum(fr[k]['median_ms'] for k in fr if k.startswith('dfl_mesh_'))
    res['first_round']['host_share'] = host / (host + kern)
    plain, reduced = [], []
    for (xs_k, undo), t_k in smoothed:
        pos = mesh.transform(xs_k, undo)
        plain.append((pos, mesh.vertex_normals(pos, t_k), t_k))
        xr, tr, _ = mesh.decimate(xs_k, t_k, REDUCTION)
        pos = mesh.transform(xr, undo)
        reduced.append((pos, mesh.vertex_normals(pos, tr), tr))
    res['glb_bytes'] = {'plain': glb_bytes(plain), 'reduced': glb_bytes(reduced)}
    res['triangles'] = {'plain': [int(s[2].shape[0]) for s in plain], 'reduced': [int(s[2].shape[0]) for s in reduced]}
    if a.render != 'none':
        meshes, view_proj, near = BR.build_scene(n, dev)
        W, H = BR.W, BR.H
        res['render'] = {'image': [W, H], 'ssaa': 1}
        for which, surf in (('plain', plain), ('reduced', reduced)):
            if a.render in ('both', which):
                ms = [raster.Mesh(p, tr, normals=nr, rgb=rgb) for (p, nr, tr), rgb in zip(surf, BR.COLORS)] + meshes[4:]
                T = sum(int(m.tris.shape[0]) for m in ms)
                res['render'][which] = dict(events(lambda: raster.render(ms, view_proj, W, H, ssaa=1, near=near), a.reps),
                                            triangles=T, tris_bytes=48 * T)
    return finish(res, a)


def finish(res, a):
    for item in a.kernel_stats:                          # one profiled run per --render choice: rs_tris rows stay apart
        which, path = item.split('=', 1)
        rows = kernel_rows(path)
        for name, r in rows.items():
            b = res['first_round']['compulsory_bytes'].get(name)
            if b:                                        # the longest launch is the first round's, on the whole mesh
                r['first_round_compulsory_bytes'] = b
                r['first_round_gb_per_s'] = b / (r['max_us'] * 1e3)
        res.setdefault('kernels', {})[which] = rows
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
