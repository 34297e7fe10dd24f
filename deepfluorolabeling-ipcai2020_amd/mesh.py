"""Bone surfaces on the GPU: the vtkDiscreteMarchingCubes -> vtkWindowedSincPolyDataFilter -> transform chain of the
reference's examples_dataset/full_res_3d_viz.py, restated in DESIGN.md section 12 (no VTK parity is claimed).

label_surfaces() runs discrete marching cubes for up to MAX_LABELS labels in one pass over a uint8 volume; smooth()
applies the windowed-sinc filter; transform() applies an fp64 affine 4x4; vertex_normals() gives area-weighted
normals; decimate() reduces a surface by rounds of quadric-error edge collapses (the place of the
reference's vtkQuadricDecimation).  The kernels are csrc/mesh.hip and csrc/decimate.hip (include/dfl_hip.h "Bone
surfaces"); sorting and deduplicating keys is done with torch.  There is no host path: CPU tensors are refused."""
import math
import os

import numpy as np
import torch

from . import _native as nat

TABLE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'data', 'mc_cases.txt')
MAX_LABELS = nat.MESH_MAX_LABELS
ITERATIONS, PASSBAND = 25, 0.1           # full_res_3d_viz.py create_mesh

_loops = None
_table = None
_table_dev = {}


def case_loops():
    """[256] lists of loops (lists of edge numbers) of data/mc_cases.txt (tools/gen_mc_table.py)."""
    global _loops
    if _loops is None:
        loops = [None] * 256
        with open(TABLE_PATH) as f:
            for line in f:
                if line.startswith('#') or not line.strip():
                    continue
                tok = line.split()
                loops[int(tok[0])] = [[int(e) for e in t.split(',')] for t in tok[1:]]
        if any(lp is None for lp in loops):
            raise nat.DflError('%s: not every case is listed' % TABLE_PATH)
        _loops = loops
    return _loops


def case_table():
    """(tri_off int32 [257], tri_edges uint8 [n, 3]): the fan (l0, l_k, l_k+1) of every loop, cases in order."""
    global _table
    if _table is None:
        off, tris = [0], []
        for loops in case_loops():
            for lp in loops:
                tris += [(lp[0], lp[k], lp[k + 1]) for k in range(1, len(lp) - 1)]
            off.append(len(tris))
        _table = (np.array(off, np.int32), np.array(tris, np.uint8).reshape(-1, 3))
    return _table


def _table_on(dev):
    t = _table_dev.get(dev)
    if t is None:
        off, edges = case_table()
        t = _table_dev[dev] = (torch.from_numpy(off).to(dev), torch.from_numpy(edges).to(dev))
    return t


def sinc_coefficients(iterations=ITERATIONS, passband=PASSBAND):
    """a_n, n = 0 .. iterations (fp64): Hamming-windowed Chebyshev coefficients of the low-pass, normalised to sum 1."""
    theta = math.acos(1.0 - passband / 2.0)
    n = np.arange(iterations + 1, dtype=np.float64)
    c = np.empty(iterations + 1)
    c[0] = theta / math.pi
    c[1:] = 2.0 * np.sin(n[1:] * theta) / (n[1:] * math.pi)
    w = 0.54 + 0.46 * np.cos(n * math.pi / (iterations + 1))
    return w * c / np.sum(w * c)


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _gpu(t, what, dtype, shape_ok=None):
    if not torch.is_tensor(t):
        raise nat.DflError('mesh.%s: a torch tensor is required' % what)
    if t.dtype != dtype:
        raise nat.DflError('mesh.%s: dtype %s, %s expected' % (what, t.dtype, dtype))
    if not t.is_cuda:
        raise nat.DflError('mesh.%s needs its tensors on the GPU (no CPU path)' % what)
    if shape_ok is not None and not shape_ok(t.shape):
        raise nat.DflError('mesh.%s: bad shape %s' % (what, tuple(t.shape)))
    return t.contiguous()


def label_surfaces(volume, labels):
    """Discrete marching cubes of volume [nz, ny, nx] (uint8, GPU, x fastest) for each label: a list of
    (verts [V, 3] fp32 in index space (x, y, z), tris [T, 3] int32).  Vertices are edge midpoints in ascending edge key
    order, triangles in ascending cell order, then table order; counter-clockwise seen from outside the label."""
    vol = _gpu(volume, 'label_surfaces: volume', torch.uint8, lambda s: len(s) == 3)
    labels = [int(v) for v in labels]
    if not 1 <= len(labels) <= MAX_LABELS or any(not 0 <= v <= 255 for v in labels):
        raise nat.DflError('mesh.label_surfaces: 1 to %d labels in 0..255, got %r' % (MAX_LABELS, labels))
    nz, ny, nx = vol.shape
    if min(nx, ny, nz) < 2:
        raise nat.DflError('mesh.label_surfaces: volume %s has no cells' % (tuple(vol.shape),))
    cells = (nx - 1) * (ny - 1) * (nz - 1)
    if cells >= 2 ** 31:
        raise nat.DflError('mesh.label_surfaces: %d cells, at most 2^31 - 1' % cells)
    dev = vol.device
    off, edges = _table_on(dev)
    nb = -(-cells // nat.MESH_MC_CELLS)
    counts = torch.empty(nb * MAX_LABELS, dtype=torch.int32, device=dev)
    offsets = torch.empty(nb * MAX_LABELS, dtype=torch.int64, device=dev)
    totals = torch.empty(MAX_LABELS + 1, dtype=torch.int64, device=dev)
    a = nat.MeshMcArgs(volume=vol.data_ptr(), tri_off=off.data_ptr(), tri_edges=edges.data_ptr(),
                       block_counts=counts.data_ptr(), block_offsets=offsets.data_ptr(), totals=totals.data_ptr(),
                       nx=nx, ny=ny, nz=nz, n_labels=len(labels))
    for i, v in enumerate(labels):
        a.labels[i] = v
    s = _stream(vol)
    nat.call('dfl_mesh_mc_count', a, s)
    first = totals.cpu().tolist()
    keys = torch.empty(max(3 * first[len(labels)], 1), dtype=torch.int64, device=dev)
    a.keys = keys.data_ptr()
    nat.call('dfl_mesh_mc_emit', a, s)
    out = []
    for l in range(len(labels)):
        k = keys[3 * first[l]:3 * first[l + 1]]
        uniq, inv = torch.unique(k, sorted=True, return_inverse=True)
        if uniq.numel() >= 2 ** 31:
            raise nat.DflError('mesh.label_surfaces: %d vertices, at most 2^31 - 1' % uniq.numel())
        verts = torch.empty((uniq.numel(), 3), dtype=torch.float32, device=dev)
        if uniq.numel():
            nat.call('dfl_mesh_decode', nat.MeshDecodeArgs(keys=uniq.data_ptr(), pos=verts.data_ptr(), V=uniq.numel(),
                                                           nx=nx, ny=ny), s)
        out.append((verts, inv.view(-1, 3).to(torch.int32)))
    return out


def _check_mesh(verts, tris, what):
    verts = _gpu(verts, what + ': verts', torch.float32, lambda s: len(s) == 2 and s[1] == 3)
    tris = _gpu(tris, what + ': tris', torch.int32, lambda s: len(s) == 2 and s[1] == 3)
    if verts.device != tris.device:
        raise nat.DflError('mesh.%s: verts and tris on different devices' % what)
    return verts, tris


def _csr(keys, counts, div, col_div, n_rows):
    dev = keys.device
    col = torch.empty(keys.numel(), dtype=torch.int32, device=dev)
    row_ptr = torch.empty(n_rows + 1, dtype=torch.int32, device=dev)
    fixed = torch.empty(n_rows, dtype=torch.uint8, device=dev) if counts is not None else None
    nat.call('dfl_mesh_csr', nat.MeshCsrArgs(keys=keys.data_ptr(), counts=nat.ptr(counts), col=col.data_ptr(),
                                             row_ptr=row_ptr.data_ptr(), fixed=nat.ptr(fixed), nnz=keys.numel(), div=div,
                                             col_div=col_div, n_rows=n_rows), _stream(keys))
    return row_ptr, col, fixed


def neighbours(tris, V):
    """(row_ptr [V + 1], col, fixed [V] uint8) of the vertex graph of tris: each vertex's distinct neighbours in
    ascending id order; fixed = on an edge of exactly one triangle."""
    T = tris.shape[0]
    ek = torch.empty(6 * T, dtype=torch.int64, device=tris.device)
    nat.call('dfl_mesh_topology', nat.MeshTopoArgs(tris=tris.data_ptr(), edge_keys=ek.data_ptr(), T=T, V=V), _stream(tris))
    uk, cnt = torch.unique(ek, sorted=True, return_counts=True)
    return _csr(uk, cnt, V, 1, V)


def vertex_triangles(tris, V):
    """(vt_ptr [V + 1], vt_tri [3T]): the triangles of each vertex in ascending order."""
    T = tris.shape[0]
    vk = torch.empty(3 * T, dtype=torch.int64, device=tris.device)
    nat.call('dfl_mesh_topology', nat.MeshTopoArgs(tris=tris.data_ptr(), vt_keys=vk.data_ptr(), T=T, V=V), _stream(tris))
    ptr, tri, _ = _csr(torch.sort(vk).values, None, 3 * T, 3, V)
    return ptr, tri


def normalize(verts):
    """(verts centred on their bounding box and scaled to [-1, 1] by the largest half extent, in fp64, rounded to
    fp32; the fp64 4x4 that undoes it)."""
    verts = _gpu(verts, 'normalize: verts', torch.float32, lambda s: len(s) == 2 and s[1] == 3 and s[0] > 0)
    lo, hi = (t.double().cpu().numpy() for t in torch.aminmax(verts, dim=0))
    c = (lo + hi) / 2.0
    h = float(np.max(hi - lo)) / 2.0
    if not h > 0:
        raise nat.DflError('mesh.normalize: the vertices have no extent')
    M = np.eye(4)
    M[:3, :3] /= h
    M[:3, 3] = -c / h
    undo = np.eye(4)
    undo[:3, :3] *= h
    undo[:3, 3] = c
    return transform(verts, M), undo


def smooth(verts, tris, iterations=ITERATIONS, passband=PASSBAND):
    """Windowed-sinc smoothing of verts [V, 3] fp32 with the triangles tris [T, 3] int32:
    (smoothed positions in the normalised frame of normalize(), fp32 [V, 3]; the fp64 4x4 back to the input frame).
    Vertices on an edge of exactly one triangle, and vertices that no triangle uses, keep their normalised position bit
    for bit."""
    verts, tris = _check_mesh(verts, tris, 'smooth')
    if not 1 <= int(iterations) <= nat.MESH_MAX_ITERS:
        raise nat.DflError('mesh.smooth: 1 to %d iterations' % nat.MESH_MAX_ITERS)
    if tris.shape[0] == 0:
        raise nat.DflError('mesh.smooth: no triangles')
    V = verts.shape[0]
    xn, undo = normalize(verts)
    row_ptr, col, fixed = neighbours(tris, V)
    dev = verts.device
    scratch = [torch.empty((V, 4), dtype=torch.float32, device=dev) for _ in range(3)]
    out = torch.empty((V, 3), dtype=torch.float32, device=dev)
    a = nat.MeshSmoothArgs(x=xn.data_ptr(), row_ptr=row_ptr.data_ptr(), col=col.data_ptr(), fixed=fixed.data_ptr(),
                           t_a=scratch[0].data_ptr(), t_b=scratch[1].data_ptr(), acc=scratch[2].data_ptr(),
                           out=out.data_ptr(), V=V, iterations=int(iterations))
    for n, v in enumerate(sinc_coefficients(int(iterations), passband)):
        a.coef[n] = float(v)
    nat.call('dfl_mesh_smooth', a, _stream(verts))
    return out, undo


def transform(x, M):
    """fp32(M x) for x [V, 3] fp32, M an affine 4x4, evaluated in fp64."""
    x = _gpu(x, 'transform: x', torch.float32, lambda s: len(s) == 2 and s[1] == 3)
    M = np.asarray(M, dtype=np.float64)
    if M.shape != (4, 4) or not np.array_equal(M[3], [0, 0, 0, 1]) or not np.all(np.isfinite(M)):
        raise nat.DflError('mesh.transform: a finite affine 4x4 (last row 0 0 0 1) is required')
    out = torch.empty_like(x)
    a = nat.MeshXformArgs(x=x.data_ptr(), out=out.data_ptr(), V=x.shape[0])
    for i, v in enumerate(M.reshape(-1)):
        a.M[i] = float(v)
    nat.call('dfl_mesh_transform', a, _stream(x))
    return out


REDUCTION, MAX_ROUNDS = 0.25, 64         # full_res_3d_viz.py create_mesh: vtkQuadricDecimation.SetTargetReduction(0.25)


def collapse_budget(reduction, T):
    """Edge collapses that take `reduction` of T triangles away, two per collapse: floor(reduction T) // 2."""
    return int(math.floor(float(reduction) * T)) // 2


def _round_topology(tris, V):
    """The lists one decimation round gathers over (include/dfl_hip.h: dfl_mesh_collapse_keys): the neighbour CSR with the
    use count and the undirected edge of every entry, the undirected edges in ascending order, the vertex-triangle CSR."""
    T = tris.shape[0]
    ek = torch.empty(6 * T, dtype=torch.int64, device=tris.device)
    vk = torch.empty(3 * T, dtype=torch.int64, device=tris.device)
    nat.call('dfl_mesh_topology', nat.MeshTopoArgs(tris=tris.data_ptr(), edge_keys=ek.data_ptr(), vt_keys=vk.data_ptr(), T=T, V=V),
             _stream(tris))
    uk, cnt = torch.unique(ek, sorted=True, return_counts=True)
    row_ptr, col, _ = _csr(uk, cnt, V, 1, V)
    vt_ptr, vt_tri, _ = _csr(torch.sort(vk).values, None, 3 * T, 3, V)
    row = torch.div(uk, V, rounding_mode='floor')
    to = uk - row * V
    und = row < to
    eid = torch.searchsorted(uk[und], torch.minimum(row, to) * V + torch.maximum(row, to)).to(torch.int32)
    return dict(row_ptr=row_ptr, col=col, use=cnt.to(torch.int32), eid=eid, edge_u=row[und].to(torch.int32),
                edge_v=to[und].to(torch.int32), vt_ptr=vt_ptr, vt_tri=vt_tri)


def decimate(verts, tris, reduction=REDUCTION, max_rounds=MAX_ROUNDS):
    """Quadric-error decimation by rounds of edge collapses that do not touch: (verts', tris',
    {'collapses', 'rounds', 'budget'}).  budget = floor(reduction T) // 2 collapses, each taking one vertex and two
    triangles away; rounds end when the budget is spent, a round finds no collapse, or after max_rounds.  Vertices on a
    border or a non-manifold edge stay where they are; surviving vertices and triangles keep their order and winding."""
    if not 0.0 < float(reduction) < 1.0:
        raise nat.DflError('mesh.decimate: reduction %r outside (0, 1)' % (reduction,))
    verts, tris = _check_mesh(verts, tris, 'decimate')
    if tris.shape[0] == 0:
        raise nat.DflError('mesh.decimate: no triangles')
    lo, hi = (int(v) for v in torch.aminmax(tris))
    if lo < 0 or hi >= verts.shape[0]:
        raise nat.DflError('mesh.decimate: triangle indices %d .. %d outside [0, %d)' % (lo, hi, verts.shape[0]))
    if bool(((tris[:, 0] == tris[:, 1]) | (tris[:, 1] == tris[:, 2]) | (tris[:, 2] == tris[:, 0])).any()):
        raise nat.DflError('mesh.decimate: a triangle repeats a vertex')
    dev, s = verts.device, _stream(verts)
    budget = collapse_budget(reduction, tris.shape[0])
    done = rounds = 0
    while done < budget and rounds < int(max_rounds):
        V, T = verts.shape[0], tris.shape[0]
        tp = _round_topology(tris, V)
        E = tp['edge_u'].numel()
        p = {k: t.data_ptr() for k, t in tp.items()}
        Q = torch.empty((V, 10), dtype=torch.float64, device=dev)
        nat.call('dfl_mesh_quadrics', nat.MeshQuadricsArgs(pos=verts.data_ptr(), tris=tris.data_ptr(), vt_ptr=p['vt_ptr'],
                                                           vt_tri=p['vt_tri'], Q=Q.data_ptr(), V=V, T=T), s)
        key = torch.empty(E, dtype=torch.int64, device=dev)          # uint64 bits; torch sorts them as int64 below
        cand = torch.empty((E, 3), dtype=torch.float32, device=dev)
        nat.call('dfl_mesh_collapse_keys', nat.MeshCollapseKeysArgs(
            pos=verts.data_ptr(), tris=tris.data_ptr(), row_ptr=p['row_ptr'], col=p['col'], use=p['use'], vt_ptr=p['vt_ptr'],
            vt_tri=p['vt_tri'], Q=Q.data_ptr(), edge_u=p['edge_u'], edge_v=p['edge_v'], key=key.data_ptr(), cand=cand.data_ptr(),
            V=V, T=T, E=E), s)
        m1, m2 = (torch.empty(V, dtype=torch.int64, device=dev) for _ in range(2))
        sel = torch.empty(E, dtype=torch.uint8, device=dev)
        nat.call('dfl_mesh_collapse_select', nat.MeshCollapseSelectArgs(
            row_ptr=p['row_ptr'], col=p['col'], eid=p['eid'], edge_u=p['edge_u'], edge_v=p['edge_v'], key=key.data_ptr(),
            m1=m1.data_ptr(), m2=m2.data_ptr(), sel=sel.data_ptr(), V=V, E=E), s)
        chosen = torch.nonzero(sel).view(-1)
        if chosen.numel() > budget - done:
            # the lowest keys win: a selected key has a finite non-negative cost, so its sign bit is clear and the
            # signed order is the unsigned one
            chosen = chosen[torch.sort(key[chosen]).indices[:budget - done]]
        n = chosen.numel()
        if n == 0:
            break
        take = torch.zeros(E, dtype=torch.uint8, device=dev)
        take[chosen] = 1
        remap = torch.empty(V, dtype=torch.int32, device=dev)
        pos_out, tris_out = torch.empty_like(verts), torch.empty_like(tris)
        degen = torch.empty(T, dtype=torch.uint8, device=dev)
        nat.call('dfl_mesh_collapse_apply', nat.MeshCollapseApplyArgs(
            pos=verts.data_ptr(), tris=tris.data_ptr(), row_ptr=p['row_ptr'], col=p['col'], eid=p['eid'], take=take.data_ptr(),
            cand=cand.data_ptr(), remap=remap.data_ptr(), pos_out=pos_out.data_ptr(), tris_out=tris_out.data_ptr(),
            degen=degen.data_ptr(), V=V, T=T, E=E), s)
        keep = remap == torch.arange(V, dtype=torch.int32, device=dev)
        new_id = (torch.cumsum(keep, 0) - 1).to(torch.int32)
        verts = pos_out[keep].contiguous()
        tris = new_id[tris_out[degen == 0].long()].contiguous()
        done += n
        rounds += 1
    return verts, tris, {'collapses': done, 'rounds': rounds, 'budget': budget}


def vertex_normals(pos, tris):
    """Unit area-weighted vertex normals [V, 3] fp32 (fp64 sums over each vertex's triangles in ascending order)."""
    pos, tris = _check_mesh(pos, tris, 'vertex_normals')
    V = pos.shape[0]
    out = torch.zeros((V, 3), dtype=torch.float32, device=pos.device)
    if tris.shape[0] == 0:
        return out
    vt_ptr, vt_tri = vertex_triangles(tris, V)
    nat.call('dfl_mesh_normals', nat.MeshNormalsArgs(pos=pos.data_ptr(), tris=tris.data_ptr(), vt_ptr=vt_ptr.data_ptr(),
                                                     vt_tri=vt_tri.data_ptr(), normals=out.data_ptr(), V=V), _stream(pos))
    return out
