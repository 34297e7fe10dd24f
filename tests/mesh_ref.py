"""numpy model of dfl_amd.mesh: discrete marching cubes from data/mc_cases.txt (with the raw keys
and the per-block counts of the two passes), the vertex graph and the vertex-triangle lists, the windowed-sinc filter in
fp64, the normals, and small mesh measures the tests use (edge use counts, Euler characteristic, enclosed volume).  It
shares only the case table, the coefficients and the block size with the package."""
import numpy as np

import dfl_amd  # noqa: F401
from dfl_amd import mesh

# lower end (dx, dy, dz) and axis of each edge (tools/gen_mc_table.py numbering)
EDGE_LO = np.array([[0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 1, 1, 0],
                    [0, 0, 0, 1], [1, 0, 0, 1], [0, 0, 1, 1], [1, 0, 1, 1],
                    [0, 0, 0, 2], [1, 0, 0, 2], [0, 1, 0, 2], [1, 1, 0, 2]], np.int64)


def cell_cases(vol, label):
    """uint8 [nz - 1, ny - 1, nx - 1]: the case of every cell of vol [nz, ny, nx] for one label (bit i = corner i inside)."""
    nz, ny, nx = vol.shape
    inside = vol == label
    case = np.zeros((nz - 1, ny - 1, nx - 1), np.uint8)
    for i in range(8):
        dx, dy, dz = i & 1, (i >> 1) & 1, (i >> 2) & 1
        case |= inside[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx].astype(np.uint8) << np.uint8(i)
    return case


def triangle_keys(vol, label):
    """(keys [T, 3] int64, ntri [cells] int64) of one label of vol [nz, ny, nx]: the three edge keys of every triangle in
    emit order (ascending cell, table order within a cell; nothing deduplicated), and the triangles of each cell."""
    nz, ny, nx = vol.shape
    case = cell_cases(vol, label).reshape(-1)
    off, edges = mesh.case_table()
    ntri = (off[1:] - off[:-1]).astype(np.int64)[case]
    cells = np.nonzero(ntri)[0]
    if cells.size == 0:
        return np.zeros((0, 3), np.int64), ntri
    z, rem = np.divmod(cells, (nx - 1) * (ny - 1))
    y, x = np.divmod(rem, nx - 1)
    base = x + nx * (y + ny * z)
    reps = ntri[cells]
    first = np.repeat(off[case[cells]].astype(np.int64), reps)
    within = np.arange(reps.sum()) - np.repeat(np.cumsum(reps) - reps, reps)
    tri_edges = edges[first + within].astype(np.int64)                     # [T, 3]
    lo = EDGE_LO[tri_edges]
    koff = 3 * (lo[..., 0] + nx * (lo[..., 1] + ny * lo[..., 2])) + lo[..., 3]
    return 3 * np.repeat(base, reps)[:, None] + koff, ntri


def marching_cubes(vol, label):
    """(verts [V, 3] fp32 (x, y, z), tris [T, 3] int32, keys [V] int64) of one label of vol [nz, ny, nx]."""
    nz, ny, nx = vol.shape
    keys, _ = triangle_keys(vol, label)
    if len(keys) == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros(0, np.int64)
    uniq, inv = np.unique(keys.reshape(-1), return_inverse=True)
    return decode(uniq, nx, ny), inv.reshape(-1, 3).astype(np.int32), uniq


def block_counts(vol, labels):
    """(block_counts int32 [n_blocks, MAX_LABELS], block_offsets int64 [n_blocks, MAX_LABELS], totals int64
    [MAX_LABELS + 1]) as dfl_mesh_mc_count leaves them (include/dfl_hip.h): per block of MESH_MC_CELLS cells the triangles
    of each label, the first triangle of each block and label with the labels one after another, totals[l] = the first
    triangle of label l and totals[n_labels] = the sum.  What the call does not write is -1 here: the offsets of the
    columns l >= n_labels and totals beyond n_labels (the counts of those columns are written, as 0)."""
    B, L = mesh.nat.MESH_MC_CELLS, mesh.MAX_LABELS
    nz, ny, nx = vol.shape
    nb = -(-((nx - 1) * (ny - 1) * (nz - 1)) // B)
    counts = np.zeros((nb, L), np.int32)
    offsets = np.full((nb, L), -1, np.int64)
    totals = np.full(L + 1, -1, np.int64)
    base = 0
    for l, lab in enumerate(labels):
        ntri = triangle_keys(vol, lab)[1]
        per = np.add.reduceat(ntri, np.arange(0, len(ntri), B))
        counts[:, l] = per
        offsets[:, l] = base + np.cumsum(per) - per
        totals[l] = base
        base += int(per.sum())
    totals[len(labels)] = base
    return counts, offsets, totals


def decode(keys, nx, ny):
    q, ax = np.divmod(keys, 3)
    x = q % nx
    y = (q // nx) % ny
    z = q // (nx * ny)
    p = np.stack([x, y, z], 1).astype(np.float64)
    p[np.arange(len(keys)), ax] += 0.5
    return p.astype(np.float32)


def edge_keys(tris, V):
    """[6T] int64 as dfl_mesh_topology writes them: i * V + j for (a,b) (b,a) (b,c) (c,b) (c,a) (a,c) of each triangle."""
    t = tris.astype(np.int64)
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    return np.stack([a * V + b, b * V + a, b * V + c, c * V + b, c * V + a, a * V + c], 1).reshape(-1)


def vt_keys(tris):
    """[3T] int64 as dfl_mesh_topology writes them: tris[t][k] * 3T + 3t + k."""
    t = tris.astype(np.int64)
    return (t * t.size + np.arange(t.size).reshape(-1, 3)).reshape(-1)


def _row_ptr(row, n_rows):
    row_ptr = np.zeros(n_rows + 1, np.int64)
    np.add.at(row_ptr, row + 1, 1)
    return np.cumsum(row_ptr)


def neighbours(tris, V):
    """(row_ptr, col, fixed bool) as dfl_mesh_csr builds them."""
    uk, cnt = np.unique(edge_keys(tris, V), return_counts=True)
    row, col = np.divmod(uk, V)
    fixed = np.zeros(V, bool)
    fixed[row[cnt == 1]] = True
    return _row_ptr(row, V), col, fixed


def vertex_triangles(tris, V):
    """(vt_ptr [V + 1], vt_tri [3T]) as dfl_mesh_csr over the sorted vt_keys builds them: each vertex's triangles ascending
    (one entry per corner, so a triangle that repeats a vertex is listed twice for it)."""
    row, rem = np.divmod(np.sort(vt_keys(tris)), 3 * len(tris))
    return _row_ptr(row, V), rem // 3


def normals(pos, tris, V):
    """[V, 3] fp64: unit(sum over a vertex's triangles, ascending, of (b - a) x (c - a)) in fp64 on the fp32 positions;
    0 where the sum is 0 (a vertex in no triangle, degenerate triangles only, or areas that cancel)."""
    vt_ptr, vt_tri = vertex_triangles(tris, V)
    p = pos.astype(np.float64)[tris[vt_tri]]                                # [3T, 3 corners, 3]
    fn = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    cnt = np.diff(vt_ptr)
    acc = np.zeros((V, 3))
    for k in range(int(cnt.max())):
        sel = cnt > k
        acc[sel] += fn[vt_ptr[:-1][sel] + k]
    length = np.sqrt((acc * acc).sum(1))
    return acc * np.where(length > 0, 1.0 / np.where(length > 0, length, 1.0), 0.0)[:, None]


def normalize(verts):
    """fp64 model of mesh.normalize: (x - c) / h on fp32 input, rounded to fp32; and the undo 4x4."""
    v = verts.astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    c, h = (lo + hi) / 2.0, float(np.max(hi - lo)) / 2.0
    M = np.eye(4)
    M[:3, :3] /= h
    M[:3, 3] = -c / h
    return apply(M, verts), np.linalg.inv(M)


def apply(M, x):
    """fp32(M x) evaluated in fp64, x [V, 3] fp32."""
    return (x.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)


def smooth(x, tris, iterations=mesh.ITERATIONS, passband=mesh.PASSBAND, dtype=np.float64):
    """sum a_n T_n(W) x in `dtype` (fp64: the reference of the tests; fp32: the kernel's operation order).  W is the
    identity for a fixed vertex and for one without neighbours (no triangle uses it): both keep their input bit for bit."""
    V = x.shape[0]
    row_ptr, col, fixed = neighbours(tris, V)
    cnt = np.diff(row_ptr)
    keep = fixed | (cnt == 0)
    coef = mesh.sinc_coefficients(iterations, passband)
    if dtype == np.float32:
        coef = coef.astype(np.float32)

    def W(y):
        s = np.zeros((V, 3), dtype)
        for k in range(int(cnt.max())):                   # neighbours summed in CSR order, as the kernel does
            sel = cnt > k
            s[sel] += y[col[row_ptr[:-1][sel] + k]]
        m = s / np.maximum(cnt, 1)[:, None].astype(dtype)
        m[keep] = y[keep]
        return m

    x0 = x.astype(dtype)
    t_prev, t = x0, W(x0)
    acc = coef[0] * x0 + coef[1] * t
    for n in range(2, iterations + 1):
        t_prev, t = t, (dtype(2) * W(t) - t_prev).astype(dtype)
        acc = acc + coef[n] * t
    acc = acc.astype(np.float64)
    acc[keep] = x[keep]
    return acc, fixed


def edge_uses(tris):
    """{(i, j) with i < j: number of triangles using the edge}."""
    t = tris.astype(np.int64)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), 1)
    u, cnt = np.unique(e, axis=0, return_counts=True)
    return dict(zip(map(tuple, u), cnt))


def euler(verts, tris):
    return len(verts) - len(edge_uses(tris)) + len(tris)


def signed_volume(verts, tris):
    p = verts.astype(np.float64)[tris]
    return float(np.einsum('ij,ij->i', p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def ball(n, r, c=None):
    """uint8 [n, n, n] with 1 inside the ball of radius r (voxel units) about c."""
    c = (n - 1) / 2.0 if c is None else c
    z, y, x = np.mgrid[:n, :n, :n]
    return (((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) <= r * r).astype(np.uint8)


def torus(n, R, r):
    c = (n - 1) / 2.0
    z, y, x = np.mgrid[:n, :n, :n].astype(np.float64) - c
    return (((np.sqrt(x * x + y * y) - R) ** 2 + z * z) <= r * r).astype(np.uint8)
