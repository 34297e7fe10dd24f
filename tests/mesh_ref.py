"""numpy model of dfl_amd.mesh: discrete marching cubes from data/mc_cases.txt, the vertex graph,
the windowed-sinc filter in fp64, and small mesh measures the tests use (edge use counts, Euler characteristic,
enclosed volume).  It shares only the case table and the coefficients with the package."""
import numpy as np

import dfl_amd  # noqa: F401
from dfl_amd import mesh

# lower end (dx, dy, dz) and axis of each edge (tools/gen_mc_table.py numbering)
EDGE_LO = np.array([[0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 1, 1, 0],
                    [0, 0, 0, 1], [1, 0, 0, 1], [0, 0, 1, 1], [1, 0, 1, 1],
                    [0, 0, 0, 2], [1, 0, 0, 2], [0, 1, 0, 2], [1, 1, 0, 2]], np.int64)


def marching_cubes(vol, label):
    """(verts [V, 3] fp32 (x, y, z), tris [T, 3] int32, keys [V] int64) of one label of vol [nz, ny, nx]."""
    nz, ny, nx = vol.shape
    inside = vol == label
    case = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    for i in range(8):
        dx, dy, dz = i & 1, (i >> 1) & 1, (i >> 2) & 1
        case |= inside[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx].astype(np.int64) << i
    off, edges = mesh.case_table()
    ntri = (off[1:] - off[:-1])[case].reshape(-1)
    cells = np.nonzero(ntri)[0]
    if cells.size == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros(0, np.int64)
    z, rem = np.divmod(cells, (nx - 1) * (ny - 1))
    y, x = np.divmod(rem, nx - 1)
    base = x + nx * (y + ny * z)
    reps = ntri[cells]
    first = np.repeat(off[case.reshape(-1)[cells]], reps)
    within = np.arange(reps.sum()) - np.repeat(np.cumsum(reps) - reps, reps)
    tri_edges = edges[first + within].astype(np.int64)                     # [T, 3]
    lo = EDGE_LO[tri_edges]
    koff = 3 * (lo[..., 0] + nx * (lo[..., 1] + ny * lo[..., 2])) + lo[..., 3]
    keys = 3 * np.repeat(base, reps)[:, None] + koff
    uniq, inv = np.unique(keys.reshape(-1), return_inverse=True)
    return decode(uniq, nx, ny), inv.reshape(-1, 3).astype(np.int32), uniq


def decode(keys, nx, ny):
    q, ax = np.divmod(keys, 3)
    x = q % nx
    y = (q // nx) % ny
    z = q // (nx * ny)
    p = np.stack([x, y, z], 1).astype(np.float64)
    p[np.arange(len(keys)), ax] += 0.5
    return p.astype(np.float32)


def neighbours(tris, V):
    """(row_ptr, col, fixed bool) as dfl_mesh_csr builds them."""
    t = tris.astype(np.int64)
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    keys = np.stack([a * V + b, b * V + a, b * V + c, c * V + b, c * V + a, a * V + c], 1).reshape(-1)
    uk, cnt = np.unique(keys, return_counts=True)
    row, col = np.divmod(uk, V)
    row_ptr = np.zeros(V + 1, np.int64)
    np.add.at(row_ptr, row + 1, 1)
    fixed = np.zeros(V, bool)
    fixed[row[cnt == 1]] = True
    return np.cumsum(row_ptr), col, fixed


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
    """sum a_n T_n(W) x in `dtype` (fp64: the reference of the tests; fp32: the kernel's operation order)."""
    V = x.shape[0]
    row_ptr, col, fixed = neighbours(tris, V)
    cnt = np.diff(row_ptr)
    coef = mesh.sinc_coefficients(iterations, passband)
    if dtype == np.float32:
        coef = coef.astype(np.float32)

    def W(y):
        s = np.zeros((V, 3), dtype)
        for k in range(int(cnt.max())):                   # neighbours summed in CSR order, as the kernel does
            sel = cnt > k
            s[sel] += y[col[row_ptr[:-1][sel] + k]]
        m = s / cnt[:, None].astype(dtype)
        m[fixed] = y[fixed]
        return m

    x0 = x.astype(dtype)
    t_prev, t = x0, W(x0)
    acc = coef[0] * x0 + coef[1] * t
    for n in range(2, iterations + 1):
        t_prev, t = t, (dtype(2) * W(t) - t_prev).astype(dtype)
        acc = acc + coef[n] * t
    acc = acc.astype(np.float64)
    acc[fixed] = x[fixed]
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
