"""The kernels of csrc/mesh.hip through their C entry points (include/dfl_hip.h "Bone surfaces"), as dfl_amd/mesh.py calls
them, at the sizes where they branch: cell counts around a round of 256 and a block of 4096 cells, the second round of the
block scan, four labels filling the packed 16-bit counts, every marching-cubes case, keys beyond 2^32, CSR rows without
entries, every template form of the smoother, the transform in place and the normals' zero cases.

Reference: the numpy model tests/mesh_ref.py.  Everything but the smoother, the transform and the normals is integer work
and is compared for exact equality, order included.

Every output and scratch buffer is filled with a sentinel before the call (-1, 0xff, NaN), and outputs carry GUARD
elements past their end that must still hold it afterwards.  Integer outputs that a later kernel uses as addresses are
asserted against the model before that kernel is launched (block_offsets and totals before dfl_mesh_mc_emit, row_ptr and
col before dfl_mesh_smooth and dfl_mesh_normals): a wrong offset fails an assertion instead of becoming a wild store.
Every index handed to a kernel is in range.

Smoother bar.  E32 = max |model in fp32 - model in fp64| on the same mesh and number of terms, measured in the test.  The
kernel and the fp32 model evaluate the same sums over the same neighbours in the same order and differ only where the
compiler contracts a multiply-add (half an ulp per operation), so the kernel must stay within 4 x E32 of the fp64 model.
Transform bar, per component: 0.5 ulp32(exact) + 2^-50 (sum_j |M_rj x_j| + |M_r3|), `exact` evaluated in numpy fp64; the
second term covers the fp64 evaluation order and contraction on both sides.  Normals bar: 2^-23 absolute (fp64 inside,
one rounding of a component of a unit vector), on a surface where no vertex's sum cancels below 1e-3 of its terms."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, 'tests'))
import mesh_ref as R  # noqa: E402
from dfl_amd import _native as nat, mesh  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 64
L = nat.MESH_MAX_LABELS
B = nat.MESH_MC_CELLS
NAN = float('nan')


def stream():
    return torch.cuda.current_stream().cuda_stream


def filled(n, dtype, value):
    return torch.full((n + GUARD,), value, dtype=dtype, device=DEV)


def head(t, n, what):
    """The first n elements of a buffer made by filled(n, ...), on the host; its guard must still hold the sentinel."""
    a = t.cpu().numpy()
    g = a[n:]
    assert g.size == GUARD
    if a.dtype.kind == 'f':
        assert np.all(np.isnan(g)), what + ': written past the end'
    else:
        assert np.all(g == (255 if a.dtype == np.uint8 else -1)), what + ': written past the end'
    return a[:n]


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, '%s: %d of %d differ, first at %d: got %s, model %s' % (
        what, bad.size, got.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- marching cubes -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table():
    return tuple(torch.from_numpy(a).to(DEV) for a in mesh.case_table())


def mc_model(vol, labels):
    """(block_counts, block_offsets, totals, keys [T, 3] of all labels in order) of the model."""
    return R.block_counts(vol, labels) + (np.concatenate([R.triangle_keys(vol, lab)[0] for lab in labels]),)


def check_mc(vol, labels, model=None):
    """dfl_mesh_mc_count, its outputs against the model, then dfl_mesh_mc_emit and the raw keys; twice, equal bytes."""
    want_counts, want_offsets, want_totals, want_keys = model or mc_model(vol, labels)
    nz, ny, nx = vol.shape
    nb = -(-((nx - 1) * (ny - 1) * (nz - 1)) // B)
    assert want_counts.shape == (nb, L)
    T = int(want_totals[len(labels)])
    assert want_keys.shape == (T, 3)
    vol_d = torch.from_numpy(vol).to(DEV)
    off, edges = table()
    runs = []
    for _ in range(2):
        counts, offsets = filled(nb * L, torch.int32, -1), filled(nb * L, torch.int64, -1)
        totals = filled(L + 1, torch.int64, -1)
        a = nat.MeshMcArgs(volume=vol_d.data_ptr(), tri_off=off.data_ptr(), tri_edges=edges.data_ptr(),
                           block_counts=counts.data_ptr(), block_offsets=offsets.data_ptr(), totals=totals.data_ptr(),
                           nx=nx, ny=ny, nz=nz, n_labels=len(labels))
        for i, v in enumerate(labels):
            a.labels[i] = v
        nat.call('dfl_mesh_mc_count', a, stream())
        got = [head(counts, nb * L, 'block_counts').reshape(nb, L), head(offsets, nb * L, 'block_offsets').reshape(nb, L),
               head(totals, L + 1, 'totals')]
        # before emit is launched: it addresses `keys` by these
        same(got[0], want_counts, 'block_counts')
        same(got[1], want_offsets, 'block_offsets')
        same(got[2], want_totals, 'totals')
        keys = filled(3 * T, torch.int64, -1)
        a.keys = keys.data_ptr()
        nat.call('dfl_mesh_mc_emit', a, stream())
        got.append(head(keys, 3 * T, 'keys').reshape(T, 3))
        same(got[3], want_keys, 'keys')
        same(head(offsets, nb * L, 'block_offsets'), want_offsets.reshape(-1), 'block_offsets after emit')
        runs.append(b''.join(g.tobytes() for g in got))
    assert runs[0] == runs[1], 'two runs differ'
    return want_counts, want_totals


def random_volume(shape, seed=0, top=5):
    return np.random.default_rng([seed, *shape]).integers(0, top, shape).astype(np.uint8)


def all_cases_strip():
    """(2, 2, 768): the cell at x = 3k has case k (corner i of it set when bit i of k is), for every k."""
    vol = np.zeros((2, 2, 768), np.uint8)
    k = np.arange(256)
    for i in range(8):
        vol[(i >> 2) & 1, (i >> 1) & 1, 3 * k + (i & 1)] = (k >> i) & 1
    case = R.cell_cases(vol, 1).reshape(-1)
    assert np.array_equal(case[::3], k) and np.array_equal(np.unique(case), k)      # the condition: every case occurs
    return vol


def test_every_case_of_the_table():
    check_mc(all_cases_strip(), [1])


@pytest.mark.parametrize('shape', [(3, 3, 3), (17, 17, 17), (17, 17, 18), (18, 18, 18), (9, 11, 13), (5, 4, 2)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_cell_count_tails(shape):
    """8 cells (less than a round); 4096 (one block); 4352 (a block and one round); 4913 (a partial round); three
    different sizes (an nx / ny swap); nx - 1 == 1 (the 32-bit division of mc_classify)."""
    vol = random_volume(shape)
    counts, totals = check_mc(vol, [1, 2, 3, 4])
    assert np.all(np.diff(totals) > 0), 'a label without triangles'
    assert int(np.prod(np.array(shape) - 1)) == {(3, 3, 3): 8, (17, 17, 17): 4096, (17, 17, 18): 4352, (18, 18, 18): 4913,
                                                 (9, 11, 13): 960, (5, 4, 2): 12}[shape]


def checkerboard():
    z, y, x = np.mgrid[:18, :18, :18]
    return ((x + y + z) & 1).astype(np.uint8)


def test_packed_counts_full_in_all_four_fields():
    """Four labels with 4 triangles in every cell: each 16-bit field of a full block's packed count holds 16384, so a carry
    between fields would show.  Duplicate labels are legal."""
    vol, labels = checkerboard(), [1, 0, 1, 0]
    counts = R.block_counts(vol, labels)[0]
    assert counts.shape == (2, 4) and np.all(counts[0] == 4 * B)            # the condition, on the model
    assert np.all(R.triangle_keys(vol, 1)[1] == 4) and np.all(R.triangle_keys(vol, 0)[1] == 4)
    check_mc(vol, labels)


LABEL_FORMS = [[1], [1, 2], [1, 2, 3], [1, 2, 3, 4], [7, 1, 2], [1, 7, 2], [1, 2, 7], [0, 255], [255, 0, 3]]


@pytest.mark.parametrize('labels', LABEL_FORMS, ids=lambda v: '-'.join(map(str, v)))
def test_label_forms(labels):
    """1 to 4 labels; an absent label (7) first, in the middle and last: an empty range between equal totals; 0 and 255."""
    vol = random_volume((9, 11, 13), seed=1, top=6)
    vol[vol == 5] = 255
    _, totals = check_mc(vol, labels)
    n = np.diff(totals[:len(labels) + 1])
    assert np.array_equal(n == 0, np.array(labels) == 7), (labels, totals)


SCAN_STRIPS = {524289: 1024, 527105: 1030}         # nx of a (3, 5, nx) strip: blocks of its 8 (nx - 1) cells


@functools.lru_cache(maxsize=None)
def scan_strip(nx):
    """A (3, 5, nx) strip with about 20000 voxels of labels 1..4 and its model.  One voxel of every label is planted in
    blocks 0, 1023, 1024 (where the strip has it) and the last, so that, on the model, every label has triangles on both
    sides of the scan's round boundary and in the last block."""
    rng = np.random.default_rng(nx)
    vol = np.zeros((3, 5, nx), np.uint8)
    idx = rng.choice(vol.size, 20000, replace=False)
    vol.reshape(-1)[idx] = rng.integers(1, 5, idx.size)
    cells = 8 * (nx - 1)
    nb = -(-cells // B)
    assert nb == SCAN_STRIPS[nx]
    blocks = sorted({0, 1023, min(1024, nb - 1), nb - 1})
    for b in blocks:
        for lab in (1, 2, 3, 4):
            c = b * B + 100 * lab
            assert c < cells
            z, rem = divmod(c, 4 * (nx - 1))
            y, x = divmod(rem, nx - 1)
            vol[z, y, x] = lab                              # the lower corner of cell c
    model = mc_model(vol, [1, 2, 3, 4])
    assert np.all(model[0][blocks] > 0), 'a planted block without triangles'      # the condition
    return vol, model


@pytest.mark.parametrize('nx', sorted(SCAN_STRIPS))
def test_scan_rounds(nx):
    """Exactly 1024 blocks (one full round of mc_scan_kernel and no second), and 1030 (a second round of 6 that starts
    from the first round's carry)."""
    vol, model = scan_strip(nx)
    check_mc(vol, [1, 2, 3, 4], model)


def test_label_surfaces_beyond_one_scan_round():
    vol, _ = scan_strip(527105)
    got = mesh.label_surfaces(torch.from_numpy(vol).to(DEV), [1, 2, 3, 4])
    for lab, (v, t) in zip((1, 2, 3, 4), got):
        P, T, _ = R.marching_cubes(vol, lab)
        assert len(T) > 0
        same(t.cpu().numpy(), T, 'triangles of label %d' % lab)
        same(bits(v.cpu().numpy()), bits(P), 'vertices of label %d' % lab)


# ---- decode -------------------------------------------------------------------------------------------------------------
DECODE_NX, DECODE_NY = 2000, 1500


def check_decode(keys):
    V = len(keys)
    assert np.all(np.diff(keys) > 0)
    pos = filled(3 * V, torch.float32, NAN)
    kd = torch.from_numpy(keys).to(DEV)
    nat.call('dfl_mesh_decode', nat.MeshDecodeArgs(keys=kd.data_ptr(), pos=pos.data_ptr(), V=V, nx=DECODE_NX, ny=DECODE_NY),
             stream())
    same(bits(head(pos, 3 * V, 'pos')).reshape(V, 3), bits(R.decode(keys, DECODE_NX, DECODE_NY)), 'pos')


@pytest.mark.parametrize('V', [1, 256, 257])
def test_decode_beyond_32_bits(V):
    """Sorted keys of a 2000 x 1500 grid with z up to 700 (no volume is allocated): keys reach 6.3e9, past 2^32.  The
    linear index itself stays just below 2^31 at z = 700, so one key at z = 720 is added where it does not."""
    nx, ny = DECODE_NX, DECODE_NY
    top = nx - 1 + nx * (ny - 1 + ny * 700)
    if V == 1:
        for ax in range(3):
            check_decode(np.array([3 * top + ax], np.int64))
        check_decode(np.array([0], np.int64))
        return
    rng = np.random.default_rng(V)
    q = rng.integers(0, nx, V) + nx * (rng.integers(0, ny, V) + ny * rng.integers(0, 701, V))
    keys = 3 * q + rng.integers(0, 3, V)
    keys[:5] = [0, 1, 3 * top + 2, 3 * (17 + nx * (5 + ny * 720)) + 1, 3 * (nx - 1) + 2]
    keys = np.unique(keys).astype(np.int64)
    assert len(keys) == V and keys.max() > 2 ** 32 and (keys // 3).max() > 2 ** 31
    assert set((keys % 3).tolist()) == {0, 1, 2} and np.sum(keys > 2 ** 31) > V // 2
    check_decode(keys)


# ---- topology and CSR ---------------------------------------------------------------------------------------------------
TETRA = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)      # closed, consistently wound
TETRA_IDS = np.array([1, 2, 4, 6], np.int32)                                  # of 8: 0, 3, 5 and 7 are in no triangle


@functools.lru_cache(maxsize=None)
def mesh_case(name):
    """(positions [V, 3] fp32 in the smoother's normalised frame, tris [T, 3] int32)."""
    rng = np.random.default_rng(11)
    if name.startswith('blob'):
        z = load_golden('viz3d_blob')
        i = int(name[4:])
        return R.normalize(z['verts_%d' % i])[0], z['tris_%d' % i]
    V, tris = {'triangle': (3, TETRA[:1]), 'two': (4, np.array([[0, 1, 2], [0, 2, 3]], np.int32)), 'tetra': (4, TETRA),
               'tetra+unused': (8, TETRA_IDS[TETRA])}[name]
    return rng.uniform(-1, 1, (V, 3)).astype(np.float32), tris


def topology(tris, V, edge, vt):
    T = len(tris)
    td = torch.from_numpy(np.ascontiguousarray(tris)).to(DEV)
    ek = filled(6 * T, torch.int64, -1) if edge else None
    vk = filled(3 * T, torch.int64, -1) if vt else None
    nat.call('dfl_mesh_topology', nat.MeshTopoArgs(tris=td.data_ptr(), edge_keys=nat.ptr(ek), vt_keys=nat.ptr(vk), T=T, V=V),
             stream())
    if edge:
        same(head(ek, 6 * T, 'edge_keys'), R.edge_keys(tris, V), 'edge_keys')
    if vt:
        same(head(vk, 3 * T, 'vt_keys'), R.vt_keys(tris), 'vt_keys')


def csr(keys, counts, div, col_div, n_rows, want_ptr, want_col, want_fixed=None):
    """dfl_mesh_csr over sorted keys, asserted against the model; the device buffers (with their guards)."""
    nnz = len(keys)
    kd = torch.from_numpy(keys).to(DEV)
    cd = None if counts is None else torch.from_numpy(counts.astype(np.int64)).to(DEV)
    col, row_ptr = filled(nnz, torch.int32, -1), filled(n_rows + 1, torch.int32, -1)
    fixed = None if counts is None else filled(n_rows, torch.uint8, 255)        # the launcher must clear it
    nat.call('dfl_mesh_csr', nat.MeshCsrArgs(keys=kd.data_ptr(), counts=nat.ptr(cd), col=col.data_ptr(),
                                             row_ptr=row_ptr.data_ptr(), fixed=nat.ptr(fixed), nnz=nnz, div=div,
                                             col_div=col_div, n_rows=n_rows), stream())
    same(head(row_ptr, n_rows + 1, 'row_ptr'), want_ptr, 'row_ptr')
    same(head(col, nnz, 'col'), want_col, 'col')
    if counts is not None:
        same(head(fixed, n_rows, 'fixed'), want_fixed.astype(np.uint8), 'fixed')
    return row_ptr, col, fixed


def gpu_neighbours(tris, V):
    uk, cnt = np.unique(R.edge_keys(tris, V), return_counts=True)
    return csr(uk, cnt, V, 1, V, *R.neighbours(tris, V))


def gpu_vertex_triangles(tris, V):
    return csr(np.sort(R.vt_keys(tris)), None, 3 * len(tris), 3, V, *R.vertex_triangles(tris, V))[:2]


@pytest.mark.parametrize('name', ['triangle', 'two', 'tetra', 'blob0', 'blob1', 'blob2', 'tetra+unused'])
def test_topology_and_csr(name):
    x, tris = mesh_case(name)
    V = len(x)
    for edge, vt in ((True, False), (False, True), (True, True)):
        topology(tris, V, edge, vt)
    row_ptr, col, fixed = R.neighbours(tris, V)
    empty = np.flatnonzero(np.diff(row_ptr) == 0)
    # the conditions, on the model
    if name == 'triangle':
        assert fixed.all()
    if name == 'two':
        assert fixed.all() and sorted(np.diff(row_ptr)) == [2, 2, 3, 3]
    if name == 'tetra':
        assert not fixed.any()
    if name.startswith('blob'):
        assert fixed.any() and not fixed.all() and len(col) > 4 * 256 and V % 256 and empty.size == 0
    if name == 'tetra+unused':
        assert empty.tolist() == [0, 3, 5, 7] and V == 8 and not fixed.any()
    gpu_neighbours(tris, V)
    gpu_vertex_triangles(tris, V)


# ---- smoother -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def graph(name):
    """The mesh's neighbour CSR on the device, built by the kernels and asserted against the model on the way."""
    x, tris = mesh_case(name)
    return gpu_neighbours(tris, len(x))


def gpu_smooth(x, g, iterations):
    V = len(x)
    xd = torch.from_numpy(x).to(DEV)
    t_a, t_b, acc = (torch.full((V, 4), NAN, dtype=torch.float32, device=DEV) for _ in range(3))
    out = filled(3 * V, torch.float32, NAN)
    a = nat.MeshSmoothArgs(x=xd.data_ptr(), row_ptr=g[0].data_ptr(), col=g[1].data_ptr(), fixed=g[2].data_ptr(),
                           t_a=t_a.data_ptr(), t_b=t_b.data_ptr(), acc=acc.data_ptr(), out=out.data_ptr(), V=V,
                           iterations=iterations)
    for n, v in enumerate(mesh.sinc_coefficients(iterations)):
        a.coef[n] = float(v)
    nat.call('dfl_mesh_smooth', a, stream())
    return head(out, 3 * V, 'out').reshape(V, 3)


@pytest.mark.parametrize('iterations', [1, 2, 3, 4, 25, nat.MESH_MAX_ITERS])
@pytest.mark.parametrize('name', ['blob0', 'tetra+unused'])
def test_smooth_forms(name, iterations):
    """N = 1: <true, true>; N = 2: <false, true> with T_0 read from x; N = 3: the first read of `dst` as T_{n-2}; N = 4:
    both ping-pong directions; 25: the default; 64: the most the argument block holds.  Measured kernel error / E32 on
    blob0: see DESIGN.md section 12."""
    assert nat.MESH_MAX_ITERS == 64
    x, tris = mesh_case(name)
    g = graph(name)
    got = gpu_smooth(x, g, iterations)
    assert not np.isnan(got).any(), 'NaN at vertices %s' % np.flatnonzero(np.isnan(got).any(1))[:8]
    ref, fixed = R.smooth(x, tris, iterations=iterations)
    ref32, _ = R.smooth(x, tris, iterations=iterations, dtype=np.float32)
    held = fixed | (np.diff(R.neighbours(tris, len(x))[0]) == 0)
    assert held.any() and not held.all()
    same(bits(got[held]), bits(x[held]), 'fixed and no-neighbour vertices')
    same(bits(gpu_smooth(x, g, iterations)), bits(got), 'two runs')
    e32 = float(np.abs(ref32 - ref).max())
    err = float(np.abs(got - ref).max())
    print('smooth %s N=%d: V=%d err %.3e E32 %.3e ratio %.3f' % (name, iterations, len(x), err, e32, err / e32))
    assert e32 > 0
    assert err <= 4 * e32, (name, iterations, err, e32)
    assert float(np.abs(ref - x).max()) > 1e3 * err                  # the filter moved the surface


# ---- transform ----------------------------------------------------------------------------------------------------------
def gpu_transform(xd, out, V, M):
    a = nat.MeshXformArgs(x=xd.data_ptr(), out=out.data_ptr(), V=V)
    for i, v in enumerate(M.reshape(-1)):
        a.M[i] = float(v)
    nat.call('dfl_mesh_transform', a, stream())
    return head(out, 3 * V, 'out').reshape(V, 3)


@pytest.mark.parametrize('V', [1, 257])
def test_transform_bound_and_in_place(V):
    """Points near 4000 on every axis, rotated, scaled by 1.25 and moved back to near the origin: the translation (about
    -5000 per axis) nearly cancels the rotated term, so a sum kept in fp32 anywhere would be off by thousands of ulp."""
    rng = np.random.default_rng(V)
    x = (4000 + rng.uniform(-2, 2, (V, 3))).astype(np.float32)
    w = np.array([0.3, -0.5, 0.8])
    w /= np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    A = 1.25 * (np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K)
    M = np.eye(4)
    M[:3, :3] = A
    M[:3, 3] = -A @ np.full(3, 4000.0) + [0.25, -0.5, 0.125]
    x64 = x.astype(np.float64)
    exact = x64 @ A.T + M[:3, 3]
    mag = np.abs(x64) @ np.abs(A).T + np.abs(M[:3, 3])
    assert np.abs(exact).max() < 2e-3 * mag.min()                   # the condition: the terms nearly cancel
    bound = 0.5 * np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64) + 2.0 ** -50 * mag
    xd = filled(3 * V, torch.float32, NAN)
    xd[:3 * V] = torch.from_numpy(x.reshape(-1)).to(DEV)
    got = gpu_transform(xd, filled(3 * V, torch.float32, NAN), V, M)
    over = np.abs(got - exact) / bound
    print('transform V=%d: max |got - exact| / bound = %.3f' % (V, float(over.max())))
    assert not np.isnan(got).any() and float(over.max()) <= 1.0
    same(bits(head(xd, 3 * V, 'x')), bits(x.reshape(-1)), 'input')
    same(bits(gpu_transform(xd, xd, V, M)), bits(got), 'in place')


# ---- normals ------------------------------------------------------------------------------------------------------------
def gpu_normals(pos, tris):
    V = len(pos)
    vt_ptr, vt_tri = gpu_vertex_triangles(tris, V)           # asserted against the model before the normals gather over them
    pd = torch.from_numpy(pos).to(DEV)
    td = torch.from_numpy(np.ascontiguousarray(tris)).to(DEV)
    out = filled(3 * V, torch.float32, NAN)
    nat.call('dfl_mesh_normals', nat.MeshNormalsArgs(pos=pd.data_ptr(), tris=td.data_ptr(), vt_ptr=vt_ptr.data_ptr(),
                                                     vt_tri=vt_tri.data_ptr(), normals=out.data_ptr(), V=V), stream())
    return head(out, 3 * V, 'normals').reshape(V, 3)


def test_normals_on_a_placed_surface():
    z, g = load_golden('viz3d_container'), load_golden('viz3d_scene')
    k = z['labels'].tolist().index(5)
    tris = z['tris_%d' % k]
    _, undo = R.normalize(z['verts_%d' % k])
    pos = R.apply(g['surf_pose'][k] @ g['surf_inner'][k] @ undo, z['smooth_%d' % k].astype(np.float32))
    V = len(pos)
    p = pos.astype(np.float64)[tris]
    fn = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    total, terms = np.zeros((V, 3)), np.zeros(V)
    for c in range(3):
        np.add.at(total, tris[:, c], fn)
        np.add.at(terms, tris[:, c], np.linalg.norm(fn, axis=1))
    assert V % 256 and np.all(np.linalg.norm(total, axis=1) > 1e-3 * terms)         # the condition: mild cancellation
    ref = R.normals(pos, tris, V)
    np.testing.assert_allclose(np.linalg.norm(ref, axis=1), 1, rtol=0, atol=1e-15)
    got = gpu_normals(pos, tris)
    err = float(np.abs(got - ref).max())
    print('normals: V=%d max error %.3e (bar %.3e)' % (V, err, 2.0 ** -23))
    assert not np.isnan(got).any() and err <= 2.0 ** -23


def test_normals_zero_cases():
    """Integer coordinates, so the fp64 cross products are exact.  Vertex 0: no triangle.  Vertex 1: only a triangle that
    repeats a vertex.  Vertices 2, 3, 4: only a triangle of collinear points.  Vertex 5: two triangles over the same
    points in opposite order (its partners 6, 7 and 8, 9 sit on the same two points).  Vertex 10: no triangle, last.
    All of them get exact zeros: not NaN, not what the buffer held."""
    pos = np.array([[9, 9, 9], [1, 2, 3], [0, 0, 0], [1, 1, 1], [3, 3, 3], [4, 0, 0], [5, 2, 0], [4, 3, 1], [5, 2, 0],
                    [4, 3, 1], [7, 7, 7], [2, 0, 5], [6, 1, 0]], np.float32)
    tris = np.array([[1, 11, 11], [2, 3, 4], [5, 6, 7], [5, 9, 8], [11, 12, 6]], np.int32)
    zero = [0, 1, 2, 3, 4, 5, 10]
    ref = R.normals(pos, tris, len(pos))
    others = np.setdiff1d(np.arange(len(pos)), zero)
    assert not ref[zero].any() and np.all(np.abs(np.linalg.norm(ref[others], axis=1) - 1) < 1e-15)   # the condition
    got = gpu_normals(pos, tris)
    same(got[zero], np.zeros((len(zero), 3), np.float32), 'zero normals')
    assert float(np.abs(got - ref).max()) <= 2.0 ** -23
