"""examples/full_res_3d_viz.py and dfl_amd.mesh without a GPU: the marching-cubes case table (regenerated, loops
covering every crossing edge once), the numpy model against the surface fixtures, the script's matrix chain and scene
geometry against the calls recorded from the reference (tests/golden/viz3d_scene.npz, tools/gen_viz3d_golden.py),
a GLB round trip, the usage line and the refusals."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'examples'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SURFACES = ['voxel', 'ball', 'torus', 'blob', 'container']
CONTAINER = os.path.join(GOLDEN, 'viz3d_container.h5')


# ---- case table -------------------------------------------------------------------------------------------------------
def test_table_regenerates_identically():
    import gen_mc_table
    from dfl_amd import mesh
    with open(mesh.TABLE_PATH) as f:
        assert f.read() == gen_mc_table.table_text()


def test_loops_cover_every_crossing_edge_once():
    import gen_mc_table as G
    from dfl_amd import mesh
    loops = mesh.case_loops()
    off, edges = mesh.case_table()
    for case in range(256):
        crossing = [e for e, (lo, hi) in enumerate(G.EDGES) if (case >> lo & 1) != (case >> hi & 1)]
        used = sorted(e for lp in loops[case] for e in lp)
        assert used == crossing, case
        assert all(lp[0] == min(lp) and len(lp) >= 3 for lp in loops[case]), case
        assert [lp[0] for lp in loops[case]] == sorted(lp[0] for lp in loops[case]), case
        assert off[case + 1] - off[case] == sum(len(lp) - 2 for lp in loops[case])
    assert off[0] == 0 and off[-1] == len(edges)


def test_table_winding_points_away_from_inside():
    """Each loop's fan area vector points away from the inside ends of its edges (counter-clockwise seen from outside)."""
    import gen_mc_table as G
    from dfl_amd import mesh
    for case in range(1, 255):
        for lp in mesh.case_loops()[case]:
            P = np.array([G.edge_mid(e) for e in lp])
            area = sum(np.cross(P[k] - P[0], P[k + 1] - P[0]) for k in range(1, len(P) - 1))
            inward = [G.corner_pos(lo if case >> lo & 1 else hi) - G.edge_mid(e) for e in lp for lo, hi in [G.EDGES[e]]]
            assert area @ np.mean(inward, 0) < 0, (case, lp)


# ---- numpy model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SURFACES)
def test_model_matches_the_fixtures(name):
    import mesh_ref as R
    z = load_golden('viz3d_' + name)
    for i, lab in enumerate(z['labels']):
        P, T, K = R.marching_cubes(z['volume'], int(lab))
        assert np.array_equal(K, z['keys_%d' % i]) and np.array_equal(T, z['tris_%d' % i])
        assert np.array_equal(P, z['verts_%d' % i])
        xn, _ = R.normalize(P)
        np.testing.assert_allclose(R.smooth(xn, T)[0], z['smooth_%d' % i], rtol=0, atol=1e-12)


@pytest.mark.parametrize('name', SURFACES)
def test_triangle_keys_and_block_counts_match_the_fixtures(name):
    import mesh_ref as R
    from dfl_amd import _native as nat
    z = load_golden('viz3d_' + name)
    labels = [int(v) for v in z['labels']]
    cells = int(np.prod(np.array(z['volume'].shape) - 1))
    counts, offsets, totals = R.block_counts(z['volume'], labels)
    nb = -(-cells // nat.MESH_MC_CELLS)
    assert counts.shape == offsets.shape == (nb, nat.MESH_MAX_LABELS) and totals.shape == (nat.MESH_MAX_LABELS + 1,)
    first = 0
    for i, lab in enumerate(labels):
        K, ntri = R.triangle_keys(z['volume'], lab)
        T = len(z['tris_%d' % i])
        assert K.shape == (T, 3) and K.dtype == np.int64 and ntri.shape == (cells,) and int(ntri.sum()) == T
        uniq, inv = np.unique(K.reshape(-1), return_inverse=True)
        assert np.array_equal(uniq, z['keys_%d' % i]) and np.array_equal(inv.reshape(-1, 3), z['tris_%d' % i])
        assert int(counts[:, i].sum()) == T and totals[i] == first
        assert np.array_equal(offsets[:, i], first + np.cumsum(counts[:, i]) - counts[:, i])
        assert np.array_equal(counts[:, i], [ntri[b * nat.MESH_MC_CELLS:(b + 1) * nat.MESH_MC_CELLS].sum() for b in range(nb)])
        first += T
    n = len(labels)
    assert totals[n] == first and np.all(totals[n + 1:] == -1)
    assert not counts[:, n:].any() and np.all(offsets[:, n:] == -1)          # written as 0; not written


def two_triangles():
    """A unit square cut along its diagonal 0-2, in the z = 0 plane, counter-clockwise seen from +z; vertex 4 unused."""
    P = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [5, 5, 5]], np.float32)
    return P, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def test_vertex_triangles_and_normals_by_hand():
    import mesh_ref as R
    P, T = two_triangles()
    assert R.vt_keys(T).tolist() == [0, 7, 14, 3, 16, 23]
    assert R.edge_keys(T, 5).tolist() == [1, 5, 7, 11, 10, 2, 2, 10, 13, 17, 15, 3]
    ptr, tri = R.vertex_triangles(T, 5)
    assert ptr.tolist() == [0, 2, 3, 5, 6, 6] and tri.tolist() == [0, 1, 0, 0, 1, 1]
    n = R.normals(P, T, 5)
    assert n.dtype == np.float64 and np.array_equal(n, [[0, 0, 1]] * 4 + [[0, 0, 0]])
    # tilt triangle 1 about the diagonal: vertex 3 up by 1.  Areas: (0, 0, 1) and (1, -1, 1) (twice the area vectors)
    P[3, 2] = 1
    n = R.normals(P, T, 5)
    s3, s6 = 1 / np.sqrt(3), 1 / np.sqrt(6)
    np.testing.assert_allclose(n, [[s6, -s6, 2 * s6], [0, 0, 1], [s6, -s6, 2 * s6], [s3, -s3, s3], [0, 0, 0]], rtol=0, atol=1e-15)
    # degenerate (a repeated vertex; collinear points) and exactly cancelling triangles give exact zeros
    Q = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 0, 1]], np.float32)
    assert not R.normals(Q, np.array([[0, 1, 2], [3, 3, 0]], np.int32), 4).any()
    assert not R.normals(Q, np.array([[0, 1, 3], [0, 3, 1]], np.int32), 4).any()


def test_neighbours_of_two_triangles():
    import mesh_ref as R
    _, T = two_triangles()
    ptr, col, fixed = R.neighbours(T, 5)
    assert ptr.tolist() == [0, 3, 5, 8, 10, 10] and col.tolist() == [1, 2, 3, 0, 2, 0, 1, 3, 0, 2]
    assert fixed.tolist() == [True, True, True, True, False]                  # every vertex is on a border edge


def test_vertex_without_neighbours_keeps_its_position():
    """A closed tetrahedron (no fixed vertex) plus one vertex that no triangle uses: the model leaves it in place bit for
    bit, in fp64 and in fp32, for every number of terms, and moves the others as it moves them without it."""
    import mesh_ref as R
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (5, 3)).astype(np.float32)
    T = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
    ptr, _, fixed = R.neighbours(T, 5)
    assert not fixed.any() and ptr[4] == ptr[5]
    for n in (1, 2, 3, 25):
        for dtype in (np.float64, np.float32):
            got, fx = R.smooth(x, T, iterations=n, dtype=dtype)
            assert np.all(np.isfinite(got)) and not fx.any()
            assert np.array_equal(got[4], x[4].astype(np.float64))
            assert np.array_equal(got[:4], R.smooth(x[:4], T, iterations=n, dtype=dtype)[0])
            assert np.abs(got[:4] - x[:4]).max() > 1e-2


def test_single_voxel_is_an_octahedron():
    import mesh_ref as R
    z = load_golden('viz3d_voxel')
    P, T = z['verts_0'], z['tris_0']
    assert len(P) == 6 and len(T) == 8
    assert sorted(map(tuple, P - 1.0)) == sorted([(0.5, 0, 0), (-0.5, 0, 0), (0, 0.5, 0), (0, -0.5, 0), (0, 0, 0.5), (0, 0, -0.5)])
    assert R.signed_volume(P, T) == 1.0 / 6.0
    assert set(R.edge_uses(T).values()) == {2} and R.euler(P, T) == 2


def test_closed_surfaces_of_the_model():
    import mesh_ref as R
    for name, chi in (('ball', 2), ('torus', 0)):
        z = load_golden('viz3d_' + name)
        P, T = z['verts_0'], z['tris_0']
        assert set(R.edge_uses(T).values()) == {2}, name
        assert R.euler(P, T) == chi, name
        assert R.signed_volume(P, T) > 0.8 * z['volume'].sum(), name


def test_filter_coefficients():
    from dfl_amd import mesh
    a = mesh.sinc_coefficients()
    th = np.arccos(0.95)
    n = np.arange(1, 26)
    c = np.concatenate([[th / np.pi], 2 * np.sin(n * th) / (n * np.pi)])
    w = 0.54 + 0.46 * np.cos(np.arange(26) * np.pi / 26)
    np.testing.assert_allclose(a, w * c / np.sum(w * c), rtol=1e-15, atol=0)
    assert abs(a.sum() - 1) < 1e-14


# ---- the script's host half against the reference's recorded calls ---------------------------------------------------
def geometry():
    import full_res_3d_viz as V
    src = V.Source(CONTAINER)
    try:
        return V.host_geometry(src, 'spec-a', 0, log=lambda s: None)
    finally:
        src.close()


def test_recorded_settings_are_the_restated_ones():
    from dfl_amd import mesh
    import full_res_3d_viz as V
    z = load_golden('viz3d_scene')
    assert int(z['flip_axis']) == 1 and int(z['flip_about_origin']) == 0
    assert z['smoother'].tolist() == [mesh.ITERATIONS, mesh.PASSBAND, 0, 0]
    assert z['surf_labels'].tolist() == [s[2] for s in V.SURFACES]
    assert z['surf_colors'].tolist() == [list(s[3]) for s in V.SURFACES]
    assert z['background'].tolist() == list(V.BACKGROUND)


def test_matrix_chain_matches_the_recorded_calls():
    import full_res_3d_viz as V
    z = load_golden('viz3d_scene')
    g = geometry()
    ny = g['volume'].shape[1]
    for k in range(4):
        rec = z['surf_pose'][k] @ z['surf_inner'][k] @ V.flip_y(ny)
        np.testing.assert_allclose(g['surface_xforms'][k], rec, rtol=0, atol=1e-9 * np.abs(rec).max())
        # flip + vertex_xform together: y -> y + 2 in index space
        inds_to_phys = z['surf_inner'][k] @ np.linalg.inv(V.vertex_xform(ny))
        shift = np.eye(4)
        shift[1, 3] = 2.0
        np.testing.assert_allclose(g['surface_xforms'][k], z['surf_pose'][k] @ inds_to_phys @ shift, rtol=0,
                                   atol=1e-9 * np.abs(rec).max())
        assert abs(np.linalg.det(V.vertex_xform(ny) @ V.flip_y(ny)) - 1.0) < 1e-15
    assert not np.allclose(z['surf_pose'][0], z['surf_pose'][2]) and not np.allclose(z['surf_pose'][2], z['surf_pose'][3])


def test_scene_geometry_matches_the_recorded_calls():
    import full_res_3d_viz as V
    z = load_golden('viz3d_scene')
    g = geometry()
    n3, n2 = len(z['land3d_names']), len(z['land2d_names'])
    assert list(g['lands_3d']) == z['land3d_names'].tolist()
    assert list(g['lands_2d']) == z['land2d_names'].tolist() == list(g['rays'])
    c, r, col = z['sphere_center'], z['sphere_radius'], z['sphere_color']
    np.testing.assert_allclose(np.array(list(g['lands_3d'].values())), c[:n3], rtol=1e-12, atol=1e-9)
    assert np.all(r[:n3] == V.LAND3D_RADIUS) and np.all(col[:n3] == V.LAND3D_COLOR)
    assert np.all(c[n3] == 0) and r[n3] == V.SOURCE_RADIUS and np.all(col[n3] == V.SOURCE_COLOR)
    np.testing.assert_allclose(np.array(list(g['lands_2d'].values())), c[n3 + 1:], rtol=1e-12, atol=1e-9)
    assert np.all(r[n3 + 1:] == V.LAND2D_RADIUS) and np.all(col[n3 + 1:] == V.LAND2D_COLOR)
    assert len(c) == n3 + 1 + n2
    np.testing.assert_allclose(np.array(list(g['rays'].values())), z['line_p2'], rtol=1e-12, atol=1e-9)
    assert np.all(z['line_p1'] == 0) and np.all(z['line_color'] == V.RAY_COLOR)
    np.testing.assert_allclose(g['detector'], z['det_points'], rtol=1e-12, atol=1e-9)
    assert np.array_equal(g['texture'], z['texture']) and z['texture'].dtype == np.uint8


def test_landmark_visibility_is_strict_against_size_minus_one():
    z = load_golden('viz3d_scene')
    vis = z['land2d_names'].tolist()
    assert 'FH-r' not in vis and 'GSN-l' not in vis            # exactly at cols - 1 / rows - 1
    assert 'IOF-r' in vis and 'GSN-r' in vis                    # (0, 0) and (cols - 1.5, rows - 1.5)


def test_constant_projection_gives_zero_texture(tmp_path):
    import full_res_3d_viz as V
    src = V.Source(CONTAINER)
    keys = {}
    for path in ['proj-params/' + k for k in src.children('proj-params')]:
        keys[path] = src.get(path)
    pfx = 'spec-a/projections/000/'
    for sub in ('gt-poses', 'gt-landmarks'):
        for k in src.children(pfx + sub):
            keys[pfx + sub + '/' + k] = src.get(pfx + sub + '/' + k)
    for k in src.children('spec-a/vol-landmarks'):
        keys['spec-a/vol-landmarks/' + k] = src.get('spec-a/vol-landmarks/' + k)
    for k in ('pixels', 'spacing', 'dir-mat', 'origin'):
        keys['spec-a/vol-seg/image/' + k] = src.get('spec-a/vol-seg/image/' + k)
    src.close()
    keys[pfx + 'image/pixels'] = np.full((64, 80), 3.5, np.float32)
    np.savez(tmp_path / 'c.npz', **keys)
    g = V.host_geometry(V.Source(str(tmp_path / 'c.npz')), 'spec-a', 0, log=lambda s: None)
    assert g['texture'].dtype == np.uint8 and not g['texture'].any()
    keys['spec-a/vol-seg/image/pixels'] = keys['spec-a/vol-seg/image/pixels'].astype(np.int16)
    np.savez(tmp_path / 'd.npz', **keys)
    from dfl_amd import _native as nat
    with pytest.raises(nat.DflError, match='int16'):
        V.host_geometry(V.Source(str(tmp_path / 'd.npz')), 'spec-a', 0, log=lambda s: None)


# ---- GLB ---------------------------------------------------------------------------------------------------------------
def test_glb_round_trip():
    from dfl_amd import gltf
    sc = gltf.Scene()
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], np.float32)
    m = sc.mesh('tri', P, np.array([[0, 1, 2]]), sc.material('red', (1, 0, 0)), normals=np.tile([[0, 0, 1.0]], (3, 1)))
    sc.node('tri', m, translation=[1, 2, 3], scale=[2, 2, 2])
    tex = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    q = sc.mesh('quad', P, None, sc.material('tex', (1, 1, 1), texture_rgb=tex), texcoords=P[:, :2], mode=gltf.LINES)
    sc.node('quad', q)
    sc.node('empty')
    data = sc.encode()
    assert len(data) % 4 == 0
    g = gltf.Glb(data)
    assert all(n % 4 == 0 for n in g.chunk_lengths)
    assert [n['name'] for n in g.doc['nodes']] == ['tri', 'quad', 'empty'] and 'mesh' not in g.node('empty')
    p = g.primitive('tri')
    assert np.array_equal(g.accessor(p['attributes']['POSITION']), P)
    acc = g.doc['accessors'][p['attributes']['POSITION']]
    assert acc['min'] == [0, 0, 0] and acc['max'] == [1, 2, 0]
    idx = g.doc['accessors'][p['indices']]
    assert idx['componentType'] == gltf.UINT32 and g.accessor(p['indices']).tolist() == [0, 1, 2]
    assert g.doc['materials'][p['material']]['doubleSided'] is True
    assert g.node('tri')['translation'] == [1, 2, 3] and g.node('tri')['scale'] == [2, 2, 2]
    assert g.primitive('quad')['mode'] == gltf.LINES
    assert np.array_equal(g.image(0), tex)
    assert g.doc['samplers'][0] == {'magFilter': gltf.NEAREST, 'minFilter': gltf.NEAREST}


# ---- command line and refusals ----------------------------------------------------------------------------------------
def test_usage_and_exit_status():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'full_res_3d_viz.py'), 'a.h5', 'spec'],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1
    assert r.stdout.strip() == 'Usage: full_res_3d_viz.py <HDF5 full-res data file> <specimen ID> <projection index>'


def test_cpu_tensors_and_bad_dtypes_are_refused():
    from dfl_amd import _native as nat, mesh
    with pytest.raises(nat.DflError, match='int16'):
        mesh.label_surfaces(torch.zeros(4, 4, 4, dtype=torch.int16), [1])
    with pytest.raises(nat.DflError, match='GPU'):
        mesh.label_surfaces(torch.zeros(4, 4, 4, dtype=torch.uint8), [1])
    v, t = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    for fn in (lambda: mesh.smooth(v, t), lambda: mesh.vertex_normals(v, t), lambda: mesh.transform(v, np.eye(4))):
        with pytest.raises(nat.DflError, match='GPU'):
            fn()
    with pytest.raises(nat.DflError, match='float64'):
        mesh.smooth(v.double(), t)


def test_c_abi_refuses_bad_arguments():
    from dfl_amd import _native as nat
    L = nat.lib()
    a = nat.MeshMcArgs(volume=16, tri_off=16, tri_edges=16, block_counts=16, block_offsets=16, totals=16, nx=1300,
                       ny=1300, nz=1300, n_labels=1)
    assert L.dfl_mesh_mc_count(C.addressof(a), None) == -1
    assert b'2^31' in L.dfl_last_error()
    a.nx, a.ny, a.nz, a.n_labels = 8, 8, 8, 5
    assert L.dfl_mesh_mc_count(C.addressof(a), None) == -1
    a.n_labels = 1
    assert L.dfl_mesh_mc_emit(C.addressof(a), None) == -1            # no keys
    s = nat.MeshSmoothArgs(x=16, row_ptr=16, col=16, fixed=16, out=16, V=10, iterations=65)
    assert L.dfl_mesh_smooth(C.addressof(s), None) == -1
    c = nat.MeshCsrArgs(keys=16, col=16, row_ptr=16, nnz=0, div=1, col_div=1, n_rows=1)
    assert L.dfl_mesh_csr(C.addressof(c), None) == -1
