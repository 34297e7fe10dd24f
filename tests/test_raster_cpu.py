"""The rasteriser without a GPU: the numpy model (tests/raster_ref.py) against brute-force float64 point-in-triangle
tests on the snapped coordinates, the fill rule on a closed fan, the cameras and the ribbon of dfl_amd.raster, every
refusal of the C ABI (the library loads without a GPU and refuses before it launches), the dfl_sizeof entries, the
committed floor, and the new flags of examples/full_res_3d_viz.py."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'examples'))

import raster_floor as FL  # noqa: E402
import raster_ref as RR  # noqa: E402
import raster_scenes as SC  # noqa: E402
from dfl_amd import _native as nat, raster  # noqa: E402


def coverage_counts(sc):
    """Per sample how many triangles cover it (no depth test), and the snapped corners of every drawn triangle."""
    Ws, Hs = sc['W'] * sc['ssaa'], sc['H'] * sc['ssaa']
    c = RR.candidates(SC.recs(sc), Ws, Hs, sc['near'])
    return np.bincount(c['pix'], minlength=Ws * Hs).reshape(Hs, Ws), c


@pytest.mark.parametrize('name', ['pixel_centres', 'shared_edge', 'back_facing', 'interpenetrating', 'both_paths', 'perspective', '67x45'])
def test_model_coverage_against_brute_force(name):
    """Strictly inside (float64 on the integer coordinates, exact) is covered, strictly outside is not; samples on an edge
    are the fill rule's."""
    sc = SC.cases()[name]
    Ws, Hs = sc['W'] * sc['ssaa'], sc['H'] * sc['ssaa']
    jj, ii = np.mgrid[0:Hs, 0:Ws]
    Px, Py = 256.0 * ii + 128.0, 256.0 * jj + 128.0
    n_edge = 0
    for rec in SC.recs(sc):
        status, X, Y, A, _, _ = RR.vertex_stage(rec, Ws, Hs, sc['near'])
        for t in np.nonzero(status == RR.DRAWN)[0]:
            x, y = X[t].astype(np.float64), Y[t].astype(np.float64)
            cr = [(x[(k + 2) % 3] - x[(k + 1) % 3]) * (Py - y[(k + 1) % 3]) - (y[(k + 2) % 3] - y[(k + 1) % 3]) * (Px - x[(k + 1) % 3])
                  for k in range(3)]
            cr = np.stack(cr) * np.sign(A[t])
            inside, outside = np.all(cr > 0, 0), np.any(cr < 0, 0)
            one = RR.Rec(rec.pos, rec.tris[t:t + 1], np.eye(4))
            one.mvp = rec.mvp
            c = RR.candidates([one], Ws, Hs, sc['near'])
            got = np.bincount(c['pix'], minlength=Ws * Hs).reshape(Hs, Ws)
            assert got.max(initial=0) <= 1
            assert np.all(got[inside] == 1) and not np.any(got[outside])
            n_edge += int(np.sum(~inside & ~outside))
    if name in ('pixel_centres', 'shared_edge'):
        assert n_edge > 0                                    # the fixture does put sample centres on edges


def test_fill_rule_on_corners_at_pixel_centres():
    got, _ = coverage_counts(SC.cases()['pixel_centres'])
    # (4.5, 4.5) (30.5, 4.5) (4.5, 25.5): the top edge (row 4) and the left edge (column 4) are in, the hypotenuse's
    # centres are out, and so are the two far corners
    assert got[4, 4] == 1 and np.all(got[4, 4:30] == 1) and got[4, 30] == 0
    assert np.all(got[4:25, 4] == 1) and got[25, 4] == 0
    assert got[3].sum() == 0 and got[:, 3].sum() == 0


def test_shared_edge_is_covered_once():
    got, c = coverage_counts(SC.cases()['shared_edge'])
    assert got.max() == 1 and got.sum() > 500
    # the shared diagonal (5.5, 6.5) - (35.5, 36.5) passes through 29 sample centres: each belongs to exactly one of the two
    assert all(got[6 + k, 5 + k] == 1 for k in range(1, 30))


def test_closed_fan_covers_every_sample_once():
    """Eight triangles around a vertex on a sample centre, rim corners on sample centres too: the union is covered
    exactly once, the hub included, whatever the winding of each triangle."""
    hub = (20.5, 20.5, 0.5)
    rim = [(32.5, 20.5), (30.5, 30.5), (20.5, 34.5), (8.5, 32.5), (4.5, 20.5), (9.5, 9.5), (20.5, 5.5), (33.5, 8.5)]
    pos = [hub] + [(x, y, 0.5) for x, y in rim]
    tris = [[0, 1 + k, 1 + (k + 1) % 8] if k % 2 else [0, 1 + (k + 1) % 8, 1 + k] for k in range(8)]
    got, _ = coverage_counts(SC.scene([SC.spec(pos, tris)]))
    assert got.max() == 1 and got[20, 20] == 1
    # the polygon's interior by the even-odd rule in float64, away from its boundary
    jj, ii = np.mgrid[0:SC.H0, 0:SC.W0]
    x, y = ii + 0.5, jj + 0.5
    inside = np.zeros(x.shape, bool)
    dist = np.full(x.shape, np.inf)
    for k in range(8):
        (x0, y0), (x1, y1) = rim[k], rim[(k + 1) % 8]
        cross = ((y0 > y) != (y1 > y)) & (x < (x1 - x0) * (y - y0) / (y1 - y0 + 1e-300) + x0)
        inside ^= cross
        tt = np.clip(((x - x0) * (x1 - x0) + (y - y0) * (y1 - y0)) / ((x1 - x0) ** 2 + (y1 - y0) ** 2), 0, 1)
        dist = np.minimum(dist, np.hypot(x - x0 - tt * (x1 - x0), y - y0 - tt * (y1 - y0)))
    assert np.all(got[inside & (dist > 1e-6)] == 1) and not np.any(got[~inside & (dist > 1e-6)])


def test_model_counts_and_paths():
    c = SC.cases()
    assert SC.model(c['degenerate_and_offscreen'])['counts'].tolist() == [2, 0, 0, 2]
    assert SC.model(c['behind_near'])['counts'].tolist() == [1, 1, 0, 0]
    assert SC.model(c['guard_band'])['counts'].tolist() == [2, 0, 1, 0]
    assert SC.model(c['bad_index'])['counts'].tolist() == [1, 0, 0, 2]
    m = SC.model(c['box_threshold'])
    assert m['n_large'] == 2 and m['counts'][0] == 5            # 17-boxes go to the list, 16-boxes do not
    m = SC.model(c['both_paths'])
    assert m['n_large'] == 2 and m['counts'][0] > 250
    ids = SC.model(c['coplanar_duplicates'])['ids']
    # of two identical copies the lower id wins everywhere; the third copy lists the corners in reverse, sums its depth in
    # another order and may win a sample by a rounding
    assert 1 not in ids and set(np.unique(ids).tolist()) >= {-1, 0}
    assert SC.model(c['empty'])['ids'].min() == -1 == SC.model(c['empty'])['ids'].max()
    ids = SC.model(c['instances'])['ids']
    assert set(np.unique(ids).tolist()) == {-1, 0, 1, 2}
    for equal, want in ((False, 4095), (True, 0)):
        ids = SC.model(SC.contention(equal))['ids']
        assert ids[7, 10] == want and set(np.unique(ids).tolist()) == {-1, want}


def test_cameras():
    eye, target, up = np.array([3.0, -2.0, 7.0]), np.array([0.5, 0.25, -1.0]), np.array([0.1, 1.0, 0.2])
    V = raster.look_at(eye, target, up)
    assert np.abs(V[:3, :3] @ V[:3, :3].T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(V[:3, :3]) - 1) < 1e-12
    assert np.abs(V @ np.append(eye, 1) - [0, 0, 0, 1]).max() < 1e-9
    t = V @ np.append(target, 1)
    assert abs(t[0]) < 1e-9 and abs(t[1]) < 1e-9 and abs(t[2] + np.linalg.norm(target - eye)) < 1e-9
    assert (V[:3, :3] @ up)[1] > 0
    P = raster.perspective(50.0, 1.5, 0.5, 40.0)
    f = 1 / np.tan(np.radians(25.0))
    for p, depth in (((0.0, 0.0, -0.5), 0.0), ((0.0, 0.0, -40.0), 1.0)):
        c = P @ np.append(p, 1)
        assert abs(c[2] / c[3] - depth) < 1e-9 and abs(c[3] + p[2]) < 1e-12
    c = P @ np.array([1.2, -0.7, -3.0, 1.0])
    assert abs(c[0] / c[3] - f / 1.5 * 1.2 / 3.0) < 1e-9 and abs(c[1] / c[3] + f * 0.7 / 3.0) < 1e-9
    # from_intrinsics against K X / z, both signs of z; sample coordinates by the header's px, py
    K = np.array([[-1200.5, 0.3, 310.25], [0.0, -1180.0, 255.5], [0.0, 0.0, 1.0]])
    rows, cols = 480, 640
    for sign, pts in ((-1, [(10.0, -20.0, -600.0), (-35.0, 12.0, -900.0), (0.0, 0.0, -50.0)]),
                      (1, [(10.0, -20.0, 600.0), (-35.0, 12.0, 900.0)])):
        P = raster.from_intrinsics(K, rows, cols, 50.0, 1000.0, z_sign=sign)
        for X in pts:
            X = np.array(X)
            u, v = (K @ X / X[2])[:2]
            c = P @ np.append(X, 1)
            px, py = (c[0] / c[3] + 1) * 0.5 * cols, (1 - c[1] / c[3]) * 0.5 * rows
            assert abs(px - (u + 0.5)) < 1e-9 and abs(py - (v + 0.5)) < 1e-9, (px, u, py, v)
            d = abs(X[2])
            assert abs(c[3] - d) < 1e-12 and abs(c[2] / c[3] - 1000.0 * (d - 50.0) / (d * 950.0)) < 1e-9
    # frame: every point inside the view, the target in the middle
    pts = np.array([[0, 0, 0], [100, 20, -30], [40, -80, 10], [-20, 30, 60.0]])
    eye, target = raster.frame(pts, (0.3, -0.5, -1.0), 35.0, 4 / 3)
    V, P = raster.look_at(eye, target, (0, 1, 0)), raster.perspective(35.0, 4 / 3, 1.0, 1e4)
    c = (P @ V @ np.concatenate([pts, np.ones((4, 1))], 1).T).T
    assert np.all(np.abs(c[:, :2] / c[:, 3:]) < 1.0) and np.all(c[:, 3] > 0)
    assert np.abs(target - (pts.min(0) + pts.max(0)) / 2).max() < 1e-12
    for bad in (lambda: raster.perspective(0, 1, 1, 2), lambda: raster.perspective(30, 1, 2, 1), lambda: raster.look_at(eye, eye, up),
                lambda: raster.from_intrinsics(np.eye(4), 4, 4, 1, 2), lambda: raster.frame(np.zeros((0, 3)), (0, 0, 1), 30, 1)):
        with pytest.raises(nat.DflError):
            bad()


def test_ribbon_geometry():
    p0, p1, eye = np.array([1.0, 2.0, 3.0]), np.array([11.0, -4.0, 8.0]), np.array([3.0, 30.0, -5.0])
    pos, tris = raster.ribbon(p0, p1, 0.5, eye)
    assert pos.dtype == np.float32 and pos.shape == (4, 3) and tris.dtype == np.int32 and tris.tolist() == [[0, 1, 2], [0, 2, 3]]
    pos = pos.astype(np.float64)
    assert np.abs((pos[0] + pos[1]) / 2 - p0).max() < 1e-5 and np.abs((pos[2] + pos[3]) / 2 - p1).max() < 1e-5
    side = pos[1] - pos[0]
    assert abs(np.linalg.norm(side) - 0.5) < 1e-5 and np.abs(side - (pos[2] - pos[3])).max() < 1e-5
    assert abs(side @ (p1 - p0)) < 1e-4 and abs(side @ ((p0 + p1) / 2 - eye)) < 1e-4          # faces the eye
    with pytest.raises(nat.DflError):
        raster.ribbon(p0, p1, 0.5, p0 - (p1 - p0))                                              # seen end-on


def test_sizeof_entries_and_their_position():
    L = nat.lib()
    k = nat._SIZEOF_ORDER.index(nat.SimPatchGradnccArgs)
    assert nat._SIZEOF_ORDER[k + 1:k + 4] == [nat.RasterMesh, nat.RasterArgs, nat.SimGradnccBwdArgs]
    assert L.dfl_sizeof(k + 1) == C.sizeof(nat.RasterMesh) == 176 and L.dfl_sizeof(k + 2) == C.sizeof(nat.RasterArgs) == 104
    assert L.dfl_sizeof(len(nat._SIZEOF_ORDER)) == -1
    assert 'dfl_raster_draw' in nat.EXPORTS and 'dfl_raster_scratch_bytes' in nat.EXPORTS
    assert L.dfl_raster_draw.restype is C.c_int and L.dfl_raster_scratch_bytes.restype is C.c_int
    assert (nat.RASTER_UNLIT, nat.RASTER_TEXTURED, nat.RASTER_SMALL_BOX, nat.RASTER_MAX_SSAA, nat.RASTER_MAX_DIM) == (1, 2, RR.SMALL_BOX, 4, 16384)


def test_scratch_bytes():
    L = nat.lib()
    small = L.dfl_raster_scratch_bytes(64, 48, 1, 3)
    assert small > 64 * 48 * 12 and small % 8 == 0
    assert L.dfl_raster_scratch_bytes(64, 48, 2, 3) - small == 3 * 64 * 48 * 12
    assert L.dfl_raster_scratch_bytes(1, 1, 1, 0) > 0
    for bad in ((0, 4, 1, 1), (4, 0, 1, 1), (4, 4, 0, 1), (4, 4, 5, 1), (4, 4, 1, -1), (16385, 4, 1, 1), (8192, 4, 3, 1),
                (4, 4, 1, nat.RASTER_MAX_MESHES + 1)):
        assert L.dfl_raster_scratch_bytes(*bad) == -1 and b'bad sizes' in L.dfl_last_error(), bad
    assert L.dfl_raster_scratch_bytes(16384, 16384, 1, 1) == -1 and b'2^31' in L.dfl_last_error()      # 3 GiB


def test_c_abi_refuses_bad_arguments():
    """Every refusal comes back as -1 with a message, before anything is launched (there is no GPU here to launch on)."""
    L = nat.lib()
    P = 4096                                                  # never dereferenced: the checks come first
    need = L.dfl_raster_scratch_bytes(64, 48, 2, 2)

    def mesh(**k):
        m = nat.RasterMesh(**dict(dict(pos=P, nrm=P, uv=P, tris=P, tex=P, n_verts=3, n_tris=1, tw=4, th=4, first_prim=0, flags=0), **k))
        return m

    def run(recs, **k):
        arr = (nat.RasterMesh * max(len(recs), 1))(*recs)
        a = nat.RasterArgs(**dict(dict(meshes=C.addressof(arr), meshes_dev=P, scratch=P, rgb=P, ids=None, depth=None, counts=None,
                                       n_mesh=len(recs), W=64, H=48, ssaa=2, scratch_bytes=need, znear=0.5, ambient=0.2,
                                       diffuse=0.8), **k))
        rc = L.dfl_raster_draw(C.addressof(a), None)
        return rc, L.dfl_last_error()

    two = [mesh(), mesh(first_prim=1)]
    for kw, word in ((dict(scratch=None), b'required'), (dict(rgb=None), b'required'), (dict(meshes=None), b'required'),
                     (dict(meshes_dev=None), b'required'), (dict(W=0), b'bad sizes'), (dict(H=-1), b'bad sizes'),
                     (dict(ssaa=0), b'bad sizes'), (dict(ssaa=5), b'bad sizes'), (dict(W=8193), b'bad sizes'),
                     (dict(n_mesh=-1), b'bad sizes'), (dict(scratch_bytes=need - 1), b'short'), (dict(scratch_bytes=0), b'short'),
                     (dict(znear=0.0), b'znear'), (dict(znear=-1.0), b'znear'), (dict(znear=float('nan')), b'znear'),
                     (dict(scratch=P + 4), b'aligned')):
        rc, msg = run(two, **kw)
        assert rc == -1 and word in msg and b'dfl_raster_draw' in msg, (kw, msg)
    for bad, word in ((mesh(nrm=None), b'nrm'), (mesh(flags=nat.RASTER_TEXTURED, uv=None), b'textured'),
                      (mesh(flags=nat.RASTER_TEXTURED, tex=None), b'textured'), (mesh(flags=nat.RASTER_TEXTURED, tw=0), b'textured'),
                      (mesh(flags=nat.RASTER_TEXTURED | nat.RASTER_UNLIT, th=0), b'textured'), (mesh(pos=None), b'pos'),
                      (mesh(tris=None), b'tris'), (mesh(n_tris=-1), b'sizes'), (mesh(flags=4), b'flags'),
                      (mesh(first_prim=0xffffffff), b'first_prim')):
        rc, msg = run([bad, mesh(first_prim=0xfffffff0)])
        assert rc == -1 and word in msg and b'record 0' in msg, msg
    rc, msg = run([mesh(n_tris=5), mesh(first_prim=4)])          # overlapping id ranges
    assert rc == -1 and b'record 1' in msg and b'first_prim' in msg
    assert L.dfl_raster_draw(None, None) == -1 and b'null' in L.dfl_last_error()
    # what is allowed passes the checks and fails only at the launch, for want of a GPU
    if not torch.cuda.is_available():
        assert run([mesh(nrm=None, flags=nat.RASTER_UNLIT), mesh(first_prim=7, uv=None, tex=None)])[0] == nat.ERR_LAUNCH


def test_python_refuses_cpu_tensors_and_wrong_dtypes():
    pos, tris = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    with pytest.raises(nat.DflError, match='GPU'):
        raster.Mesh(pos, tris, unlit=True)
    with pytest.raises(nat.DflError, match='tensor'):
        raster.Mesh(pos.numpy(), tris, unlit=True)
    with pytest.raises(nat.DflError, match='float64'):
        raster.Mesh(pos.double(), tris, unlit=True)
    with pytest.raises(nat.DflError, match='raster.Mesh'):
        raster.render([(pos, tris)], (np.eye(4), np.eye(4)), 8, 8, device='cuda')
    with pytest.raises(nat.DflError, match='pair'):
        raster.render([], np.eye(4), 8, 8)
    with pytest.raises(nat.DflError, match='GPU'):
        raster.render([], (np.eye(4), np.eye(4)), 8, 8, device='cpu')


def test_the_committed_floor_is_the_models():
    with open(os.path.join(GOLDEN, 'floors', 'raster.json')) as f:
        committed = json.load(f)
    now = FL.measure()
    assert committed == json.loads(json.dumps(now))
    # the fixtures keep the float32 model inside the issue's bars by themselves
    for name, r in now['scenes'].items():
        assert r['winner_differs'] <= 0.001 * r['covered'], (name, r)
        assert r['differing_winners_that_are_near_ties'] == r['winner_differs'], (name, r)
        assert r['max_lit_level_error_f32'] <= 1, (name, r)


def test_png_flag_needs_a_path_and_the_rest_is_unchanged(capsys):
    import full_res_3d_viz as V
    assert V.main(['a.h5', 'spec', '0', '--png']) == 1
    assert capsys.readouterr().out.strip() == '--png needs a path'
    for bad in (['a.h5', 'spec', '0', '--png', 'x.png', '--view', 'top'], ['a.h5', 'spec', '0', '--png', 'x.png', '--ssaa', '5'],
                ['a.h5', 'spec', '0', '--png', 'x.png', '--png-size', '12'], ['a.h5', 'spec', '0', '--png', 'x.png', '--png-size', '0x4'],
                ['a.h5', 'spec', '0', '--ssaa', '2'], ['a.h5', 'spec', '0', '--png', 'x.png', '--png-size', '9000x10', '--ssaa', '2']):
        assert V.main(bad) == 1, bad
        assert capsys.readouterr().out.startswith('--')
    # without --png: as before
    assert V.main(['a.h5', 'spec']) == 1
    assert capsys.readouterr().out.strip() == V.USAGE.format(os.path.basename(sys.argv[0]))
    assert V.main(['a.h5', 'spec', '0', '--out']) == 1
    assert capsys.readouterr().out.strip() == '--out needs a path'
    assert V.options(['a.h5', '--out', 'o.glb', 'spec', '3']) == (['a.h5', 'spec', '3'], {'--out': 'o.glb'})
    assert V.options(['f', 's', '1', '--png', 'p.png', '--png-size', '160x120', '--view', 'source', '--ssaa', '1']) == \
        (['f', 's', '1'], {'--png': 'p.png', '--png-size': (160, 120), '--view': 'source', '--ssaa': 1})
