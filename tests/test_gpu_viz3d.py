"""dfl_amd.mesh and examples/full_res_3d_viz.py on the GPU: marching cubes bit-identical to the numpy model's
fixtures (tests/golden/viz3d_*.npz), closed surfaces watertight with the right Euler characteristic and oriented
outward, the windowed-sinc filter against the fp64 model on the same mesh, fixed vertices and run-to-run bits, the
fp64 transform, the normals, and the example end to end on the h5lite container against the calls recorded from the
reference."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, 'tests'))
import mesh_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SURFACES = ['voxel', 'ball', 'torus', 'blob', 'container']


def gpu_surfaces(z):
    from dfl_amd import mesh
    return mesh.label_surfaces(torch.from_numpy(z['volume']).cuda(), z['labels'].tolist())


@pytest.mark.parametrize('name', SURFACES)
def test_marching_cubes_is_bit_identical(name):
    z = load_golden('viz3d_' + name)
    for i, (v, t) in enumerate(gpu_surfaces(z)):
        v, t = v.cpu().numpy(), t.cpu().numpy()
        assert t.dtype == np.int32 and v.dtype == np.float32
        assert np.array_equal(t, z['tris_%d' % i]), (name, i, t.shape, z['tris_%d' % i].shape)
        assert np.array_equal(v.view(np.int32), z['verts_%d' % i].view(np.int32)), (name, i)


def test_absent_label_gives_an_empty_surface():
    from dfl_amd import mesh
    z = load_golden('viz3d_ball')
    (v, t), (v2, t2) = mesh.label_surfaces(torch.from_numpy(z['volume']).cuda(), [7, 1])
    assert v.shape == (0, 3) and t.shape == (0, 3)
    assert np.array_equal(t2.cpu().numpy(), z['tris_0'])


@pytest.mark.parametrize('name,chi', [('ball', 2), ('torus', 0), ('voxel', 2)])
def test_closed_surfaces_are_watertight_and_outward(name, chi):
    from dfl_amd import mesh
    z = load_golden('viz3d_' + name)
    (v, t), = gpu_surfaces(z)
    P, T = v.cpu().numpy(), t.cpu().numpy()
    assert set(R.edge_uses(T).values()) == {2}
    assert R.euler(P, T) == chi
    assert R.signed_volume(P, T) > 0
    if name != 'voxel':
        xs, undo = mesh.smooth(v, t)
        pos = mesh.transform(xs, undo)
        n = mesh.vertex_normals(pos, t).cpu().numpy()
        p = pos.cpu().numpy().astype(np.float64)
        c = p.mean(0)
        radial = p - c
        if name == 'torus':                     # away from the tube's centre circle in the z = c plane
            ring = radial.copy()
            ring[:, 2] = 0
            ring *= 8.0 / np.linalg.norm(ring, axis=1, keepdims=True)
            radial = radial - ring
        cosang = np.einsum('ij,ij->i', n, radial) / np.linalg.norm(radial, axis=1)
        assert np.all(np.abs(np.linalg.norm(n, axis=1) - 1) < 1e-6)
        assert np.mean(cosang) > 0.9 and np.mean(cosang > 0) > 0.99, (name, float(cosang.min()))


@pytest.mark.parametrize('name', ['ball', 'torus', 'blob', 'container'])
def test_smoothing_against_the_fp64_model(name):
    from dfl_amd import mesh
    z = load_golden('viz3d_' + name)
    for i, (v, t) in enumerate(gpu_surfaces(z)):
        xn, _ = mesh.normalize(v)
        xs, _ = mesh.smooth(v, t)
        xs2, _ = mesh.smooth(v, t)
        got, x = xs.cpu().numpy(), xn.cpu().numpy()
        assert np.array_equal(got.view(np.int32), xs2.cpu().numpy().view(np.int32)), 'two runs differ'
        ref, fixed = R.smooth(x, t.cpu().numpy())
        assert np.array_equal(got[fixed].view(np.int32), x[fixed].view(np.int32)), 'fixed vertices moved'
        diag = float(np.linalg.norm(x.max(0).astype(np.float64) - x.min(0)))
        err = float(np.abs(got - ref).max())
        assert err <= 1e-5 * diag, (name, i, err, diag)
        assert float(np.abs(ref - x).max()) > 1e3 * err          # the filter moved the surface
        if name == 'blob':
            assert fixed.any()                                    # open at the volume border


def test_transform_within_two_ulp_and_normals():
    from dfl_amd import mesh
    z = load_golden('viz3d_container')
    g = load_golden('viz3d_scene')
    (v, t), = mesh.label_surfaces(torch.from_numpy(z['volume']).cuda(), [5])
    xs, undo = mesh.smooth(v, t)
    M = g['surf_pose'][2] @ g['surf_inner'][2] @ undo
    got = mesh.transform(xs, M).cpu().numpy()
    x = xs.cpu().numpy().astype(np.float64)
    exact = x @ M[:3, :3].T + M[:3, 3]
    ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    assert float((np.abs(got - exact) / ulp).max()) <= 2.0
    n = mesh.vertex_normals(torch.from_numpy(got).cuda(), t).cpu().numpy()
    p = got.astype(np.float64)[t.cpu().numpy()]
    fn = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    acc = np.zeros((len(got), 3))
    for k in range(3):
        np.add.at(acc, t.cpu().numpy()[:, k], fn)
    ref = acc / np.linalg.norm(acc, axis=1, keepdims=True)
    assert float(np.abs(n - ref).max()) < 1e-5


def test_example_end_to_end(tmp_path):
    from dfl_amd import gltf
    out = tmp_path / 'scene.glb'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'full_res_3d_viz.py'),
                        os.path.join(GOLDEN, 'viz3d_container.h5'), 'spec-a', '0', '--out', str(out)],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[:10] == [
        'reading projection parameters...', 'reading projection...', 'reading GT poses...', 'reading GT 2D landmarks...',
        'reading 3D landmarks...', 'reading 3D segmentation...', 'creating left hemipelvis mesh...',
        'creating right hemipelvis mesh...', 'creating left femur mesh...', 'creating right femur mesh...']
    g = gltf.Glb(str(out))
    z = load_golden('viz3d_scene')
    # texture bytes and texel placement: texel (r, c) at the detector point of index (c, r)
    tex = g.image(0)
    assert np.array_equal(tex[:, :, 0], z['texture']) and np.array_equal(tex[:, :, 2], z['texture'])
    prim = g.primitive('detector')
    P = g.accessor(prim['attributes']['POSITION']).astype(np.float64)
    UV = g.accessor(prim['attributes']['TEXCOORD_0']).astype(np.float64)
    np.testing.assert_allclose(P, z['det_points'], rtol=1e-6, atol=1e-6)
    sampler = g.doc['samplers'][g.doc['textures'][0]['sampler']]
    assert sampler['magFilter'] == gltf.NEAREST and sampler['minFilter'] == gltf.NEAREST
    H, W = z['texture'].shape
    D0, Dc, Dr = z['det_points'][0], z['det_points'][3] - z['det_points'][0], z['det_points'][1] - z['det_points'][0]
    basis = np.stack([P[3] - P[0], P[1] - P[0]], 1)
    for r_ in range(0, H, 7):
        for c_ in range(0, W, 9):
            d = D0 + c_ / (W - 1) * Dc + r_ / (H - 1) * Dr
            wc, wr = np.linalg.lstsq(basis, d - P[0], rcond=None)[0]
            u, v = UV[0] + wc * (UV[3] - UV[0]) + wr * (UV[1] - UV[0])
            assert (int(v * H), int(u * W)) == (r_, c_)
    # spheres
    n3, names2 = len(z['land3d_names']), z['land2d_names'].tolist()
    nodes = [g.node('vol-landmark/' + n) for n in z['land3d_names'].tolist()] + [g.node('source')] + \
            [g.node('proj-landmark/' + n) for n in names2]
    np.testing.assert_allclose([n['translation'] for n in nodes], z['sphere_center'], rtol=1e-12, atol=1e-9)
    assert [n['scale'][0] for n in nodes] == z['sphere_radius'].tolist()
    colors = [g.doc['materials'][g.doc['meshes'][n['mesh']]['primitives'][0]['material']]['pbrMetallicRoughness']
              ['baseColorFactor'][:3] for n in nodes]
    np.testing.assert_allclose(colors, z['sphere_color'])
    # rays
    for k, n in enumerate(names2):
        p = g.primitive('ray/' + n)
        assert p['mode'] == gltf.LINES
        ends = g.accessor(p['attributes']['POSITION'])
        np.testing.assert_allclose(ends, np.stack([z['line_p1'][k], z['line_p2'][k]]), rtol=1e-6, atol=1e-6)
    # surfaces: the model's mesh through the recorded matrices
    zc = load_golden('viz3d_container')
    ny = zc['volume'].shape[1]
    F = np.eye(4)
    F[1, 1], F[1, 3] = -1, ny - 1
    for k, name in enumerate(['left-hemipelvis', 'right-hemipelvis', 'left-femur', 'right-femur']):
        p = g.primitive(name)
        assert np.array_equal(g.accessor(p['indices']).reshape(-1, 3), zc['tris_%d' % k])
        got = g.accessor(p['attributes']['POSITION']).astype(np.float64)
        xn, undo = R.normalize(zc['verts_%d' % k])
        M = z['surf_pose'][k] @ z['surf_inner'][k] @ F @ undo
        exp = zc['smooth_%d' % k] @ M[:3, :3].T + M[:3, 3]
        ext = float(np.linalg.norm(exp.max(0) - exp.min(0)))
        assert float(np.abs(got - exp).max()) <= 1e-5 * ext, name
        acc = g.doc['accessors'][p['attributes']['POSITION']]
        np.testing.assert_allclose(acc['min'], got.min(0)) and np.testing.assert_allclose(acc['max'], got.max(0))
        assert 'NORMAL' in p['attributes']
        col = g.doc['materials'][p['material']]['pbrMetallicRoughness']['baseColorFactor'][:3]
        assert col == z['surf_colors'][k].tolist()
    assert g.doc['scenes'][0]['extras']['background'] == z['background'].tolist()
