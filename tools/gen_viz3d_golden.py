"""Writes the fixtures of examples/full_res_3d_viz.py and dfl_amd.mesh: tests/golden/viz3d_*.

Dev-only.  Two kinds of data:

  Reference-derived scene geometry.  A small container in the full-resolution layout (volume 56 x 48 x 40 with labels
  1 - 6, some touching the border; three distinct rigid poses; a 64 x 80 projection; landmarks inside, outside and
  exactly at cols - 1 and rows - 1) is written with dfl_amd.h5lite to tests/golden/viz3d_container.h5.  The reference's
  unmodified examples_dataset/full_res_3d_viz.py then runs under runpy with stand-in `vtk` and `h5py` modules (h5py
  backed by the container through h5lite) and np.mat = np.asmatrix; the stand-ins record every call that places
  something in the scene.  Only the recording is kept: viz3d_scene.npz.
    surf_labels [4], surf_colors [4, 3], surf_inner [4, 4, 4] (inds_to_phys * vertex_xform, the first xform_mesh),
    surf_pose [4, 4, 4] (the second xform_mesh), flip_axis, flip_about_origin, smoother (iterations, passband,
    boundary smoothing, feature edge smoothing), decimation, sphere_center [S, 3], sphere_radius [S],
    sphere_color [S, 3], line_p1 / line_p2 [L, 3], line_color [L, 3], det_points [4, 3], tcoords [4, 2],
    texture [rows, cols] uint8, background [3], land3d_names, land2d_names (the visible ones, in scene order).

  Self-defined surfaces.  tests/mesh_ref.py (numpy marching cubes from data/mc_cases.txt, fp64 filter) gives
  viz3d_{voxel,ball,torus,blob,container}.npz: volume, labels, and per label i verts_i, tris_i, keys_i, and the fp64
  filter output smooth_i of the model's own normalised positions.

    python tools/gen_viz3d_golden.py /path/to/reference        # the reference checkout (read only)
"""
import os
import runpy
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import dfl_amd  # noqa: E402,F401
from dfl_amd import h5lite  # noqa: E402
import mesh_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CONTAINER = os.path.join(GOLDEN, 'viz3d_container.h5')
SPEC = 'spec-a'
ROWS, COLS = 64, 80
NZ, NY, NX = 56, 48, 40
LABELS = [1, 2, 5, 6]


def rigid(rng, t_scale):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    H = np.eye(4)
    H[:3, :3] = Rm
    H[:3, 3] = rng.uniform(-t_scale, t_scale, 3)
    return H


def label_volume(rng):
    z, y, x = np.mgrid[:NZ, :NY, :NX].astype(np.float64)
    vol = np.zeros((NZ, NY, NX), np.uint8)
    blobs = [(1, (12, 14, 20), (9, 8, 11)),     # left hemipelvis
             (2, (27, 14, 20), (8, 9, 10)),     # right hemipelvis, touches nothing
             (3, (20, 40, 52), (6, 7, 8)),      # touches y and z ends
             (4, (2, 30, 8), (5, 6, 9)),        # touches x = 0 and z = 0
             (5, (10, 34, 40), (5, 8, 14)),     # left femur, touches z = nz - 1
             (6, (33, 35, 30), (5, 7, 12))]     # right femur, touches x = nx - 1
    for lab, (cx, cy, cz), (rx, ry, rz) in blobs:
        noise = rng.normal(scale=0.08, size=vol.shape)
        inside = ((x - cx) / rx) ** 2 + ((y - cy) / ry) ** 2 + ((z - cz) / rz) ** 2 + noise <= 1.0
        vol[inside] = lab
    return vol


def write_container(path, rng):
    K = np.array([[-5257.73, 0.0, COLS / 2 - 1.3], [0.0, -5257.73, ROWS / 2 + 0.7], [0.0, 0.0, 1.0]])
    ext = rigid(rng, 30.0)
    lands = {'FH-l': (12.25, 30.5), 'FH-r': (COLS - 1, 20.0), 'GSN-l': (40.0, ROWS - 1), 'GSN-r': (COLS - 1.5, ROWS - 1.5),
             'IOF-l': (-0.5, 10.0), 'IOF-r': (0.0, 0.0), 'MOF-l': (COLS + 3.0, 5.0), 'MOF-r': (33.0, -2.0)}
    vol = label_volume(rng)
    with h5lite.File(path, 'w') as f:
        f['proj-params/extrinsic'] = ext
        f['proj-params/intrinsic'] = K
        f['proj-params/num-cols'] = np.int64(COLS)
        f['proj-params/num-rows'] = np.int64(ROWS)
        f['proj-params/pixel-col-spacing'] = np.float64(0.194)
        f['proj-params/pixel-row-spacing'] = np.float64(0.194)
        g = SPEC + '/projections/000/'
        img = (rng.normal(size=(ROWS, COLS)) * 0.3 + np.linspace(0, 2, COLS)[None, :]).astype(np.float32)
        f.create_dataset(g + 'image/pixels', data=img, chunks=(ROWS, COLS), compression='gzip')
        for k, name in enumerate(sorted(lands)):
            v = np.array(lands[name], np.float32)
            f[g + 'gt-landmarks/' + name] = v if k % 2 == 0 else v.reshape(2, 1)
        f[g + 'gt-poses/cam-to-pelvis-vol'] = rigid(rng, 40.0)
        f[g + 'gt-poses/cam-to-left-femur-vol'] = rigid(rng, 40.0)
        f[g + 'gt-poses/cam-to-right-femur-vol'] = rigid(rng, 40.0)
        for name in sorted(lands):
            f[SPEC + '/vol-landmarks/' + name] = rng.uniform(0, 40, 3).reshape(3, 1)
        v = SPEC + '/vol-seg/image/'
        f.create_dataset(v + 'pixels', data=vol, chunks=(8, NY, NX), compression='gzip')
        f[v + 'spacing'] = np.array([0.8, 0.75, 1.1])
        d = rigid(rng, 0.0)[:3, :3]
        f[v + 'dir-mat'] = d
        f[v + 'origin'] = np.array([-20.0, 15.5, 120.25])
    return vol


# ---- the recording stand-ins ---------------------------------------------------------------------------------------
REC = {}


def _pt(*a):
    v = a[0] if len(a) == 1 else a
    return [float(np.asarray(c).reshape(-1)[0]) for c in v]


class _Obj:
    """Any VTK object the scene does not depend on: every method accepts anything and returns another such object."""

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return lambda *a, **k: _Obj()


class vtkImageImport(_Obj):
    def SetImportVoidPointer(self, arr, save=True):
        self.arr = np.array(arr)

    def GetOutput(self):
        return types.SimpleNamespace(arr=self.arr)


class vtkImageFlip(_Obj):
    def SetInputData(self, img):
        self.img = img

    def SetFilteredAxis(self, ax):
        REC['flip_axis'] = ax

    def FlipAboutOriginOff(self):
        REC['flip_about_origin'] = 0

    def GetOutput(self):
        return self.img


class vtkDiscreteMarchingCubes(_Obj):
    def __init__(self):
        self.labels = []

    def SetValue(self, i, v):
        self.labels.append(v)

    def GetOutput(self):
        return types.SimpleNamespace(labels=self.labels, xforms=[])


class vtkWindowedSincPolyDataFilter(_Obj):
    def SetInputData(self, m):
        self.m = m

    def SetNumberOfIterations(self, n):
        REC['smoother'][0] = n

    def SetPassBand(self, p):
        REC['smoother'][1] = p

    def SetBoundarySmoothing(self, b):
        REC['smoother'][2] = bool(b)

    def SetFeatureEdgeSmoothing(self, b):
        REC['smoother'][3] = bool(b)

    def GetOutput(self):
        return self.m


class vtkQuadricDecimation(vtkWindowedSincPolyDataFilter):
    def SetTargetReduction(self, r):
        REC['decimation'] = r


class vtkMatrix4x4(_Obj):
    def __init__(self):
        self.M = np.eye(4)

    def SetElement(self, i, j, v):
        self.M[i, j] = float(v)


class vtkMatrixToHomogeneousTransform(_Obj):
    def SetInput(self, m):
        self.M = m.M


class vtkTransformPolyDataFilter(_Obj):
    def SetInputData(self, m):
        self.m = m

    def SetTransform(self, t):
        self.M = t.M.copy()

    def GetOutput(self):
        return types.SimpleNamespace(labels=self.m.labels, xforms=self.m.xforms + [self.M])


class vtkSphereSource(_Obj):
    def SetCenter(self, *c):
        self.c = _pt(*c)

    def SetRadius(self, r):
        self.r = float(r)

    def GetOutput(self):
        return types.SimpleNamespace(kind='sphere', c=self.c, r=self.r)


class vtkLineSource(_Obj):
    def SetPoint1(self, *p):
        self.p1 = _pt(*p)

    def SetPoint2(self, *p):
        self.p2 = _pt(*p)

    def GetOutput(self):
        return types.SimpleNamespace(kind='line', p1=self.p1, p2=self.p2)


class vtkPoints(_Obj):
    def InsertNextPoint(self, *p):
        REC['det_points'].append(_pt(*p))


class vtkFloatArray(_Obj):
    def InsertNextTuple(self, t):
        REC['tcoords'].append([float(v) for v in t])


class vtkTexture(_Obj):
    def SetInputData(self, img):
        REC['texture'] = img.arr


class vtkPolyDataMapper(_Obj):
    def SetInputData(self, d):
        self.d = d


class _Prop(_Obj):
    color = None

    def SetColor(self, *c):
        self.color = [float(v) for v in c]


class vtkActor(_Obj):
    def __init__(self):
        self.prop = _Prop()

    def SetMapper(self, m):
        self.mapper = m

    def GetProperty(self):
        return self.prop


class vtkRenderer(_Obj):
    def AddViewProp(self, a):
        if isinstance(a, vtkActor):
            REC['actors'].append(a)

    def SetBackground(self, *c):
        REC['background'] = [float(v) for v in c]


class vtkCubeAxesActor(_Obj):
    VTK_GRID_LINES_FURTHEST = 2


def vtk_module():
    m = types.ModuleType('vtk')
    for name in ('VTK_FLOAT', 'VTK_UNSIGNED_CHAR'):
        setattr(m, name, name)
    here = globals()
    for name in ('vtkImageData', 'vtkRenderWindow', 'vtkRenderWindowInteractor', 'vtkInteractorStyleTrackballCamera',
                 'vtkQuad', 'vtkCellArray', 'vtkPolyData'):
        setattr(m, name, type(name, (_Obj,), {}))
    for name, v in here.items():
        if name.startswith('vtk') and isinstance(v, type):
            setattr(m, name, v)
    return m


def h5py_module():
    m = types.ModuleType('h5py')
    m.File = lambda path, mode='r': h5lite.File(path, 'r')
    return m


def record(ref_root, container):
    REC.clear()
    REC.update(smoother=[None] * 4, det_points=[], tcoords=[], actors=[])
    saved = {k: sys.modules.get(k) for k in ('vtk', 'h5py')}
    sys.modules['vtk'], sys.modules['h5py'] = vtk_module(), h5py_module()
    had_mat = hasattr(np, 'mat')
    np.mat = np.asmatrix
    argv = sys.argv
    sys.argv = ['full_res_3d_viz.py', container, SPEC, '0']
    try:
        runpy.run_path(os.path.join(ref_root, 'examples_dataset', 'full_res_3d_viz.py'), run_name='__main__')
    finally:
        sys.argv = argv
        if not had_mat:
            del np.mat
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    out = {k: REC[k] for k in ('flip_axis', 'flip_about_origin', 'background', 'decimation')}
    out['smoother'] = np.array(REC['smoother'], np.float64)
    out['det_points'] = np.array(REC['det_points'])
    out['tcoords'] = np.array(REC['tcoords'])
    out['texture'] = REC['texture']
    def kind(a):
        d = a.mapper.d
        return vars(d).get('kind', 'surface') if isinstance(d, types.SimpleNamespace) else 'plane'

    surf = [a for a in REC['actors'] if kind(a) == 'surface']
    spheres = [a for a in REC['actors'] if kind(a) == 'sphere']
    lines = [a for a in REC['actors'] if kind(a) == 'line']
    out['surf_labels'] = np.array([a.mapper.d.labels[0] for a in surf])
    out['surf_colors'] = np.array([a.prop.color for a in surf])
    out['surf_inner'] = np.array([a.mapper.d.xforms[0] for a in surf])
    out['surf_pose'] = np.array([a.mapper.d.xforms[1] for a in surf])
    out['sphere_center'] = np.array([a.mapper.d.c for a in spheres])
    out['sphere_radius'] = np.array([a.mapper.d.r for a in spheres])
    out['sphere_color'] = np.array([a.prop.color for a in spheres])
    out['line_p1'] = np.array([a.mapper.d.p1 for a in lines])
    out['line_p2'] = np.array([a.mapper.d.p2 for a in lines])
    out['line_color'] = np.array([a.prop.color for a in lines])
    assert len(surf) + len(spheres) + len(lines) + 1 == len(REC['actors'])
    return out


def surface_fixture(name, vol, labels):
    d = {'volume': vol, 'labels': np.array(labels, np.int32)}
    for i, lab in enumerate(labels):
        P, T, K = R.marching_cubes(vol, lab)
        d['verts_%d' % i], d['tris_%d' % i], d['keys_%d' % i] = P, T, K
        if len(T):
            xn, _ = R.normalize(P)
            d['smooth_%d' % i] = R.smooth(xn, T)[0]
        print('  %s label %d: %d vertices, %d triangles' % (name, lab, len(P), len(T)))
    np.savez_compressed(os.path.join(GOLDEN, 'viz3d_%s.npz' % name), **d)


def main(argv):
    if len(argv) != 1:
        print(__doc__)
        return 1
    rng = np.random.default_rng(20260415)
    vol = write_container(CONTAINER, rng)
    rec = record(argv[0], CONTAINER)
    with h5lite.File(CONTAINER, 'r') as f:
        g = f[SPEC + '/projections/000/gt-landmarks']
        names = list(g)
        vis = [n for n in names if 0 <= float(np.asarray(g[n][()]).reshape(-1)[0]) < COLS - 1
               and 0 <= float(np.asarray(g[n][()]).reshape(-1)[1]) < ROWS - 1]
    rec['land3d_names'] = np.array(sorted(f3 for f3 in names))
    rec['land2d_names'] = np.array(vis)
    assert len(rec['sphere_radius']) == len(names) + 1 + len(vis) and len(rec['line_p1']) == len(vis)
    np.savez_compressed(os.path.join(GOLDEN, 'viz3d_scene.npz'), **rec)
    print('recorded %d surfaces, %d spheres, %d lines; visible 2D landmarks %s' %
          (len(rec['surf_labels']), len(rec['sphere_radius']), len(rec['line_p1']), vis))
    one = np.zeros((3, 3, 3), np.uint8)
    one[1, 1, 1] = 1
    surface_fixture('voxel', one, [1])
    surface_fixture('ball', R.ball(20, 7.2), [1])
    surface_fixture('torus', R.torus(28, 8, 3.2), [1])
    blob = np.random.default_rng(7).integers(0, 4, (14, 17, 19)).astype(np.uint8)
    blob[np.random.default_rng(8).random(blob.shape) < 0.3] = 0
    surface_fixture('blob', blob, [1, 2, 3])
    surface_fixture('container', vol, LABELS)
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
