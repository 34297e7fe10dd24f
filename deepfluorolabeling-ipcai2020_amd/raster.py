"""A triangle rasteriser on the GPU: the picture the reference's full_res_3d_viz.py shows in its VTK window, as an
8-bit RGB image on the device.  The kernels are csrc/raster.hip (include/dfl_hip.h
"Rasteriser"): a visibility buffer filled by the 64-bit integer atomic minimum, one shading pass per sample with a
headlight, a box resolve of ssaa x ssaa samples.  The kernels see triangles only: lines are drawn as ribbon().

Cameras are fp64 on the host: look_at() gives a view matrix (the eye looks down its -z axis), perspective() and
from_intrinsics() give projections to clip space with depth 0 (near) .. 1 (far).  render() takes the pair
(view, projection), multiplies each mesh's matrix in fp64 and rounds once to fp32.
There is no host path: CPU tensors are refused."""
import ctypes as C

import numpy as np
import torch

from . import _native as nat

AMBIENT, DIFFUSE = 0.15, 0.85
BACKGROUND = (0.0, 0.0, 0.0)
NEAR = 1e-3
MAX_SSAA, MAX_DIM, SMALL_BOX = nat.RASTER_MAX_SSAA, nat.RASTER_MAX_DIM, nat.RASTER_SMALL_BOX


def _vec(v, what):
    v = np.asarray(v, np.float64).reshape(-1)
    if v.shape != (3,) or not np.all(np.isfinite(v)):
        raise nat.DflError('raster.%s: three finite numbers are required' % what)
    return v


def _unit(v, what):
    n = np.linalg.norm(v)
    if not n > 0:
        raise nat.DflError('raster.%s has no length' % what)
    return v / n


def look_at(eye, target, up):
    """View matrix (fp64 4x4) of a camera at `eye` that looks at `target`: x right, y up, the view direction -z."""
    eye, target, up = _vec(eye, 'look_at: eye'), _vec(target, 'look_at: target'), _vec(up, 'look_at: up')
    f = _unit(target - eye, 'look_at: target - eye')
    s = _unit(np.cross(f, up), 'look_at: the view direction x up')
    u = np.cross(s, f)
    V = np.eye(4)
    V[0, :3], V[1, :3], V[2, :3] = s, u, -f
    V[:3, 3] = -V[:3, :3] @ eye
    return V


def _depth_terms(near, far, what):
    near, far = float(near), float(far)
    if not 0 < near < far < np.inf:
        raise nat.DflError('raster.%s: 0 < near < far is required' % what)
    return far / (far - near), -far * near / (far - near)          # depth = (a d + b) / d for the distance d


def perspective(fov_y_deg, aspect, near, far):
    """Projection (fp64 4x4) of eye space (looking down -z) with a vertical field of view and aspect = width / height."""
    a, b = _depth_terms(near, far, 'perspective')
    if not 0 < float(fov_y_deg) < 180 or not float(aspect) > 0:
        raise nat.DflError('raster.perspective: 0 < fov_y_deg < 180 and aspect > 0 are required')
    f = 1.0 / np.tan(np.radians(float(fov_y_deg)) / 2.0)
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1] = f / float(aspect), f
    P[2, 2], P[2, 3] = -a, b
    P[3, 2] = -1.0
    return P


def from_intrinsics(K, rows, cols, near, far, z_sign=1):
    """Projection (fp64 4x4) of a pinhole camera frame with the 3x3 intrinsic matrix K (last row 0 0 1): the point X lands
    on the pixel (K X / z)[:2] of a rows x cols image, pixel (c, r) being the centre of picture element (c, r).  The
    camera sees the half space z_sign * z > 0 (-1 for the projective frame of the full-resolution files)."""
    K = np.asarray(K, np.float64)
    if K.shape != (3, 3) or not np.all(np.isfinite(K)) or not np.array_equal(K[2], [0, 0, 1]):
        raise nat.DflError('raster.from_intrinsics: a finite 3x3 K with last row 0 0 1 is required')
    if int(rows) < 1 or int(cols) < 1 or z_sign not in (1, -1):
        raise nat.DflError('raster.from_intrinsics: rows, cols >= 1 and z_sign +1 or -1 are required')
    a, b = _depth_terms(near, far, 'from_intrinsics')
    s = float(z_sign)
    P = np.zeros((4, 4))
    half = np.array([0.0, 0.0, 0.5])
    P[0, :3] = s * ((2.0 / cols) * (K[0] + half) - np.array([0.0, 0.0, 1.0]))
    P[1, :3] = s * (np.array([0.0, 0.0, 1.0]) - (2.0 / rows) * (K[1] + half))
    P[2, 2], P[2, 3] = s * a, b
    P[3, 2] = s
    return P


def frame(points, direction, fov_y_deg, aspect, margin=1.05):
    """(eye, target) of a camera that looks along `direction` and holds every point of `points` [N, 3] in a view of the
    given vertical field and aspect: the target is the centre of the bounding box, the eye far enough for the
    bounding sphere (times margin) to fit the narrower of the two fields."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if not len(p) or not np.all(np.isfinite(p)):
        raise nat.DflError('raster.frame: finite points are required')
    d = _unit(_vec(direction, 'frame: direction'), 'frame: direction')
    c = (p.min(0) + p.max(0)) / 2.0
    r = max(float(np.linalg.norm(p - c, axis=1).max()), 1e-12) * float(margin)
    half_y = np.radians(float(fov_y_deg)) / 2.0
    half = min(half_y, np.arctan(np.tan(half_y) * float(aspect)))
    return c - d * (r / np.sin(half)), c


def ribbon(p0, p1, width, eye):
    """The line p0 -> p1 as two triangles that face `eye`: (positions fp32 [4, 3], triangles int32 [2, 3]); the ribbon is
    `width` wide, perpendicular to the line and to the direction from the eye to its middle."""
    p0, p1, eye = _vec(p0, 'ribbon: p0'), _vec(p1, 'ribbon: p1'), _vec(eye, 'ribbon: eye')
    side = _unit(np.cross(p1 - p0, (p0 + p1) / 2.0 - eye), 'ribbon: (p1 - p0) x (middle - eye)') * (float(width) / 2.0)
    pos = np.stack([p0 - side, p0 + side, p1 + side, p1 - side])
    return pos.astype(np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def _gpu(t, what, dtype, shape_ok):
    if not torch.is_tensor(t):
        raise nat.DflError('raster.%s: a torch tensor is required' % what)
    if t.dtype != dtype:
        raise nat.DflError('raster.%s: dtype %s, %s expected' % (what, t.dtype, dtype))
    if not t.is_cuda:
        raise nat.DflError('raster.%s needs its tensors on the GPU (no CPU path)' % what)
    if not shape_ok(t.shape):
        raise nat.DflError('raster.%s: bad shape %s' % (what, tuple(t.shape)))
    return t.contiguous()


class Mesh:
    """Triangles with one colour: pos [V, 3] fp32, tris [T, 3] int32, normals [V, 3] fp32 (required unless unlit),
    uv [V, 2] fp32 and texture [th, tw] uint8 (grey, sampled NEAREST, times rgb), all on the GPU; matrix = the fp64 4x4
    from the mesh's frame to the world.  Several Mesh objects may share tensors under different matrices."""

    def __init__(self, pos, tris, normals=None, uv=None, rgb=(1.0, 1.0, 1.0), unlit=False, texture=None, matrix=None):
        self.pos = _gpu(pos, 'Mesh: pos', torch.float32, lambda s: len(s) == 2 and s[1] == 3)
        self.tris = _gpu(tris, 'Mesh: tris', torch.int32, lambda s: len(s) == 2 and s[1] == 3)
        V = self.pos.shape[0]
        self.normals = None if normals is None else _gpu(normals, 'Mesh: normals', torch.float32, lambda s: tuple(s) == (V, 3))
        self.uv = None if uv is None else _gpu(uv, 'Mesh: uv', torch.float32, lambda s: tuple(s) == (V, 2))
        self.texture = None if texture is None else _gpu(texture, 'Mesh: texture', torch.uint8,
                                                         lambda s: len(s) == 2 and s[0] > 0 and s[1] > 0)
        self.unlit = bool(unlit)
        if self.normals is None and not self.unlit:
            raise nat.DflError('raster.Mesh: normals are required unless unlit')
        if (self.texture is None) != (self.uv is None):
            raise nat.DflError('raster.Mesh: uv and texture come together')
        self.rgb = _vec(rgb, 'Mesh: rgb')
        self.matrix = np.eye(4) if matrix is None else np.asarray(matrix, np.float64)
        if self.matrix.shape != (4, 4) or not np.all(np.isfinite(self.matrix)):
            raise nat.DflError('raster.Mesh: a finite 4x4 matrix is required')
        if any(t is not None and t.device != self.pos.device for t in (self.tris, self.normals, self.uv, self.texture)):
            raise nat.DflError('raster.Mesh: tensors on different devices')


def records(meshes, view, proj):
    """The dfl_raster_mesh array of a scene (a ctypes array) and the first primitive id of each mesh: ids count the
    triangles of the meshes one after the other."""
    view, proj = np.asarray(view, np.float64), np.asarray(proj, np.float64)
    if view.shape != (4, 4) or proj.shape != (4, 4) or not (np.all(np.isfinite(view)) and np.all(np.isfinite(proj))):
        raise nat.DflError('raster.render: view_proj is the pair (view, projection) of finite 4x4 matrices')
    arr = (nat.RasterMesh * max(len(meshes), 1))()
    first, nxt = [], 0
    for r, m in zip(arr, meshes):
        mv = view @ m.matrix
        mvp = (proj @ mv).astype(np.float32).reshape(-1)
        lin = mv[:3, :3]
        if not abs(np.linalg.det(lin)) > 0:
            raise nat.DflError('raster.render: a mesh matrix is singular')
        nmat = np.linalg.inv(lin).T.astype(np.float32).reshape(-1)
        r.pos, r.nrm, r.uv, r.tris, r.tex = m.pos.data_ptr(), nat.ptr(m.normals), nat.ptr(m.uv), m.tris.data_ptr(), nat.ptr(m.texture)
        r.n_verts, r.n_tris = m.pos.shape[0], m.tris.shape[0]
        r.th, r.tw = (m.texture.shape if m.texture is not None else (0, 0))
        r.first_prim = nxt
        r.flags = (nat.RASTER_UNLIT if m.unlit else 0) | (nat.RASTER_TEXTURED if m.texture is not None else 0)
        r.mvp[:], r.nmat[:], r.rgb[:] = mvp.tolist(), nmat.tolist(), m.rgb.astype(np.float32).tolist()
        first.append(nxt)
        nxt += m.tris.shape[0]
    if nxt >= 2 ** 31:
        raise nat.DflError('raster.render: %d triangles, at most 2^31 - 1' % nxt)
    return arr, first


def draw(meshes, view_proj, width, height, ssaa=1, background=BACKGROUND, ambient=AMBIENT, diffuse=DIFFUSE, near=NEAR,
         device=None, want=('rgb',)):
    """One dfl_raster_draw: a dict of the outputs named in `want` -- 'rgb' uint8 [H, W, 3], 'ids' int32 [Hs, Ws] (first id
    of mesh k = the number of triangles before it, -1 background), 'depth' fp32 [Hs, Ws] (inf background), 'counts' int32
    [4] (drawn, near-dropped, guard-dropped, degenerate) -- plus 'first_prim', the list of each mesh's first id."""
    meshes = list(meshes)
    try:
        view, proj = view_proj
    except (TypeError, ValueError):
        raise nat.DflError('raster.render: view_proj is the pair (view, projection)')
    W, H, ssaa = int(width), int(height), int(ssaa)
    if not all(isinstance(m, Mesh) for m in meshes):
        raise nat.DflError('raster.render: a list of raster.Mesh is required')
    dev = meshes[0].pos.device if meshes else (torch.device(device) if device is not None else torch.device('cuda'))
    if dev.type != 'cuda' or any(m.pos.device != dev for m in meshes):
        raise nat.DflError('raster.render needs every mesh on one GPU (no CPU path)')
    arr, first = records(meshes, view, proj)
    L = nat.lib()
    need = L.dfl_raster_scratch_bytes(W, H, ssaa, len(meshes))
    nat.check(need, 'dfl_raster_scratch_bytes')
    Ws, Hs = W * ssaa, H * ssaa
    scratch = torch.empty(need // 8, dtype=torch.int64, device=dev)
    host = np.frombuffer(arr, dtype=np.uint8, count=C.sizeof(nat.RasterMesh) * len(meshes)) if meshes else np.zeros(0, np.uint8)
    recs_dev = torch.from_numpy(host.copy()).to(dev) if meshes else None
    out = {'rgb': torch.empty((H, W, 3), dtype=torch.uint8, device=dev)}
    if 'ids' in want:
        out['ids'] = torch.empty((Hs, Ws), dtype=torch.int32, device=dev)
    if 'depth' in want:
        out['depth'] = torch.empty((Hs, Ws), dtype=torch.float32, device=dev)
    if 'counts' in want:
        out['counts'] = torch.empty(4, dtype=torch.int32, device=dev)
    a = nat.RasterArgs(meshes=C.addressof(arr) if meshes else None, meshes_dev=nat.ptr(recs_dev), scratch=scratch.data_ptr(),
                       rgb=out['rgb'].data_ptr(), ids=nat.ptr(out.get('ids')), depth=nat.ptr(out.get('depth')),
                       counts=nat.ptr(out.get('counts')), n_mesh=len(meshes), W=W, H=H, ssaa=ssaa, scratch_bytes=need,
                       znear=float(near), ambient=float(ambient), diffuse=float(diffuse))
    a.background[:] = _vec(background, 'render: background').tolist()
    with torch.cuda.device(dev):
        nat.call('dfl_raster_draw', a, torch.cuda.current_stream(dev).cuda_stream)
    out['first_prim'] = first         # (scratch and records go back to torch's allocator, which reuses them in stream order)
    return out


def render(meshes, view_proj, width, height, ssaa=1, background=BACKGROUND, ambient=AMBIENT, diffuse=DIFFUSE, near=NEAR,
           return_ids=False, device=None):
    """The scene as uint8 [H, W, 3] on the device; with return_ids also int32 [ssaa H, ssaa W], the primitive id of every
    sample (-1 background; the ids of mesh k start at the number of triangles of the meshes before it).
    view_proj = (view, projection), fp64 4x4 each (look_at, perspective / from_intrinsics); intensity of a lit sample =
    ambient + diffuse |n_z| / |n| in eye space (a headlight).  An empty list gives the background (on `device`)."""
    out = draw(meshes, view_proj, width, height, ssaa, background, ambient, diffuse, near, device,
               ('rgb', 'ids') if return_ids else ('rgb',))
    return (out['rgb'], out['ids']) if return_ids else out['rgb']
