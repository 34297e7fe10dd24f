#!/usr/bin/env python3
"""3D ground truth of one projection of the full-resolution file, as a glTF 2.0 binary scene: the reference's
examples_dataset/full_res_3d_viz.py, with the bone surfaces built on the GPU (dfl_amd.mesh) and a .glb file in place of
its interactive VTK window (any glTF viewer can rotate it).

    python examples/full_res_3d_viz.py ipcai_2020_full_res_data.h5 17-1882 0      # writes 17-1882_000.glb
    python examples/full_res_3d_viz.py full_res.h5 17-1882 0 --out scene.glb
    python examples/full_res_3d_viz.py full_res.h5 17-1882 0 --png scene.png --view oblique --png-size 1920x1080 --ssaa 2

--png PATH also renders the scene on the GPU (dfl_amd.raster) and writes it as a PNG: the same
actors, colours, radii and texture, BACKGROUND behind them, the rays as ribbons RAY_WIDTH mm wide.  --view oblique
(default) frames the whole scene from the side; --view source is what the X-ray sees, through the file's intrinsic
matrix: the bones in front of their own projection (the source sphere lies behind the near plane there, and the rays,
seen end-on, are left out).  --png-size WxH (default 1280x960; for the source view the detector's shape scaled to at
most 1280 columns), --ssaa N samples per pixel side (1..4, default 2).

--decimate R reduces every bone surface by the fraction R of its triangles after smoothing (dfl_amd.mesh.decimate,
DESIGN.md section 23; the reference's vtkQuadricDecimation runs at 0.25).  Without it the surfaces are not decimated.

Scene, in the camera projective frame, in mm: the left / right hemipelvis (labels 1 / 2, green / red) and the left /
right femur (5 / 6, cyan / orange) placed by the ground-truth poses, the 3D landmarks (purple spheres, radius 5), the
X-ray source (green, radius 10), the detector plane textured with the projection, and for each visible 2D landmark a
green sphere (radius 2.5) on the detector and a ray from the source to where its 3D landmark projects.  The surfaces
keep the reference's quirk of sitting 2 voxels off along the volume's y axis.
Files: the reference's HDF5 (dfl_amd.h5lite) or .npz with the same names as keys.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, drr, fullres, gltf, mesh, png, raster  # noqa: E402
from dfl_amd.fullres import Source  # noqa: E402

USAGE = 'Usage: {} <HDF5 full-res data file> <specimen ID> <projection index>'
# (node name, progress name, label, colour, pose)
SURFACES = (('left-hemipelvis', 'left hemipelvis', 1, (0.0, 1.0, 0.0), 'cam-to-pelvis-vol'),
            ('right-hemipelvis', 'right hemipelvis', 2, (1.0, 0.0, 0.0), 'cam-to-pelvis-vol'),
            ('left-femur', 'left femur', 5, (0.0, 1.0, 1.0), 'cam-to-left-femur-vol'),
            ('right-femur', 'right femur', 6, (1.0, 0.5, 0.0), 'cam-to-right-femur-vol'))
LAND3D_COLOR, LAND3D_RADIUS = (0.5, 0.0, 0.5), 5.0
SOURCE_COLOR, SOURCE_RADIUS = (0.0, 1.0, 0.0), 10.0
LAND2D_COLOR, LAND2D_RADIUS = (0.0, 1.0, 0.0), 2.5
RAY_COLOR = (0.0, 1.0, 0.0)
RAY_WIDTH = 1.0                     # mm, of the ribbons the PNG draws for the rays
PNG_SIZE, PNG_SSAA, PNG_FOV = (1280, 960), 2, 30.0
OBLIQUE = (0.55, -0.75, -0.35)      # view direction of --view oblique: along the beam, towards -columns and -rows of the detector
BACKGROUND = (0.7, 0.8, 1.0)
SPHERE_RES = 20                     # vtkSphereSource theta / phi resolution


def invert_rigid(H):
    out = np.eye(4)
    R_inv = H[0:3, 0:3].T
    out[0:3, 0:3] = R_inv
    out[0:3, 3] = R_inv @ -H[0:3, 3]
    return out


def flip_y(ny):
    """vtkImageFlip(FilteredAxis 1, FlipAboutOriginOff) on index coordinates: y -> ny - 1 - y."""
    F = np.eye(4)
    F[1, 1], F[1, 3] = -1.0, ny - 1
    return F


def vertex_xform(ny):
    """create_mesh's vertex_xform: y -> ny + 1 - y (together with flip_y: y -> y + 2)."""
    X = np.eye(4)
    X[1, 1], X[1, 3] = -1.0, ny + 1
    return X


def host_geometry(src, spec, idx, log=print):
    """Everything of the scene but the surfaces, in fp64 as the script computes it, plus the volume and the 4x4 that
    takes each label's marching-cubes index coordinates into the camera projective frame."""
    g = {}
    log('reading projection parameters...')
    intrinsic, extrinsic, rows, cols = fullres.proj_params(src)
    intrinsic_inv = np.linalg.inv(intrinsic)
    col_sp = float(fullres.scalar(src.get('proj-params/pixel-col-spacing')))
    row_sp = float(fullres.scalar(src.get('proj-params/pixel-row-spacing')))
    focal_len = abs((intrinsic[0, 0] * col_sp) + (intrinsic[1, 1] * row_sp)) / 2.0
    g['intrinsic'], g['rows'], g['cols'], g['focal_len'] = intrinsic, rows, cols, focal_len

    def det(x):
        return (intrinsic_inv * -focal_len) @ np.asarray(x, np.float64).reshape(3)

    g['detector'] = np.stack([det([0, 0, 1]), det([0, rows - 1, 1]), det([cols - 1, rows - 1, 1]), det([cols - 1, 0, 1])])
    pfx = fullres.projection_prefix(spec, idx)
    log('reading projection...')
    pix = np.asarray(src.get(pfx + 'image/pixels'))
    if pix.dtype.kind != 'f':
        raise nat.DflError('%simage/pixels has dtype %s: a float type expected' % (pfx, pix.dtype))
    lo, hi = pix.min(), pix.max()
    with np.errstate(invalid='ignore', divide='ignore'):
        scaled = 255 * ((pix - lo) / (hi - lo))
    g['texture'] = np.where(np.isnan(scaled), 0, scaled).astype(np.uint8)       # constant image: 0
    if g['texture'].shape != (rows, cols):
        raise nat.DflError('%simage/pixels has shape %s, proj-params say %s' % (pfx, pix.shape, (rows, cols)))
    log('reading GT poses...')
    poses = {k: extrinsic @ invert_rigid(P) for k, P in fullres.gt_poses(src, pfx).items()}
    log('reading GT 2D landmarks...')
    lands_2d = {}
    for name, l2 in fullres.gt_landmarks(src, pfx).items():
        if l2[0] >= 0 and l2[1] >= 0 and l2[0] < cols - 1 and l2[1] < rows - 1:
            lands_2d[name] = det(np.append(l2, 1))
    log('reading 3D landmarks...')
    lands_3d = {}
    for name, l3 in fullres.volume_landmarks(src, spec).items():
        lands_3d[name] = poses['cam-to-pelvis-vol'] @ np.append(l3, 1)
    g['lands_3d'] = {k: v[:3] for k, v in lands_3d.items()}
    g['lands_2d'] = lands_2d
    g['rays'] = {}
    for name in lands_2d:
        p = intrinsic @ lands_3d[name][0:3]
        g['rays'][name] = det(p / p[2])
    log('reading 3D segmentation...')
    img = spec + '/vol-seg/image/'
    vol = np.asarray(src.get(img + 'pixels'))
    if vol.dtype != np.uint8:
        raise nat.DflError('%spixels has dtype %s: uint8 expected (the reference reads it as unsigned char)' % (img, vol.dtype))
    if vol.ndim != 3:
        raise nat.DflError('%spixels has shape %s: [z, y, x] expected' % (img, vol.shape))
    inds_to_phys = drr.inds_to_phys(*fullres.volume_frame(src, spec, 'vol-seg/image'))     # the annotation's own frame
    ny = vol.shape[1]
    g['volume'] = vol
    g['surface_xforms'] = [poses[pose] @ inds_to_phys @ vertex_xform(ny) @ flip_y(ny) for _, _, _, _, pose in SURFACES]
    return g


def unit_sphere(res=SPHERE_RES):
    """(positions [V, 3], triangles [T, 3]) of a unit UV sphere: two poles and res - 1 rings of res points."""
    phi = np.pi * np.arange(1, res) / res
    th = 2 * np.pi * np.arange(res) / res
    ring = np.stack([np.outer(np.sin(phi), np.cos(th)), np.outer(np.sin(phi), np.sin(th)),
                     np.repeat(np.cos(phi)[:, None], res, 1)], -1).reshape(-1, 3)
    pos = np.concatenate([[[0, 0, 1]], ring, [[0, 0, -1]]])
    tris = []
    ring_at = lambda k, j: 1 + k * res + j % res        # noqa: E731
    for j in range(res):
        tris.append((0, ring_at(0, j), ring_at(0, j + 1)))
        for k in range(res - 2):
            a, b, c, d = ring_at(k, j), ring_at(k + 1, j), ring_at(k + 1, j + 1), ring_at(k, j + 1)
            tris += [(a, b, c), (a, c, d)]
        tris.append((len(pos) - 1, ring_at(res - 2, j + 1), ring_at(res - 2, j)))
    return pos.astype(np.float32), np.array(tris, np.uint32)


def surfaces_on_gpu(g, dev, log=print, on_device=None, decimate=None):
    """[(positions, normals, triangles) or None] per entry of SURFACES: one marching-cubes pass for all labels, then
    per label the smoother, with decimate=R the quadric decimation by R in the smoother's normalised frame (where the
    reference decimates), the transform into the camera projective frame and the normals.  A list passed as on_device
    receives the same entries as GPU tensors."""
    vol = torch.from_numpy(np.ascontiguousarray(g['volume'])).to(dev)
    meshes = mesh.label_surfaces(vol, [s[2] for s in SURFACES])
    out = []
    for (_, what, _, _, _), (verts, tris), M in zip(SURFACES, meshes, g['surface_xforms']):
        log('creating {} mesh...'.format(what))
        if tris.shape[0] == 0:
            out.append(None)
            if on_device is not None:
                on_device.append(None)
            continue
        xs, undo = mesh.smooth(verts, tris)
        if decimate is not None:
            xs, tris, _ = mesh.decimate(xs, tris, decimate)
        pos = mesh.transform(xs, M @ undo)
        nrm = mesh.vertex_normals(pos, tris)
        out.append((pos.cpu().numpy(), nrm.cpu().numpy(), tris.cpu().numpy()))
        if on_device is not None:
            on_device.append((pos, nrm, tris))
    return out


def build_scene(g, surfaces):
    sc = gltf.Scene()
    sc.doc['scenes'][0]['extras'] = {'background': list(BACKGROUND)}
    for (name, _, label, rgb, _), s in zip(SURFACES, surfaces):
        if s is None:
            sc.node(name)
            continue
        pos, nrm, tris = s
        sc.node(name, sc.mesh(name, pos, tris.astype(np.uint32), sc.material(name, rgb), normals=nrm))
    sp, st = unit_sphere()
    land3d = sc.mesh('sphere-landmark', sp, st, sc.material('landmark', LAND3D_COLOR), normals=sp)
    green = sc.mesh('sphere-green', sp, st, sc.material('green', SOURCE_COLOR), normals=sp)
    for name, p in g['lands_3d'].items():
        sc.node('vol-landmark/' + name, land3d, translation=p, scale=[LAND3D_RADIUS] * 3)
    sc.node('source', green, translation=[0, 0, 0], scale=[SOURCE_RADIUS] * 3)
    ray_mat = sc.material('ray', RAY_COLOR)
    for name, p in g['lands_2d'].items():
        sc.node('proj-landmark/' + name, green, translation=p, scale=[LAND2D_RADIUS] * 3)
        line = np.stack([np.zeros(3), g['rays'][name]])
        sc.node('ray/' + name, sc.mesh('ray/' + name, line, None, ray_mat, mode=gltf.LINES))
    H, W = g['texture'].shape
    corners = g['detector']                                   # r0c0, rMc0, rMcN, r0cN as the reference inserts them
    # texel (r, c) lands on the detector point of index (c, r): corners at texel centres, sampled NEAREST
    uv = np.array([[0.5 / W, 0.5 / H], [0.5 / W, (H - 0.5) / H], [(W - 0.5) / W, (H - 0.5) / H], [(W - 0.5) / W, 0.5 / H]])
    n = np.cross(corners[1] - corners[0], corners[2] - corners[0])
    n = np.tile(n / max(np.linalg.norm(n), 1e-300), (4, 1))
    tex = np.repeat(g['texture'][:, :, None], 3, 2)
    det_mat = sc.material('detector', (1.0, 1.0, 1.0), texture_rgb=tex)
    sc.node('detector', sc.mesh('detector', corners, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), det_mat, normals=n,
                                texcoords=uv))
    return sc


def raster_scene(g, surfaces, dev, view):
    """[(actor name, raster.Mesh)] of the scene build_scene() writes, from the surfaces' GPU tensors."""
    actors = []
    for (name, _, _, rgb, _), s in zip(SURFACES, surfaces):
        if s is not None:
            actors.append((name, raster.Mesh(s[0], s[2], normals=s[1], rgb=rgb)))
    sp, st = unit_sphere()
    sp, st = torch.from_numpy(sp).to(dev), torch.from_numpy(st.astype(np.int32)).to(dev)

    def sphere(name, centre, radius, rgb):            # instances of the one unit sphere
        M = np.diag([radius, radius, radius, 1.0])
        M[:3, 3] = centre
        actors.append((name, raster.Mesh(sp, st, normals=sp, rgb=rgb, matrix=M)))

    for name, p in g['lands_3d'].items():
        sphere('vol-landmark/' + name, p, LAND3D_RADIUS, LAND3D_COLOR)
    sphere('source', np.zeros(3), SOURCE_RADIUS, SOURCE_COLOR)
    eye = np.linalg.inv(view)[:3, 3]
    for name, p in g['lands_2d'].items():
        sphere('proj-landmark/' + name, p, LAND2D_RADIUS, LAND2D_COLOR)
        if np.linalg.norm(eye) > SOURCE_RADIUS:       # from the source itself a ray is a point
            pos, tris = raster.ribbon(np.zeros(3), g['rays'][name], RAY_WIDTH, eye)
            actors.append(('ray/' + name, raster.Mesh(torch.from_numpy(pos).to(dev), torch.from_numpy(tris).to(dev),
                                                      rgb=RAY_COLOR, unlit=True)))
    H, W = g['texture'].shape
    corners = g['detector']
    uv = np.array([[0.5 / W, 0.5 / H], [0.5 / W, (H - 0.5) / H], [(W - 0.5) / W, (H - 0.5) / H], [(W - 0.5) / W, 0.5 / H]])
    n = np.cross(corners[1] - corners[0], corners[2] - corners[0])
    n = np.tile(n / max(np.linalg.norm(n), 1e-300), (4, 1))
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)        # noqa: E731
    actors.append(('detector', raster.Mesh(f32(corners), torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32, device=dev),
                                           normals=f32(n), uv=f32(uv), texture=torch.from_numpy(g['texture']).to(dev))))
    return actors


def scene_points(g, surfaces):
    """Points whose bounding sphere holds the scene: detector corners, sphere extremes, the surfaces' boxes."""
    pts = [g['detector']]
    for c, r in [(np.zeros(3), SOURCE_RADIUS)] + [(p, LAND3D_RADIUS) for p in g['lands_3d'].values()]:
        pts.append(np.asarray(c)[None] + r * np.concatenate([np.eye(3), -np.eye(3)]))
    for s in surfaces:
        if s is not None:
            lo, hi = torch.aminmax(s[0], dim=0)
            pts.append(torch.stack([lo, hi]).double().cpu().numpy())
    return np.concatenate(pts)


def camera(g, surfaces, which, width, height):
    """(view, projection, near) of --view `which` for a width x height picture."""
    if which == 'source':
        near = 2.0 * SOURCE_RADIUS
        return np.eye(4), raster.from_intrinsics(g['intrinsic'], g['rows'], g['cols'], near, 2.0 * g['focal_len'], z_sign=-1), near
    c = g['detector']
    beam = g['detector'].mean(0) / np.linalg.norm(g['detector'].mean(0))
    right, down = (c[3] - c[0]) / np.linalg.norm(c[3] - c[0]), (c[1] - c[0]) / np.linalg.norm(c[1] - c[0])
    direction = OBLIQUE[0] * beam + OBLIQUE[1] * right + OBLIQUE[2] * down
    pts = scene_points(g, surfaces)
    eye, target = raster.frame(pts, direction, PNG_FOV, width / height)
    view = raster.look_at(eye, target, -down)
    depth = -(pts @ view[2, :3] + view[2, 3])
    near = max(float(depth.min()) - 2.0 * SOURCE_RADIUS, 1e-3 * float(depth.max()))
    return view, raster.perspective(PNG_FOV, width / height, near, float(depth.max()) + 2.0 * SOURCE_RADIUS), near


def render_png(g, surfaces, dev, which, width, height, ssaa, return_ids=False):
    """The picture of --png as uint8 [H, W, 3] on the device (with return_ids: also the ids and the actors' names in
    record order)."""
    view, proj, near = camera(g, surfaces, which, width, height)
    actors = raster_scene(g, surfaces, dev, view)
    out = raster.render([m for _, m in actors], (view, proj), width, height, ssaa=ssaa, background=BACKGROUND, near=near,
                        return_ids=return_ids, device=dev)
    return (out[0], out[1], actors, (view, proj, near)) if return_ids else out


def options(argv):
    """(positional arguments, {flag: value}) or a message: --out, --png, --png-size, --view, --ssaa and --decimate take
    one value."""
    argv, opt = list(argv), {}
    for flag in ('--out', '--png', '--png-size', '--view', '--ssaa', '--decimate'):
        if flag in argv:
            k = argv.index(flag)
            if k + 1 >= len(argv):
                return '{} needs a {}'.format(flag, 'path' if flag in ('--out', '--png') else 'value')
            opt[flag] = argv[k + 1]
            del argv[k:k + 2]
    if '--decimate' in opt:
        try:
            opt['--decimate'] = float(opt['--decimate'])
        except ValueError:
            opt['--decimate'] = float('nan')
        if not 0.0 < opt['--decimate'] < 1.0:
            return '--decimate is a reduction between 0 and 1 (the reference: {})'.format(mesh.REDUCTION)
    if any(f in opt for f in ('--png-size', '--view', '--ssaa')) and '--png' not in opt:
        return '--png-size, --view and --ssaa go with --png'
    if '--png' in opt:
        try:
            w, h = (int(t) for t in opt.get('--png-size', '0x0').lower().split('x'))
            opt['--png-size'] = (w, h) if '--png-size' in opt else None
            opt['--ssaa'] = int(opt.get('--ssaa', PNG_SSAA))
        except ValueError:
            return '--png-size is WxH and --ssaa an integer'
        opt.setdefault('--view', 'oblique')
        if opt['--view'] not in ('oblique', 'source') or not 1 <= opt['--ssaa'] <= raster.MAX_SSAA or \
                (opt['--png-size'] is not None and not (1 <= min(opt['--png-size'])
                                                         and max(opt['--png-size']) * opt['--ssaa'] <= raster.MAX_DIM)):
            return '--view is oblique or source, --ssaa 1..{}, --png-size times --ssaa at most {}'.format(raster.MAX_SSAA,
                                                                                                         raster.MAX_DIM)
    return argv, opt


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    parsed = options(argv)
    if isinstance(parsed, str):
        print(parsed)
        return 1
    argv, opt = parsed
    out = opt.get('--out')
    if len(argv) < 3:
        print(USAGE.format(os.path.basename(sys.argv[0])))
        return 1
    spec, idx = argv[1], int(argv[2])
    if not torch.cuda.is_available():
        raise nat.DflError('no GPU visible: the bone surfaces are built by HIP kernels (no CPU path)')
    src = Source(argv[0])
    try:
        g = host_geometry(src, spec, idx)
    finally:
        src.close()
    dev = dfl_amd.get_device()
    on_device = [] if '--png' in opt else None
    surfaces = surfaces_on_gpu(g, dev, on_device=on_device, decimate=opt.get('--decimate'))
    out = out or '{}_{:03d}.glb'.format(spec, idx)
    build_scene(g, surfaces).write(out)
    print('wrote {}'.format(out))
    if '--png' in opt:
        size = opt['--png-size']
        if size is None:
            size = PNG_SIZE
            if opt['--view'] == 'source':
                w = min(g['cols'], PNG_SIZE[0])
                size = (w, max(1, int(round(w * g['rows'] / g['cols']))))
        png.write(opt['--png'], render_png(g, on_device, dev, opt['--view'], size[0], size[1], opt['--ssaa']).cpu().numpy())
        print('wrote {}'.format(opt['--png']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
