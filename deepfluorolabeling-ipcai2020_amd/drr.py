"""Digitally reconstructed radiographs, per-label path lengths, a 2D label map and projected landmarks from the CT,
the 3D annotation and the ground-truth poses of the full-resolution file, on the pixel grid of the training file.

The geometry is float64 on the host, chained as the reference's full_res_3d_viz.py chains its matrices
(examples/full_res_3d_viz.py restates that chain); the rays are cast by csrc/drr.hip (dfl_drr_render).  DESIGN.md
section 15 states the semantics, tests/drr_ref.py restates them in numpy.  The file is read through dfl_amd.fullres.

    K, E = the intrinsic and extrinsic matrix of proj-params, P_o = the projection's cam-to-{pelvis,left-femur,right-femur}-vol
    I2P = [dir-mat * spacing | origin] of the volume; index coordinates are (x, y, z) = (column, row, slice)
    C2I_o = inv(I2P) P_o inv(E)                      camera projective frame -> volume index coordinates
    ray of output pixel (c, r): q = -inv(K) G [c, r, 1]; o = C2I_o[:3, 3]; d = C2I_o[:3, :3] q; points o + t d, t >= 0;
    one unit of t is |q| mm (the poses are rigid)

G maps an output pixel to a detector pixel.  On the training grid (preprocess: crop, factor f, 180-degree turn), with
Rc x Cc = (rows - 2 crop) x (cols - 2 crop) the crop window:

    not turned   c_det = crop + f c + (f - 1) / 2                 G = [[ f, 0, crop + (f - 1) / 2],
                 r_det = crop + f r + (f - 1) / 2                      [ 0, f, crop + (f - 1) / 2], [0, 0, 1]]
    turned       c_det = crop + Cc - 1 - f c - (f - 1) / 2        G = [[-f, 0, crop + Cc - 1 - (f - 1) / 2],
                 r_det = crop + Rc - 1 - f r - (f - 1) / 2             [ 0, -f, crop + Rc - 1 - (f - 1) / 2], [0, 0, 1]]

which is the inverse of preprocess.map_lands: output pixel (c, r) looks along the ray through the centre of the box of
detector pixels it covers.  A 3D landmark X (volume physical frame) projects to K (E inv(P_pelvis) X), divided by its
third component and pulled through inv(G): the reference's own `intrinsic * land_3d`.

The volume is assumed to lie between source and detector: rays are not clipped at the detector plane.
Tensors on the CPU are refused: there is no CPU path.
"""

import ctypes as C

import numpy as np
import torch

from . import _native as nat
from . import fullres, preprocess
from .fullres import POSES

__all__ = ['Obj', 'Grid', 'Geometry', 'Volume', 'geometry', 'read_volume', 'training_grid', 'default_objects', 'pack', 'pack_objects',
           'render', 'render_args', 'args_for_records', 'pose_gradient', 'box_pivots', 'project', 'project_points', 'hu_to_mu', 'label_mask', 'POSES', 'DEFAULT_MASKS']

# labels of the 3D annotation: 1, 2 hemipelves, 3 vertebrae, 4 sacrum, 5, 6 femurs
DEFAULT_MASKS = ((1, 2, 3, 4), (5,), (6,))
OBJECT_DTYPE = np.dtype([('o', np.float32, 3), ('M', np.float32, 9), ('box_lo', np.int32, 3), ('box_hi', np.int32, 3),
                         ('mask', np.uint32)])
assert OBJECT_DTYPE.itemsize == C.sizeof(nat.DrrObject)
_INTERP = {'exact': nat.DRR_EXACT, 'trilinear': nat.DRR_TRILINEAR}


def label_mask(labels):
    """Labels (0..15) -> the 16-bit mask with those bits set."""
    m = 0
    for l in labels:
        if not 0 <= int(l) < nat.DRR_MAX_LABELS:
            raise nat.DflError('drr: label %d in a mask (labels 0..15 are supported)' % int(l))
        m |= 1 << int(l)
    return m


class Obj:
    """A rigid pose (C2I: camera projective frame -> volume index coordinates, 4 x 4 float64) and a label mask."""

    def __init__(self, c2i, mask):
        self.c2i = np.array(c2i, np.float64).reshape(4, 4)
        self.mask = int(mask) if not isinstance(mask, (tuple, list, set, frozenset)) else label_mask(mask)
        if not 0 <= self.mask <= 0xffff:
            raise nat.DflError('drr: an object mask of %#x (16 bits: labels 0..15)' % self.mask)


class Grid:
    """The output pixel grid: Q = -inv(K) G (3 x 3 float64) and the output size."""

    def __init__(self, Q, H, W):
        self.Q = np.array(Q, np.float64).reshape(3, 3)
        self.H, self.W = int(H), int(W)
        if self.H < 1 or self.W < 1:
            raise nat.DflError('drr: an output grid of %d x %d' % (self.H, self.W))


class Geometry:
    """What geometry() returns: K, E, poses {name: P}, I2P, G (float64), objects [Obj], grid, size = (H, W)."""

    def __init__(self, K, E, poses, I2P, G, objects, grid):
        self.K, self.E, self.poses, self.I2P, self.G, self.objects, self.grid = K, E, poses, I2P, G, objects, grid
        self.size = (grid.H, grid.W)


def training_grid(rows, cols, crop=0, factor=1, rot180=False):
    """(G, (H, W)): the 3 x 3 map from a pixel of the preprocessed image to a detector pixel (module docstring)."""
    H, W = preprocess.out_size(rows, cols, crop, factor)
    f, crop = int(factor), int(crop)
    Rc, Cc = int(rows) - 2 * crop, int(cols) - 2 * crop
    h = (f - 1) / 2.0
    if rot180:
        G = np.array([[-f, 0, crop + Cc - 1 - h], [0, -f, crop + Rc - 1 - h], [0, 0, 1]], np.float64)
    else:
        G = np.array([[f, 0, crop + h], [0, f, crop + h], [0, 0, 1]], np.float64)
    return G, (H, W)


def inds_to_phys(dir_mat, spacing, origin):
    M = np.eye(4)
    M[:3, :3] = np.asarray(dir_mat, np.float64).reshape(3, 3) * np.asarray(spacing, np.float64).reshape(-1)[None, :]
    M[:3, 3] = np.asarray(origin, np.float64).reshape(-1)
    return M


def default_objects(E, poses, I2P, bones_only=True):
    """Pelvis {1, 2, 3, 4}, left femur {5}, right femur {6}; bones_only=False adds the pelvis pose with bit 0 alone (the
    soft tissue)."""
    back = np.linalg.inv(I2P)
    Ei = np.linalg.inv(E)
    obs = [Obj(back @ np.asarray(poses[name], np.float64) @ Ei, labels) for name, labels in zip(POSES, DEFAULT_MASKS)]
    if not bones_only:
        obs.append(Obj(back @ np.asarray(poses[POSES[0]], np.float64) @ Ei, (0,)))
    return obs


def geometry(src, spec, proj, crop=0, factor=1, rot180=None, bones_only=True):
    """The float64 matrices of projection `proj` of specimen `spec`, read from src (a fullres.Source, or anything with
    its get(path)), its objects and its output grid.  rot180=None reads the projection's own flag."""
    K, E, rows, cols = fullres.proj_params(src)
    pfx = fullres.projection_prefix(spec, proj)
    poses = fullres.gt_poses(src, pfx)
    I2P = inds_to_phys(*fullres.volume_frame(src, spec))
    if rot180 is None:
        rot180 = fullres.rot180(src, pfx)
    G, (H, W) = training_grid(rows, cols, crop, factor, rot180)
    return Geometry(K, E, poses, I2P, G, default_objects(E, poses, I2P, bones_only), Grid(-np.linalg.inv(K) @ G, H, W))


def _project(K, E, P, xyz):
    X = np.asarray(xyz, np.float64).reshape(-1, 3)
    cam = (E @ np.linalg.inv(P)) @ np.concatenate([X, np.ones((X.shape[0], 1))], 1).T
    p = K @ cam[:3]
    return p / p[2:3]


def project(K, E, P, xyz):
    """3D points of the volume's physical frame, [L, 3] (or [3]), -> detector (column, row) [2, L], float64: K (E inv(P) X)
    divided by its third component."""
    return _project(K, E, P, xyz)[:2]


def project_points(geom, xyz):
    """project() under geom's pelvis pose, pulled through inv(G): [2, L] (column, row) on the output grid."""
    return (np.linalg.inv(geom.G) @ _project(geom.K, geom.E, geom.poses[POSES[0]], xyz))[:2]


def hu_to_mu(vol, mu_water=0.02):
    """Hounsfield units -> linear attenuation per mm (float32): mu_water * max(HU + 1000, 0) / 1000."""
    if not torch.is_tensor(vol) or not vol.is_cuda:
        raise nat.DflError('drr.hu_to_mu needs its tensor on the GPU (no CPU path)')
    return ((vol.to(torch.float32) + 1000.0).clamp_(min=0.0) * (float(mu_water) / 1000.0)).contiguous()


def _device_volume(t, what, dtype):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise nat.DflError('drr.Volume needs its tensor on the GPU (no CPU path)')
    if t.dim() != 3:
        raise nat.DflError('drr.Volume: %s must be [z, y, x], got shape %s' % (what, tuple(t.shape)))
    if t.dtype != dtype:
        raise nat.DflError('drr.Volume: %s has dtype %s, expected %s' % (what, t.dtype, dtype))
    return t.detach().contiguous()


class Volume:
    """mu (float32 [nz, ny, nx], per mm) and labels (uint8, same shape, 0..15) on one GPU, and per mask the index box
    of the voxels it admits (computed once)."""

    def __init__(self, mu, labels):
        self.mu = _device_volume(mu, 'mu', torch.float32)
        self.labels = _device_volume(labels, 'labels', torch.uint8)
        if self.mu.shape != self.labels.shape or self.mu.device != self.labels.device:
            raise nat.DflError('drr.Volume: mu is %s on %s, labels are %s on %s' % (tuple(self.mu.shape), self.mu.device,
                                                                                 tuple(self.labels.shape), self.labels.device))
        if self.mu.numel() < 1 or self.mu.numel() >= 2 ** 31:
            raise nat.DflError('drr.Volume: %d voxels (1 .. 2^31 - 1 are supported)' % self.mu.numel())
        present = torch.bincount(self.labels.reshape(-1).to(torch.int64), minlength=256).cpu().numpy()
        if present[nat.DRR_MAX_LABELS:].any():
            raise nat.DflError('drr.Volume: a label above 15 in the volume (labels 0..15 are supported)')
        self.n_labels = int(np.nonzero(present)[0].max()) + 1
        self.shape = tuple(int(n) for n in self.mu.shape)                      # (nz, ny, nx)
        self._boxes = {}

    @property
    def full_box(self):
        nz, ny, nx = self.shape
        return (0, 0, 0), (nx - 1, ny - 1, nz - 1)

    def box(self, mask):
        """((x0, y0, z0), (x1, y1, z1)), inclusive, of the voxels whose label is in the mask; empty: hi = lo - 1."""
        mask = int(mask)
        if mask not in self._boxes:
            lut = torch.tensor([(mask >> l) & 1 for l in range(256)], dtype=torch.bool, device=self.labels.device)
            adm = lut[self.labels.to(torch.int64)]
            lo, hi = [], []
            for axis, keep in ((2, (0, 1)), (1, (0, 2)), (0, (1, 2))):          # x, y, z
                on = torch.nonzero(adm.any(dim=keep[1]).any(dim=keep[0])).reshape(-1)
                if on.numel() == 0:
                    lo, hi = [0, 0, 0], [-1, -1, -1]
                    break
                lo.append(int(on[0]))
                hi.append(int(on[-1]))
            self._boxes[mask] = (tuple(lo), tuple(hi))
        return self._boxes[mask]


def _views(objects):
    """objects: [Obj] or [[Obj]] (a leading view axis) -> ([[Obj]], had a view axis)."""
    objects = list(objects)
    if not objects:
        raise nat.DflError('drr: no objects')
    if isinstance(objects[0], Obj):
        return [objects], False
    views = [list(v) for v in objects]
    if any(len(v) != len(views[0]) or not v for v in views):
        raise nat.DflError('drr: every view needs the same, non-zero number of objects')
    return views, True


def read_volume(src, spec, dev, cast_labels=False):
    """The drr.Volume of a specimen of the full-resolution file on `dev`: mu from 'vol/pixels' (Hounsfield units), the
    labels from 'vol-seg/image/pixels'.  Labels that are not uint8 are refused, or cast with cast_labels=True."""
    hu = np.asarray(src.get(spec + '/vol/pixels'))
    lab = np.asarray(src.get(spec + '/vol-seg/image/pixels'))
    if hu.ndim != 3 or lab.shape != hu.shape:
        raise nat.DflError('%s: vol/pixels has shape %s, vol-seg/image/pixels %s: two equal [z, y, x] volumes expected'
                           % (spec, hu.shape, lab.shape))
    if cast_labels:
        lab = lab.astype(np.uint8, copy=False)
    elif lab.dtype != np.uint8:
        raise nat.DflError('%s/vol-seg/image/pixels has dtype %s: uint8 expected' % (spec, lab.dtype))
    mu = hu_to_mu(torch.from_numpy(np.ascontiguousarray(hu.astype(np.float32, copy=False))).to(dev))
    return Volume(mu, torch.from_numpy(np.ascontiguousarray(lab)).to(dev))


def pack(volume, c2is, masks, grid, interp='exact', tight_boxes=True):
    """The fp32 argument records of the kernel, a numpy array [views, n_obj] of OBJECT_DTYPE, rounded from float64:
    o = C2I[:3, 3], M = C2I[:3, :3] Q, the object's box and mask.  c2is is [views, n_obj, 4, 4] float64; masks (integers,
    as Obj.mask) is [n_obj], or [views, n_obj] where the views differ.  Trilinear samples reach half a voxel past the
    voxels they read, so their tight boxes are one voxel wider (clipped to the volume)."""
    A, m = np.asarray(c2is, np.float64), np.asarray(masks)
    if A.ndim != 4 or A.shape[2:] != (4, 4) or A.shape[0] < 1 or A.shape[1] < 1 or m.shape not in (A.shape[1:2], A.shape[:2]):
        raise nat.DflError('drr.pack: c2is of shape %s for masks of shape %s: [views, n_obj, 4, 4] and [n_obj] or [views, n_obj] '
                           'expected' % (A.shape, m.shape))
    flat = m.ravel().tolist()
    if m.dtype.kind not in 'iu' or not all(0 <= x <= 0xffff for x in flat):
        raise nat.DflError('drr.pack: masks must be integers of 16 bits (labels 0..15; label_mask makes one of a set of labels)')
    flo, fhi = volume.full_box
    boxes = {}
    for mask in set(flat):
        lo, hi = volume.box(mask) if tight_boxes else (flo, fhi)
        if tight_boxes and interp == 'trilinear' and hi[0] >= lo[0]:
            lo = tuple(max(a - 1, 0) for a in lo)
            hi = tuple(min(a + 1, b) for a, b in zip(hi, fhi))
        boxes[mask] = lo, hi
    out = np.zeros(A.shape[:2], OBJECT_DTYPE)
    out['o'] = A[:, :, :3, 3]
    out['M'] = (A[:, :, :3, :3] @ grid.Q).reshape(A.shape[0], A.shape[1], 9)
    out['mask'] = m                                                            # masks [n_obj] serve every view, and so do their boxes
    out['box_lo'] = np.array([boxes[x][0] for x in flat], np.int32).reshape(m.shape + (3,))
    out['box_hi'] = np.array([boxes[x][1] for x in flat], np.int32).reshape(m.shape + (3,))
    return out


def pack_objects(volume, objects, grid, interp='exact', tight_boxes=True):
    """pack() of [Obj], or of [[Obj]] with a leading view axis."""
    views, _ = _views(objects)
    return pack(volume, [[ob.c2i for ob in obs] for obs in views], [[ob.mask for ob in obs] for obs in views], grid, interp,
                tight_boxes)


def launch(dev, entry, a):
    """One call of a C entry point on dev's current stream."""
    with torch.cuda.device(dev):
        nat.call(entry, a, torch.cuda.current_stream(dev).cuda_stream)


def _scene_fields(volume, recs, grid, step_mm):
    """(the uploaded records, the fields DrrArgs and DrrPoseGradArgs share) for packed records [views, n_obj]."""
    nz, ny, nx = volume.shape
    d_objs = torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(-1)).to(volume.mu.device)
    return d_objs, dict(mu=volume.mu.data_ptr(), labels=volume.labels.data_ptr(), objects=d_objs.data_ptr(),
                        qscale=(nat.f32 * 9)(*grid.Q.astype(np.float32).reshape(-1)), nx=nx, ny=ny, nz=nz, H=grid.H, W=grid.W,
                        views=recs.shape[0], n_obj=recs.shape[1], step_mm=float(step_mm))


def args_for_records(volume, recs, grid, interp='exact', step_mm=0.5, want_plen=False, want_labels=True, min_len_mm=1.0, mapping=0):
    """(DrrArgs, (att, plen, labels) with the view axis, tensors to keep alive) for packed records [views, n_obj]: the
    upload, the freshly allocated outputs and the argument block of dfl_drr_render, nothing launched."""
    exact = interp == 'exact'
    dev = volume.mu.device
    V, H, W, NL = recs.shape[0], grid.H, grid.W, volume.n_labels
    d_objs, shared = _scene_fields(volume, recs, grid, step_mm)
    att = torch.empty((V, H, W), dtype=torch.float32, device=dev)
    plen = torch.empty((V, NL, H, W), dtype=torch.float32, device=dev) if exact and want_plen else None
    lab = torch.empty((V, H, W), dtype=torch.uint8, device=dev) if exact and want_labels else None
    a = nat.DrrArgs(att=att.data_ptr(), plen=nat.ptr(plen), label_map=nat.ptr(lab), n_labels=NL, interp=_INTERP[interp],
                    mapping=int(mapping), min_len_mm=float(min_len_mm), **shared)
    return a, (att, plen, lab), [d_objs, volume]


def box_pivots(recs):
    """float32 [..., 3]: the middle of every record's box in index coordinates (0 for an empty box): the default pivots
    of pose_gradient."""
    lo, hi = recs['box_lo'].astype(np.float64), recs['box_hi'].astype(np.float64)
    return np.where((hi < lo).any(-1, keepdims=True), 0.0, (lo + hi) / 2).astype(np.float32)


def pose_gradient(volume, recs, grid, d_att, pivots=None, step_mm=0.5):
    """The force F and moment Mom that the detector-space adjoint d_att [V, H, W] (float32, on the GPU) exerts on every
    object of the trilinear DRR of the packed records recs [V, n_obj] (pack(..., interp='trilinear')), with the
    renderer's sampling frozen (dfl_drr_pose_grad): float64 [V, n_obj, 12] on the device, F[3] then
    Mom[3][3] row-major about pivots [V, n_obj, 3] (index coordinates; default: box_pivots(recs)).  For a motion
    x -> x + eps (L (x - pivot) + tau) of an object, d (sum d_att att) / d eps = <Mom, L> + F . tau."""
    if not isinstance(volume, Volume):
        raise nat.DflError('drr.pose_gradient needs a drr.Volume (device tensors; no CPU path)')
    recs = np.asarray(recs)
    if recs.dtype != OBJECT_DTYPE or recs.ndim != 2 or recs.shape[0] < 1 or recs.shape[1] < 1:
        raise nat.DflError('drr.pose_gradient: records [views, n_obj] of drr.OBJECT_DTYPE expected (drr.pack)')
    if not float(step_mm) > 0:
        raise nat.DflError('drr.pose_gradient: step_mm must be positive, got %r' % (step_mm,))
    V, n_obj = recs.shape
    dev, H, W = volume.mu.device, grid.H, grid.W
    if not torch.is_tensor(d_att) or not d_att.is_cuda:
        raise nat.DflError('drr.pose_gradient needs d_att on the GPU (no CPU path)')
    if d_att.dtype != torch.float32 or tuple(d_att.shape) != (V, H, W) or d_att.device != dev:
        raise nat.DflError('drr.pose_gradient: d_att has shape %s and dtype %s on %s: float32 %s on %s expected'
                           % (tuple(d_att.shape), d_att.dtype, d_att.device, (V, H, W), dev))
    piv = box_pivots(recs) if pivots is None else np.asarray(pivots, np.float32)
    if piv.shape != (V, n_obj, 3) or not np.isfinite(piv).all():
        raise nat.DflError('drr.pose_gradient: pivots of shape %s: finite [%d, %d, 3] expected' % (piv.shape, V, n_obj))
    lib = nat.lib()
    need = int(lib.dfl_drr_pose_grad_scratch_doubles(V, n_obj, H, W))
    if need < 0:
        raise nat.DflError('drr.pose_gradient: %s' % lib.dfl_last_error().decode())
    d_att = d_att.detach().contiguous()
    d_objs, shared = _scene_fields(volume, recs, grid, step_mm)
    d_piv = torch.from_numpy(np.ascontiguousarray(piv)).to(dev)
    grad = torch.empty((V, n_obj, 12), dtype=torch.float64, device=dev)
    scratch = torch.empty(need, dtype=torch.float64, device=dev)
    a = nat.DrrPoseGradArgs(d_att=d_att.data_ptr(), pivots=d_piv.data_ptr(), grad=grad.data_ptr(), scratch=scratch.data_ptr(),
                            scratch_doubles=need, interp=nat.DRR_TRILINEAR, **shared)
    launch(dev, 'dfl_drr_pose_grad', a)
    return grad                                                   # stream order keeps the uploads alive until the kernels ran


def render_args(volume, objects, grid, interp='exact', step_mm=0.5, want_plen=False, want_labels=True, min_len_mm=1.0,
                tight_boxes=True, mapping=0):
    """args_for_records of pack_objects(objects), after the checks of render() -- render() below, and tools/bench_drr.py
    for repeated calls."""
    if not isinstance(volume, Volume):
        raise nat.DflError('drr.render needs a drr.Volume (device tensors; no CPU path)')
    if interp not in _INTERP:
        raise nat.DflError("drr.render: interp must be 'exact' or 'trilinear', got %r" % (interp,))
    if not float(step_mm) > 0:
        raise nat.DflError('drr.render: step_mm must be positive, got %r' % (step_mm,))
    if not float(min_len_mm) >= 0:
        raise nat.DflError('drr.render: min_len_mm must not be negative, got %r' % (min_len_mm,))
    return args_for_records(volume, pack_objects(volume, objects, grid, interp, tight_boxes), grid, interp, step_mm, want_plen,
                            want_labels, min_len_mm, mapping)


def render(volume, objects, grid, interp='exact', step_mm=0.5, want_plen=False, want_labels=True, min_len_mm=1.0,
           tight_boxes=True, mapping=0):
    """(att, plen, labels): the line integral of mu [H, W] float32, the per-label path lengths [n_labels, H, W] in mm
    (or None) and the label map [H, W] uint8 (or None; interp='trilinear' gives att alone).  With a leading view axis on
    `objects` ([[Obj]]) every output has one too.  mapping 1 is the row mapping tools/bench_drr.py measures."""
    a, (att, plen, lab), keep = render_args(volume, objects, grid, interp, step_mm, want_plen, want_labels, min_len_mm,
                                            tight_boxes, mapping)
    launch(att.device, 'dfl_drr_render', a)
    del keep
    if not _views(objects)[1]:
        att, plen, lab = att[0], None if plen is None else plen[0], None if lab is None else lab[0]
    return att, plen, lab
