"""The reference's full-resolution file (hdf5_layouts/Readme.md): the one place that knows its names.

    proj-params/{intrinsic, extrinsic, num-rows, num-cols, ...}
    <specimen>/vol/{pixels, dir-mat, spacing, origin}, <specimen>/vol-seg/image/{the same}, <specimen>/vol-landmarks/<name>
    <specimen>/projections/NNN/{image/pixels, gt-seg/pixels, gt-landmarks/<name>, rot-180-for-up,
                                gt-poses/{cam-to-{pelvis,left-femur,right-femur}-vol, {left,right}-femur-good-fov}}

Source opens an .h5 (h5lite) or an .npz with the same names as keys; the functions below read through anything with
get(path) / children(path), in float64 where they return geometry.  numpy and h5lite only: no tensors, no kernels.
"""
import numpy as np

from . import h5lite
from ._native import DflError

__all__ = ['Source', 'scalar', 'detector_size', 'proj_params', 'specimens', 'n_projections', 'projection_prefix', 'gt_poses', 'rot180', 'femur_fov',
           'volume_frame', 'volume_landmarks', 'gt_landmarks', 'specimen_order', 'land_order', 'SPECIMEN_ORDER', 'LAND_ORDER', 'POSES']

# README of the reference: the preprocessed files number the specimens 01..06 in this order
SPECIMEN_ORDER = ['17-1882', '18-1109', '18-0725', '18-2799', '18-2800', '17-1905']
# the reference's landmark list (land-00 .. land-13 of its preprocessed files)
LAND_ORDER = ['FH-l', 'FH-r', 'GSN-l', 'GSN-r', 'IOF-l', 'IOF-r', 'MOF-l', 'MOF-r', 'SPS-l', 'SPS-r', 'IPS-l', 'IPS-r',
              'ASIS-l', 'ASIS-r']
POSES = ('cam-to-pelvis-vol', 'cam-to-left-femur-vol', 'cam-to-right-femur-vol')


class Source:
    """get(path) -> numpy value, children(path) -> sorted names below path, for an .h5 (h5lite) or .npz file."""

    def __init__(self, path):
        self._f = None
        if str(path).endswith('.npz'):
            self._z = np.load(path)
            self._keys = list(self._z.files)
        else:
            self._f = h5lite.File(path, 'r')
            self._z = None
        self.h5 = self._f                   # the open h5lite file (None for an .npz), for copies of groups as they are stored

    def get(self, path):
        if self._z is not None:
            return self._z[path]
        return self._f[path][()]

    def children(self, path=''):
        if self._z is not None:
            pre = path.rstrip('/') + '/' if path else ''
            return sorted({k[len(pre):].split('/')[0] for k in self._keys if k.startswith(pre) and len(k) > len(pre)})
        node = self._f[path] if path else self._f
        return sorted(node.keys())

    def close(self):
        if self._f is not None:
            self._f.close()


def specimen_order(ids):
    """The README's numbering when exactly its six specimens are present, else sorted."""
    ids = list(ids)
    return list(SPECIMEN_ORDER) if sorted(ids) == sorted(SPECIMEN_ORDER) else sorted(ids)


def land_order(present):
    """The reference's list filtered to the names present, then any other names, sorted."""
    present = set(present)
    return [n for n in LAND_ORDER if n in present] + sorted(present - set(LAND_ORDER))


def scalar(v):
    return np.asarray(v).reshape(-1)[0]


def _f64(src, path, shape):
    return np.asarray(src.get(path)).astype(np.float64).reshape(shape)


def detector_size(src):
    """(rows, cols): all of 'proj-params' that a reader of the pixels alone needs (and all that some files have)."""
    return int(scalar(src.get('proj-params/num-rows'))), int(scalar(src.get('proj-params/num-cols')))


def proj_params(src):
    """(K [3, 3], E [4, 4], rows, cols)."""
    return (_f64(src, 'proj-params/intrinsic', (3, 3)), _f64(src, 'proj-params/extrinsic', (4, 4))) + detector_size(src)


def specimens(src, wanted=None, who='fullres'):
    """The specimen ids to work on: `wanted` as given when the file has them all, by default all in specimen_order.
    `who` ('<caller>: <file>') opens the message of the two refusals."""
    found = [k for k in src.children() if k != 'proj-params']
    if wanted is None:
        wanted = specimen_order(found)
    else:
        wanted = list(wanted)
        missing = [s for s in wanted if s not in found]
        if missing:
            raise DflError('%s has no specimen %s' % (who, ', '.join(missing)))
    if not wanted:
        raise DflError('%s holds no specimen' % who)
    return wanted


def n_projections(src, spec):
    return len(src.children(spec + '/projections'))


def projection_prefix(spec, p):
    return '%s/projections/%03d/' % (spec, int(p))


def gt_poses(src, pfx):
    """{name: P}: the three cam-to-*-vol matrices of one projection."""
    return {k: _f64(src, pfx + 'gt-poses/' + k, (4, 4)) for k in POSES}


def rot180(src, pfx):
    return bool(scalar(src.get(pfx + 'rot-180-for-up')))


def femur_fov(src, pfx, default=None):
    """(left, right) good-fov flags as ints; a flag the file lacks reads as `default`, or raises KeyError without one."""
    have = src.children(pfx + 'gt-poses')
    return tuple(int(default) if default is not None and n not in have else int(scalar(src.get(pfx + 'gt-poses/' + n)))
                 for n in ('left-femur-good-fov', 'right-femur-good-fov'))


def volume_frame(src, spec, image='vol'):
    """(dir_mat [3, 3], spacing [3], origin [3]) of '<specimen>/vol', or of another image group of the specimen."""
    grp = '%s/%s/' % (spec, image)
    return _f64(src, grp + 'dir-mat', (3, 3)), _f64(src, grp + 'spacing', -1), _f64(src, grp + 'origin', -1)


def volume_landmarks(src, spec):
    """{name: [3]} of '<specimen>/vol-landmarks', in the order of children()."""
    return {n: _f64(src, '%s/vol-landmarks/%s' % (spec, n), -1)[:3] for n in src.children(spec + '/vol-landmarks')}


def gt_landmarks(src, pfx, names=None):
    """{name: [2] (column, row)} of one projection's 'gt-landmarks', in the order of children(); with `names`, only
    those of them that the projection has are read."""
    return {n: _f64(src, pfx + 'gt-landmarks/' + n, -1)[:2] for n in src.children(pfx + 'gt-landmarks') if names is None or n in names}
