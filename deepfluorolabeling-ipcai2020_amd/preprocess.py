"""Training files from the full-resolution dataset.

The reference's README says how its preprocessed files were made from the full-resolution file -- crop 50 pixels from
each border, log-transform, rotate by 180 degrees where the projection's flag (rot180 in dfl_amd.fullres) is set,
downsample by 2, 4, 8 or 16 -- but the program that did it is not part of the reference.  This module is that step
(DESIGN.md section 14 pins the arithmetic; tests/preproc_ref.py restates it in numpy), and its inverse for labels and
landmarks:

    crop window   rows crop .. R-crop-1, columns likewise: Rc x Cc = (R - 2 crop) x (C - 2 crop)
    rotation      cropped pixel (r, c) -> (Rc-1-r, Cc-1-c) where the flag is set
    reduction     output (i, j) of ceil(Rc / f) x ceil(Cc / f) covers rows i f .. min((i+1) f, Rc)-1, columns likewise

The pixel work is HIP (csrc/preproc.hip: dfl_preproc_projs, dfl_preproc_segs, dfl_restore_labels); tensors on the CPU
are refused.  Landmarks are a handful of numbers per projection and are mapped on the host in float64.
"""

import numpy as np
import torch

from . import _native as nat
from . import fullres, h5lite
from .fullres import SPECIMEN_ORDER, LAND_ORDER, specimen_order, land_order  # noqa: F401  (defined there, used from here)

__all__ = ['out_size', 'map_lands', 'unmap_lands', 'preprocess_projs', 'preprocess_segs', 'restore_labels',
           'convert_file', 'write_land_names', 'create_specimen', 'SPECIMEN_ORDER', 'LAND_ORDER']


def _check(R, C, crop, factor):
    R, C, crop, factor = int(R), int(C), int(crop), int(factor)
    if R < 1 or C < 1 or crop < 0:
        raise nat.DflError('preprocess: bad sizes (R %d, C %d, crop %d)' % (R, C, crop))
    if not 1 <= factor <= nat.PREPROC_MAX_FACTOR:
        raise nat.DflError('preprocess: factor must be 1..%d, got %d' % (nat.PREPROC_MAX_FACTOR, factor))
    if 2 * crop >= min(R, C):
        raise nat.DflError('preprocess: a crop of %d leaves nothing of %d x %d images' % (crop, R, C))
    return R, C, crop, factor


def out_size(R, C, crop=50, factor=8):
    """(Ro, Co) of R x C images: ceil((R - 2 crop) / factor), ceil((C - 2 crop) / factor)."""
    R, C, crop, factor = _check(R, C, crop, factor)
    return -(-(R - 2 * crop) // factor), -(-(C - 2 * crop) // factor)


def _lands_args(lands, rot180, R, C, crop, factor):
    R, C, crop, factor = _check(R, C, crop, factor)
    x = np.array(lands, dtype=np.float64)
    if x.ndim != 3 or x.shape[1] != 2:
        raise nat.DflError('preprocess: lands must be [N, 2, L] (row 0 the column), got shape %s' % (x.shape,))
    rot = np.array([bool(r) for r in rot180])
    if rot.shape != (x.shape[0],):
        raise nat.DflError('preprocess: %d rotation flags for %d projections' % (rot.size, x.shape[0]))
    return x, rot, np.array([C - 2 * crop - 1, R - 2 * crop - 1], np.float64)[None, :, None], crop, factor


def map_lands(lands, rot180, R, C, crop=50, factor=8):
    """Full-resolution (column, row) pixel-centre coordinates [N, 2, L] -> coordinates of the preprocessed image
    (float64): crop, rotate where flagged, reduce ((x + 0.5) / factor - 0.5).  Out-of-view landmarks are mapped like any
    other and stay finite."""
    x, rot, last, crop, factor = _lands_args(lands, rot180, R, C, crop, factor)
    x -= crop
    x[rot] = last - x[rot]
    return (x + 0.5) / factor - 0.5


def unmap_lands(lands, rot180, R, C, crop=50, factor=8):
    """The inverse of map_lands: preprocessed coordinates back onto the R x C detector frame."""
    x, rot, last, crop, factor = _lands_args(lands, rot180, R, C, crop, factor)
    x = (x + 0.5) * factor - 0.5
    x[rot] = last - x[rot]
    return x + crop


def _device_batch(t, what, dtypes):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise nat.DflError('preprocess.%s needs its tensor on the GPU (no CPU path)' % what)
    if t.dim() != 3:
        raise nat.DflError('preprocess.%s: [N, rows, cols] expected, got shape %s' % (what, tuple(t.shape)))
    if t.dtype not in dtypes:
        raise nat.DflError('preprocess.%s: dtype %s, expected one of %s' % (what, t.dtype, ', '.join(str(d) for d in dtypes)))
    if t.shape[0] < 1:
        raise nat.DflError('preprocess.%s: empty batch' % what)
    return t.detach().contiguous()


def _flags(rot180, N, dev, what):
    if torch.is_tensor(rot180) and rot180.device == dev and rot180.dtype == torch.int32 and tuple(rot180.shape) == (N,):
        return rot180.contiguous()                   # already on the device: no upload
    if len(rot180) != N:
        raise nat.DflError('preprocess.%s: %d rotation flags for %d images' % (what, len(rot180), N))
    return torch.tensor([int(bool(r)) for r in rot180], dtype=torch.int32).to(dev)


def preprocess_projs(pixels, rot180, crop=50, factor=8, log=True, min_intensity=1.0):
    """[N, R, C] float32 or uint16 intensities on the GPU -> [N, Ro, Co] float32: the box mean of
    log(I0) - log(max(I, min_intensity)), I0 the largest clamped intensity of the projection's crop window (log=True),
    or the box mean of I."""
    px = _device_batch(pixels, 'preprocess_projs', (torch.float32, torch.uint16))
    N, R, Cn = px.shape
    Ro, Co = out_size(R, Cn, crop, factor)
    if log and not float(min_intensity) > 0:
        raise nat.DflError('preprocess.preprocess_projs: min_intensity must be positive for the log transform')
    dev = px.device
    rot = _flags(rot180, N, dev, 'preprocess_projs')
    out = torch.empty((N, Ro, Co), dtype=torch.float32, device=dev)
    scratch = torch.empty(N, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        a = nat.PreprocProjsArgs(pixels=px.data_ptr(), rot180=rot.data_ptr(), out=out.data_ptr(), scratch=scratch.data_ptr(),
                                 N=N, R=R, C=Cn, crop=int(crop), factor=int(factor), u16=int(px.dtype == torch.uint16),
                                 log=int(bool(log)), min_intensity=float(min_intensity))
        nat.call('dfl_preproc_projs', a, torch.cuda.current_stream(dev).cuda_stream)
    return out


def preprocess_segs(segs, rot180, crop=50, factor=8):
    """[N, R, C] uint8 labels (0..15) on the GPU -> [N, Ro, Co] uint8: the most frequent label of each box, of equally
    frequent ones the smallest.  A label above 15 raises."""
    sg = _device_batch(segs, 'preprocess_segs', (torch.uint8,))
    N, R, Cn = sg.shape
    Ro, Co = out_size(R, Cn, crop, factor)
    dev = sg.device
    rot = _flags(rot180, N, dev, 'preprocess_segs')
    out = torch.empty((N, Ro, Co), dtype=torch.uint8, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        a = nat.PreprocSegsArgs(segs=sg.data_ptr(), rot180=rot.data_ptr(), out=out.data_ptr(), status=status.data_ptr(),
                                N=N, R=R, C=Cn, crop=int(crop), factor=int(factor))
        nat.call('dfl_preproc_segs', a, torch.cuda.current_stream(dev).cuda_stream)
    if int(status.item()) != 0:
        raise nat.DflError('preprocess.preprocess_segs: a label above 15 in the crop window (labels 0..15 are supported)')
    return out


def restore_labels(labels, rot180, R, C, crop=50, factor=8):
    """[N, Ro, Co] uint8 labels on the GPU -> [N, R, C] uint8 on the original detector frame: every pixel of the crop
    window takes the label of the box that contains it (rotation undone), the border of `crop` pixels is 0."""
    lb = _device_batch(labels, 'restore_labels', (torch.uint8,))
    Ro, Co = out_size(R, C, crop, factor)
    N = lb.shape[0]
    if tuple(lb.shape[1:]) != (Ro, Co):
        raise nat.DflError('preprocess.restore_labels: labels are %d x %d, %d x %d images with crop %d and factor %d give '
                           '%d x %d' % (lb.shape[1], lb.shape[2], R, C, crop, factor, Ro, Co))
    dev = lb.device
    rot = _flags(rot180, N, dev, 'restore_labels')
    out = torch.empty((N, int(R), int(C)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        a = nat.RestoreLabelsArgs(labels=lb.data_ptr(), rot180=rot.data_ptr(), out=out.data_ptr(), N=N, R=int(R), C=int(C),
                                  crop=int(crop), factor=int(factor))
        nat.call('dfl_restore_labels', a, torch.cuda.current_stream(dev).cuda_stream)
    return out


# ---- the full-resolution file -> the preprocessed file ----------------------------------------------------------------
def write_land_names(out, names):
    """The 'land-names' group of a training file: 'num-lands' and 'land-XX'."""
    g = out.create_group('land-names')
    g['num-lands'] = len(names)
    for l, name in enumerate(names):
        g['land-%02d' % l] = name


def create_specimen(out, index, n, Ro, Co, compression=None):
    """(group name 'NN', its 'projs' float32 and 'segs' uint8 datasets [n, Ro, Co], one image per chunk) of specimen
    number `index` (from 1) of a training file; the caller fills them and writes 'NN/lands'."""
    grp = '%02d' % index
    kw = dict(compression='gzip') if compression else {}
    d_projs = out.create_dataset(grp + '/projs', (n, Ro, Co), dtype='f4', chunks=(1, Ro, Co), **kw)
    d_segs = out.create_dataset(grp + '/segs', (n, Ro, Co), dtype='u1', chunks=(1, Ro, Co), **kw)
    return grp, d_projs, d_segs


def convert_file(src, dst, factor=8, crop=50, specimens=None, land_names=None, chunk=32, compression=None, log=True,
                 min_intensity=1.0, device=None, report=None):
    """Full-resolution layout (dfl_amd.fullres) -> preprocessed layout ('land-names/num-lands', 'land-names/land-XX',
    'NN/projs' float32, 'NN/segs' uint8, 'NN/lands' float32 [N, 2, L] with row 0 the column), `chunk` projections on the
    device at a time.  Returns [(specimen id, index, projections, (Ro, Co))]; report(line) gets one line per specimen."""
    if not torch.cuda.is_available():
        raise nat.DflError('preprocess.convert_file: no GPU visible (the reduction runs in HIP kernels; no CPU path)')
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if int(chunk) < 1:
        raise nat.DflError('preprocess.convert_file: chunk must be at least 1')
    f = fullres.Source(src)
    try:
        R, Cn = fullres.detector_size(f)
        Ro, Co = out_size(R, Cn, crop, factor)
        specimens = fullres.specimens(f, specimens, 'preprocess.convert_file: %s' % src)
        counts = {s: fullres.n_projections(f, s) for s in specimens}
        if land_names is None:
            present = set()
            for s in specimens:
                for p in range(counts[s]):
                    present.update(f.children(fullres.projection_prefix(s, p) + 'gt-landmarks'))
            land_names = land_order(present)
        land_names = list(land_names)
        L = len(land_names)
        done = []
        out = h5lite.File(dst, 'w')
        try:
            write_land_names(out, land_names)
            for k, s in enumerate(specimens):
                num = counts[s]
                if num < 1:
                    raise nat.DflError('preprocess.convert_file: specimen %s has no projections' % s)
                grp, d_projs, d_segs = create_specimen(out, k + 1, num, Ro, Co, compression)
                lands = np.zeros((num, 2, L), np.float64)
                flags = []
                for p0 in range(0, num, int(chunk)):
                    imgs, segs, rots = [], [], []
                    for p in range(p0, min(p0 + int(chunk), num)):
                        pfx = fullres.projection_prefix(s, p)
                        img = np.asarray(f.get(pfx + 'image/pixels'))
                        seg = np.asarray(f.get(pfx + 'gt-seg/pixels'))
                        if img.shape != (R, Cn) or seg.shape != (R, Cn):
                            raise nat.DflError('preprocess.convert_file: %s is %s / %s, proj-params say %s'
                                               % (pfx, img.shape, seg.shape, (R, Cn)))
                        if img.dtype != np.uint16:
                            img = img.astype(np.float32, copy=False)
                        have = fullres.gt_landmarks(f, pfx, land_names)
                        for l, name in enumerate(land_names):
                            if name not in have:
                                raise nat.DflError('preprocess.convert_file: specimen %s, projection %03d has no landmark %s'
                                                   % (s, p, name))
                            lands[p, :, l] = have[name]
                        imgs.append(img)
                        segs.append(seg.astype(np.uint8, copy=False))
                        rots.append(fullres.rot180(f, pfx))
                    if len({im.dtype for im in imgs}) > 1:          # uint16 next to float pixels: all as fp32, said out loud
                        imgs = [im.astype(np.float32) for im in imgs]
                    px = torch.from_numpy(np.stack(imgs)).to(dev)
                    sg = torch.from_numpy(np.stack(segs)).to(dev)
                    d_projs[p0:p0 + len(imgs)] = preprocess_projs(px, rots, crop, factor, log, min_intensity).cpu().numpy()
                    d_segs[p0:p0 + len(imgs)] = preprocess_segs(sg, rots, crop, factor).cpu().numpy()
                    flags += rots
                out[grp + '/lands'] = map_lands(lands, flags, R, Cn, crop, factor).astype(np.float32)
                done.append((s, k + 1, num, (Ro, Co)))
                if report is not None:
                    report('%s -> %s: %d projections, %d x %d' % (s, grp, num, Ro, Co))
        finally:
            out.close()
    finally:
        f.close()
    return done
