"""Clean-up of predicted label maps on the GPU: connected components per value, keep-largest / drop-specks / close
pin-holes, and a dilated bone mask (csrc/labels.hip; definitions in include/dfl_hip.h).

Everything downstream of the network takes 'nn-segs' as the arg-max left it; a stray island of "left femur" on the right
side is enough to put a landmark there (est_lands_csv.py --use-seg).  ``clean`` is the usual remedy, per bone, without the
round trip through scipy.ndimage on the host; ``bone_mask`` turns the cleaned map into the pixel mask that
``register.Similarity(fixed, mask)`` takes.

All results are exact integers and canonical: the root of a component is the smallest flat index (row * W + col) of its
pixels, whatever the tile size or the order in which workgroups run.

``edt`` is the exact squared Euclidean distance transform to a label set or to its boundary, and ``surface_distances``
scores a predicted map where Dice cannot: Hausdorff distance, its percentile and the average symmetric surface distance per
bone (csrc/labels_dist.hip).
"""
import ctypes

import numpy as np
import torch

from . import _native as nat

__all__ = ['TILE', 'components', 'clean', 'bone_mask', 'edt', 'surface_distances']

TILE = (nat.LABEL_TILE_H, nat.LABEL_TILE_W)      # (th, tw) of the components kernel's LDS tile
# surface_distances works through a stack in chunks of images whose two squared-distance arrays and row scratch
# (3 * (num_classes - 1) * H * W int32 per image) stay below this many bytes; a single image may exceed it
SURFACE_CHUNK_BYTES = 256 << 20


def _device_labels(t, who):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise nat.DflError('labels.%s: segs must be a tensor on the GPU (no CPU path)' % who)
    if t.dim() not in (2, 3) or t.dtype != torch.uint8:
        raise nat.DflError('labels.%s: segs has shape %s and dtype %s: [B, H, W] or [H, W] of torch.uint8 expected'
                           % (who, tuple(t.shape), t.dtype))
    if t.numel() == 0:
        raise nat.DflError('labels.%s: segs has shape %s: an empty label map' % (who, tuple(t.shape)))
    t = t.detach().contiguous()
    return t if t.dim() == 3 else t.unsqueeze(0)


def _connectivity(connectivity, who):
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise nat.DflError('labels.%s: a connectivity of %r (4 or 8)' % (who, connectivity))
    return int(connectivity)


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _components(s, connectivity):
    """(root, area, info) of a contiguous uint8 [B, H, W] on the device."""
    B, H, W = s.shape
    root = torch.empty((B, H, W), dtype=torch.int32, device=s.device)
    area = torch.empty_like(root)
    info = torch.empty_like(root)        # the uint32 words of dfl_label_components; bit 31 is the sign here
    with torch.cuda.device(s.device):
        nat.check(nat.lib().dfl_label_components(s.data_ptr(), B, H, W, connectivity, root.data_ptr(), area.data_ptr(),
                                                 info.data_ptr(), _stream(s)), 'dfl_label_components')
    return root, area, info


def components(segs, connectivity=8):
    """Connected components of every value of a label map (dfl_label_components): uint8 [B, H, W] or [H, W] on the device ->
    (root, area, info) of the same shape.  root: int32, the smallest flat index (row * W + col) of the pixel's component; area:
    int32, the component's pixel count at its root pixel and 0 elsewhere; info: int32 holding the header's uint32 word at
    each root -- bit 31 (the sign) = touches the border, bits 0..30 = the values (30 = "30 or more") of the 4-neighbours
    outside the component."""
    s = _device_labels(segs, 'components')
    out = _components(s, _connectivity(connectivity, 'components'))
    return out if segs.dim() == 3 else tuple(t[0] for t in out)


def _select(s, comp, num_classes, keep, min_area, fill_below, counts):
    B, H, W = s.shape
    root, area, info = comp
    lib = nat.lib()
    nbytes = nat.check(lib.dfl_label_select_scratch_bytes(B, num_classes), 'dfl_label_select_scratch_bytes')
    scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=s.device)
    out = torch.empty_like(s)
    with torch.cuda.device(s.device):
        nat.check(lib.dfl_label_select(s.data_ptr(), root.data_ptr(), area.data_ptr(), info.data_ptr(), B, H, W, num_classes,
                                       keep, min_area, fill_below, out.data_ptr(), counts.data_ptr(), scratch.data_ptr(),
                                       _stream(s)), 'dfl_label_select')
    return out


def clean(segs, num_classes=7, connectivity=8, keep='largest', min_area=0, fill_holes=0):
    """Per-bone clean-up of a label map: uint8 [B, H, W] or [H, W] on the device -> (cleaned, stats).

    Stage 1: components at ``connectivity``; of every label 1..num_classes-1 the components smaller than ``min_area`` pixels
    and, with keep='largest', all but the largest of the image (ties: the one that comes first in row-major order) become
    background.  Stage 2, only when ``fill_holes`` > 0: background components of the stage-1 result of at most ``fill_holes``
    pixels that do not touch the border and are enclosed by exactly one label take that label.  Background is always
    4-connected there, so a ring closed only diagonally still encloses its hole.  The default leaves holes alone: the
    obturator foramen is a true hole of a projected hemipelvis.

    stats = {'removed': int32 [B, C], 'filled': int32 [B, C]} on the host: pixels per image and label ([C] for an [H, W]
    input)."""
    s = _device_labels(segs, 'clean')
    connectivity = _connectivity(connectivity, 'clean')
    if keep not in ('largest', 'all'):
        raise nat.DflError("labels.clean: keep=%r ('largest' or 'all')" % (keep,))
    ints = all(isinstance(v, int) and not isinstance(v, bool) for v in (num_classes, min_area, fill_holes))
    if not ints or not 2 <= num_classes <= nat.LABEL_MAX_CLASSES or min_area < 0 or fill_holes < 0:
        raise nat.DflError('labels.clean: num_classes=%r (2..%d), min_area=%r and fill_holes=%r (integers, not negative)'
                           % (num_classes, nat.LABEL_MAX_CLASSES, min_area, fill_holes))
    B = s.shape[0]
    fill_holes = min(fill_holes, 2 ** 31 - 1)
    removed = torch.empty((B, num_classes, 2), dtype=torch.int32, device=s.device)
    out = _select(s, _components(s, connectivity), num_classes, 1 if keep == 'largest' else 0, min_area, 0, removed)
    filled = None
    if fill_holes > 0:
        filled = torch.empty_like(removed)
        out = _select(out, _components(out, 4), num_classes, 0, 0, fill_holes, filled)
    stats = {'removed': removed[:, :, 0].cpu(),
             'filled': filled[:, :, 1].cpu() if filled is not None else torch.zeros((B, num_classes), dtype=torch.int32)}
    if segs.dim() == 2:
        return out[0], {k: v[0] for k, v in stats.items()}
    return out, stats


def bone_mask(segs, labels, dilate=0):
    """uint8 mask of the pixels within ``dilate`` pixels (Euclidean, 0..32) of a pixel whose label is in ``labels`` (an integer
    or several, each 0..31): 1 inside, 0 outside, same shape as ``segs`` -- the dtype and layout register.Similarity(fixed,
    mask) takes (dfl_label_dilate)."""
    s = _device_labels(segs, 'bone_mask')
    labels = [labels] if isinstance(labels, int) else list(labels)
    if not labels or any(isinstance(l, bool) or not isinstance(l, int) or not 0 <= l < 32 for l in labels):
        raise nat.DflError('labels.bone_mask: labels=%r (one or more integers 0..31)' % (labels,))
    if isinstance(dilate, bool) or not isinstance(dilate, int) or not 0 <= dilate <= nat.LABEL_MAX_RADIUS:
        raise nat.DflError('labels.bone_mask: dilate=%r (an integer 0..%d)' % (dilate, nat.LABEL_MAX_RADIUS))
    bits = 0
    for l in labels:
        bits |= 1 << l
    B, H, W = s.shape
    mask = torch.empty_like(s)
    with torch.cuda.device(s.device):
        nat.check(nat.lib().dfl_label_dilate(s.data_ptr(), B, H, W, bits, dilate, mask.data_ptr(), _stream(s)),
                  'dfl_label_dilate')
    return mask if segs.dim() == 3 else mask[0]


def _set_bits(labels, who):
    bits = 0
    for l in labels:
        if isinstance(l, bool) or not isinstance(l, int) or not 0 <= l < 32:
            raise nat.DflError('labels.%s: label %r in a label set (integers 0..31)' % (who, l))
        bits |= 1 << l
    return bits


def _label_sets(label_sets, who):
    """-> (list of 32-bit words, nested): an int or a flat sequence of ints is one set, a sequence of sequences several."""
    if isinstance(label_sets, int):
        return [_set_bits([label_sets], who)], False
    try:
        sets = list(label_sets)
    except TypeError:
        raise nat.DflError('labels.%s: label_sets=%r (an integer, integers, or several sequences of integers)' % (who, label_sets))
    if not sets:
        raise nat.DflError('labels.%s: an empty label set' % who)
    if all(isinstance(s, int) for s in sets):
        return [_set_bits(sets, who)], False
    if any(isinstance(s, int) for s in sets):
        raise nat.DflError('labels.%s: label_sets=%r mixes integers and sequences' % (who, label_sets))
    sets = [list(s) for s in sets]
    if any(not s for s in sets) or len(sets) > nat.LABEL_MAX_CLASSES:
        raise nat.DflError('labels.%s: %d label sets (1..%d, none of them empty)' % (who, len(sets), nat.LABEL_MAX_CLASSES))
    return [_set_bits(s, who) for s in sets], True


def _edt(s, words, boundary, rowdist=None, out=None):
    """dfl_label_edt of a contiguous uint8 [B, H, W] on the device -> int32 [B, S, H, W]; rowdist / out may be passed in."""
    B, H, W = s.shape
    S = len(words)
    if rowdist is None:
        rowdist = torch.empty(B * S * (H * W + 1), dtype=torch.int32, device=s.device)
    if out is None:
        out = torch.empty((B, S, H, W), dtype=torch.int32, device=s.device)
    host = (ctypes.c_uint32 * S)(*words)
    with torch.cuda.device(s.device):
        nat.check(nat.lib().dfl_label_edt(s.data_ptr(), B, H, W, ctypes.addressof(host), S, 1 if boundary else 0,
                                          rowdist.data_ptr(), out.data_ptr(), _stream(s)), 'dfl_label_edt')
    return out


def edt(segs, label_sets, boundary=False):
    """Exact squared Euclidean distance transform (dfl_label_edt): uint8 [B, H, W] or [H, W] on the device -> int32, per pixel
    the smallest drow^2 + dcol^2 to a pixel of the same image whose label is in the set (``boundary=True``: to a boundary
    pixel of the set -- an in-set pixel with a 4-neighbour outside the set or on the image border).  nat.LABEL_EDT_NONE
    everywhere in an image without such a pixel.

    ``label_sets``: an integer or a flat sequence of integers 0..31 is ONE set and the result has the shape of ``segs``; a
    sequence of sequences is S sets and the result has an extra dimension after the batch: [B, S, H, W] ([S, H, W]).

    ``labels.edt(segs, which) <= r * r`` is the mask of the pixels within r pixels of the set: bone_mask for radii beyond its
    32."""
    s = _device_labels(segs, 'edt')
    words, nested = _label_sets(label_sets, 'edt')
    if not isinstance(boundary, (bool, int)) or boundary not in (0, 1):
        raise nat.DflError('labels.edt: boundary=%r (False or True)' % (boundary,))
    out = _edt(s, words, bool(boundary))
    if not nested:
        out = out[:, 0]
    return out if segs.dim() == 3 else out[0]


def _surface_chunk(e, g, C, percentile, rowdist, d2g, d2e):
    """The per-direction figures of one chunk of images, on the host: n [B, C-1, 2] int32, max2 int32, sum float64, and the
    order statistics kth2 [B, C-1, 2] int32 of the ranks floor(pos), min(floor(pos) + 1, N - 1) with their weights."""
    B, H, W = e.shape
    lib = nat.lib()
    words = [1 << l for l in range(1, C)]
    _edt(g, words, True, rowdist, d2g)
    _edt(e, words, True, rowdist, d2e)
    nbytes = nat.check(lib.dfl_label_surface_scratch_bytes(B, H, W, C), 'dfl_label_surface_scratch_bytes')
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=e.device)
    n = torch.empty((B, C - 1, 2), dtype=torch.int32, device=e.device)
    max2 = torch.empty_like(n)
    total = torch.empty((B, C - 1, 2), dtype=torch.float64, device=e.device)
    with torch.cuda.device(e.device):
        nat.check(lib.dfl_label_surface_stats(e.data_ptr(), g.data_ptr(), B, H, W, C, d2g.data_ptr(), d2e.data_ptr(),
                                              n.data_ptr(), max2.data_ptr(), total.data_ptr(), scratch.data_ptr(), _stream(e)),
                  'dfl_label_surface_stats')
    n_h = n.cpu()                                              # the one read the ranks need
    N = n_h.sum(-1).to(torch.int64)
    both = (n_h[..., 0] > 0) & (n_h[..., 1] > 0)
    pos = (percentile / 100.0) * (N - 1).clamp(min=0).to(torch.float64)
    lo = pos.floor().to(torch.int64)
    hi = torch.minimum(lo + 1, (N - 1).clamp(min=0))
    ranks_h = torch.stack([lo, hi], -1).to(torch.int32)
    ranks_h[~both] = -1
    ranks = ranks_h.to(e.device)
    kth2 = torch.empty_like(n)
    with torch.cuda.device(e.device):
        nat.check(lib.dfl_label_surface_select(e.data_ptr(), g.data_ptr(), B, H, W, C, d2g.data_ptr(), d2e.data_ptr(),
                                               ranks.data_ptr(), kth2.data_ptr(), scratch.data_ptr(), _stream(e)),
                  'dfl_label_surface_select')
    return n_h, max2.cpu(), total.cpu(), kth2.cpu(), pos - lo.to(torch.float64)


def surface_distances(est, gt, num_classes=7, spacing=1.0, percentile=95.0):
    """Boundary distances between a predicted label map and the ground truth, per image and label 1..num_classes-1: uint8
    [B, H, W] or [H, W] on the device, both -> a dict of host tensors [B, C-1] ([C-1]):

      hd              Hausdorff distance: the larger of the two directed maxima                       float64
      hdp             the ``percentile``-th percentile of the union of both directions' distances     float64
                      (numpy's default linear interpolation)
      assd            average symmetric surface distance: the mean of the two directed means          float64
      mean_est_to_gt, mean_gt_to_est   the directed means                                             float64
      n_est, n_gt     boundary pixels of the label in either map                                      int32

    A distance runs from a boundary pixel of the label in one map to the nearest boundary pixel of the label in the other
    (boundary: a 4-neighbour of another value, or the image border), in pixels times ``spacing``.  A label in neither map
    gives 0.0 everywhere, a label in only one map inf.  The distance transforms, counts, maxima, sums and order statistics
    are computed on the device (dfl_label_edt, dfl_label_surface_stats, dfl_label_surface_select), exactly and with the
    same bits on every run; the stack is worked through in chunks of images (SURFACE_CHUNK_BYTES)."""
    e = _device_labels(est, 'surface_distances')
    g = _device_labels(gt, 'surface_distances')
    if e.shape != g.shape or e.device != g.device:
        raise nat.DflError('labels.surface_distances: est %s on %s and gt %s on %s differ' % (tuple(e.shape), e.device, tuple(g.shape), g.device))
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 2 <= num_classes <= nat.LABEL_MAX_CLASSES:
        raise nat.DflError('labels.surface_distances: num_classes=%r (an integer 2..%d)' % (num_classes, nat.LABEL_MAX_CLASSES))
    spacing, percentile = float(spacing), float(percentile)
    if not spacing > 0.0 or not 0.0 <= percentile <= 100.0:
        raise nat.DflError('labels.surface_distances: spacing=%r (positive), percentile=%r (0..100)' % (spacing, percentile))
    B, H, W = e.shape
    C = num_classes
    per_image = 3 * (C - 1) * H * W * 4
    step = max(1, min(B, SURFACE_CHUNK_BYTES // per_image))
    rowdist = torch.empty(step * (C - 1) * (H * W + 1), dtype=torch.int32, device=e.device)
    d2g = torch.empty((step, C - 1, H, W), dtype=torch.int32, device=e.device)
    d2e = torch.empty_like(d2g)
    parts = [_surface_chunk(e[i:i + step], g[i:i + step], C, percentile, rowdist, d2g[:min(step, B - i)], d2e[:min(step, B - i)])
             for i in range(0, B, step)]
    # the last arithmetic in numpy: its float64 sqrt is the correctly rounded one (torch's vectorised CPU sqrt is not always)
    n, max2, total, kth2, frac = (torch.cat([p[k] for p in parts]).numpy() for k in range(5))
    n0, n1 = n[..., 0], n[..., 1]
    both, neither = (n0 > 0) & (n1 > 0), (n0 == 0) & (n1 == 0)

    def settle(v):          # the label in both maps: v; in neither: 0; in one only: inf
        return torch.from_numpy(np.where(both, v * spacing, np.where(neither, 0.0, np.inf)))
    means = total / np.maximum(n, 1).astype(np.float64)
    k = np.sqrt(np.maximum(kth2, 0).astype(np.float64))
    out = {'hd': settle(np.sqrt(max2.max(-1).astype(np.float64))),
           'hdp': settle(k[..., 0] + frac * (k[..., 1] - k[..., 0])),
           'assd': settle((means[..., 0] + means[..., 1]) / 2.0),
           'mean_est_to_gt': settle(means[..., 0]), 'mean_gt_to_est': settle(means[..., 1]),
           'n_est': torch.from_numpy(np.ascontiguousarray(n0)), 'n_gt': torch.from_numpy(np.ascontiguousarray(n1))}
    return out if est.dim() == 3 else {key: v[0] for key, v in out.items()}
