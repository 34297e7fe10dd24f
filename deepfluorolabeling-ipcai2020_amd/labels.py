"""Clean-up of predicted label maps on the GPU: connected components per value, keep-largest / drop-specks / close
pin-holes, and a dilated bone mask (csrc/labels.hip; definitions in include/dfl_hip.h).

Everything downstream of the network takes 'nn-segs' as the arg-max left it; a stray island of "left femur" on the right
side is enough to put a landmark there (est_lands_csv.py --use-seg).  ``clean`` is the usual remedy, per bone, without the
round trip through scipy.ndimage on the host; ``bone_mask`` turns the cleaned map into the pixel mask that
``register.Similarity(fixed, mask)`` takes.

All results are exact integers and canonical: the root of a component is the smallest flat index (row * W + col) of its
pixels, whatever the tile size or the order in which workgroups run.
"""
import torch

from . import _native as nat

__all__ = ['TILE', 'components', 'clean', 'bone_mask']

TILE = (nat.LABEL_TILE_H, nat.LABEL_TILE_W)      # (th, tw) of the components kernel's LDS tile


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
