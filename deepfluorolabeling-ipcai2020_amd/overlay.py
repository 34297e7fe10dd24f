"""Result overlays on the GPU (dfl_overlay_batch): the pixel work of the reference's overlay_est_ann.py,
overlay_est_heat.py and examples_dataset/make_preproc_overlays.py, for a whole batch in two launches.

render() reproduces the reference's fp32 arithmetic operation by operation -- min/max normalisation, TF.to_pil_image's
truncation to 8 bits, TF.to_tensor's / 255, the 0.35 alpha tint, the heat blend, and save_image's rounding (or, when
markers are drawn, the truncation of the second to_pil_image) -- and Pillow's filled ellipses through a stamp table
generated from Pillow (data/ellipse_stamps.txt, tools/gen_overlay_golden.py).  A constant image (max == min) has grey
level 0 where the reference divides 0 by 0.  There is no host path: CPU tensors are refused."""
import math
import os

import numpy as np
import torch

from . import _native as nat

ALPHA = 0.35
ANN_COLORS = ((0.0, 1.0, 0.0),   # pelvis green       (overlay_est_ann.py label_colors)
              (1.0, 0.0, 0.0),   # left femur red
              (0.0, 0.0, 1.0),   # right femur blue
              (1.0, 1.0, 0.0),   # yellow
              (0.0, 1.0, 1.0),   # cyan
              (1.0, 0.5, 0.0),   # orange
              (0.5, 0.0, 0.5))   # purple
HEAT_COLOR = (0.0, 1.0, 0.0)     # overlay_est_heat.py heat_base_color
STAMPS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'data', 'ellipse_stamps.txt')

_stamps_host = None
_stamps_dev = {}


def stamp_table():
    """(index [DIM*DIM] int32, spans int32, boxes set): Pillow's filled-ellipse stamps as the kernel reads them."""
    global _stamps_host
    if _stamps_host is None:
        D = nat.OVERLAY_STAMP_DIM
        index = np.full(D * D, -1, np.int32)
        spans, boxes = [], set()
        with open(STAMPS_PATH) as f:
            for line in f:
                if line.startswith('#') or not line.strip():
                    continue
                tok = line.split()
                w, h = int(tok[0]), int(tok[1])
                rows = [tuple(int(v) for v in t.split(':')) for t in tok[2:]]
                if len(rows) != h + 1 or not (0 <= w < D and 0 <= h < D):
                    raise nat.DflError('%s: bad stamp line for box (%d, %d)' % (STAMPS_PATH, w, h))
                index[w * D + h] = len(spans)
                spans += [(lo & 0xffff) | (hi << 16) for lo, hi in rows]
                boxes.add((w, h))
        _stamps_host = (index, np.array(spans, np.int32), frozenset(boxes))
    return _stamps_host


def _stamps_on(dev):
    t = _stamps_dev.get(dev)
    if t is None:
        index, spans, _ = stamp_table()
        t = _stamps_dev[dev] = (torch.from_numpy(index).to(dev), torch.from_numpy(spans).to(dev))
    return t


def box_sizes(radius):
    """Every box extent trunc(c + r) - trunc(c - r) a centre c can give (one more on each side for the rounding of c +- r)."""
    return range(max(int(math.floor(2 * radius)) - 2, 0), int(math.ceil(2 * radius)) + 2)


def check_radius(radius):
    """The stamp table must hold every box a centre can produce with this radius; DflError otherwise."""
    if not (radius >= 0 and math.isfinite(radius)):
        raise nat.DflError('overlay: radius must be finite and >= 0 (got %r)' % (radius,))
    boxes = stamp_table()[2]
    missing = [(w, h) for w in box_sizes(radius) for h in box_sizes(radius) if (w, h) not in boxes]
    if missing:
        raise nat.DflError('overlay: radius %g needs ellipse boxes outside the stamp table, e.g. %r' % (radius, missing[0]))


def grid_shape(B, H, W, nrow=8, padding=2):
    """Canvas [rows, cols] of torchvision's make_grid (a single image is returned unchanged)."""
    if B == 1:
        return H, W
    xmaps = min(nrow, B)
    ymaps = int(math.ceil(float(B) / xmaps))
    return (H + padding) * ymaps + padding, (W + padding) * xmaps + padding


def _batch(t, name, dims):
    if t.dim() == dims - 1:
        t = t.unsqueeze(0)
    if t.dim() != dims:
        raise nat.DflError('overlay.render: %s has shape %s' % (name, tuple(t.shape)))
    return t


def render(images, segs=None, num_classes=7, heats=None, gt_lands=None, radius=2, est_lands=None, cross=6,
           colors=ANN_COLORS, grid=False, heat_color=HEAT_COLOR):
    """uint8 RGB overlays of a batch, on the images' GPU.

    images [B,H,W] (or [H,W], [B,1,H,W]) float, converted to fp32; segs [B,H,W] integer labels (labels 1 ..
    min(num_classes - 1, len(colors)) are tinted); heats [B,H,W] float, blended in heat_color; gt_lands [B,L,2] (x, y)
    fp32 / fp64 centres of filled ellipses of this radius (non-finite = none); est_lands [B,L,2] integer (column, row)
    centres of +-cross crosses (negative = none).  Passing either marker tensor, even an empty one, selects the
    quantisation of the reference's marker path (truncation); otherwise save_image's rounding.
    Returns [B,H,W,3], or with grid=True the make_grid(nrow=8, padding=2) canvas [rows, cols, 3]."""
    if not torch.is_tensor(images) or not images.is_cuda:
        raise nat.DflError('overlay.render needs the images on the GPU (no CPU path)')
    dev = images.device
    img = images.detach()
    if img.dim() == 4 and img.shape[1] == 1:
        img = img[:, 0]
    img = _batch(img, 'images', 3).to(torch.float32).contiguous()
    B, H, W = img.shape
    if len(colors) > nat.OVERLAY_MAX_COLORS:
        raise nat.DflError('overlay.render: at most %d colours' % nat.OVERLAY_MAX_COLORS)
    a = nat.OverlayArgs(image=img.data_ptr(), B=B, H=H, W=W, ld_image=W, tint_scale=1 - ALPHA, radius=float(radius),
                        cross=int(cross), grid=int(bool(grid)))
    keep = [img]

    def on_dev(t, name, dtype, per_pixel):
        if not torch.is_tensor(t) or t.device != dev:
            raise nat.DflError('overlay.render: %s must be a tensor on %s' % (name, dev))
        t = _batch(t.detach(), name, 3)
        if per_pixel and tuple(t.shape) != (B, H, W):
            raise nat.DflError('overlay.render: %s has shape %s, images %s' % (name, tuple(t.shape), (B, H, W)))
        if dtype == torch.uint8 and t.dtype != torch.uint8:
            t = t.clamp(0, 255)                     # labels past 255 stay untinted
        t = t.to(dtype).contiguous()
        keep.append(t)
        return t

    if segs is not None:
        s = on_dev(segs, 'segs', torch.uint8, True)
        a.labels, a.ld_labels = s.data_ptr(), W
        a.n_tint = max(0, min(int(num_classes) - 1, len(colors)))
        for l, col in enumerate(colors):
            for c in range(3):
                a.tint_add[l][c] = ALPHA * col[c]      # rounded to fp32, as torch does with a Python-float operand
    if heats is not None:
        h = on_dev(heats, 'heats', torch.float32, True)
        a.heat, a.ld_heat = h.data_ptr(), W
        for c in range(3):
            a.heat_color[c] = heat_color[c]
    if gt_lands is not None:
        dt = torch.float64 if gt_lands.dtype == torch.float64 else torch.float32
        g = on_dev(gt_lands, 'gt_lands', dt, False)
        if g.shape[0] != B or g.shape[2] != 2 or g.shape[1] > nat.OVERLAY_MAX_MARKERS:
            raise nat.DflError('overlay.render: gt_lands must be [B, L <= %d, 2], got %s' % (nat.OVERLAY_MAX_MARKERS, tuple(g.shape)))
        if g.shape[1] > 0:
            check_radius(float(radius))
            idx, spans = _stamps_on(dev)
            a.gt_lands, a.n_gt, a.gt_f64 = g.data_ptr(), g.shape[1], int(dt == torch.float64)
            a.stamp_index, a.stamp_spans = idx.data_ptr(), spans.data_ptr()
    if est_lands is not None:
        e = on_dev(est_lands, 'est_lands', torch.int32, False)
        if e.shape[0] != B or e.shape[2] != 2 or e.shape[1] > nat.OVERLAY_MAX_MARKERS:
            raise nat.DflError('overlay.render: est_lands must be [B, L <= %d, 2], got %s' % (nat.OVERLAY_MAX_MARKERS, tuple(e.shape)))
        if e.shape[1] > 0:
            if int(cross) < 0:
                raise nat.DflError('overlay.render: cross must be >= 0')
            a.est_lands, a.n_est = e.data_ptr(), e.shape[1]
    a.quant = nat.OVERLAY_TRUNC if (gt_lands is not None or est_lands is not None) else nat.OVERLAY_ROUND
    if grid:
        out = torch.empty(grid_shape(B, H, W) + (3,), dtype=torch.uint8, device=dev)
    else:
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    scratch = torch.empty(B * nat.OVERLAY_SCRATCH_FLOATS, dtype=torch.float32, device=dev)
    a.out, a.scratch = out.data_ptr(), scratch.data_ptr()
    keep += [scratch]
    nat.call('dfl_overlay_batch', a, torch.cuda.current_stream(dev).cuda_stream)
    return out
