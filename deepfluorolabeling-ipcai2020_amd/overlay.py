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
NROW, PADDING = 8, 2             # make_grid's nrow and padding, as the kernels have them (csrc/overlay.h: OVL_NROW, OVL_PAD)
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


def grid_shape(B, H, W, nrow=NROW, padding=PADDING):
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


def _images(images, who, dtypes=None, channel=False):
    """overlay.<who>'s images, on the GPU (of one of dtypes if given), as fp32 [B,H,W]; channel: [B,1,H,W] is [B,H,W]."""
    if not torch.is_tensor(images) or not images.is_cuda:
        raise nat.DflError('overlay.%s needs the images on the GPU (no CPU path)' % who)
    if dtypes is not None and images.dtype not in dtypes:
        raise nat.DflError('overlay.%s: image pixels must be float32 or float64, got %s' % (who, images.dtype))
    img = images.detach()
    if channel and img.dim() == 4 and img.shape[1] == 1:
        img = img[:, 0]
    return _batch(img, 'images', 3).to(torch.float32).contiguous()


def _on_dev(t, who, name, img, dtype, per_pixel=True):
    """overlay.<who>'s tensor `name` as a contiguous batch of dtype on the images' device; per_pixel: at their shape."""
    if not torch.is_tensor(t) or t.device != img.device:
        raise nat.DflError('overlay.%s: %s must be a tensor on %s' % (who, name, img.device))
    t = _batch(t.detach(), name, 3)
    if per_pixel and t.shape != img.shape:
        raise nat.DflError('overlay.%s: %s has shape %s, images %s' % (who, name, tuple(t.shape), tuple(img.shape)))
    if dtype == torch.uint8 and t.dtype != torch.uint8:
        t = t.clamp(0, 255)                         # labels past 255 stay untinted
    return t.to(dtype).contiguous()


def _fill_tint(a, colors):
    for l, col in enumerate(colors):
        for c in range(3):
            a.tint_add[l][c] = ALPHA * col[c]       # rounded to fp32, as torch does with a Python-float operand


def _scratch(img):
    """The min / max record both entry points write before they render: OVERLAY_SCRATCH_FLOATS per image."""
    return torch.empty(img.shape[0] * nat.OVERLAY_SCRATCH_FLOATS, dtype=torch.float32, device=img.device)


def render(images, segs=None, num_classes=7, heats=None, gt_lands=None, radius=2, est_lands=None, cross=6,
           colors=ANN_COLORS, grid=False, heat_color=HEAT_COLOR):
    """uint8 RGB overlays of a batch, on the images' GPU.

    images [B,H,W] (or [H,W], [B,1,H,W]) float, converted to fp32; segs [B,H,W] integer labels (labels 1 ..
    min(num_classes - 1, len(colors)) are tinted); heats [B,H,W] float, blended in heat_color; gt_lands [B,L,2] (x, y)
    fp32 / fp64 centres of filled ellipses of this radius (non-finite = none); est_lands [B,L,2] integer (column, row)
    centres of +-cross crosses (negative = none).  Passing either marker tensor, even an empty one, selects the
    quantisation of the reference's marker path (truncation); otherwise save_image's rounding.
    Returns [B,H,W,3], or with grid=True the make_grid(nrow=8, padding=2) canvas [rows, cols, 3]."""
    img = _images(images, 'render', channel=True)
    dev = img.device
    B, H, W = img.shape
    if len(colors) > nat.OVERLAY_MAX_COLORS:
        raise nat.DflError('overlay.render: at most %d colours' % nat.OVERLAY_MAX_COLORS)
    a = nat.OverlayArgs(image=img.data_ptr(), B=B, H=H, W=W, ld_image=W, tint_scale=1 - ALPHA, radius=float(radius),
                        cross=int(cross), grid=int(bool(grid)))
    if segs is not None:
        s = _on_dev(segs, 'render', 'segs', img, torch.uint8)
        a.labels, a.ld_labels = s.data_ptr(), W
        a.n_tint = max(0, min(int(num_classes) - 1, len(colors)))
        _fill_tint(a, colors)
    if heats is not None:
        h = _on_dev(heats, 'render', 'heats', img, torch.float32)
        a.heat, a.ld_heat = h.data_ptr(), W
        for c in range(3):
            a.heat_color[c] = heat_color[c]
    if gt_lands is not None:
        dt = torch.float64 if gt_lands.dtype == torch.float64 else torch.float32
        g = _on_dev(gt_lands, 'render', 'gt_lands', img, dt, per_pixel=False)
        if g.shape[0] != B or g.shape[2] != 2 or g.shape[1] > nat.OVERLAY_MAX_MARKERS:
            raise nat.DflError('overlay.render: gt_lands must be [B, L <= %d, 2], got %s' % (nat.OVERLAY_MAX_MARKERS, tuple(g.shape)))
        if g.shape[1] > 0:
            check_radius(float(radius))
            idx, spans = _stamps_on(dev)
            a.gt_lands, a.n_gt, a.gt_f64 = g.data_ptr(), g.shape[1], int(dt == torch.float64)
            a.stamp_index, a.stamp_spans = idx.data_ptr(), spans.data_ptr()
    if est_lands is not None:
        e = _on_dev(est_lands, 'render', 'est_lands', img, torch.int32, per_pixel=False)
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
    scratch = _scratch(img)
    a.out, a.scratch = out.data_ptr(), scratch.data_ptr()
    nat.call('dfl_overlay_batch', a, torch.cuda.current_stream(dev).cuda_stream)
    return out


# ---- full-resolution dataset overlays (examples_dataset/make_full_res_overlays.py; dfl_fullres_overlay) --------------
FULLRES_COLORS = ANN_COLORS[:6]          # make_full_res_overlays.py label_colors
FULLRES_RADIUS = 16                      # its get_box box_radius
FULLRES_DS = 0.125                       # its overlay_ds_factor
FULLRES_TEXTS = ('L. Femur FOV OK', 'R. Femur FOV OK')
FULLRES_FH = ('FH-l', 'FH-r')            # the landmark each text is drawn at
TEXT_STAMPS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'data', 'text_stamps.txt')
PIL_PRECISION_BITS = 22                  # libImaging/Resample.c, 8-bit images

_text_host = None
_text_dev = {}
_plans = {}
_plans_dev = {}


class TextStamps:
    """Pillow 12.2's default-font masks of FULLRES_TEXTS, as data/text_stamps.txt stores them.

    For a start fraction f (math.modf of the draw position), per axis the bin is the number of rule thresholds t with
    f >= t; (string, x bin, y bin) names one mask with its offset from (int(x), int(y))."""

    def __init__(self, path=TEXT_STAMPS_PATH):
        self.strings, self.rules, self.index = {}, {}, {}
        table, masks = [], []
        nbytes = 0
        with open(path) as f:
            for line in f:
                if line.startswith('#') or not line.strip():
                    continue
                tok = line.split()
                if tok[0] == 'string':
                    self.strings[line.split(None, 2)[2].rstrip('\n')] = int(tok[1])
                elif tok[0] == 'rule':
                    self.rules[tok[1]] = tuple(float.fromhex(t) for t in tok[2:])
                elif tok[0] == 'stamp':
                    s, bx, by, dx, dy, w, h = (int(t) for t in tok[1:8])
                    data = bytes.fromhex(tok[8]) if len(tok) > 8 else b''
                    if len(data) != w * h or w < 0 or h < 0:
                        raise nat.DflError('%s: stamp %d/%d/%d has %d bytes for %d x %d' % (path, s, bx, by, len(data), w, h))
                    self.index[(s, bx, by)] = (len(table), dx, dy)
                    table.append((w, h, nbytes))
                    masks.append(np.frombuffer(data, np.uint8))
                    nbytes += len(data)
                else:
                    raise nat.DflError('%s: unknown line %r' % (path, tok[0]))
        if set(self.rules) != {'x', 'y'} or sorted(self.strings.values()) != list(range(len(self.strings))):
            raise nat.DflError('%s: needs one rule per axis and strings numbered from 0' % path)
        nx, ny = len(self.rules['x']) + 1, len(self.rules['y']) + 1
        for s in self.strings.values():
            for bx in range(nx):
                for by in range(ny):
                    if (s, bx, by) not in self.index:
                        raise nat.DflError('%s: no stamp for string %d, bins (%d, %d)' % (path, s, bx, by))
        self.table = np.array(table, np.int32).reshape(-1, 3)
        self.masks = np.concatenate(masks) if masks else np.zeros(0, np.uint8)

    def bin(self, axis, f):
        return sum(1 for t in self.rules[axis] if f >= t)

    def mask(self, i):
        w, h, off = (int(v) for v in self.table[i])
        return self.masks[off:off + w * h].reshape(h, w)

    def place(self, text, x, y):
        """(left, top, stamp id) of draw.text((x, y), text) with Pillow's default font: x, y as the reference passes
        them (fp32 landmark coordinates, or 0)."""
        s = self.strings[text]
        fx, fy = math.modf(float(x))[0], math.modf(float(y))[0]
        i, dx, dy = self.index[(s, self.bin('x', fx), self.bin('y', fy))]
        return int(float(x)) + dx, int(float(y)) + dy, i


def text_stamps():
    global _text_host
    if _text_host is None:
        _text_host = TextStamps()
    return _text_host


def _text_on(dev):
    t = _text_dev.get(dev)
    if t is None:
        ts = text_stamps()
        masks = ts.masks if ts.masks.size else np.zeros(1, np.uint8)
        t = _text_dev[dev] = (torch.from_numpy(ts.table.copy()).to(dev), torch.from_numpy(masks.copy()).to(dev))
    return t


def pillow_coeffs(in_size, out_size):
    """Pillow's BILINEAR coefficients for one axis (libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc):
    bounds [out][2] (first input index, taps) int32, coefs [out][ksize] int32 in 22-bit fixed point."""
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), np.int32)
    coefs = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        w, ww = [], 0.0
        for x in range(xmax):
            t = (x + xmin - center + 0.5) * ss
            t = -t if t < 0.0 else t
            v = 1.0 - t if t < 1.0 else 0.0
            w.append(v)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            coefs[xx, x] = int(-0.5 + v * (1 << PIL_PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PIL_PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, coefs


def _span(bounds, tile):
    ends = bounds[:, 0] + bounds[:, 1]
    return max(int(ends[i:i + tile].max() - bounds[i:i + tile, 0].min()) for i in range(0, len(bounds), tile))


def resample_plan(in_hw, out_hw):
    """Host tables of Pillow's 8-bit BILINEAR resize from in_hw to out_hw (rows, cols), computed once per shape."""
    key = (tuple(int(v) for v in in_hw), tuple(int(v) for v in out_hw))
    p = _plans.get(key)
    if p is None:
        (h_in, w_in), (h_out, w_out) = key
        if min(h_in, w_in, h_out, w_out) < 1:
            raise nat.DflError('resize: sizes must be positive, got %s -> %s' % key)
        vb, vc = pillow_coeffs(h_in, h_out)
        hb, hc = pillow_coeffs(w_in, w_out)
        span_rows, span_cols = _span(vb, nat.RESAMPLE_TILE_ROWS), _span(hb, nat.RESAMPLE_TILE_COLS)
        if 4 * (4 * span_cols + nat.RESAMPLE_TILE_COLS * span_rows) > nat.RESAMPLE_MAX_LDS:
            raise nat.DflError('resize: %s -> %s reduces too strongly for one tile (%d x %d input pixels)'
                               % (key[0], key[1], span_rows, span_cols))
        p = _plans[key] = dict(h_bounds=hb, h_coefs=hc, v_bounds=vb, v_coefs=vc, h_in=h_in, w_in=w_in, h_out=h_out,
                               w_out=w_out, kh=hc.shape[1], kv=vc.shape[1], span_rows=span_rows, span_cols=span_cols)
    return p


def _plan_on(dev, in_hw, out_hw):
    """(ResamplePlan with device tables, tensors to keep alive)."""
    p = resample_plan(in_hw, out_hw)
    key = (dev, p['h_in'], p['w_in'], p['h_out'], p['w_out'])
    t = _plans_dev.get(key)
    if t is None:
        t = _plans_dev[key] = [torch.from_numpy(np.ascontiguousarray(p[k])).to(dev)
                               for k in ('h_bounds', 'h_coefs', 'v_bounds', 'v_coefs')]
    plan = nat.ResamplePlan(h_bounds=t[0].data_ptr(), h_coefs=t[1].data_ptr(), v_bounds=t[2].data_ptr(),
                            v_coefs=t[3].data_ptr(), **{k: p[k] for k in ('h_in', 'w_in', 'h_out', 'w_out', 'kh', 'kv',
                                                                         'span_rows', 'span_cols')})
    return plan, t


def resize_bilinear(rgb, size):
    """Pillow's Image.resize((w, h), Image.BILINEAR) of 8-bit RGB images on the GPU: rgb [B,H,W,3] or [H,W,3] uint8,
    size (h, w).  Returns the same layout at the new size."""
    if not torch.is_tensor(rgb) or not rgb.is_cuda:
        raise nat.DflError('overlay.resize_bilinear needs the images on the GPU (no CPU path)')
    if rgb.dtype != torch.uint8 or rgb.dim() not in (3, 4) or rgb.shape[-1] != 3:
        raise nat.DflError('overlay.resize_bilinear: expected uint8 [B,H,W,3] or [H,W,3], got %s %s'
                           % (rgb.dtype, tuple(rgb.shape)))
    x = rgb.detach().contiguous()
    single = x.dim() == 3
    if single:
        x = x.unsqueeze(0)
    B, H, W, _ = x.shape
    h, w = int(size[0]), int(size[1])
    plan, keep = _plan_on(x.device, (H, W), (h, w))
    out = torch.empty((B, h, w, 3), dtype=torch.uint8, device=x.device)
    a = nat.ResampleArgs(inp=x.data_ptr(), out=out.data_ptr(), plan=plan, B=B)
    nat.call('dfl_resample_bilinear_u8', a, torch.cuda.current_stream(x.device).cuda_stream)
    return out[0] if single else out


def fullres_size(H, W, factor=FULLRES_DS):
    """make_full_res_overlays.py's reduced size int(round(n * factor)) per dimension."""
    return int(round(H * factor)), int(round(W * factor))


def fullres_marks(lands, rot180, fov, H, W, radius=FULLRES_RADIUS):
    """The host half of one projection (make_full_res_overlays.py:104-137, 176-190): lands is a sequence of
    (name, (x, y)) in the file's order.  Keeps the landmarks with x >= 0, y >= 0, x < W and y < W (the reference
    compares the row with the column count), mirrors them in fp32 when rot180, and returns
    (ellipse boxes [n][5] int32 (x0, y0, w, h, first stamp row), texts [MAX_TEXTS][3] int32 (left, top, stamp or -1))."""
    index, spans, _ = stamp_table()
    D = nat.OVERLAY_STAMP_DIM
    r = np.float32(radius)
    vis, fh = [], {}
    for name, xy in lands:
        x, y = (np.float32(v) for v in np.asarray(xy, dtype=np.float32).reshape(-1)[:2])
        if x >= 0 and y >= 0 and x < W and y < W:
            if name in FULLRES_FH:
                fh[name] = len(vis)
            vis.append([x, y])
    if rot180:
        vis = [[np.float32(W - 1) - x, np.float32(H - 1) - y] for x, y in vis]
    boxes = []
    for x, y in vis:
        if not (math.isfinite(x) and math.isfinite(y)):
            continue
        x0, y0, x1, y1 = (int(v) for v in (x - r, y - r, x + r, y + r))      # fp32, truncated as Pillow does (render's rule: ovl_box, overlay.hip)
        if x1 < 0 or y1 < 0 or x0 >= W or y0 >= H:
            continue
        w, h = x1 - x0, y1 - y0
        if not (0 <= w < D and 0 <= h < D) or index[w * D + h] < 0:
            raise nat.DflError('overlay: radius %g needs ellipse box %r outside the stamp table' % (radius, (w, h)))
        boxes.append((x0, y0, w, h, int(index[w * D + h])))
    if len(boxes) > nat.FULLRES_MAX_BOXES:
        raise nat.DflError('overlay.render_full_res: %d visible landmarks, at most %d' % (len(boxes), nat.FULLRES_MAX_BOXES))
    texts = np.full((nat.FULLRES_MAX_TEXTS, 3), -1, np.int32)
    ts = text_stamps()
    for k, (text, name) in enumerate(zip(FULLRES_TEXTS, FULLRES_FH)):
        if fov[k]:
            x, y = vis[fh[name]] if name in fh else (0, 0)
            texts[k] = ts.place(text, x, y)
    return np.array(boxes, np.int32).reshape(-1, 5), texts


def render_full_res(images, segs, rot180, lands, fov, size=None, canvas=None, tile0=0, n_tiles=None,
                    radius=FULLRES_RADIUS):
    """make_full_res_overlays.py's overlay of a batch of projections, reduced, as tiles of one make_grid canvas.

    images [B,H,W] float on the GPU (fp32 kept, fp64 converted to fp32, anything else refused); segs [B,H,W] uint8 on
    the same GPU; rot180 [B] flags; lands: per image a sequence of (name, (x, y)) in the file's order; fov: per image
    (left femur good FOV, right femur good FOV).  size (h, w) defaults to int(round(n / 8)).  The images are tiles
    tile0 .. tile0 + B - 1 of a make_grid(nrow=8, padding=2) canvas of n_tiles (default B) images; pass the canvas of
    an earlier call to add to it.  Returns the canvas [rows, cols, 3] uint8 (the reduced image itself when n_tiles
    == 1)."""
    img = _images(images, 'render_full_res', dtypes=(torch.float32, torch.float64))
    dev = img.device
    B, H, W = img.shape
    seg = _on_dev(segs, 'render_full_res', 'segs', img, torch.uint8)
    if len(rot180) != B or len(lands) != B or len(fov) != B:
        raise nat.DflError('overlay.render_full_res: rot180, lands and fov need one entry per image')
    check_radius(float(radius))
    h, w = fullres_size(H, W) if size is None else (int(size[0]), int(size[1]))
    n_tiles = B if n_tiles is None else int(n_tiles)
    if not (0 <= tile0 and tile0 + B <= n_tiles):
        raise nat.DflError('overlay.render_full_res: tiles %d..%d outside a canvas of %d' % (tile0, tile0 + B - 1, n_tiles))
    shape = grid_shape(n_tiles, h, w) + (3,)
    if canvas is None:
        canvas = torch.zeros(shape, dtype=torch.uint8, device=dev)
    elif (not torch.is_tensor(canvas) or canvas.device != dev or canvas.dtype != torch.uint8
          or tuple(canvas.shape) != shape or not canvas.is_contiguous()):
        raise nat.DflError('overlay.render_full_res: canvas must be a contiguous uint8 %s tensor on %s' % (shape, dev))
    boxes = np.zeros((B, nat.FULLRES_MAX_BOXES, 5), np.int32)
    n_boxes = np.zeros(B, np.int32)
    texts = np.zeros((B, nat.FULLRES_MAX_TEXTS, 3), np.int32)
    for b in range(B):
        bx, texts[b] = fullres_marks(lands[b], bool(rot180[b]), fov[b], H, W, radius)
        boxes[b, :len(bx)] = bx
        n_boxes[b] = len(bx)
    host = np.concatenate([np.asarray([bool(r) for r in rot180], np.int32), n_boxes, boxes.ravel(), texts.ravel()])
    small = torch.from_numpy(host).to(dev)
    rot_d, nb_d = small[:B], small[B:2 * B]
    boxes_d = small[2 * B:2 * B + boxes.size]
    texts_d = small[2 * B + boxes.size:]
    _, spans = _stamps_on(dev)
    tstamps, tmasks = _text_on(dev)
    plan, keep = _plan_on(dev, (H, W), (h, w))
    scratch = _scratch(img)
    a = nat.FullresArgs(image=img.data_ptr(), labels=seg.data_ptr(), rot180=rot_d.data_ptr(), boxes=boxes_d.data_ptr(),
                        n_boxes=nb_d.data_ptr(), texts=texts_d.data_ptr(), stamp_spans=spans.data_ptr(),
                        text_stamps=tstamps.data_ptr(), text_masks=tmasks.data_ptr(), scratch=scratch.data_ptr(),
                        out=canvas.data_ptr(), plan=plan, B=B, H=H, W=W, n_tint=len(FULLRES_COLORS),
                        tint_scale=1 - ALPHA, n_text_stamps=len(text_stamps().table), n_stamp_spans=int(spans.numel()),
                        tile0=int(tile0), n_tiles=n_tiles)
    _fill_tint(a, FULLRES_COLORS)
    nat.call('dfl_fullres_overlay', a, torch.cuda.current_stream(dev).cuda_stream)
    return canvas
