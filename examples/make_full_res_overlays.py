#!/usr/bin/env python3
"""Ground-truth segmentations, landmarks and femur-FOV notes over every projection of the full-resolution file, one
tiled PNG per specimen: the reference's examples_dataset/make_full_res_overlays.py, drawn and reduced 8x on the GPU by
dfl_fullres_overlay (dfl_amd.overlay.render_full_res), chunks of at most CHUNK projections per call, all into one
make_grid(nrow=8, padding=2) canvas.

    python examples/make_full_res_overlays.py ipcai_2020_full_res_data.h5     # writes <specimen>.png into the working directory

Per projection NNN of '<specimen>/projections': 'image/pixels' (fp32; fp64 is accepted and rounded to fp32),
'gt-seg/pixels', 'gt-landmarks/<name>' ((2,) or (2, 1): column, row), the rotation flag and the two femur good-fov
flags; the detector size comes from 'proj-params' (hdf5_layouts/Readme.md; the names live in dfl_amd.fullres).
A landmark is drawn when x >= 0, y >= 0, x < cols and y < cols (the reference compares the row with the column count).
Files: the reference's HDF5 (dfl_amd.h5lite) or .npz with the same names as keys.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, fullres, overlay, png  # noqa: E402
from dfl_amd.fullres import Source  # noqa: E402,F401

CHUNK = 16          # projections uploaded per call: host and device memory stay bounded


def read_projection(src, pfx):
    """(image, labels, [(name, (x, y))], rot180, (left fov, right fov)) of one projection group."""
    img = np.asarray(src.get(pfx + 'image/pixels'))
    if img.dtype not in (np.float32, np.float64):
        raise nat.DflError('%simage/pixels has dtype %s: float32 or float64 expected' % (pfx, img.dtype))
    seg = np.asarray(src.get(pfx + 'gt-seg/pixels'))
    lands = [(n, v.astype(np.float32)) for n, v in fullres.gt_landmarks(src, pfx).items()]
    fov = tuple(bool(v) for v in fullres.femur_fov(src, pfx))
    return img.astype(np.float32, copy=False), seg, lands, fullres.rot180(src, pfx), fov


def render_specimen(src, spec, rows, cols, dev, chunk=CHUNK):
    """The tiled canvas of one specimen, [rows, cols, 3] uint8 on dev."""
    num = fullres.n_projections(src, spec)
    size = overlay.fullres_size(rows, cols)
    canvas = None
    for c0 in range(0, num, chunk):
        items = [read_projection(src, fullres.projection_prefix(spec, p)) for p in range(c0, min(c0 + chunk, num))]
        for img, seg, _, _, _ in items:
            if img.shape != (rows, cols) or seg.shape != (rows, cols):
                raise nat.DflError('%s: projection of shape %s / %s, proj-params say %s' % (spec, img.shape, seg.shape, (rows, cols)))
        imgs = torch.from_numpy(np.stack([it[0] for it in items])).to(dev)
        segs = torch.from_numpy(np.stack([it[1] for it in items]).astype(np.uint8, copy=False)).to(dev)
        canvas = overlay.render_full_res(imgs, segs, [it[3] for it in items], [it[2] for it in items],
                                         [it[4] for it in items], size=size, canvas=canvas, tile0=c0, n_tiles=num)
    return canvas


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) < 1:
        print('ERROR: supply path to HDF5 data file as first argument')
        return 1
    if not torch.cuda.is_available():
        raise nat.DflError('no GPU visible: the overlays are drawn by HIP kernels (no CPU path)')
    dev = dfl_amd.get_device()
    src = Source(argv[0])
    rows, cols = fullres.detector_size(src)
    for spec in src.children():
        if spec == 'proj-params':
            continue
        canvas = render_specimen(src, spec, rows, cols, dev)
        if canvas is not None:
            png.write('{}.png'.format(spec), canvas.cpu().numpy())
    src.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
