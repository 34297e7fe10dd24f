#!/usr/bin/env python3
"""Ground-truth segmentations and landmarks over every projection of a preprocessed file, one tiled PNG per specimen:
the reference's examples_dataset/make_preproc_overlays.py, with each specimen's projections rendered in ONE
dfl_overlay_batch call (dfl_amd.overlay.render(grid=True): make_grid(nrow=8, padding=2) canvas).

    python examples/make_preproc_overlays.py ipcai_2020_full_res_data.h5      # writes <group>.png into the working directory

Raw 'projs' / 'segs' / 'lands' (no standardisation), labels 1-6 tinted, landmarks as filled yellow circles of radius
max(16 rows / 1536, 3) (fixed by the first specimen), drawn when x >= 0, y >= 0, x < cols and y < cols (the reference
compares y with cols too).  Files: the reference's HDF5 (dfl_amd.h5lite) or .npz with the same names.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, overlay, png  # noqa: E402

PREPROC_COLORS = overlay.ANN_COLORS[:6]


def groups(path):
    """(name, get) per top-level group of the file, in the file's order (h5py iterates names sorted)."""
    if str(path).endswith('.npz'):
        z = np.load(path)
        names = sorted({k.split('/')[0] for k in z.files if '/' in k})
        return [(g, (lambda k, g=g: z[g + '/' + k] if (g + '/' + k) in z.files else None)) for g in names], (lambda: None)
    from dfl_amd import h5lite
    f = h5lite.File(path, 'r')
    out = []
    for g in sorted(f.keys()):
        node = f[g]
        if not isinstance(node, h5lite.Group):
            continue
        out.append((g, (lambda k, node=node: node[k][()] if k in node else None)))
    return out, f.close


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) < 1:
        print('ERROR: supply path to HDF5 data file as first argument')
        return 1
    if not torch.cuda.is_available():
        raise nat.DflError('no GPU visible: the overlays are drawn by HIP kernels (no CPU path)')
    dev = dfl_amd.get_device()
    box_radius = None
    specs, close = groups(argv[0])
    for name, get in specs:
        projs = get('projs')
        if projs is None:               # e.g. 'land-names'
            continue
        projs = np.asarray(projs, dtype=np.float32)
        segs, lands = np.asarray(get('segs')), np.asarray(get('lands'))
        num_projs, rows, cols = projs.shape
        assert segs.shape == projs.shape
        assert lands.shape[0] == num_projs and lands.shape[1] == 2
        if box_radius is None:
            box_radius = max(16 * (rows / 1536.0), 3.0)
        if lands.dtype != np.float64:
            lands = lands.astype(np.float32)
        gt = np.ascontiguousarray(lands.transpose(0, 2, 1))           # [N, L, 2] (x, y)
        x, y = gt[..., 0], gt[..., 1]
        gt[~((x >= 0) & (y >= 0) & (x < cols) & (y < cols))] = np.nan
        rgb = overlay.render(torch.from_numpy(projs).to(dev), segs=torch.from_numpy(segs).to(dev), num_classes=7,
                             gt_lands=torch.from_numpy(gt).to(dev), radius=box_radius, colors=PREPROC_COLORS, grid=True)
        png.write('{}.png'.format(name), rgb.cpu().numpy())
    close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
