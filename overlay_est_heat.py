#!/usr/bin/env python3
"""Overlay one landmark's estimated heat map onto a projection: the command line of the reference's
train_test_code/overlay_est_heat.py (:24-36 arguments and defaults), with the pixel work done on the GPU by
dfl_overlay_batch (dfl_amd.overlay.render) and the PNG written by dfl_amd.png.

    python overlay_est_heat.py data.h5 out.h5 nn-heats 1 3 1 proj_3_fhr.png

The projection is get_dataset(ds_path, [pat], num_classes)[proj][0]; the heat map is seg_group[proj, land_ind], min/max
normalised when its range exceeds 1e-3, and blended in green.  Files: the reference's HDF5 (dfl_amd.h5lite) or .npz.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfl_amd  # noqa: E402,F401
from dfl_amd import dataset, overlay, png  # noqa: E402
from overlay_est_ann import require_gpu  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description='overlay estimated heat maps for a specific projection and landmark',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('ds_path', help='Path to dataset containing projections', type=str)
    p.add_argument('seg_file', help='Path to H5 file with estimated segmentations and heatmaps', type=str)
    p.add_argument('seg_group', help='Path within H5 file of estimated heatmaps', type=str)
    p.add_argument('pat_ind', help='patient index', type=int)
    p.add_argument('proj_ind', help='proj', type=int)
    p.add_argument('land_ind', help='landmark index', type=int)
    p.add_argument('out_overlay', help='Path to output overlay image', type=str)
    p.add_argument('--num-classes', help='number of classes in segmentation', type=int, default=7)
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    dev = require_gpu()
    ds = dataset.get_dataset(args.ds_path, [args.pat_ind], num_classes=args.num_classes, device=dev)
    img = ds[args.proj_ind][0]
    get, close = dataset._open_container(args.seg_file)
    heat = np.asarray(get(args.seg_group))[args.proj_ind, args.land_ind]
    close()
    heat = torch.from_numpy(np.ascontiguousarray(heat, dtype=np.float32)).unsqueeze(0).to(dev)
    rgb = overlay.render(img, heats=heat)
    png.write(args.out_overlay, rgb[0].cpu().numpy())


if __name__ == '__main__':
    main()
