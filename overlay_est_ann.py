#!/usr/bin/env python3
"""Overlay estimated annotations (segmentation tint and landmark markers) onto a projection: the command line of the
reference's train_test_code/overlay_est_ann.py (:26-47 arguments and defaults), with the pixel work done on the GPU by
dfl_overlay_batch (dfl_amd.overlay.render) and the PNG written by dfl_amd.png.

    python overlay_est_ann.py data.h5 out.h5 nn-segs 1 3 proj_3.png --lands --no-gt-lands --lands-csv lands.csv

The projection is get_dataset(ds_path, [pat], num_classes)[proj][0] and the ground-truth landmarks its item [2], as in
the reference.  Estimated landmarks come from the CSV rows of this patient and projection with row, col >= 0 (a
landmark index listed twice is an error).  Files: the reference's HDF5 (dfl_amd.h5lite) or .npz with the same names.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, dataset, overlay, png  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description='overlay segs', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('ds_path', help='Path to dataset containing projections', type=str)
    p.add_argument('seg_file', help='Path to H5 file with estimated segmentations and heatmaps', type=str)
    p.add_argument('seg_group', help='Path within H5 file of estimated segmentations', type=str)
    p.add_argument('pat_ind', help='patient index', type=int)
    p.add_argument('proj_ind', help='proj', type=int)
    p.add_argument('out_overlay', help='Path to output overlay image', type=str)
    p.add_argument('--lands', help='overlay GT and est. landmark locations', action='store_true')
    p.add_argument('--no-gt-lands', help='do not overlay GT landmarks', action='store_true')
    p.add_argument('--no-seg', help='do not overlay est. seg.', action='store_true')
    p.add_argument('--lands-csv', help='path to CSV file of estimated landmark locations', type=str)
    p.add_argument('--num-classes', help='number of classes in segmentation', type=int, default=7)
    return p


def est_lands_from_csv(path, pat_ind, proj):
    """{landmark index: (col, row)} of the CSV rows (pat,proj,land,row,col,...; header skipped) of this patient and
    projection whose row and col are >= 0 (overlay_est_ann.py:75-90)."""
    est = {}
    with open(path, 'r') as f:
        lines = f.readlines()[1:]
    for line in lines:
        toks = line.strip().split(',')
        if int(toks[0]) == pat_ind and int(toks[1]) == proj:
            row, col = int(toks[3]), int(toks[4])
            if row >= 0 and col >= 0:
                idx = int(toks[2])
                if idx in est:
                    raise ValueError('%s: landmark %d of patient %d, projection %d is listed twice' % (path, idx, pat_ind, proj))
                est[idx] = (col, row)
    return est


def require_gpu():
    if not torch.cuda.is_available():
        raise nat.DflError('no GPU visible: the overlays are drawn by HIP kernels (no CPU path)')
    return dfl_amd.get_device()


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.lands and not args.lands_csv:
        parser.error('--lands needs --lands-csv')
    dev = require_gpu()
    est = est_lands_from_csv(args.lands_csv, args.pat_ind, args.proj_ind) if args.lands else {}
    ds = dataset.get_dataset(args.ds_path, [args.pat_ind], num_classes=args.num_classes, device=dev)
    item = ds[args.proj_ind]
    segs = gt = est_t = None
    if not args.no_seg:
        get, close = dataset._open_container(args.seg_file)
        segs = torch.from_numpy(np.ascontiguousarray(np.asarray(get(args.seg_group))[args.proj_ind])).unsqueeze(0).to(dev)
        close()
    if args.lands:
        gt = torch.empty((1, 0, 2), dtype=torch.float32, device=dev)
        if not args.no_gt_lands:
            gt = item[2].t().unsqueeze(0).contiguous()          # [2, L] (row 0 = x) -> [1, L, 2]
        est_t = torch.tensor([list(v) for v in est.values()], dtype=torch.int32).view(1, -1, 2).to(dev)
    rgb = overlay.render(item[0], segs=segs, num_classes=args.num_classes, gt_lands=gt, est_lands=est_t)
    png.write(args.out_overlay, rgb[0].cpu().numpy())


if __name__ == '__main__':
    main()
