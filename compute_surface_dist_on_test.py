#!/usr/bin/env python3
"""Boundary distances per projection and foreground label as CSV, the sibling of compute_actual_dice_on_test.py (same
positional arguments and files): Hausdorff distance, its percentile and the average symmetric surface distance between the
estimated and the ground-truth outline of every bone, rows ``pat,proj,label,hd,hd95,assd`` with two decimals.  Computed on
the GPU by dfl_amd.labels.surface_distances (exact distance transforms, no round trip through scipy.ndimage).  (The
reference scores overlap only.)

    python compute_surface_dist_on_test.py data.h5 out.h5 nn-segs dist.csv 4 [--no-hdr] [--num-classes 7] [--pixel-mm 1.0]
                                           [--percentile 95]

A label that neither map has scores 0.00, a label that only one of them has ``inf``.  --pixel-mm scales pixels to
millimetres; the name of the fifth column follows --percentile (hd95, hd90, hd99.5).
Files: the reference's HDF5 (dependency-free reader dfl_amd.h5lite) or .npz with the same dataset names.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, dataset, labels  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description='compute boundary distances (Hausdorff, percentile Hausdorff, average symmetric '
                                            'surface distance) between estimated segmentations and ground truth. Scores '
                                            'are written out in CSV format.',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('ds_path', type=str, help='Path to dataset containing projections')
    p.add_argument('seg_file', type=str, help='Path to H5 file with estimated segmentations')
    p.add_argument('seg_group', type=str, help='Path within H5 file of estimated segmentations')
    p.add_argument('csv_out', type=str, help='Path to output CSV file')
    p.add_argument('pat_ind', type=int, help='patient index')
    p.add_argument('--no-hdr', action='store_true', help='No CSV header')
    p.add_argument('--num-classes', type=int, default=7, help='number of classes in segmentation')
    p.add_argument('--pixel-mm', type=float, default=1.0, help='pixel spacing: distances are multiplied by it')
    p.add_argument('--percentile', type=float, default=95.0, help='percentile of the union of both directed distances')
    return p


def header(percentile):
    return 'pat,proj,label,hd,hd{:g},assd'.format(percentile)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise nat.DflError('compute_surface_dist_on_test: no GPU visible: this build has no CPU path (the distance '
                           'transform and the statistics are HIP kernels for MI355X)')
    dev = dfl_amd.get_device()
    get, close = dataset._open_container(args.ds_path)
    gt_segs = torch.from_numpy(np.asarray(get('{:02d}/segs'.format(args.pat_ind))))
    close()
    get, close = dataset._open_container(args.seg_file)
    est_segs = torch.from_numpy(np.asarray(get(args.seg_group)))
    close()
    num_projs = gt_segs.shape[0]
    assert num_projs == est_segs.shape[0]
    res = labels.surface_distances(est_segs.to(dev), gt_segs.to(dev), num_classes=args.num_classes, spacing=args.pixel_mm,
                                   percentile=args.percentile)
    with open(args.csv_out, 'w') as csv_out:
        if not args.no_hdr:
            csv_out.write(header(args.percentile) + '\n')
        for proj in range(num_projs):
            for l in range(1, args.num_classes):            # background excluded
                csv_out.write('{},{},{},{:.2f},{:.2f},{:.2f}\n'.format(
                    args.pat_ind, proj, l, float(res['hd'][proj, l - 1]), float(res['hdp'][proj, l - 1]),
                    float(res['assd'][proj, l - 1])))


if __name__ == '__main__':
    main()
