#!/usr/bin/env python3
"""Clean the predicted label maps of a results file on the GPU: per bone keep the largest connected component, drop
specks, optionally close pin-holes (dfl_amd.labels.clean: dfl_label_components, dfl_label_select), and store the result as a
new dataset next to the old one -- a drop-in ``seg_group`` for compute_actual_dice_on_test.py, est_lands_csv.py --use-seg
and overlay_est_ann.py.  (The reference has no such step: its tools take 'nn-segs' as the arg-max left it.)

    python clean_segs.py out.h5 nn-segs nn-segs-clean [--out-file other.h5] [--num-classes 7] [--connectivity 8]
                         [--keep largest|all] [--min-area 0] [--fill-holes 0]

Files: HDF5 (dependency-free reader and writer dfl_amd.h5lite) or .npz.  The whole [N, H, W] stack is cleaned in one call.
h5lite writes a file in one pass and cannot add a dataset to an existing one: the output file is WRITTEN ANEW with every
other dataset of the input copied through unchanged (values, shape, dtype, chunking and gzip level), to a temporary name
that replaces the file only once it is complete.  The new dataset has the chunking test_ensemble.py gives 'nn-segs' (one
image per chunk, gzip 9).  Prints one line per label: components removed, pixels removed, pixels filled.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, dataset, h5lite, labels  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description='clean estimated segmentations: per label keep the largest connected component, '
                                            'drop small ones, optionally fill small holes. The result is written as a new '
                                            'dataset.',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('seg_file', type=str, help='Path to H5 (or .npz) file with estimated segmentations')
    p.add_argument('seg_group', type=str, help='Path within the file of the estimated segmentations')
    p.add_argument('out_group', type=str, help='Path within the output file of the cleaned segmentations')
    p.add_argument('--out-file', type=str, default=None, help='Write to this file instead of into seg_file')
    p.add_argument('--num-classes', type=int, default=7, help='number of classes in segmentation')
    p.add_argument('--connectivity', type=int, default=8, choices=(4, 8), help='pixel connectivity of a label')
    p.add_argument('--keep', type=str, default='largest', choices=('largest', 'all'),
                   help='components of a label to keep in each image')
    p.add_argument('--min-area', type=int, default=0, help='remove components of fewer pixels than this')
    p.add_argument('--fill-holes', type=int, default=0,
                   help='fill background holes of at most this many pixels that one label encloses (0: none)')
    return p


def _copy_h5(src, dst, skip):
    """Every dataset of the open h5lite group `src` except path `skip` into the writer group `dst`."""
    for name in src.keys():
        node = src[name]
        path = node.name.strip('/')
        if isinstance(node, h5lite.Group):
            _copy_h5(node, dst.create_group(name), skip)
        elif path == skip:
            continue
        elif not isinstance(node._type, np.dtype):
            if node._type[0] != 'vlen_str' or node.shape != ():
                raise nat.DflError('clean_segs: cannot copy %s (a fixed-length or array string dataset)' % node.name)
            dst[name] = bytes(node[()])
        elif node._layout[0] == 'chunked':
            level = [cd[0] for fid, cd in node._filters if fid == 1]
            dst.create_dataset(name, data=node[...], dtype=node.dtype, chunks=node._layout[2],
                               compression='gzip' if level else None, compression_opts=level[0] if level else None)
        else:
            dst.create_dataset(name, data=node[()], dtype=node.dtype)


def _write(args, cleaned):
    out_path = args.out_file or args.seg_file
    out_group = args.out_group.strip('/')
    if str(out_path).endswith('.npz'):
        old = dict(np.load(out_path)) if os.path.exists(out_path) else {}
        old[args.out_group] = cleaned
        tmp = out_path + '.tmp.npz'
        np.savez(tmp, **old)
        os.replace(tmp, out_path)
        return
    tmp = out_path + '.tmp'
    with h5lite.File(tmp, 'w') as dst:
        if os.path.exists(out_path):
            with h5lite.File(out_path, 'r') as src:
                _copy_h5(src, dst, out_group)
        dst.create_dataset(out_group, data=cleaned, dtype='u1', chunks=(1,) + cleaned.shape[1:], compression='gzip',
                           compression_opts=9)
    os.replace(tmp, out_path)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise nat.DflError('clean_segs: no GPU visible: this build has no CPU path (the clean-up is HIP kernels for MI355X)')
    dev = dfl_amd.get_device()
    get, close = dataset._open_container(args.seg_file)
    est = np.asarray(get(args.seg_group))
    close()
    if est.ndim != 3 or est.dtype != np.uint8:
        raise nat.DflError('clean_segs: %s has shape %s and dtype %s: [N, H, W] of uint8 expected'
                           % (args.seg_group, est.shape, est.dtype))
    segs = torch.from_numpy(est).to(dev)
    cleaned, stats = labels.clean(segs, num_classes=args.num_classes, connectivity=args.connectivity, keep=args.keep,
                                  min_area=args.min_area, fill_holes=args.fill_holes)
    # components removed: the root pixel of a component belongs to it, so it went to background with the component
    _, area, _ = labels.components(segs, args.connectivity)
    gone = (area > 0) & (segs != 0) & (segs < args.num_classes)
    if args.fill_holes > 0:          # (a removed component may have been filled again: judge by stage 1 alone)
        stage1, _ = labels.clean(segs, num_classes=args.num_classes, connectivity=args.connectivity, keep=args.keep,
                                 min_area=args.min_area)
        gone &= stage1 == 0
    else:
        gone &= cleaned == 0
    comps = torch.bincount(segs[gone].long(), minlength=args.num_classes).cpu()
    _write(args, cleaned.cpu().numpy())
    removed, filled = stats['removed'].sum(0), stats['filled'].sum(0)
    for l in range(1, args.num_classes):
        print('label {}: {} components removed, {} pixels removed, {} pixels filled'.format(
            l, int(comps[l]), int(removed[l]), int(filled[l])))


if __name__ == '__main__':
    main()
