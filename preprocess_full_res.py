#!/usr/bin/env python3
"""Training file from the full-resolution dataset file: crop the borders, log-transform, rotate by 180 degrees where
'rot-180-for-up' is set, reduce -- the steps the reference's README names for its preprocessed files (the program that
made those is not part of the reference; DESIGN.md section 14 pins the arithmetic used here).  The pixel work runs on
the GPU (dfl_amd.preprocess: dfl_preproc_projs, dfl_preproc_segs), --chunk projections at a time.

    python preprocess_full_res.py full_res.h5 out.h5 --ds-factor 8 [--crop 50] [--specimens a,b] [--no-log]
                                  [--min-intensity 1] [--chunk 32] [--gzip]

Reads '<id>/projections/NNN/{image/pixels, gt-seg/pixels, gt-landmarks/<name>, rot-180-for-up}' and 'proj-params';
writes 'NN/projs', 'NN/segs', 'NN/lands' and 'land-names' as train.py, test_ensemble.py and the other entry points read
them.  Specimens are numbered in the README's order (17-1882, 18-1109, 18-0725, 18-2799, 18-2800, 17-1905 -> 01..06)
when exactly those are present, else sorted; --specimens gives the order itself.  One line per specimen is printed.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def build_parser():
    p = argparse.ArgumentParser(description='preprocess the full-resolution dataset file into a training file',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('src', type=str, help='path to the full-resolution HDF5 file')
    p.add_argument('dst', type=str, help='path of the preprocessed HDF5 file to write')
    p.add_argument('--ds-factor', type=int, default=8, help='downsampling factor in each dimension (1..16)')
    p.add_argument('--crop', type=int, default=50, help='pixels removed from each border')
    p.add_argument('--specimens', type=lambda s: [t for t in s.split(',') if t], default=None,
                   help='comma-separated specimen ids, numbered 01, 02, ... in this order')
    p.add_argument('--no-log', action='store_true', help='keep intensities (box means) instead of line integrals')
    p.add_argument('--min-intensity', type=float, default=1.0, help='intensities are clamped to this before the log')
    p.add_argument('--chunk', type=int, default=32, help='projections moved to the device per call')
    p.add_argument('--gzip', action='store_true', help='compress projs and segs (gzip)')
    return p


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    import dfl_amd
    dfl_amd.convert_file(args.src, args.dst, factor=args.ds_factor, crop=args.crop, specimens=args.specimens,
                         chunk=args.chunk, compression='gzip' if args.gzip else None, log=not args.no_log,
                         min_intensity=args.min_intensity, report=print)
    return 0


if __name__ == '__main__':
    sys.exit(main())
