#!/usr/bin/env python3
"""Synthetic training data from the full-resolution dataset file: poses sampled around the acquired ones, projections
rendered from the CT, its 3D annotation and its 3D landmarks (dfl_amd.drr), turned into detector images (transmission,
blur, quantum and electronic noise, gain: dfl_drr_expose) and written as a full-resolution file or directly as a
training file.  'gt-seg', 'gt-landmarks' and 'gt-poses' are exact by construction.

    python synthesize_dataset.py full_res.h5 synth.h5 --views 200 [--seed 0] [--layout full-res|preprocessed]
           [--specimens a,b] [--crop 50] [--ds-factor 8] [--rot-sigma-deg 10] [--trans-sigma-mm 20,20,50]
           [--femur-sigma-deg 5] [--min-lands 4] [--photons 20000] [--gain 2] [--electronic-sigma 3] [--blur-sigma-px 1]
           [--no-noise] [--bones-only] [--no-volumes] [--chunk 8] [--gzip]
           [--tools 0] [--tool-mu 0.5] [--tool-anchor-sigma-mm 30] [--tool-length-mm 60,220] [--tool-radius-mm 0.5,1.6]
           [--bead-prob 0.25] [--tool-mask]

--views is per specimen.  Specimens are numbered as preprocess_full_res.py numbers them.  One line per specimen is
printed.  --tools N puts up to N straight metal tools (wires as capsules, beads as spheres) into every
view; --tool-mask (full-res layout) also writes where they are.  The renderer and the detector model are HIP kernels: a machine without a GPU is refused.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _triple(s):
    v = [float(t) for t in s.split(',')]
    if len(v) != 3:
        raise argparse.ArgumentTypeError('three comma-separated numbers expected, got %r' % s)
    return tuple(v)


def _pair(s):
    v = [float(t) for t in s.split(',')]
    if len(v) != 2 or not 0 < v[0] <= v[1]:
        raise argparse.ArgumentTypeError('two comma-separated numbers lo,hi with 0 < lo <= hi expected, got %r' % s)
    return tuple(v)


def _count(s):
    v = int(s)
    if not 0 <= v <= 64:
        raise argparse.ArgumentTypeError('0..64 expected, got %r' % s)
    return v


def _prob(s):
    v = float(s)
    if not 0 <= v <= 1:
        raise argparse.ArgumentTypeError('a probability 0..1 expected, got %r' % s)
    return v


def _not_negative(s):
    v = float(s)
    if not 0 <= v < float('inf'):
        raise argparse.ArgumentTypeError('a finite number that is not negative expected, got %r' % s)
    return v


def build_parser():
    p = argparse.ArgumentParser(description='synthesise projections, labels and landmarks from the full-resolution dataset file',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('src', type=str, help='path to the full-resolution HDF5 file')
    p.add_argument('dst', type=str, help='path of the HDF5 file to write')
    p.add_argument('--views', type=int, default=200, help='synthetic projections per specimen')
    p.add_argument('--seed', type=int, default=0, help='seed of the poses and of the image noise')
    p.add_argument('--layout', choices=['full-res', 'preprocessed'], default='preprocessed', help='layout of the file written')
    p.add_argument('--specimens', type=lambda s: [t for t in s.split(',') if t], default=None,
                   help='comma-separated specimen ids, numbered 01, 02, ... in this order')
    p.add_argument('--crop', type=int, default=50, help='pixels removed from each border (also bounds the accepted poses)')
    p.add_argument('--ds-factor', type=int, default=8, help='downsampling factor of the preprocessed layout (1..16)')
    p.add_argument('--rot-sigma-deg', type=float, default=10.0, help='sigma of the common rotation, per axis')
    p.add_argument('--trans-sigma-mm', type=_triple, default=(20.0, 20.0, 50.0), help='sigma of the common translation x,y,z in the camera frame')
    p.add_argument('--femur-sigma-deg', type=float, default=5.0, help='sigma of each femur\'s rotation about its head, per axis')
    p.add_argument('--min-lands', type=int, default=4, help='landmarks that must project inside the crop window')
    p.add_argument('--photons', type=float, default=20000.0, help='photons per pixel of an unattenuated ray')
    p.add_argument('--gain', type=float, default=2.0, help='detector counts per photon')
    p.add_argument('--electronic-sigma', type=float, default=3.0, help='sigma of the additive noise, in photons')
    p.add_argument('--blur-sigma-px', type=float, default=1.0, help='sigma of the detector blur in pixels (at most 8/3)')
    p.add_argument('--no-noise', action='store_true', help='no quantum and no electronic noise')
    p.add_argument('--bones-only', action='store_true', help='leave the soft tissue out of the rendering')
    p.add_argument('--no-volumes', action='store_true', help="full-res layout: leave out 'vol' and 'vol-seg'")
    p.add_argument('--chunk', type=int, default=8, help='views rendered per launch')
    p.add_argument('--gzip', action='store_true', help='compress the pixel datasets (gzip)')
    p.add_argument('--tools', type=_count, default=0, help='at most this many tools per view (0: none, and the file of a run without the flag)')
    p.add_argument('--tool-mu', type=_not_negative, default=0.5, help='attenuation of every tool per mm (a parameter, not an alloy)')
    p.add_argument('--tool-anchor-sigma-mm', type=_not_negative, default=30.0, help='sigma of a tool\'s anchor about a landmark, per axis')
    p.add_argument('--tool-length-mm', type=_pair, default=(60.0, 220.0), help='length of a wire lo,hi')
    p.add_argument('--tool-radius-mm', type=_pair, default=(0.5, 1.6), help='radius of a wire lo,hi')
    p.add_argument('--bead-prob', type=_prob, default=0.25, help='probability that a tool is a bead of 0.75 mm radius')
    p.add_argument('--tool-mask', action='store_true', help="full-res layout: write 'tools/mask' (1 where a ray crosses a tool)")
    return p


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    import dfl_amd
    dfl_amd.synthesize(args.src, args.dst, args.views, seed=args.seed, layout=args.layout, specimens=args.specimens, crop=args.crop,
                       factor=args.ds_factor, rot_sigma_deg=args.rot_sigma_deg, trans_sigma_mm=args.trans_sigma_mm,
                       femur_sigma_deg=args.femur_sigma_deg, min_lands=args.min_lands, photons=args.photons, gain=args.gain,
                       electronic_sigma=args.electronic_sigma, blur_sigma_px=args.blur_sigma_px, noise=not args.no_noise,
                       bones_only=args.bones_only, volumes=not args.no_volumes, chunk=args.chunk,
                       compression='gzip' if args.gzip else None, report=print, tools=args.tools,
                       tool_options=dict(tool_mu=args.tool_mu, anchor_sigma_mm=args.tool_anchor_sigma_mm, length_mm=args.tool_length_mm,
                                         wire_radius_mm=args.tool_radius_mm, bead_prob=args.bead_prob), tool_mask=args.tool_mask)
    return 0


if __name__ == '__main__':
    sys.exit(main())
