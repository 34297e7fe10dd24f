#!/usr/bin/env python3
"""A digitally reconstructed radiograph, a 2D label map and the projected landmarks of one projection of the
full-resolution file, rendered on the GPU (dfl_amd.drr -> dfl_drr_render) from the CT ('<specimen>/vol'), the 3D
annotation ('<specimen>/vol-seg/image'), the ground-truth poses and '<specimen>/vol-landmarks', on the pixel grid
preprocess_full_res.py writes for the same --crop and --ds-factor.

    python examples/full_res_drr.py full_res.h5 17-1882 0                      # writes 17-1882_000_drr.png, _labels.png, .npz
    python examples/full_res_drr.py full_res.h5 17-1882 0 --out view --ds-factor 4 --interp trilinear --step 0.25 --compare
    python examples/full_res_drr.py synth.h5 17-1882 3 --tools-from synth.h5   # one tooled view of synthesize_dataset.py --tools

PREFIX_drr.png is the line integral, 8-bit, min / max scaled (a constant image comes out as 0); PREFIX_labels.png the
label map tinted over it in the overlay palette; PREFIX.npz holds att, labels and lands ([2, L] (column, row) in
preprocess.LAND_ORDER; inf where the file has no such 3D landmark).  --bones-only leaves the soft tissue out.  The
label map always comes from the exact radiological path; --interp chooses how att is integrated.
--compare renders the file's own projection, gt-seg and gt-landmarks on the same grid and prints the NCC of the DRR
with the projection, the hard Dice per label and the largest landmark distance in output pixels.
--tools-from FILE reads 'projections/NNN/tools/capsules' of the same specimen and projection from FILE (a full-res file
of synthesize_dataset.py --tools N) and adds those capsules to att (dfl_amd.tools.add_tools); the
label map is the anatomy's, whatever lies in front of it.  A projection without that dataset has no tools.
Files: the reference's HDF5 (dfl_amd.h5lite) or .npz with the same names as keys.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, drr, fullres, ncc, overlay, png, preprocess, tools, util  # noqa: E402

USAGE = ('Usage: {} <HDF5 full-res data file> <specimen ID> <projection index> [--out PREFIX] [--crop 50] [--ds-factor 8] '
         '[--interp exact|trilinear] [--step 0.5] [--bones-only] [--compare] [--tools-from FILE]')
VALUED = {'--out': str, '--crop': int, '--ds-factor': int, '--interp': str, '--step': float}
FLAGS = ('--bones-only', '--compare')


def parse_options(argv, valued, flags, opts):
    """(three positional arguments, options over the defaults `opts`) or None when the command line is not understood."""
    opts = dict(opts, **{a: False for a in flags})
    pos, k = [], 0
    while k < len(argv):
        a = argv[k]
        if a in valued:
            if k + 1 >= len(argv):
                return None
            try:
                opts[a] = valued[a](argv[k + 1])
            except ValueError:
                return None
            k += 2
        elif a in flags:
            opts[a] = True
            k += 1
        elif a.startswith('--'):
            return None
        else:
            pos.append(a)
            k += 1
    return (pos, opts) if len(pos) == 3 else None


def parse(argv):
    """(positional, options) or None when the command line is not understood."""
    parsed = parse_options(argv, VALUED, FLAGS, {'--out': None, '--crop': 50, '--ds-factor': 8, '--interp': 'exact', '--step': 0.5})
    return parsed if parsed and parsed[1]['--interp'] in ('exact', 'trilinear') else None


def parse_tools(argv):
    """(argv without '--tools-from FILE', FILE or None), or None when the option has no value."""
    argv = list(argv)
    if '--tools-from' not in argv:
        return argv, None
    k = argv.index('--tools-from')
    if k + 1 >= len(argv) or argv[k + 1].startswith('--') or '--tools-from' in argv[k + 2:]:
        return None
    return argv[:k] + argv[k + 2:], argv[k + 1]


def to_u8(img):
    """Min / max scaling to 8 bits; a constant image comes out as 0."""
    lo, hi = img.min(), img.max()
    with np.errstate(invalid='ignore', divide='ignore'):
        scaled = 255 * ((img - lo) / (hi - lo))
    return np.where(np.isfinite(scaled), scaled, 0).astype(np.uint8)


def projected_landmarks(src, spec, geom):
    """[2, L] in preprocess.LAND_ORDER; inf where the name is absent."""
    have = fullres.volume_landmarks(src, spec)
    return np.stack([drr.project_points(geom, have[n])[:, 0] if n in have else np.full(2, np.inf) for n in preprocess.LAND_ORDER], 1)


def read_capsules(path, spec, idx):
    """[tools.Capsule] of 'projections/NNN/tools/capsules' of a file synthesize_dataset.py --tools wrote; none: []."""
    src = fullres.Source(path)
    try:
        pfx = fullres.projection_prefix(spec, idx)
        if 'tools' not in src.children(pfx) or 'capsules' not in src.children(pfx + 'tools'):
            return []
        return [tools.Capsule.from_row(row) for row in np.asarray(src.get(pfx + 'tools/capsules')).reshape(-1, 8)]
    finally:
        src.close()


def compare(src, spec, idx, crop, factor, geom, att, labels, lands, n_classes, dev, log=print):
    """The file's own projection, labels and landmarks on the same grid against the rendered ones."""
    pfx = fullres.projection_prefix(spec, idx)
    rot = [fullres.rot180(src, pfx)]
    pix = np.asarray(src.get(pfx + 'image/pixels'))
    if pix.dtype != np.uint16:
        pix = pix.astype(np.float32, copy=False)
    seg = np.asarray(src.get(pfx + 'gt-seg/pixels')).astype(np.uint8, copy=False)
    proj = preprocess.preprocess_projs(torch.from_numpy(np.ascontiguousarray(pix))[None].to(dev), rot, crop, factor)
    gt = preprocess.preprocess_segs(torch.from_numpy(np.ascontiguousarray(seg))[None].to(dev), rot, crop, factor)
    res = {'ncc': float(ncc.ncc_2d(att[None, None].contiguous(), proj[None].contiguous()).mean())}
    log('NCC(DRR, projection) = {:.6f}'.format(res['ncc']))
    dice = util.hard_dice(labels[None], gt, n_classes).cpu().numpy()[0]
    res['dice'] = dice
    for l, v in enumerate(dice):
        log('Dice of label {} = {:.6f}'.format(l + 1, v))
    have = fullres.gt_landmarks(src, pfx)
    dist = 0.0
    for l, name in enumerate(preprocess.LAND_ORDER):
        if name in have and np.all(np.isfinite(lands[:, l])):
            m = preprocess.map_lands(have[name].reshape(1, 2, 1), rot, pix.shape[0], pix.shape[1], crop, factor)[0, :, 0]
            dist = max(dist, float(np.hypot(*(m - lands[:, l]))))
    res['land_dist'] = dist
    log('largest landmark distance = {:.6f} px'.format(dist))
    return res


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    split = parse_tools(argv)
    parsed = parse(split[0]) if split is not None else None
    if parsed is None:
        print(USAGE.format(os.path.basename(sys.argv[0])))
        return 1
    (path, spec, idx), o = parsed
    idx = int(idx)
    if not torch.cuda.is_available():
        raise nat.DflError('no GPU visible: the rays are cast by a HIP kernel (no CPU path)')
    dev = dfl_amd.get_device()
    src = fullres.Source(path)
    try:
        geom = drr.geometry(src, spec, idx, crop=o['--crop'], factor=o['--ds-factor'], bones_only=o['--bones-only'])
        vol = drr.read_volume(src, spec, dev)
        att, _, labels = drr.render(vol, geom.objects, geom.grid)
        if o['--interp'] == 'trilinear':
            att, _, _ = drr.render(vol, geom.objects, geom.grid, interp='trilinear', step_mm=o['--step'])
        if split[1] is not None:
            caps = read_capsules(split[1], spec, idx)
            att = att[None].contiguous()
            tools.add_tools(att, geom.grid, [caps])
            att = att[0]
            print('{} capsules from {}'.format(len(caps), split[1]))
        lands = projected_landmarks(src, spec, geom)
        n_classes = max(vol.n_labels, 2)
        prefix = o['--out'] or '{}_{:03d}'.format(spec, idx)
        a = att.cpu().numpy()
        png.write(prefix + '_drr.png', np.repeat(to_u8(a)[:, :, None], 3, 2))
        png.write(prefix + '_labels.png', overlay.render(att, segs=labels, num_classes=n_classes)[0].cpu().numpy())
        np.savez(prefix + '.npz', att=a, labels=labels.cpu().numpy(), lands=lands)
        print('wrote {0}_drr.png, {0}_labels.png, {0}.npz ({1} x {2})'.format(prefix, *geom.size))
        if o['--compare']:
            compare(src, spec, idx, o['--crop'], o['--ds-factor'], geom, att, labels, lands, n_classes, dev)
    finally:
        src.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
