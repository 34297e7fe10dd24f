#!/usr/bin/env python3
"""Register the CT to a projection on the bone outlines the network predicted, then on intensities: the 2D/3D
registration of examples/register_2d3d.py with a coarse first stage whose cost is the truncated chamfer distance between
the boundaries of the predicted label map and of the label maps dfl_drr_render writes for the candidate poses
(dfl_amd.register(similarity='outline'): dfl_label_edt and dfl_sim_outline).  The outline cost sees
a pose from half an image away and needs no landmarks; the gradient-NCC stage that follows resolves what is below a pixel.

    python examples/register_outline.py full_res.h5 17-1882 0 out.h5 nn-segs --lands-csv lands.csv --clean
    python examples/register_outline.py full_res.h5 17-1882 1 out.h5 nn-segs-clean --start-npz 17-1882_000_reg.npz
    python examples/register_outline.py full_res.h5 17-1882 0 out.h5 nn-segs --offset 5,-3.75,6.25,10,-7.5,37.5 --out run1

The fourth and fifth argument name the results file and its dataset of predicted label maps (what test_ensemble.py or
clean_segs.py wrote, [N, H, W] uint8 on the grid of --crop and --ds-factor); row <projection index> is used.  --clean
passes it through labels.clean first, with the defaults of clean_segs.py (per bone the largest component).
The start pose comes from exactly one of
  --start-npz FILE   `poses` of an earlier PREFIX_reg.npz, for example the neighbouring projection's: the way in when
                     fewer than 4 landmarks were found;
  --lands-csv FILE, --gt-lands, --offset rx,ry,rz,tx,ty,tz   as register_2d3d.py takes them.
Stage 1 (--outline-generations, --outline-sigma, --outline-cap in pixels) moves all bones together on the outline cost;
stage 2 (--generations, --sigma) continues from its result with the global gradient-NCC and seed + 1.  The cost of both
stages is printed, and where the file has gt-poses the pose errors of the pelvis at the start, after stage 1 ('outline')
and at the end ('final').  PREFIX_reg.npz holds what register_2d3d.py writes plus outline_poses [3, 4, 4] and outline_cost
(the best cost of every generation of stage 1; `cost` is stage 2's); PREFIX_reg.png shows the projection, the DRR at the
start pose and the DRR at the final pose side by side.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, dataset, drr, fullres, labels, png, preprocess, register as reg  # noqa: E402
from full_res_drr import to_u8  # noqa: E402
from register_2d3d import _WithPoses, _six, pose_errors, read_lands_csv  # noqa: E402

USAGE = ('Usage: {} <HDF5 full-res data file> <specimen ID> <projection index> <results file> <segmentation dataset> '
         '(--start-npz FILE | --lands-csv FILE | --gt-lands | --offset rx,ry,rz,tx,ty,tz) [--clean] [--outline-generations 40] '
         '[--outline-sigma 4.0] [--outline-cap 32] [--generations 40] [--sigma 1.0] [--out PREFIX] [--crop 50] [--ds-factor 8] '
         '[--popsize 16] [--seed 0] [--step 1.0]')

VALUED = {'--start-npz': str, '--lands-csv': str, '--offset': _six, '--outline-generations': int, '--outline-sigma': float,
          '--outline-cap': float, '--generations': int, '--sigma': float, '--out': str, '--crop': int, '--ds-factor': int,
          '--popsize': int, '--seed': int, '--step': float}
FLAGS = ('--gt-lands', '--clean')
DEFAULTS = {'--start-npz': None, '--lands-csv': None, '--offset': None, '--gt-lands': False, '--clean': False, '--outline-generations': 40,
            '--outline-sigma': 4.0, '--outline-cap': 32.0, '--generations': 40, '--sigma': 1.0, '--out': None, '--crop': 50,
            '--ds-factor': 8, '--popsize': 16, '--seed': 0, '--step': 1.0}


def parse(argv):
    """((file, specimen, projection, results file, dataset), options), or None when the command line is not understood, names
    no start or more than one, or holds a value register() would refuse."""
    opts, pos = dict(DEFAULTS), []
    it = iter(argv)
    for a in it:
        if a in VALUED:
            try:
                opts[a] = VALUED[a](next(it))
            except (StopIteration, ValueError):
                return None
        elif a in FLAGS:
            opts[a] = True
        elif a.startswith('--'):
            return None
        else:
            pos.append(a)
    starts = sum(opts[k] is not None for k in ('--start-npz', '--lands-csv', '--offset')) + bool(opts['--gt-lands'])
    positive = all(opts[k] > 0 and np.isfinite(opts[k]) for k in ('--outline-sigma', '--outline-cap', '--sigma', '--step'))
    if len(pos) != 5 or not pos[2].isdigit() or starts != 1 or not positive or opts['--popsize'] < 4 or opts['--outline-generations'] < 1 or \
            opts['--generations'] < 1 or opts['--crop'] < 0 or opts['--ds-factor'] < 1:
        return None
    return tuple(pos), opts


def read_segmentation(path, name, proj, size, dev, clean):
    """Row `proj` of dataset `name` of the results file as a uint8 [H, W] tensor on the device; `size` is the grid's."""
    get, close = dataset._open_container(path)
    try:
        segs = np.asarray(get(name))
    finally:
        close()
    if segs.ndim != 3 or not 0 <= proj < segs.shape[0] or tuple(segs.shape[1:]) != tuple(size):
        raise nat.DflError('{}: {} has shape {}: [N, {}, {}] with N > {} expected (the grid of --crop and --ds-factor)'.format(
            path, name, segs.shape, size[0], size[1], proj))
    seg = torch.from_numpy(np.ascontiguousarray(segs[proj]).astype(np.uint8)).to(dev)
    return labels.clean(seg)[0] if clean else seg


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    parsed = parse(argv)
    if parsed is None:
        print(USAGE.format(os.path.basename(sys.argv[0])))
        return 1
    (path, spec, idx, seg_path, seg_name), o = parsed
    idx = int(idx)
    if not torch.cuda.is_available():
        raise nat.DflError('no GPU visible: the DRRs, the distance maps and the costs are HIP kernels (no CPU path)')
    dev = dfl_amd.get_device()
    src = fullres.Source(path)
    try:
        wrapped = _WithPoses(src)
        geom = drr.geometry(wrapped, spec, idx, crop=o['--crop'], factor=o['--ds-factor'], bones_only=True)
        has_gt = not wrapped.missing
        if o['--offset'] is not None and not has_gt:
            raise nat.DflError('--offset starts from the ground-truth poses, and this projection has none')
        seg = read_segmentation(seg_path, seg_name, idx, geom.size, dev, o['--clean'])
        vol = drr.read_volume(src, spec, dev)
        pfx = fullres.projection_prefix(spec, idx)
        rot = [fullres.rot180(src, pfx)]
        pix = np.asarray(src.get(pfx + 'image/pixels'))
        if pix.dtype != np.uint16:
            pix = pix.astype(np.float32, copy=False)
        fixed = preprocess.preprocess_projs(torch.from_numpy(np.ascontiguousarray(pix))[None].to(dev), rot, o['--crop'], o['--ds-factor'])[0]
        lands3d = fullres.volume_landmarks(src, spec)
        names = [n for n in preprocess.LAND_ORDER if n in lands3d]
        X3d = np.array([lands3d[n] for n in names]).reshape(-1, 3)
        centre = reg.volume_centre(vol.shape, geom.I2P)
        back, Ei = np.linalg.inv(geom.I2P), np.linalg.inv(geom.E)

        def placed(ps):
            return drr.Geometry(geom.K, geom.E, geom.poses, geom.I2P, geom.G, [drr.Obj(back @ P @ Ei, ob.mask) for P, ob in zip(ps, geom.objects)],
                                geom.grid)

        theta0 = np.zeros(6)
        if o['--offset'] is not None:
            theta0 = np.array(o['--offset'])
            base, start = geom, [reg.pose_delta(theta0, centre) @ geom.poses[k] for k in drr.POSES]
        elif o['--start-npz'] is not None:
            start = list(np.asarray(np.load(o['--start-npz'])['poses'], np.float64).reshape(3, 4, 4))
            base = placed(start)
        else:
            if o['--gt-lands']:
                have = fullres.gt_landmarks(src, pfx)
                x2d = np.full((2, len(names)), np.nan)
                for l, n in enumerate(names):
                    if n in have:
                        x2d[:, l] = preprocess.map_lands(have[n].reshape(1, 2, 1), rot, pix.shape[0], pix.shape[1], o['--crop'], o['--ds-factor'])[0, :, 0]
            else:
                full = read_lands_csv(o['--lands-csv'], idx, len(preprocess.LAND_ORDER))
                x2d = np.stack([full[:, preprocess.LAND_ORDER.index(n)] for n in names], 1) if names else np.zeros((2, 0))
            usable = int((np.isfinite(x2d).all(0) & np.isfinite(X3d).all(1)).sum()) if len(names) else 0
            if usable < 4:
                print('{} usable landmarks for projection {}: register.pnp needs at least 4.  Start from a pose instead: --start-npz '
                      'PREFIX_reg.npz of a neighbouring projection'.format(usable, idx))
                return 1
            start = [reg.pnp(geom, X3d, x2d)] * 3
            base = placed(start)
        kw = dict(moving=(0, 1, 2), popsize=o['--popsize'], step_mm=o['--step'])
        first = reg.register(vol, base, None, theta0=theta0, similarity='outline', segmentation=seg, outline_cap=o['--outline-cap'],
                             generations=o['--outline-generations'], sigma0=o['--outline-sigma'], seed=o['--seed'], **kw)
        print('outline: cost {:.6f} -> {:.6f} in {} renders'.format(first.cost[0], first.final_cost, first.renders))
        res = reg.register(vol, base, fixed, theta0=first.theta, similarity='global', generations=o['--generations'], sigma0=o['--sigma'],
                           seed=o['--seed'] + 1, **kw)
        print('gradient-NCC: cost {:.6f} -> {:.6f} in {} renders'.format(res.cost[0], res.final_cost, res.renders))
        poses = list(res.poses)

        def view(ps):
            return drr.render(vol, [drr.Obj(back @ P @ Ei, ob.mask) for P, ob in zip(ps, geom.objects)], geom.grid,
                              interp='trilinear', step_mm=o['--step'])[0].cpu().numpy()

        def lands(P):
            return drr.project_points(reg.with_pelvis_pose(geom, P), X3d) if len(names) else np.zeros((2, 0))

        prefix = o['--out'] or '{}_{:03d}'.format(spec, idx)
        panel = np.concatenate([to_u8(fixed.cpu().numpy()), to_u8(view(start)), to_u8(view(poses))], 1)
        png.write(prefix + '_reg.png', np.repeat(panel[:, :, None], 3, 2))
        np.savez(prefix + '_reg.npz', start_poses=np.stack(start), poses=np.stack(poses), cost=res.cost, theta=res.theta,
                 similarity_cost=res.similarity_cost, landmark_cost=res.landmark_cost, start_lands=lands(start[0]), lands=lands(poses[0]),
                 land_names=np.array(names), outline_poses=np.stack(first.poses), outline_cost=first.cost)
        print('wrote {0}_reg.npz, {0}_reg.png ({1} x {2}, {3} renders)'.format(prefix, geom.size[0], geom.size[1], first.renders + res.renders))
        if has_gt:
            P_gt = geom.poses[drr.POSES[0]]
            for what, P in (('start', start[0]), ('outline', first.poses[0]), ('final', poses[0])):
                ang, mm = pose_errors(P, P_gt, centre)
                print('{} rotation error = {:.4f} deg'.format(what, ang))
                print('{} translation error = {:.4f} mm'.format(what, mm))
                if len(names):
                    print('{} largest reprojection distance = {:.4f} px'.format(what, float(np.hypot(*(lands(P) - lands(P_gt))).max())))
    finally:
        src.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
