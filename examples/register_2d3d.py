#!/usr/bin/env python3
"""Where is the pelvis in this projection: 2D/3D registration of the CT of the full-resolution file to one of its
projections (dfl_amd.register: a start pose from landmarks, then a CMA-ES on the gradient-NCC between DRRs rendered by
dfl_drr_render and the projection, compared by dfl_sim_gradncc), on the pixel grid preprocess_full_res.py writes for the
same --crop and --ds-factor.

    python examples/register_2d3d.py full_res.h5 17-1882 0 --lands-csv lands.csv          # the start the paper uses
    python examples/register_2d3d.py full_res.h5 17-1882 0 --gt-lands --femurs
    python examples/register_2d3d.py full_res.h5 17-1882 0 --offset 2,-1.5,2.5,4,-3,15 --seed 1 --out run1
    python examples/register_2d3d.py full_res.h5 17-1882 0 --lands-csv lands.csv --similarity patch --landmark-weight 0.01
    python examples/register_2d3d.py full_res.h5 17-1882 0 --offset 2,-1.5,2.5,4,-3,15 --generations 25 --refine 30
    python examples/register_2d3d.py full_res.h5 17-1882 0 --gt-lands --similarity patch --patch-weight variance --refine 20
    python examples/register_2d3d.py full_res.h5 17-1882 0 --gt-lands --mi-bins 16 --refine 10

The start pose comes from exactly one of
  --lands-csv FILE   2D landmarks as est_lands_csv.py writes them (pat,proj,land,row,col,time on this grid; land indexes
                     preprocess.LAND_ORDER; row = col = -1: not found), solved for the pelvis pose by register.pnp;
  --gt-lands         the projection's gt-landmarks, solved the same way;
  --offset rx,ry,rz,tx,ty,tz   the ground-truth poses moved by register.pose_delta of these six parameters (rotation
                     in units of 0.02 rad about the volume centre, translation in mm).
--similarity global (the default) compares the whole image with one gradient-NCC; --similarity patch takes the mean over
patches of radius --patch-radius (7) every --patch-stride (4) pixels, which is less sensitive to what the CT does not hold.
--landmark-weight W (per square pixel, default 0) adds W times the mean squared distance between the projected 3D
landmarks and the 2D landmarks that gave the start to the pelvis cost; it needs a landmark start, not --offset.
--refine K (default 0) finishes every registration with at most K quasi-Newton iterations on the pose gradient of the
renderer (dfl_drr_pose_grad, dfl_sim_gradncc_bwd; the global similarity, or the patch one with --patch-weight variance) and
prints the cost before and after them.  --patch-weight variance (with --similarity patch; default uniform) weighs every
patch by the energy of the projection's gradient in it, so that flat background patches hardly count (dfl_sim_patch_eval).
--mi-bins N (2..64) replaces the gradient-NCC by the negative mutual information of the intensities over N x N bins
(dfl_sim_mi, register(similarity='mi'): no known intensity mapping of the projection is needed, and strong edges the CT
does not hold count as a few pixels); --refine works with it (dfl_sim_mi_bwd); not with --similarity patch or --patch-weight variance.
With a landmark start all bones begin at the pelvis pose (the anatomy as it was scanned).  The pelvis is registered with
every bone following it; --femurs then registers each femur on its own with the others held.
PREFIX_reg.npz holds start_poses and poses ([3, 4, 4] cam-to-{pelvis, left-femur, right-femur}-vol), cost (the best cost
of every generation), theta, similarity_cost and landmark_cost (the two parts of the pelvis cost at theta) and
start_lands / lands ([2, L] projected 3D landmarks).  PREFIX_reg.png shows the projection,
the DRR at the start pose and the DRR at the final pose side by side.  Where the file has gt-poses the rotation error
(degrees), the translation error (mm, of the volume centre) and the largest reprojection distance of the 3D landmarks
(pixels) of the pelvis are printed.
Files: the reference's HDF5 (dfl_amd.h5lite) or .npz with the same names as keys.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, drr, fullres, png, preprocess, register as reg  # noqa: E402
from full_res_drr import parse_options, to_u8  # noqa: E402

USAGE = ('Usage: {} <HDF5 full-res data file> <specimen ID> <projection index> (--lands-csv FILE | --gt-lands | --offset '
         'rx,ry,rz,tx,ty,tz) [--femurs] [--out PREFIX] [--crop 50] [--ds-factor 8] [--popsize 16] [--generations 80] [--sigma 2.0] '
         '[--step 1.0] [--mi-bins N] [--patch-weight uniform|variance] [--refine 0] [--seed 0] [--similarity global|patch] [--patch-radius 7] [--patch-stride 4] [--landmark-weight 0]')


def _six(text):
    v = [float(t) for t in text.split(',')]
    if len(v) != 6:
        raise ValueError(text)
    return v


VALUED = {'--out': str, '--crop': int, '--ds-factor': int, '--popsize': int, '--generations': int, '--seed': int, '--sigma': float,
          '--step': float, '--lands-csv': str, '--offset': _six}
FLAGS = ('--femurs', '--gt-lands')


def parse(argv):
    """(positional, options), or None when the command line is not understood or names no start or more than one."""
    parsed = parse_options(argv, VALUED, FLAGS, {'--out': None, '--crop': 50, '--ds-factor': 8, '--popsize': 16, '--generations': 80,
                                                 '--seed': 0, '--sigma': 2.0, '--step': 1.0, '--lands-csv': None, '--offset': None})
    if parsed is None:
        return None
    opts = parsed[1]
    starts = (opts['--lands-csv'] is not None) + bool(opts['--gt-lands']) + (opts['--offset'] is not None)
    return parsed if starts == 1 and opts['--popsize'] >= 4 and opts['--generations'] >= 1 else None


SIMILARITY = {'--similarity': str, '--patch-radius': int, '--patch-stride': int, '--landmark-weight': float}


def parse_similarity(argv):
    """(the command line without the options of the cost, those options), or None when one of them has no or a bad value.
    '--landmark-weight' is None when it was not given."""
    rest, opts = [], {'--similarity': 'global', '--patch-radius': 7, '--patch-stride': 4, '--landmark-weight': None}
    it = iter(argv)
    for a in it:
        if a not in SIMILARITY:
            rest.append(a)
            continue
        try:
            opts[a] = SIMILARITY[a](next(it))
        except (StopIteration, ValueError):
            return None
    w = opts['--landmark-weight']
    if opts['--similarity'] not in ('global', 'patch') or opts['--patch-radius'] < 1 or opts['--patch-stride'] < 1 or \
            (w is not None and not (w >= 0.0 and np.isfinite(w))):
        return None
    return rest, opts


def parse_patch_weight(argv):
    """(the command line without --patch-weight W, W), W = 'uniform' when it was not given; None when it has no or an unknown value."""
    rest, weight = [], 'uniform'
    it = iter(argv)
    for a in it:
        if a != '--patch-weight':
            rest.append(a)
            continue
        weight = next(it, None)
        if weight not in ('uniform', 'variance'):
            return None
    return rest, weight


def parse_mi_bins(argv):
    """(the command line without --mi-bins N, N), N = None when it was not given; None when it has no value or one outside 2..64."""
    rest, bins = [], None
    it = iter(argv)
    for a in it:
        if a != '--mi-bins':
            rest.append(a)
            continue
        try:
            bins = int(next(it))
        except (StopIteration, ValueError):
            return None
        if not 2 <= bins <= 64:
            return None
    return rest, bins


def cost_keywords(similarity, patch_weight, mi_bins):
    """The keywords of register() and register_many() that select the cost, or None for --mi-bins together with patches."""
    if mi_bins is None:
        return dict(similarity=similarity, patch_weight=patch_weight)
    if similarity == 'patch' or patch_weight != 'uniform':
        return None
    return dict(similarity='mi', mi_bins=mi_bins)


def parse_refine(argv):
    """(the command line without --refine K, K), K = 0 when it was not given; None when it has no or a bad value."""
    rest, refine = [], 0
    it = iter(argv)
    for a in it:
        if a != '--refine':
            rest.append(a)
            continue
        try:
            refine = int(next(it))
        except (StopIteration, ValueError):
            return None
        if refine < 0:
            return None
    return rest, refine


def read_lands_csv(path, proj, n_lands):
    """[2, n_lands] (column, row), NaN where the landmark was not found or is not listed for projection `proj`."""
    out = np.full((2, n_lands), np.nan)
    with open(path) as f:
        for line in f:
            cells = line.strip().split(',')
            if len(cells) < 5 or not cells[1].strip().lstrip('-').isdigit():
                continue                                          # the header
            if int(cells[1]) != proj or not 0 <= int(cells[2]) < n_lands:
                continue
            row, col = float(cells[3]), float(cells[4])
            if row >= 0 and col >= 0:
                out[:, int(cells[2])] = col, row
    return out


class _WithPoses:
    """A source whose missing gt-poses read as the identity (drr.geometry needs the three names)."""

    def __init__(self, src):
        self.src, self.missing = src, False

    def get(self, path):
        try:
            return self.src.get(path)
        except KeyError:
            if path.rsplit('/', 1)[-1] not in drr.POSES:
                raise
            self.missing = True
            return np.eye(4)


def pose_errors(P, P_gt, centre):
    """(rotation error in degrees, translation error in mm: how far the volume centre is from where it belongs)."""
    Dm = P @ np.linalg.inv(P_gt)
    ang = np.degrees(np.arccos(np.clip(0.5 * (np.trace(Dm[:3, :3]) - 1.0), -1.0, 1.0)))
    return float(ang), float(np.linalg.norm(Dm[:3, :3] @ centre + Dm[:3, 3] - centre))


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    binned = parse_mi_bins(argv)
    weighted = None if binned is None else parse_patch_weight(binned[0])
    fine = None if weighted is None else parse_refine(weighted[0])
    cost = None if fine is None else parse_similarity(fine[0])
    parsed = None if cost is None else parse(cost[0])
    if parsed is None or (cost[1]['--landmark-weight'] is not None and parsed[1]['--offset'] is not None) or \
            (fine[1] > 0 and cost[1]['--similarity'] == 'patch' and weighted[1] == 'uniform') or \
            (weighted[1] != 'uniform' and cost[1]['--similarity'] != 'patch') or \
            cost_keywords(cost[1]['--similarity'], weighted[1], binned[1]) is None:
        print(USAGE.format(os.path.basename(sys.argv[0])))
        return 1
    (path, spec, idx), o = parsed
    so = cost[1]
    idx = int(idx)
    if not torch.cuda.is_available():
        raise nat.DflError('no GPU visible: the DRRs and the similarity are HIP kernels (no CPU path)')
    dev = dfl_amd.get_device()
    src = fullres.Source(path)
    try:
        wrapped = _WithPoses(src)
        geom = drr.geometry(wrapped, spec, idx, crop=o['--crop'], factor=o['--ds-factor'], bones_only=True)
        has_gt = not wrapped.missing
        if o['--offset'] is not None and not has_gt:
            raise nat.DflError('--offset starts from the ground-truth poses, and this projection has none')
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
        kw = dict(popsize=o['--popsize'], generations=o['--generations'], sigma0=o['--sigma'], step_mm=o['--step'], seed=o['--seed'],
                  patch_radius=so['--patch-radius'], patch_stride=so['--patch-stride'], refine=fine[1],
                  **cost_keywords(so['--similarity'], weighted[1], binned[1]))

        def refined(what, r):
            if len(r.refine_cost):
                print('{}: refinement cost {:.6f} -> {:.6f} in {} gradient evaluations'.format(what, r.refine_cost[0], r.refine_cost[-1],
                                                                                                r.gradient_evaluations))

        if o['--offset'] is not None:
            Dm = reg.pose_delta(o['--offset'], centre)
            start = [Dm @ geom.poses[k] for k in drr.POSES]
            res = reg.register(vol, geom, fixed, moving=(0, 1, 2), theta0=o['--offset'], **kw)
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
            P_start = reg.pnp(geom, X3d, x2d)
            start = [P_start] * 3
            res = reg.register(vol, geom, fixed, moving=(0, 1, 2), P0=P_start, landmarks=(X3d, x2d),
                               landmark_weight=so['--landmark-weight'] or 0.0, **kw)
        poses, trace, renders = list(res.poses), [res.cost], res.renders
        print('pelvis: cost {:.6f} -> {:.6f} in {} renders'.format(res.cost[0], res.final_cost, res.renders))
        refined('pelvis', res)
        if res.landmark_cost:
            print('pelvis: similarity {:.6f}, landmark term {:.6f}'.format(res.similarity_cost, res.landmark_cost))
        if o['--femurs']:
            for n in (1, 2):
                held = drr.Geometry(geom.K, geom.E, geom.poses, geom.I2P, geom.G,
                                    [drr.Obj(back @ P @ Ei, ob.mask) for P, ob in zip(poses, geom.objects)], geom.grid)
                r = reg.register(vol, held, fixed, moving=(n,), **kw)
                poses[n] = r.pose
                trace.append(r.cost)
                renders += r.renders
                print('{}: cost {:.6f} -> {:.6f} in {} renders'.format(drr.POSES[n], r.cost[0], r.final_cost, r.renders))
                refined(drr.POSES[n], r)

        def view(ps):
            return drr.render(vol, [drr.Obj(back @ P @ Ei, ob.mask) for P, ob in zip(ps, geom.objects)], geom.grid,
                              interp='trilinear', step_mm=o['--step'])[0].cpu().numpy()

        def lands(P):
            return drr.project_points(reg.with_pelvis_pose(geom, P), X3d) if len(names) else np.zeros((2, 0))

        prefix = o['--out'] or '{}_{:03d}'.format(spec, idx)
        panel = np.concatenate([to_u8(fixed.cpu().numpy()), to_u8(view(start)), to_u8(view(poses))], 1)
        png.write(prefix + '_reg.png', np.repeat(panel[:, :, None], 3, 2))
        np.savez(prefix + '_reg.npz', start_poses=np.stack(start), poses=np.stack(poses), cost=np.concatenate(trace), theta=res.theta,
                 similarity_cost=res.similarity_cost, landmark_cost=res.landmark_cost, start_lands=lands(start[0]), lands=lands(poses[0]), land_names=np.array(names))
        print('wrote {0}_reg.npz, {0}_reg.png ({1} x {2}, {3} renders)'.format(prefix, geom.size[0], geom.size[1], renders))
        if has_gt:
            P_gt = geom.poses[drr.POSES[0]]
            for what, P in (('start', start[0]), ('final', poses[0])):
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
