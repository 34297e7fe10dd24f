#!/usr/bin/env python3
"""Where is the pelvis in every projection of a specimen: the 2D/3D registration of examples/register_2d3d.py for many
projections of the full-resolution file at once (dfl_amd.register.register_many: every generation renders the candidates
of all projections in one dfl_drr_render launch and scores them against a bank of fixed images in one
dfl_sim_bank_gradncc launch).

    python examples/register_specimen.py full_res.h5 17-1882 --lands-csv lands.csv
    python examples/register_specimen.py full_res.h5 17-1882 --gt-lands --projs 0,3,7 --refine 20 --out run1
    python examples/register_specimen.py full_res.h5 17-1882 --gt-lands --similarity patch --patch-weight variance --refine 20
    python examples/register_specimen.py full_res.h5 17-1882 --gt-lands --mi-bins 16

Every selected projection (--projs, default: all of the specimen) gets its geometry, its preprocessed fixed image and its
start pose from landmarks (register.pnp) exactly as register_2d3d.py gives them to one projection: --lands-csv FILE reads
the 2D landmarks est_lands_csv.py writes, --gt-lands takes the projection's gt-landmarks.  All bones start at the pelvis
pose and follow it.  Projections whose detector image is turned (rot-180-for-up) have another pixel grid than the others,
so the two kinds go into one register_many call each.  The result of a projection has the bytes register_2d3d.py finds
for it alone with the same options.
--mi-bins N selects the mutual-information cost, as in register_2d3d.py (not with --similarity patch or --patch-weight variance).
A projection without enough usable landmarks for pnp is left out of the batch and written with empty fields; the exit
status is 1 only when no projection could be registered or the command line is not understood.
PREFIX_reg.csv: proj, start_rot_deg, start_trans_mm, rot_deg, trans_mm (register_2d3d.pose_errors against gt-poses; empty
without them), final_cost, renders, gradient_evaluations.  PREFIX_reg.npz: projs, registered (0 / 1), start_poses and
poses [n, 4, 4] (cam-to-pelvis-vol; NaN where not registered), theta [n, 6], final_cost [n].  The last line printed holds
the median and the largest of the two final errors.  The femurs (--femurs of register_2d3d.py) are not registered here.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, drr, fullres, preprocess, register as reg  # noqa: E402
from register_2d3d import _WithPoses, cost_keywords, parse_mi_bins, parse_patch_weight, parse_refine, parse_similarity, pose_errors, read_lands_csv  # noqa: E402

USAGE = ('Usage: {} <HDF5 full-res data file> <specimen ID> (--lands-csv FILE | --gt-lands) [--projs 0,3,7] [--out PREFIX] [--crop 50] '
         '[--ds-factor 8] [--popsize 16] [--generations 80] [--mi-bins N] [--patch-weight uniform|variance] [--seed 0] [--similarity global|patch] [--patch-radius 7] [--patch-stride 4] '
         '[--landmark-weight 0] [--refine 0] [--max-views N]')


def _projs(text):
    v = [int(t) for t in text.split(',')]
    if not v or min(v) < 0 or len(set(v)) != len(v):
        raise ValueError(text)
    return v


VALUED = {'--out': str, '--crop': int, '--ds-factor': int, '--popsize': int, '--generations': int, '--seed': int, '--lands-csv': str,
          '--projs': _projs, '--max-views': int}
DEFAULTS = {'--out': None, '--crop': 50, '--ds-factor': 8, '--popsize': 16, '--generations': 80, '--seed': 0, '--lands-csv': None,
            '--projs': None, '--max-views': None, '--gt-lands': False}


def parse(argv, patch_weight='uniform'):
    """((file, specimen), options) with '--refine', the options of the cost and the rest in one dict, or None when the
    command line is not understood, names no or two landmark sources, or asks for what register_many refuses.
    patch_weight is what register_2d3d.parse_patch_weight took out of the command line before."""
    fine = parse_refine(list(argv))
    cost = None if fine is None else parse_similarity(fine[0])
    if cost is None:
        return None
    opts, pos = dict(DEFAULTS, **cost[1]), []
    opts['--refine'] = fine[1]
    it = iter(cost[0])
    for a in it:
        if a == '--gt-lands':
            opts[a] = True
        elif a in VALUED:
            try:
                opts[a] = VALUED[a](next(it))
            except (StopIteration, ValueError):
                return None
        elif a.startswith('--'):
            return None
        else:
            pos.append(a)
    ok = len(pos) == 2 and (opts['--lands-csv'] is not None) + opts['--gt-lands'] == 1 and opts['--popsize'] >= 4 and \
        opts['--generations'] >= 0 and not (opts['--refine'] > 0 and opts['--similarity'] == 'patch' and patch_weight == 'uniform') and \
        not (patch_weight != 'uniform' and opts['--similarity'] != 'patch') and \
        (opts['--max-views'] is None or opts['--popsize'] <= opts['--max-views'] <= 65535)
    return (tuple(pos), opts) if ok else None


def main(argv=None):
    binned = parse_mi_bins(sys.argv[1:] if argv is None else argv)
    weighted = None if binned is None else parse_patch_weight(binned[0])
    parsed = None if weighted is None else parse(*weighted)
    if parsed is None or cost_keywords(parsed[1]['--similarity'], weighted[1], binned[1]) is None:
        print(USAGE.format(os.path.basename(sys.argv[0])))
        return 1
    (path, spec), o = parsed
    if not torch.cuda.is_available():
        raise nat.DflError('no GPU visible: the DRRs and the similarity are HIP kernels (no CPU path)')
    dev = dfl_amd.get_device()
    src = fullres.Source(path)
    try:
        count = fullres.n_projections(src, spec)
        projs = list(range(count)) if o['--projs'] is None else o['--projs']
        if not projs or max(projs) >= count:
            print('{} has the projections 0 .. {}, --projs asks for {}'.format(spec, count - 1, ','.join(str(p) for p in projs)))
            return 1
        vol = drr.read_volume(src, spec, dev)
        lands3d = fullres.volume_landmarks(src, spec)
        names = [n for n in preprocess.LAND_ORDER if n in lands3d]
        X3d = np.array([lands3d[n] for n in names]).reshape(-1, 3)
        jobs, rows = {}, {}                                       # jobs: projection -> what register_many needs of it
        for idx in projs:
            wrapped = _WithPoses(src)
            geom = drr.geometry(wrapped, spec, idx, crop=o['--crop'], factor=o['--ds-factor'], bones_only=True)
            pfx = fullres.projection_prefix(spec, idx)
            rot = [fullres.rot180(src, pfx)]
            pix = np.asarray(src.get(pfx + 'image/pixels'))
            if pix.dtype != np.uint16:
                pix = pix.astype(np.float32, copy=False)
            if o['--gt-lands']:
                have = fullres.gt_landmarks(src, pfx)
                x2d = np.full((2, len(names)), np.nan)
                for l, n in enumerate(names):
                    if n in have:
                        x2d[:, l] = preprocess.map_lands(have[n].reshape(1, 2, 1), rot, pix.shape[0], pix.shape[1], o['--crop'],
                                                         o['--ds-factor'])[0, :, 0]
            else:
                full = read_lands_csv(o['--lands-csv'], idx, len(preprocess.LAND_ORDER))
                x2d = np.stack([full[:, preprocess.LAND_ORDER.index(n)] for n in names], 1) if names else np.zeros((2, 0))
            try:
                P_start = reg.pnp(geom, X3d, x2d)
            except nat.DflError as e:
                print('projection {}: left out ({})'.format(idx, e))
                rows[idx] = None
                continue
            fixed = preprocess.preprocess_projs(torch.from_numpy(np.ascontiguousarray(pix))[None].to(dev), rot, o['--crop'], o['--ds-factor'])[0]
            jobs[idx] = dict(geom=geom, fixed=fixed, P0=P_start, lands=(X3d, x2d), rot=rot[0], gt=None if wrapped.missing else geom.poses[drr.POSES[0]])
        if not jobs:
            print('no projection of {} has enough usable landmarks for a start pose'.format(spec))
            return 1
        centre = reg.volume_centre(vol.shape, next(iter(jobs.values()))['geom'].I2P)
        for turned in (False, True):                              # one pixel grid per call
            group = [idx for idx in jobs if jobs[idx]['rot'] == turned]
            if not group:
                continue
            res = reg.register_many(vol, [jobs[i]['geom'] for i in group], torch.stack([jobs[i]['fixed'] for i in group]), moving=(0, 1, 2),
                                    P0=np.stack([jobs[i]['P0'] for i in group]), popsize=o['--popsize'], generations=o['--generations'],
                                    seed=o['--seed'], patch_radius=o['--patch-radius'],
                                    patch_stride=o['--patch-stride'], landmarks=[jobs[i]['lands'] for i in group],
                                    landmark_weight=o['--landmark-weight'] or 0.0, refine=o['--refine'], max_views=o['--max-views'],
                                    **cost_keywords(o['--similarity'], weighted[1], binned[1]))
            for i, r in zip(group, res):
                rows[i] = r
        prefix = o['--out'] or '{}_all'.format(spec)
        n = len(projs)
        start_poses, poses, thetas, costs = np.full((n, 4, 4), np.nan), np.full((n, 4, 4), np.nan), np.full((n, 6), np.nan), np.full(n, np.nan)
        errors = []
        with open(prefix + '_reg.csv', 'w') as f:
            f.write('proj,start_rot_deg,start_trans_mm,rot_deg,trans_mm,final_cost,renders,gradient_evaluations\n')
            for k, idx in enumerate(projs):
                r = rows[idx]
                if r is None:
                    f.write('{},,,,,,,\n'.format(idx))
                    continue
                start_poses[k], poses[k], thetas[k], costs[k] = jobs[idx]['P0'], r.pose, r.theta, r.final_cost
                err = ['', '', '', '']
                if jobs[idx]['gt'] is not None:
                    e = pose_errors(jobs[idx]['P0'], jobs[idx]['gt'], centre) + pose_errors(r.pose, jobs[idx]['gt'], centre)
                    errors.append(e[2:])
                    err = ['{:.6f}'.format(v) for v in e]
                f.write('{},{},{:.9f},{},{}\n'.format(idx, ','.join(err), r.final_cost, r.renders, r.gradient_evaluations))
        np.savez(prefix + '_reg.npz', projs=np.array(projs), registered=np.array([int(rows[i] is not None) for i in projs]),
                 start_poses=start_poses, poses=poses, theta=thetas, final_cost=costs)
        print('wrote {0}_reg.csv, {0}_reg.npz ({1} of {2} projections registered)'.format(prefix, len(jobs), n))
        if errors:
            e = np.array(errors)
            print('rotation error: median {:.4f} deg, largest {:.4f} deg; translation error: median {:.4f} mm, largest {:.4f} mm'
                  .format(np.median(e[:, 0]), e[:, 0].max(), np.median(e[:, 1]), e[:, 1].max()))
        else:
            print('no gt-poses: no errors to report')
    finally:
        src.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
