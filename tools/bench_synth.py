"""Times of the synthesis path (dfl_amd.synth) on one GPU, on the phantom of tools/bench_drr.py (a CT of 384 x 320 x 400
voxels of 0.8 mm, three label blobs under three poses, a 1536 x 1536 detector of 0.194 mm pixels), 8 views per launch:

  render    dfl_drr_render on the full detector grid, exact, tight boxes, att + label map, with and without the
            soft-tissue object (the pelvis pose with bit 0)
  expose    dfl_drr_expose for blur sigma 0 and 1, float32 and uint16 output, noise on; next to it the same arithmetic
            with torch ops on the device (exp, two conv2d passes over a replicate-padded image, randn_like for the normals,
            clamp / round / cast): what one would write without the kernel
  preproc   dfl_preproc_projs and dfl_preproc_segs, crop 50, factor 8, on the uint16 images and the label maps
  synthesize  views per second end to end for both layouts, from a container written here: poses, render, expose,
            (preprocess,) the copy to the host and the h5lite writes; the volumes are not copied into the output
            (--no-volumes).  Two lengths are run; the rate is taken from their difference, the rest is the fixed cost
            per specimen (reading and uploading the CT, its boxes)

Device kernels are timed with device events around back-to-back calls (argument blocks built once), after a warm-up,
`reps` windows of at least --window seconds each; the median is reported with the spread.  synthesize is timed by the
wall clock.

    python tools/bench_synth.py [--window 0.3] [--reps 5] [--out profiles/synth_bench.json]
"""
import argparse
import datetime
import json
import os
import socket
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import bench_drr as B  # noqa: E402

VIEWS = 8
PHOTONS, GAIN, ESIGMA = 20000.0, 2.0, 3.0
SPEC = 'phantom'


def measure(fn, window, reps):
    """{'ms', 'min_ms', 'max_ms', 'launches_per_window'} per call of fn."""
    B.timed(fn, 1)
    iters = max(int(1e3 * window / max(B.timed(fn, 1), 1e-3)) + 1, 1)
    ms = [B.timed(fn, iters) for _ in range(reps)]
    return {'ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms), 'launches_per_window': iters}


def per_view(m):
    return {'ms_per_view': round(m['ms'] / VIEWS, 4), 'min_ms_per_view': round(m['min_ms'] / VIEWS, 4),
            'max_ms_per_view': round(m['max_ms'] / VIEWS, 4), 'launches_per_window': m['launches_per_window']}


def torch_expose(att, taps, u16):
    """The detector model with torch ops (its own normals: the cost is what is compared, not the bits)."""
    import torch
    import torch.nn.functional as F
    T = torch.exp(-att)
    rho = (taps.numel() - 1) // 2
    if rho:
        x = F.pad(T[:, None], (rho, rho, rho, rho), mode='replicate')
        x = F.conv2d(x, taps.reshape(1, 1, 1, -1))
        T = F.conv2d(x, taps.reshape(1, 1, -1, 1))[:, 0]
    N = PHOTONS * T
    out = GAIN * (N + torch.sqrt(N) * torch.randn_like(N) + ESIGMA * torch.randn_like(N))
    return out.clamp_(0, 65535).round_().to(torch.uint16) if u16 else out


def write_container(path, mu_hu, lab, K, n_seeds=2):
    from dfl_amd import drr, h5lite
    I2P = np.eye(4)
    I2P[:3, :3] *= B.SPACING
    I2P[:3, 3] = [-150.0, -120.0, -160.0]
    with h5lite.File(path, 'w') as f:
        f['proj-params/intrinsic'] = K
        f['proj-params/extrinsic'] = np.eye(4)
        f['proj-params/num-rows'] = np.int64(B.DET)
        f['proj-params/num-cols'] = np.int64(B.DET)
        for grp, px in ((SPEC + '/vol/', mu_hu), (SPEC + '/vol-seg/image/', lab)):
            f[grp + 'pixels'] = px
            f[grp + 'dir-mat'] = np.eye(3)
            f[grp + 'spacing'] = np.full(3, B.SPACING)
            f[grp + 'origin'] = I2P[:3, 3]
        names = ('FH-l', 'FH-r', 'GSN-l', 'GSN-r', 'IOF-l', 'IOF-r')
        spots = ((90, 200, 150), (294, 200, 150), (150, 150, 200), (234, 150, 200), (170, 120, 230), (214, 120, 230))
        for name, idx in zip(names, spots):
            f[SPEC + '/vol-landmarks/' + name] = (I2P @ np.array(idx + (1.0,)))[:3].reshape(3, 1)
        for p, view in enumerate(B.poses(n_seeds)):
            pfx = SPEC + '/projections/%03d/' % p
            for k, A in zip(drr.POSES, view):                 # C2I = inv(I2P) P inv(E) with E = identity
                f[pfx + 'gt-poses/' + k] = I2P @ A
            f[pfx + 'gt-poses/left-femur-good-fov'] = np.int64(1)
            f[pfx + 'gt-poses/right-femur-good-fov'] = np.int64(1)
            f[pfx + 'rot-180-for-up'] = np.int64(p % 2)
            for g in ('image/', 'gt-seg/'):
                f[pfx + g + 'spacing'] = np.full(2, B.PIXEL_MM)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=0.3, help='seconds of device work per timed window, at least')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'synth_bench.json'))
    ap.add_argument('--no-end-to-end', action='store_true', help='kernels only')
    args = ap.parse_args()
    import torch
    from dfl_amd import _native as nat, drr, preprocess, synth
    if not torch.cuda.is_available():
        raise SystemExit('bench_synth.py needs a GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda', 0)
    mu, lab = B.phantom(dev)
    vol = drr.Volume(mu, lab)
    f = 1000.0 / B.PIXEL_MM
    K = np.array([[-f, 0, 767.5], [0, -f, 767.5], [0, 0, 1]])
    stream = torch.cuda.current_stream(dev).cuda_stream
    prop = torch.cuda.get_device_properties(dev)
    res = {'tool': 'tools/bench_synth.py --window %g --reps %d (device events around back-to-back calls; median of the repetitions; '
                   'synthesize by the wall clock)' % (args.window, args.reps),
           'date': datetime.date.today().isoformat(), 'host': socket.gethostname(), 'device': torch.cuda.get_device_name(dev),
           'arch': getattr(prop, 'gcnArchName', ''), 'compute_units': prop.multi_processor_count, 'torch': torch.__version__,
           'hip': torch.version.hip, 'volume': [B.NX, B.NY, B.NZ], 'detector': [B.DET, B.DET], 'views_per_launch': VIEWS,
           'photons': PHOTONS, 'gain': GAIN, 'electronic_sigma': ESIGMA, 'render': {}, 'expose': {}, 'preproc': {}, 'synthesize': {}}
    grid = drr.Grid(-np.linalg.inv(K), B.DET, B.DET)
    att = None
    for name, soft in (('bones', False), ('bones_and_soft_tissue', True)):
        objs = [[drr.Obj(A, m) for A, m in zip(view, drr.DEFAULT_MASKS)] + ([drr.Obj(view[0], (0,))] if soft else []) for view in B.poses(VIEWS)]
        a, (att, _, labels), keep = drr.render_args(vol, objs, grid, interp='exact', want_plen=False, want_labels=True, tight_boxes=True)
        res['render'][name] = per_view(measure(lambda a=a: nat.call('dfl_drr_render', a, stream), args.window, args.reps))
        print('render %-22s %.4f ms per view' % (name, res['render'][name]['ms_per_view']), flush=True)
    keys = [synth.noise_keys(0, 0, v) for v in range(VIEWS)]
    kq, ke = [q for q, _ in keys], [e for _, e in keys]
    img = None
    for sigma in (0.0, 1.0):
        taps = torch.from_numpy(synth.gaussian_taps(sigma)[0]).to(dev)
        for u16 in (False, True):
            a, (out, _, _), keep = synth.expose_args(att, PHOTONS, GAIN, ESIGMA, sigma, kq, ke, u16=u16)
            case = per_view(measure(lambda a=a: nat.call('dfl_drr_expose', a, stream), args.window, args.reps))
            case['torch_ops'] = per_view(measure(lambda: torch_expose(att, taps, u16), args.window, args.reps))
            case['bytes_per_pixel'] = 4 + (2 if u16 else 4)
            case['GB_per_s'] = round(case['bytes_per_pixel'] * B.DET * B.DET / (case['ms_per_view'] * 1e6), 1)
            key = 'sigma%g/%s' % (sigma, 'uint16' if u16 else 'float32')
            res['expose'][key] = case
            print('expose %-16s %.4f ms per view (%.0f GB/s), torch ops %.4f ms' % (key, case['ms_per_view'], case['GB_per_s'],
                                                                                   case['torch_ops']['ms_per_view']), flush=True)
            if u16:
                img = out
    rots = torch.tensor([v % 2 for v in range(VIEWS)], dtype=torch.int32, device=dev)
    res['preproc']['projs_uint16_f8'] = per_view(measure(lambda: preprocess.preprocess_projs(img, rots, B.CROP, 8), args.window, args.reps))
    res['preproc']['segs_f8'] = per_view(measure(lambda: preprocess.preprocess_segs(labels, rots, B.CROP, 8), args.window, args.reps))
    res['preproc']['note'] = 'through the Python wrappers (they allocate their outputs; preprocess_segs reads its status word back)'
    for k in ('projs_uint16_f8', 'segs_f8'):
        print('preproc %-16s %.4f ms per view' % (k, res['preproc'][k]['ms_per_view']), flush=True)
    r = res['render']['bones_and_soft_tissue']['ms_per_view']
    res['expose_over_render'] = {k: round(v['ms_per_view'] / r, 4) for k, v in res['expose'].items()}
    if not args.no_end_to_end:
        with tempfile.TemporaryDirectory() as d:
            src = os.path.join(d, 'phantom.h5')
            hu = (mu / 0.02 * 1000.0 - 1000.0).cpu().numpy()
            t0 = time.perf_counter()
            write_container(src, hu, lab.cpu().numpy(), K)
            res['synthesize']['container_write_s'] = round(time.perf_counter() - t0, 2)
            del hu
            for layout in ('full-res', 'preprocessed'):
                secs = {}
                for views in (8, 40):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    synth.synthesize(src, os.path.join(d, 'out.h5'), views, seed=1, layout=layout, volumes=False, rot_sigma_deg=3.0,
                                     trans_sigma_mm=(5.0, 5.0, 20.0), chunk=VIEWS)
                    secs[views] = time.perf_counter() - t0
                    size = os.path.getsize(os.path.join(d, 'out.h5'))
                per = (secs[40] - secs[8]) / 32.0
                res['synthesize'][layout] = {'seconds_8_views': round(secs[8], 3), 'seconds_40_views': round(secs[40], 3),
                                             'ms_per_view': round(1e3 * per, 2), 'views_per_second': round(1.0 / per, 1),
                                             'fixed_seconds_per_specimen': round(secs[8] - 8 * per, 3), 'bytes_40_views': size}
                print('synthesize %-13s %.1f views per second (%.2f ms per view; %.2f s fixed per specimen)'
                      % (layout, 1.0 / per, 1e3 * per, secs[8] - 8 * per), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
