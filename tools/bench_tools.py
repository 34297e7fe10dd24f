"""Times of the tool kernel (dfl_drr_tools, dfl_amd.tools) on one GPU beside the kernels it sits between, on the phantom
and the views of tools/bench_synth.py (a CT of 384 x 320 x 400 voxels, a 1536 x 1536 detector, 8 views per launch):

  render      dfl_drr_render, exact, tight boxes, att + label map, with and without the soft-tissue object
  expose      dfl_drr_expose, blur sigma 1, uint16 and float32 output, noise on
  tools       dfl_drr_tools with 8 and with 64 capsules per view (tools.sample_tools around the phantom's landmarks,
              drawn until the view has that many), with the host's pixel rectangles and with whole-image ones, and
              once with the tool_len output
  synthesize  views per second end to end with --tools 8 against --tools 0 (layout 'preprocessed', volumes left out),
              from the difference of two lengths as tools/bench_synth.py takes it

Device kernels are timed with device events around back-to-back calls (argument blocks built once), after a warm-up,
`reps` windows of at least --window seconds each; the median is reported with the spread.  The tool launches add to a
scratch copy of att over and over: the values grow, the work does not change.

    python tools/bench_tools.py [--window 0.3] [--reps 5] [--out profiles/tools_bench.json]
"""
import argparse
import datetime
import json
import os
import socket
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import bench_drr as B  # noqa: E402
import bench_synth as S  # noqa: E402

VIEWS = S.VIEWS
SPOTS = ((90, 200, 150), (294, 200, 150), (150, 150, 200), (234, 150, 200), (170, 120, 230), (214, 120, 230))   # bench_synth's landmarks


def capsules(view, n, seed):
    """n capsules around the phantom's landmarks under one view's pelvis pose (C2I: camera -> index coordinates)."""
    from dfl_amd import tools
    back = np.linalg.inv(view[0])
    cam = np.array([(back @ np.array(idx + (1.0,)))[:3] for idx in SPOTS])
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        out += tools.sample_tools(rng, cam, 8)
    return out[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=0.3, help='seconds of device work per timed window, at least')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tools_bench.json'))
    ap.add_argument('--no-end-to-end', action='store_true', help='kernels only')
    args = ap.parse_args()
    import torch
    from dfl_amd import _native as nat, drr, synth, tools
    if not torch.cuda.is_available():
        raise SystemExit('bench_tools.py needs a GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda', 0)
    mu, lab = B.phantom(dev)
    vol = drr.Volume(mu, lab)
    f = 1000.0 / B.PIXEL_MM
    K = np.array([[-f, 0, 767.5], [0, -f, 767.5], [0, 0, 1]])
    stream = torch.cuda.current_stream(dev).cuda_stream
    prop = torch.cuda.get_device_properties(dev)
    res = {'tool': 'tools/bench_tools.py --window %g --reps %d (device events around back-to-back calls; median of the repetitions; '
                   'synthesize by the wall clock)' % (args.window, args.reps),
           'date': datetime.date.today().isoformat(), 'host': socket.gethostname(), 'device': torch.cuda.get_device_name(dev),
           'arch': getattr(prop, 'gcnArchName', ''), 'compute_units': prop.multi_processor_count, 'torch': torch.__version__,
           'hip': torch.version.hip, 'volume': [B.NX, B.NY, B.NZ], 'detector': [B.DET, B.DET], 'views_per_launch': VIEWS,
           'render': {}, 'expose': {}, 'tools': {}, 'synthesize': {}}
    grid = drr.Grid(-np.linalg.inv(K), B.DET, B.DET)
    views = B.poses(VIEWS)
    att = None
    for name, soft in (('bones', False), ('bones_and_soft_tissue', True)):
        objs = [[drr.Obj(A, m) for A, m in zip(view, drr.DEFAULT_MASKS)] + ([drr.Obj(view[0], (0,))] if soft else []) for view in views]
        a, (att, _, _), keep = drr.render_args(vol, objs, grid, interp='exact', want_plen=False, want_labels=True, tight_boxes=True)
        res['render'][name] = S.per_view(S.measure(lambda a=a: nat.call('dfl_drr_render', a, stream), args.window, args.reps))
        print('render %-24s %.4f ms per view' % (name, res['render'][name]['ms_per_view']), flush=True)
    keys = [synth.noise_keys(0, 0, v) for v in range(VIEWS)]
    for u16 in (True, False):
        a, _, keep = synth.expose_args(att, S.PHOTONS, S.GAIN, S.ESIGMA, 1.0, [q for q, _ in keys], [e for _, e in keys], u16=u16)
        key = 'sigma1/%s' % ('uint16' if u16 else 'float32')
        res['expose'][key] = S.per_view(S.measure(lambda a=a: nat.call('dfl_drr_expose', a, stream), args.window, args.reps))
        print('expose %-24s %.4f ms per view' % (key, res['expose'][key]['ms_per_view']), flush=True)
    work = att.clone()
    for n in (8, 64):
        caps = [capsules(view, n, 100 + v) for v, view in enumerate(views)]
        for cull, want_len in ((True, False), (False, False), (True, True)):
            recs = tools.pack(caps, grid, cull)
            a, _, keep = tools.tools_args(work, grid, recs, want_len)
            key = '%d_capsules/%s%s' % (n, 'culled' if cull else 'whole_image', '/tool_len' if want_len else '')
            case = S.per_view(S.measure(lambda a=a: nat.call('dfl_drr_tools', a, stream), args.window, args.reps))
            rect = recs['rect'].astype(np.int64)
            area = np.clip(rect[..., 2] - rect[..., 0] + 1, 0, None) * np.clip(rect[..., 3] - rect[..., 1] + 1, 0, None)
            case['rect_pixels_per_view'] = int(area.sum() / VIEWS)
            case['rect_share_of_capsule_pixel_pairs'] = round(float(area.sum()) / (VIEWS * n * B.DET * B.DET), 4)
            res['tools'][key] = case
            print('tools %-32s %.4f ms per view (rectangles: %.1f%% of all capsule-pixel pairs)'
                  % (key, case['ms_per_view'], 100 * case['rect_share_of_capsule_pixel_pairs']), flush=True)
            work.copy_(att)
    r = res['render']['bones_and_soft_tissue']['ms_per_view']
    res['tools_over_render'] = {k: round(v['ms_per_view'] / r, 4) for k, v in res['tools'].items()}
    if not args.no_end_to_end:
        with tempfile.TemporaryDirectory() as d:
            src = os.path.join(d, 'phantom.h5')
            hu = (mu / 0.02 * 1000.0 - 1000.0).cpu().numpy()
            S.write_container(src, hu, lab.cpu().numpy(), K)
            del hu
            for n_tools in (0, 8):
                secs = {}
                for n_views in (8, 40):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    synth.synthesize(src, os.path.join(d, 'out.h5'), n_views, seed=1, layout='preprocessed', volumes=False, rot_sigma_deg=3.0,
                                     trans_sigma_mm=(5.0, 5.0, 20.0), chunk=VIEWS, tools=n_tools)
                    secs[n_views] = time.perf_counter() - t0
                per = (secs[40] - secs[8]) / 32.0
                res['synthesize']['tools_%d' % n_tools] = {'seconds_8_views': round(secs[8], 3), 'seconds_40_views': round(secs[40], 3),
                                                           'ms_per_view': round(1e3 * per, 2), 'views_per_second': round(1.0 / per, 1)}
                print('synthesize --tools %d: %.1f views per second (%.2f ms per view)' % (n_tools, 1.0 / per, 1e3 * per), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
