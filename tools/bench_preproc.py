"""Times of the full-resolution preprocessing (dfl_amd.preprocess -> dfl_preproc_projs, dfl_preproc_segs) on one GPU.

64 fp32 projections of 1536 x 1536 with their label maps, resident on the device, crop 50, reduced by 8 and by 2, every
second one rotated.  Timed with device events around back-to-back calls of the C entry points (argument blocks
built once: no host work between launches), after a warm-up, `reps` times, alternating with the baseline; the median
is reported with the spread.  The input (604 MB of pixels) is larger than the last-level cache, so every call reads it
from HBM.  GB/s is over compulsory bytes: the input read once and the output written once.

Baseline, in the same run: the same arithmetic composed from torch operations on the same device -- slice, clamp, log,
flip, avg_pool2d(ceil_mode=True, divisor_override=1) divided by the clipped box sizes.  Nothing earlier exists to
compare against.  Its result is compared with the kernels' before anything is timed.

Every timed window lasts at least --window seconds: the number of calls per window is set from a first timing.

    python tools/bench_preproc.py [--n 64] [--window 0.5] [--reps 5] [--out profiles/preproc_bench.json]
"""
import argparse
import datetime
import json
import os
import socket
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S, CROP = 1536, 50
HBM_PEAK_GBPS = 8000.0          # MI355X HBM3E, specification


def torch_projs(px, rotated, crop, f, counts):
    import torch
    import torch.nn.functional as F
    w = px[:, crop:S - crop, crop:S - crop].clamp(min=1.0)
    v = torch.log(w.amax(dim=(1, 2), keepdim=True)) - torch.log(w)
    v[rotated] = v[rotated].flip(1, 2)
    return F.avg_pool2d(v.unsqueeze(1), f, ceil_mode=True, divisor_override=1).squeeze(1) / counts


def timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--window', type=float, default=0.5, help='seconds of device work per timed window, at least')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'preproc_bench.json'))
    args = ap.parse_args()
    import torch
    from dfl_amd import _native as nat, preprocess as pp
    if not torch.cuda.is_available():
        raise SystemExit('bench_preproc.py needs a GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda', 0)
    N = args.n
    g = torch.Generator(device=dev).manual_seed(0)
    px = torch.rand((N, S, S), device=dev, generator=g) * 30000.0
    px[torch.rand((N, S, S), device=dev, generator=g) < 0.02] = 0.0
    coarse = (torch.rand((N, S // 12, S // 12), device=dev, generator=g) * 7).to(torch.uint8)
    sg = coarse.repeat_interleave(12, 1).repeat_interleave(12, 2).contiguous()
    flags = [b % 2 for b in range(N)]
    rot = torch.tensor(flags, dtype=torch.int32, device=dev)
    rotated = rot.nonzero().squeeze(1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    prop = torch.cuda.get_device_properties(dev)
    res = {'tool': 'tools/bench_preproc.py --n %d --window %g --reps %d (device events around back-to-back calls; median of '
                   'the repetitions)' % (N, args.window, args.reps),
           'date': datetime.date.today().isoformat(), 'host': socket.gethostname(),
           'device': torch.cuda.get_device_name(dev), 'arch': getattr(prop, 'gcnArchName', ''),
           'compute_units': prop.multi_processor_count, 'torch': torch.__version__, 'hip': torch.version.hip,
           'hbm_peak_gbps': HBM_PEAK_GBPS, 'cases': {}}
    for f in (8, 2):
        Ro, Co = pp.out_size(S, S, CROP, f)
        out = torch.empty((N, Ro, Co), dtype=torch.float32, device=dev)
        lab = torch.empty((N, Ro, Co), dtype=torch.uint8, device=dev)
        scratch = torch.empty(N, dtype=torch.int32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        pa = nat.PreprocProjsArgs(pixels=px.data_ptr(), rot180=rot.data_ptr(), out=out.data_ptr(), scratch=scratch.data_ptr(),
                                  N=N, R=S, C=S, crop=CROP, factor=f, u16=0, log=1, min_intensity=1.0)
        sa = nat.PreprocSegsArgs(segs=sg.data_ptr(), rot180=rot.data_ptr(), out=lab.data_ptr(), status=status.data_ptr(),
                                 N=N, R=S, C=S, crop=CROP, factor=f)
        ones = torch.ones((1, 1, S - 2 * CROP, S - 2 * CROP), device=dev)
        counts = torch.nn.functional.avg_pool2d(ones, f, ceil_mode=True, divisor_override=1).squeeze(1)
        run_p = lambda: nat.call('dfl_preproc_projs', pa, stream)              # noqa: E731
        run_s = lambda: nat.call('dfl_preproc_segs', sa, stream)               # noqa: E731
        run_t = lambda: torch_projs(px, rotated, CROP, f, counts)                  # noqa: E731
        run_p()
        run_s()
        diff = float((run_t() - out).abs().max())
        assert diff < 1e-4 and int(status.item()) == 0, diff                    # both sides are fp32: not the parity test
        assert torch.equal(pp.preprocess_segs(sg[:2], flags[:2], CROP, f), lab[:2])
        for fn, it in ((run_p, 3), (run_s, 3), (run_t, 2)):
            timed(fn, it)                                                       # warm-up of every shape that is timed
        runs = {'projs': run_p, 'torch_projs': run_t, 'segs': run_s}
        iters = {k: max(int(1e3 * args.window / timed(fn, 5)) + 1, 5) for k, fn in runs.items()}
        ms = {k: [] for k in runs}
        for _ in range(args.reps):                                              # alternating: one box, one moment
            for k, fn in runs.items():
                ms[k].append(timed(fn, iters[k]))
        pix = N * (S - 2 * CROP) ** 2
        outp = N * Ro * Co
        bytes_p, bytes_s = 4 * pix + 4 * outp, pix + outp
        case = {'output': [Ro, Co], 'max_abs_diff_hip_vs_torch': diff}
        for k, nbytes in (('projs', bytes_p), ('segs', bytes_s), ('torch_projs', bytes_p)):
            m = statistics.median(ms[k])
            case[k] = {'calls_per_window': iters[k], 'ms_per_call': round(m, 4), 'ms_per_projection': round(m / N, 5), 'min_ms': round(min(ms[k]), 4),
                       'max_ms': round(max(ms[k]), 4), 'compulsory_bytes': nbytes, 'gbps': round(nbytes / m / 1e6, 1),
                       'fraction_of_hbm_peak': round(nbytes / m / 1e6 / HBM_PEAK_GBPS, 3)}
        both = statistics.median(ms['projs']) + statistics.median(ms['segs'])
        case['projs_and_segs'] = {'ms_per_projection': round(both / N, 5), 'gbps': round((bytes_p + bytes_s) / both / 1e6, 1)}
        case['speedup_over_torch'] = round(case['torch_projs']['ms_per_call'] / case['projs']['ms_per_call'], 2)
        res['cases']['f%d' % f] = case
        print('f = %d: projections %.4f ms each, %.0f GB/s (%.0f %% of the HBM peak); labels %.4f ms each, %.0f GB/s; torch '
              'composition %.4f ms each: %.1fx' % (f, case['projs']['ms_per_projection'], case['projs']['gbps'],
                                                  100 * case['projs']['fraction_of_hbm_peak'], case['segs']['ms_per_projection'],
                                                  case['segs']['gbps'], case['torch_projs']['ms_per_projection'],
                                                  case['speedup_over_torch']))
        assert case['projs']['ms_per_call'] < case['torch_projs']['ms_per_call'], 'the HIP path must beat the torch composition'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
