"""Cost of the device-side augmentation (dfl_amd.DeviceAugment + dfl_augment_batch) on one GPU.

1. ms per prepared batch-16 item set (184 x 184 images, loader pad to 192, 7 classes, 14 landmarks -- the paper preset's
   input) by device events: augment=None, prob 0.5 (the reference's rate) and prob 1 (every row augmented).
2. the batch-16 paper-preset training step (bf16s arithmetic, as bench.py) with the batch prepared by the loader each
   step, images/s without and with augmentation, alternated in blocks within the one process.

Prints one JSON line.   python tools/bench_aug.py [--iters 200] [--steps 40] [--rounds 3]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAPER = dict(n_classes=7, depth=6, wf=5, batch_norm=True, padding=True, max_pool=False, num_lands=14, do_res=True,
             block_depth=2)


def make_dataset(dev, n=64, H=184, C=7, L=14):
    from dfl_amd import dataset as D
    g = torch.Generator().manual_seed(7)
    projs = torch.rand(n, 1, H, H, generator=g) * 3000 + 100
    segs = torch.randint(0, C, (n, H, H), generator=g)
    lands = torch.rand(n, 2, L, generator=g) * (H - 1)
    return D.DeviceDataSet(projs, segs, lands, proj_pad_dim=192, num_classes=C, device=dev)


def time_prepare(ds, aug, B, iters):
    ds.augment = aug
    order = list(range(len(ds)))
    batches = [order[(k * B) % len(ds):(k * B) % len(ds) + B] for k in range(len(ds) // B)]
    for k in range(5):
        ds._prepare(batches[k % len(batches)])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(iters):
        ds._prepare(batches[k % len(batches)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batch', type=int, default=16)
    args = ap.parse_args()
    import dfl_amd
    from dfl_amd import _native as nat
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    lib = nat.lib()
    B = args.batch
    ds = make_dataset(dev)
    res = {'batch': B, 'image': 184, 'padded': 192}
    for name, aug in (('prep_ms', None), ('prep_aug_p05_ms', dfl_amd.DeviceAugment(1, prob=0.5)),
                      ('prep_aug_p1_ms', dfl_amd.DeviceAugment(1, prob=1.0))):
        res[name] = round(time_prepare(ds, aug, B, args.iters), 4)

    nat.check(lib.dfl_set_math_mode(4), 'dfl_set_math_mode')       # bf16s, bench.py's default
    torch.manual_seed(1234)
    net = dfl_amd.UNet(**PAPER).to(dev).train()
    crit = dfl_amd.DiceAndHeatMapLoss2D(skip_bg=False, heatmap_wgt=0.5)
    opt = dfl_amd.SGD(net.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4, nesterov=True)
    from dfl_amd.util import _squeeze_heats

    def run(aug, steps):
        ds.augment = aug
        it = iter(())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            b = next(it, None)
            if b is None:
                it = ds.batches(B, shuffle=True, drop_last=True)
                b = next(it)
            x, m, _, h = b
            opt.zero_grad()
            seg, heat = net(x)
            h = _squeeze_heats(h)
            loss = crit((dfl_amd.center_crop(seg, m.shape), dfl_amd.center_crop(heat, h.shape)), (m, h))
            loss.backward()
            opt.step()
        e1.record()
        torch.cuda.synchronize()
        return steps * B / (e0.elapsed_time(e1) / 1000.0)

    aug = dfl_amd.DeviceAugment(1, prob=0.5)
    run(None, 10)
    run(aug, 10)
    plain, augd = [], []
    for r in range(args.rounds):
        plain.append(run(None, args.steps))
        augd.append(run(aug, args.steps))
    res['step_images_per_s'] = [round(v, 1) for v in plain]
    res['step_aug_images_per_s'] = [round(v, 1) for v in augd]
    res['step_aug_cost_pct'] = round(100.0 * (1.0 - (sum(augd) / len(augd)) / (sum(plain) / len(plain))), 2)
    res['prep_aug_p05_extra_ms'] = round(res['prep_aug_p05_ms'] - res['prep_ms'], 4)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
