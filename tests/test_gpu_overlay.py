"""dfl_overlay_batch on the GPU: bit-identical to the overlays of the reference's scripts as restated with torch + Pillow
12.2 (tests/golden/overlay_*.npz, tools/gen_overlay_golden.py), the kernel's ellipses against every reachable Pillow stamp,
batching and the make_grid canvas, then overlay_est_ann.py / overlay_est_heat.py / examples/make_preproc_overlays.py end
to end on a container in the reference's layout, and a 1536^2 x 64 batch (timing printed, not asserted)."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden
from test_gpu_entrypoints import make_file, LAND_NAMES, H, W, L, NC

pytestmark = pytest.mark.gpu

FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, 'overlay_*.npz'))
                  if not p.endswith('overlay_stamps.npz'))


def render_fixture(z, **kw):
    from dfl_amd import overlay
    dev = torch.device('cuda')
    t = {k: torch.from_numpy(z[k]).to(dev) for k in ('images', 'segs', 'heats', 'gt_lands', 'est_lands') if k in z}
    args = dict(segs=t.get('segs'), num_classes=int(z['num_classes']), heats=t.get('heats'), gt_lands=t.get('gt_lands'),
                radius=float(z['radius']), est_lands=t.get('est_lands'), cross=int(z['cross']),
                colors=[tuple(c) for c in z['colors'].tolist()], grid=bool(z['grid']))
    args.update(kw)
    return overlay.render(t['images'], **args).cpu().numpy()


def test_fixture_list():
    assert len(FIXTURES) == 12, FIXTURES


@pytest.mark.parametrize('name', FIXTURES)
def test_render_is_bit_identical_to_the_reference(name):
    z = load_golden(name)
    got = render_fixture(z)
    exp = z['expected']
    assert got.shape == exp.shape and got.dtype == np.uint8
    bad = np.argwhere(got != exp)
    assert bad.size == 0, (name, len(bad), bad[:8].tolist())


def test_kernel_ellipse_matches_every_reachable_pillow_stamp():
    """Box (w, h) with |w - h| <= 1 from a circle of radius max(w, h) / 2: the long side's centre at 2 + r (box from 2),
    the short side's at r - 0.5 (truncation toward zero puts the box at 0 .. 2r - 1).  A black image (constant) shows the
    stamp alone."""
    from dfl_amd import overlay
    z = load_golden('overlay_stamps')
    S = 48
    by_r = {}
    for (w, h), st in zip(z['boxes'].tolist(), z['stamps']):
        if abs(w - h) <= 1:
            by_r.setdefault(max(w, h) / 2.0, []).append((w, h, st))
    n = 0
    for r, items in sorted(by_r.items()):
        gt = np.zeros((len(items), 1, 2), np.float32)
        exp = np.zeros((len(items), S, S, 3), np.uint8)
        for k, (w, h, st) in enumerate(items):
            ox, oy = (2, 2) if w == h else ((2, 0) if w > h else (0, 2))
            gt[k, 0, 0] = 2 + r if ox == 2 else r - 0.5
            gt[k, 0, 1] = 2 + r if oy == 2 else r - 0.5
            m = st[:h + 1, :w + 1].astype(bool)
            exp[k, oy:oy + h + 1, ox:ox + w + 1][m] = (255, 255, 0)
        imgs = torch.zeros((len(items), S, S), device='cuda')
        got = overlay.render(imgs, gt_lands=torch.from_numpy(gt).cuda(), radius=r).cpu().numpy()
        for k, (w, h, _) in enumerate(items):
            assert np.array_equal(got[k], exp[k]), (w, h)
            n += 1
    assert n >= 100


def test_batch_of_11_equals_single_renders_and_the_grid():
    from dfl_amd import overlay
    z = load_golden('overlay_grid_48x11')
    tiles = render_fixture(z, grid=False)
    assert tiles.shape == (11, 48, 48, 3)
    for b in range(11):
        one = {k: z[k][b:b + 1] for k in ('images', 'segs', 'gt_lands')}
        one.update({k: z[k] for k in ('num_classes', 'radius', 'cross', 'colors')})
        one['grid'] = np.int32(0)
        assert np.array_equal(render_fixture(one)[0], tiles[b]), b
    canvas = render_fixture(z)
    assert canvas.shape == overlay.grid_shape(11, 48, 48) + (3,)
    assert np.array_equal(canvas, z['expected'])
    for b in range(11):
        y, x = (b // 8) * 50 + 2, (b % 8) * 50 + 2
        assert np.array_equal(canvas[y:y + 48, x:x + 48], tiles[b])
    # padding and the empty tiles of the second row are zero; a single image has no padding
    mask = np.ones(canvas.shape[:2], bool)
    for b in range(11):
        y, x = (b // 8) * 50 + 2, (b % 8) * 50 + 2
        mask[y:y + 48, x:x + 48] = False
    assert not canvas[mask].any()
    one = {k: z[k][:1] for k in ('images', 'segs', 'gt_lands')}
    one.update({k: z[k] for k in ('num_classes', 'radius', 'cross', 'colors')})
    one['grid'] = np.int32(1)
    assert np.array_equal(render_fixture(one), tiles[0])


def run(script, args, cwd):
    p = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    return p.stdout


def test_scripts_end_to_end(tmp_path):
    """A container in the reference's layout, an output file with nn-segs / nn-heats, est_lands_csv.py for the CSV, then
    the reference README's two overlay commands, the other flag combinations and the preproc example; every PNG equals
    render() on the same inputs."""
    import overlay_est_ann
    from dfl_amd import dataset, overlay, png
    cwd = str(tmp_path)
    make_file(os.path.join(cwd, 'data.npz'))
    make_file(os.path.join(cwd, 'data.h5'))
    gt = np.load(os.path.join(cwd, 'data.npz'))
    pat, n = 1, 8
    Y, X = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing='ij')
    heats = np.zeros((n, L, H, W), np.float32)
    for i in range(n):
        for l in range(L):
            cx, cy = gt['01/lands'][i, :, l]
            heats[i, l] = np.exp(-((X - cx) ** 2 + (Y - cy) ** 2) / np.float32(2 * 2.5 ** 2)) * np.float32(0.3)
    out = {'nn-segs': gt['01/segs'], 'nn-heats': heats, 'land-names/num-lands': np.int64(L)}
    for l, name in enumerate(LAND_NAMES):
        out['land-names/land-%02d' % l] = np.array(name)
    np.savez(os.path.join(cwd, 'out.npz'), **out)
    run('est_lands_csv.py', ['out.npz', 'nn-heats', '--use-seg', 'nn-segs', '--pat', '1', '--out', 'lands.csv'], cwd)
    proj = 3
    est = overlay_est_ann.est_lands_from_csv(os.path.join(cwd, 'lands.csv'), pat, proj)
    assert len(est) > 0

    dev = torch.device('cuda')
    item = dataset.get_dataset(os.path.join(cwd, 'data.npz'), [pat], num_classes=NC, device=dev)[proj]
    seg = torch.from_numpy(gt['01/segs'][proj:proj + 1]).to(dev)
    gtl = item[2].t().unsqueeze(0).contiguous()
    est_t = torch.tensor([list(v) for v in est.values()], dtype=torch.int32, device=dev).view(1, -1, 2)
    none = torch.empty((1, 0, 2), device=dev)
    cases = {
        'readme.png': (['--lands', '--no-gt-lands', '--lands-csv', 'lands.csv'], dict(segs=seg, gt_lands=none, est_lands=est_t)),
        'all.png': (['--lands', '--lands-csv', 'lands.csv'], dict(segs=seg, gt_lands=gtl, est_lands=est_t)),
        'seg.png': ([], dict(segs=seg)),
        'noseg.png': (['--no-seg', '--lands', '--lands-csv', 'lands.csv'], dict(gt_lands=gtl, est_lands=est_t)),
    }
    for png_name, (flags, kw) in cases.items():
        run('overlay_est_ann.py', ['data.npz', 'out.npz', 'nn-segs', str(pat), str(proj), png_name, '--num-classes', str(NC)]
            + flags, cwd)
        want = overlay.render(item[0], num_classes=NC, **kw)[0].cpu().numpy()
        assert np.array_equal(png.read(os.path.join(cwd, png_name)), want), png_name
    for land in (0, 1):
        run('overlay_est_heat.py', ['data.npz', 'out.npz', 'nn-heats', str(pat), str(proj), str(land), 'heat.png'], cwd)
        want = overlay.render(item[0], heats=torch.from_numpy(heats[proj, land][None]).to(dev))[0].cpu().numpy()
        assert np.array_equal(png.read(os.path.join(cwd, 'heat.png')), want), land
    # the preproc example on the HDF5 form of the same container: one canvas per specimen group
    run(os.path.join('examples', 'make_preproc_overlays.py'), ['data.h5'], cwd)
    for g, n_g in (('01', 8), ('02', 4)):
        projs = gt[g + '/projs']
        lands = gt[g + '/lands'].transpose(0, 2, 1).copy()
        x, y = lands[..., 0], lands[..., 1]
        lands[~((x >= 0) & (y >= 0) & (x < W) & (y < W))] = np.nan
        want = overlay.render(torch.from_numpy(projs).to(dev), segs=torch.from_numpy(gt[g + '/segs']).to(dev), num_classes=7,
                              gt_lands=torch.from_numpy(lands).to(dev), radius=3.0, colors=overlay.ANN_COLORS[:6],
                              grid=True).cpu().numpy()
        got = png.read(os.path.join(cwd, g + '.png'))
        assert got.shape == overlay.grid_shape(n_g, H, W) + (3,)
        assert np.array_equal(got, want), g
    assert not os.path.exists(os.path.join(cwd, 'land-names.png'))


def test_full_size_batch_runs_and_is_timed():
    """1536^2 x 64 with labels and 14 ellipse markers per image (the preproc example at full resolution) plus the host
    PNG encode of one tile; times printed, not asserted."""
    import time
    from dfl_amd import overlay, png
    B, S, Lm = 64, 1536, 14
    g = torch.Generator(device='cuda').manual_seed(0)
    imgs = torch.rand((B, S, S), device='cuda', generator=g)
    segs = (torch.rand((B, S, S), device='cuda', generator=g) * 8).to(torch.uint8)
    lands = torch.rand((B, Lm, 2), device='cuda', generator=g) * S
    for grid in (False, True):
        out = overlay.render(imgs, segs=segs, gt_lands=lands, radius=16.0, grid=grid)       # warm-up
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            out = overlay.render(imgs, segs=segs, gt_lands=lands, radius=16.0, grid=grid)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 5
        print('overlay 1536^2 x 64 grid=%d: %.3f ms per render (%.0f GB/s at 12 B per pixel)'
              % (grid, ms, 12.0 * B * S * S / ms / 1e6))
    assert out.shape == overlay.grid_shape(B, S, S) + (3,)
    assert int(out[2:2 + S, 2:2 + S].float().mean().item() > 0)
    tile = out[2:2 + S, 2:2 + S].cpu().numpy()
    t0 = time.time()
    png.encode(tile)
    print('host PNG encode of one 1536^2 tile: %.1f ms' % ((time.time() - t0) * 1e3))
