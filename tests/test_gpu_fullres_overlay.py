"""dfl_fullres_overlay / dfl_resample_bilinear_u8 on the GPU: bit-identical to examples_dataset/make_full_res_overlays.py
as restated with torch + Pillow 12.2 (tests/golden/fullres_*.npz, tools/gen_fullres_overlay_golden.py) -- Pillow's
BILINEAR reduction alone, the L-mask blend of the text, text stamps at fractional / zero / negative starts, whole
overlays and a 19-projection canvas drawn in chunks, the identity reduction against dfl_overlay_batch's canvas -- then
examples/make_full_res_overlays.py end to end on an HDF5
container in the full-resolution layout, and a 1536^2 x 16 batch (timing printed, not asserted)."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden

pytestmark = pytest.mark.gpu

RESIZE = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, 'fullres_resize_*.npz')))
OVERLAYS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, 'fullres_*.npz'))
                  if 'fullres_resize_' not in p and not p.endswith('fullres_blend.npz'))


def same(got, exp, what):
    assert got.shape == exp.shape and got.dtype == np.uint8, (what, got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, (what, len(bad), bad[:8].tolist())


def test_fixture_list():
    assert len(RESIZE) == 5, RESIZE
    assert len(OVERLAYS) == 8, OVERLAYS


@pytest.mark.parametrize('name', RESIZE)
def test_resize_is_bit_identical_to_pillow(name):
    from dfl_amd import overlay
    z = load_golden(name)
    x = torch.from_numpy(z['input']).cuda()
    got = overlay.resize_bilinear(x, tuple(z['size'].tolist()))
    same(got.cpu().numpy(), z['expected'], name)
    one = overlay.resize_bilinear(x[0], tuple(z['size'].tolist()))          # [H, W, 3] form
    same(one.cpu().numpy(), z['expected'][0], name + '[0]')


def render_fixture(z, chunk=None):
    """render_full_res over the fixture's projections, `chunk` (default: the fixture's) images per call, one canvas."""
    from dfl_amd import overlay
    N = z['images'].shape[0]
    chunk = int(z['chunk']) if chunk is None else chunk
    names = z['land_names'].tolist()
    canvas = None
    for c0 in range(0, N, chunk):
        sl = slice(c0, min(c0 + chunk, N))
        lands = [list(zip(names, z['lands'][p])) for p in range(sl.start, sl.stop)]
        fov = [tuple(bool(v) for v in z['fov'][p]) for p in range(sl.start, sl.stop)]
        canvas = overlay.render_full_res(torch.from_numpy(z['images'][sl]).cuda(), torch.from_numpy(z['segs'][sl]).cuda(),
                                         z['rot180'][sl].tolist(), lands, fov, size=tuple(z['size'].tolist()),
                                         canvas=canvas, tile0=c0, n_tiles=N)
    return canvas.cpu().numpy()


@pytest.mark.parametrize('name', OVERLAYS)
def test_overlay_is_bit_identical_to_the_reference(name):
    z = load_golden(name)
    same(render_fixture(z), z['expected'], name)


def test_chunking_does_not_change_the_canvas():
    z = load_golden('fullres_grid19')
    exp = z['expected']
    for chunk in (1, 5, 19):
        same(render_fixture(z, chunk), exp, 'chunk %d' % chunk)


def test_text_blend_matches_pillow_for_every_coverage_and_background():
    """The kernel's blend through a one-stamp text table whose row r has coverage r, over an image whose column c has
    grey level g(c) (all 256 occur), at the identity resample: pixel (r, c) must be Pillow's blend of coverage r over
    g(c) (fullres_blend.npz)."""
    from dfl_amd import _native as nat, overlay
    table = load_golden('fullres_blend')['expected']                  # [coverage, background]
    H, W = 256, 512
    dev = torch.device('cuda')
    img = np.tile((np.arange(W, dtype=np.float32) / np.float32(W - 1))[None], (H, 1))
    grey = ((img[0] - img.min()) / (img.max() - img.min()) * np.float32(255)).astype(np.int32)
    assert sorted(set(grey.tolist())) == list(range(256))
    img_d = torch.from_numpy(img[None]).to(dev)
    seg_d = torch.zeros((1, H, W), dtype=torch.uint8, device=dev)
    small = torch.tensor([0, 0] + [0, 0, 0, -1, -1, -1], dtype=torch.int32, device=dev)   # rot, n_boxes, texts
    boxes = torch.zeros(nat.FULLRES_MAX_BOXES * 5, dtype=torch.int32, device=dev)
    stamps = torch.tensor([[W, H, 0]], dtype=torch.int32, device=dev)
    masks = torch.arange(H, dtype=torch.uint8, device=dev)[:, None].expand(H, W).contiguous()
    _, spans = overlay._stamps_on(dev)
    plan, keep = overlay._plan_on(dev, (H, W), (H, W))
    scratch = torch.empty(nat.OVERLAY_SCRATCH_FLOATS, dtype=torch.float32, device=dev)
    out = torch.full((H, W, 3), 7, dtype=torch.uint8, device=dev)
    a = nat.FullresArgs(image=img_d.data_ptr(), labels=seg_d.data_ptr(), rot180=small.data_ptr(), n_boxes=small[1:].data_ptr(),
                        texts=small[2:].data_ptr(), boxes=boxes.data_ptr(), stamp_spans=spans.data_ptr(),
                        text_stamps=stamps.data_ptr(), text_masks=masks.data_ptr(), scratch=scratch.data_ptr(),
                        out=out.data_ptr(), plan=plan, B=1, H=H, W=W, n_tint=0, tint_scale=0.65, n_text_stamps=1,
                        n_stamp_spans=int(spans.numel()), tile0=0, n_tiles=1)
    nat.call('dfl_fullres_overlay', a, torch.cuda.current_stream().cuda_stream)
    got = out.cpu().numpy()
    exp = table[np.arange(H)[:, None], grey[None, :]]
    same(got, np.repeat(exp[..., None], 3, -1), 'blend')


@pytest.mark.parametrize('rot', [False, True])
def test_identity_reduction_equals_the_batch_overlay(rot):
    """A resample of equal size is the identity for Pillow's coefficients, so without text render_full_res is the
    grid=True canvas of render on the same inputs, byte for byte -- rotated: on the flipped images and labels and the
    landmarks mirrored in fp32 as fullres_marks mirrors them.  9 images of 40 x 72: a full and a partial 64-column
    tile, five row tiles, a second canvas row with seven empty cells; labels 0..7 (7 untinted on both sides); six
    landmarks of radius 2, one within 1 px of the left edge, one within 1 px of the bottom edge, two 1.5 px apart."""
    from dfl_amd import overlay
    B, H, W, L = 9, 40, 72, 6
    rng = np.random.default_rng(11)
    images = rng.standard_normal((B, H, W)).astype(np.float32)
    segs = rng.integers(0, 8, (B, H, W)).astype(np.uint8)
    lands = np.stack([rng.uniform(0, W - 1, (B, L)), rng.uniform(0, H - 1, (B, L))], -1).astype(np.float32)
    lands[:, 0, 0] = rng.uniform(0, 0.99, B)
    lands[:, 1, 1] = H - 1 + rng.uniform(0.01, 0.99, B)
    lands[:, 2] = np.stack([rng.uniform(10, 60, B), rng.uniform(10, 30, B)], -1)
    lands[:, 3] = lands[:, 2] + np.float32([0.9, 1.2])                      # 1.5 px away
    x, y = lands[..., 0], lands[..., 1]
    assert (x >= 0).all() and (x < W).all() and (y >= 0).all() and (y < H).all()
    assert (x[:, 0] < 1).all() and (y[:, 1] > H - 1).all() and sorted(set(segs.ravel().tolist())) == list(range(8))
    img_d, seg_d = torch.from_numpy(images).cuda(), torch.from_numpy(segs).cuda()
    got = overlay.render_full_res(img_d, seg_d, [rot] * B, [[('L%02d' % l, lands[b, l]) for l in range(L)] for b in range(B)],
                                  [(0, 0)] * B, size=(H, W), radius=2)
    if rot:
        img_d, seg_d = torch.flip(img_d, (1, 2)), torch.flip(seg_d, (1, 2))
        lands = np.stack([np.float32(W - 1) - x, np.float32(H - 1) - y], -1)
    want = overlay.render(img_d, segs=seg_d, gt_lands=torch.from_numpy(lands).cuda(), radius=2, grid=True)
    assert want.shape == overlay.grid_shape(B, H, W) + (3,)
    yellow = torch.tensor([255, 255, 0], dtype=torch.uint8, device='cuda')
    assert int((want == yellow).all(-1).sum()) > B * L * 5                  # the ellipses are there
    same(got.cpu().numpy(), want.cpu().numpy(), 'rot180 %d' % rot)


def write_container(path, specs, rows, cols, seed=5):
    """A small file in the full-resolution layout (hdf5_layouts/Readme.md), written by h5lite; returns per specimen
    the arrays render_full_res takes."""
    from dfl_amd import h5lite
    z = load_golden('fullres_grid19')
    names = z['land_names'].tolist()
    rng = np.random.default_rng(seed)
    out = {}
    with h5lite.File(path, 'w') as f:
        f['proj-params/num-cols'] = np.int64(cols)
        f['proj-params/num-rows'] = np.int64(rows)
        for s, (spec, n) in enumerate(specs):
            imgs, segs, rots, lands, fovs = [], [], [], [], []
            for p in range(n):
                k = (s * 7 + p) % z['images'].shape[0]
                img = z['images'][k][:rows, :cols] + np.float32(rng.uniform(-1, 1))
                seg = z['segs'][k][:rows, :cols]
                la = z['lands'][k] * np.float32(cols / z['images'].shape[2])
                rot, fov = int(p % 3 == 1), (int(p % 2 == 0), int(p % 4 < 2))
                g = '%s/projections/%03d/' % (spec, p)
                f.create_dataset(g + 'image/pixels', data=img, chunks=(rows, cols), compression='gzip')
                f.create_dataset(g + 'gt-seg/pixels', data=seg, chunks=(rows, cols), compression='gzip')
                for l, name in enumerate(names):
                    v = la[l].astype(np.float32)
                    f[g + 'gt-landmarks/' + name] = v if (l + s) % 2 == 0 else v.reshape(2, 1)
                f[g + 'rot-180-for-up'] = np.int64(rot)
                f[g + 'gt-poses/left-femur-good-fov'] = np.int64(fov[0])
                f[g + 'gt-poses/right-femur-good-fov'] = np.int64(fov[1])
                imgs.append(img)
                segs.append(seg)
                rots.append(rot)
                lands.append(sorted(zip(names, la)))
                fovs.append(fov)
            out[spec] = (np.stack(imgs), np.stack(segs), rots, lands, fovs)
    return out


def test_make_full_res_overlays_end_to_end(tmp_path):
    """The example on a written container: one PNG per specimen (19 projections: two chunks; 2 projections), equal to
    one render_full_res call over all projections of the specimen."""
    from dfl_amd import overlay, png
    rows, cols = 60, 72
    data = write_container(str(tmp_path / 'full.h5'), [('17-1882', 19), ('18-0725', 2)], rows, cols)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'make_full_res_overlays.py'), 'full.h5'],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(str(tmp_path))) == ['17-1882.png', '18-0725.png', 'full.h5']
    for spec, (imgs, segs, rots, lands, fovs) in data.items():
        want = overlay.render_full_res(torch.from_numpy(imgs).cuda(), torch.from_numpy(segs).cuda(), rots, lands, fovs)
        got = png.read(str(tmp_path / (spec + '.png')))
        assert got.shape == overlay.grid_shape(len(rots), 8, 9) + (3,)
        same(got, want.cpu().numpy(), spec)


@pytest.mark.parametrize('B', [16])
def test_full_size_batch_runs_and_is_timed(B):
    """1536^2 x B with labels, 14 landmarks and both texts per image; time printed, not asserted."""
    from dfl_amd import overlay
    S = 1536
    g = torch.Generator(device='cuda').manual_seed(0)
    imgs = torch.rand((B, S, S), device='cuda', generator=g)
    segs = (torch.rand((B, S, S), device='cuda', generator=g) * 8).to(torch.uint8)
    rng = np.random.default_rng(0)
    lands = [[('FH-l' if l == 0 else 'FH-r' if l == 1 else 'L%02d' % l, rng.uniform(0, S, 2).astype(np.float32))
              for l in range(14)] for _ in range(B)]
    args = (imgs, segs, [b % 2 for b in range(B)], lands, [(1, 1)] * B)
    out = overlay.render_full_res(*args)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        out = overlay.render_full_res(*args)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 5
    print('fullres overlay 1536^2 x %d: %.3f ms per call (%.0f GB/s at 9 B per pixel)' % (B, ms, 9.0 * B * S * S / ms / 1e6))
    assert out.shape == overlay.grid_shape(B, 192, 192) + (3,)
    assert float(out.float().mean()) > 0
