"""Full-resolution overlay entry points without a GPU: the text stamp table and its fraction rule, Pillow's resample
coefficients against the resize fixtures (a numpy two-pass model), the ellipse boxes and text anchors of the host half,
the command line of examples/make_full_res_overlays.py against the reference's (examples_dataset/
make_full_res_overlays.py:28-31), h5lite reading the full-resolution layout, and the refusals: CPU tensors, an unknown
pixel dtype, a radius outside the stamp table, bad arguments at the C ABI."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'examples'))


# ---- text stamps ------------------------------------------------------------------------------------------------------
def test_text_stamp_table_parses():
    from dfl_amd import overlay
    ts = overlay.TextStamps()
    assert ts.strings == {'L. Femur FOV OK': 0, 'R. Femur FOV OK': 1}
    assert len(ts.rules['x']) == 3 and len(ts.rules['y']) == 3
    assert list(ts.rules['x']) == sorted(ts.rules['x']) and list(ts.rules['y']) == sorted(ts.rules['y'])
    assert ts.table.shape == (2 * 4 * 4, 3)
    for i in range(len(ts.table)):
        m = ts.mask(i)
        assert m.shape[0] >= 7 and m.shape[1] >= 70 and m.max() >= 240 and m.min() == 0
    assert int(ts.table[:, 2].max() + ts.table[-1, 0] * ts.table[-1, 1]) <= ts.masks.size
    # the two strings differ in the first glyph only
    a, b = ts.mask(ts.index[(0, 1, 1)][0]), ts.mask(ts.index[(1, 1, 1)][0])
    assert a.shape == b.shape and not np.array_equal(a, b) and np.array_equal(a[:, 12:], b[:, 12:])


def test_text_fraction_rule():
    """Four bins per axis: about (-1, -32.5/64), [-32.5/64, 0], (0, 31.5/64), [31.5/64, 1) in x and about
    (-1, -31.5/64), [-31.5/64, 0], (0, 32.5/64), [32.5/64, 1) in y, boundaries exact in double (the y ones sit a few
    fp32 steps off the 1/128 grid)."""
    from dfl_amd import overlay
    ts = overlay.text_stamps()
    bx = lambda f: ts.bin('x', f)        # noqa: E731
    by = lambda f: ts.bin('y', f)        # noqa: E731
    assert [bx(f) for f in (-0.99, -0.51, -0.5, -1e-9, -0.0, 0.0, 1e-9, 0.49, 0.4921875, 0.99)] == [0, 0, 1, 1, 1, 1, 2, 2, 3, 3]
    assert [by(f) for f in (-0.99, -0.5, -0.4921875, 0.0, 1e-9, 0.507, 0.5078125, 0.99)] == [0, 0, 1, 1, 2, 2, 3, 3]
    # every fp32 neighbour of 31.5 / 64 falls on the side the threshold says
    f = np.float32(31.5 / 64)
    assert bx(float(np.nextafter(f, np.float32(0)))) == 2 and bx(float(f)) == 3
    # placement: int() of the position plus the stamp's offset, the bin of math.modf of each coordinate
    for x, y in ((30.25, 40.75), (-0.5, 3.0), (0.0, 0.0), (118.01, -20.5)):
        left, top, i = ts.place('R. Femur FOV OK', np.float32(x), np.float32(y))
        k, dx, dy = ts.index[(1, bx(math.modf(x)[0]), by(math.modf(y)[0]))]
        assert (left, top, i) == (int(x) + dx, int(y) + dy, k)


# ---- resample ---------------------------------------------------------------------------------------------------------
def model_resize(rgb, size):
    from dfl_amd import overlay
    H, W, _ = rgb.shape
    vb, vc = overlay.pillow_coeffs(H, size[0])
    hb, hc = overlay.pillow_coeffs(W, size[1])
    x = rgb.astype(np.int64)
    t = np.stack([np.clip((2 ** 21 + (x[:, s:s + n] * hc[o, :n, None]).sum(1)) >> 22, 0, 255)
                  for o, (s, n) in enumerate(hb)], 1)
    return np.stack([np.clip((2 ** 21 + (t[s:s + n] * vc[o, :n, None, None]).sum(0)) >> 22, 0, 255)
                     for o, (s, n) in enumerate(vb)], 0).astype(np.uint8)


@pytest.mark.parametrize('name', ['fullres_resize_203_25', 'fullres_resize_200x232_25x29', 'fullres_resize_37x53_up_64x100'])
def test_pillow_coefficients_reproduce_the_resize_fixtures(name):
    z = load_golden(name)
    size = tuple(z['size'].tolist())
    for b in range(z['input'].shape[0]):
        assert np.array_equal(model_resize(z['input'][b], size), z['expected'][b]), (name, b)


def test_resample_plan_for_the_full_resolution_file():
    from dfl_amd import _native as nat, overlay
    assert overlay.fullres_size(1536, 1536) == (192, 192)
    p = overlay.resample_plan((1536, 1536), (192, 192))
    assert p['kh'] == p['kv'] == 17
    assert (p['h_bounds'][:, 1] <= 17).all() and (p['h_bounds'].sum(1) <= 1536).all() and (p['h_bounds'][:, 0] >= 0).all()
    s = p['h_coefs'].sum(1)
    assert (abs(s - 2 ** 22) <= 17).all()
    assert p['span_rows'] <= 8 * 8 + 8 and p['span_cols'] <= 8 * 64 + 8          # about 8 input pixels per output, plus the taps
    assert 4 * (4 * p['span_cols'] + nat.RESAMPLE_TILE_COLS * p['span_rows']) <= nat.RESAMPLE_MAX_LDS
    with pytest.raises(nat.DflError, match='too strongly'):
        overlay.resample_plan((4096, 4096), (8, 8))


# ---- host half of a projection ----------------------------------------------------------------------------------------
def test_marks_follow_the_reference_rules():
    from dfl_amd import overlay
    H, W = 200, 232
    lands = [('A', (5.5, 210.0)),            # y >= H but < W: visible (the reference compares y with the columns)
             ('FH-l', (231.5, 10.25)),       # x in (W-1, W): visible, mirrored to x in (-1, 0)
             ('FH-r', (-0.5, 20.0)),         # invisible
             ('B', (100.0, 232.0))]          # y == W: invisible
    boxes, texts = overlay.fullres_marks(lands, False, (1, 1), H, W)
    assert boxes.shape == (2, 5)
    assert tuple(boxes[1, :4]) == (215, -5, 32, 31)        # trunc(231.5 - 16), trunc(10.25 - 16) == -5 (toward zero)
    assert tuple(texts[1]) == overlay.text_stamps().place('R. Femur FOV OK', 0, 0)          # FH-r not visible -> (0, 0)
    assert tuple(texts[0]) == overlay.text_stamps().place('L. Femur FOV OK', np.float32(231.5), np.float32(10.25))
    boxes, texts = overlay.fullres_marks(lands, True, (1, 0), H, W)
    x, y = np.float32(W - 1) - np.float32(231.5), np.float32(H - 1) - np.float32(10.25)
    assert -1 < x < 0
    assert tuple(texts[0]) == overlay.text_stamps().place('L. Femur FOV OK', x, y)
    assert texts[0][0] == int(x) + overlay.text_stamps().index[(0, 1, overlay.text_stamps().bin('y', math.modf(y)[0]))][1]
    assert tuple(texts[1]) == (-1, -1, -1)


def test_radius_outside_the_stamps_is_refused():
    from dfl_amd import _native as nat, overlay
    with pytest.raises(nat.DflError, match='stamp table'):
        overlay.fullres_marks([('FH-l', (50.0, 50.0))], False, (0, 0), 100, 100, radius=30)


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused():
    from dfl_amd import _native as nat, overlay
    with pytest.raises(nat.DflError, match='GPU'):
        overlay.render_full_res(torch.zeros(1, 16, 16), torch.zeros(1, 16, 16, dtype=torch.uint8), [0], [[]], [(0, 0)])
    with pytest.raises(nat.DflError, match='GPU'):
        overlay.resize_bilinear(torch.zeros(16, 16, 3, dtype=torch.uint8), (2, 2))


def test_c_abi_refuses_bad_arguments():
    from dfl_amd import _native as nat
    L = nat.lib()
    for k, cls in ((21, nat.ResamplePlan), (22, nat.ResampleArgs), (23, nat.FullresArgs)):
        assert L.dfl_sizeof(k) == C.sizeof(cls)
    assert L.dfl_sizeof(999) == -1
    a = nat.FullresArgs()
    assert L.dfl_fullres_overlay(C.addressof(a), None) == -1 and b'required' in L.dfl_last_error()
    a = nat.FullresArgs(image=16, labels=16, rot180=16, boxes=16, n_boxes=16, texts=16, scratch=16, out=16, B=1, H=64, W=64,
                        n_tiles=1, plan=nat.ResamplePlan(h_in=64, w_in=60))
    assert L.dfl_fullres_overlay(C.addressof(a), None) == -1 and b'plan' in L.dfl_last_error()
    a.plan.w_in, a.tile0 = 64, 1
    assert L.dfl_fullres_overlay(C.addressof(a), None) == -1 and b'canvas' in L.dfl_last_error()
    r = nat.ResampleArgs(inp=16, out=16, B=1, plan=nat.ResamplePlan(h_bounds=16, h_coefs=16, v_bounds=16, v_coefs=16,
                                                                   h_in=4096, w_in=4096, h_out=8, w_out=8, kh=1025,
                                                                   kv=1025, span_rows=4096, span_cols=4096))
    assert L.dfl_resample_bilinear_u8(C.addressof(r), None) == -1 and b'LDS' in L.dfl_last_error()


# ---- the example's command line and reader ----------------------------------------------------------------------------
def test_command_line_matches_the_reference(capsys):
    """The reference takes one positional path (sys.argv[1]) and, without it, prints its error and exits 1."""
    import make_full_res_overlays as ex
    assert ex.main([]) == 1
    assert capsys.readouterr().out == 'ERROR: supply path to HDF5 data file as first argument\n'


def write_layout(path, img_dtype=np.float32):
    from dfl_amd import h5lite
    with h5lite.File(path, 'w') as f:
        f['proj-params/num-cols'] = np.int64(6)
        f['proj-params/num-rows'] = np.int64(4)
        for p in range(2):
            g = 'S1/projections/%03d/' % p
            f[g + 'image/pixels'] = (np.arange(24).reshape(4, 6) * (p + 1)).astype(img_dtype)
            f[g + 'gt-seg/pixels'] = np.full((4, 6), p, np.uint8)
            f[g + 'gt-landmarks/FH-r'] = np.array([1.5, 2.25], np.float32)
            f[g + 'gt-landmarks/FH-l'] = np.array([[3.5], [0.75]], np.float32)      # (2, 1)
            f[g + 'rot-180-for-up'] = np.int64(p)
            f[g + 'gt-poses/left-femur-good-fov'] = np.int64(1)
            f[g + 'gt-poses/right-femur-good-fov'] = np.int64(p)


def test_h5lite_reads_the_full_resolution_layout(tmp_path):
    import make_full_res_overlays as ex
    path = str(tmp_path / 'f.h5')
    write_layout(path)
    src = ex.Source(path)
    assert src.children() == ['S1', 'proj-params']
    assert int(src.get('proj-params/num-cols')) == 6 and int(src.get('proj-params/num-rows')) == 4
    assert src.children('S1/projections') == ['000', '001']
    img, seg, lands, rot, fov = ex.read_projection(src, 'S1/projections/001/')
    assert img.dtype == np.float32 and np.array_equal(img, np.arange(24).reshape(4, 6) * 2)
    assert seg.dtype == np.uint8 and (seg == 1).all()
    assert [n for n, _ in lands] == ['FH-l', 'FH-r']                        # sorted, as h5py iterates
    assert np.array_equal(lands[0][1], [3.5, 0.75]) and np.array_equal(lands[1][1], [1.5, 2.25])
    assert rot is True and fov == (True, True)
    assert ex.read_projection(src, 'S1/projections/000/')[3:] == (False, (True, False))
    src.close()
    # the same names in an .npz
    npz = str(tmp_path / 'f.npz')
    np.savez(npz, **{'proj-params/num-cols': 6, 'S1/projections/000/image/pixels': np.zeros((4, 6), np.float64),
                     'S1/projections/000/gt-landmarks/FH-l': np.zeros(2, np.float32)})
    z = ex.Source(npz)
    assert z.children() == ['S1', 'proj-params'] and z.children('S1/projections/000') == ['gt-landmarks', 'image']


def test_unknown_pixel_dtype_is_refused(tmp_path):
    import make_full_res_overlays as ex
    from dfl_amd import _native as nat
    path = str(tmp_path / 'f.h5')
    write_layout(path, img_dtype=np.uint16)
    with pytest.raises(nat.DflError, match='uint16'):
        ex.read_projection(ex.Source(path), 'S1/projections/000/')
    write_layout(str(tmp_path / 'g.h5'), img_dtype=np.float64)
    img = ex.read_projection(ex.Source(str(tmp_path / 'g.h5')), 'S1/projections/000/')[0]
    assert img.dtype == np.float32
