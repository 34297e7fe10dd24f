"""Overlay entry points without a GPU: the PNG codec (dfl_amd.png), the command lines of overlay_est_ann.py /
overlay_est_heat.py against the reference's (train_test_code/overlay_est_ann.py:26-47, overlay_est_heat.py:24-36), the
CSV selection rule, the ellipse stamp table against the Pillow fixture, and the refusal of CPU tensors / a missing GPU."""
import os
import struct
import sys
import zlib

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, ROOT)

# option -> default, as declared by the reference's parsers; store_true flags default to False
ANN_FLAGS = {'lands': False, 'no_gt_lands': False, 'no_seg': False, 'lands_csv': None, 'num_classes': 7}
ANN_POS = ['ds_path', 'seg_file', 'seg_group', 'pat_ind', 'proj_ind', 'out_overlay']
HEAT_FLAGS = {'num_classes': 7}
HEAT_POS = ['ds_path', 'seg_file', 'seg_group', 'pat_ind', 'proj_ind', 'land_ind', 'out_overlay']


# ---- PNG ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', [(1, 1), (1, 7), (5, 3), (13, 37), (64, 65), (37, 53)])
def test_png_round_trip(tmp_path, H, W):
    from dfl_amd import png
    a = np.random.default_rng(H * 100 + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    p = str(tmp_path / 'x.png')
    png.write(p, a)
    raw = open(p, 'rb').read()
    assert raw[:8] == png.SIGNATURE
    assert struct.unpack('>IIBBBBB', raw[16:29]) == (W, H, 8, 2, 0, 0, 0)
    b = png.read(p)
    assert b.dtype == np.uint8 and b.shape == (H, W, 3) and np.array_equal(a, b)


def _filter_rows(a, types):
    """Encode the rows of [H, W, 3] uint8 with the given PNG filter types (the encoder side of RFC 2083 section 6)."""
    H, W, _ = a.shape
    rows = a.reshape(H, 3 * W).astype(np.int32)
    out = bytearray()
    for y in range(H):
        ft = types[y % len(types)]
        cur = rows[y]
        prev = rows[y - 1] if y > 0 else np.zeros_like(cur)
        left = np.concatenate([np.zeros(3, np.int32), cur[:-3]])
        ul = np.concatenate([np.zeros(3, np.int32), prev[:-3]])
        if ft == 0:
            f = cur
        elif ft == 1:
            f = cur - left
        elif ft == 2:
            f = cur - prev
        elif ft == 3:
            f = cur - (left + prev) // 2
        else:
            p = left + prev - ul
            pa, pb, pc = np.abs(p - left), np.abs(p - prev), np.abs(p - ul)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, ul))
            f = cur - pred
        out.append(ft)
        out += (f & 0xff).astype(np.uint8).tobytes()
    return bytes(out)


def _chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)


@pytest.mark.parametrize('types', [[0], [1], [2], [3], [4], [0, 1, 2, 3, 4]])
def test_png_decodes_every_filter_type(types):
    from dfl_amd import png
    a = np.random.default_rng(len(types) * 7 + types[0]).integers(0, 256, (9, 11, 3), dtype=np.uint8)
    a[3:6] = a[2]                                   # repeated rows and smooth runs, not only noise
    a[:, 4:8] = 200
    body = zlib.compress(_filter_rows(a, types))
    buf = png.SIGNATURE + _chunk(b'IHDR', struct.pack('>IIBBBBB', 11, 9, 8, 2, 0, 0, 0)) + \
        _chunk(b'IDAT', body[:10]) + _chunk(b'IDAT', body[10:]) + _chunk(b'IEND', b'')
    assert np.array_equal(png.decode(buf), a)


def test_png_refuses_what_it_does_not_write():
    from dfl_amd import png
    with pytest.raises(ValueError):
        png.encode(np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError):
        png.encode(np.zeros((4, 4, 3), np.float32))
    gray = png.SIGNATURE + _chunk(b'IHDR', struct.pack('>IIBBBBB', 1, 1, 8, 0, 0, 0, 0)) + \
        _chunk(b'IDAT', zlib.compress(b'\0\0')) + _chunk(b'IEND', b'')
    with pytest.raises(ValueError):
        png.decode(gray)


# ---- command lines ----------------------------------------------------------------------------------------------------
def test_ann_parser_matches_the_reference_flags():
    import overlay_est_ann
    pos = ['d.h5', 'o.h5', 'nn-segs', '1', '3', 'x.png']
    ns = vars(overlay_est_ann.build_parser().parse_args(pos))
    assert [ns.pop(k) for k in ANN_POS] == ['d.h5', 'o.h5', 'nn-segs', 1, 3, 'x.png']
    assert ns == ANN_FLAGS
    a = overlay_est_ann.build_parser().parse_args(pos + ['--lands', '--no-gt-lands', '--no-seg', '--lands-csv', 'l.csv',
                                                         '--num-classes', '4'])
    assert (a.lands, a.no_gt_lands, a.no_seg, a.lands_csv, a.num_classes) == (True, True, True, 'l.csv', 4)


def test_heat_parser_matches_the_reference_flags():
    import overlay_est_heat
    pos = ['d.h5', 'o.h5', 'nn-heats', '1', '3', '0', 'x.png']
    ns = vars(overlay_est_heat.build_parser().parse_args(pos))
    assert [ns.pop(k) for k in HEAT_POS] == ['d.h5', 'o.h5', 'nn-heats', 1, 3, 0, 'x.png']
    assert ns == HEAT_FLAGS


def test_csv_selection_rule(tmp_path):
    import overlay_est_ann
    p = str(tmp_path / 'l.csv')
    with open(p, 'w') as f:
        f.write('pat,proj,land,row,col,time\n')
        f.write('1,3,0,10,20,0.1\n1,3,1,-1,-1,0.1\n1,3,2,5,-1,0.1\n1,3,3,0,0,0.1\n1,2,4,7,8,0.1\n2,3,5,7,8,0.1\n'
                '1,3,6,44,9,0.1\n')
    assert overlay_est_ann.est_lands_from_csv(p, 1, 3) == {0: (20, 10), 3: (0, 0), 6: (9, 44)}
    assert overlay_est_ann.est_lands_from_csv(p, 1, 2) == {4: (8, 7)}
    assert overlay_est_ann.est_lands_from_csv(p, 5, 3) == {}
    with open(p, 'a') as f:
        f.write('1,3,0,11,21,0.1\n')
    with pytest.raises(ValueError):
        overlay_est_ann.est_lands_from_csv(p, 1, 3)


# ---- the stamp table the kernel reads ---------------------------------------------------------------------------------
def test_stamp_table_matches_the_pillow_fixture():
    from dfl_amd import overlay
    from dfl_amd import _native as nat
    index, spans, boxes = overlay.stamp_table()
    z = load_golden('overlay_stamps')
    D = nat.OVERLAY_STAMP_DIM
    for (w, h), st in zip(z['boxes'], z['stamps']):
        off = int(index[w * D + h])
        assert off >= 0, (w, h)
        got = np.zeros_like(st)
        for j in range(h + 1):
            lo, hi = int(spans[off + j]) & 0xffff, int(spans[off + j]) >> 16
            got[j, lo:hi + 1] = 1
        assert np.array_equal(got, st), (w, h)
    # every radius of a 192^2 .. 1536^2 file and of the annotation script is covered
    for r in (2, 3.0, 4.0, 8.0, 16.0, 16 * 400 / 1536.0):
        overlay.check_radius(r)
    assert overlay.grid_shape(11, 48, 48) == (2 * 50 + 2, 8 * 50 + 2)
    assert overlay.grid_shape(3, 37, 53) == (39 + 2, 3 * 55 + 2)
    assert overlay.grid_shape(1, 37, 53) == (37, 53)


# ---- no host path -----------------------------------------------------------------------------------------------------
def test_render_and_scripts_refuse_cpu_tensors_and_a_missing_gpu(tmp_path, monkeypatch):
    from dfl_amd import overlay
    from dfl_amd._native import DflError
    with pytest.raises(DflError):
        overlay.render(torch.zeros(1, 8, 8))
    with pytest.raises(DflError):
        overlay.render(np.zeros((1, 8, 8), np.float32))
    import overlay_est_ann
    import overlay_est_heat
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import make_preproc_overlays
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(DflError):
        overlay_est_ann.main(['d.npz', 'o.npz', 'nn-segs', '1', '0', 'x.png'])
    with pytest.raises(DflError):
        overlay_est_heat.main(['d.npz', 'o.npz', 'nn-heats', '1', '0', '0', 'x.png'])
    with pytest.raises(DflError):
        make_preproc_overlays.main(['d.npz'])
    assert not os.path.exists('x.png')
