"""dfl_amd.synth.synthesize with tools, end to end on the GPU, on the tilted-scene container of tests/test_gpu_synth.py
(its helpers are imported): views = 5, crop = 2.  Everything is bit for bit: tools = 0 writes the file of a call without
the argument; with tools the labels, landmarks and poses do not move, the image changes exactly under the written mask,
and there it is the detector model of a fresh render plus add_tools of the written capsules.
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
import test_gpu_synth as GS  # noqa: E402
import dfl_amd  # noqa: E402,F401
from dfl_amd import dataset, drr, fullres, preprocess as pp, synth, tools  # noqa: E402
from dfl_amd.fullres import Source  # noqa: E402

pytestmark = pytest.mark.gpu

DEV, SPEC, VIEWS, SEED, KW = GS.DEV, GS.SPEC, GS.VIEWS, GS.SEED, GS.KW
QUIET = dict(KW, blur_sigma_px=0.0)                      # with noise=False: gain photons exp(-att), rounded
TOOLS = 4
OPTIONS = dict(anchor_sigma_mm=8.0, length_mm=(20.0, 80.0))     # the scene's field of view is 36 x 49 mm at the landmarks' depth


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    d = str(tmp_path_factory.mktemp('synth_tools'))
    paths = {k: os.path.join(d, k + '.h5') for k in ('src', 'plain', 'zero', 'pre_plain', 'pre_zero', 'quiet', 'quiet_tools', 'noisy', 'noisy_again',
                                                     'noisy_other', 'pre_tools', 'converted')}
    GS._write_source(paths['src'])
    assert VIEWS == 5 and KW['crop'] == 2
    full = dict(layout='full-res', **KW)
    synth.synthesize(paths['src'], paths['plain'], VIEWS, seed=SEED, **full)
    synth.synthesize(paths['src'], paths['zero'], VIEWS, seed=SEED, tools=0, tool_options=dict(tool_mu=0.9), **full)
    synth.synthesize(paths['src'], paths['pre_plain'], VIEWS, seed=SEED, layout='preprocessed', **KW)
    synth.synthesize(paths['src'], paths['pre_zero'], VIEWS, seed=SEED, layout='preprocessed', tools=0, tool_mask=True, **KW)
    synth.synthesize(paths['src'], paths['quiet'], VIEWS, seed=SEED, layout='full-res', noise=False, **QUIET)
    synth.synthesize(paths['src'], paths['quiet_tools'], VIEWS, seed=SEED, layout='full-res', noise=False, tools=TOOLS, tool_options=OPTIONS, tool_mask=True, **QUIET)
    synth.synthesize(paths['src'], paths['noisy'], VIEWS, seed=SEED, tools=TOOLS, tool_options=OPTIONS, tool_mask=True, **full)
    return paths


def test_tools_zero_writes_the_file_of_a_call_without_the_argument(files):
    a, b = GS._all(files['plain']), GS._all(files['zero'])
    assert sorted(a) == sorted(b) and GS._same(a, b) and not any('tools' in k for k in b)
    assert open(files['plain'], 'rb').read() == open(files['zero'], 'rb').read()
    assert open(files['pre_plain'], 'rb').read() == open(files['pre_zero'], 'rb').read()


def _capsules(got, n):
    key = SPEC + '/projections/%03d/tools/capsules' % n
    return [tools.Capsule.from_row(row) for row in got[key]] if key in got else []


def test_tools_change_the_image_under_the_mask_and_nothing_else(files):
    clean, got = GS._all(files['quiet']), GS._all(files['quiet_tools'])
    extra = sorted(set(got) - set(clean))
    assert not set(clean) - set(got) and all('/tools/' in k for k in extra)
    # labels, landmarks, poses and flags: those of the run without tools
    same = [k for k in clean if not k.endswith('image/pixels')]
    assert len(same) > 10 * VIEWS and all(np.asarray(clean[k]).tobytes() == np.asarray(got[k]).tobytes() for k in same)
    src = Source(files['quiet_tools'])
    # the volume as synthesize reads it from the file: drr.hu_to_mu on the device (test_gpu_synth's own volume rounds mu on the
    # host, one ulp apart in places, which moves a count or two per image whatever the tools do)
    volume = drr.read_volume(src, SPEC, DEV, cast_labels=True)
    with_caps = masked = 0
    for n in range(VIEWS):
        pfx = SPEC + '/projections/%03d/' % n
        caps = _capsules(got, n)
        mask = got[pfx + 'tools/mask/pixels']
        img, before = got[pfx + 'image/pixels'], clean[pfx + 'image/pixels']
        assert mask.dtype == np.uint8 and mask.shape == img.shape and set(np.unique(mask)) <= {0, 1}
        if caps:
            rows = got[pfx + 'tools/capsules']
            assert rows.dtype == np.float64 and rows.shape == (len(caps), 8) and 1 <= len(caps) <= TOOLS
            # the written capsules are the view's own stream
            want = tools.sample_tools(synth.tool_rng(SEED, 0, n), tools.lands_in_camera(
                fullres.proj_params(src)[1], got[pfx + 'gt-poses/' + drr.POSES[0]], fullres.volume_landmarks(src, SPEC)), TOOLS, **OPTIONS)
            assert len(want) == len(caps) and all(np.array_equal(w.row(), c.row()) for w, c in zip(want, caps))
        else:
            assert (pfx + 'tools/capsules') not in got and not mask.any()
        # the image differs exactly where the mask is 1 ...
        assert np.array_equal(img != before, mask == 1), (n, int((img != before).sum()), int(mask.sum()))
        assert (img[mask == 1] < before[mask == 1]).all()
        # ... and is the detector model of a fresh render plus the written capsules, bit for bit
        geom = drr.geometry(src, SPEC, n, crop=0, factor=1, rot180=False, bones_only=False)
        att, _, lab = drr.render(volume, geom.objects, geom.grid)
        assert np.array_equal(lab.cpu().numpy(), got[pfx + 'gt-seg/pixels'])
        att = att[None].contiguous()
        plain = synth.expose(att, QUIET['photons'], QUIET['gain'], QUIET['electronic_sigma'], 0.0, None, None, u16=True)
        assert np.array_equal(plain[0].cpu().numpy(), before)
        tl = tools.add_tools(att, geom.grid, [caps], want_len=True)
        assert np.array_equal((tl[0] > 0).cpu().numpy().astype(np.uint8), mask)
        again = synth.expose(att, QUIET['photons'], QUIET['gain'], QUIET['electronic_sigma'], 0.0, None, None, u16=True)
        assert np.array_equal(again[0].cpu().numpy(), img)
        with_caps += bool(caps)
        masked += int(mask.sum())
    src.close()
    assert with_caps >= 1 and masked > 0


def test_seeds_and_noise(files):
    kw = dict(layout='full-res', tools=TOOLS, tool_options=OPTIONS, tool_mask=True, **KW)
    synth.synthesize(files['src'], files['noisy_again'], VIEWS, seed=SEED, **dict(kw, chunk=5))
    synth.synthesize(files['src'], files['noisy_other'], VIEWS, seed=SEED + 1, **kw)
    assert open(files['noisy'], 'rb').read() == open(files['noisy_again'], 'rb').read()            # (chunk does not move a bit)
    first, other, quiet = GS._all(files['noisy']), GS._all(files['noisy_other']), GS._all(files['quiet_tools'])
    caps = {k: v for k, v in first.items() if k.endswith('tools/capsules')}
    assert caps and all(np.array_equal(v, quiet[k]) for k, v in caps.items())       # the tools do not depend on the noise
    caps_other = {k: v for k, v in other.items() if k.endswith('tools/capsules')}
    assert caps_other and not any(k in caps_other and np.array_equal(v, caps_other[k]) for k, v in caps.items())
    # the poses are those of the run without tools: the tool stream is apart from the pose stream
    plain = GS._all(files['plain'])
    for k in plain:
        if '/gt-poses/' in k or '/gt-landmarks/' in k or k.endswith('gt-seg/pixels'):
            assert np.asarray(plain[k]).tobytes() == np.asarray(first[k]).tobytes(), k


def test_the_preprocessed_layout_is_the_converted_full_res_file(files):
    synth.synthesize(files['src'], files['pre_tools'], VIEWS, seed=SEED, layout='preprocessed', tools=TOOLS, tool_options=OPTIONS, tool_mask=True, **KW)
    pp.convert_file(files['noisy'], files['converted'], factor=GS.FACTOR, crop=GS.CROP)
    a, b = GS._all(files['converted']), GS._all(files['pre_tools'])
    assert sorted(a) == sorted(b) == sorted(GS._all(files['pre_plain'])) and not any('tools' in k for k in b)
    for k in a:
        assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    plain = GS._all(files['pre_plain'])
    assert not np.array_equal(b['01/projs'], plain['01/projs']) and np.array_equal(b['01/segs'], plain['01/segs']) and np.array_equal(b['01/lands'], plain['01/lands'])
    Ro, Co = pp.out_size(45, 61, GS.CROP, GS.FACTOR)
    ds = dataset.get_dataset(files['pre_tools'], [1], num_classes=7, pad_img_dim=0, device=DEV)
    assert len(ds) == VIEWS
    x, masks, lands, heats = next(iter(ds.batches(VIEWS, shuffle=False)))
    assert tuple(x.shape) == (VIEWS, 1, Ro, Co) and tuple(masks.shape) == (VIEWS, 7, Ro, Co) and bool(torch.isfinite(x).all())
    assert np.array_equal(masks.argmax(1).cpu().numpy(), b['01/segs'])


def test_the_drr_example_adds_the_written_capsules(files, tmp_path, capsys):
    """examples/full_res_drr.py --tools-from on a view that is not turned, on the detector's own grid: att grows exactly
    under the written mask."""
    import full_res_drr as cli
    got = GS._all(files['quiet_tools'])
    n = 2
    pfx = SPEC + '/projections/%03d/' % n
    mask = got[pfx + 'tools/mask/pixels']
    assert int(got[pfx + 'rot-180-for-up']) == 0 and mask.any() and (pfx + 'tools/capsules') in got
    plain, tooled = os.path.join(str(tmp_path), 'plain'), os.path.join(str(tmp_path), 'tooled')
    base = [files['quiet_tools'], SPEC, str(n), '--crop', '0', '--ds-factor', '1']
    assert cli.main(base + ['--out', plain]) == 0
    assert cli.main(base + ['--out', tooled, '--tools-from', files['quiet_tools']]) == 0
    assert '%d capsules from' % len(got[pfx + 'tools/capsules']) in capsys.readouterr().out
    a, b = np.load(plain + '.npz'), np.load(tooled + '.npz')
    assert np.array_equal(b['att'] > a['att'], mask == 1) and np.array_equal((b['att'] != a['att']), mask == 1)
    assert np.array_equal(a['labels'], b['labels']) and np.array_equal(a['labels'], got[pfx + 'gt-seg/pixels'])
    # a projection without capsules, and a file without tools at all: nothing is added
    assert cli.main([files['plain'], SPEC, '0', '--crop', '0', '--ds-factor', '1', '--out', tooled, '--tools-from', files['plain']]) == 0
    assert '0 capsules from' in capsys.readouterr().out
