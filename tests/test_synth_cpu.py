"""dfl_amd.synth without a GPU: the sampled poses (rigid common motion, articulation about the femoral head, the requested
sigmas, seeds, the bounded rejection), the noise keys, the blur taps, the ctypes mirror of dfl_expose_args, the
refusals at the C ABI that need no device, the command line and the committed floors of the detector model."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import drr_ref as D  # noqa: E402
import expose_floor as FL  # noqa: E402
import expose_ref as X  # noqa: E402
import dfl_amd  # noqa: E402
from dfl_amd import _native as nat, drr, preprocess as pp, synth  # noqa: E402

ROWS, COLS, CROP = 45, 61, 2


def _scene():
    """(K, E, {pose name: P}, {landmark name: xyz}) of the tilted scene: six landmarks at the ellipsoids' centres."""
    S = D.scene('tilted')
    poses = dict(zip(drr.POSES, S['poses']))
    lands = {n: (S['I2P'] @ np.array(c + (1.0,)))[:3] for n, (c, _, _) in zip(pp.LAND_ORDER[:6], D.ELLIPSOIDS)}
    return S['K'], S['E'], poses, lands


def test_the_common_motion_is_rigid():
    K, E, poses, lands = _scene()
    rng = np.random.default_rng(5)
    for _ in range(5):
        m = synth.draw_motion(rng, 10.0, (20.0, 20.0, 50.0), 0.0)
        assert not m['femur_deg'].any()
        new = synth.apply_motion(poses, E, lands, m)
        for f in drr.POSES[1:]:
            assert np.abs(new[f] @ np.linalg.inv(new[drr.POSES[0]]) - poses[f] @ np.linalg.inv(poses[drr.POSES[0]])).max() <= 1e-12
        assert np.abs(new[drr.POSES[0]] - poses[drr.POSES[0]]).max() > 1e-3
        Rm = new[drr.POSES[0]][:3, :3]
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(Rm) - 1) <= 1e-12
    # the translation is drawn in the camera frame: the landmarks' centroid moves by t_c there
    m = dict(rot_deg=np.array([4.0, -7.0, 9.0]), trans_mm=np.array([3.0, -2.0, 11.0]), femur_deg=np.zeros((2, 3)))
    new = synth.apply_motion(poses, E, lands, m)
    ctr = np.append(np.mean(list(lands.values()), 0), 1.0)
    before, after = (E @ np.linalg.inv(P[drr.POSES[0]]) @ ctr for P in (poses, new))
    assert np.abs((after - before)[:3] - m['trans_mm']).max() <= 1e-9


def test_articulation_turns_a_femur_about_its_head():
    K, E, poses, lands = _scene()
    m = dict(rot_deg=np.array([3.0, 1.0, -2.0]), trans_mm=np.array([1.0, 2.0, -5.0]), femur_deg=np.array([[5.0, -8.0, 3.0], [-4.0, 6.0, 7.0]]))
    still = synth.apply_motion(poses, E, lands, dict(m, femur_deg=np.zeros((2, 3))))
    new = synth.apply_motion(poses, E, lands, m)
    assert np.array_equal(new[drr.POSES[0]], still[drr.POSES[0]])                   # the pelvis pose is untouched
    for side, name in enumerate(('FH-l', 'FH-r')):
        f = drr.POSES[1 + side]
        head = np.append(lands[name], 1.0)
        assert np.abs(np.linalg.inv(new[f]) @ head - np.linalg.inv(still[f]) @ head).max() <= 1e-9
        assert np.abs(new[f] - still[f]).max() > 1e-3
        other = np.append(lands['GSN-l'], 1.0)
        assert np.abs(np.linalg.inv(new[f]) @ other - np.linalg.inv(still[f]) @ other).max() > 0.1
    # a specimen without the landmark gets no articulation for that femur
    less = {k: v for k, v in lands.items() if k != 'FH-r'}
    part = synth.apply_motion(poses, E, less, m)
    part_still = synth.apply_motion(poses, E, less, dict(m, femur_deg=np.zeros((2, 3))))
    assert np.array_equal(part[drr.POSES[2]], part_still[drr.POSES[2]]) and not np.array_equal(part[drr.POSES[1]], part_still[drr.POSES[1]])


def test_sample_standard_deviations():
    rng = np.random.default_rng(11)
    n = 2000
    draws = [synth.draw_motion(rng, 10.0, (20.0, 20.0, 50.0), 5.0) for _ in range(n)]
    cols = [(np.array([d['rot_deg'][a] for d in draws]), 10.0) for a in range(3)]
    cols += [(np.array([d['trans_mm'][a] for d in draws]), s) for a, s in enumerate((20.0, 20.0, 50.0))]
    cols += [(np.array([d['femur_deg'][sd][a] for d in draws]), 5.0) for sd in range(2) for a in range(3)]
    assert len(cols) == 12
    for x, sigma in cols:
        assert abs(x.std(ddof=1) - sigma) <= 5.0 * sigma / np.sqrt(2.0 * (n - 1))
        assert abs(x.mean()) <= 5.0 * sigma / np.sqrt(n)


KW = dict(rot_sigma_deg=2.0, trans_sigma_mm=(1.0, 1.0, 5.0), femur_sigma_deg=2.0, min_lands=4)


def _plan(seed, views=6, spec=0, **kw):
    K, E, poses, lands = _scene()
    return synth.sample_poses(seed, spec, 'spec-a', [poses, poses], views, K, E, lands, ROWS, COLS, CROP, **dict(KW, **kw))


def test_seeds_repeat_bit_for_bit():
    a, b, c, d = _plan(3), _plan(3), _plan(4), _plan(3, spec=1)
    assert [s for _, s, _ in a] == [0, 1, 0, 1, 0, 1]
    for (pa, _, _), (pb, _, _), (pc, _, _), (pd, _, _) in zip(a, b, c, d):
        for k in drr.POSES:
            assert pa[k].tobytes() == pb[k].tobytes()
            assert not np.array_equal(pa[k], pc[k]) and not np.array_equal(pa[k], pd[k])


def test_rejection_is_bounded_and_names_the_specimen():
    K, E, poses, lands = _scene()
    assert synth.lands_in_window(K, E, poses[drr.POSES[0]], lands, ROWS, COLS, CROP) == 6
    # the same poses seen by a camera that looks away: the landmarks project far outside the detector
    away = D.rot(1, 2.0) @ E
    assert synth.lands_in_window(K, away, poses[drr.POSES[0]], lands, ROWS, COLS, CROP) == 0

    class Counting:
        def __init__(self):
            self.rng, self.calls = np.random.default_rng(0), 0

        def standard_normal(self, n):
            self.calls += 1
            return self.rng.standard_normal(n)

    rng = Counting()
    with pytest.raises(nat.DflError, match='spec-a') as e:
        synth.sample_pose(rng, poses, K, away, lands, ROWS, COLS, CROP, 'spec-a', **KW)
    assert rng.calls == synth.MAX_DRAWS == 20 and 'crop window' in str(e.value)
    rng = Counting()
    new, draws = synth.sample_pose(rng, poses, K, E, lands, ROWS, COLS, CROP, 'spec-a', **KW)
    assert draws == rng.calls == 1
    # a window only some draws reach: accepted poses keep min_lands landmarks inside, rejected draws are counted
    wide = dict(KW, trans_sigma_mm=(6.0, 6.0, 5.0), min_lands=6)
    plan = synth.sample_poses(1, 0, 'spec-a', [poses], 40, K, E, lands, ROWS, COLS, CROP, **wide)
    assert sum(d - 1 for _, _, d in plan) > 0
    for new, _, _ in plan:
        assert synth.lands_in_window(K, E, new[drr.POSES[0]], lands, ROWS, COLS, CROP) == 6
    with pytest.raises(nat.DflError, match='no 3D landmarks'):
        synth.sample_pose(np.random.default_rng(0), poses, K, E, {}, ROWS, COLS, CROP, 'spec-a', **KW)


def test_fov_flags_follow_the_femoral_heads():
    K, E, poses, lands = _scene()
    assert synth.fov_flags(K, E, poses, lands, ROWS, COLS) == (1, 1)
    far = dict(lands)
    far['FH-l'] = lands['FH-l'] + np.array([400.0, 0.0, 0.0])
    assert synth.fov_flags(K, E, poses, far, ROWS, COLS) == (0, 1)
    less = {k: v for k, v in lands.items() if k != 'FH-r'}
    assert synth.fov_flags(K, E, poses, less, ROWS, COLS, seed_flags=(0, 0)) == (1, 0)
    assert synth.fov_flags(K, E, poses, less, ROWS, COLS, seed_flags=(0, 1)) == (1, 1)


def test_noise_keys_are_distinct_and_do_not_depend_on_rejections():
    keys = [k for spec in range(10) for view in range(1000) for k in synth.noise_keys(7, spec, view)]
    assert len(set(keys)) == 20000 and all(0 <= k < 2 ** 64 for k in keys)
    assert synth.noise_keys(7, 3, 5) != synth.noise_keys(8, 3, 5)
    assert synth.noise_keys(7, 3, 5) == synth.noise_keys(7, 3, 5)
    # keys are a function of (seed, specimen, view) alone: a plan with rejected draws and one without share them
    sig = re.search(r'def noise_keys\((.*?)\)', open(os.path.join(ROOT, 'deepfluorolabeling-ipcai2020_amd', 'synth.py')).read()).group(1)
    assert sig == 'seed, specimen, view'


def test_gaussian_taps():
    for sigma, rho in ((0.0, 0), (0.2, 1), (1.0, 3), (2.5, 8), (8.0 / 3.0, 8)):
        w, r = synth.gaussian_taps(sigma)
        assert r == rho and w.dtype == np.float32 and w.size == 2 * rho + 1
        assert abs(float(w.astype(np.float64).sum()) - 1.0) <= (2 * rho + 1) * 2.0 ** -25        # each tap rounded once
        assert np.array_equal(w, w[::-1]) and w.argmax() == rho
        wx, rx = X.taps(sigma)
        assert rx == r and np.array_equal(wx, w)
    assert synth.gaussian_taps(0.0)[0].tolist() == [1.0]
    for bad in (2.7, 3.0, 100.0):
        with pytest.raises(nat.DflError, match='radius'):
            synth.gaussian_taps(bad)
    with pytest.raises(nat.DflError, match='negative'):
        synth.gaussian_taps(-1.0)


def test_struct_mirror_and_symbol():
    L = nat.lib()
    k = nat._SIZEOF_ORDER.index(nat.ExposeArgs)
    assert L.dfl_sizeof(k) == C.sizeof(nat.ExposeArgs) == 160
    assert 'dfl_drr_expose' in nat.EXPORTS and hasattr(L, 'dfl_drr_expose')
    header = open(os.path.join(ROOT, 'include', 'dfl_hip.h')).read()
    assert 'int dfl_drr_expose(const dfl_expose_args* a, dfl_stream_t stream);' in header
    assert '#define DFL_EXPOSE_MAX_RADIUS %d' % nat.EXPOSE_MAX_RADIUS in header and X.MAX_RADIUS == nat.EXPOSE_MAX_RADIUS
    body = header[header.index('#define DFL_EXPOSE_MAX_RADIUS'):header.index('} dfl_expose_args;')]
    names = re.findall(r'(\w+)(?:\[[^\]]*\])?\s*[;,]', re.sub(r'/\*.*?\*/', '', body.split('typedef struct {')[1], flags=re.S))
    assert names == [n for n, _ in nat.ExposeArgs._fields_]
    assert open(os.path.join(ROOT, 'deepfluorolabeling-ipcai2020_amd', 'csrc', 'build.sh')).read().count('expose.hip') >= 2


def test_c_abi_refuses_before_it_launches():
    L = nat.lib()
    P = 4096                                                  # never dereferenced: the checks come first

    def mk(**k):
        return nat.ExposeArgs(**dict(dict(att=P, out=P, key_q=P, key_e=P, rho=3, V=2, R=9, C=11, u16=1, quantum=1, electronic=1,
                                          photons=100.0, gain=1.0, electronic_sigma=1.0), **k))

    for kw, word in ((dict(att=None), b'required'), (dict(out=None), b'required'), (dict(V=0), b'sizes'), (dict(R=0), b'sizes'),
                     (dict(C=0), b'sizes'), (dict(R=46341, C=46341), b'2^31'), (dict(rho=9), b'rho'), (dict(photons=0.0), b'photons'),
                     (dict(gain=0.0), b'gain'), (dict(electronic_sigma=-1.0), b'electronic_sigma'), (dict(key_q=None), b'key_q'),
                     (dict(key_e=None), b'key_e')):
        a = mk(**kw)
        assert L.dfl_drr_expose(C.addressof(a), None) == -1, kw
        assert word in L.dfl_last_error() and b'dfl_drr_expose' in L.dfl_last_error(), (kw, L.dfl_last_error())
    assert L.dfl_drr_expose(None, None) == -1 and b'null' in L.dfl_last_error()


def test_cpu_tensors_and_a_machine_without_a_gpu_are_refused(tmp_path):
    with pytest.raises(nat.DflError, match='GPU'):
        synth.expose(torch.zeros(1, 4, 4))
    with pytest.raises(nat.DflError, match='GPU'):
        synth.expose(np.zeros((1, 4, 4), np.float32))
    with pytest.raises(nat.DflError, match='layout'):
        synth.synthesize('a.h5', 'b.h5', 3, layout='other')
    assert dfl_amd.synth is synth and dfl_amd.synthesize is synth.synthesize
    if not torch.cuda.is_available():
        import synthesize_dataset as cli
        with pytest.raises(nat.DflError, match='no GPU'):
            cli.main([os.path.join(str(tmp_path), 'missing.h5'), os.path.join(str(tmp_path), 'out.h5'), '--views', '2'])
        assert not os.path.exists(os.path.join(str(tmp_path), 'out.h5'))


def test_command_line():
    import synthesize_dataset as cli
    a = cli.parse_args(['full.h5', 'synth.h5'])
    assert (a.src, a.dst, a.views, a.seed, a.layout, a.specimens, a.crop, a.ds_factor) == ('full.h5', 'synth.h5', 200, 0, 'preprocessed', None, 50, 8)
    assert (a.rot_sigma_deg, a.trans_sigma_mm, a.femur_sigma_deg, a.min_lands) == (10.0, (20.0, 20.0, 50.0), 5.0, 4)
    assert (a.photons, a.gain, a.electronic_sigma, a.blur_sigma_px) == tuple(synth.DEFAULTS[k] for k in ('photons', 'gain', 'electronic_sigma', 'blur_sigma_px'))
    assert (a.no_noise, a.bones_only, a.no_volumes, a.chunk, a.gzip) == (False, False, False, 8, False)
    a = cli.parse_args(['full.h5', 'synth.h5', '--views', '7', '--seed', '9', '--layout', 'full-res', '--specimens', 'a,b', '--crop', '10',
                        '--ds-factor', '4', '--rot-sigma-deg', '3', '--trans-sigma-mm', '1,2,3', '--femur-sigma-deg', '0', '--min-lands',
                        '6', '--photons', '1e4', '--gain', '0.5', '--electronic-sigma', '0', '--blur-sigma-px', '0', '--no-noise',
                        '--bones-only', '--no-volumes', '--chunk', '3', '--gzip'])
    assert (a.views, a.seed, a.layout, a.specimens, a.crop, a.ds_factor) == (7, 9, 'full-res', ['a', 'b'], 10, 4)
    assert (a.rot_sigma_deg, a.trans_sigma_mm, a.femur_sigma_deg, a.min_lands) == (3.0, (1.0, 2.0, 3.0), 0.0, 6)
    assert (a.photons, a.gain, a.electronic_sigma, a.blur_sigma_px) == (1e4, 0.5, 0.0, 0.0)
    assert (a.no_noise, a.bones_only, a.no_volumes, a.chunk, a.gzip) == (True, True, True, 3, True)
    for bad in (['full.h5'], ['full.h5', 'synth.h5', '--layout', 'other'], ['full.h5', 'synth.h5', '--trans-sigma-mm', '1,2']):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)


def test_the_model_blurs_what_it_says():
    """The restatement against a direct double loop, and its exact cases."""
    rng = np.random.default_rng(2)
    att = rng.uniform(0, 2, (1, 6, 9)).astype(np.float32)
    w, rho = X.taps(1.0)
    T = np.exp(-att[0].astype(np.float64))
    rows = np.zeros_like(T)
    out = np.zeros_like(T)
    for r in range(6):
        for c in range(9):
            rows[r, c] = sum(float(w[k]) * T[r, min(max(c + k - rho, 0), 8)] for k in range(2 * rho + 1))
    for r in range(6):
        for c in range(9):
            out[r, c] = sum(float(w[k]) * rows[min(max(r + k - rho, 0), 5), c] for k in range(2 * rho + 1))
    got = X.expose(att, w, 100.0, 2.0, 0.0)
    assert np.abs(got[0] - 200.0 * out).max() <= 1e-10
    z = rng.standard_normal((1, 6, 9)).astype(np.float32)
    noisy = X.expose(att, np.ones(1, np.float32), 100.0, 2.0, 3.0, z1=z, z2=-z)
    N, z64 = 100.0 * T, z[0].astype(np.float64)
    assert np.abs(noisy[0] - 2.0 * (N + np.sqrt(N) * z64 - 3.0 * z64)).max() <= 1e-10
    assert np.array_equal(X.expose(att, np.ones(1, np.float32), 100.0, 2.0, 0.0, dtype=np.float32),
                          np.float32(2.0) * (np.float32(100.0) * np.exp(-att)))
    assert X.quantise(np.array([-3.0, 0.5, 1.5, 2.5, 65534.5, 65535.5, 1e9], np.float32)).tolist() == [0, 0, 2, 2, 65534, 65535, 65535]
    for name, shape in (('scene', (3, 45, 61)), ('corner', (3, 5, 7)), ('smooth', (3,) + X.SMOOTH_SIZE)):
        a = X.inputs(name)
        assert a.shape == shape and a.dtype == np.float32 and a.min() >= 0 and np.isfinite(a).all()
    assert (X.inputs('scene') == 0).mean() > 0.2 and X.inputs('corner')[0].max() == X.inputs('scene')[0].max()
    assert X.SMOOTH_SIZE[0] > 3 * X.TILE[0] and X.SMOOTH_SIZE[0] % X.TILE[0] and X.SMOOTH_SIZE[1] > 3 * X.TILE[1] and X.SMOOTH_SIZE[1] % X.TILE[1]
    src = open(os.path.join(ROOT, 'deepfluorolabeling-ipcai2020_amd', 'csrc', 'expose.hip')).read()
    assert 'EX_TH = %d, EX_TW = %d' % X.TILE in src


def test_the_committed_floors_are_the_models():
    """tests/golden/floors/expose.json is what tests/expose_floor.py measures (to the last digits numpy versions may move)."""
    doc = FL.load()
    assert doc['bar_factor'] == FL.BAR_FACTOR == 8.0
    now = FL.measure()
    assert sorted(now) == sorted(doc['floors']) == sorted(X.case_key(*c) for c in X.CASES) and len(now) == 18
    for key, e in now.items():
        for name, v in e.items():
            assert abs(v - doc['floors'][key][name]) <= 0.05 * doc['floors'][key][name], (key, name, v)


def test_the_end_to_end_seed_meets_the_dice_bar_between_the_models():
    """tests/test_gpu_synth.py asks Dice >= 0.99 per class of the float64 model against the rendered labels.  Its seed is
    one at which the float32 model -- the kernel's arithmetic, no kernel involved -- meets that bar with room: near-tie
    pixels in a small class would fail any float32 renderer."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('gpu_synth_consts', os.path.join(ROOT, 'tests', 'test_gpu_synth.py'))
    src = open(spec.origin).read()
    consts = re.search(r"SPEC, CROP, FACTOR, VIEWS, SEED = '([^']+)', (\d+), (\d+), (\d+), (\d+)", src)
    name, crop, views, seed = consts.group(1), int(consts.group(2)), int(consts.group(4)), int(consts.group(5))
    sig = re.search(r"KW = dict\(crop=CROP, factor=FACTOR, rot_sigma_deg=([\d.]+), trans_sigma_mm=\(([\d., ]+)\), femur_sigma_deg=([\d.]+)", src)
    kw = dict(rot_sigma_deg=float(sig.group(1)), trans_sigma_mm=tuple(float(v) for v in sig.group(2).split(',')),
              femur_sigma_deg=float(sig.group(3)))
    S = D.scene('tilted')
    K, E, poses, lands = _scene()
    seeds = [poses, dict(zip(drr.POSES, D.perturbed(S)))]
    Q = -np.linalg.inv(K)
    worst = 1.0
    for new, _, _ in synth.sample_poses(seed, 0, name, seeds, views, K, E, lands, ROWS, COLS, crop, **kw):
        obs = drr.default_objects(E, new, S['I2P'], bones_only=False)
        recs = D.pack([o.c2i for o in obs], [o.mask for o in obs], Q, S['lab'])
        maps = [D.label_map(D.render(S['mu'], S['lab'], recs, Q.astype(np.float32), ROWS, COLS, dtype=dt)[1].astype(np.float64))
                for dt in (np.float64, np.float32)]
        present = [l for l in range(1, 7) if (maps[0] == l).any()]
        assert len(present) >= 4
        for l in present:
            worst = min(worst, 2.0 * ((maps[0] == l) & (maps[1] == l)).sum() / ((maps[0] == l).sum() + (maps[1] == l).sum()))
    assert worst >= 0.995, worst
