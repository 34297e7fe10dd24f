"""dfl_amd.drr without a GPU: the numpy model of tests/drr_ref.py against analytic chords, the sign conventions against
the reference's projection formula, the training grid against preprocess.map_lands, tight boxes, the conditions the
test scenes must meet, the ctypes mirrors against dfl_sizeof, refusals at the C ABI and in Python, and the command
line of examples/full_res_drr.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'examples'))

import drr_floor as FL  # noqa: E402
import drr_ref as D  # noqa: E402
import dfl_amd  # noqa: E402
from dfl_amd import _native as nat, drr, preprocess as pp  # noqa: E402

SCENES = ('tilted', 'aligned')


def _chords(rec, q, H, W):
    """s (t1 - t0) of every ray through the box of one record by the slab method, ray by ray in Python floats."""
    o = [float(v) for v in rec['o']]
    M = [float(v) for v in rec['M']]
    q = [float(v) for v in np.asarray(q, np.float32).reshape(-1)]
    out = np.zeros((H, W))
    for r in range(H):
        for c in range(W):
            s = sum((q[3 * a] * c + q[3 * a + 1] * r + q[3 * a + 2]) ** 2 for a in range(3)) ** 0.5
            t0, t1 = 0.0, float('inf')
            for a in range(3):
                d = M[3 * a] * c + M[3 * a + 1] * r + M[3 * a + 2]
                lo, hi = rec['box_lo'][a] - 0.5, rec['box_hi'][a] + 0.5
                if d == 0:
                    if not lo <= o[a] < hi:
                        t1 = -1.0
                    continue
                ta, tb = (lo - o[a]) / d, (hi - o[a]) / d
                t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
            if t1 > t0:
                out[r, c] = s * (t1 - t0)
    return out


@pytest.mark.parametrize('kind', SCENES)
def test_constant_volume_gives_the_analytic_chord(kind):
    S = D.scene(kind)
    recs = D.pack(D.scene_views(S)[0][:1], [0xffff], S['Q'], S['lab'], tight=True)
    nz, ny, nx = S['lab'].shape
    assert tuple(recs[0]['box_lo']) == (0, 0, 0) and tuple(recs[0]['box_hi']) == (nx - 1, ny - 1, nz - 1)   # bit 0 admits everything
    mu = np.full(S['lab'].shape, 0.0173, np.float32)
    att, plen, _ = D.render(mu, S['lab'], recs, S['Q'].astype(np.float32), S['rows'], S['cols'])
    chord = _chords(recs[0], S['Q'], S['rows'], S['cols'])
    assert chord.max() > 30 and (chord > 0).mean() > 0.5
    assert np.abs(plen.sum(0) - chord).max() <= 1e-9
    assert np.abs(att - float(np.float32(0.0173)) * chord).max() <= 1e-9
    if kind == 'aligned':                                  # the ray with two direction components exactly 0
        m = recs[0]['M'].reshape(3, 3)
        d = m[:, 0] * np.float32(32) + m[:, 1] * np.float32(16) + m[:, 2]                 # in fp32, as the kernel forms it
        assert d.dtype == np.float32 and d[0] == 0 and d[1] == 0 and d[2] != 0
        assert abs(chord[16, 32] - nz * 1.1) <= 1e-4


def _geometry(S, crop=0, factor=1, rot180=False, zoom=1):
    """The scene as a drr.Geometry; zoom = detector pixels per mm (the scene's own detector has 1)."""
    K = np.diag([zoom, zoom, 1.0]) @ S['K']
    G, (H, W) = drr.training_grid(zoom * S['rows'], zoom * S['cols'], crop, factor, rot180)
    poses = dict(zip(drr.POSES, S['poses']))
    return drr.Geometry(K, S['E'], poses, S['I2P'], G, drr.default_objects(S['E'], poses, S['I2P']),
                        drr.Grid(-np.linalg.inv(K) @ G, H, W))


@pytest.mark.parametrize('kind,rot180', [('tilted', False), ('tilted', True), ('aligned', False)])
def test_a_one_voxel_label_lands_where_its_centre_projects(kind, rot180):
    """Pins the sign conventions: project_points is the reference's K (E inv(P) X), the rays are -inv(K) G [c, r, 1].
    Detector pixels of 0.5 mm: a voxel of 0.8 x 0.75 x 1.1 mm at magnification 1.25 covers about 2 x 2 of them, so no voxel
    falls between the rays."""
    S = D.scene(kind)
    geom = _geometry(S, crop=3, factor=1, rot180=rot180, zoom=2)
    H, W = geom.size
    assert (H, W) == (84, 116)
    for vox in ((20, 25, 30), (9, 14, 30), (30, 33, 20), (28, 12, 33)):
        lab = np.zeros_like(S['lab'])
        lab[vox[2], vox[1], vox[0]] = 1
        recs = D.pack([geom.objects[0].c2i], [0x2], geom.grid.Q, lab)
        assert tuple(recs[0]['box_lo']) == vox == tuple(recs[0]['box_hi'])
        _, plen, _ = D.render(S['mu'], lab, recs, geom.grid.Q.astype(np.float32), H, W, n_labels=2)
        lm = D.label_map(plen, 0.01)
        rr, cc = np.nonzero(lm == 1)
        assert 1 <= rr.size <= 16, (vox, rr.size)
        want = drr.project_points(geom, (S['I2P'] @ np.array(vox + (1.0,)))[:3])
        assert want.shape == (2, 1) and 0 <= want[0, 0] <= W - 1 and 0 <= want[1, 0] <= H - 1
        assert abs(cc.mean() - want[0, 0]) <= 1 and abs(rr.mean() - want[1, 0]) <= 1, (vox, cc.mean(), rr.mean(), want)


@pytest.mark.parametrize('rot180', [0, 1])
@pytest.mark.parametrize('R,C,crop,f', [(1536, 1536, 50, 8), (53, 70, 3, 4), (45, 61, 2, 1), (200, 232, 50, 3)])
def test_the_training_grid_inverts_map_lands(R, C, crop, f, rot180):
    G, (H, W) = drr.training_grid(R, C, crop, f, rot180)
    assert (H, W) == pp.out_size(R, C, crop, f)
    out = np.array([[0.0, W - 1.0, 3.0, 0.25], [0.0, H - 1.0, 1.0, 7.5], [1, 1, 1, 1]])       # (column, row, 1)
    det = G @ out
    assert np.array_equal(det[2], np.ones(4))
    back = pp.map_lands(det[:2][None], [rot180], R, C, crop, f)[0]
    assert np.abs(back - out[:2]).max() <= 1e-9
    if f == 1 and not rot180:
        assert np.array_equal(G, [[1, 0, crop], [0, 1, crop], [0, 0, 1]])
    assert np.array_equal(drr.training_grid(R, C)[0], np.eye(3)) and drr.training_grid(R, C)[1] == (R, C)


@pytest.mark.parametrize('kind', SCENES)
def test_model_tight_boxes_change_nothing(kind):
    for view in (0, 1):
        a1, p1, _, r1 = D.model(kind, 'exact', view, tight=True)
        a0, p0, _, r0 = D.model(kind, 'exact', view, tight=False)
        assert (r1['box_hi'] - r1['box_lo'] < r0['box_hi'] - r0['box_lo']).any(1).all()           # every box is tighter
        assert np.abs(a1 - a0).max() <= 1e-9 and np.abs(p1 - p0).max() <= 1e-9


@pytest.mark.parametrize('kind', SCENES)
def test_scene_conditions(kind):
    """What the GPU comparison relies on: every label is seen on enough pixels, many rays miss everything (their outputs
    must be exactly 0), and few pixels sit so close to a tie that the label map may legitimately differ."""
    _, plen_bar = FL.bars(kind, 'exact')
    for view in (0, 1):
        att, plen, _, _ = D.model(kind, 'exact', view)
        for l in range(1, 7):
            assert int((plen[l] >= 1.0).sum()) >= 50, (kind, view, l, int((plen[l] >= 1.0).sum()))
        assert plen[0].max() == 0                             # no default object admits label 0
        assert float((plen.sum(0) == 0).mean()) >= 0.20
        assert np.array_equal(att == 0, plen.sum(0) == 0)
        assert float(D.near_tie(plen, plen_bar).mean()) <= 0.02
        frac = D.model(kind, 'trilinear', view)[2]
        assert float(D.near_integer(frac).mean()) <= 0.005


def test_the_committed_floors_are_the_models():
    """tests/golden/floors/drr.json is what tests/drr_floor.py measures (to the last digits numpy versions may move)."""
    doc = FL.load()
    assert doc['bar_factor'] == FL.BAR_FACTOR == 8.0
    now = FL.measure()
    assert sorted(now) == sorted(doc['floors'])
    for key, e in now.items():
        for name, v in e.items():
            assert abs(v - doc['floors'][key][name]) <= 0.05 * doc['floors'][key][name], (key, name, v)


def test_label_map_rule():
    plen = np.zeros((4, 1, 5))
    plen[1, 0] = [2.0, 0.5, 3.0, 0.0, 1.0]
    plen[2, 0] = [2.0, 0.9, 1.0, 0.0, 0.2]
    plen[3, 0] = [1.0, 0.2, 4.0, 0.0, 0.1]
    plen[0, 0] = 9.0                                          # label 0 never wins
    assert D.label_map(plen, 1.0).tolist() == [[1, 0, 3, 0, 1]]      # a tie goes to the lowest label; below 1 mm: 0
    assert D.near_tie(plen, 0.01).tolist() == [[True, False, False, False, True]]


def test_pack_objects_matches_the_model_and_rounds_to_fp32():
    assert drr.OBJECT_DTYPE == D.OBJECT_DTYPE and drr.OBJECT_DTYPE.itemsize == C.sizeof(nat.DrrObject) == 76
    assert tuple(drr.label_mask(m) for m in drr.DEFAULT_MASKS) == D.MASKS
    S = D.scene('tilted')
    obs = drr.default_objects(S['E'], dict(zip(drr.POSES, S['poses'])), S['I2P'], bones_only=False)
    assert [o.mask for o in obs] == [0x1e, 0x20, 0x40, 0x1]
    for o, A in zip(obs, D.scene_views(S)[0] + D.scene_views(S)[0][:1]):
        assert np.abs(o.c2i - A).max() <= 1e-12
    with pytest.raises(nat.DflError):
        drr.label_mask([16])
    with pytest.raises(nat.DflError):
        drr.Obj(np.eye(4), 1 << 16)


def test_struct_mirrors_match_the_library():
    L = nat.lib()
    for cls in (nat.DrrObject, nat.DrrArgs):
        assert L.dfl_sizeof(nat._SIZEOF_ORDER.index(cls)) == C.sizeof(cls) > 0
    assert nat._SIZEOF_ORDER[-3:] == [nat.DrrObject, nat.DrrArgs, nat.OptimPackArgs]
    assert 'dfl_drr_render' in nat.EXPORTS and hasattr(L, 'dfl_drr_render')
    assert (nat.DRR_EXACT, nat.DRR_TRILINEAR, nat.DRR_MAX_LABELS) == (0, 1, 16)


def test_c_abi_refuses_bad_arguments():
    """Every refusal comes back as -1 with a message, before anything is launched."""
    L = nat.lib()
    P = 4096                                                  # never dereferenced: the checks come first

    def mk(**k):
        return nat.DrrArgs(**dict(dict(mu=P, labels=P, objects=P, att=P, plen=P, label_map=P, nx=8, ny=9, nz=10, H=16, W=20, views=1,
                                       n_obj=3, n_labels=7, interp=0, mapping=0, step_mm=0.5, min_len_mm=1.0), **k))

    for kw, word in ((dict(mu=None), b'required'), (dict(labels=None), b'required'), (dict(objects=None), b'required'),
                     (dict(att=None), b'required'), (dict(n_labels=17), b'n_labels'), (dict(n_labels=0), b'n_labels'),
                     (dict(interp=2), b'interp'), (dict(interp=-1), b'interp'), (dict(step_mm=0.0), b'step_mm'),
                     (dict(step_mm=-0.5), b'step_mm'), (dict(interp=1, step_mm=0.0, plen=None, label_map=None), b'step_mm'),
                     (dict(interp=1), b'exact'), (dict(nx=0), b'sizes'), (dict(views=0), b'sizes'), (dict(n_obj=0), b'sizes'),
                     (dict(nx=2048, ny=2048, nz=512), b'2^31'), (dict(views=65536), b'65535'), (dict(mapping=2), b'mapping'),
                     (dict(min_len_mm=-1.0), b'min_len_mm')):
        a = mk(**kw)
        assert L.dfl_drr_render(C.addressof(a), None) == -1, kw
        assert word in L.dfl_last_error() and b'dfl_drr_render' in L.dfl_last_error(), (kw, L.dfl_last_error())
    assert L.dfl_drr_render(None, None) == -1 and b'null' in L.dfl_last_error()


def test_cpu_tensors_and_wrong_dtypes_are_refused():
    mu, lab = torch.zeros(4, 5, 6), torch.zeros(4, 5, 6, dtype=torch.uint8)
    with pytest.raises(nat.DflError, match='GPU'):
        drr.Volume(mu, lab)
    with pytest.raises(nat.DflError, match='GPU'):
        drr.Volume(mu.numpy(), lab.numpy())
    with pytest.raises(nat.DflError, match='GPU'):
        drr.hu_to_mu(mu)
    with pytest.raises(nat.DflError, match='GPU'):
        dfl_amd.hu_to_mu(mu.numpy())
    with pytest.raises(nat.DflError, match='Volume'):
        drr.render((mu, lab), [drr.Obj(np.eye(4), 2)], drr.Grid(np.eye(3), 4, 4))
    with pytest.raises(nat.DflError):
        drr.Grid(np.eye(3), 0, 4)
    assert dfl_amd.drr is drr


def test_hu_to_mu_model():
    hu = np.array([-2000.0, -1000.0, 0.0, 1000.0], np.float32)
    np.testing.assert_allclose(D.hu_to_mu(hu), [0.0, 0.0, 0.02, 0.04], rtol=1e-7)


def test_command_line(capsys):
    import full_res_drr as cli
    pos, o = cli.parse(['f.h5', '17-1882', '3'])
    assert pos == ['f.h5', '17-1882', '3']
    assert o == {'--out': None, '--crop': 50, '--ds-factor': 8, '--interp': 'exact', '--step': 0.5, '--bones-only': False,
                 '--compare': False}
    pos, o = cli.parse(['f.h5', '--out', 'p', '17-1882', '--crop', '10', '--ds-factor', '4', '3', '--interp', 'trilinear', '--step',
                        '0.25', '--bones-only', '--compare'])
    assert pos == ['f.h5', '17-1882', '3']
    assert (o['--out'], o['--crop'], o['--ds-factor'], o['--interp'], o['--step'], o['--bones-only'], o['--compare']) == \
        ('p', 10, 4, 'trilinear', 0.25, True, True)
    for bad in ([], ['f.h5'], ['f.h5', '17-1882'], ['f.h5', '17-1882', '0', 'extra'], ['f.h5', '17-1882', '0', '--out'],
                ['f.h5', '17-1882', '0', '--interp', 'cubic'], ['f.h5', '17-1882', '0', '--what'],
                ['f.h5', '17-1882', '0', '--crop', 'x']):
        assert cli.main(bad) == 1, bad
        out = capsys.readouterr().out
        assert out.startswith('Usage: ') and '<HDF5 full-res data file> <specimen ID> <projection index>' in out
    assert cli.to_u8(np.full((3, 4), 2.5)).tolist() == [[0] * 4] * 3                 # a constant image comes out as 0
    assert cli.to_u8(np.array([[0.0, 1.0, 2.0]])).tolist() == [[0, 127, 255]]
