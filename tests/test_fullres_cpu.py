"""dfl_amd.fullres without a GPU: one tiny full-resolution container (two specimens of two projections, 8 x 10
detectors, a 4 x 5 x 6 volume, three landmarks of which one specimen lacks 'FH-r') written as .npz and, through h5lite,
as .h5; every reader gives the same values from both.  The specimen order, the two refusals with the caller's prefix,
drr.geometry against matrices composed here by hand, and drr.project against drr.project_points."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import drr_ref as D  # noqa: E402
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, drr, fullres, h5lite, preprocess as pp  # noqa: E402

SPECS = ('s-b', 's-a')                      # written in this order, read back sorted
ROWS, COLS = 8, 10
LANDS = ('FH-l', 'FH-r', 'GSN-l')


def _rigid(rng):
    P = D.rot(0, rng.uniform(-1, 1)) @ D.rot(1, rng.uniform(-1, 1)) @ D.rot(2, rng.uniform(-1, 1))
    P[:3, 3] = rng.uniform(-50, 50, 3)
    return P


def _container():
    rng = np.random.default_rng(7)
    c = {'proj-params/intrinsic': np.array([[-900.0, 0, 4.6], [0, -900.0, 3.3], [0, 0, 1]]), 'proj-params/extrinsic': _rigid(rng),
         'proj-params/num-rows': np.int64(ROWS), 'proj-params/num-cols': np.array([COLS], np.int64)}
    for k, s in enumerate(SPECS):
        for grp, px in ((s + '/vol/', rng.integers(-1000, 1500, (4, 5, 6)).astype(np.int16)),
                        (s + '/vol-seg/image/', rng.integers(0, 7, (4, 5, 6)).astype(np.uint8))):
            c[grp + 'pixels'] = px
            c[grp + 'dir-mat'] = _rigid(rng)[:3, :3]
            c[grp + 'spacing'] = np.array([0.8, 0.75, 1.1]).reshape(3, 1) * (1 + k)
            c[grp + 'origin'] = rng.uniform(-20, 20, 3).astype(np.float32)
        for name in LANDS:
            if not (k == 1 and name == 'FH-r'):
                c['%s/vol-landmarks/%s' % (s, name)] = rng.uniform(-30, 30, (3, 1))
        for p in range(2):
            pfx = '%s/projections/%03d/' % (s, p)
            c[pfx + 'image/pixels'] = rng.integers(0, 60000, (ROWS, COLS)).astype(np.uint16)
            c[pfx + 'gt-seg/pixels'] = rng.integers(0, 7, (ROWS, COLS)).astype(np.uint8)
            c[pfx + 'gt-landmarks/GSN-l'] = rng.uniform(0, 8, (2, 1)).astype(np.float32)
            c[pfx + 'gt-landmarks/FH-l'] = rng.uniform(0, 8, 2)
            for name in drr.POSES:
                c[pfx + 'gt-poses/' + name] = _rigid(rng).astype(np.float32 if p else np.float64)
            c[pfx + 'gt-poses/left-femur-good-fov'] = np.int64(p)
            if k == 0:                                                  # the second specimen has no right flag
                c[pfx + 'gt-poses/right-femur-good-fov'] = np.int64(1 - p)
            c[pfx + 'rot-180-for-up'] = np.int64((p + k) % 2)
    return c


@pytest.fixture(scope='module')
def both(tmp_path_factory):
    d = str(tmp_path_factory.mktemp('fullres'))
    c = _container()
    np.savez(os.path.join(d, 'c.npz'), **c)
    with h5lite.File(os.path.join(d, 'c.h5'), 'w') as f:
        for k, v in c.items():
            f[k] = v
    srcs = fullres.Source(os.path.join(d, 'c.npz')), fullres.Source(os.path.join(d, 'c.h5'))
    yield c, srcs
    for s in srcs:
        s.close()


def _same(a, b):
    """Equal values of equal types, through tuples and dicts; arrays by dtype, shape and bytes."""
    assert type(a) is type(b), (a, b)
    if isinstance(a, dict):
        assert list(a) == list(b)
        for k in a:
            _same(a[k], b[k])
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    else:
        assert a == b


def test_every_reader_gives_the_same_from_npz_and_h5(both):
    c, (z, h) = both
    assert z.children() == h.children() == ['proj-params', 's-a', 's-b']
    _same(fullres.detector_size(z), fullres.detector_size(h))
    _same(fullres.proj_params(z), fullres.proj_params(h))
    K, E, rows, cols = fullres.proj_params(h)
    assert (rows, cols) == (ROWS, COLS) == fullres.detector_size(h) and K.shape == (3, 3) and E.shape == (4, 4) and K.dtype == E.dtype == np.float64
    assert np.array_equal(K, c['proj-params/intrinsic']) and np.array_equal(E, c['proj-params/extrinsic'])
    assert fullres.specimens(z) == fullres.specimens(h) == ['s-a', 's-b']
    assert fullres.specimens(h, ['s-b']) == ['s-b'] and fullres.specimens(z, ('s-b', 's-a')) == ['s-b', 's-a']
    for s in SPECS:
        assert fullres.n_projections(z, s) == fullres.n_projections(h, s) == 2
        _same(fullres.volume_frame(z, s), fullres.volume_frame(h, s))
        _same(fullres.volume_frame(z, s, 'vol-seg/image'), fullres.volume_frame(h, s, 'vol-seg/image'))
        dm, sp, org = fullres.volume_frame(h, s)
        assert dm.shape == (3, 3) and sp.shape == org.shape == (3,) and dm.dtype == sp.dtype == org.dtype == np.float64
        assert np.array_equal(sp, c[s + '/vol/spacing'].reshape(-1)) and np.array_equal(org, c[s + '/vol/origin'].astype(np.float64))
        assert not np.array_equal(dm, fullres.volume_frame(h, s, 'vol-seg/image')[0])
        _same(fullres.volume_landmarks(z, s), fullres.volume_landmarks(h, s))
        lands = fullres.volume_landmarks(h, s)
        assert list(lands) == sorted(n for n in LANDS if s + '/vol-landmarks/' + n in c)
        assert all(v.shape == (3,) and v.dtype == np.float64 and np.array_equal(v, c['%s/vol-landmarks/%s' % (s, n)].reshape(-1))
                   for n, v in lands.items())
        for p in range(2):
            pfx = fullres.projection_prefix(s, p)
            assert pfx == '%s/projections/%03d/' % (s, p) == fullres.projection_prefix(s, str(p))
            _same(fullres.gt_poses(z, pfx), fullres.gt_poses(h, pfx))
            poses = fullres.gt_poses(h, pfx)
            assert tuple(poses) == drr.POSES == fullres.POSES
            assert all(P.shape == (4, 4) and P.dtype == np.float64 and np.array_equal(P, c[pfx + 'gt-poses/' + n]) for n, P in poses.items())
            assert fullres.rot180(z, pfx) is fullres.rot180(h, pfx) is bool(c[pfx + 'rot-180-for-up'])
            _same(fullres.gt_landmarks(z, pfx), fullres.gt_landmarks(h, pfx))
            lands2d = fullres.gt_landmarks(h, pfx)
            assert list(lands2d) == ['FH-l', 'GSN-l'] and all(v.shape == (2,) and v.dtype == np.float64 for v in lands2d.values())
            assert np.array_equal(lands2d['GSN-l'], c[pfx + 'gt-landmarks/GSN-l'].astype(np.float64).reshape(-1))
            _same(fullres.femur_fov(z, pfx, default=0), fullres.femur_fov(h, pfx, default=0))
            assert fullres.femur_fov(h, pfx, default=0) == (p, 1 - p if s == 's-b' else 0)
    assert 'FH-r' in fullres.volume_landmarks(h, 's-b') and 'FH-r' not in fullres.volume_landmarks(h, 's-a')
    assert fullres.femur_fov(h, 's-b/projections/001/') == (1, 0)
    for src in (z, h):
        with pytest.raises(KeyError):
            fullres.femur_fov(src, 's-a/projections/000/')               # no default: the flag is required
    assert fullres.scalar(np.array([[5]])) == 5 and fullres.scalar(3.5) == 3.5 and fullres.scalar(z.get('proj-params/num-cols')) == COLS
    # the open file behind an HDF5 source, for copies of groups as stored; an .npz has none
    assert isinstance(h.h5['s-a/vol'], h5lite.Group) and z.h5 is None


class _Ids:
    def __init__(self, ids):
        self.ids = list(ids)

    def children(self, path=''):
        return sorted(self.ids + ['proj-params'])


def test_specimen_order_and_refusals(both):
    six = list(pp.SPECIMEN_ORDER)
    assert fullres.specimens(_Ids(reversed(six))) == six == fullres.SPECIMEN_ORDER and six != sorted(six)
    assert fullres.specimens(_Ids(six[:5])) == sorted(six[:5])                              # not the six: sorted
    assert fullres.specimens(_Ids(six + ['99-0001'])) == sorted(six + ['99-0001'])
    assert fullres.specimens(_Ids(six), ['18-2800', '17-1882']) == ['18-2800', '17-1882']   # as asked for
    assert pp.specimen_order is fullres.specimen_order and pp.land_order is fullres.land_order and pp.LAND_ORDER is fullres.LAND_ORDER
    _, (z, h) = both
    for src in (z, h):
        with pytest.raises(nat.DflError, match=r'^synth\.synthesize: f\.h5 has no specimen nobody, x$'):
            fullres.specimens(src, ['s-a', 'nobody', 'x'], 'synth.synthesize: f.h5')
        with pytest.raises(nat.DflError, match=r'^preprocess\.convert_file: f\.h5 holds no specimen$'):
            fullres.specimens(src, [], 'preprocess.convert_file: f.h5')
    with pytest.raises(nat.DflError, match=r'^me: empty holds no specimen$'):
        fullres.specimens(_Ids([]), None, 'me: empty')


@pytest.mark.parametrize('crop,factor,rot', [(0, 1, None), (1, 2, None), (1, 3, True), (2, 1, False)])
def test_geometry_is_the_chain_composed_by_hand(both, crop, factor, rot):
    c, srcs = both
    for src in srcs:
        for s in SPECS:
            for p in range(2):
                geom = drr.geometry(src, s, p, crop=crop, factor=factor, rot180=rot, bones_only=False)
                pfx = '%s/projections/%03d/' % (s, p)
                K, E = c['proj-params/intrinsic'].astype(np.float64), c['proj-params/extrinsic'].astype(np.float64)
                I2P = np.eye(4)
                I2P[:3, :3] = c[s + '/vol/dir-mat'].astype(np.float64) * c[s + '/vol/spacing'].astype(np.float64).reshape(1, 3)
                I2P[:3, 3] = c[s + '/vol/origin'].astype(np.float64)
                turned = bool(c[pfx + 'rot-180-for-up']) if rot is None else rot
                f, Rc, Cc, h = factor, ROWS - 2 * crop, COLS - 2 * crop, (factor - 1) / 2.0
                G = np.array([[-f, 0, crop + Cc - 1 - h], [0, -f, crop + Rc - 1 - h], [0, 0, 1]] if turned else
                             [[f, 0, crop + h], [0, f, crop + h], [0, 0, 1]], np.float64)
                assert np.array_equal(geom.K, K) and np.array_equal(geom.E, E) and np.array_equal(geom.I2P, I2P) and np.array_equal(geom.G, G)
                assert geom.size == pp.out_size(ROWS, COLS, crop, factor) == (-(-Rc // f), -(-Cc // f))
                assert np.array_equal(geom.grid.Q, -np.linalg.inv(K) @ G)
                names = drr.POSES + drr.POSES[:1]
                assert [o.mask for o in geom.objects] == [0x1e, 0x20, 0x40, 0x1]
                for o, name in zip(geom.objects, names):
                    P = c[pfx + 'gt-poses/' + name].astype(np.float64)
                    assert np.array_equal(geom.poses[name], P)
                    assert np.array_equal(o.c2i, np.linalg.inv(I2P) @ P @ np.linalg.inv(E))


def test_project_is_project_points_on_the_identity_grid():
    S = D.scene('tilted')
    poses = dict(zip(drr.POSES, S['poses']))
    geom = drr.Geometry(S['K'], S['E'], poses, S['I2P'], np.eye(3), drr.default_objects(S['E'], poses, S['I2P']),
                        drr.Grid(S['Q'], S['rows'], S['cols']))
    X = np.array([(S['I2P'] @ np.array(ctr + (1.0,)))[:3] for ctr, _, _ in D.ELLIPSOIDS])
    got = drr.project(S['K'], S['E'], S['poses'][0], X)
    assert got.shape == (2, 6) and got.dtype == np.float64 and got.tobytes() == drr.project_points(geom, X).tobytes()
    one = drr.project(S['K'], S['E'], S['poses'][0], X[2])                      # a single [3] point: [2, 1]
    assert one.shape == (2, 1) and np.abs(one - got[:, 2:3]).max() <= 1e-9
    cam = (S['E'] @ np.linalg.inv(S['poses'][0])) @ np.append(X[1], 1.0)
    uv = S['K'] @ cam[:3]
    assert np.abs(got[:, 1] - uv[:2] / uv[2]).max() <= 1e-9
