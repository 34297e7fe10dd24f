"""dfl_amd.raster on the GPU against the numpy model (tests/raster_ref.py, scenes of tests/raster_scenes.py): primitive
ids and depth bits bit for bit, the counters, both coverage paths, contention on one sample, run-to-run bytes, order
independence, the shading bars (unlit and textured exact, lit within one level of the float64 model), the ball of
tests/golden/viz3d_ball.npz through dfl_amd.mesh, and examples/full_res_3d_viz.py --png end to end.  Every call goes
through buffers pre-filled with a sentinel and fenced by guard bytes that must survive."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'examples'))
import raster_ref as RR  # noqa: E402
import raster_scenes as SC  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 256, 0xA5
LIGHT = dict(ambient=0.15, diffuse=0.85, background=(0.7, 0.8, 1.0))
CASES = sorted(SC.cases())


def gpu_meshes(sc, dev):
    """raster.Mesh of every spec; specs that share a numpy array share the tensor (instances)."""
    from dfl_amd import raster
    cache = {}

    def up(a):
        if a is None:
            return None
        if id(a) not in cache:
            cache[id(a)] = (a, torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        return cache[id(a)][1]

    return [raster.Mesh(up(s['pos']), up(s['tris']), normals=up(s['nrm']), uv=up(s['uv']), rgb=s['rgb'], unlit=s['unlit'],
                        texture=up(s['tex']), matrix=s['matrix']) for s in sc['specs']]


def fenced(nbytes, dev):
    """(the whole allocation, its payload view): sentinel everywhere, GUARD bytes on either side of the payload."""
    whole = torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    return whole, whole[GUARD:GUARD + nbytes]


def gpu_draw(sc, light=LIGHT, meshes=None, view_proj=None):
    """dfl_raster_draw on fenced, sentinel-filled buffers: dict(rgb, ids, depth, counts) as numpy."""
    from dfl_amd import _native as nat, raster
    dev = torch.device('cuda:0')
    meshes = gpu_meshes(sc, dev) if meshes is None else meshes
    view, proj = (sc['view'], sc['proj']) if view_proj is None else view_proj
    arr, _ = raster.records(meshes, view, proj)
    W, H, s = sc['W'], sc['H'], sc['ssaa']
    S = W * s * H * s
    L = nat.lib()
    need = L.dfl_raster_scratch_bytes(W, H, s, len(meshes))
    assert need > 0
    n_rec = C.sizeof(nat.RasterMesh) * len(meshes)
    recs = torch.from_numpy(np.frombuffer(arr, np.uint8, n_rec).copy()).to(dev) if meshes else None
    bufs = {k: fenced(n, dev) for k, n in (('scratch', need), ('rgb', W * H * 3), ('ids', S * 4), ('depth', S * 4), ('counts', 16))}
    a = nat.RasterArgs(meshes=C.addressof(arr) if meshes else None, meshes_dev=nat.ptr(recs), n_mesh=len(meshes), W=W, H=H, ssaa=s,
                       scratch_bytes=need, znear=sc['near'], ambient=light['ambient'], diffuse=light['diffuse'],
                       **{k: v[1].data_ptr() for k, v in bufs.items()})
    a.background[:] = list(light['background'])
    nat.call('dfl_raster_draw', a, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    for k, (whole, _) in bufs.items():
        w = whole.cpu().numpy()
        assert np.all(w[:GUARD] == SENTINEL) and np.all(w[-GUARD:] == SENTINEL), 'guard bytes of %s were written' % k
    out = {k: v[1].cpu().numpy() for k, v in bufs.items()}
    return dict(rgb=out['rgb'].reshape(H, W, 3), ids=out['ids'].view(np.int32).reshape(H * s, W * s),
                depth=out['depth'].view(np.float32).reshape(H * s, W * s), counts=out['counts'].view(np.int32))


def assert_visibility(got, ref, what):
    """ids and depth bits against the float32 model, sample for sample."""
    bad = np.argwhere(got['ids'] != ref['ids'])
    assert not len(bad), '%s: %d samples with another id, first (row, col) %s: %d, model %d' % (
        what, len(bad), bad[0].tolist(), got['ids'][tuple(bad[0])], ref['ids'][tuple(bad[0])])
    gd, rd = got['depth'].view(np.uint32), ref['depth'].astype(np.float32).view(np.uint32)
    bad = np.argwhere(gd != rd)
    assert not len(bad), '%s: %d samples with other depth bits, first %s: %r, model %r' % (
        what, len(bad), bad[0].tolist(), got['depth'][tuple(bad[0])], ref['depth'][tuple(bad[0])])
    assert got['counts'].tolist() == ref['counts'].tolist(), (what, got['counts'], ref['counts'])


@pytest.mark.parametrize('name', CASES)
def test_ids_depth_and_counts_are_the_models(name):
    sc = SC.cases()[name]
    ref = SC.model(sc, **LIGHT)
    got = gpu_draw(sc)
    assert_visibility(got, ref, name)
    if all(s['unlit'] for s in sc['specs']):
        assert np.array_equal(got['rgb'], ref['rgb']), name          # unlit colours, the background and the resolve: exact
    if name == 'both_paths':
        assert ref['n_large'] == 2 and ref['counts'][0] > 250
    if name == 'box_threshold':
        assert ref['n_large'] == 2


@pytest.mark.parametrize('equal', [False, True])
def test_contention_on_one_sample(equal):
    sc = SC.contention(equal)
    got = gpu_draw(sc)
    assert_visibility(got, SC.model(sc, **LIGHT), 'contention')
    assert got['ids'][7, 10] == (0 if equal else 4095) and got['counts'][0] == 4096


def test_two_runs_give_the_same_bytes():
    sc = SC.cases()['both_paths']
    a, b = gpu_draw(sc), gpu_draw(sc)
    for k in ('rgb', 'ids', 'counts'):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a['depth'].view(np.uint32), b['depth'].view(np.uint32))


def test_triangle_order_does_not_change_the_picture():
    sc = SC.cases()['ssaa2']
    ref = SC.model(sc, **LIGHT)
    # the fixture has no depth tie: no sample holds two valid candidates of equal depth
    c, d, ok = ref['cand'], ref['d'], ref['ok']
    order = np.lexsort((d[ok], c['pix'][ok]))
    pix, dd = c['pix'][ok][order], d[ok][order]
    assert not np.any((pix[1:] == pix[:-1]) & (dd[1:] == dd[:-1]))
    rev = dict(sc, specs=[dict(s, tris=s['tris'][::-1].copy()) for s in sc['specs'][::-1]])
    a, b = gpu_draw(sc), gpu_draw(rev)
    assert np.array_equal(a['rgb'], b['rgb']) and np.array_equal(a['rgb'], ref['rgb'])
    assert np.array_equal(a['depth'].view(np.uint32), b['depth'].view(np.uint32))
    assert len(np.unique(a['rgb'].reshape(-1, 3), axis=0)) > 3           # several colours did meet


def assert_shading(got_rgb, sc, ref32, ref64, what):
    """Unlit (textured or not) and background samples exact against the float32 model; lit ones within one level of the
    float64 model.  ssaa = 1: rgb is the samples.  Returns (lit samples, lit samples that differ from float64 at all)."""
    assert sc['ssaa'] == 1
    recs = SC.recs(sc)
    ids = ref32['ids']
    assert np.array_equal(ids, ref64['ids']), 'the fixture must keep the two models on the same winners'
    lit = np.zeros(ids.shape, bool)
    for rec in recs:
        if not rec.flags & RR.UNLIT:
            lit |= (ids >= rec.first_prim) & (ids < rec.first_prim + len(rec.tris))
    assert np.array_equal(got_rgb[~lit], ref32['samples'][~lit]), what
    err = np.abs(got_rgb.astype(int) - ref64['samples'].astype(int)).max(2)
    print('%s: %d lit samples, %d differ from the float64 model, largest difference %d level(s); float32 model: %d differ'
          % (what, lit.sum(), np.sum(err[lit] > 0), err[lit].max(initial=0),
             np.sum(np.abs(ref32['samples'].astype(int) - ref64['samples'].astype(int)).max(2)[lit] > 0)))
    assert err[lit].max(initial=0) <= 1, what
    return int(lit.sum()), int(np.sum(err[lit] > 0))


def test_shading_bars():
    sc = SC.shading_scene()
    ref32, ref64 = SC.model(sc, **LIGHT), SC.model(sc, np.float64, **LIGHT)
    got = gpu_draw(sc)
    assert_visibility(got, ref32, 'shading')
    n_lit, _ = assert_shading(got['rgb'], sc, ref32, ref64, 'shading')
    assert n_lit > 1000 and np.sum(ref32['ids'] >= 6) > 500              # the unlit records are seen too
    assert np.array_equal(got['rgb'], ref32['rgb'])                      # and here the lit samples match float32 as well


def test_texel_edges_are_exact():
    sc = SC.texel_edges()
    ref = SC.model(sc, **LIGHT)
    got = gpu_draw(sc)
    assert_visibility(got, ref, 'texel edges')
    assert np.array_equal(got['rgb'], ref['rgb'])
    tex = sc['specs'][0]['tex']
    assert np.array_equal(got['rgb'][:16, :32, 0], np.repeat(np.repeat(tex, 4, 0), 4, 1))       # each texel 4 x 4 samples, uv 0 and 1 at the corners
    want = np.rint(255 * (np.repeat(np.repeat(tex, 4, 0), 4, 1) / np.float32(255.0) * np.float32(0.25)))
    assert np.abs(got['rgb'][20:36, :32, 2].astype(int) - want).max() <= 1 and got['rgb'][20, 0, 0] == tex[0, 0]


def test_texel_ties_follow_the_float32_model():
    sc = SC.texel_ties()
    ref32, ref64 = SC.model(sc, **LIGHT), SC.model(sc, np.float64, **LIGHT)
    got = gpu_draw(sc)
    assert_visibility(got, ref32, 'texel ties')
    assert_shading(got['rgb'], sc, ref32, ref64, 'texel ties')
    assert np.array_equal(got['rgb'], ref32['rgb'])


def mesh_recs(meshes, view, proj):
    """The model's records of a list of raster.Mesh (tensors downloaded)."""
    out, first = [], 0
    n = lambda t: None if t is None else t.cpu().numpy()         # noqa: E731
    for m in meshes:
        mv = view @ m.matrix
        out.append(RR.Rec(n(m.pos), n(m.tris), proj @ mv, first_prim=first, nrm=n(m.normals), uv=n(m.uv), tex=n(m.texture),
                          nmat=np.linalg.inv(mv[:3, :3]).T, rgb=m.rgb,
                          flags=(RR.UNLIT if m.unlit else 0) | (RR.TEXTURED if m.texture is not None else 0)))
        first += m.tris.shape[0]
    return out


def test_ball_silhouette():
    from dfl_amd import mesh, raster
    z = load_golden('viz3d_ball')
    (v, t), = mesh.label_surfaces(torch.from_numpy(z['volume']).cuda(), z['labels'].tolist())
    xs, undo = mesh.smooth(v, t)
    pos = mesh.transform(xs, undo)
    nrm = mesh.vertex_normals(pos, t)
    p = pos.cpu().numpy().astype(np.float64)
    eye, target = raster.frame(p, (0.4, -0.3, -1.0), 30.0, 64 / 48)
    view = raster.look_at(eye, target, (0, 1, 0))
    dist = float(np.linalg.norm(eye - target))
    proj = raster.perspective(30.0, 64 / 48, dist / 4, dist * 4)
    m = raster.Mesh(pos, t, normals=nrm, rgb=(0.9, 0.8, 0.2))
    rgb, ids = raster.render([m], (view, proj), 64, 48, near=dist / 4, return_ids=True, **LIGHT)
    ref = RR.draw(mesh_recs([m], view, proj), 64, 48, 1, znear=dist / 4, **LIGHT)
    ids = ids.cpu().numpy()
    assert np.array_equal(ids >= 0, ref['ids'] >= 0) and np.array_equal(ids, ref['ids'])
    sil = ids >= 0
    assert 300 < sil.sum() < 64 * 48
    for row in sil:                                               # convex: no background between a row's first and last covered sample
        k = np.nonzero(row)[0]
        assert not len(k) or row[k[0]:k[-1] + 1].all()
    for col in sil.T:
        k = np.nonzero(col)[0]
        assert not len(k) or col[k[0]:k[-1] + 1].all()
    bg = np.rint(255 * np.array(LIGHT['background'], np.float32)).astype(np.uint8)
    assert np.all(rgb.cpu().numpy()[~sil] == bg)
    err = np.abs(rgb.cpu().numpy().astype(int) - RR.draw(mesh_recs([m], view, proj), 64, 48, 1, znear=dist / 4, dtype=np.float64,
                                                          **LIGHT)['samples'].astype(int))
    assert err.max() <= 1


@pytest.mark.parametrize('which', ['oblique', 'source'])
def test_example_png_end_to_end(which, tmp_path):
    import full_res_3d_viz as V
    from dfl_amd import png
    h5 = os.path.join(GOLDEN, 'viz3d_container.h5')
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        assert V.main([h5, 'spec-a', '0', '--out', 'plain.glb']) == 0
        assert V.main([h5, 'spec-a', '0', '--out', 'with.glb', '--png', 'scene.png', '--png-size', '160x120', '--view', which]) == 0
    finally:
        os.chdir(cwd)
    assert (tmp_path / 'plain.glb').read_bytes() == (tmp_path / 'with.glb').read_bytes()
    img = png.read(str(tmp_path / 'scene.png'))
    assert img.shape == (120, 160, 3) and img.dtype == np.uint8
    # the same picture in-process, with ids, against the model on the tensors the example drew
    src = V.Source(h5)
    try:
        g = V.host_geometry(src, 'spec-a', 0, log=lambda s: None)
    finally:
        src.close()
    dev = torch.device('cuda:0')
    surf = []
    V.surfaces_on_gpu(g, dev, log=lambda s: None, on_device=surf)
    rgb, ids, actors, (view, proj, near) = V.render_png(g, surf, dev, which, 160, 120, V.PNG_SSAA, return_ids=True)
    assert np.array_equal(rgb.cpu().numpy(), img)
    recs = mesh_recs([m for _, m in actors], view, proj)
    kw = dict(znear=near, ambient=V.raster.AMBIENT, diffuse=V.raster.DIFFUSE, background=V.BACKGROUND)
    ref32 = RR.draw(recs, 160, 120, V.PNG_SSAA, **kw)
    ref64 = RR.draw(recs, 160, 120, V.PNG_SSAA, dtype=np.float64, **kw)
    ids = ids.cpu().numpy()
    assert np.array_equal(ids, ref32['ids'])
    s = V.PNG_SSAA
    empty = (ref32['ids'] < 0).reshape(120, s, 160, s).all(axis=(1, 3))
    bg = np.rint(255 * np.array(V.BACKGROUND, np.float32)).astype(np.uint8)
    assert empty.any() and np.all(img[empty] == bg)
    seen = 0
    for (name, m), rec in zip(actors, recs):
        mine = (ref32['ids'] >= rec.first_prim) & (ref32['ids'] < rec.first_prim + len(rec.tris))
        if mine.any():
            seen += 1
            assert np.any((ids >= rec.first_prim) & (ids < rec.first_prim + len(rec.tris))), name
    names = [n for n, _ in actors]
    assert seen >= 4 and 'detector' in names and (which == 'source') == (not any(n.startswith('ray/') for n in names))
    # shading: exact where no sample of the pixel is lit, within one level of the float64 model where both models see the same
    lit = np.zeros(ids.shape, bool)
    for rec in recs:
        if not rec.flags & RR.UNLIT:
            lit |= (ref32['ids'] >= rec.first_prim) & (ref32['ids'] < rec.first_prim + len(rec.tris))
    lit_px = lit.reshape(120, s, 160, s).any(axis=(1, 3))
    agree = (ref32['ids'] == ref64['ids']).reshape(120, s, 160, s).all(axis=(1, 3))
    assert np.mean(agree) > 0.999
    assert np.array_equal(img[~lit_px], ref32['rgb'][~lit_px])
    assert np.abs(img.astype(int) - ref64['rgb'].astype(int)).max(2)[agree].max() <= 1
