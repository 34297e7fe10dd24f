"""The kernels of csrc/decimate.hip through their C entry points, stage by stage, and dfl_amd.mesh.decimate end to end,
against the numpy model tests/decimate_ref.py.

Stage by stage: each stage's model is fed the GPU's own output of the stage before (the quadrics the kernel wrote go into
the model of the keys, the keys into the model of the minima, ...), and every output -- Q, key, cand, m1, m2, the flags,
remap, positions, triangles, degenerate flags -- must be equal bit for bit: the kernels are built without contraction,
fp64 division and square root are correctly rounded, and the model writes every expression in the kernels' order.

Every output buffer is filled with a sentinel before the call (NaN, -1, 0xff, 0x5a5a... for the 64-bit keys, whose own
"no candidate" value is all ones) and carries GUARD elements past its end that must still hold it afterwards.  The lists
a kernel uses as addresses (the CSRs, the edge lists, eid) are asserted against the model before the first launch, and
the flags `take` that the apply kernels follow are the model's cut of the asserted selection."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'examples'))
import decimate_ref as D  # noqa: E402
import mesh_ref as R  # noqa: E402
from dfl_amd import _native as nat, mesh  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 64
NAN = float('nan')
SENT64 = 0x5A5A5A5A5A5A5A5A


def stream():
    return torch.cuda.current_stream().cuda_stream


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def filled(n, dtype, value):
    return torch.full((n + GUARD,), value, dtype=dtype, device=DEV)


def untouched(a, value):
    return np.all(np.isnan(a)) if a.dtype.kind == 'f' else np.all(a == value)


def head(t, n, what, value):
    """The first n elements of a buffer made by filled(n, ..., value), on the host; its guard must still hold the sentinel."""
    a = t.cpu().numpy()
    assert a[n:].size == GUARD and untouched(a[n:], value), what + ': written past the end'
    return a[:n]


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, '%s: %d of %d differ, first at %d: got %s, model %s' % (
        what, bad.size, got.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


@functools.lru_cache(maxsize=None)
def case(name):
    """(positions [V, 3] fp32, tris [T, 3] int32)."""
    if name in ('ball', 'torus', 'blob'):
        z = load_golden('viz3d_' + name)
        return z['smooth_0'].astype(np.float32), z['tris_0']
    if name == 'tetra+unused':
        return D.random_points(8, 1), D.TETRA_IDS[D.TETRA]
    if name == 'fin':                 # a torus grid with a third triangle glued to one of its edges
        pos, tris = D.torus_grid(8, 8, seed=3)
        a, b = int(tris[0, 0]), int(tris[0, 1])
        return (np.concatenate([pos, (1.3 * (pos[a] + pos[b]) / 2)[None]]).astype(np.float32),
                np.concatenate([tris, [[a, b, len(pos)]]]).astype(np.int32))
    return {'V256': lambda: D.torus_grid(16, 16, seed=7), 'V257': lambda: D.uv_sphere(15, 17, seed=8)}[name]()


def gpu_round(pos, tris, remaining):
    """One round through the four entry points, every output asserted against the model fed the GPU's previous output.
    Returns what the model makes of the GPU's last outputs: (pos', tris', collapses, candidates, selected)."""
    V, T = len(pos), len(tris)
    pd, td = up(pos), up(tris)
    want = D.topology(tris, V)
    tp = mesh._round_topology(td, V)
    assert sorted(tp) == sorted(want)
    for k in want:                                    # before any kernel of this module uses them as addresses
        same(tp[k].cpu().numpy(), want[k], k)
    E = len(want['edge_u'])
    p = {k: t.data_ptr() for k, t in tp.items()}

    Q = filled(10 * V, torch.float64, NAN)
    nat.call('dfl_mesh_quadrics', nat.MeshQuadricsArgs(pos=pd.data_ptr(), tris=td.data_ptr(), vt_ptr=p['vt_ptr'], vt_tri=p['vt_tri'],
                                                       Q=Q.data_ptr(), V=V, T=T), stream())
    q = head(Q, 10 * V, 'Q', None).reshape(V, 10)
    same(bits(q), bits(D.quadrics(pos, tris, want)), 'Q')

    key, cand = filled(E, torch.int64, SENT64), filled(3 * E, torch.float32, NAN)
    nat.call('dfl_mesh_collapse_keys', nat.MeshCollapseKeysArgs(
        pos=pd.data_ptr(), tris=td.data_ptr(), row_ptr=p['row_ptr'], col=p['col'], use=p['use'], vt_ptr=p['vt_ptr'],
        vt_tri=p['vt_tri'], Q=Q.data_ptr(), edge_u=p['edge_u'], edge_v=p['edge_v'], key=key.data_ptr(), cand=cand.data_ptr(),
        V=V, T=T, E=E), stream())
    k = head(key, E, 'key', SENT64).view(np.uint64)
    c = head(cand, 3 * E, 'cand', None).reshape(E, 3)
    want_key, want_cand, _ = D.collapse_keys(pos, tris, want, q)
    same(k, want_key, 'key')
    same(bits(c), bits(want_cand), 'cand')

    m1, m2, sel = filled(V, torch.int64, SENT64), filled(V, torch.int64, SENT64), filled(E, torch.uint8, 255)
    nat.call('dfl_mesh_collapse_select', nat.MeshCollapseSelectArgs(
        row_ptr=p['row_ptr'], col=p['col'], eid=p['eid'], edge_u=p['edge_u'], edge_v=p['edge_v'], key=key.data_ptr(),
        m1=m1.data_ptr(), m2=m2.data_ptr(), sel=sel.data_ptr(), V=V, E=E), stream())
    g1, g2 = head(m1, V, 'm1', SENT64).view(np.uint64), head(m2, V, 'm2', SENT64).view(np.uint64)
    gs = head(sel, E, 'sel', 255)
    same(g1, D.select_m1(k, want), 'm1')
    same(g2, D.select_m2(g1, want), 'm2')
    same(gs, D.select_flags(k, g2, want), 'sel')

    take = D.budget_cut(k, gs, remaining)
    remap, pos_out = filled(V, torch.int32, -1), filled(3 * V, torch.float32, NAN)
    tris_out, degen = filled(3 * T, torch.int32, -1), filled(T, torch.uint8, 255)
    nat.call('dfl_mesh_collapse_apply', nat.MeshCollapseApplyArgs(
        pos=pd.data_ptr(), tris=td.data_ptr(), row_ptr=p['row_ptr'], col=p['col'], eid=p['eid'], take=up(take).data_ptr(),
        cand=cand.data_ptr(), remap=remap.data_ptr(), pos_out=pos_out.data_ptr(), tris_out=tris_out.data_ptr(),
        degen=degen.data_ptr(), V=V, T=T, E=E), stream())
    got = (head(remap, V, 'remap', -1), head(pos_out, 3 * V, 'pos_out', None).reshape(V, 3),
           head(tris_out, 3 * T, 'tris_out', -1).reshape(T, 3), head(degen, T, 'degen', 255))
    model = D.apply(pos, tris, want, take, c)
    same(got[0], model[0], 'remap')
    same(bits(got[1]), bits(model[1]), 'pos_out')
    same(got[2], model[2], 'tris_out')
    same(got[3], model[3], 'degen')
    # the inputs are as they were
    same(bits(pd.cpu().numpy()), bits(pos), 'pos')
    same(td.cpu().numpy(), tris, 'tris')
    return D.compact(*got) + (int(take.sum()), int(np.sum(k != D.KEY_NONE)), int(gs.sum()))


@pytest.mark.parametrize('name', ['ball', 'torus', 'blob', 'V256', 'V257'])
def test_stages_bit_for_bit(name):
    """Two rounds: the second runs on the mesh the first left (renumbered vertices, vertices of higher degree)."""
    pos, tris = case(name)
    V0 = len(pos)
    if name in ('V256', 'V257'):
        assert V0 == int(name[1:]) and set(R.edge_uses(tris).values()) == {2}
    for rnd in range(2):
        V, T = len(pos), len(tris)
        pos, tris, n, cands, selected = gpu_round(pos, tris, 10 ** 9)
        print('%s round %d: V %d T %d candidates %d selected %d' % (name, rnd, V, T, cands, selected))
        assert n == selected > 0 and cands > selected
        assert (len(pos), len(tris)) == (V - n, T - 2 * n)
    if name == 'blob':                                # the borders are where they were
        p0, t0 = case(name)
        border = lambda p, t: {frozenset((p[a].tobytes(), p[b].tobytes())) for (a, b), m in R.edge_uses(t).items() if m == 1}   # noqa: E731
        assert border(pos, tris) == border(p0, t0) and len(border(p0, t0)) == 933


def test_stages_with_a_budget_cut():
    pos, tris = case('torus')
    _, t1, n, _, selected = gpu_round(pos, tris, 5)
    assert n == 5 < selected and len(t1) == len(tris) - 10


def test_tetrahedron_among_unused_vertices():
    pos, tris = case('tetra+unused')
    p1, t1, n, cands, selected = gpu_round(pos, tris, 10 ** 9)
    assert (n, cands, selected) == (0, 0, 0)
    same(bits(p1), bits(pos), 'pos')
    same(t1, tris, 'tris')
    got = mesh.decimate(up(pos), up(tris), 0.5)
    assert got[2] == {'collapses': 0, 'rounds': 0, 'budget': 1}
    same(bits(got[0].cpu().numpy()), bits(pos), 'pos')
    same(got[1].cpu().numpy(), tris, 'tris')


def test_non_manifold_fin():
    pos, tris = case('fin')
    a, b, f = int(tris[0, 0]), int(tris[0, 1]), len(pos) - 1
    assert R.edge_uses(tris)[(min(a, b), max(a, b))] == 3
    p1, t1, n, cands, _ = gpu_round(pos, tris, 10 ** 9)
    assert n > 0 and cands > 0
    have = {v.tobytes() for v in p1}
    assert all(pos[k].tobytes() in have for k in (a, b, f))


def check_surface(p0, t0, p1, t1, info, reduction):
    assert info['budget'] == D.budget(reduction, len(t0))
    assert len(t1) == len(t0) - 2 * info['collapses'] and len(p1) == len(p0) - info['collapses']
    assert R.euler(p1, t1) == R.euler(p0, t0)
    assert set(R.edge_uses(t1).values()) == set(R.edge_uses(t0).values()) == {2}
    assert R.signed_volume(p0, t0) * R.signed_volume(p1, t1) > 0


@pytest.mark.parametrize('name,reduction', [('ball', 0.25), ('torus', 0.25), ('ball', 0.9)])
def test_decimate_end_to_end(name, reduction):
    """At 0.9 the ball takes 34 rounds and the budget ends in the middle of the last one."""
    pos, tris = case(name)
    wp, wt, winfo = D.decimate(pos, tris, reduction)
    assert winfo['per_round'][-1] < D.one_round(pos, tris, 10 ** 9)[2] and winfo['collapses'] == winfo['budget']
    runs = []
    for _ in range(2):
        gp, gt, info = mesh.decimate(up(pos), up(tris), reduction)
        assert gp.dtype == torch.float32 and gt.dtype == torch.int32 and gp.is_contiguous() and gt.is_contiguous()
        runs.append((gp.cpu().numpy(), gt.cpu().numpy(), info))
    gp, gt, info = runs[0]
    assert info == {k: winfo[k] for k in ('collapses', 'rounds', 'budget')}
    same(gt, wt, 'tris')
    same(bits(gp), bits(wp), 'verts')
    assert runs[1][2] == info and runs[1][0].tobytes() == gp.tobytes() and runs[1][1].tobytes() == gt.tobytes()
    check_surface(pos, tris, gp, gt, info, reduction)


def test_max_rounds_ends_the_run():
    pos, tris = case('ball')
    gp, gt, info = mesh.decimate(up(pos), up(tris), 0.9, max_rounds=2)
    wp, wt, winfo = D.decimate(pos, tris, 0.9, max_rounds=2)
    assert info == {'collapses': winfo['collapses'], 'rounds': 2, 'budget': 883} and info['collapses'] < 883
    same(gt.cpu().numpy(), wt, 'tris')
    same(bits(gp.cpu().numpy()), bits(wp), 'verts')


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_outputs_untouched():
    pos, tris = case('tetra+unused')
    V, T = len(pos), len(tris)
    tp = D.topology(tris, V)
    E = len(tp['edge_u'])
    d = {k: up(v) for k, v in tp.items()}
    d.update(pos=up(pos), tris=up(tris), Q=filled(10 * V, torch.float64, NAN), key=filled(E, torch.int64, SENT64),
             cand=filled(3 * E, torch.float32, NAN), m1=filled(V, torch.int64, SENT64), m2=filled(V, torch.int64, SENT64),
             sel=filled(E, torch.uint8, 255), take=up(np.zeros(E, np.uint8)), remap=filled(V, torch.int32, -1),
             pos_out=filled(3 * V, torch.float32, NAN), tris_out=filled(3 * T, torch.int32, -1), degen=filled(T, torch.uint8, 255))
    outputs = dict(Q=None, key=SENT64, cand=None, m1=SENT64, m2=SENT64, sel=255, remap=-1, pos_out=None, tris_out=-1, degen=255)
    L = nat.lib()
    for fn, cls in (('dfl_mesh_quadrics', nat.MeshQuadricsArgs), ('dfl_mesh_collapse_keys', nat.MeshCollapseKeysArgs),
                    ('dfl_mesh_collapse_select', nat.MeshCollapseSelectArgs), ('dfl_mesh_collapse_apply', nat.MeshCollapseApplyArgs)):
        fields = [f for f, _ in cls._fields_]
        good = {f: d[f].data_ptr() for f in fields if f in d}
        good.update({c: n for c, n in (('V', V), ('T', T), ('E', E)) if c in fields})
        assert sorted(good) == sorted(fields)
        refusals = [{c: 0} for c in 'VTE' if c in fields] + [{c: 2 ** 31} for c in 'VTE' if c in fields] + \
                   [{f: None} for f in fields if f not in 'VTE']
        for kw in refusals:
            a = cls(**dict(good, **kw))
            assert getattr(L, fn)(C.addressof(a), stream()) == -1 and fn.encode() in L.dfl_last_error(), (fn, kw)
        torch.cuda.synchronize()
        for f, value in outputs.items():
            assert untouched(d[f].cpu().numpy(), value), (fn, f)


def test_python_refuses_bad_meshes_before_any_launch():
    pos, tris = case('tetra+unused')
    pd = up(pos)
    for bad, word in ((np.where(tris == 6, 8, tris), 'outside'), (np.where(tris == 1, -1, tris), 'outside'),
                      (np.where(tris == 6, 4, tris), 'repeats'), (tris[:0], 'no triangles')):
        with pytest.raises(nat.DflError, match=word):
            mesh.decimate(pd, up(bad.astype(np.int32)), 0.5)
    with pytest.raises(nat.DflError, match='reduction'):
        mesh.decimate(pd, up(tris), 1.0)
    with pytest.raises(nat.DflError, match='GPU'):
        mesh.decimate(pd, torch.from_numpy(tris), 0.5)


# ---- the example --------------------------------------------------------------------------------------------------------
SURFACE_NODES = ['left-hemipelvis', 'right-hemipelvis', 'left-femur', 'right-femur']


def test_example_with_and_without_the_flag(tmp_path, capsys):
    import full_res_3d_viz as V
    from dfl_amd import gltf, png
    from dfl_amd.fullres import Source
    h5 = os.path.join(GOLDEN, 'viz3d_container.h5')
    zc = load_golden('viz3d_container')
    plain, reduced, picture = tmp_path / 'plain.glb', tmp_path / 'reduced.glb', tmp_path / 'reduced.png'
    assert V.main([h5, 'spec-a', '0', '--out', str(plain)]) == 0
    assert V.main([h5, 'spec-a', '0', '--out', str(reduced), '--decimate', '0.25', '--png', str(picture), '--png-size', '320x240']) == 0
    capsys.readouterr()
    # without the flag: the scene of the undecimated path, byte for byte, with the golden triangles
    src = Source(h5)
    try:
        g = V.host_geometry(src, 'spec-a', 0, log=lambda *a: None)
    finally:
        src.close()
    dev = torch.device(DEV)
    assert plain.read_bytes() == V.build_scene(g, V.surfaces_on_gpu(g, dev, log=lambda *a: None)).encode()
    a, b = gltf.Glb(str(plain)), gltf.Glb(str(reduced))
    for k, name in enumerate(SURFACE_NODES):
        t0 = a.accessor(a.primitive(name)['indices']).reshape(-1, 3)
        assert np.array_equal(t0, zc['tris_%d' % k])
        prim = b.primitive(name)
        t1 = b.accessor(prim['indices']).reshape(-1, 3).astype(np.int32)
        p1 = b.accessor(prim['attributes']['POSITION'])
        n1 = b.accessor(prim['attributes']['NORMAL']).astype(np.float64)
        p0 = a.accessor(a.primitive(name)['attributes']['POSITION'])
        budget = D.budget(0.25, len(t0))
        print('%s: T %d -> %d (budget %d), V %d -> %d' % (name, len(t0), len(t1), budget, len(p0), len(p1)))
        assert len(t1) == len(t0) - 2 * budget and len(p1) == len(p0) - budget == len(n1)
        assert t1.min() == 0 and t1.max() == len(p1) - 1
        assert np.abs(np.sqrt((n1 * n1).sum(1)) - 1).max() < 1e-5
        assert R.euler(p1, t1) == R.euler(p0, t0.astype(np.int32)) and set(R.edge_uses(t1).values()) == {2}
    # everything but the surfaces is the same scene
    assert [n['name'] for n in a.doc['nodes']] == [n['name'] for n in b.doc['nodes']]
    img = png.decode(picture.read_bytes())
    assert img.shape == (240, 320, 3) and len(np.unique(img.reshape(-1, 3), axis=0)) > 10
