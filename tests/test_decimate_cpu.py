"""Quadric-error decimation without a GPU: the numpy model (tests/decimate_ref.py) on the committed surfaces -- counts,
rounds, Euler characteristic, edge uses, held borders, degrees, orientation and enclosed volume -- its corner cases, every
refusal of the four C entry points (the library loads without a GPU and refuses before it launches), the dfl_sizeof
entries, the refusals of mesh.decimate that come before any GPU work, and --decimate of examples/full_res_3d_viz.py."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'examples'))
import decimate_ref as D  # noqa: E402
import mesh_ref as R  # noqa: E402
from dfl_amd import _native as nat, mesh  # noqa: E402

# the model's relative change of the enclosed volume at reduction 0.25: a property of the definition
VOLUME_CHANGE = {'ball': 5.93e-4, 'torus': 5.97e-4}


def smoothed(name, i=0):
    z = load_golden('viz3d_' + name)
    return z['smooth_%d' % i].astype(np.float32), z['tris_%d' % i]


@functools.lru_cache(maxsize=None)
def run(name, i, reduction):
    pos, tris = smoothed(name, i)
    return (pos, tris) + D.decimate(pos, tris, reduction)


def border_edges(pos, tris):
    """The edges of exactly one triangle as a set of pairs of position bytes (vertex ids change, held positions do not)."""
    return {frozenset((pos[a].tobytes(), pos[b].tobytes())) for (a, b), n in R.edge_uses(tris).items() if n == 1}


# (fixture, surface, reduction): rounds, T in, T out, V in, V out, Euler characteristic, border edges
TABLE = {('ball', 0, 0.25): (4, 1964, 1474, 984, 739, 2, 0), ('torus', 0, 0.25): (4, 2800, 2100, 1400, 1050, 0, 0),
         ('container', 1, 0.25): (5, 3820, 2866, 1920, 1443, 10, 0), ('blob', 0, 0.25): (4, 5681, 4261, 3954, 3244, 647, 933),
         ('ball', 0, 0.9): (34, 1964, 198, 984, 101, 2, 0), ('torus', 0, 0.75): (21, 2800, 700, 1400, 350, 0, 0)}


@pytest.mark.parametrize('case', sorted(TABLE), ids=lambda c: '%s%d-%g' % c)
def test_the_committed_surfaces(case):
    rounds, T0, T1, V0, V1, chi, borders = TABLE[case]
    pos, tris, p2, t2, info = run(*case)
    assert (len(tris), len(pos)) == (T0, V0) and R.euler(pos, tris) == chi
    assert (info['rounds'], len(t2), len(p2)) == (rounds, T1, V1)
    assert info['budget'] == int(case[2] * T0) // 2 == info['collapses'] == sum(info['per_round'])
    assert len(t2) == T0 - 2 * info['collapses'] and len(p2) == V0 - info['collapses']
    assert R.euler(p2, t2) == chi
    uses = np.array(list(R.edge_uses(t2).values()))
    assert np.sum(uses == 1) == borders and np.all((uses == 2) | (uses == 1))
    assert border_edges(p2, t2) == border_edges(pos, tris) and len(border_edges(pos, tris)) == borders
    assert len(np.unique(np.sort(t2, 1), axis=0)) == len(t2), 'duplicate triangles'
    assert t2.min() == 0 and t2.max() == len(p2) - 1 and len(np.unique(t2)) == len(p2)
    if borders == 0:
        assert np.diff(D.topology(t2, len(p2))['row_ptr']).min() >= 3
    # no triangle turned over: the enclosed volume keeps its sign (and, for the closed surfaces, nearly its size)
    v0, v1 = R.signed_volume(pos, tris), R.signed_volume(p2, t2)
    assert v0 * v1 > 0
    if borders == 0:
        assert abs(v1 - v0) < 0.02 * abs(v0)


@pytest.mark.parametrize('name', ['ball', 'torus'])
def test_enclosed_volume_at_a_quarter(name):
    pos, tris, p2, t2, _ = run(name, 0, 0.25)
    v0, v1 = R.signed_volume(pos, tris), R.signed_volume(p2, t2)
    change = abs(v1 - v0) / abs(v0)
    print('%s: enclosed volume %.6f -> %.6f, relative change %.3e' % (name, v0, v1, change))
    assert change <= 2 * VOLUME_CHANGE[name]


def test_survivors_keep_their_order_and_winding():
    """A vertex that no collapse touched keeps its position bits, in the input's order; every surviving triangle keeps its
    place and its first-corner rotation."""
    pos, tris = smoothed('ball')
    p1, t1, n, st = D.one_round(pos, tris, 10 ** 9)
    assert n == st['take'].sum() == st['sel'].sum() > 50
    remap, pos_out, tris_out, degen = D.apply(pos, tris, st['tp'], st['take'], st['cand'])
    assert degen.sum() == 2 * n and np.sum(remap != np.arange(len(pos))) == n
    keep = remap == np.arange(len(pos))
    assert np.array_equal(p1, pos_out[keep])
    moved = np.zeros(len(pos), bool)
    moved[st['tp']['edge_u'][st['take'] == 1]] = True
    assert np.array_equal(pos_out[keep & ~moved].view(np.int32), pos[keep & ~moved].view(np.int32))
    # the taken edges share no vertex and no neighbour's edge: their ends are pairwise non-adjacent
    ends = np.concatenate([st['tp']['edge_u'][st['take'] == 1], st['tp']['edge_v'][st['take'] == 1]])
    assert len(np.unique(ends)) == 2 * n
    on = np.zeros(len(pos), bool)
    on[ends] = True
    touched = on[tris].sum(1)
    assert touched.max() == 2 and np.sum(touched == 2) == 2 * n


def test_tetrahedron_and_octahedron_have_no_candidate():
    z = load_golden('viz3d_voxel')
    for pos, tris in ((D.random_points(4, 1), D.TETRA), (z['verts_0'], z['tris_0'])):
        tp = D.topology(tris, len(pos))
        key, cand, aux = D.collapse_keys(pos, tris, tp, D.quadrics(pos, tris, tp))
        assert not aux['held'].any() and np.all(key == D.KEY_NONE) and not cand.any()
        p2, t2, info = D.decimate(pos, tris, 0.5)
        assert info == dict(collapses=0, rounds=0, budget=len(tris) // 4, per_round=[]) and info['budget'] >= 1
        assert np.array_equal(p2.view(np.int32), pos.view(np.int32)) and np.array_equal(t2, tris)
    assert len(z['tris_0']) == 8 and len(z['verts_0']) == 6


def test_three_triangles_on_one_edge_hold_its_vertices():
    """A torus grid with a fin glued to one of its edges: that edge has use 3, both its ends are held, no edge at them is
    a candidate, and both keep their position through a whole run."""
    pos, tris = D.torus_grid(8, 8, seed=3)
    a, b = int(tris[0, 0]), int(tris[0, 1])
    pos = np.concatenate([pos, (1.3 * (pos[a] + pos[b]) / 2)[None]]).astype(np.float32)
    tris = np.concatenate([tris, [[a, b, len(pos) - 1]]]).astype(np.int32)
    assert R.edge_uses(tris)[(min(a, b), max(a, b))] == 3
    tp = D.topology(tris, len(pos))
    key, _, aux = D.collapse_keys(pos, tris, tp, D.quadrics(pos, tris, tp))
    assert aux['held'][[a, b, len(pos) - 1]].all() and aux['held'].sum() == 3
    at = (tp['edge_u'] == a) | (tp['edge_v'] == a) | (tp['edge_u'] == b) | (tp['edge_v'] == b)
    assert np.all(key[at] == D.KEY_NONE) and np.any(key[~at] != D.KEY_NONE)
    p2, t2, info = D.decimate(pos, tris, 0.5)
    assert info['collapses'] > 0
    have = {p.tobytes() for p in p2}
    assert all(pos[k].tobytes() in have for k in (a, b, len(pos) - 1))
    assert np.all(D.collapse_keys(D.random_points(5, 2), D.FAN, D.topology(D.FAN, 5), np.zeros((5, 10)))[0] == D.KEY_NONE)


def test_unused_vertices_pass_through():
    pos, tris = smoothed('ball')
    extra = D.random_points(3, 5)
    pos_x = np.concatenate([extra[:2], pos, extra[2:]])
    p2, t2, info = D.decimate(pos, tris, 0.25)
    px, tx, info_x = D.decimate(pos_x, tris + 2, 0.25)
    assert info_x == info
    assert np.array_equal(px.view(np.int32), np.concatenate([extra[:2], p2, extra[2:]]).view(np.int32))
    assert np.array_equal(tx, t2 + 2)


def test_a_budget_of_one_takes_the_lowest_key():
    pos, tris = smoothed('torus')
    _, t1, n, st = D.one_round(pos, tris, 1)
    assert n == 1 and len(t1) == len(tris) - 2 and st['sel'].sum() > 1
    e = int(np.flatnonzero(st['take'])[0])
    assert st['key'][e] == st['key'][st['sel'] == 1].min() == st['key'].min()
    # and a cut in the middle takes the lowest keys of the selected
    take = D.budget_cut(st['key'], st['sel'], 7)
    assert take.sum() == 7 and st['key'][take == 1].max() < st['key'][(st['sel'] == 1) & (take == 0)].min()


def test_selected_edges_are_candidates_with_the_two_ring_minimum():
    pos, tris = smoothed('container', 1)
    tp = D.topology(tris, len(pos))
    key, _, aux = D.collapse_keys(pos, tris, tp, D.quadrics(pos, tris, tp))
    assert aux['solved'][key != D.KEY_NONE].any() and (~aux['solved'][key != D.KEY_NONE]).any()     # both position forms occur
    m1 = D.select_m1(key, tp)
    m2 = D.select_m2(m1, tp)
    sel = D.select_flags(key, m2, tp)
    assert sel.sum() > 100 and np.all(key[sel == 1] != D.KEY_NONE)
    rows = np.repeat(np.arange(len(pos)), np.diff(tp['row_ptr']))
    for e in np.flatnonzero(sel)[:20]:
        ring = set()
        for w in (tp['edge_u'][e], tp['edge_v'][e]):
            ring |= {int(w)} | set(tp['col'][rows == w].tolist())
        near = np.isin(tp['edge_u'], list(ring)) | np.isin(tp['edge_v'], list(ring))
        assert key[e] == key[near].min()


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
P = 4096                                                  # never dereferenced: the checks come first
ENTRY = {
    'dfl_mesh_quadrics': (nat.MeshQuadricsArgs, ('pos', 'tris', 'vt_ptr', 'vt_tri', 'Q'), ('V', 'T')),
    'dfl_mesh_collapse_keys': (nat.MeshCollapseKeysArgs, ('pos', 'tris', 'row_ptr', 'col', 'use', 'vt_ptr', 'vt_tri', 'Q', 'edge_u',
                                                          'edge_v', 'key', 'cand'), ('V', 'T', 'E')),
    'dfl_mesh_collapse_select': (nat.MeshCollapseSelectArgs, ('row_ptr', 'col', 'eid', 'edge_u', 'edge_v', 'key', 'm1', 'm2', 'sel'),
                                 ('V', 'E')),
    'dfl_mesh_collapse_apply': (nat.MeshCollapseApplyArgs, ('pos', 'tris', 'row_ptr', 'col', 'eid', 'take', 'cand', 'remap', 'pos_out',
                                                            'tris_out', 'degen'), ('V', 'T', 'E')),
}


@pytest.mark.parametrize('fn', sorted(ENTRY))
def test_c_abi_refuses_bad_arguments(fn):
    """Every refusal comes back as -1 with a message, before anything is launched (there is no GPU here to launch on)."""
    L = nat.lib()
    cls, pointers, counts = ENTRY[fn]
    assert [f for f, _ in cls._fields_] == list(pointers) + list(counts)          # every field is covered below

    def call(**k):
        a = cls(**dict(dict({f: P for f in pointers}, **{c: 100 for c in counts}), **k))
        return getattr(L, fn)(C.addressof(a), None), L.dfl_last_error()

    for f in pointers:
        rc, msg = call(**{f: None})
        assert rc == -1 and b'required' in msg and fn.encode() in msg and f.encode() in msg, (f, msg)
    big = {'V': 2 ** 31, 'T': (2 ** 31 + 2) // 3, 'E': 2 ** 30}        # V, 3 T and 2 E reach 2^31
    for c in counts:
        for bad in (0, -1, big[c], 2 ** 31, 2 ** 40):
            rc, msg = call(**{c: bad})
            assert rc == -1 and b'2^31' in msg and fn.encode() in msg, (c, bad, msg)
    assert getattr(L, fn)(None, None) == -1 and b'required' in L.dfl_last_error()
    if not torch.cuda.is_available():                     # what is allowed fails only at the launch, for want of a GPU
        assert call()[0] == nat.ERR_LAUNCH
        assert call(**{c: big[c] - 1 for c in counts})[0] == nat.ERR_LAUNCH


def test_sizeof_entries_and_their_position():
    L = nat.lib()
    k = nat._SIZEOF_ORDER.index(nat.MeshNormalsArgs)
    new = [nat.MeshQuadricsArgs, nat.MeshCollapseKeysArgs, nat.MeshCollapseSelectArgs, nat.MeshCollapseApplyArgs]
    assert nat._SIZEOF_ORDER[k + 1:k + 5] == new and nat._SIZEOF_ORDER[k + 5] is nat.PreprocProjsArgs
    for i, (cls, size) in enumerate(zip(new, (56, 120, 88, 112))):
        assert L.dfl_sizeof(k + 1 + i) == C.sizeof(cls) == size, cls
    assert L.dfl_sizeof(len(nat._SIZEOF_ORDER)) == -1
    for fn in ENTRY:
        assert fn in nat.EXPORTS and getattr(L, fn).restype is C.c_int and getattr(L, fn).argtypes == [C.c_void_p, C.c_void_p]


def test_python_refuses_before_any_gpu_work():
    pos, tris = torch.zeros(4, 3), torch.from_numpy(D.TETRA)
    for bad in (0.0, 1.0, -0.25, 1.5, float('nan')):
        with pytest.raises(nat.DflError, match='reduction'):
            mesh.decimate(pos, tris, bad)
    with pytest.raises(nat.DflError, match='GPU'):
        mesh.decimate(pos, tris)
    with pytest.raises(nat.DflError, match='tensor'):
        mesh.decimate(pos.numpy(), tris)
    with pytest.raises(nat.DflError, match='dtype'):
        mesh.decimate(pos.double(), tris)
    assert mesh.collapse_budget(0.25, 1964) == 245 == D.budget(0.25, 1964) and mesh.collapse_budget(0.9, 1964) == 883
    assert (mesh.REDUCTION, mesh.MAX_ROUNDS) == (0.25, 64) == (float(load_golden('viz3d_scene')['decimation']), D.MAX_ROUNDS)


def test_decimate_flag_of_the_example(capsys):
    import full_res_3d_viz as V
    assert V.options(['f', 's', '1', '--decimate', '0.25']) == (['f', 's', '1'], {'--decimate': 0.25})
    assert V.options(['f', '--decimate', '0.5', 's', '1', '--png', 'p.png']) == \
        (['f', 's', '1'], {'--decimate': 0.5, '--png': 'p.png', '--png-size': None, '--view': 'oblique', '--ssaa': V.PNG_SSAA})
    assert V.options(['f', 's', '1']) == (['f', 's', '1'], {})
    assert V.main(['a.h5', 'spec', '0', '--decimate']) == 1
    assert capsys.readouterr().out.strip() == '--decimate needs a value'
    for bad in ('0', '1', '-0.5', '2', 'half', 'nan'):
        assert V.main(['a.h5', 'spec', '0', '--decimate', bad]) == 1, bad
        assert capsys.readouterr().out.startswith('--decimate is a reduction')
    assert V.main(['a.h5', 'spec', '--decimate', '0.25']) == 1                    # the usage line is unchanged
    assert capsys.readouterr().out.strip() == 'Usage: {} <HDF5 full-res data file> <specimen ID> <projection index>'.format(
        os.path.basename(sys.argv[0]))
