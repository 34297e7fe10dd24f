"""dfl_amd.tools without a GPU: the float64 model of tests/tools_ref.py against brute force and its exact cases, the
culling rectangle, the sampled tools and their stream, the command line, the ctypes mirror of dfl_tools_args, the refusals
at the C ABI that need no device, and the committed floors."""
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
import tools_floor as FL  # noqa: E402
import tools_ref as T  # noqa: E402
import dfl_amd  # noqa: E402
from dfl_amd import _native as nat, drr, preprocess as pp, synth, tools  # noqa: E402


def _grid(name):
    Q, H, W = T.grid(name)
    return drr.Grid(Q, H, W)


def test_the_model_against_brute_force():
    """40 rays over the cases' capsules, 2 10^5 samples of t each: the float64 model's chord within one sampling step
    times |d|."""
    rng = np.random.default_rng(3)
    names = ['bead_on_ray', 'bead_between', 'oblique_wire', 'wire_along_ray', 'wire_leaves_image', 'wire_through_source_plane',
             'crossing_wires', 'many_short_wires']
    hit = 0
    for n in range(40):
        name = names[n % len(names)]
        g, views = T.cases()[name]
        Q, H, W = T.grid(g)
        caps = views[0]
        cap = caps[int(rng.integers(len(caps)))]
        s, tl = T.add([T.records([cap])], Q.astype(np.float32), H, W)
        lit = np.argwhere(tl[0] > 0)
        r, c = lit[int(rng.integers(len(lit)))] if n % 5 else (int(rng.integers(H)), int(rng.integers(W)))
        rec = T.records([cap])[0]                                           # what the model saw: float32 values
        d = Q.astype(np.float32).astype(np.float64) @ np.array([c, r, 1.0])
        want, step = T.brute_chord((rec['a'], rec['b'], rec['r'], rec['mu']), d)
        assert abs(tl[0, r, c] - want) <= step, (name, r, c, tl[0, r, c], want, step)
        assert abs(s[0, r, c] - float(rec['mu']) * tl[0, r, c]) <= 1e-12
        hit += want > 0
    assert hit >= 30


def test_exact_cases_of_the_model():
    Q, H, W = T.grid('full')
    q32 = Q.astype(np.float32)
    d = q32.astype(np.float64) @ np.array([20.0, 10.0, 1.0])
    u = d / np.linalg.norm(d)
    # a bead through its centre: 2 r.  (The centre is given in float32-exact numbers so that the ray really goes through it.)
    ctr = (np.float32(800.0) * u).astype(np.float32).astype(np.float64)
    t = float(ctr @ u)
    off = ctr - t * u
    for r in (0.75, 2.5):
        _, tl = T.add([T.records([(ctr, ctr, r, 0.5)])], q32, H, W, pixels=([10], [20]))
        assert abs(tl[0, 0] - 2 * np.sqrt(np.float64(np.float32(r)) ** 2 - off @ off)) <= 1e-12
        assert abs(tl[0, 0] - 2 * np.float64(np.float32(r))) <= 1e-9
    # a wire seen end-on: its length plus 2 r, through the parallel branch (the two spheres alone)
    a, b = 760.0 * u, 840.0 * u
    rec = T.records([(a, b, 0.8, 0.5)])
    _, tl = T.add([rec], q32, H, W, pixels=([10], [20]))
    length = np.linalg.norm(rec[0]['b'].astype(np.float64) - rec[0]['a'].astype(np.float64))
    assert abs(tl[0, 0] - (length + 2 * np.float64(np.float32(0.8)))) <= 1e-6 and abs(length - 80) <= 1e-3
    # the clip at t >= 0: a bead about the source gives r on every ray; one behind it gives nothing
    _, tl = T.add([T.records([(np.zeros(3), np.zeros(3), 3.0, 1.0)]), T.records([(-50 * u, -50 * u, 3.0, 1.0)])], q32, H, W)
    assert np.abs(tl[0] - 3.0).max() <= 1e-12 and not tl[1].any()
    # records that contribute nothing: r = 0, r < 0, a field that is not finite
    bad = T.records([(ctr, ctr, 0.75, 0.5)] * 4)
    bad['r'][0], bad['r'][1], bad['a'][2, 1], bad['mu'][3] = 0, -1, np.nan, np.inf
    s, tl = T.add([bad], q32, H, W)
    assert not s.any() and not tl.any()
    # the order of the sum: ascending j in the model's dtype
    s32, _ = T.model('crossing_wires', np.float32)
    assert s32.dtype == np.float32 and T.model('crossing_wires')[0].dtype == np.float64


def test_pixel_rect_is_conservative():
    """On every case no pixel with a positive chord in the model lies outside the rectangle, and the module's rule is the
    one tests/tools_ref.py states."""
    tight = 0
    for name, (g, views) in T.cases().items():
        Q, H, W = T.grid(g)
        grid = drr.Grid(Q, H, W)
        for caps in views:
            for cap in caps:
                rect = tools.pixel_rect(tools.Capsule(*cap), grid)
                assert rect == T.pixel_rect(cap, Q, H, W), (name, rect)
                for dt in (np.float64, np.float32):
                    _, tl = T.add([T.records([cap])], Q.astype(np.float32), H, W, dt)
                    rows, cols = np.nonzero(tl[0] > 0)
                    assert rows.size and rows.min() >= rect[1] and rows.max() <= rect[3] and cols.min() >= rect[0] and cols.max() <= rect[2], (name, rect)
                tight += (rect[2] - rect[0] + 1) * (rect[3] - rect[1] + 1) < H * W
    assert tight >= 60                                                   # the short wires and beads are really culled
    Q, H, W = T.grid('full')
    grid = drr.Grid(Q, H, W)
    assert tools.pixel_rect(tools.Capsule(*T.cases()['wire_through_source_plane'][1][0][0]), grid) == (0, 0, W - 1, H - 1)
    assert tools.pixel_rect(tools.Capsule([0, 0, -2.0], [0, 0, -2.0], 2.0, 1.0), grid) == (0, 0, W - 1, H - 1)
    far = 800.0 * (Q @ np.array([500.0, 10.0, 1.0]))
    assert tools.pixel_rect(tools.Capsule(far, far, 1.0, 1.0), grid) == (0, 0, -1, -1)
    recs = tools.pack([[tools.Capsule(far, far, 1.0, 1.0)], []], grid)
    assert recs.shape == (2, 1) and recs.dtype == tools.TOOL_DTYPE and recs['r'][1, 0] == 0 and recs['rect'][1, 0].tolist() == [0, 0, -1, -1]
    assert tools.pack([[tools.Capsule(far, far, 1.0, 1.0)]], grid, cull=False)['rect'][0, 0].tolist() == [0, 0, W - 1, H - 1]


def test_capsules_are_validated():
    ok = tools.Capsule([1, 2, 3], [4, 5, 6], 1.5, 0.0)
    assert ok.row().tolist() == [1, 2, 3, 4, 5, 6, 1.5, 0.0] and ok.row().dtype == np.float64
    again = tools.Capsule.from_row(ok.row())
    assert np.array_equal(again.row(), ok.row())
    for bad, word in ((dict(r=0.0), 'positive'), (dict(r=-1.0), 'positive'), (dict(mu=-0.1), 'negative'), (dict(r=np.nan), 'finite'),
                      (dict(mu=np.inf), 'finite'), (dict(a=[0, np.nan, 0]), 'finite'), (dict(b=[0, 0]), 'three')):
        with pytest.raises(nat.DflError, match=word):
            tools.Capsule(**dict(dict(a=[0, 0, -800], b=[1, 0, -800], r=1.0, mu=0.5), **bad))
    with pytest.raises(nat.DflError, match='8 numbers'):
        tools.Capsule.from_row(np.zeros(7))
    grid = _grid('full')
    with pytest.raises(nat.DflError, match='at most 64'):
        tools.pack([[ok] * 65], grid)
    with pytest.raises(nat.DflError, match='Capsule'):
        tools.pack([[(1, 2, 3)]], grid)


def _lands():
    S = D.scene('tilted')
    lands = {n: (S['I2P'] @ np.array(c + (1.0,)))[:3] for n, (c, _, _) in zip(pp.LAND_ORDER[:6], D.ELLIPSOIDS)}
    return S, lands, tools.lands_in_camera(S['E'], S['poses'][0], lands)


def test_sample_tools_repeats_and_takes_a_fixed_count_of_draws():
    S, lands, cam = _lands()
    # the landmarks in the camera frame project where drr.project puts them
    uv = drr.project(S['K'], S['E'], S['poses'][0], list(lands.values()))
    P = np.linalg.inv(S['Q'])
    assert np.abs((P @ cam.T)[:2] / (P @ cam.T)[2] - uv).max() <= 1e-9 and (cam[:, 2] < -700).all()
    a = tools.sample_tools(np.random.default_rng([4, 0, 1, 2]), cam, 8)
    b = tools.sample_tools(np.random.default_rng([4, 0, 1, 2]), cam, 8)
    assert len(a) == len(b) and all(np.array_equal(x.row(), y.row()) for x, y in zip(a, b))
    # whatever the kinds turn out to be, the stream is left at the same place: all beads, all wires, the default mix
    counts, nexts = [], []
    for prob in (0.0, 1.0, 0.25):
        rng = np.random.default_rng(71)
        caps = tools.sample_tools(rng, cam, 8, bead_prob=prob)
        counts.append(len(caps))
        nexts.append(rng.random())
        beads = [np.array_equal(cap.a, cap.b) for cap in caps]
        assert all(beads) if prob == 1.0 else not any(beads) if prob == 0.0 else True
    rng = np.random.default_rng(71)
    n = int(rng.integers(0, 9))
    for _ in range(n):
        rng.random(tools.UNIFORMS_PER_TOOL)
        rng.standard_normal(tools.NORMALS_PER_TOOL)
    assert counts == [n] * 3 and n >= 1 and nexts == [rng.random()] * 3
    # the statistics of the defaults
    rng = np.random.default_rng(5)
    caps, sizes = [], []
    for _ in range(400):
        got = tools.sample_tools(rng, cam, 5)
        sizes.append(len(got))
        caps += got
    assert set(sizes) == set(range(6)) and abs(np.mean(sizes) - 2.5) < 0.3
    beads = [c for c in caps if np.array_equal(c.a, c.b)]
    wires = [c for c in caps if not np.array_equal(c.a, c.b)]
    assert abs(len(beads) / len(caps) - 0.25) < 0.05 and all(c.r == 0.75 for c in beads) and all(c.mu == 0.5 for c in caps)
    lens = np.array([np.linalg.norm(c.b - c.a) for c in wires])
    rad = np.array([c.r for c in wires])
    assert 60 <= lens.min() < 70 and 210 < lens.max() <= 220 and 0.5 <= rad.min() < 0.6 and 1.5 < rad.max() <= 1.6
    near = np.array([np.linalg.norm(cam - c.a, axis=1).min() for c in beads])
    assert 20 < near.mean() < 60                                         # sigma 30 per axis about some landmark
    dirs = np.array([(c.b - c.a) / np.linalg.norm(c.b - c.a) for c in wires])
    assert np.abs(dirs.mean(0)).max() < 0.1
    assert tools.sample_tools(np.random.default_rng(1), cam, 0) == []
    for kw, word in ((dict(max_tools=65), 'max_tools'), (dict(bead_prob=1.5), 'parameters'), (dict(length_mm=(5.0, 2.0)), 'parameters'),
                     (dict(wire_radius_mm=(0.0, 1.0)), 'parameters'), (dict(tool_mu=-1.0), 'parameters')):
        with pytest.raises(nat.DflError, match=word):
            tools.sample_tools(np.random.default_rng(1), cam, **dict(dict(max_tools=3), **kw))
    with pytest.raises(nat.DflError, match='landmark'):
        tools.sample_tools(np.random.default_rng(1), np.zeros((0, 3)), 3)


def test_the_pose_plan_does_not_depend_on_tools():
    """The tool stream is its own generator: sample_poses gives the same plan whether or not tools are drawn in between."""
    S, lands, cam = _lands()
    seeds = [dict(zip(drr.POSES, S['poses']))]
    kw = dict(rot_sigma_deg=2.0, trans_sigma_mm=(1.0, 1.0, 5.0), femur_sigma_deg=2.0)
    plain = synth.sample_poses(6, 0, 'x', seeds, 4, S['K'], S['E'], lands, 45, 61, 2, **kw)
    drawn = [tools.sample_tools(synth.tool_rng(6, 0, n), cam, 8) for n in range(4)]
    again = synth.sample_poses(6, 0, 'x', seeds, 4, S['K'], S['E'], lands, 45, 61, 2, **kw)
    assert all(np.array_equal(p[0][k], q[0][k]) for p, q in zip(plain, again) for k in drr.POSES) and [p[1:] for p in plain] == [q[1:] for q in again]
    assert sum(len(d) for d in drawn) >= 4
    rows = [np.stack([c.row() for c in d]) for d in drawn if d]
    assert not np.array_equal(rows[0][0], rows[1][0])                    # every view has its own stream
    other = tools.sample_tools(synth.tool_rng(7, 0, 0), cam, 8)
    assert not (len(other) == len(drawn[0]) and all(np.array_equal(x.row(), y.row()) for x, y in zip(other, drawn[0])))
    # the stream is the documented one
    want = tools.sample_tools(np.random.default_rng([6, 0, 1, 2]), cam, 8)
    assert len(want) == len(drawn[2]) and all(np.array_equal(x.row(), y.row()) for x, y in zip(want, drawn[2]))


def test_command_line():
    import synthesize_dataset as cli
    a = cli.parse_args(['full.h5', 'synth.h5'])
    assert (a.tools, a.tool_mu, a.tool_anchor_sigma_mm, a.tool_length_mm, a.tool_radius_mm, a.bead_prob, a.tool_mask) == \
        (0, 0.5, 30.0, (60.0, 220.0), (0.5, 1.6), 0.25, False)
    D_ = tools.TOOL_DEFAULTS
    assert (a.tool_mu, a.tool_anchor_sigma_mm, a.tool_length_mm, a.tool_radius_mm, a.bead_prob) == \
        (D_['tool_mu'], D_['anchor_sigma_mm'], D_['length_mm'], D_['wire_radius_mm'], D_['bead_prob'])
    assert (a.views, a.seed, a.layout, a.crop, a.ds_factor, a.chunk, a.no_noise) == (200, 0, 'preprocessed', 50, 8, 8, False)
    a = cli.parse_args(['full.h5', 'synth.h5', '--tools', '8', '--tool-mu', '0.3', '--tool-anchor-sigma-mm', '12', '--tool-length-mm', '40,90',
                        '--tool-radius-mm', '0.4,0.9', '--bead-prob', '0.5', '--tool-mask', '--views', '3'])
    assert (a.tools, a.tool_mu, a.tool_anchor_sigma_mm, a.tool_length_mm, a.tool_radius_mm, a.bead_prob, a.tool_mask, a.views) == \
        (8, 0.3, 12.0, (40.0, 90.0), (0.4, 0.9), 0.5, True, 3)
    for bad in (['--tools', '-1'], ['--tools', '65'], ['--tools', 'x'], ['--tool-mu', '-1'], ['--tool-anchor-sigma-mm', '-2'],
                ['--tool-length-mm', '5'], ['--tool-length-mm', '9,3'], ['--tool-radius-mm', '0,1'], ['--tool-radius-mm', '1,2,3'],
                ['--bead-prob', '1.5'], ['--bead-prob', '-0.1']):
        with pytest.raises(SystemExit):
            cli.parse_args(['full.h5', 'synth.h5'] + bad)
    assert '--tools' in cli.__doc__ and '--tool-mask' in cli.__doc__
    with pytest.raises(nat.DflError, match='tools must be'):
        synth.synthesize('a.h5', 'b.h5', 3, tools=65)
    with pytest.raises(nat.DflError, match='unknown tool option'):
        synth.synthesize('a.h5', 'b.h5', 3, tools=2, tool_options=dict(alloy='steel'))


def test_the_drr_example_takes_tools_from_a_file(capsys):
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import full_res_drr as cli
    assert cli.parse_tools(['f.h5', '17-1882', '3']) == (['f.h5', '17-1882', '3'], None)
    assert cli.parse_tools(['f.h5', '--tools-from', 'synth.h5', '17-1882', '3', '--crop', '0']) == (['f.h5', '17-1882', '3', '--crop', '0'], 'synth.h5')
    for bad in (['f.h5', '17-1882', '3', '--tools-from'], ['f.h5', '17-1882', '3', '--tools-from', '--compare'],
                ['f.h5', '17-1882', '3', '--tools-from', 'a.h5', '--tools-from', 'b.h5']):
        assert cli.parse_tools(bad) is None and cli.main(bad) == 1
        assert '[--tools-from FILE]' in capsys.readouterr().out
    assert '--tools-from' in cli.__doc__


def test_struct_mirror_and_symbol():
    L = nat.lib()
    for cls, size in ((nat.ToolsCapsule, 48), (nat.ToolsArgs, 80)):
        assert L.dfl_sizeof(nat._SIZEOF_ORDER.index(cls)) == C.sizeof(cls) == size
    k = nat._SIZEOF_ORDER.index(nat.ExposeArgs)
    assert nat._SIZEOF_ORDER[k + 1:k + 3] == [nat.ToolsCapsule, nat.ToolsArgs] and nat._SIZEOF_ORDER[-1] is nat.OptimPackArgs
    assert 'dfl_drr_tools' in nat.EXPORTS and hasattr(L, 'dfl_drr_tools') and nat.TOOLS_MAX == T.MAX_TOOLS == 64
    header = open(os.path.join(ROOT, 'include', 'dfl_hip.h')).read()
    assert 'int dfl_drr_tools(const dfl_tools_args* a, dfl_stream_t stream);' in header and '#define DFL_TOOLS_MAX 64' in header
    assert ' * Tools: ' in header and '|u_perp|^2 <= 1e-10' in header and T.PARALLEL == 1e-10
    body = header[header.index('} dfl_tools_capsule;'):header.index('} dfl_tools_args;')]
    names = re.findall(r'(\w+)(?:\[[^\]]*\])?\s*[;,]', re.sub(r'/\*.*?\*/', '', body.split('typedef struct {')[1], flags=re.S))
    assert names == [n for n, _ in nat.ToolsArgs._fields_] == ['att', 'tool_len', 'tools', 'qscale', 'views', 'H', 'W', 'n_tools', 'reserved']
    assert [n for n, _ in nat.ToolsCapsule._fields_] == list(tools.TOOL_DTYPE.names)
    assert [tools.TOOL_DTYPE.fields[n][1] for n in tools.TOOL_DTYPE.names] == [getattr(nat.ToolsCapsule, n).offset for n in tools.TOOL_DTYPE.names]
    build = open(os.path.join(ROOT, 'deepfluorolabeling-ipcai2020_amd', 'csrc', 'build.sh')).read()
    assert build.count('drr_tools.hip') >= 2 and re.search(r'case "\$s" in [^)]*drr_tools\.hip[^)]*\) extra="-ffp-contract=off"', build)
    src = open(os.path.join(ROOT, 'deepfluorolabeling-ipcai2020_amd', 'csrc', 'drr_tools.hip')).read()
    assert 'TOOLS_PARALLEL = 1e-10f' in src
    assert dfl_amd.tools is tools and 'tools' in dfl_amd.__all__


def test_c_abi_refuses_before_it_launches():
    L = nat.lib()
    P = 4096                                                  # never dereferenced: the checks come first
    q = D.scene('tilted')['Q'].astype(np.float32).reshape(-1)

    def mk(**k):
        k = dict(dict(att=P, tool_len=P, tools=P, views=2, H=9, W=11, n_tools=3, qscale=q), **k)
        k['qscale'] = (nat.f32 * 9)(*k['qscale'])
        return nat.ToolsArgs(**k)

    def q_with(i, v):
        out = q.copy()
        out[i] = v
        return out

    for kw, word in ((dict(att=None), b'att'), (dict(tools=None), b'tools array'), (dict(views=0), b'views'), (dict(views=65536), b'views'),
                     (dict(H=0), b'sizes'), (dict(W=0), b'sizes'), (dict(H=46341, W=46341), b'2^31'), (dict(n_tools=-1), b'n_tools'),
                     (dict(n_tools=65), b'n_tools'), (dict(qscale=q_with(4, np.nan)), b'finite'), (dict(qscale=q_with(8, np.inf)), b'finite'),
                     (dict(qscale=q_with(0, -np.inf)), b'finite')):
        a = mk(**kw)
        assert L.dfl_drr_tools(C.addressof(a), None) == -1, kw
        assert word in L.dfl_last_error() and b'dfl_drr_tools' in L.dfl_last_error(), (kw, L.dfl_last_error())
    assert L.dfl_drr_tools(None, None) == -1 and b'null' in L.dfl_last_error()
    # no capsule: success, nothing launched, no pointer read -- also without the array
    for kw in (dict(n_tools=0), dict(n_tools=0, tools=None, tool_len=None)):
        a = mk(**kw)
        assert L.dfl_drr_tools(C.addressof(a), None) == 0, kw


def test_cpu_tensors_are_refused():
    grid = _grid('window')
    cap = tools.Capsule([0, 0, -800], [5, 0, -800], 1.0, 0.5)
    with pytest.raises(nat.DflError, match='GPU'):
        tools.add_tools(torch.zeros(1, 5, 7), grid, [[cap]])
    with pytest.raises(nat.DflError, match='GPU'):
        tools.add_tools(np.zeros((1, 5, 7), np.float32), grid, [[cap]])
    with pytest.raises(nat.DflError, match='GPU'):
        tools.tools_args(torch.zeros(1, 5, 7), grid, tools.pack([[cap]], grid))


def test_the_committed_floors():
    """tests/golden/floors/tools.json is what tests/tools_floor.py measures, every case is there, and every floor is far
    below 0.1 mm: the vector form of the perpendicular offset, not the difference of squares."""
    doc = FL.load()
    assert doc['bar_factor'] == FL.BAR_FACTOR == 8.0
    now = FL.measure()
    assert sorted(now) == sorted(doc['floors']) == sorted(T.cases()) and len(now) == 10
    for key, e in now.items():
        for name, v in e.items():
            assert abs(v - doc['floors'][key][name]) <= 0.05 * doc['floors'][key][name], (key, name, v)
        assert 0 < doc['floors'][key]['tool_len'] < 0.1 and 0 < doc['floors'][key]['att'] < 0.1, key
    views = {k: len(v) for k, (_, v) in T.cases().items()}
    assert views['three_views'] == 3 and [len(v) for v in T.cases()['three_views'][1]] == [0, 1, 5] and len(T.cases()['many_short_wires'][1][0]) == 64
    assert T.grid('window')[1:] == (5, 7) and T.grid('full')[1:] == (45, 61)
    # the parallel branch is really taken in the wire_along_ray case, in both precisions, and the clip in its case
    g, v = T.cases()['wire_along_ray']
    Q, H, W = T.grid(g)
    rec = T.records(v[0])[0]
    for dt in (np.float32, np.float64):
        u, _ = T.rays(Q.astype(np.float32), H, W, dt, pixels=([20], [25]))
        w = rec['b'].astype(dt) - rec['a'].astype(dt)
        e = w / np.sqrt((w * w).sum())
        ue = sum(u[k][0] * e[k] for k in range(3))
        assert sum((u[k][0] - ue * e[k]) ** 2 for k in range(3)) <= T.PARALLEL
    assert T.model('wire_along_ray')[1][0, 20, 25] > 81 and T.model('wire_through_source_plane')[1].max() > 700
