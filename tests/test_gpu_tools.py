"""dfl_drr_tools on the GPU (csrc/drr_tools.hip) against tests/tools_ref.py, the numpy restatement of include/dfl_hip.h
("Tools") and DESIGN.md section 27, on the cases of that file: the 45 x 61 grid of the tilted scene and a 5 x 7 window.

Bars: what the launch adds to zeros, and tool_len, lie within 8 x the floors of tests/golden/floors/tools.json -- the
largest |float32 model - float64 model| of the same case (tests/tools_floor.py; both sides the model, never the kernel) --
of the float64 model, every pixel of every view.  Everything else is bit for bit: the in-place sum, culling on and off,
repeated runs, a view alone and in a batch, records that must contribute nothing, refusals.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
import tools_floor as FL  # noqa: E402
import tools_ref as T  # noqa: E402
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, drr, tools  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
_RUNS = {}


def _grid(name):
    Q, H, W = T.grid(T.cases()[name][0])
    return drr.Grid(Q, H, W)


def _caps(name):
    return [[tools.Capsule(*cap) for cap in view] for view in T.cases()[name][1]]


def _field(name):
    """A non-zero field to add to: float32 [V, H, W] in 0..6, the same on every call."""
    grid = _grid(name)
    rng = np.random.default_rng(17)
    return rng.uniform(0, 6, (len(T.cases()[name][1]), grid.H, grid.W)).astype(np.float32)


def _run(name, cull=True, base=None):
    """(att, tool_len) as numpy of one launch on zeros (or on `base`); launches on zeros are made once and shared."""
    key = (name, cull)
    if base is None and key in _RUNS:
        return _RUNS[key]
    grid = _grid(name)
    V = len(T.cases()[name][1])
    att = torch.zeros((V, grid.H, grid.W), dtype=torch.float32, device=DEV) if base is None else torch.from_numpy(base.copy()).to(DEV)
    tl = tools.add_tools(att, grid, _caps(name), want_len=True, cull=cull)
    out = att.cpu().numpy(), tl.cpu().numpy()
    if base is None:
        for a in out:
            a.setflags(write=False)
        _RUNS[key] = out
    return out


@pytest.mark.parametrize('name', sorted(T.cases()))
def test_every_case_within_its_bar(name):
    s64, l64 = T.model(name)
    att, tl = _run(name)
    assert att.shape == s64.shape == tl.shape and att.dtype == tl.dtype == np.float32
    e_att, e_len = np.abs(att.astype(np.float64) - s64).max(), np.abs(tl.astype(np.float64) - l64).max()
    print('tools %s: att max |error| %.3e (bar %.3e), tool_len %.3e (bar %.3e), largest chord %.3f mm'
          % (name, e_att, FL.bar(name, 'att'), e_len, FL.bar(name, 'tool_len'), l64.max()))
    assert e_att <= FL.bar(name, 'att') and e_len <= FL.bar(name, 'tool_len')
    assert (l64 > 0).any()


@pytest.mark.parametrize('name', ['three_views', 'window', 'many_short_wires'])
def test_the_sum_is_made_in_place(name):
    base = _field(name)
    s, tl0 = _run(name)
    att, tl = _run(name, base=base)
    assert np.array_equal(att.view(np.uint32), (base + s).astype(np.float32).view(np.uint32))      # float32(old + s), one rounding
    assert np.array_equal(tl.view(np.uint32), tl0.view(np.uint32))
    assert (s > 0).any() and np.array_equal(s > 0, tl0 > 0)
    if name == 'three_views':                                             # a view with no capsule keeps its bits
        assert not s[0].any() and not tl0[0].any() and np.array_equal(att[0].view(np.uint32), base[0].view(np.uint32))


@pytest.mark.parametrize('name', sorted(T.cases()))
def test_culling_and_repeats_do_not_move_a_bit(name):
    att, tl = _run(name)
    full_att, full_tl = _run(name, cull=False)
    assert np.array_equal(att.view(np.uint32), full_att.view(np.uint32)) and np.array_equal(tl.view(np.uint32), full_tl.view(np.uint32))
    grid = _grid(name)
    again = torch.zeros(att.shape, dtype=torch.float32, device=DEV)
    tl2 = tools.add_tools(again, grid, _caps(name), want_len=True)
    assert np.array_equal(again.cpu().numpy().view(np.uint32), att.view(np.uint32)) and np.array_equal(tl2.cpu().numpy().view(np.uint32), tl.view(np.uint32))
    # without tool_len the sum has the same bits, and nothing is returned
    bare = torch.zeros(att.shape, dtype=torch.float32, device=DEV)
    assert tools.add_tools(bare, grid, _caps(name)) is None
    assert np.array_equal(bare.cpu().numpy().view(np.uint32), att.view(np.uint32))


@pytest.mark.parametrize('name', ['three_views', 'window'])
def test_a_view_alone_has_the_bits_it_has_in_the_batch(name):
    att, tl = _run(name)
    grid = _grid(name)
    one = torch.zeros((1, grid.H, grid.W), dtype=torch.float32, device=DEV)
    tl1 = tools.add_tools(one, grid, _caps(name)[1:2], want_len=True)
    assert np.array_equal(one[0].cpu().numpy().view(np.uint32), att[1].view(np.uint32)) and att[1].any()
    assert np.array_equal(tl1[0].cpu().numpy().view(np.uint32), tl[1].view(np.uint32))


def _launch(att, grid, recs, want_len=True):
    a, tl, keep = tools.tools_args(att, grid, recs, want_len)
    nat.call('dfl_drr_tools', a, torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize(DEV)
    del keep
    return tl


def test_padding_and_records_that_are_not_finite_contribute_nothing():
    name = 'crossing_wires'
    att, tl = _run(name)
    grid = _grid(name)
    clean = tools.pack(_caps(name), grid)
    whole = (0, 0, grid.W - 1, grid.H - 1)
    recs = np.zeros((1, 8), tools.TOOL_DTYPE)
    recs[0, 1], recs[0, 5] = clean[0, 0], clean[0, 1]                      # the order of the two real records is kept
    for j, (field, value) in ((0, ('r', 0.0)), (2, ('r', -1.0)), (3, ('r', np.nan)), (4, ('mu', np.inf)), (6, ('a', np.nan)), (7, ('b', -np.inf))):
        recs[0, j] = clean[0, j % 2]
        recs['rect'][0, j] = whole
        recs[field][0, j] = value
    got = torch.zeros((1, grid.H, grid.W), dtype=torch.float32, device=DEV)
    got_tl = _launch(got, grid, recs)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), att.view(np.uint32)) and np.array_equal(got_tl.cpu().numpy().view(np.uint32), tl.view(np.uint32))
    # a rectangle that is empty, or that lies outside the image, skips the capsule and reads nothing out of bounds
    recs = clean.copy()
    recs['rect'][0, 0] = (0, 0, -1, -1)
    recs['rect'][0, 1] = (grid.W + 100, grid.H + 100, grid.W + 200, grid.H + 200)
    got = torch.zeros((1, grid.H, grid.W), dtype=torch.float32, device=DEV)
    got_tl = _launch(got, grid, recs)
    assert not got.cpu().numpy().any() and not got_tl.cpu().numpy().any()
    # no capsule in any view: nothing is launched, att keeps its bits, tool_len is zero
    base = _field(name)
    att0 = torch.from_numpy(base.copy()).to(DEV)
    tl0 = tools.add_tools(att0, grid, [[]], want_len=True)
    assert np.array_equal(att0.cpu().numpy().view(np.uint32), base.view(np.uint32)) and not tl0.cpu().numpy().any()


def test_refusals_leave_the_outputs_untouched():
    L = nat.lib()
    name = 'window'
    grid = _grid(name)
    V = 2
    att = torch.full((V, grid.H, grid.W), 7.0, dtype=torch.float32, device=DEV)
    tl = torch.full((V, grid.H, grid.W), -3.0, dtype=torch.float32, device=DEV)
    recs = tools.pack(_caps(name), grid)
    d_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1)).to(DEV)
    q = grid.Q.astype(np.float32).reshape(-1)
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def mk(**k):
        k = dict(dict(att=att.data_ptr(), tool_len=tl.data_ptr(), tools=d_recs.data_ptr(), views=V, H=grid.H, W=grid.W,
                      n_tools=recs.shape[1], qscale=q), **k)
        k['qscale'] = (nat.f32 * 9)(*k['qscale'])
        return nat.ToolsArgs(**k)

    def q_with(i, v):
        out = q.copy()
        out[i] = v
        return out

    for kw, word in ((dict(att=None), b'att'), (dict(tools=None), b'tools array'), (dict(views=0), b'views'), (dict(views=65536), b'views'),
                     (dict(H=0), b'sizes'), (dict(W=-1), b'sizes'), (dict(H=46341, W=46341), b'2^31'), (dict(n_tools=-1), b'n_tools'),
                     (dict(n_tools=65), b'n_tools'), (dict(qscale=q_with(2, np.nan)), b'finite'), (dict(qscale=q_with(6, np.inf)), b'finite')):
        a = mk(**kw)
        assert L.dfl_drr_tools(C.addressof(a), stream) == -1, kw
        assert word in L.dfl_last_error() and b'dfl_drr_tools' in L.dfl_last_error(), (kw, L.dfl_last_error())
    assert L.dfl_drr_tools(None, stream) == -1 and b'null' in L.dfl_last_error()
    a = mk(n_tools=0)
    assert L.dfl_drr_tools(C.addressof(a), stream) == 0                     # no capsule: nothing launched
    torch.cuda.synchronize(DEV)
    assert bool((att == 7.0).all()) and bool((tl == -3.0).all())
    a = mk()                                                               # and the same block, unchanged, is accepted
    assert L.dfl_drr_tools(C.addressof(a), stream) == 0
    torch.cuda.synchronize(DEV)
    s, tl_want = _run(name)
    assert np.array_equal(att.cpu().numpy(), (np.float32(7.0) + s).astype(np.float32)) and np.array_equal(tl.cpu().numpy(), tl_want)
    # the Python entry point, in DflError's words
    caps = _caps(name)
    z = torch.zeros((V, grid.H, grid.W), dtype=torch.float32, device=DEV)
    for bad, word in ((lambda: tools.add_tools(z.cpu(), grid, caps), 'GPU'), (lambda: tools.add_tools(z[0], grid, caps), 'lists of capsules'),
                      (lambda: tools.add_tools(z, grid, caps[:1]), 'lists of capsules'), (lambda: tools.add_tools(z.double(), grid, caps), 'float32'),
                      (lambda: tools.add_tools(z[:, :, :5], grid, caps), 'contiguous'),
                      (lambda: tools.add_tools(torch.zeros((V, 6, 7), dtype=torch.float32, device=DEV), grid, caps), 'the grid'),
                      (lambda: tools.add_tools(z, grid, [caps[0] * 33, []]), 'at most 64')):
        with pytest.raises(nat.DflError, match=word):
            bad()
    assert not z.cpu().numpy().any()
