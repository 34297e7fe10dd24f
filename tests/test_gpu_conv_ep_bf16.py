"""The row epilogue the two patch-resident bf16 kernels share (csrc/conv_ep_bf16.h): where convp_bf16.hip and convq_bf16.hip sum in
the same order, they now agree BIT FOR BIT -- in y and in the statistics rows -- under every epilogue case.

The shape is the smallest on which both kernels run one workgroup per column block with the same decomposition: N = 1, 32 -> 32
channels, 12 x 12 (and 13 x 12: a ragged last patch row), 3 x 3 / pad 1.  K = 288 is ONE resident channel block, so every output
element is one k loop -- taps outside, 16-channel chunks inside -- in convp as in convq.  convp's tile 12 (4 x 1 waves, three
32-row tiles each, 32 columns) over a 12-wide patch and convq's layout 46 (4 x 1 waves of 96 pixels, 32 columns) then give thread
(row, unit) the same pixels in the same order and reduce 64 row-threads in the same order: equal accumulators must give equal
bits everywhere.  Layout 48 (two k-groups: the chunk halves meet in LDS) sums in another order and is held to the fp64 bar and to
repeatability only.  pytest -m gpu."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dfl_amd import _native as nat
import problems as PR
from test_gpu_bf16 import rb, nhwc, pack16, conv_bf16, _mode4  # noqa: F401
from test_gpu_convq import close_bf16

pytestmark = pytest.mark.gpu
CIN = 32
P_TILE, Q_TILE, Q_TILE_2G = 12, 46, 48           # csrc/convp_bf16.hip convp_tiles()[12] = {4, 1, 3, 1}; csrc/convq_bf16.hip layouts 6 and 8
CASES = ('plain', 'relu_stats', 'add_given', 'add_live', 'accumulate', 'stat_other')
EPS = 1e-5


class forced:
    def __init__(self, geom):
        self.g = (C.c_int32 * 5)(*geom)

    def __enter__(self):
        nat.check(nat.lib().dfl_conv_force_geometry(C.addressof(self.g)), 'force')

    def __exit__(self, *exc):
        nat.lib().dfl_conv_force_geometry(None)


def geoms(H):
    """One patch over the whole image in either kernel: (tile, images per patch, patch rows, patch columns, K slices)."""
    return {'convp': (P_TILE, 1, H, 12, 1), 'convq': (Q_TILE, 1, 32, 12, 1), 'convq2': (Q_TILE_2G, 1, 32, 12, 1)}


# 40 columns take 64-column blocks: convp's tile 3 = {2, 2, 3, 1} and convq's layout 43 (2 x 2 waves) -- again the same rows per thread
GEOMS_40 = {'convp': (3, 1, 12, 12, 1), 'convq': (43, 1, 16, 12, 1)}


_PROBLEMS = {}


def problem(H, Cout):
    """Operands and the fp64 reference of every case, once per shape."""
    if (H, Cout) in _PROBLEMS:
        return _PROBLEMS[(H, Cout)]
    W = 12
    g = torch.Generator().manual_seed(1000 + 10 * H + Cout)
    x = rb(torch.randn(1, CIN, H, W, generator=g))
    w = rb(torch.randn(Cout, CIN, 3, 3, generator=g) / (CIN * 9) ** 0.5)
    b = torch.randn(Cout, generator=g)
    other = rb(torch.randn(1, Cout, H, W, generator=g))
    asc, ash = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.2
    y0 = rb(torch.randn(1, Cout, H, W, generator=g))
    partner = rb(torch.randn(1, Cout, H, W, generator=g))
    # live totals of `add`: row 0 carries the sums of a batch of `count` values per channel, the other rows nothing; the scale and
    # shift the kernel derives from them, in its own arithmetic (csrc/common.h bn_live_affine)
    count = 4096.0
    gam, bet = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.2
    mean, var = torch.randn(Cout, generator=g).double() * 0.2, torch.rand(Cout, generator=g).double() + 0.5
    tot = torch.zeros(8, 2, Cout, dtype=torch.float64)
    tot[0, 0], tot[0, 1] = mean * count, (var + mean * mean) * count
    m = tot[:, 0].sum(0) / count
    v = (tot[:, 1].sum(0) / count - m * m).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(v + float(np.float32(EPS)))
    lsc, lsh = (gam.double() * invstd).float(), (bet.double() - m * gam.double() * invstd).float()
    conv = F.conv2d(x.double(), w.double(), padding=1)
    cb = conv + b.double().view(1, -1, 1, 1)
    aff = lambda sc, sh: other.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
    kw = {
        'plain': dict(),
        'relu_stats': dict(bias=b, relu=1, stats=True),
        'add_given': dict(bias=b, add=other, add_aff=(asc, ash), stats=True),
        'add_live': dict(bias=b, add=other, add_live=(tot, gam, bet, count, EPS), stats=True),
        'accumulate': dict(bias=b, y_init=y0, accumulate=1, stats=True),
        'stat_other': dict(bias=b, relu=1, stats=True, stat_other=partner),
    }
    ref = {
        'plain': conv, 'relu_stats': F.relu(cb), 'add_given': cb + aff(asc, ash), 'add_live': cb + aff(lsc, lsh),
        'accumulate': cb + y0.double(), 'stat_other': F.relu(cb),
    }
    pr = dict(x=x, wp=pack16(w, 1), kw=kw, ref={k: nhwc(r) for k, r in ref.items()}, partner=nhwc(partner).double(), H=H, W=W, Cout=Cout)
    _PROBLEMS[(H, Cout)] = pr
    return pr


def launch(pr, case, geom, ldy=None):
    """y with all its ldy channels, the statistics rows as written (None without statistics)."""
    kw = dict(pr['kw'][case])
    with forced(geom):
        out = conv_bf16(pr['x'], pr['wp'], pr['Cout'], 3, 3, 1, 1, pr['H'], pr['W'], force_splits=1, whole=True, ldy=ldy,
                        stats_fill=float('nan'), **kw)
    return out if kw.get('stats') else (out, None)


def check_against_fp64(pr, case, y, st, what):
    Cout = pr['Cout']
    close_bf16(y[..., :Cout], pr['ref'][case], what)
    if st is None:
        return
    assert not bool(torch.isnan(st).any()), '%s: a statistics row was not written' % what
    yd = y[..., :Cout].double().reshape(-1, Cout)
    ud = pr['partner'].reshape(-1, Cout) if case == 'stat_other' else yd
    s = st.double().sum(0)
    np.testing.assert_allclose(s[0].numpy(), yd.sum(0).numpy(), rtol=2e-5, atol=2e-5 * float(yd.abs().sum(0).max()))
    np.testing.assert_allclose(s[1].numpy(), (yd * ud).sum(0).numpy(), rtol=2e-5, atol=2e-5 * float((yd * ud).abs().sum(0).max()))


def same_bits(a, b):
    """torch.equal on the bit patterns (NaN padding compares equal to itself)."""
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_the_forced_geometries_are_candidates_of_the_shape():
    """A geometry the library does not list for the shape would be a mistake in this file, not a reason to skip."""
    for H in (12, 13):
        cands = set(PR.conv_candidates(1, CIN, 32, H, 12, 3, 1, 1))
        for name, geom in geoms(H).items():
            assert geom in cands, (name, geom)
    cands = set(PR.conv_candidates(1, CIN, 40, 12, 12, 3, 1, 1))
    assert GEOMS_40['convp'] in cands and GEOMS_40['convq'] in cands


@pytest.mark.parametrize('H', [12, 13])
@pytest.mark.parametrize('case', CASES)
def test_shared_epilogue_case(case, H):
    pr = problem(H, 32)
    out = {}
    for name, geom in geoms(H).items():
        y1, st1 = launch(pr, case, geom)
        y2, st2 = launch(pr, case, geom)
        check_against_fp64(pr, case, y1, st1, '%s %s H %d' % (name, case, H))
        assert same_bits(y1, y2) and same_bits(st1, st2), '%s %s H %d: two launches differ' % (name, case, H)
        out[name] = (y1, st1)
    # one k-group in both kernels: the accumulators are the same bits (the plain case stores them rounded, nothing else) ...
    yp, _ = launch(pr, 'plain', geoms(H)['convp'])
    yq, _ = launch(pr, 'plain', geoms(H)['convq'])
    assert torch.equal(yp, yq), 'plain H %d: convp and convq sum in another order here; %d elements differ' % (H, int((yp != yq).sum()))
    # ... so the shared body leaves the same y and the same statistics rows
    (yp, sp), (yq, sq) = out['convp'], out['convq']
    assert same_bits(yp, yq), '%s H %d: y differs between convp and convq in %d elements' % (case, H, int((yp != yq).sum()))
    assert same_bits(sp, sq), '%s H %d: the statistics rows differ between convp and convq' % (case, H)


def test_units_beyond_ntot_are_left_alone():
    """40 columns: the 64-column block of either kernel holds five units inside Ntot and three beyond it.  Their columns of y (the
    pixel stride is 64) keep the NaN they were filled with; the statistics rows have 40 columns and are all written."""
    pr = problem(12, 40)
    got = {}
    for name in ('convp', 'convq'):
        y, st = launch(pr, 'add_given', GEOMS_40[name], ldy=64)
        check_against_fp64(pr, 'add_given', y, st, '%s 40 columns' % name)
        assert y.shape[-1] == 64 and bool(torch.isnan(y[..., 40:]).all()), '%s wrote beyond column 40' % name
        assert st.shape[-1] == 40
        got[name] = (y, st)
    assert same_bits(got['convp'][0], got['convq'][0]) and same_bits(got['convp'][1], got['convq'][1])
