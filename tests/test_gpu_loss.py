"""dfl_dice_ncc_loss (csrc/loss.hip) through its C ABI, at the shapes and argument forms where its three kernels branch.

Reference: fp64 autograd over the oracle's restatement of dice.py / ncc.py (oracle.ref_cpu), on the same fp32 inputs seen
through the same centre crop.  The kernels' own closed form is used for one thing only: the size of the terms a gradient
element is made of, which sets its error bar.

Bars.  Loss value: 2e-6 absolute.  ncc_vals: rtol 1e-5.  Gradients: the kernel evaluates fma(c2, q, fma(c1, p, c0)) in fp32
with coefficients that were cast from fp64 (and multiplied by the incoming gradient) -- one cast and two fmas per element,
each 2^-24 relative to the term it rounds; with a factor 2 for slack, per plane
    |got - ref| <= 8 * 2^-24 * max(|c2 q| + |c1 p| + |c0|)
with the coefficients taken in fp64.  Where a coefficient is exactly zero (a skipped background plane, a zero weight, an
all-zero target plane) the bar is zero: the gradient must be exact zeros.

Windows (h, w) at crop offset (oy, ox) of an [h + 2 oy, w + 2 ox] plane, the smallest per branch of the kernels:
    (3, 8) @ (0, 4)      h < LOSS_NS: a row range per row, the fourth empty
    (9, 12) @ (1, 4)     float4 path; row ranges of 3 rows, the last of them empty for wave 3
    (13, 10) @ (2, 3)    scalar path, ragged last lane (w % 4 = 2)
    (6, 260) @ (0, 4)    second trip of the x += 256 loop, float4
    (5, 259) @ (1, 1)    second trip, scalar, ragged
    (37, 12) @ (1, 4)    row ranges of 10 rows: a wave holds rows y and y + 4 in flight, then takes the remainder row y + 8
                         (the two-rows-in-flight loop needs more than 4 rows per range, i.e. h > 16)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import dfl_amd
from dfl_amd import _native as nat
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENT = 1234.5                      # border of the strided outputs
U = 2.0 ** -24

WINDOWS = [(3, 8, 0, 4), (9, 12, 1, 4), (13, 10, 2, 3), (6, 260, 0, 4), (5, 259, 1, 1), (37, 12, 1, 4)]
CL = [(7, 3), (2, 1), (0, 3), (7, 0), (2, 0), (0, 1), (2, 3), (7, 1)]


def stream():
    return torch.cuda.current_stream().cuda_stream


class Problem:
    """fp32 inputs of one loss call: full-size network outputs whose centre window the kernels read, dense targets."""

    def __init__(self, B, Cc, L, h, w, oy, ox, seed=0, heat_mean=0.0, heat_std=1.0, zero_target=None):
        g = torch.Generator().manual_seed(1000 * seed + 17 * h + w + 3 * Cc + L)
        self.dims = (B, Cc, L, h, w, oy, ox)
        Hp, Wp = h + 2 * oy, w + 2 * ox
        self.Hp, self.Wp = Hp, Wp
        self.seg = self.tseg = self.heat = self.theat = None
        if Cc > 0:
            self.seg = torch.softmax(2.0 * torch.randn(B, Cc, Hp, Wp, generator=g), 1).float()
            lab = torch.randint(0, Cc, (B, h, w), generator=g)
            self.tseg = R.one_hot_masks(lab, Cc).float()
        if L > 0:
            z = torch.randn(B, L, Hp, Wp, generator=g)
            self.heat = (heat_mean + heat_std * z).float()
            zc = z[..., oy:oy + h, ox:ox + w]
            self.theat = (0.6 * zc + 0.4 * torch.randn(B, L, h, w, generator=g)).float().contiguous()
            if zero_target is not None:
                self.theat[zero_target] = 0.0
        self.dev = {k: (None if v is None else v.to(DEV)) for k, v in
                    (('seg', self.seg), ('tseg', self.tseg), ('heat', self.heat), ('theat', self.theat))}
        self._ref = {}

    def window(self, t):
        B, Cc, L, h, w, oy, ox = self.dims
        return t[..., oy:oy + h, ox:ox + w]

    def reference(self, skip_bg, dice_wgt, heat_wgt, gs, dtype=torch.float64):
        """(loss, dseg, dheat, ncc) by autograd over the oracle in `dtype`; gradients as [B, C, h, w] windows."""
        key = (skip_bg, dice_wgt, heat_wgt, gs, dtype)
        if key in self._ref:
            return self._ref[key]
        B, Cc, L, h, w, oy, ox = self.dims
        seg = self.seg.to(dtype).clone().requires_grad_(True) if Cc > 0 else None
        heat = self.heat.to(dtype).clone().requires_grad_(True) if L > 0 else None
        shape = (h, w)
        ncc = None
        if Cc > 0 and L > 0 and heat_wgt > 1e-8 and abs(dice_wgt + heat_wgt - 1.0) < 1e-12:
            loss = R.dice_and_heatmap_loss_2d((R.center_crop(seg, shape), R.center_crop(heat, shape)),
                                              (self.tseg.to(dtype), self.theat.to(dtype)), skip_bg=bool(skip_bg), heatmap_wgt=heat_wgt)
        else:
            loss = torch.zeros((), dtype=dtype)
            if Cc > 0:
                loss = loss + dice_wgt * R.dice_loss_2d(R.center_crop(seg, shape), self.tseg.to(dtype), skip_bg=bool(skip_bg))
            if L > 0:
                loss = loss + heat_wgt * ((R.ncc_2d(R.center_crop(heat, shape), self.theat.to(dtype)) + 1) * -0.5).mean()
        if L > 0:
            with torch.no_grad():
                ncc = R.ncc_2d(R.center_crop(heat, shape), self.theat.to(dtype)).detach()
        loss.backward(torch.tensor(1.0 if gs is None else gs, dtype=dtype))
        outs = []
        for t in (seg, heat):
            if t is None:
                outs.append(None)
                continue
            gr = t.grad if t.grad is not None else torch.zeros_like(t)
            border = gr.clone()
            self.window(border).zero_()
            assert not bool(border.any())                                  # the crop's gradient outside the window
            outs.append(self.window(gr).contiguous())
        self._ref[key] = (loss.detach(), outs[0], outs[1], ncc)
        return self._ref[key]

    def term_bounds(self, skip_bg, dice_wgt, heat_wgt, gs):
        """Per plane max(|c2 q| + |c1 p| + |c0|) of the gradient's closed form, coefficients in fp64:
        ([B, C], [B, L]).  Sets the bar only; the expected values come from autograd."""
        B, Cc, L, h, w, oy, ox = self.dims
        gsv = 1.0 if gs is None else gs
        bs = bh = None
        if Cc > 0:
            s, t = self.window(self.seg).double(), self.tseg.double()
            I, T, S = (t * s).sum((2, 3)), (t * t).sum((2, 3)), (s * s).sum((2, 3))
            num, den = -2.0 * I + 1e-4, T + S + 1e-4
            gq = dice_wgt / (B * (Cc - (1 if skip_bg else 0)))
            a1, a2 = -2.0 / den * gq * gsv, -2.0 * num / (den * den) * gq * gsv
            if skip_bg:
                a1[:, 0] = 0.0
                a2[:, 0] = 0.0
            bs = ((a1[..., None, None] * t).abs() + (a2[..., None, None] * s).abs()).amax((2, 3))
        if L > 0:
            x, y = self.window(self.heat).double(), self.theat.double()
            N = float(h * w)
            mx, my = x.mean((2, 3), keepdim=True), y.mean((2, 3), keepdim=True)
            xz, yz = x - mx, y - my
            sdx, sdy = ((xz * xz).sum((2, 3)) / (N - 1)).sqrt(), ((yz * yz).sum((2, 3)) / (N - 1)).sqrt()
            cxy = (xz * yz).sum((2, 3))
            D = N * sdx * sdy + 1e-8
            E = cxy * N * sdy / (D * D * (N - 1) * sdx)
            q = -0.5 * heat_wgt / (B * L) * gsv
            k1, k2 = (q / D)[..., None, None], (-q * E)[..., None, None]
            k0 = -k1 * my - k2 * mx
            bh = ((k1 * y).abs() + (k2 * x).abs() + k0.abs()).amax((2, 3))
        return bs, bh


_PROBLEMS = {}


def problem(*key, **kw):
    k = key + tuple(sorted(kw.items()))
    if k not in _PROBLEMS:
        _PROBLEMS[k] = Problem(*key, **kw)
    return _PROBLEMS[k]


def odd_pitch(Wp):
    """A row stride >= Wp that is no multiple of 4."""
    return Wp + 1 if (Wp + 1) % 4 else Wp + 2


def run(p, skip_bg=0, dice_wgt=0.5, heat_wgt=0.5, gs=None, want=('seg', 'heat'), layout='dense', stages=(0,), ncc=False):
    """One dfl_dice_ncc_loss call (or a stage-1 and a stage-2 call with the same struct) on problem p.  Scratch and outputs
    start as NaN; a strided output is the window of a SENT-filled full-size tensor whose border must come back untouched.
    Returns dict(loss, dseg, dheat, ncc) of CPU tensors (None where not asked for)."""
    lib = nat.lib()
    B, Cc, L, h, w, oy, ox = p.dims
    a = nat.LossArgs()
    d = p.dev
    for name, nch in (('seg', Cc), ('heat', L)):
        if nch == 0:
            continue
        full, tgt = d[name], d['t' + name]
        win = p.window(full)
        setattr(a, name, win.data_ptr())
        setattr(a, 't' + name, tgt.data_ptr())
        for s, v in zip(('_sN', '_sC', '_sH'), win.stride()[:3]):
            setattr(a, name + s, v)
        for s, v in zip(('_sN', '_sC', '_sH'), tgt.stride()[:3]):
            setattr(a, 't' + name + s, v)
    loss = torch.full((), float('nan'), device=DEV)
    sums = torch.full((int(lib.dfl_loss_scratch_doubles(B, Cc, L)),), float('nan'), dtype=torch.float64, device=DEV)
    a.loss, a.sums = loss.data_ptr(), sums.data_ptr()
    a.B, a.C, a.L, a.h, a.w = B, Cc, L, h, w
    a.skip_bg, a.dice_wgt, a.heat_wgt = skip_bg, dice_wgt, heat_wgt
    gsd = None
    if gs is not None:
        gsd = torch.tensor([gs], dtype=torch.float32, device=DEV)
        a.grad_scale = gsd.data_ptr()
    nccd = None
    if ncc:
        nccd = torch.full((B, L), float('nan'), device=DEV)
        a.ncc_vals = nccd.data_ptr()
    outs, fulls = {}, {}
    for name, nch in (('seg', Cc), ('heat', L)):
        if name not in want or nch == 0:
            continue
        if layout == 'dense':
            o = torch.full((B, nch, h, w), float('nan'), device=DEV)
            setattr(a, 'd' + name, o.data_ptr())
            outs[name] = o
        else:
            Wq = p.Wp if layout == 'strided4' else odd_pitch(p.Wp)
            full = torch.full((B, nch, p.Hp, Wq), SENT, device=DEV)
            o = full[..., oy:oy + h, ox:ox + w]
            o.fill_(float('nan'))
            setattr(a, 'd' + name, o.data_ptr())
            for s, v in zip(('_sN', '_sC', '_sH'), o.stride()[:3]):
                setattr(a, 'd' + name + s, v)
            outs[name], fulls[name] = o, full
    for st in stages:
        a.stage = st
        nat.check(lib.dfl_dice_ncc_loss(C.addressof(a), stream()), 'dfl_dice_ncc_loss')
    torch.cuda.synchronize()
    for name, full in fulls.items():
        f = full.cpu()
        f[..., oy:oy + h, ox:ox + w] = SENT
        assert bool((f == SENT).all()), 'the border of the strided d%s was written' % name
    res = {'loss': loss.cpu(), 'ncc': None if nccd is None else nccd.cpu()}
    for name in ('seg', 'heat'):
        res['d' + name] = outs[name].cpu().contiguous() if name in outs else None
    return res


def check_grad(got, ref, bound, what):
    """Per plane |got - ref| <= 8 * 2^-24 * bound; exact zeros where the bound is zero."""
    assert got.shape == ref.shape, what
    err = (got.double() - ref).abs().amax((2, 3))
    bar = 8 * U * bound
    print('%s: worst |err| / bar %.3f' % (what, float((err / bar.clamp_min(1e-300)).max())))
    assert bool((err <= bar).all()), '%s: |err| %s over the bar %s' % (what, err.tolist(), bar.tolist())


def check(p, res, skip_bg, dice_wgt, heat_wgt, gs, what):
    loss, gseg, gheat, ncc = p.reference(skip_bg, dice_wgt, heat_wgt, gs)
    bs, bh = p.term_bounds(skip_bg, dice_wgt, heat_wgt, gs)
    assert abs(float(res['loss']) - float(loss)) < 2e-6, (what, float(res['loss']), float(loss))
    if res['dseg'] is not None:
        check_grad(res['dseg'], gseg, bs, what + ' dseg')
        if skip_bg:
            assert bool((res['dseg'][:, 0] == 0).all()), what + ': the background plane is not exact zeros'
    if res['dheat'] is not None:
        check_grad(res['dheat'], gheat, bh, what + ' dheat')
    if res['ncc'] is not None:
        np.testing.assert_allclose(res['ncc'].numpy(), ncc.numpy(), rtol=1e-5, err_msg=what)


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


@pytest.mark.parametrize('Cc,L', CL)
@pytest.mark.parametrize('h,w,oy,ox', WINDOWS)
def test_loss_kernels_per_window_and_argument_form(h, w, oy, ox, Cc, L):
    """Every window of the module docstring with C in {0, 2, 7} and L in {0, 1, 3} (B = 2): value, ncc_vals and gradients
    against fp64 autograd with skip_bg 0 / 1 and grad_scale NULL / -2.5, outputs dense, strided with the input's row stride
    (float4-compatible where the window is) and strided with a row stride that is no multiple of 4; stage 0 against stage 1
    then 2, and dseg alone / dheat alone / neither against both, bit for bit."""
    B = 2
    p = problem(B, Cc, L, h, w, oy, ox)
    dw, hw_ = (0.5, 0.5) if (Cc > 0 and L > 0) else ((1.0, 0.0) if L == 0 else (0.0, 1.0))
    for skip_bg in ((0, 1) if Cc >= 2 else (0,)):
        for gs in (None, -2.5):
            what = 'window %s C %d L %d skip_bg %d gs %s' % ((h, w, oy, ox), Cc, L, skip_bg, gs)
            kw = dict(skip_bg=skip_bg, dice_wgt=dw, heat_wgt=hw_, gs=gs)
            base = run(p, ncc=L > 0, **kw)
            check(p, base, what=what + ' dense', **kw)
            for layout in ('strided4', 'strided_odd'):
                r = run(p, layout=layout, **kw)
                check(p, r, what=what + ' ' + layout, **kw)
                # (the float4 and the scalar path of the gradient kernel do the same two fmas per element)
                assert same_bits(r['dseg'], base['dseg']) and same_bits(r['dheat'], base['dheat']) and same_bits(r['loss'], base['loss']), what + ' ' + layout
            two = run(p, stages=(1, 2), ncc=L > 0, **kw)
            for k in ('loss', 'dseg', 'dheat', 'ncc'):
                assert same_bits(two[k], base[k]), what + ': stage 1 + 2 and stage 0 differ in ' + k
            for want in (('seg',), ('heat',), ()):
                r = run(p, want=want, **kw)
                assert same_bits(r['loss'], base['loss']), what
                assert same_bits(r['dseg'], base['dseg'] if 'seg' in want else None), what + ' want %s' % (want,)
                assert same_bits(r['dheat'], base['dheat'] if 'heat' in want else None), what + ' want %s' % (want,)


def test_loss_stage_one_alone_writes_value_and_ncc_but_no_gradient():
    """Stage 1 with gradient pointers set leaves them alone (the NaN fill stays); the value and ncc_vals are final."""
    p = problem(2, 7, 3, 9, 12, 1, 4)
    r = run(p, stages=(1,), ncc=True)
    check(p, dict(r, dseg=None, dheat=None), 0, 0.5, 0.5, None, 'stage 1')
    assert bool(torch.isnan(r['dseg']).all()) and bool(torch.isnan(r['dheat']).all())


@pytest.mark.parametrize('h,w,oy,ox', [(9, 12, 1, 4), (13, 10, 2, 3)])
def test_loss_all_zero_target_heat_plane(h, w, oy, ox):
    """A landmark outside the view: its target heat map is all zero.  The reference (fp64, checked here on the CPU) gives
    NCC = 0 / (0 + 1e-8) = 0 and a gradient of exact zeros on that plane; so must the kernels (k1 = q / 1e-8 is large and
    multiplies zeros, k2 and k0 are zero)."""
    p = problem(2, 7, 3, h, w, oy, ox, zero_target=(0, 1))
    loss, gseg, gheat, ncc = p.reference(0, 0.5, 0.5, None)
    assert float(ncc[0, 1]) == 0.0 and not bool(gheat[0, 1].any()) and bool(torch.isfinite(gheat).all())
    for gs in (None, -2.5):
        for layout in ('dense', 'strided_odd'):
            r = run(p, gs=gs, ncc=True, layout=layout)
            check(p, r, 0, 0.5, 0.5, gs, 'zero target plane %s' % layout)
            assert float(r['ncc'][0, 1]) == 0.0
            assert bool((r['dheat'][0, 1] == 0).all()), 'gradient on the all-zero target plane'
            assert bool((r['dheat'][1, 1] != 0).any())


def test_loss_heat_maps_with_offset_mean():
    """Predicted heat maps with mean 10 and standard deviation 0.01: k2 x + k0 cancels to 1e-3 of its terms in fp32.  The
    gradient keeps the per-term bar of this file; its error relative to the largest gradient is also held to 4x the error
    of the oracle's own fp32 run (R.ncc_2d under fp32 autograd against fp64), which does the same arithmetic in another
    order.  Measured on the MI355X at B = 2, L = 3, errors relative to the largest |gradient|: window (9, 12) fp32 oracle
    4.3e-7, kernel 8.3e-8; window (5, 259) fp32 oracle 3.2e-7, kernel 1.9e-7.  (With the coefficients rounded to fp32 and
    nothing else, the kernel's error was 3.6e-5 and 2.9e-5: 2^-24 |k2 mx| on every pixel, which the mean subtraction of
    the reference's backward pass takes off.  The gradient kernel now adds that constant back, see csrc/loss.hip.)"""
    worst = []
    for h, w, oy, ox in ((9, 12, 1, 4), (5, 259, 1, 1)):
        p = problem(2, 0, 3, h, w, oy, ox, heat_mean=10.0, heat_std=0.01)
        loss, _, g64, ncc = p.reference(0, 0.0, 1.0, None)
        _, _, g32, _ = p.reference(0, 0.0, 1.0, None, dtype=torch.float32)
        r = run(p, dice_wgt=0.0, heat_wgt=1.0, ncc=True)
        check(p, r, 0, 0.0, 1.0, None, 'offset mean %s' % ((h, w),))
        scale = float(g64.abs().max())
        e_ref = float((g32.double() - g64).abs().max()) / scale
        e_ker = float((r['dheat'].double() - g64).abs().max()) / scale
        print('offset mean, window %s: fp32 oracle error %.3e, kernel error %.3e of the largest gradient' % ((h, w), e_ref, e_ker))
        worst.append((e_ker, e_ref))
    for e_ker, e_ref in worst:
        assert e_ker <= 4.0 * e_ref, (e_ker, e_ref)


def test_loss_ncc_values_with_zero_heat_weight():
    """ncc_vals with heat_wgt = 0 (what ncc_2d asks for at C = 0, here next to a Dice term): the values are right, the
    loss is the Dice term alone."""
    p = problem(2, 7, 3, 13, 10, 2, 3)
    r = run(p, dice_wgt=1.0, heat_wgt=0.0, ncc=True, want=('seg',))
    check(p, r, 0, 1.0, 0.0, None, 'ncc_vals at heat_wgt 0')
    p0 = problem(2, 0, 3, 13, 10, 2, 3)
    r = run(p0, dice_wgt=0.0, heat_wgt=0.0, ncc=True, want=())
    assert float(r['loss']) == 0.0
    np.testing.assert_allclose(r['ncc'].numpy(), p0.reference(0, 0.0, 1.0, None)[3].numpy(), rtol=1e-5)


@pytest.mark.parametrize('stages', [(0,), (1, 2)])
@pytest.mark.parametrize('layout', ['dense', 'strided4', 'strided_odd'])
def test_loss_zero_dice_weight_gives_exact_zero_dseg(layout, stages):
    """dice_wgt = 0 with dseg asked for (DiceAndHeatMapLoss2D(heatmap_wgt=1.0)): the reference's gradient is exact zeros.
    The scratch starts as NaN, so coefficients the finalize kernel does not write show."""
    p = problem(2, 7, 3, 9, 12, 1, 4)
    for skip_bg in (0, 1):
        for gs in (None, -2.5):
            r = run(p, skip_bg=skip_bg, dice_wgt=0.0, heat_wgt=1.0, gs=gs, layout=layout, stages=stages, ncc=True)
            assert bool((r['dseg'] == 0).all()), 'dseg at dice_wgt 0: %s' % r['dseg'].flatten()[:4].tolist()
            check(p, r, skip_bg, 0.0, 1.0, gs, 'dice_wgt 0')


@pytest.mark.parametrize('stages', [(0,), (1, 2)])
@pytest.mark.parametrize('layout', ['dense', 'strided4', 'strided_odd'])
def test_loss_zero_heat_weight_gives_exact_zero_dheat(layout, stages):
    """heat_wgt = 0 with dheat asked for and ncc_vals NULL: exact zeros, also on a plane whose target is all zero (where
    q * E would be 0 * finite but a constant predicted plane's would be 0 * NaN: the zeros are written as such)."""
    for p in (problem(2, 7, 3, 9, 12, 1, 4), problem(2, 0, 1, 13, 10, 2, 3), problem(2, 7, 3, 9, 12, 1, 4, zero_target=(0, 1))):
        Cc = p.dims[1]
        dw = 1.0 if Cc > 0 else 0.0
        for gs in (None, -2.5):
            r = run(p, dice_wgt=dw, heat_wgt=0.0, gs=gs, layout=layout, stages=stages)
            assert bool((r['dheat'] == 0).all()), 'dheat at heat_wgt 0: %s' % r['dheat'].flatten()[:4].tolist()
            if Cc > 0:
                check(p, r, 0, 1.0, 0.0, gs, 'heat_wgt 0')
            else:
                assert float(r['loss']) == 0.0


def test_module_with_heatmap_weight_one_gives_exact_zero_seg_gradient():
    """DiceAndHeatMapLoss2D(heatmap_wgt=1.0) passes the reference's assert and has dice_wgt = 0.0: on cropped network
    outputs that require a gradient, seg.grad is exact zeros and heat.grad the fp64 gradient.  The module allocates its
    scratch with torch.empty: a NaN-filled block of the same size is handed back to the caching allocator just before."""
    B, Cc, L, h, w, oy, ox = 2, 7, 3, 9, 12, 1, 4
    p = problem(B, Cc, L, h, w, oy, ox)
    seg = p.dev['seg'].clone().requires_grad_(True)
    heat = p.dev['heat'].clone().requires_grad_(True)
    crit = dfl_amd.DiceAndHeatMapLoss2D(skip_bg=False, heatmap_wgt=1.0)
    n = int(nat.lib().dfl_loss_scratch_doubles(B, Cc, L))
    torch.cuda.synchronize()
    # (several blocks of the scratch's size and of the smallest size, so the loss scalar allocated first does not split the one)
    poison = [torch.full((m,), float('nan'), dtype=torch.float64, device=DEV) for m in (n, n, n, n, 8, 8, 8, 8)]
    torch.cuda.synchronize()
    del poison
    loss = crit((dfl_amd.center_crop(seg, (h, w)), dfl_amd.center_crop(heat, (h, w))), (p.dev['tseg'], p.dev['theat']))
    loss.backward()
    torch.cuda.synchronize()
    rl, _, gheat, _ = p.reference(0, 0.0, 1.0, None)
    assert abs(loss.item() - float(rl)) < 2e-6
    assert seg.grad is not None and seg.grad.shape == seg.shape
    assert bool((seg.grad == 0).all().cpu()), 'seg.grad at dice_wgt 0.0: %s' % p.window(seg.grad).flatten()[:4].tolist()
    hg = heat.grad.cpu()
    _, bh = p.term_bounds(0, 0.0, 1.0, None)
    check_grad(p.window(hg).contiguous(), gheat, bh, 'module heat.grad')
    border = hg.clone()
    p.window(border).zero_()
    assert not bool(border.any())
