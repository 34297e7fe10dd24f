"""The streaming NHWC kernels of csrc/bn_elem.hip and csrc/upsample.hip -- dfl_colstats, dfl_bn_relu_bwd_apply, dfl_affine_copy,
dfl_maxpool2x2_fwd / _bwd, dfl_upsample2x_fwd / _bwd -- through the C ABI, against the fp64 models of tests/stream_ref.py: in each
of the three channel-unit forms a launch can take (8 bf16 channels, one float4, one fp32 channel) and by every route that selects
one (C, a pixel stride, a pointer's alignment), at the edges of the row kernels' launch geometry, in the second pass of the
grid-stride loops, and at what the entry points must refuse.

Every operand lives inside a larger allocation filled with a NaN bit pattern (Buf): whatever a kernel may not write must keep its
bits, whatever it overwrites must come back finite, and a read outside an operand poisons the result.

Tolerances are derived, none is tuned: u = 2^-24, S = the sum of the absolute values of an output's terms (stream_ref), k = the
fp32 operations on the longest path of the kernel's expression, written next to each bound.
  fp32 outputs   |got - ref| <= (k + 1) u S
  bf16 outputs   the same + 2^-8 |ref|   (round to nearest even of a value the fp32 error may have moved across a boundary)
  column sums    |total - ref| <= (M + 2) u sum|term|   (sequential summation's worst case; it holds for every grouping)"""
import ctypes as C
import math
from collections import namedtuple

import pytest
import torch

from dfl_amd import _native as nat
import stream_ref as SR

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF = torch.bfloat16
F64 = torch.float64
U = 2.0 ** -24
GUARD = 64                      # sentinel elements in front of and behind every operand
SENT32, SENT16 = 0x7fc12345, 0x7fc1   # quiet NaNs, fp32 and bf16
TINY = 2.0 ** -126              # the smallest positive normal of fp32 and of bf16
GRID_CAP = 8192 * 256           # csrc: stream_grid / up_grid cap a launch at 8192 workgroups of 256 threads


def stream():
    return torch.cuda.current_stream().cuda_stream


def launch(fn, args):
    """The entry point's return code, taken directly; the device is idle afterwards."""
    rc = getattr(nat.lib(), fn)(C.addressof(args), stream())
    torch.cuda.synchronize()
    return rc


def run(fn, args):
    rc = launch(fn, args)
    assert rc == 0, '%s refused (%d): %s' % (fn, rc, nat.lib().dfl_last_error().decode())


# ---------------------------------------------------------------------------------------------------- operand forms
# step: what the pixel stride grows by from one tensor of a call to the next (lda != ldb, ldx != ldy != lddx) without leaving the form
Form = namedtuple('Form', 'bf16 C ld choff base step')
FORMS = {
    'f4': Form(False, 8, 8, 0, 0, 4),            # float4
    'f4_slice': Form(False, 8, 24, 8, 0, 4),     # float4, inside a wider buffer
    'f1_c': Form(False, 6, 6, 0, 0, 1),          # one channel: C % 4 != 0
    'f1_ld': Form(False, 8, 10, 0, 0, 1),        # one channel: a stride that is no multiple of 4
    'f1_ptr': Form(False, 8, 12, 0, 1, 4),       # one channel: base + 1 float
    'b8': Form(True, 16, 16, 0, 0, 8),           # 8 bf16
    'b8_slice': Form(True, 16, 40, 8, 0, 8),     # 8 bf16, inside a wider buffer
}
FORM_IDS = list(FORMS)


def plain(bf16, Cc, step=0):
    return Form(bf16, Cc, Cc, 0, 0, step)


class Buf:
    """An operand [*pix][C] with pixel stride ld, `choff` channels into its pixels and `base` elements off an aligned address, inside
    a host array of sentinels that is uploaded for the call and compared with what comes back."""

    def __init__(self, pix, Cc, ld, bf16, choff=0, base=0):
        assert choff + Cc <= ld
        self.pix, self.C, self.ld, self.bf16 = tuple(pix), Cc, ld, bf16
        self.dtype, self.raw = (BF, torch.int16) if bf16 else (torch.float32, torch.int32)
        self.off = GUARD + base + choff
        n = GUARD + base + max(math.prod(self.pix), 1) * ld + GUARD
        self.host = torch.full((n,), SENT16 if bf16 else SENT32, dtype=self.raw)
        self.writable = torch.zeros(n, dtype=torch.bool)
        self.dev = None

    def _view(self, t):
        strides, s = [], self.ld
        for d in reversed(self.pix):
            strides.append(s)
            s *= d
        return t.as_strided(self.pix + (self.C,), tuple(reversed(strides)) + (1,), self.off)

    def set(self, v, sl=slice(None)):
        """Store v (rounded to the storage type) in the operand, or in its part sl; returns what is stored, as fp64."""
        part = self._view(self.host.view(self.dtype))[sl]
        part.copy_(v)
        return part.double()

    def allow(self, sl=slice(None)):
        """The contract lets the kernel write this part of the operand."""
        self._view(self.writable)[sl] = True
        return self

    def upload(self):
        self.dev = self.host.to(DEV)
        return self.dev.data_ptr() + self.off * self.host.element_size()

    def fetch(self, what):
        """(values as fp64, bits) of the operand after the call; everything outside allow() must have kept its bits."""
        after = self.dev.cpu()
        keep = ~self.writable
        changed = after[keep] != self.host[keep]
        assert not bool(changed.any()), '%s: %d elements outside the contract region were written' % (what, int(changed.sum()))
        return self._view(after.view(self.dtype)).double(), self._view(after).clone()

    def bits_of(self, v):
        """The bit patterns of values v in this operand's storage type."""
        return v.to(self.dtype).contiguous().view(self.raw)


def operand(form, pix, k, defect=None):
    """Tensor k of a call in the given form.  defect = (k, 'ld' | 'base', value) spoils that one tensor (refusal tests)."""
    ld, base = form.ld + k * form.step, form.base
    if defect is not None and defect[0] == k:
        ld, base = (defect[2], base) if defect[1] == 'ld' else (ld, defect[2])
    return Buf(pix, form.C, ld, form.bf16, form.choff, base)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def data(g, pix, Cc):
    """randn scaled per channel by 0.5 .. 4 and offset per image (per row for [M][C]): a swapped channel, pixel or image index
    moves a value by far more than any bound of this file."""
    v = torch.randn(*pix, Cc, generator=g, dtype=F64) * torch.linspace(0.5, 4.0, Cc, dtype=F64)
    lead = torch.arange(pix[0], dtype=F64).reshape(-1, *([1] * len(pix)))
    return v + (0.75 * lead if len(pix) == 3 else 0.25 * (lead % 5))


def assert_close(got, ref, S, k, bf16, what):
    assert bool(torch.isfinite(got).all()), '%s: %d non-finite outputs' % (what, int((~torch.isfinite(got)).sum()))
    bound = (k + 1) * U * S
    if bf16:
        bound = bound + 2.0 ** -8 * ref.abs()
    err = (got - ref).abs()
    bad = err > bound
    assert not bool(bad.any()), '%s: %d of %d elements off; worst excess %.3e (|err| %.3e, value %.3e)' % (
        what, int(bad.sum()), bad.numel(), float((err - bound).max()), float(err.flatten()[(err - bound).argmax()]),
        float(ref.flatten()[(err - bound).argmax()]))


def assert_sums(total, ref, S, M, what):
    assert bool(torch.isfinite(total).all()), '%s: non-finite sums' % what
    err, bound = (total - ref).abs(), (M + 2) * U * S
    assert bool((err <= bound).all()), '%s: worst |err| %.3e over a bound of %.3e' % (what, float(err.max()), float(bound[err.argmax()]))


def assert_bits(bits, expected, what):
    assert bits.shape == expected.shape and torch.equal(bits, expected), '%s: %d of %d elements differ in their bits' % (
        what, int((bits != expected).sum()), bits.numel())


# ---------------------------------------------------------------------------------------------------- upsample
UP_SHAPES = [(1, 1, 1), (1, 1, 5), (2, 5, 1), (1, 2, 2), (3, 3, 4), (2, 7, 9)]
K_UP_FWD = 4    # wy1 * (wx0 * v10 + wx1 * v11) on top of wy0 * (..): product, fused multiply-add, product, fused multiply-add
K_UP_BWD = 16   # 16 taps, one fused multiply-add each (their weights 1/16 .. 9/16 .. 1 are exact); + 1 add with accumulate


def shape_id(s):
    return 'x'.join(str(v) for v in s)


def up_call(form, shape, g, bwd, acc=False, defect=None):
    N, H, W = shape
    x, y = operand(form, (N, H, W), 0, defect), operand(form, (N, 2 * H, 2 * W), 1, defect)
    if bwd:
        src, old = y.set(data(g, (N, 2 * H, 2 * W), form.C)), (x.set(data(g, (N, H, W), form.C)) if acc else None)
        x.allow()
    else:
        src, old = x.set(data(g, (N, H, W), form.C)), None
        y.allow()
    args = nat.UpsampleArgs(x=x.upload(), y=y.upload(), N=N, H=H, W=W, C=form.C, ldx=x.ld, ldy=y.ld, bf16=int(form.bf16),
                            accumulate=int(acc))
    return 'dfl_upsample2x_bwd' if bwd else 'dfl_upsample2x_fwd', args, [x, y], (src, old)


def up_run(form, shape, g, bwd, acc=False):
    """-> (the input as stored, the kernel's output, the model's, the bound of their difference)"""
    fn, args, (x, y), (src, old) = up_call(form, shape, g, bwd, acc)
    run(fn, args)
    what = '%s %s acc=%d' % (fn, shape_id(shape), acc)
    got_x, _ = x.fetch(what + ' x')
    got_y, _ = y.fetch(what + ' y')
    if bwd:
        ref, S = SR.upsample2x_bwd(src, old, acc)
        got, k = got_x, K_UP_BWD + int(acc)
    else:
        ref, S = SR.upsample2x_fwd(src)
        got, k = got_y, K_UP_FWD
    assert_close(got, ref, S, k, form.bf16, what)
    return src, got, ref, (k + 1) * U * S + (2.0 ** -8 * ref.abs() if form.bf16 else 0.0)


@pytest.mark.parametrize('shape', UP_SHAPES, ids=shape_id)
@pytest.mark.parametrize('form', FORM_IDS)
def test_upsample2x_fwd(form, shape):
    up_run(FORMS[form], shape, gen(1), bwd=False)


@pytest.mark.parametrize('acc', [0, 1])
@pytest.mark.parametrize('shape', UP_SHAPES, ids=shape_id)
@pytest.mark.parametrize('form', FORM_IDS)
def test_upsample2x_bwd(form, shape, acc):
    up_run(FORMS[form], shape, gen(2), bwd=True, acc=bool(acc))


@pytest.mark.parametrize('shape', UP_SHAPES, ids=shape_id)
@pytest.mark.parametrize('form', FORM_IDS)
def test_upsample2x_adjoint_identity_of_the_gpu_outputs(form, shape):
    """<up(x), y> == <x, up^T(y)> in fp64 on what the two kernels wrote, to within what their own bounds leave of it."""
    x, up, _, b_up = up_run(FORMS[form], shape, gen(3), bwd=False)
    y, upT, _, b_upT = up_run(FORMS[form], shape, gen(4), bwd=True)
    lhs, rhs = float((up * y).sum()), float((x * upT).sum())
    assert abs(lhs - rhs) <= float((b_up * y.abs()).sum()) + float((x.abs() * b_upT).sum()), (lhs, rhs)


# ---------------------------------------------------------------------------------------------------- max-pool
POOL_SHAPES = [(1, 2, 2), (2, 3, 3), (2, 7, 9), (3, 10, 8)]
K_POOL_BWD = 1  # dx + g


def pool_call(form, shape, g, bwd, dx_old=None, defect=None):
    N, H, W = shape
    Ho, Wo = H // 2, W // 2
    x, y = operand(form, (N, H, W), 0, defect), operand(form, (N, Ho, Wo), 1, defect)
    dx = operand(form, (N, H, W), 2, defect) if bwd else None
    xv = x.set(torch.randint(0, 4, (N, H, W, form.C), generator=g).double())      # 0..3: ties everywhere
    win = (slice(None), slice(0, 2 * Ho), slice(0, 2 * Wo))
    dyv = oldv = None
    if bwd:
        dyv = y.set(data(g, (N, Ho, Wo), form.C))
        # an odd last row / column of dx stays sentinel: it belongs to no window and must keep its bits
        oldv = dx.set(torch.zeros(N, 2 * Ho, 2 * Wo, form.C, dtype=F64) if dx_old is None else dx_old, win)
        dx.allow(win)
    else:
        y.allow()
    args = nat.PoolArgs(x=x.upload(), y=y.upload(), dx=dx.upload() if bwd else None, N=N, H=H, W=W, C=form.C, ldx=x.ld, ldy=y.ld,
                        lddx=dx.ld if bwd else 0, bf16=int(form.bf16))
    return 'dfl_maxpool2x2_bwd' if bwd else 'dfl_maxpool2x2_fwd', args, [b for b in (x, y, dx) if b is not None], (xv, dyv, oldv, win)


def pool_fwd_check(form, shape, g):
    fn, args, (x, y), (xv, _, _, _) = pool_call(form, shape, g, bwd=False)
    run(fn, args)
    x.fetch(fn + ' x')
    got, _ = y.fetch(fn + ' y')
    ref, _ = SR.maxpool2x2_fwd(xv)
    assert torch.equal(got, ref), '%s %s: %d outputs differ' % (fn, shape_id(shape), int((got != ref).sum()))


def pool_bwd_check(form, shape, g):
    N, H, W = shape
    Ho, Wo = H // 2, W // 2
    what = 'dfl_maxpool2x2_bwd ' + shape_id(shape)
    # onto zeros: the gradient lands on the first maximum and nowhere else, as the very value
    fn, args, (x, y, dx), (xv, dyv, oldv, win) = pool_call(form, shape, g, bwd=True)
    run(fn, args)
    x.fetch(what + ' x')
    y.fetch(what + ' dy')
    got, _ = dx.fetch(what + ' dx')
    ref, _, _ = SR.maxpool2x2_bwd(xv[win], dyv, oldv)
    assert torch.equal(got[win], ref), '%s: the winners differ at %d elements' % (what, int((got[win] != ref).sum()))
    # onto a gradient that is already there: added, and the three losers of every window keep their bits
    fn, args, (x, y, dx), (xv, dyv, oldv, win) = pool_call(form, shape, g, bwd=True, dx_old=data(g, (N, 2 * Ho, 2 * Wo), form.C))
    run(fn, args)
    got, bits = dx.fetch(what + ' dx (accumulating)')
    ref, S, _ = SR.maxpool2x2_bwd(xv[win], dyv, oldv)
    assert_close(got[win], ref, S, K_POOL_BWD, form.bf16, what + ' (accumulating)')
    losers = ref == oldv
    assert_bits(bits[win][losers], dx.bits_of(oldv)[losers], what + ' losers')


@pytest.mark.parametrize('shape', POOL_SHAPES, ids=shape_id)
@pytest.mark.parametrize('form', FORM_IDS)
def test_maxpool2x2_fwd(form, shape):
    pool_fwd_check(FORMS[form], shape, gen(5))


@pytest.mark.parametrize('shape', POOL_SHAPES, ids=shape_id)
@pytest.mark.parametrize('form', FORM_IDS)
def test_maxpool2x2_bwd(form, shape):
    pool_bwd_check(FORMS[form], shape, gen(6))


# ---------------------------------------------------------------------------------------------------- affine copy
AFFINE_WINDOWS = [(1, 1), (1, 6), (5, 6)]
K_AFFINE = 2    # fused multiply-add, then the add of the old contents


def affine_call(form, win, g, scale, acc, N=2, xo=(2, 3), yo=(1, 2), xpad=(1, 2), ypad=(2, 1), defect=None):
    H, W = win
    xH, xW, yH, yW = xo[0] + H + xpad[0], xo[1] + W + xpad[1], yo[0] + H + ypad[0], yo[1] + W + ypad[1]
    x, y = operand(form, (N, xH, xW), 0, defect), operand(form, (N, yH, yW), 1, defect)
    xv = x.set(data(g, (N, xH, xW), form.C))
    # overwritten: the whole destination image is sentinel, and all of it but the window has to stay so
    yv = y.set(data(g, (N, yH, yW), form.C)) if acc else torch.zeros(N, yH, yW, form.C, dtype=F64)
    w = (slice(None), slice(yo[0], yo[0] + H), slice(yo[1], yo[1] + W))
    y.allow(w)
    sc = sh = None
    if scale:
        sc, sh = (torch.rand(form.C, generator=g) + 0.5).to(DEV), torch.randn(form.C, generator=g).to(DEV)
    args = nat.AffineCopyArgs(x=x.upload(), y=y.upload(), scale=nat.ptr(sc), shift=nat.ptr(sh), N=N, H=H, W=W, C=form.C,
                              ldx=x.ld, xH=xH, xW=xW, xoy=xo[0], xox=xo[1], ldy=y.ld, yH=yH, yW=yW, yoy=yo[0], yox=yo[1],
                              accumulate=int(acc), bf16=int(form.bf16))
    return 'dfl_affine_copy', args, [x, y], (xv, yv, w, sc, sh)


def affine_check(form, win, g, scale, acc, **kw):
    fn, args, (x, y), (xv, yv, w, sc, sh) = affine_call(form, win, g, scale, acc, **kw)
    run(fn, args)
    what = '%s %dx%d scale=%d acc=%d' % (fn, win[0], win[1], scale, acc)
    x.fetch(what + ' x')
    got, bits = y.fetch(what + ' y')
    ref, S = SR.affine_copy(xv, yv, win[0], win[1], args.xoy, args.xox, args.yoy, args.yox,
                            sc.cpu() if scale else None, sh.cpu() if scale else None, acc)
    if not scale and not acc:
        src = xv[:, args.xoy:args.xoy + win[0], args.xox:args.xox + win[1]]
        assert_bits(bits[w], y.bits_of(src), what + ' (a copy)')
    else:
        assert_close(got[w], ref[w], S[w], K_AFFINE, form.bf16, what)


@pytest.mark.parametrize('acc', [0, 1])
@pytest.mark.parametrize('scale', [0, 1])
@pytest.mark.parametrize('win', AFFINE_WINDOWS, ids=shape_id)
@pytest.mark.parametrize('form', FORM_IDS)
def test_affine_copy(form, win, scale, acc):
    affine_check(FORMS[form], win, gen(7), bool(scale), bool(acc))


# ---------------------------------------------------------------------------------------------------- row kernels
K_BRB = 2       # fma(A, dy, fma(B, r, C))


def rowblocks(M, Cc):
    return nat.lib().dfl_rowblock_count(M, Cc)


def brb_call(form, M, g, coef=True, partials=True, split=False, defect=None, nb_delta=0, rv=None, dyv=None, coefv=None):
    nb = rowblocks(M, form.C) + nb_delta
    dy, r, dpre = operand(form, (M,), 0, defect), operand(form, (M,), 1, defect), operand(form, (M,), 2, defect)
    dyv = dy.set(data(g, (M,), form.C) if dyv is None else dyv)
    if rv is None:
        rv = data(g, (M,), form.C) - 1.0
        rv.view(-1)[:3] = torch.tensor([0.0, -0.0, TINY], dtype=F64)      # a strict r > 0: only the third one passes
    rv = r.set(rv)
    dpre.allow()
    cd = None
    if coef:
        if coefv is None:
            coefv = torch.randn(3, form.C, generator=g) * torch.tensor([[0.5], [0.3], [0.2]]) + torch.tensor([[1.0], [0.0], [0.0]])
        cd = coefv.float().to(DEV)
    part = Buf((nb,), form.C, form.C, False).allow() if partials else None
    args = nat.BnReluBwdArgs(dy=dy.upload(), r=r.upload(), coef=nat.ptr(cd), dpre=dpre.upload(),
                             partials=part.upload() if partials else None, M=M, C=form.C, lddy=dy.ld, ldr=r.ld, ldo=dpre.ld,
                             nblocks=nb, split_out=int(split), bf16=int(form.bf16))
    return 'dfl_bn_relu_bwd_apply', args, [b for b in (dy, r, dpre, part) if b is not None], (dyv, rv, cd, part)


def decode_split(bits):
    """A split tensor's float4 slots [M][C] (as int32 bits) -> (hi, lo) bf16 values as fp64: half-words 0..3 of a slot are the
    high parts of its four channels, half-words 4..7 the low parts."""
    M, Cc = bits.shape
    h = bits.contiguous().view(torch.int16).reshape(M, Cc // 4, 8)
    hi, lo = h[:, :, :4].reshape(M, Cc).contiguous(), h[:, :, 4:].reshape(M, Cc).contiguous()
    return hi.view(BF).double(), lo.view(BF).double(), hi


def brb_check(form, M, g, coef=True, partials=True, split=False, what='', **kw):
    fn, args, bufs, (dyv, rv, cd, part) = brb_call(form, M, g, coef, partials, split, **kw)
    dy, r, dpre = bufs[:3]
    run(fn, args)
    what = '%s %s M=%d C=%d coef=%d split=%d' % (fn, what, M, form.C, coef, split)
    dy.fetch(what + ' dy')
    r.fetch(what + ' r')
    got, bits = dpre.fetch(what + ' dpre')
    ref, S = SR.bn_relu_bwd(dyv, rv, cd.cpu() if coef else None)
    if split:
        hi, lo, hi_bits = decode_split(bits)
        assert bool(torch.isfinite(hi).all() and torch.isfinite(lo).all()), what + ': non-finite parts'
        err, bound = (hi + lo - ref).abs(), 2.0 ** -16 * ref.abs() + (K_BRB + 1) * U * S
        assert bool((err <= bound).all()), '%s: hi + lo off by %.3e over its bound at worst' % (what, float((err - bound).max()))
        # hi + lo has at most 24 significant bits, so its fp32 is exact and .to(BF) the one rounding to nearest even.  Where lo
        # is exactly half a step of hi (the rounding of lo can take it there from just below), hi + lo lies midway between two
        # bf16 values, hi is one of them by construction and nearest-even may name the other: those elements are left out.
        tie = lo.abs() == torch.ldexp(torch.ones_like(hi), torch.frexp(hi).exponent - 9)
        rne_bits = (hi + lo).float().to(BF).view(torch.int16)
        assert_bits(torch.where(tie, rne_bits, hi_bits), rne_bits, what + ': hi is not the bf16 of hi + lo')
        assert int(tie.sum()) * 8 <= tie.numel(), what + ': too many ties to prove the layout'
        stored, sS = SR.colsum(ref)               # the sums are of the fp32 values, which a split tensor does not hold:
        sS = sS + S.sum(0) * (K_BRB + 1) / (M + 2)  # ... the model's, each term with its own fp32 error on top
    elif not coef:
        zero = torch.zeros((), dtype=F64)
        assert_bits(bits, dpre.bits_of(torch.where(rv > 0, dyv, zero)), what + ' (plain ReLU backward)')
        stored, sS = SR.colsum(got)
    else:
        assert_close(got, ref, S, K_BRB, form.bf16, what)
        stored, sS = SR.colsum(got)               # "of the values as stored"
    if partials:
        p, _ = part.fetch(what + ' partials')
        assert bool(torch.isfinite(p).all()), '%s: %d partial slots were left unwritten' % (what, int((~torch.isfinite(p)).sum()))
        assert_sums(p.sum(0), stored, sS, M, what + ' sums')


def colstats_call(form, M, g, with_b=True, defect=None, nb_delta=0):
    nb = rowblocks(M, form.C) + nb_delta
    a, b = operand(form, (M,), 0, defect), (operand(form, (M,), 1, defect) if with_b else None)
    av = a.set(data(g, (M,), form.C))
    bv = b.set(data(g, (M,), form.C)) if with_b else None
    part = Buf((nb, 2), form.C, form.C, False).allow()
    args = nat.ColstatsArgs(a=a.upload(), b=b.upload() if with_b else None, partials=part.upload(), M=M, C=form.C, lda=a.ld,
                            ldb=b.ld if with_b else 0, nblocks=nb, bf16=int(form.bf16))
    return 'dfl_colstats', args, [t for t in (a, b, part) if t is not None], (av, bv, part)


def colstats_check(form, M, g, with_b=True, what=''):
    fn, args, bufs, (av, bv, part) = colstats_call(form, M, g, with_b)
    run(fn, args)
    what = '%s %s M=%d C=%d b=%d' % (fn, what, M, form.C, with_b)
    for t in bufs[:-1]:
        t.fetch(what + ' input')
    p, _ = part.fetch(what + ' partials')
    assert bool(torch.isfinite(p).all()), '%s: %d partial slots were left unwritten' % (what, int((~torch.isfinite(p)).sum()))
    ref, S = SR.colstats(av, bv)
    assert_sums(p.sum(0), ref, S, M, what)


M_FORMS = 37


@pytest.mark.parametrize('partials', [0, 1])
@pytest.mark.parametrize('coef', [0, 1])
@pytest.mark.parametrize('form', FORM_IDS)
def test_bn_relu_bwd_apply(form, coef, partials):
    brb_check(FORMS[form], M_FORMS, gen(8), bool(coef), bool(partials), what=form)


@pytest.mark.parametrize('coef', [0, 1])
@pytest.mark.parametrize('form', ['f4', 'f4_slice'])
def test_bn_relu_bwd_apply_split_out(form, coef):
    brb_check(FORMS[form], M_FORMS, gen(9), bool(coef), True, split=True, what=form)


@pytest.mark.parametrize('with_b', [0, 1])
@pytest.mark.parametrize('form', FORM_IDS)
def test_colstats(form, with_b):
    colstats_check(FORMS[form], M_FORMS, gen(10), bool(with_b), what=form)


def test_bn_relu_bwd_sums_are_of_the_values_as_stored():
    """bf16, A = 1.00293: every stored dpre is exactly 1.0 or 0.0, so the column totals are the counts of rows with r > 0, exactly;
    sums of the unrounded 1.00293 would be off by about 3."""
    M, Cc = 1000, 16
    g = gen(11)
    mask = (torch.rand(M, Cc, generator=g) < 0.5).double()
    coefv = torch.tensor([[1.00293], [0.0], [0.0]]).repeat(1, Cc)
    fn, args, bufs, (dyv, rv, cd, part) = brb_call(plain(True, Cc), M, g, rv=mask, dyv=torch.ones(M, Cc, dtype=F64), coefv=coefv)
    run(fn, args)
    got, _ = bufs[2].fetch('dpre')
    assert torch.equal(got, mask)
    p, _ = part.fetch('partials')
    assert torch.equal(p.sum(0), mask.sum(0))
    assert abs(float(mask.sum(0).min()) * 0.00293) > 1.0      # the unrounded sums would have been told apart


# ---------------------------------------------------------------------------------------------------- row-kernel geometry
ROWS_F4 = (1, 127, 128, 129, 255, 256, 257, 385)     # float4, C = 8: 2 units x 128 row lanes, 2 rows in flight
ROWS_B8 = (1, 255, 256, 257, 1023, 1024)             # bf16, C = 8: 1 unit x 256 row lanes, 4 rows in flight
GEOM = ([('gy2', False, 37, 258), ('gy2', False, 37, 1028), ('gy2', True, 37, 2056)]
        + [('rows', False, M, 8) for M in ROWS_F4] + [('rows', True, M, 8) for M in ROWS_B8]
        + [('empty', False, 9, 4608), ('empty', True, 9, 4608), ('capM', False, 3, 16392), ('capM', True, 3, 16392),
           ('cap2048', False, 530003, 32), ('cap2048', True, 530003, 32)])


def geom_id(c):
    return '%s_%s_M%d_C%d' % (c[0], 'b8' if c[1] else ('f4' if c[3] % 4 == 0 else 'f1'), c[2], c[3])


def assert_premise(kind, bf16, M, Cc):
    """What makes the case the edge it is meant to be, from the library's own row-block count: a change of the block constants
    then fails here, loudly, instead of leaving the case without its point."""
    nb = rowblocks(M, Cc)
    rows = -(-M // nb)
    uncapped = -(-M * Cc // 8192)
    units = Cc // (8 if bf16 else (4 if Cc % 4 == 0 else 1))
    if kind == 'gy2':       # a second block of 256 units with one lane in it (two in the one-channel form)
        assert 256 < units <= 258 and nb == uncapped
    elif kind == 'rows':    # one row block: the rows per lane run from below to just above "R rows in flight"
        assert nb == 1
    elif kind == 'empty':   # the last block owns no rows, and its slots are still summed by whoever reads the partials
        assert (nb, rows) == (6, 2) and (nb - 1) * rows >= M
    elif kind == 'capM':
        assert nb == M < uncapped
    else:
        assert nb == 2048 < uncapped and rows == 259 and M % rows != 0


@pytest.mark.parametrize('case', GEOM, ids=geom_id)
def test_colstats_geometry(case):
    kind, bf16, M, Cc = case
    assert_premise(kind, bf16, M, Cc)
    colstats_check(plain(bf16, Cc), M, gen(12), True, what=kind)


@pytest.mark.parametrize('case', GEOM, ids=geom_id)
def test_bn_relu_bwd_apply_geometry(case):
    kind, bf16, M, Cc = case
    assert_premise(kind, bf16, M, Cc)
    brb_check(plain(bf16, Cc), M, gen(13), True, True, what=kind)


# ---------------------------------------------------------------------------------------------------- grid-stride second pass
# One-channel fp32 with C = 33 (33 units per pixel, no power of two), N = 2, and grids of just over 63,551 pixels: more units than
# the 8192 x 256 threads of a capped launch, fewer than twice as many.  bf16 with C = 264 (33 units again) for the two kernels
# whose operands stay small.  Every element is compared.
STRIDE_F1, STRIDE_B8 = plain(False, 33, 1), plain(True, 264, 8)


def assert_second_pass(pixels, form):
    units = pixels * (form.C // (8 if form.bf16 else 1))
    assert GRID_CAP < units < 2 * GRID_CAP, units


@pytest.mark.parametrize('form', [STRIDE_F1, STRIDE_B8], ids=['f1_C33', 'b8_C264'])
def test_affine_copy_grid_stride(form):
    assert_second_pass(2 * 181 * 181, form)
    affine_check(form, (181, 181), gen(14), True, True, xo=(1, 2), yo=(1, 0), xpad=(0, 1), ypad=(0, 0))


@pytest.mark.parametrize('form', [STRIDE_F1, STRIDE_B8], ids=['f1_C33', 'b8_C264'])
def test_upsample2x_fwd_grid_stride(form):
    assert_second_pass(2 * 180 * 180, form)          # counted on the large grid
    up_run(form, (2, 90, 90), gen(15), bwd=False)


def test_upsample2x_bwd_grid_stride():
    assert_second_pass(2 * 181 * 181, STRIDE_F1)     # counted on the small grid
    up_run(STRIDE_F1, (2, 181, 181), gen(16), bwd=True, acc=True)


def test_maxpool2x2_fwd_grid_stride():
    assert_second_pass(2 * 181 * 181, STRIDE_F1)     # counted on the output grid; an odd last row on top
    pool_fwd_check(STRIDE_F1, (2, 363, 362), gen(17))


def test_maxpool2x2_bwd_grid_stride():
    assert_second_pass(2 * 181 * 181, STRIDE_F1)
    pool_bwd_check(STRIDE_F1, (2, 363, 362), gen(18))


# ---------------------------------------------------------------------------------------------------- refusals
# entry point -> (its tensors, a call in the given form)
CALLS = {
    'colstats': (2, lambda f, g, d: colstats_call(f, M_FORMS, g, defect=d)),
    'bn_relu_bwd_apply': (3, lambda f, g, d: brb_call(f, M_FORMS, g, defect=d)),
    'affine_copy': (2, lambda f, g, d: affine_call(f, (5, 6), g, True, True, defect=d)),
    'maxpool2x2_fwd': (2, lambda f, g, d: pool_call(f, (2, 7, 9), g, False, defect=d)),
    'maxpool2x2_bwd': (3, lambda f, g, d: pool_call(f, (2, 7, 9), g, True, defect=d)),
    'upsample2x_fwd': (2, lambda f, g, d: up_call(f, (2, 3, 4), g, False, defect=d)),
    'upsample2x_bwd': (2, lambda f, g, d: up_call(f, (2, 3, 4), g, True, True, defect=d)),
}


def assert_refused(fn, args, bufs, what):
    rc = launch(fn, args)
    assert rc != 0, '%s: accepted' % what
    for b in bufs:
        b.writable[:] = False
        b.fetch(what)


@pytest.mark.parametrize('entry', list(CALLS))
def test_bf16_with_12_channels_is_refused(entry):
    fn, args, bufs, _ = CALLS[entry][1](Form(True, 12, 16, 0, 0, 8), gen(19), None)
    assert_refused(fn, args, bufs, entry + ' bf16 C=12')


@pytest.mark.parametrize('entry,k', [(e, k) for e in CALLS for k in range(CALLS[e][0])])
def test_bf16_with_a_pixel_stride_of_20_is_refused(entry, k):
    fn, args, bufs, _ = CALLS[entry][1](FORMS['b8'], gen(20), (k, 'ld', 20))
    assert_refused(fn, args, bufs, '%s bf16 ld=20 on tensor %d' % (entry, k))


@pytest.mark.parametrize('entry,k', [(e, k) for e in CALLS for k in range(CALLS[e][0])])
def test_bf16_two_bytes_off_alignment_is_refused(entry, k):
    fn, args, bufs, _ = CALLS[entry][1](FORMS['b8'], gen(21), (k, 'base', 1))
    assert_refused(fn, args, bufs, '%s bf16 base + 2 bytes on tensor %d' % (entry, k))


@pytest.mark.parametrize('form', ['f1_c', 'f1_ld', 'f1_ptr', 'b8'])
def test_split_out_is_refused_outside_the_float4_form(form):
    fn, args, bufs, _ = brb_call(FORMS[form], M_FORMS, gen(22), split=True)
    assert_refused(fn, args, bufs, 'split_out in form ' + form)


@pytest.mark.parametrize('delta', [-1, 1])
@pytest.mark.parametrize('entry', ['colstats', 'bn_relu_bwd_apply'])
@pytest.mark.parametrize('form', ['f4', 'b8'])
def test_a_wrong_row_block_count_is_refused(form, entry, delta):
    M = 1500                                       # several row blocks, so one fewer is still a positive count
    assert rowblocks(M, FORMS[form].C) + delta >= 1
    call = colstats_call if entry == 'colstats' else brb_call
    fn, args, bufs, _ = call(FORMS[form], M, gen(23), nb_delta=delta)
    assert_refused(fn, args, bufs, '%s nblocks %+d' % (entry, delta))


@pytest.mark.parametrize('side', ['x', 'y'])
@pytest.mark.parametrize('edge', ['bottom', 'right', 'top', 'left'])
@pytest.mark.parametrize('form', ['f4', 'b8'])
def test_affine_copy_window_outside_its_image_is_refused(form, edge, side):
    o, pad = {'bottom': ((2, 3), (-1, 2)), 'right': ((2, 3), (1, -1)), 'top': ((-1, 3), (2, 2)), 'left': ((2, -1), (1, 2))}[edge]
    kw = dict(xo=o, xpad=pad) if side == 'x' else dict(yo=o, ypad=pad)
    fn, args, bufs, _ = affine_call(FORMS[form], (5, 6), gen(24), True, True, **kw)
    assert_refused(fn, args, bufs, 'affine_copy %s window past the %s edge' % (side, edge))


@pytest.mark.parametrize('bwd', [0, 1])
@pytest.mark.parametrize('shape', [(2, 1, 6), (2, 6, 1)], ids=shape_id)
@pytest.mark.parametrize('form', ['f4', 'b8'])
def test_pool_of_a_single_row_or_column_is_refused(form, shape, bwd):
    fn, args, bufs, _ = pool_call(FORMS[form], shape, gen(25), bool(bwd))
    assert_refused(fn, args, bufs, '%s %s' % ('maxpool2x2_bwd' if bwd else 'maxpool2x2_fwd', shape_id(shape)))
