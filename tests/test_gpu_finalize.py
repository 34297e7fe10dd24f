"""The kernels that finish every sum of a training step and apply every update -- dfl_reduce_batch, dfl_reduce_partials,
dfl_sum_partials, dfl_bn_finalize / dfl_bn_bwd_finalize and their _live forms, dfl_bn_eval_prepare, dfl_sgd_step / dfl_adam_step /
dfl_rmsprop_step and dfl_sgd_pack_tiled / dfl_optim_pack_tiled (the second half of csrc/bn_elem.hip, and csrc/wgrad_gemm.hip) --
through the C ABI, against the fp64 models of tests/finalize_ref.py, at every branch of their launch geometry and at what the
entry points must refuse.

Every operand, inputs included, lives inside a larger allocation of NaN bit patterns (Buf of tests/test_gpu_streaming.py, Words
for 8-byte types): whatever the contract does not let a kernel write must keep its bits, every output must come back finite, and
the gaps that may not be read (stride > n, stride > C, between the jobs of an arena) are NaN, so a stray read shows in a result.
Every case runs twice and the two runs must agree in every bit (all of these kernels promise a fixed summation order).

No tolerance is tuned.  Two kinds of assertion:
  exact data     sums of fp32 values accumulated in fp64: the inputs are integers * 2^-10, |integer| < 2^20 (FR.exact_data), so
                 every partial sum is an exact fp64 in any order and the stored sum must be float32(exact sum), bit for bit
  derived bound  u = 2^-24.  fp32 arithmetic: |got - ref| <= (k + 1) u S, S = the sum of the absolute values of the terms
                 (finalize_ref), k = the fp32 roundings on the longest path, written next to each bound.  fp64 arithmetic rounded
                 to fp32 once (the finalizes): |got - ref| <= u |ref| + K64 2^-53 S, K64 derived where it is defined."""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

from dfl_amd import _native as nat
import finalize_ref as FR
import pack_ref as PK
from test_gpu_streaming import Buf, DEV, GUARD, U, assert_bits, assert_close, gen, stream

pytestmark = pytest.mark.gpu
F64 = torch.float64
SENT64 = 0x7ff8000012345678         # a quiet NaN of fp64
GRID_CAP = 8192 * 256               # csrc/bn_elem.hip stream_grid: a flat launch is capped at 8192 workgroups of 256 threads


def lib():
    return nat.lib()


def sync(rc, what):
    torch.cuda.synchronize()
    assert rc == 0, '%s refused (%d): %s' % (what, rc, lib().dfl_last_error().decode())


class Words:
    """A read-only or counter operand of 8-byte words (the fp64 totals of the live statistics, num_batches_tracked) between
    sentinels."""

    def __init__(self, values):
        self.dtype, self.n = values.dtype, values.numel()
        self.host = torch.full((2 * GUARD + self.n,), SENT64, dtype=torch.int64)
        self.host[GUARD:GUARD + self.n] = values.contiguous().view(torch.int64).reshape(-1)
        self.dev = None

    def upload(self):
        self.dev = self.host.to(DEV)
        return self.dev.data_ptr() + 8 * GUARD

    def fetch(self, what, written=False):
        after = self.dev.cpu()
        same = after == self.host
        if written:
            same[GUARD:GUARD + self.n] = True
        assert bool(same.all()), '%s: %d words outside the contract region were written' % (what, int((~same).sum()))
        return after[GUARD:GUARD + self.n].view(self.dtype)


def vec(v=None, n=None, room=0, base=0):
    """A vector [n] with `room` sentinel elements behind it that still belong to the allocation; .stored = its values as fp64."""
    n = v.numel() if v is not None else n
    b = Buf((1,), n, n + room, False, base=base)
    b.stored = b.set(v.reshape(1, -1))[0] if v is not None else None
    return b


def out(n, room=0):
    return vec(n=n, room=room).allow()


def fetch(b, what, finite=True):
    """(values, bits) of a vector or tensor after the call; the guards were checked, and an output must be finite."""
    v, bits = b.fetch(what)
    if finite:
        assert bool(torch.isfinite(v).all()), '%s: %d non-finite elements' % (what, int((~torch.isfinite(v)).sum()))
    return v.reshape(-1), bits.reshape(-1)


def table(arr):
    """A ctypes array of job records in device memory."""
    return torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).to(DEV)


def twice(once, what):
    """Run the case twice from the same inputs: every returned (values, bits) must agree in its bits."""
    a, b = once(), once()
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x[1], y[1]), '%s: output %d differs between two runs in %d elements' % (what, k, int((x[1] != y[1]).sum()))
    return a


def f32_bits(v):
    return v.float().contiguous().view(torch.int32).reshape(-1)


def assert_rounded(got, ref, S, k64, what):
    """An fp64 evaluation with at most k64 * 2^-53 * S of error, rounded to fp32 once."""
    err, bound = (got - ref).abs(), U * ref.abs() + k64 * 2.0 ** -53 * S
    bad = err > bound
    assert not bool(bad.any()), '%s: %d of %d off; worst |err| %.3e over a bound of %.3e' % (
        what, int(bad.sum()), bad.numel(), float(err[(err - bound).argmax()]), float(bound[(err - bound).argmax()]))


# ---------------------------------------------------------------------------------------------------- dfl_reduce_batch
# csrc/bn_elem.hip: RB_T = 256 threads, RB_O = 32 outputs and RB_S = 32 slice lanes per wide workgroup, RB_WIDE_MIN = 32.
RB_O, RB_WIDE_MIN, RB_NARROW = 32, 32, 1024
RB_COUNTS = [1, 2,
             31, 32, 33,                 # `j.count >= RB_WIDE_MIN`: the narrow and the wide form (and reduce_job_blocks' own switch)
             127, 128, 129, 160,         # `k + 3 * RB_S < j.count`: lane 0 enters the four-in-flight loop at 97, lane 31 at 128
             255, 256, 257, 300]         # `k + 7 * RB_S < j.count`: eight in flight (vector form only), lane 0 at 225, lane 31 at 256
RB_NS = [1, 3, 4, 5,
         31, 32, 33,                     # RB_O outputs of a wide workgroup: `i = b * RB_O + 4 * o4`
         1023, 1024, 1025,               # 4 * RB_T outputs of a narrow one: `i = (b * RB_T + threadIdx.x) * 4`
         4100]


def rb_cases():
    """(n, stride, count, T, base, vector form) of every job of the one launch."""
    cases = []
    for count in RB_COUNTS:
        cases.append((36, 40, count, 1, 0, True))        # float4 loads, the gap of 4 behind every slice is NaN
        cases.append((37, 37, count, 1, 0, False))       # scalar loads, three of them in the last thread's `i + e < n`
    for n in RB_NS:
        for count in (3, 40):                            # narrow, wide
            cases.append((n, n + (4 if n % 4 == 0 else 3), count, 1, 0, n % 4 == 0))
    # `vec = (n & 3) == 0 && (stride & 3) == 0 && (src & 15) == 0`: aligned, then broken one way at a time
    for count in (5, 300):
        cases += [(64, 64, count, 1, 0, True), (66, 68, count, 1, 0, False), (64, 66, count, 1, 0, False), (64, 64, count, 1, 1, False)]
    # rb_store4: `dst[(ii % (n / T)) * T + ii / (n / T)]`
    for T in (1, 2, 4, 9):
        cases += [(72, 72, 4, T, 0, True), (72, 76, 33, T, 0, True), (9 * T, 9 * T + 1, 40, T, 0, False)]
    cases.append((4100, 4100, 2, 4, 0, True))
    cases.append((1028, 1028, 1400, 4, 0, True))         # the largest: 1.44 M floats
    return cases


def rb_job(g, case):
    n, stride, count, T, base, vec_form = case
    src = Buf((count,), n, stride, False, base=base)
    v = src.set(FR.exact_data(g, count, n))
    return dict(case=case, src=src, dst=out(n), expect=f32_bits(FR.reduce_slices(v, T)[0]))


def rb_launch(jobs):
    arr, blocks = (nat.ReduceJob * len(jobs))(), 0
    for i, j in enumerate(jobs):
        n, stride, count, T, base, vec_form = j['case']
        arr[i].src, arr[i].dst, arr[i].n, arr[i].stride, arr[i].count, arr[i].T = j['src'].upload(), j['dst'].upload(), n, stride, count, T
        arr[i].first_block = blocks
        assert (n % 4 == 0 and stride % 4 == 0 and arr[i].src % 16 == 0) == vec_form, j['case']     # the form the case is here for
        nb = nat.check(lib().dfl_reduce_job_blocks(n, count), 'dfl_reduce_job_blocks')
        assert nb == -(-n // (RB_O if count >= RB_WIDE_MIN else RB_NARROW)), j['case']
        blocks += nb
    tab = table(arr)
    sync(lib().dfl_reduce_batch(tab.data_ptr(), len(jobs), blocks, stream()), 'dfl_reduce_batch')
    res = []
    for j in jobs:
        fetch(j['src'], 'dfl_reduce_batch src %s' % (j['case'],))
        res.append(fetch(j['dst'], 'dfl_reduce_batch dst %s' % (j['case'],)))
    return res


def rb_check(jobs, what):
    res = twice(lambda: rb_launch(jobs), what)
    for j, (_, bits) in zip(jobs, res):
        assert_bits(bits, j['expect'], '%s job %s' % (what, j['case']))


def test_reduce_batch_every_branch_in_one_launch():
    """All the cases as the jobs of one launch: the binary search over first_block finds each workgroup's job among 70."""
    g = gen(101)
    jobs = [rb_job(g, c) for c in rb_cases()]
    assert max(j['case'][1] * j['case'][2] for j in jobs) < 1.5e6
    rb_check(jobs, 'dfl_reduce_batch, one launch')


@pytest.mark.parametrize('case', [(36, 40, 32, 1, 0, True), (37, 37, 129, 1, 0, False), (36, 40, 257, 1, 0, True), (64, 64, 300, 1, 1, False),
                                  (1025, 1028, 3, 1, 0, False), (72, 76, 33, 9, 0, True), (5, 8, 40, 1, 0, False)],
                         ids=lambda c: 'n%d_ld%d_x%d_T%d_b%d' % c[:5])
def test_reduce_batch_single_job(case):
    rb_check([rb_job(gen(102), case)], 'dfl_reduce_batch, one job')


# ---------------------------------------------------------------------------------------------------- dfl_reduce_partials
@pytest.mark.parametrize('Cc', [1, 7, 8, 9, 1000])       # reduce_partials_kernel: `c = blockIdx.x * 8 + cl`, `c < C`
def test_reduce_partials(Cc):
    g = gen(110 + Cc)
    for nb in (1, 31, 32, 33, 1000):                     # `for (r = rl; r < nblocks; r += 32)`: 32 row lanes
        for stride in (Cc, Cc + 3):                      # the gap behind every row is NaN
            src = Buf((nb,), Cc, stride, False)
            v = src.set(FR.exact_data(g, nb, Cc))
            dst = out(Cc)

            def once():
                sync(lib().dfl_reduce_partials(src.upload(), dst.upload(), nb, stride, Cc, stream()), 'dfl_reduce_partials')
                fetch(src, 'dfl_reduce_partials src')
                return [fetch(dst, 'dfl_reduce_partials C=%d nblocks=%d stride=%d' % (Cc, nb, stride))]
            (_, bits), = twice(once, 'dfl_reduce_partials')
            assert_bits(bits, f32_bits(v.sum(0)), 'dfl_reduce_partials C=%d nblocks=%d stride=%d' % (Cc, nb, stride))


# ---------------------------------------------------------------------------------------------------- dfl_sum_partials
# csrc/wgrad_gemm.hip dfl_sum_partials: `splits >= 32 && n <= (1 << 20)` takes sum_partials_wide_kernel (16 outputs x 16 slice
# lanes per workgroup, `k + 7 * 16 < splits` eight in flight), everything else sum_partials_kernel (256 outputs per workgroup).
SP_NS = {1: [1, 15, 16, 17, 255, 256, 257], 4: [16, 20, 252, 256, 260], 9: [9, 18, 252, 261]}


@pytest.mark.parametrize('T', [1, 4, 9])
@pytest.mark.parametrize('splits', [1, 2, 31, 32, 33, 100, 129, 260])   # 129 / 260: one / two passes of the eight-in-flight loop
def test_sum_partials(splits, T):
    g = gen(120 + splits)
    for n in SP_NS[T]:
        src = Buf((splits,), n, n, False)
        v = src.set(FR.exact_data(g, splits, n))
        dst = out(n)
        what = 'dfl_sum_partials n=%d splits=%d T=%d' % (n, splits, T)

        def once():
            sync(lib().dfl_sum_partials(src.upload(), dst.upload(), n, splits, T, stream()), what)
            fetch(src, what + ' src')
            return [fetch(dst, what)]
        (_, bits), = twice(once, what)
        assert_bits(bits, f32_bits(FR.reduce_slices(v, T)[0]), what)


def test_sum_partials_of_nothing_writes_nothing_and_a_ragged_T_is_refused():
    src, dst = vec(FR.exact_data(gen(130), 40)), out(20)
    dst.writable[:] = False
    sync(lib().dfl_sum_partials(src.upload(), dst.upload(), 0, 2, 4, stream()), 'dfl_sum_partials n=0')
    fetch(dst, 'dfl_sum_partials n=0', finite=False)
    for n, T in ((18, 4), (20, 3)):
        rc = lib().dfl_sum_partials(src.upload(), dst.upload(), n, 2, T, stream())
        torch.cuda.synchronize()
        assert rc == -1 and b'multiple of T' in lib().dfl_last_error()
        fetch(dst, 'dfl_sum_partials n %% T != 0', finite=False)


# ---------------------------------------------------------------------------------------------------- dfl_bn_finalize
# finalize_cpb: `C >= 512 ? 8 : (C >= 256 ? 4 : (C >= 128 ? 2 : 1))` channels per workgroup, 256 / cpb row lanes;
# sum_partials_f64: `r + 3 * lanes < nblocks` four rows in flight, then `r < nblocks` one at a time.
FIN_CASES = [(4, 1), (6, 1025), (127, 70), (128, 70), (130, 513), (255, 9), (257, 300), (511, 40), (513, 129), (1024, 7)]
# fp64 error of the finalize outputs in units of 2^-53 S.  The statistics are chosen with var >= mean^2 / 100, so that
# s2/cnt + mean^2 <= 202 var: the three roundings of `s2 / cnt - mean * mean` leave var a relative error of at most 3 * 202 * 2^-53
# (606; the root halves it for invstd, the unbiased variance takes it whole), and at most 8 further fp64 operations follow: < 640.
# With the totals exact (exact data) nothing else enters.
K64_FWD = 640
# backward: no cancellation but the one S already carries (sum dy r - mean sum dy); at most 9 fp64 operations on the longest path
# (C = -s c1 + s c2 invstd mean through dgamma), and the operands save_mean / save_invstd / gamma are exact fp32 values.
K64_BWD = 16
EPS, MOM = 1e-5, 0.1


def cpb_of(Cc):
    return 8 if Cc >= 512 else (4 if Cc >= 256 else (2 if Cc >= 128 else 1))


def chan(Cc, lo, hi):
    return torch.linspace(lo, hi, Cc, dtype=F64) if Cc > 1 else torch.tensor([hi], dtype=F64)


def fwd_partials(g, nb, Cc, count):
    """[nb][2][C] partial sums (x, x^2) as exact data: about count / nb elements per block with a mean of -2 .. 2 and a variance
    of 0.5 .. 4 by channel, and noise by row -- a dropped or doubled row moves the mean by 1 / nb of itself."""
    e = count / nb
    mu, sig2 = chan(Cc, -2.0, 2.0), chan(Cc, 0.5, 4.0)
    m = mu + 0.25 * torch.randn(nb, Cc, generator=g, dtype=F64)          # the blocks' own means
    p1 = e * m
    p2 = e * (sig2 * (1.0 + 0.1 * torch.rand(nb, Cc, generator=g, dtype=F64)) + m * m)     # var >= sig2 whatever the rows (Jensen)
    return FR.quantize(torch.stack([p1, p2], dim=1))


def fin_call(g, Cc, nb, count, running=True, tracked=True, partials=None):
    part = Buf((nb, 2), Cc, Cc, False)
    pv = part.set(fwd_partials(g, nb, Cc, count) if partials is None else partials)
    ins = {'partials': part, 'gamma': vec(torch.randn(Cc, generator=g) * 0.5 + chan(Cc, 1.0, 2.0).float()),
           'beta': vec(torch.randn(Cc, generator=g))}
    if running:
        ins['running_mean'], ins['running_var'] = vec(torch.randn(Cc, generator=g)).allow(), vec(torch.rand(Cc, generator=g) + 0.5).allow()
    outs = {k: out(Cc) for k in ('scale', 'shift', 'save_mean', 'save_invstd')}
    nbt = Words(torch.tensor([41], dtype=torch.int64)) if tracked else None
    return ins, outs, nbt, pv


def fin_run(ins, outs, nbt, Cc, nb, count, what):
    def once():
        ptrs = {k: b.upload() for k, b in list(ins.items()) + list(outs.items())}
        a = nat.BnFinalizeArgs(num_batches_tracked=nbt.upload() if nbt else None, count=count, nblocks=nb, C=Cc, eps=EPS, momentum=MOM, **ptrs)
        sync(lib().dfl_bn_finalize(C.addressof(a), stream()), what)
        for k in ('partials', 'gamma', 'beta'):
            fetch(ins[k], '%s %s' % (what, k))
        res = [fetch(outs[k], '%s %s' % (what, k)) for k in ('scale', 'shift', 'save_mean', 'save_invstd')]
        res += [fetch(ins[k], '%s %s' % (what, k)) for k in ('running_mean', 'running_var') if k in ins]
        if nbt:
            t = nbt.fetch(what + ' num_batches_tracked', written=True)
            assert int(t[0]) == 42, '%s: num_batches_tracked went from 41 to %d' % (what, int(t[0]))
        return res
    return twice(once, what)


def fin_check(g, Cc, nb, count, running=True, tracked=True, partials=None, premise=True):
    what = 'dfl_bn_finalize C=%d nblocks=%d count=%d' % (Cc, nb, count)
    ins, outs, nbt, pv = fin_call(g, Cc, nb, count, running, tracked, partials)
    res = fin_run(ins, outs, nbt, Cc, nb, count, what)
    s = pv.sum(0)                                           # exact
    ref = FR.bn_finalize(s[0], s[1], ins['gamma'].stored, ins['beta'].stored, count, EPS, MOM,
                         ins['running_mean'].stored if running else None, ins['running_var'].stored if running else None)
    if premise:
        mean, var = ref['save_mean'][0], ref['var'][0]
        assert bool((var >= mean * mean / 100).all()), what + ': the statistics leave the regime K64_FWD is derived for'
    names = ['scale', 'shift', 'save_mean', 'save_invstd'] + (['running_mean', 'running_var'] if running else [])
    for name, (got, _) in zip(names, res):
        assert_rounded(got, ref[name][0], ref[name][1], K64_FWD, '%s %s' % (what, name))
    return dict(zip(names, res)), ref


@pytest.mark.parametrize('Cc,nb', FIN_CASES)
def test_bn_finalize(Cc, nb):
    cpb = cpb_of(Cc)
    lanes = 256 // cpb
    # what the shapes are here for, from the kernel's own constants
    assert {4: 1, 6: 1, 127: 1, 128: 2, 130: 2, 255: 2, 257: 4, 511: 4, 513: 8, 1024: 8}[Cc] == cpb
    if (Cc, nb) in ((6, 1025), (130, 513), (257, 300), (513, 129)):
        assert nb > 3 * lanes and (nb - 4 * lanes * (nb // (4 * lanes))) % lanes != 0     # the unrolled loop runs and leaves a ragged rest
    fin_check(gen(200 + Cc), Cc, nb, 16 * nb)


@pytest.mark.parametrize('running,tracked', [(False, True), (True, False), (False, False)])
def test_bn_finalize_without_running_statistics_or_counter(running, tracked):
    fin_check(gen(220), 130, 70, 16 * 70, running=running, tracked=tracked)


def test_bn_finalize_of_a_single_element_keeps_the_biased_variance():
    """count == 1: `unbiased = (cnt > 1.0) ? var * cnt / (cnt - 1.0) : var` -- the other branch would store an infinity."""
    fin_check(gen(221), 6, 1, 1)


def test_bn_finalize_clamps_a_negative_variance():
    """Channel 0: s1 = 192, s2 = 576 - 2^-10 over 64 elements: mean = 3, s2 / cnt - mean^2 = -2^-16 in exact arithmetic and in
    fp64.  `if (var < 0.0) var = 0.0`: invstd = 1 / sqrt(eps), scale finite, running_var fed with 0."""
    g = gen(222)
    Cc, nb, count = 6, 2, 64
    p = fwd_partials(g, nb, Cc, count)
    p[:, 0, 0] = 96.0
    p[0, 1, 0], p[1, 1, 0] = 288.0, 288.0 - 2.0 ** -10
    res, ref = fin_check(g, Cc, nb, count, partials=p, premise=False)
    assert float(ref['var'][0][0]) == 0.0 and bool((ref['var'][0][1:] > 0).all())
    assert_bits(res['save_invstd'][1][:1], f32_bits(torch.tensor([1.0 / math.sqrt(FR.f32(EPS))], dtype=F64)), 'invstd of the clamped channel')
    assert math.isfinite(float(res['scale'][0][0])) and float(res['save_mean'][0][0]) == 3.0


# ---------------------------------------------------------------------------------------------------- dfl_bn_bwd_finalize
def bwd_partials(g, nb, Cc):
    """[nb][2][C] partial sums (dy, dy r) as exact data, scaled by channel and offset by row."""
    v = torch.randn(nb, 2, Cc, generator=g, dtype=F64) * chan(Cc, 2.0, 16.0) + 0.25 * (torch.arange(nb, dtype=F64) % 5).reshape(-1, 1, 1)
    return FR.quantize(v)


def bwd_check(g, Cc, nb, count):
    what = 'dfl_bn_bwd_finalize C=%d nblocks=%d count=%d' % (Cc, nb, count)
    part = Buf((nb, 2), Cc, Cc, False)
    pv = part.set(bwd_partials(g, nb, Cc))
    ins = {'partials': part, 'gamma': vec(torch.randn(Cc, generator=g) * 0.5 + chan(Cc, 1.0, 2.0).float()),
           'save_mean': vec(torch.randn(Cc, generator=g) + chan(Cc, -2.0, 2.0).float()), 'save_invstd': vec(torch.rand(Cc, generator=g) + 0.5)}
    outs = {'dgamma': out(Cc), 'dbeta': out(Cc), 'coef': Buf((3,), Cc, Cc, False).allow()}

    def once():
        ptrs = {k: b.upload() for k, b in list(ins.items()) + list(outs.items())}
        a = nat.BnBwdFinalizeArgs(count=count, nblocks=nb, C=Cc, **ptrs)
        sync(lib().dfl_bn_bwd_finalize(C.addressof(a), stream()), what)
        for k, b in ins.items():
            fetch(b, '%s %s' % (what, k))
        return [fetch(outs[k], '%s %s' % (what, k)) for k in ('dgamma', 'dbeta', 'coef')]
    (dgamma, _), (_, dbeta_bits), (coef, coef_bits) = twice(once, what)
    s = pv.sum(0)                                           # exact
    ref = FR.bn_bwd_finalize(s[0], s[1], ins['gamma'].stored, ins['save_mean'].stored, ins['save_invstd'].stored, count)
    assert_bits(dbeta_bits, f32_bits(s[0]), what + ' dbeta')
    assert_rounded(dgamma, ref['dgamma'][0], ref['dgamma'][1], K64_BWD, what + ' dgamma')
    assert_rounded(coef, ref['coef'][0].reshape(-1), ref['coef'][1].reshape(-1), K64_BWD, what + ' coef')
    if count == 0:
        # `count > 0 ? .. : 0.0`: A is one exact fp64 product of two fp32 values rounded once, B and C are zeros (of either sign)
        assert_bits(coef_bits[:Cc], f32_bits(ins['gamma'].stored * ins['save_invstd'].stored), what + ' A')
        assert not bool(coef[Cc:].any()), what + ': B, C must be 0 in eval mode'


@pytest.mark.parametrize('Cc,nb', FIN_CASES)
def test_bn_bwd_finalize(Cc, nb):
    bwd_check(gen(300 + Cc), Cc, nb, 16 * nb)


@pytest.mark.parametrize('Cc,nb', [(6, 1025), (257, 300)])
def test_bn_bwd_finalize_in_eval_mode(Cc, nb):
    bwd_check(gen(320 + Cc), Cc, nb, 0)


# ---------------------------------------------------------------------------------------------------- the _live forms
# bn_finalize_live_kernel / bn_bwd_finalize_live_kernel: `jobs[blockIdx.y]`, `c = blockIdx.x * 256 + threadIdx.x`, `c < j.C`; the
# grid is ceil(max_C / 256) x njobs.  Every array has room for max_C elements and more, NaN beyond its job's C.
LIVE_C, LIVE_MAXC, LIVE_ROOM = (5, 300, 513), 513, 576
LIVE_FWD = [dict(count=37, eps=1e-5, momentum=0.1, state=True), dict(count=240, eps=1e-3, momentum=0.25, state=False),
            dict(count=400, eps=1e-4, momentum=0.01, state=True)]


def live_totals(p):
    """Partial rows [BN_R][2][C] (exact data) as the fp64 totals the convolutions accumulate."""
    return Words(p.contiguous())


def test_bn_finalize_live_three_jobs():
    g = gen(400)
    jobs = []
    for k, (Cc, cfg) in enumerate(zip(LIVE_C, LIVE_FWD)):
        p = fwd_partials(g, nat.BN_R, Cc, cfg['count'])
        j = dict(cfg, C=Cc, p=p, totals=live_totals(p), gamma=vec(torch.randn(Cc, generator=g) * 0.5 + 1.5 + k, room=LIVE_ROOM - Cc),
                 beta=vec(torch.randn(Cc, generator=g) + k, room=LIVE_ROOM - Cc))
        j['outs'] = {n: out(Cc, LIVE_ROOM - Cc) for n in ('scale', 'shift', 'save_mean', 'save_invstd')}
        if cfg['state']:
            j['running_mean'] = vec(torch.randn(Cc, generator=g), room=LIVE_ROOM - Cc).allow()
            j['running_var'] = vec(torch.rand(Cc, generator=g) + 0.5, room=LIVE_ROOM - Cc).allow()
            j['nbt'] = Words(torch.tensor([7 + 1000 * k], dtype=torch.int64))
        jobs.append(j)
    names = ('scale', 'shift', 'save_mean', 'save_invstd')

    def once():
        arr = (nat.BnLiveJob * len(jobs))()
        for i, j in enumerate(jobs):
            arr[i].totals, arr[i].gamma, arr[i].beta = j['totals'].upload(), j['gamma'].upload(), j['beta'].upload()
            for n in names:
                setattr(arr[i], n, j['outs'][n].upload())
            if j['state']:
                arr[i].running_mean, arr[i].running_var, arr[i].num_batches_tracked = j['running_mean'].upload(), j['running_var'].upload(), j['nbt'].upload()
            arr[i].count, arr[i].C, arr[i].eps, arr[i].momentum = j['count'], j['C'], j['eps'], j['momentum']
        tab = table(arr)
        sync(lib().dfl_bn_finalize_live(tab.data_ptr(), len(jobs), LIVE_MAXC, stream()), 'dfl_bn_finalize_live')
        res = []
        for i, j in enumerate(jobs):
            what = 'dfl_bn_finalize_live job %d' % i
            j['totals'].fetch(what + ' totals')
            fetch(j['gamma'], what + ' gamma')
            fetch(j['beta'], what + ' beta')
            res += [fetch(j['outs'][n], '%s %s' % (what, n)) for n in names]
            if j['state']:
                res += [fetch(j['running_mean'], what + ' running_mean'), fetch(j['running_var'], what + ' running_var')]
                t = j['nbt'].fetch(what + ' num_batches_tracked', written=True)
                assert int(t[0]) == 8 + 1000 * i, '%s: num_batches_tracked went from %d to %d' % (what, 7 + 1000 * i, int(t[0]))
        return res
    res = iter(twice(once, 'dfl_bn_finalize_live'))
    for i, j in enumerate(jobs):
        s = j['p'].sum(0)
        ref = FR.bn_finalize(s[0], s[1], j['gamma'].stored, j['beta'].stored, j['count'], j['eps'], j['momentum'],
                             j['running_mean'].stored if j['state'] else None, j['running_var'].stored if j['state'] else None)
        assert bool((ref['var'][0] >= ref['save_mean'][0] ** 2 / 100).all())
        for n in names + (('running_mean', 'running_var') if j['state'] else ()):
            assert_rounded(next(res)[0], ref[n][0], ref[n][1], K64_FWD, 'dfl_bn_finalize_live job %d %s' % (i, n))


def test_bn_bwd_finalize_live_three_jobs():
    g = gen(410)
    jobs = []
    for k, Cc in enumerate(LIVE_C):
        p = bwd_partials(g, nat.BN_R, Cc) + 0.5 * k
        j = dict(C=Cc, p=p, totals=live_totals(p), save_mean=vec(torch.randn(Cc, generator=g) + k, room=LIVE_ROOM - Cc),
                 save_invstd=vec(torch.rand(Cc, generator=g) + 0.5 + k, room=LIVE_ROOM - Cc),
                 outs={n: out(Cc, LIVE_ROOM - Cc) for n in (('dgamma', 'dbeta') if k == 1 else ('dgamma', 'dbeta', 'sum_out'))})
        jobs.append(j)

    def once():
        arr = (nat.BnBwdLiveJob * len(jobs))()
        for i, j in enumerate(jobs):
            arr[i].totals, arr[i].save_mean, arr[i].save_invstd, arr[i].C = j['totals'].upload(), j['save_mean'].upload(), j['save_invstd'].upload(), j['C']
            for n, b in j['outs'].items():
                setattr(arr[i], n, b.upload())
        tab = table(arr)
        sync(lib().dfl_bn_bwd_finalize_live(tab.data_ptr(), len(jobs), LIVE_MAXC, stream()), 'dfl_bn_bwd_finalize_live')
        res = []
        for i, j in enumerate(jobs):
            what = 'dfl_bn_bwd_finalize_live job %d' % i
            j['totals'].fetch(what + ' totals')
            fetch(j['save_mean'], what + ' save_mean')
            fetch(j['save_invstd'], what + ' save_invstd')
            res += [fetch(b, '%s %s' % (what, n)) for n, b in j['outs'].items()]
        return res
    res = iter(twice(once, 'dfl_bn_bwd_finalize_live'))
    for i, j in enumerate(jobs):
        s = j['p'].sum(0)
        ref = FR.bn_bwd_finalize(s[0], s[1], torch.ones(j['C'], dtype=F64), j['save_mean'].stored, j['save_invstd'].stored, 1)
        for n in j['outs']:
            got, bits = next(res)
            if n == 'dgamma':
                assert_rounded(got, ref['dgamma'][0], ref['dgamma'][1], K64_BWD, 'dfl_bn_bwd_finalize_live job %d dgamma' % i)
            else:
                assert_bits(bits, f32_bits(s[0]), 'dfl_bn_bwd_finalize_live job %d %s' % (i, n))


# ---------------------------------------------------------------------------------------------------- dfl_bn_eval_prepare
# bn_eval_kernel, fp32: invstd = 1 / sqrtf(rv + eps) -- the add's u is halved by the root, + u of the root, + u of the division:
# 2.5 u -- scale = gamma * invstd: 3.5 u <= (3 + 1) u;  shift = beta - rm * scale (two roundings, or one if fused): 5.5 u <= (5 + 1) u.
# sqrtf and / are correctly rounded in this build (hipcc's default; csrc/build.sh passes no fast-math flag).
K_EVAL_SCALE, K_EVAL_SHIFT = 3, 5


@pytest.mark.parametrize('Cc', [1, 255, 256, 257])        # `c = blockIdx.x * blockDim.x + threadIdx.x`, `c < C`
def test_bn_eval_prepare(Cc):
    g = gen(500 + Cc)
    ins = [vec(torch.randn(Cc, generator=g) * 0.5 + chan(Cc, 1.0, 2.0).float()), vec(torch.randn(Cc, generator=g)),
           vec(torch.randn(Cc, generator=g) + chan(Cc, -2.0, 2.0).float()), vec(torch.rand(Cc, generator=g) * chan(Cc, 0.5, 4.0).float() + 0.01)]
    scale, shift = out(Cc), out(Cc)

    def once():
        sync(lib().dfl_bn_eval_prepare(*[b.upload() for b in ins], scale.upload(), shift.upload(), Cc, EPS, stream()), 'dfl_bn_eval_prepare')
        for b in ins:
            fetch(b, 'dfl_bn_eval_prepare inputs')
        return [fetch(scale, 'dfl_bn_eval_prepare scale'), fetch(shift, 'dfl_bn_eval_prepare shift')]
    (gs, _), (gh, _) = twice(once, 'dfl_bn_eval_prepare C=%d' % Cc)
    (rs, Ss), (rh, Sh) = FR.bn_eval(*[b.stored for b in ins], EPS)
    assert_close(gs, rs, Ss, K_EVAL_SCALE, False, 'dfl_bn_eval_prepare C=%d scale' % Cc)
    assert_close(gh, rh, Sh, K_EVAL_SHIFT, False, 'dfl_bn_eval_prepare C=%d shift' % Cc)


# ---------------------------------------------------------------------------------------------------- the flat optimizer steps
# optim_kernel: `i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x` under stream_grid's cap.
OPT_NS = [1, 255, 256, 257]
OPT_BIG = GRID_CAP + 257              # 257 elements in the second pass of the grid-stride loop; 8.4 MB per tensor
LR, WD, GS = 0.05, 1e-3, 0.75
# SgdRule: g = fmaf(wd, w, gr * gscale) [2]; nb = fmaf(mom, b, g) [3]; g = fmaf(mom, nb, g) [4, nesterov]; fmaf(-lr, g, w) [last]
K_SGD_BUF = 3


def k_sgd_p(mom, nesterov):
    return 3 + int(mom != 0.0) + int(nesterov)


# AdamRule (no contraction, every operation rounded): g = gr * gscale + wd * w [2]; d = g - m [3]; m = m + w1 * d [5];
# v = v * beta2 + (omb2 * g) * g [(3) + (2) + 1 for the product of two sums, + 1 = 7];
# den = sqrt(v) / bc2 + eps: relative error 7/2 (S_v / v) + 3;  m / den: 5 + 3.5 + 3 + 1 <= 13 with the factor S_v / v in S
# (finalize_ref);  w - step_size * (..): 15.
K_ADAM_M, K_ADAM_V, K_ADAM_P = 5, 7, 15
# RmspropRule: sq as Adam's v [7]; avg = sqrt(sq) + eps: 7/2 (S_v / v) + 2;  g / avg: 2 + 3.5 + 2 + 1 <= 9;
# buf = buf * mom + (..) [10]; w + -lr * buf [12];  without momentum: -lr * (g / avg) [10], w + (..) [11].
K_RMS_SQ, K_RMS_BUF, K_RMS_P_MOM, K_RMS_P = 7, 10, 12, 11
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
RMS = dict(lr=1e-2, alpha=0.99, eps=1e-8)


def rnd(g, n, scale=1.0, pos=False):
    v = torch.rand(n, generator=g) + 0.1 if pos else torch.randn(n, generator=g)
    return v * scale


def sgd_check(n, mom, nesterov, first, wd, seed):
    g = gen(seed)
    what = 'dfl_sgd_step n=%d momentum=%g nesterov=%d first=%d wd=%g' % (n, mom, nesterov, first, wd)
    w, gr = vec(rnd(g, n)).allow(), vec(rnd(g, n, 2.0))
    buf = vec(rnd(g, n, 3.0)).allow() if mom else None       # non-zero also on a first step, which must overwrite it with g

    def once():
        sync(lib().dfl_sgd_step(w.upload(), gr.upload(), buf.upload() if buf else None, n, LR, mom, wd, GS, nesterov, first, stream()), what)
        fetch(gr, what + ' grad')
        return [fetch(w, what + ' p')] + ([fetch(buf, what + ' buf')] if buf else [])
    res = twice(once, what)
    (rp, Sp), rb = FR.sgd_step(w.stored, gr.stored, buf.stored if buf else None, LR, mom, wd, GS, nesterov, first)
    assert_close(res[0][0], rp, Sp, k_sgd_p(mom, nesterov), False, what + ' p')
    if buf:
        assert_close(res[1][0], rb[0], rb[1], K_SGD_BUF, False, what + ' buf')


SGD_FORMS = [(0.0, 0), (0.9, 0), (0.9, 1)]


@pytest.mark.parametrize('wd', [0.0, WD])
@pytest.mark.parametrize('first', [0, 1])
@pytest.mark.parametrize('mom,nesterov', SGD_FORMS)
def test_sgd_step(mom, nesterov, first, wd):
    for n in OPT_NS:
        sgd_check(n, mom, nesterov, first, wd, 600 + n)


@pytest.mark.parametrize('mom,nesterov,first', [(0.0, 0, 0), (0.9, 1, 1)])
def test_sgd_step_grid_stride(mom, nesterov, first):
    assert GRID_CAP < OPT_BIG < 2 * GRID_CAP
    sgd_check(OPT_BIG, mom, nesterov, first, WD, 610)


def adam_coefs(t):
    return ADAM['lr'] / (1.0 - ADAM['beta1'] ** t), math.sqrt(1.0 - ADAM['beta2'] ** t)


def adam_call(p, gr, m, v, n, t):
    step_size, bc2 = adam_coefs(t)
    return lib().dfl_adam_step(p, gr, m, v, n, ADAM['lr'], ADAM['beta1'], ADAM['beta2'], ADAM['eps'], WD, step_size, bc2, GS, stream())


def adam_check(n, seed):
    """Three consecutive steps from a non-zero state; each step is held against the model applied to the state the GPU left."""
    g = gen(seed)
    w, gr, m, v = vec(rnd(g, n)).allow(), vec(rnd(g, n)), vec(rnd(g, n, 0.1)).allow(), vec(rnd(g, n, 0.01, pos=True)).allow()
    f = [b.stored.float().numpy() for b in (w, m, v)]          # the same three steps op by op in numpy float32
    for t in (1, 2, 3):
        what = 'dfl_adam_step n=%d step %d' % (n, t)
        grad = gr.set(rnd(g, n, float(t)).reshape(1, -1))[0]

        def once():
            sync(adam_call(w.upload(), gr.upload(), m.upload(), v.upload(), n, t), what)
            fetch(gr, what + ' grad')
            return [fetch(b, '%s %s' % (what, s)) for b, s in ((w, 'p'), (m, 'exp_avg'), (v, 'exp_avg_sq'))]
        res = twice(once, what)
        step_size, bc2 = adam_coefs(t)
        refs = FR.adam_step(w.stored, grad, m.stored, v.stored, ADAM['beta1'], ADAM['beta2'], ADAM['eps'], WD, step_size, bc2, GS)
        for (got, _), (ref, S), k, s in zip(res, refs, (K_ADAM_P, K_ADAM_M, K_ADAM_V), ('p', 'exp_avg', 'exp_avg_sq')):
            assert_close(got, ref, S, k, False, '%s %s' % (what, s))
        f = list(FR.adam_step_f32(f[0], grad.float().numpy(), f[1], f[2], ADAM['beta1'], ADAM['beta2'], ADAM['eps'], WD, step_size, bc2, GS))
        for b, (got, _) in zip((w, m, v), res):
            b.stored = b.set(got.reshape(1, -1))[0]
    differ = sum(int((torch.from_numpy(a).view(torch.int32) != f32_bits(b.stored)).sum()) for a, b in zip(f, (w, m, v)))
    print('MEASURED adam n=%d: %d of %d elements (p, exp_avg, exp_avg_sq) differ in their bits from the op-by-op float32 numpy '
          'restatement after three steps' % (n, differ, 3 * n))


def test_adam_step():
    for n in OPT_NS:
        adam_check(n, 620 + n)


def test_adam_step_grid_stride():
    adam_check(OPT_BIG, 630)


def rms_call(p, gr, sq, buf, n, mom):
    return lib().dfl_rmsprop_step(p, gr, sq, buf, n, RMS['lr'], RMS['alpha'], RMS['eps'], WD, mom, GS, stream())


def rms_check(n, mom, seed):
    g = gen(seed)
    w, gr, sq = vec(rnd(g, n)).allow(), vec(rnd(g, n)), vec(rnd(g, n, 0.5, pos=True)).allow()
    buf = vec(rnd(g, n, 2.0)).allow() if mom else None
    state = [b for b in (w, sq, buf) if b is not None]
    f = [b.stored.float().numpy() for b in state]
    for t in (1, 2, 3):
        what = 'dfl_rmsprop_step n=%d momentum=%g step %d' % (n, mom, t)
        grad = gr.set(rnd(g, n, float(t)).reshape(1, -1))[0]

        def once():
            sync(rms_call(w.upload(), gr.upload(), sq.upload(), buf.upload() if buf else None, n, mom), what)
            fetch(gr, what + ' grad')
            return [fetch(b, what) for b in state]
        res = twice(once, what)
        refs = [r for r in FR.rmsprop_step(w.stored, grad, sq.stored, buf.stored if buf else None, RMS['lr'], RMS['alpha'], RMS['eps'],
                                           WD, mom, GS) if r is not None]
        for (got, _), (ref, S), k, s in zip(res, refs, (K_RMS_P_MOM if mom else K_RMS_P, K_RMS_SQ, K_RMS_BUF), ('p', 'square_avg', 'buf')):
            assert_close(got, ref, S, k, False, '%s %s' % (what, s))
        f = [a for a in FR.rmsprop_step_f32(f[0], grad.float().numpy(), f[1], f[2] if mom else None, RMS['lr'], RMS['alpha'], RMS['eps'],
                                            WD, mom, GS) if a is not None]
        for b, (got, _) in zip(state, res):
            b.stored = b.set(got.reshape(1, -1))[0]
    differ = sum(int((torch.from_numpy(a).view(torch.int32) != f32_bits(b.stored)).sum()) for a, b in zip(f, state))
    print('MEASURED rmsprop momentum=%g n=%d: %d of %d elements differ in their bits from the op-by-op float32 numpy restatement '
          'after three steps' % (mom, n, differ, len(state) * n))


@pytest.mark.parametrize('mom', [0.0, 0.9])
def test_rmsprop_step(mom):
    for n in OPT_NS:
        rms_check(n, mom, 640 + n)


@pytest.mark.parametrize('mom', [0.0, 0.9])
def test_rmsprop_step_grid_stride(mom):
    rms_check(OPT_BIG, mom, 650)


# ---------------------------------------------------------------------------------------------------- update + tiled re-layout
# pack_tile: the binary search `jobs[mid].first_tile <= blockIdx.x`; a tiled job has (A / 32) * (B / 32) workgroups; a
# DFL_PACK_PLAIN job one per DFL_SGD_PLAIN_TILE elements, `i1 = min(A, i0 + DFL_SGD_PLAIN_TILE)`.
TILE = nat.SGD_PLAIN_TILE
PACK_JOBS = [dict(A=32, B=32, C=1, kind=1, split=0),
             dict(A=64, B=32, C=9, kind=1, split=2, kind2=2, flip2=1, split2=1),      # the forward and the data-gradient operand
             dict(A=32, B=64, C=4, kind=3, split=1)] + [dict(A=a, plain=True) for a in (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 5)]
RULES = ['sgd', 'adam', 'rmsprop_mom', 'rmsprop']


def rule_states(rule):
    """(has state 1, has state 2)"""
    return {'sgd': (True, False), 'adam': (True, True), 'rmsprop_mom': (True, True), 'rmsprop': (True, False)}[rule]


def flat_step(rule, p, gr, s1, s2, n):
    """The flat kernel (dfl_*_step) on device tensors, in place."""
    if rule == 'sgd':
        rc = lib().dfl_sgd_step(p.data_ptr(), gr.data_ptr(), s1.data_ptr(), n, LR, 0.9, WD, GS, 1, 0, stream())
    elif rule == 'adam':
        rc = adam_call(p.data_ptr(), gr.data_ptr(), s1.data_ptr(), s2.data_ptr(), n, 2)
    else:
        mom = 0.9 if rule == 'rmsprop_mom' else 0.0
        rc = rms_call(p.data_ptr(), gr.data_ptr(), s1.data_ptr(), s2.data_ptr() if mom else None, n, mom)
    sync(rc, 'flat ' + rule)


def fused_step(rule, tab, njobs, tiles, gd, d1, d2):
    if rule == 'sgd':
        a = nat.SgdPackArgs(jobs_dev=tab.data_ptr(), grad_delta=gd, buf_delta=d1, njobs=njobs, total_tiles=tiles, lr=LR, momentum=0.9,
                            weight_decay=WD, grad_scale=GS, nesterov=1)
        return lib().dfl_sgd_pack_tiled(C.addressof(a), stream())
    step_size, bc2 = adam_coefs(2)
    a = nat.OptimPackArgs(jobs_dev=tab.data_ptr(), grad_delta=gd, state1_delta=d1, state2_delta=d2, njobs=njobs, total_tiles=tiles,
                          kind=nat.OPTIM_ADAM if rule == 'adam' else nat.OPTIM_RMSPROP, weight_decay=WD, grad_scale=GS,
                          beta1=ADAM['beta1'], beta2=ADAM['beta2'], step_size=step_size, bc2_sqrt=bc2, alpha=RMS['alpha'],
                          lr=ADAM['lr'] if rule == 'adam' else RMS['lr'], eps=ADAM['eps'] if rule == 'adam' else RMS['eps'],
                          momentum=0.9 if rule == 'rmsprop_mom' else 0.0)
    return lib().dfl_optim_pack_tiled(C.addressof(a), stream())


def layout_buf(j, split):
    """A layout of a tiled job: A * B * C elements in every format (4-byte slots of the quad forms, bf16 of the chunk form)."""
    return Buf((1,), j['A'] * j['B'] * j['C'], j['A'] * j['B'] * j['C'], split == 2).allow()


def pack_record(rec, j, src, dst, dst2, first_tile):
    rec.src, rec.A, rec.first_tile = src, j['A'], first_tile
    if j.get('plain'):
        rec.kind = nat.PACK_PLAIN
        return -(-j['A'] // TILE)
    rec.dst, rec.B, rec.C, rec.kind, rec.flip, rec.split = dst, j['B'], j['C'], j['kind'], j.get('flip', 0), j['split']
    if dst2 is not None:
        rec.dst2, rec.kind2, rec.flip2, rec.split2 = dst2, j['kind2'], j['flip2'], j['split2']
    return (j['A'] // 32) * (j['B'] // 32)


@pytest.mark.parametrize('which', [tuple(range(len(PACK_JOBS))), (1,), (2, 7)], ids=['all_jobs', 'one_job', 'two_jobs'])
@pytest.mark.parametrize('rule', RULES)
def test_update_with_tiled_relayout(rule, which):
    g = gen(700)
    jobs = [dict(PACK_JOBS[k]) for k in which]
    has1, has2 = rule_states(rule)
    # one allocation, four arenas of one layout: parameters, gradients, state 1, state 2 at distinct deltas (multiples of 4);
    # jobs back to back with NaN gaps of 4, 8, 12 .. elements between them
    pos = 4
    for k, j in enumerate(jobs):
        j['n'] = j['A'] if j.get('plain') else j['A'] * j['B'] * j['C']
        j['at'] = pos
        pos += j['n'] + 4 * (k + 1)
        if not jobs[min(k + 1, len(jobs) - 1)].get('plain'):
            pos = -(-pos // 4) * 4                     # a tiled job's 16-byte accesses
    L = -(-pos // 4) * 4
    gd, d1, d2 = L + 8, 2 * L + 20, 3 * L + 36
    arena = Buf((1,), 4 * L + 48, 4 * L + 48, False)
    values, writable = arena._view(arena.host.view(torch.float32))[0], arena._view(arena.writable)[0]
    for j in jobs:
        a, n = j['at'], j['n']
        values[a:a + n], values[gd + a:gd + a + n] = rnd(g, n), rnd(g, n, 2.0)
        writable[a:a + n] = True
        if has1:
            values[d1 + a:d1 + a + n] = rnd(g, n, 0.5, pos=True)
            writable[d1 + a:d1 + a + n] = True
        if has2:                                       # RMSprop without momentum: the whole of state 2 stays NaN and untouched
            values[d2 + a:d2 + a + n] = rnd(g, n, 0.3, pos=rule == 'adam')      # Adam's exp_avg_sq is no less than 0
            writable[d2 + a:d2 + a + n] = True
        if not j.get('plain'):
            j['dst'] = layout_buf(j, j['split'])
            j['dst2'] = layout_buf(j, j['split2']) if 'kind2' in j else None
    # what is expected: the flat kernel over each job's elements, then dfl_pack_weights_tiled on the updated master (and, below,
    # tests/pack_ref.py's bytes of that master: the two launches share their emitters)
    for j in jobs:
        a, n = j['at'], j['n']
        dev = [values[o + a:o + a + n].to(DEV) if on else None for o, on in ((0, True), (gd, True), (d1, has1), (d2, has2))]
        flat_step(rule, *dev, n)
        j['expect'] = [None if t is None else t.cpu().view(torch.int32) for t in (dev[0], dev[2], dev[3])]
        j['master'] = dev[0]
    tiled = [j for j in jobs if not j.get('plain')]
    arr, tiles = (nat.PackJob * max(len(tiled), 1))(), 0
    for i, j in enumerate(tiled):
        j['ref_dst'] = torch.zeros_like(j['dst'].host).to(DEV)
        j['ref_dst2'] = torch.zeros_like(j['dst2'].host).to(DEV) if j['dst2'] is not None else None
        tiles += pack_record(arr[i], j, j['master'].data_ptr(), j['ref_dst'].data_ptr() + j['dst'].off * j['dst'].host.element_size(),
                             None if j['dst2'] is None else j['ref_dst2'].data_ptr() + j['dst2'].off * j['dst2'].host.element_size(), tiles)
    if tiled:
        tab = table(arr)
        sync(lib().dfl_pack_weights_tiled(tab.data_ptr(), len(tiled), tiles, stream()), 'dfl_pack_weights_tiled')

    def once():
        arr, tiles = (nat.PackJob * len(jobs))(), 0
        base = arena.upload()
        for i, j in enumerate(jobs):
            tiles += pack_record(arr[i], j, base + 4 * j['at'], None if j.get('plain') else j['dst'].upload(),
                                 j['dst2'].upload() if j.get('dst2') is not None else None, tiles)
        tab = table(arr)
        sync(fused_step(rule, tab, len(jobs), tiles, gd, d1, d2), 'fused ' + rule)
        res = [fetch(arena, 'fused %s: the arenas' % rule, finite=False)]
        for j in tiled:
            res += [fetch(b, 'fused %s: a layout' % rule) for b in (j['dst'], j['dst2']) if b is not None]
        return res
    res = twice(once, 'fused ' + rule)
    bits = res[0][1]
    layouts = iter(res[1:])
    for k, j in zip(which, jobs):
        a, n = j['at'], j['n']
        for name, o, exp in (('parameters', 0, j['expect'][0]), ('state 1', d1, j['expect'][1]), ('state 2', d2, j['expect'][2])):
            if exp is not None:
                assert_bits(bits[o + a:o + a + n], exp, 'fused %s job %d: %s against the flat kernel' % (rule, k, name))
        if not j.get('plain'):
            updated = j['expect'][0].view(torch.float32).numpy().reshape(j['A'], j['B'], j['C'])
            for b, ref, form in ((j['dst'], j['ref_dst'], (j['kind'], j.get('flip', 0), j['split'])),
                                 (j['dst2'], j['ref_dst2'], (j.get('kind2'), j.get('flip2'), j.get('split2')))):
                if b is not None:
                    got = next(layouts)[1]
                    assert_bits(got, ref.cpu()[b.off:b.off + got.numel()], 'fused %s job %d: a layout against dfl_pack_weights_tiled' % (rule, k))
                    assert_bits(got.contiguous().view(torch.uint8), torch.from_numpy(PK.encode(updated, *form)),
                                'fused %s job %d: a layout against pack_ref of the updated master' % (rule, k))


# ---------------------------------------------------------------------------------------------------- refusals
# Every DFL_REQUIRE of the entry points above that tests/test_optim_cpu.py does not pin: -1, the message, and nothing written.
# All pointers are real (small, NaN-filled): a call that were accepted would still stay inside them.
def _fin(p, **kw):
    a = dict(partials=p[0], gamma=p[1], beta=p[2], running_mean=p[3], running_var=p[4], num_batches_tracked=p[5], scale=p[6], shift=p[7],
             save_mean=p[8], save_invstd=p[9], count=16, nblocks=2, C=4, eps=EPS, momentum=MOM)
    a.update(kw)
    a = nat.BnFinalizeArgs(**a)
    return lib().dfl_bn_finalize(C.addressof(a), stream())


def _bwd(p, **kw):
    a = dict(partials=p[0], gamma=p[1], save_mean=p[2], save_invstd=p[3], dgamma=p[4], dbeta=p[5], coef=p[6], count=16, nblocks=2, C=4)
    a.update(kw)
    a = nat.BnBwdFinalizeArgs(**a)
    return lib().dfl_bn_bwd_finalize(C.addressof(a), stream())


def _eval(p, C=4, **kw):
    a = dict(gamma=p[0], beta=p[1], rm=p[2], rv=p[3], scale=p[4], shift=p[5])
    a.update(kw)
    return lib().dfl_bn_eval_prepare(a['gamma'], a['beta'], a['rm'], a['rv'], a['scale'], a['shift'], C, EPS, stream())


def _sgd_pack(p, **kw):
    a = dict(jobs_dev=p[0], grad_delta=64, buf_delta=128, njobs=1, total_tiles=1, lr=LR, momentum=0.9, weight_decay=WD, grad_scale=1.0, nesterov=1)
    a.update(kw)
    a = nat.SgdPackArgs(**a)
    return lib().dfl_sgd_pack_tiled(C.addressof(a), stream())


REFUSALS = (
    [('bn_finalize %s' % k, lambda p, k=k: _fin(p, **{k: None}), b'dfl_bn_finalize: missing pointer')
     for k in ('partials', 'gamma', 'beta', 'scale', 'shift', 'save_mean', 'save_invstd')]
    + [('bn_finalize %s' % (kw,), lambda p, kw=kw: _fin(p, **kw), b'dfl_bn_finalize: bad sizes')
       for kw in (dict(C=0), dict(nblocks=0), dict(count=0), dict(count=-5))]
    + [('bn_finalize %s alone' % k, lambda p, k=k: _fin(p, **{k: None}), b'dfl_bn_finalize: running stats go together')
       for k in ('running_mean', 'running_var')]
    + [('bn_bwd_finalize %s' % k, lambda p, k=k: _bwd(p, **{k: None}), b'dfl_bn_bwd_finalize: missing pointer')
       for k in ('partials', 'gamma', 'save_mean', 'save_invstd', 'dgamma', 'dbeta', 'coef')]
    + [('bn_bwd_finalize %s' % (kw,), lambda p, kw=kw: _bwd(p, **kw), b'dfl_bn_bwd_finalize: bad sizes')
       for kw in (dict(C=0), dict(nblocks=0), dict(count=-1))]
    + [('bn_eval_prepare %s' % k, lambda p, k=k: _eval(p, **{k: None}), b'dfl_bn_eval_prepare: bad args')
       for k in ('gamma', 'beta', 'rm', 'rv', 'scale', 'shift')]
    + [('bn_eval_prepare C=0', lambda p: _eval(p, C=0), b'dfl_bn_eval_prepare: bad args')]
    + [('%s %s' % (fn, what), lambda p, fn=fn, a=a: getattr(lib(), fn)(p[0] if a[0] else None, a[1], a[2], stream()), fn.encode() + b': bad args')
       for fn in ('dfl_bn_finalize_live', 'dfl_bn_bwd_finalize_live', 'dfl_reduce_batch')
       for what, a in (('no jobs', (0, 1, 1)), ('njobs=0', (1, 0, 1)), ('max_C / total_blocks = 0', (1, 1, 0)))]
    + [('reduce_partials %s' % what, lambda p, a=a: lib().dfl_reduce_partials(p[0] if a[0] else None, p[1] if a[1] else None, a[2], a[3], a[4], stream()),
        b'dfl_reduce_partials: bad args')
       for what, a in (('no partials', (0, 1, 2, 4, 4)), ('no out', (1, 0, 2, 4, 4)), ('nblocks=0', (1, 1, 0, 4, 4)), ('C=0', (1, 1, 2, 4, 0)),
                       ('stride < C', (1, 1, 2, 3, 4)))]
    + [('reduce_job_blocks %s' % (a,), lambda p, a=a: lib().dfl_reduce_job_blocks(*a), b'dfl_reduce_job_blocks: bad args') for a in ((0, 3), (8, 0), (-1, 3))]
    + [('sum_partials %s' % what, lambda p, a=a: lib().dfl_sum_partials(p[0] if a[0] else None, p[1] if a[1] else None, a[2], a[3], 1, stream()),
        b'dfl_sum_partials: bad args')
       for what, a in (('no src', (0, 1, 8, 2)), ('no dst', (1, 0, 8, 2)), ('n < 0', (1, 1, -8, 2)), ('splits=0', (1, 1, 8, 0)))]
    + [('sgd_step %s' % what, lambda p, a=a: lib().dfl_sgd_step(p[0] if a[0] else None, p[1] if a[1] else None, p[2] if a[2] else None, a[3], LR, a[4],
                                                               0.0, 1.0, 0, 0, stream()), msg)
       for what, a, msg in (('no p', (0, 1, 1, 8, 0.9), b'dfl_sgd_step: bad args'), ('no grad', (1, 0, 1, 8, 0.9), b'dfl_sgd_step: bad args'),
                            ('n=0', (1, 1, 1, 0, 0.9), b'dfl_sgd_step: bad args'),
                            ('momentum without a buffer', (1, 1, 0, 8, 0.9), b'dfl_sgd_step: momentum buffer required'))]
    + [('sgd_pack_tiled %s' % (kw,), lambda p, kw=kw: _sgd_pack(p, **kw), msg)
       for kw, msg in ((dict(jobs_dev=None), b'empty job list'), (dict(njobs=0), b'empty job list'), (dict(total_tiles=0), b'empty job list'),
                       (dict(grad_delta=66), b'16-byte congruent'), (dict(buf_delta=129), b'16-byte congruent'),
                       (dict(momentum=-0.5, nesterov=0), b'nesterov needs a momentum'), (dict(momentum=0.0), b'nesterov needs a momentum'))]
    + [('sgd_pack_tiled NULL', lambda p: lib().dfl_sgd_pack_tiled(None, stream()), b'dfl_sgd_pack_tiled: empty job list')])


@pytest.mark.parametrize('case', REFUSALS, ids=[re.sub(r'[^A-Za-z0-9=.-]+', '_', r[0]).strip('_') for r in REFUSALS])
def test_bad_arguments_are_refused_before_anything_is_launched(case):
    name, call, msg = case
    bufs = [vec(n=256) for _ in range(10)]             # nothing of them is writable
    rc = call([b.upload() for b in bufs])
    torch.cuda.synchronize()
    assert rc == -1, '%s: accepted (%d)' % (name, rc)
    assert msg in lib().dfl_last_error(), (name, lib().dfl_last_error())
    for b in bufs:
        fetch(b, name, finite=False)
