"""The kernels of csrc/prep.hip -- dfl_prep_batch (prep_stats_kernel, prep_write_kernel), dfl_est_lands (est_lands_scan_kernel,
est_lands_kernel) and dfl_hard_dice (hard_dice_count_kernel, hard_dice_final_kernel) -- through the C ABI, against the float64
models of tests/prep_ref.py: in every regime of their loops (less than a workgroup, a second trip, a second pass of the capped
grid; empty workgroups, a partly filled unroll and a second outer trip of the arg-max scan), at the edges of their contracts
(largest reflect, the view's boundary to one float32 step, ties of the arg-max across workgroups, unroll slots and trips, labels
>= C, NULL outputs), and at what the entry points must refuse.  tests/test_prep_ref_cpu.py holds the same cases against the
regimes and the models against the oracle.

Every operand lives inside a larger allocation (Slab) filled with a NaN bit pattern, or 0xA5 bytes for integer operands: what the
contract does not let a call write must keep its bits.  Every call is made twice on the same inputs and must return the same
bytes (the statistics are summed in a fixed order; the rest is integer or per-pixel work).

Tolerances are derived next to where they are applied, none is tuned; u = 2^-24.  Each test prints the largest ratio of error to
bound it met ("RATIO ...")."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from dfl_amd import _native as nat
import prep_ref as PR

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24
U64 = 2.0 ** -53
TINY = 2.0 ** -126              # the smallest positive normal of float32
GUARD = 256                     # sentinel bytes in front of and behind every operand (keeps the operand's alignment)
SENT = {4: np.uint32(0x7fc12345), 8: np.uint64(0x7ff8123456789abc)}     # quiet NaNs, float32 and float64


def stream():
    return torch.cuda.current_stream().cuda_stream


class Slab:
    """An operand inside a host array of sentinels that is uploaded for a call and compared with what comes back.
    data: the operand's contents (an input), or None: an output of `shape` that holds the sentinel before the call."""

    def __init__(self, dtype, shape=None, data=None, shift=0):
        self.dtype = np.dtype(dtype)
        if data is not None:
            data = np.ascontiguousarray(data, dtype=self.dtype)
            shape = data.shape
        self.shape, self.shift = tuple(shape), shift
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        total = GUARD + shift + self.nbytes + GUARD
        total += -total % 8
        if self.dtype.kind == 'f':
            self.host = np.full(total // self.dtype.itemsize, SENT[self.dtype.itemsize]).view(np.uint8)
        else:
            self.host = np.full(total, 0xA5, np.uint8)
        self.lo = GUARD + shift
        if data is not None:
            self.host[self.lo:self.lo + self.nbytes] = data.reshape(-1).view(np.uint8)
        self.dev = None

    def upload(self):
        self.dev = torch.from_numpy(self.host.copy()).to(DEV)
        return self.dev.data_ptr() + self.lo

    def fetch(self, what, written=True):
        """The operand after the call; everything around it -- and the operand itself unless `written` -- must have kept its bits."""
        after = self.dev.cpu().numpy()
        keep = np.ones(after.size, bool)
        if written:
            keep[self.lo:self.lo + self.nbytes] = False
        changed = after[keep] != self.host[keep]
        assert not changed.any(), '%s: %d bytes outside the contract region were written' % (what, int(changed.sum()))
        return after[self.lo:self.lo + self.nbytes].view(self.dtype).reshape(self.shape).copy()


def twice(fn, args, slabs, fields, addr=True):
    """Upload, call and fetch, two times over; -> (return code, {name: operand after the call}).  slabs: {name: (Slab, written)};
    fields: {name: field of args that takes the slab's address} (a name missing here is allocated but not passed)."""
    out = None
    for rep in range(2):
        for name, (slab, _) in slabs.items():
            p = slab.upload()
            if name in fields:
                setattr(args, fields[name], p)
        rc = getattr(nat.lib(), fn)(C.addressof(args), stream())
        torch.cuda.synchronize()
        got = {name: slab.fetch('%s %s' % (fn, name), written and rc == 0) for name, (slab, written) in slabs.items()}
        if out is not None:
            assert rc == out[0]
            for name in got:
                assert got[name].tobytes() == out[1][name].tobytes(), '%s: %s differs between two calls on the same inputs' % (fn, name)
        out = (rc, got)
    return out


def ok(fn, rc):
    assert rc == 0, '%s refused (%d): %s' % (fn, rc, nat.lib().dfl_last_error().decode())


RATIO = {}


def ratio(kind, err, bound, what):
    """Hold err <= bound everywhere and note the largest err / bound per output kind."""
    err, bound = np.asarray(err, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(err))
    assert np.isfinite(err).all(), '%s: non-finite outputs' % what
    r = float((err / bound).max())
    RATIO[kind] = max(RATIO.get(kind, 0.0), r)
    print('RATIO %s %.4f  (%s; largest so far %.4f)' % (kind, r, what, RATIO[kind]))
    bad = err > bound
    assert not bad.any(), '%s: %d of %d elements off, worst err / bound %.3f (|err| %.3e)' % (
        what, int(bad.sum()), bad.size, r, float(err.ravel()[(err / bound).argmax()]))


# ==================================================================================================== dfl_prep_batch
def prep_slabs(B, H, W, pad, C_, L, kind='uniform', foreign=(200, 255), start=0):
    img = PR.prep_images(kind, B, H, W)
    labels = PR.prep_labels(B, H, W, C_, foreign=foreign if C_ == 7 else ())
    lands, view = PR.prep_lands(B, H, W, L, start)
    slabs = {'proj': (Slab(np.float32, data=img), False), 'labels': (Slab(np.uint8, data=labels), False),
             'lands': (Slab(np.float32, data=lands), False),
             'x': (Slab(np.float32, (B, H + 2 * pad, W + 2 * pad)), True), 'masks': (Slab(np.float32, (B, C_, H, W)), True),
             'heats': (Slab(np.float32, (B, L, H, W)), True),
             'scratch': (Slab(np.float64, (int(nat.lib().dfl_prep_scratch_doubles(B)),)), True)}
    return slabs, (img, labels, lands, view)


def prep_args(B, H, W, pad, C_, L, sigma, standardize):
    return nat.PrepArgs(B=B, H=H, W=W, pad=pad, C=C_, L=L, sigma=sigma, standardize=standardize)


ALL = {k: k for k in ('proj', 'labels', 'lands', 'x', 'masks', 'heats', 'scratch')}


def check_x(got, img, pad, what):
    """x = fl(fl(src - fl32(m')) * fl32(1 / sd')) with m', sd' the kernel's float64 statistics, against ref = (src - m) / sd:
        src - fl32(m') = (src - m) + (m - fl32(m')),  |m - fl32(m')| <= u |m|  (+ the float64 error of m', far below it)
      so after the division by sd the mean's rounding leaves u |m| / sd, and the subtraction, the rounding of 1 / sd' to float32 and
      the product leave 3 u |ref| (4 u |ref| with the second-order terms).  sd' itself: the kernel forms the variance in one pass as
      (s2 - s1 * (s1 / n)) / (n - 1) from float64 sums of n terms.  Summed in ANY order, s2 and s1 carry a relative error of at most
      (n - 1) 2^-53 each (all terms of s2 are positive, and those of s1 are for these images), so s1^2 / n carries 2 (n - 1) + 2 of
      them; both are n (m^2 + sd^2) to within a factor (n - 1) / n, and their difference is (n - 1) sd^2:
        |var' - var| / var <= 2^-53 (3 (n - 1) + 3) n (m^2 + sd^2) / ((n - 1) sd^2) <= 3 (n + 2) 2^-53 (m^2 + sd^2) / sd^2
      and the square root halves it:  d = 1.5 (n + 2) 2^-53 (m^2 + sd^2) / sd^2.
        |x - ref| <= u (4 |ref| + |m| / sd) + d |ref|"""
    for b in range(img.shape[0]):
        ref, m, sd = PR.standardize(img[b], pad)
        n = ref.size
        d = 1.5 * (n + 2) * U64 * (m * m + sd * sd) / (sd * sd)
        ratio('x', np.abs(got[b] - ref), U * (4.0 * np.abs(ref) + abs(m) / sd) + d * np.abs(ref), '%s image %d' % (what, b))


def check_masks(got, labels, C_, what):
    want = np.stack([PR.one_hot(l, C_) for l in labels])
    assert got.tobytes() == want.tobytes(), '%s: %d mask values differ' % (what, int((got != want).sum()))


def check_heats(got, lands, view, H, W, sigma, what):
    """got = fl(expf(fl(fl(dx^2 + dy^2) * kexp)) * knorm) in float32 against ref = exp(e) / (2 pi sigma^2):
      the exponent: dx, dy one rounding each (2 u relative in their squares), the squares, their sum and the product with kexp one
      each, kexp = fl(1 / fl(-2 fl(sigma^2))) two: at most 8 u |e| absolute in the argument of exp, hence 8 |e| u relative in the
      result; expf itself (1 ulp = 2 u), knorm (3 roundings) and the final product: 8 u with room.  A result below 2^-126 may be
      flushed to zero by the device:  |got - ref| <= (8 |e| + 8) u ref + 2^-126.  A map out of view is zero exactly."""
    for b in range(lands.shape[0]):
        ref, e = PR.heat(lands[b], H, W, sigma)
        for l in range(lands.shape[2]):
            if not view[b, l]:
                assert not got[b, l].any() and not np.signbit(got[b, l]).any(), '%s: out-of-view map (%d, %d) is not zero' % (what, b, l)
        ratio('heats', np.abs(got[b] - ref), (8.0 * np.abs(e) + 8.0) * U * ref + TINY, '%s image %d' % (what, b))
        assert bool(view[b].any()) == bool(got[b].any())


def shape_id(s):
    return 'x'.join(str(v) for v in s)


PREP_RUNS = [(s, k) for s in PR.PREP_SHAPES[:4] for k in ('uniform', 'offset', 'scaled')] + [(PR.PREP_BIG, 'uniform')]


@pytest.mark.parametrize('shape,kind', PREP_RUNS, ids=['%s-%s' % (shape_id(s), k) for s, k in PREP_RUNS])
def test_prep_batch_all_outputs(shape, kind):
    """x, masks and heats of one call, for every shape of the issue (the last one: the second pass of the write kernel's capped
    grid, with C = 2 and L = 1) and the three kinds of image: uniform, mean = 10^5 spreads (where a one-pass variance is weakest),
    and means that differ by 1000 x between the images of the batch."""
    B, H, W, pad = shape
    C_, L = (2, 1) if shape == PR.PREP_BIG else (7, 14)
    slabs, (img, labels, lands, view) = prep_slabs(B, H, W, pad, C_, L, kind, start=7 if shape == PR.PREP_BIG else 0)
    rc, got = twice('dfl_prep_batch', prep_args(B, H, W, pad, C_, L, 2.5, 1), slabs, ALL)
    ok('dfl_prep_batch', rc)
    what = 'prep %s %s' % (shape_id(shape), kind)
    check_x(got['x'], img, pad, what)
    check_masks(got['masks'], labels, C_, what)
    check_heats(got['heats'], lands, view, H, W, 2.5, what)
    if C_ == 7:
        assert (labels >= 7).any() or H * W < 8          # labels 200 and 255 are in the map: zeros in every channel (check_masks)


@pytest.mark.parametrize('shape', PR.PREP_SHAPES, ids=shape_id)
def test_prep_batch_without_standardisation_is_the_reflect_padded_input(shape):
    B, H, W, pad = shape
    slabs, (img, labels, lands, view) = prep_slabs(B, H, W, pad, 2, 1)
    del slabs['scratch']                                 # scratch may be NULL when nothing is standardised
    rc, got = twice('dfl_prep_batch', prep_args(B, H, W, pad, 2, 1, 2.5, 0), slabs, ALL)
    ok('dfl_prep_batch', rc)
    want = np.stack([PR.reflect_pad(img[b], pad) for b in range(B)])
    assert got['x'].tobytes() == want.tobytes()
    check_masks(got['masks'], labels, 2, 'prep unstandardised')


@pytest.mark.parametrize('C_', [1, 7, 31])
def test_prep_batch_masks_channel_counts(C_):
    B, H, W, pad = 3, 20, 31, 0
    slabs, (img, labels, lands, view) = prep_slabs(B, H, W, pad, C_, 1)
    if C_ == 1:
        labels[:, ::2] = 3                                # labels >= C with a single channel
        slabs['labels'] = (Slab(np.uint8, data=labels), False)
    rc, got = twice('dfl_prep_batch', prep_args(B, H, W, pad, C_, 1, 2.5, 1), slabs, ALL)
    ok('dfl_prep_batch', rc)
    check_masks(got['masks'], labels, C_, 'prep C=%d' % C_)
    assert got['masks'].sum() == int((labels < C_).sum())


@pytest.mark.parametrize('sigma', [2.5, 1.0])
@pytest.mark.parametrize('L', [1, 14])
@pytest.mark.parametrize('shape', PR.PREP_SHAPES[:3], ids=shape_id)
def test_prep_batch_heats(shape, L, sigma):
    """Every landmark form of prep_ref.land_entries (L = 14), and one form per image (L = 1: on the boundary, one step outside, NaN)."""
    B, H, W, pad = shape
    slabs, (img, labels, lands, view) = prep_slabs(B, H, W, pad, 2, L)
    rc, got = twice('dfl_prep_batch', prep_args(B, H, W, pad, 2, L, sigma, 1), slabs, ALL)
    ok('dfl_prep_batch', rc)
    check_heats(got['heats'], lands, view, H, W, sigma, 'heats %s L=%d sigma=%g' % (shape_id(shape), L, sigma))


@pytest.mark.parametrize('null', [('x',), ('masks',), ('heats',), ('x', 'masks'), ('x', 'heats'), ('masks', 'heats'), ('x', 'scratch')],
                         ids='+'.join)
def test_prep_batch_null_outputs(null):
    """What is asked for is what the full call gives, bit for bit, and nothing else is written: the buffers of the NULL outputs are
    allocated but not passed, and must keep their sentinels."""
    B, H, W, pad, C_, L = 2, 37, 53, 36, 7, 14
    slabs, _ = prep_slabs(B, H, W, pad, C_, L)
    rc, full = twice('dfl_prep_batch', prep_args(B, H, W, pad, C_, L, 2.5, 1), slabs, ALL)
    ok('dfl_prep_batch', rc)
    part = {k: (s, w and k not in null and not (k == 'scratch' and 'x' in null)) for k, (s, w) in slabs.items()}
    rc, got = twice('dfl_prep_batch', prep_args(B, H, W, pad, C_, L, 2.5, 1), part, {k: v for k, v in ALL.items() if k not in null})
    ok('dfl_prep_batch', rc)
    for k in ('x', 'masks', 'heats'):
        if k not in null:
            assert got[k].tobytes() == full[k].tobytes(), k


PREP_REFUSALS = {
    'B=0': dict(B=0), 'B<0': dict(B=-1), 'H=0': dict(H=0), 'H<0': dict(H=-20), 'W=0': dict(W=0), 'W<0': dict(W=-31),
    'pad<0': dict(pad=-1), 'pad=H': dict(pad=20), 'pad=W': dict(H=31, W=20, pad=20),
    'x without proj': dict(null=('proj',)), 'masks without labels': dict(null=('labels',)), 'masks with C=0': dict(C=0),
    'heats without lands': dict(null=('lands',)), 'heats with L=0': dict(L=0), 'heats with sigma=0': dict(sigma=0.0),
    'standardize without scratch': dict(null=('scratch',)),
}


@pytest.mark.parametrize('case', list(PREP_REFUSALS))
def test_prep_batch_refusals(case):
    B, H, W, pad, C_, L = 2, 20, 31, 3, 7, 14
    slabs, _ = prep_slabs(B, H, W, pad, C_, L)
    args = prep_args(B, H, W, pad, C_, L, 2.5, 1)
    change = dict(PREP_REFUSALS[case])
    null = change.pop('null', ())
    for k, v in change.items():
        setattr(args, k, v)
    rc, _ = twice('dfl_prep_batch', args, slabs, {k: v for k, v in ALL.items() if k not in null})   # fetch(): no byte of any buffer changed
    assert rc != 0, '%s was accepted' % case


def test_prep_batch_accepts_the_neighbours_of_its_refusals():
    """pad = H - 1 and pad = W - 1 (the largest reflect) are accepted: the refusals above are not a wider net than the contract's."""
    for (H, W, pad) in [(20, 31, 19), (31, 20, 19)]:
        slabs, (img, _, _, _) = prep_slabs(2, H, W, pad, 7, 14)
        rc, got = twice('dfl_prep_batch', prep_args(2, H, W, pad, 7, 14, 2.5, 1), slabs, ALL)
        ok('dfl_prep_batch', rc)
        check_x(got['x'], img, pad, 'prep %dx%d pad %d' % (H, W, pad))


# ==================================================================================================== dfl_est_lands
def est_call(heats, segs=None, lab=None, sigma=PR.EST_SIGMA, min_ncc=PR.EST_MIN_NCC, with_ncc=True, shift=0, **change):
    """-> (return code, rowcol [B][L][2], ncc [B][L] or None).  The rowcol slots hold 0xA5 bytes before the call: the entry's own
    memset must be what clears the meeting point of the arg-max pass."""
    B, L, H, W = heats.shape
    slabs = {'heats': (Slab(np.float32, data=heats), False), 'rowcol': (Slab(np.int32, (B, L, 2), shift=shift), True)}
    fields = {'heats': 'heats', 'rowcol': 'rowcol'}
    if with_ncc:
        slabs['ncc'], fields['ncc'] = (Slab(np.float32, (B, L)), True), 'ncc'
    if segs is not None:
        slabs['segs'], fields['segs'] = (Slab(np.uint8, data=segs), False), 'segs'
    if lab is not None:
        slabs['lab'], fields['lab'] = (Slab(np.int32, data=lab), False), 'label_for_land'
    args = nat.EstLandsArgs(B=B, L=L, H=H, W=W, sigma=sigma, min_ncc=min_ncc)
    null = change.pop('null', ())
    for k, v in change.items():
        setattr(args, k, v)
    rc, got = twice('dfl_est_lands', args, slabs, {k: v for k, v in fields.items() if k not in null})
    return rc, got['rowcol'], got.get('ncc')


def check_ncc(got, ref, amp_y, amp_t, what):
    """The kernel's correlation (float32 values, centring and products; float64 sums) against the float64 model.  With Y = max|y|,
    T = max|t| over the window and the template, N = 625:
      centred values.  my' = fl32(mean) is off by u Y at most and the subtraction rounds once (<= 2 u Y), so yz' = yz + a with
        |a| <= 3 u Y.  The template is itself computed in float32, t' = t (1 + tau) with |tau| <= (8 |e| + 8) u as for the heat maps,
        and (8 |e| + 8) exp(-|e|) <= 8, so |t' - t| <= 8 u T (its mean moves by less than a tenth of that: sum t ~ 1 = 625 mean);
        with the 3 u T of the centring, tz' = tz + b with |b| <= 12 u T.
      the product sum.  sum (tz + b)(yz + a)(1 + delta): |sum tz a| <= 3 u Y sum|tz| <= 3 u Y sqrt(N) |tz|_2 <= 3 u Y N sd_t, likewise
        |sum b yz| <= 12 u T N sd_y, and |sum delta tz yz| <= u |tz|_2 |yz|_2 <= u N sd_t sd_y.  Over N sd_t sd_y:
        3 u Y / sd_y + 12 u T / sd_t + u.
      the deviations.  syy' = syy (1 + 2 * 3 u Y sqrt(N) / |yz|_2 + u), so sd_y' = sd_y (1 + 3 u Y / sd_y + 2.5 u) with the cast and
        the square root; sd_t' = sd_t (1 + 12 u T / sd_t + 2.5 u).
      the quotient.  five float32 roundings (cast, two products, sum, division); the 1e-8 is far below N sd_t sd_y in these cases.
      With |ncc| <= 1:  |ncc' - ncc| <= u (1 + 5 + 5 + 2 (3 Y / sd_y + 12 T / sd_t)) = u (11 + 6 Y / sd_y + 24 T / sd_t).
    (Printed beside it, not asserted: the error over u (8 + 8 (Y / sd_y + T / sd_t)), the form that charges the template 3 u T like
    the window, i.e. takes its float32 exponential as exact.)"""
    print('RATIO ncc-template-exact %.4f  (%s)' % (float((np.abs(got.astype(np.float64) - ref) / (U * (8.0 + 8.0 * (amp_y + amp_t)))).max()), what))
    ratio('ncc',np.abs(got.astype(np.float64) - ref), U * (11.0 + 6.0 * amp_y + 24.0 * amp_t), what)


@pytest.mark.parametrize('H,W', PR.EST_SHAPES, ids=lambda v: str(v))
def test_est_lands_peaks(H, W):
    """Peaks at the corners, where the window first and last touches the border, near the border, between pixels, and noise alone;
    13 x 13 .. 64 x 80 leave workgroups of the scan without a pixel, 150 x 200 fills the unroll partly, 300 x 440 (L = 3) makes the
    second outer trip."""
    heats, names = PR.peak_case(H, W, L=3 if (H, W) == PR.EST_SHAPES[-1] else None)
    want, ncc, amp_y, amp_t = PR.est_lands(heats, min_ncc=PR.EST_MIN_NCC)
    rc, rowcol, got = est_call(heats)
    ok('dfl_est_lands', rc)
    assert np.array_equal(rowcol, want), [(names[b][l], rowcol[b, l].tolist(), want[b, l].tolist())
                                          for b in range(2) for l in range(len(names[b])) if not np.array_equal(rowcol[b, l], want[b, l])]
    check_ncc(got, ncc, amp_y, amp_t, 'ncc %dx%d' % (H, W))
    rc, rowcol2, none = est_call(heats, with_ncc=False)          # ncc = NULL is accepted and changes nothing
    ok('dfl_est_lands', rc)
    assert none is None and np.array_equal(rowcol2, rowcol)
    rc, free, _ = est_call(heats, min_ncc=-2.0)                  # the locations themselves
    ok('dfl_est_lands', rc)
    assert np.array_equal(free, PR.est_lands(heats, min_ncc=-2.0)[0]) and free.min() >= 0


@pytest.mark.parametrize('H,W', [(13, 13), (64, 80), (150, 200)], ids=lambda v: str(v))
def test_est_lands_constant_map(H, W):
    """All pixels tie: index 0.  625 equal float32 values sum exactly in float64 and their mean is the value itself, so every
    centred value, the product sum and the correlation are 0.0 exactly: rejected for any min_ncc > 0, accepted for -2."""
    heats = np.full((2, 2, H, W), np.float32(0.3))
    heats[1, 1] = np.float32(-1.7)
    for min_ncc, want in ((0.9, -1), (1e-30, -1), (-2.0, 0)):
        rc, rowcol, ncc = est_call(heats, min_ncc=min_ncc)
        ok('dfl_est_lands', rc)
        assert (rowcol == want).all() and ncc.tobytes() == np.zeros((2, 2), np.float32).tobytes(), (min_ncc, rowcol.tolist(), ncc.tolist())


@pytest.mark.parametrize('H,W', [(64, 80), (150, 200), (300, 440)], ids=lambda v: str(v))
def test_est_lands_argmax_placement(H, W):
    """min_ncc = -2: only the location is at stake.  Unique maxima on both sides of every boundary of the scan's index space, equal
    maxima in two workgroups, two unroll slots of one thread and two outer trips (the lower index wins), an all-negative map, a
    zero maximum of either sign at the lower index, positive subnormals."""
    heats, want = PR.argmax_case(H, W)
    model = PR.est_lands(heats, min_ncc=-2.0)[0]
    rc, rowcol, ncc = est_call(heats, min_ncc=-2.0)
    ok('dfl_est_lands', rc)
    for b in range(2):
        for l, (name, k) in enumerate(want[b]):
            assert model[b, l].tolist() == [k // W, k % W], name
            assert rowcol[b, l].tolist() == [k // W, k % W], '%s (image %d): got flat index %d, want %d' % (
                name, b, int(rowcol[b, l, 0]) * W + int(rowcol[b, l, 1]), k)
    assert np.isfinite(ncc).all()


def test_est_lands_masked():
    H, W = 64, 80
    heats, segs, lab = PR.masked_case(H, W)
    plain = PR.est_lands(heats, min_ncc=-2.0)[0]
    for min_ncc in (PR.EST_MIN_NCC, -2.0):
        want, ncc, amp_y, amp_t = PR.est_lands(heats, segs, lab, min_ncc=min_ncc)
        rc, rowcol, got = est_call(heats, segs, lab, min_ncc=min_ncc)
        ok('dfl_est_lands', rc)
        assert np.array_equal(rowcol, want), (rowcol.tolist(), want.tolist())
        found = np.isfinite(amp_y) & (amp_y > 0)
        check_ncc(got[found], ncc[found], amp_y[found], amp_t[found], 'ncc masked')
        assert not got[~found].any()                              # nothing eligible: ncc = 0
    l5, l9, l4 = (list(lab).index(v) for v in (5, 9, 4))
    assert rowcol[1, l5].tolist() == [-1, -1] and rowcol[0, l5].min() >= 0 and got[1, l5] == 0.0     # a label of image 0 only
    assert rowcol[:, l9].max() == -1 and rowcol[:, l4].tolist() == [[H - 1, W - 1]] * 2              # absent; one pixel at H*W-1
    assert np.array_equal(rowcol[:, lab < 0], plain[:, lab < 0])
    for kw in (dict(segs=segs), dict(lab=lab)):                   # segs without label_for_land and the reverse: unmasked
        rc, rowcol, _ = est_call(heats, min_ncc=-2.0, **kw)
        ok('dfl_est_lands', rc)
        assert np.array_equal(rowcol, plain)


EST_REFUSALS = {'H=12': dict(H=12), 'W=12': dict(W=12), 'sigma=0': dict(sigma=0.0), 'B=0': dict(B=0), 'L=0': dict(L=0),
                'heats NULL': dict(null=('heats',)), 'rowcol NULL': dict(null=('rowcol',)), 'rowcol + 4 bytes': dict(shift=4)}


@pytest.mark.parametrize('case', list(EST_REFUSALS))
def test_est_lands_refusals(case):
    heats, segs, lab = PR.masked_case(13, 40)
    rc, rowcol, ncc = est_call(heats, segs, lab, **EST_REFUSALS[case])       # fetch(): no byte of any buffer changed
    assert rc != 0, '%s was accepted' % case
    assert (rowcol.view(np.uint8) == 0xA5).all()


# ==================================================================================================== dfl_hard_dice
DICE_RUNS = ([(p, 1, 2, 'random') for p in PR.DICE_PIXELS] + [(p, 3, 7, 'random') for p in PR.DICE_PIXELS] +
             [(p, 1, 256, 'random') for p in PR.DICE_PIXELS[2:]] + [(257, 3, 7, 'foreign'), (70 * 90, 1, 7, 'foreign'),
             (PR.DICE_PIXELS[-1], 1, 7, 'foreign'), (70 * 90, 3, 7, 'special'), (70 * 90, 3, 256, 'random')])


def dice_call(est, gt, B, C_, pixels, null=()):
    slabs = {'est': (Slab(np.uint8, data=est), False), 'gt': (Slab(np.uint8, data=gt), False),
             'counts': (Slab(np.int64, (B, max(C_, 1), 3)), True), 'dice': (Slab(np.float64, (B, max(C_ - 1, 1))), True)}
    out = None
    for rep in range(2):
        p = {k: (s.upload() if k not in null else None) for k, (s, _) in slabs.items()}
        rc = nat.lib().dfl_hard_dice(p['est'], p['gt'], pixels, B, C_, p['counts'], p['dice'], stream())
        torch.cuda.synchronize()
        got = {k: s.fetch('dfl_hard_dice ' + k, w and rc == 0) for k, (s, w) in slabs.items() if k not in null}
        if out is not None:
            assert rc == out[0] and all(got[k].tobytes() == out[1][k].tobytes() for k in got)
        out = (rc, got)
    return out


@pytest.mark.parametrize('pixels,B,C_,kind', DICE_RUNS, ids=['%d-B%d-C%d-%s' % r for r in DICE_RUNS])
def test_hard_dice_counts_and_dice_equal_the_model(pixels, B, C_, kind):
    """counts and dice hold garbage (0xA5 bytes, NaN) before the call: the entry's memset and the final kernel write every slot."""
    est, gt = PR.dice_case(pixels, B, C_, kind)
    counts, dice = PR.dice_counts(est, gt, C_)
    rc, got = dice_call(est, gt, B, C_, pixels)
    ok('dfl_hard_dice', rc)
    assert got['counts'].tolist() == counts
    assert got['dice'].tobytes() == np.array(dice, np.float64).tobytes(), (got['dice'].tolist(), dice)
    for b in range(B):
        assert int(got['counts'][b, :, 0].sum()) == int((est[b] < C_).sum()) and int(got['counts'][b, :, 1].sum()) == int((gt[b] < C_).sum())
    if kind == 'special':
        assert got['dice'][0, 0] == 1.0 and got['dice'][0, 1] == 0.0 and (got['dice'][B - 1] == 1.0).all()
    if kind == 'foreign':
        assert int(got['counts'][0, :, 0].sum()) < pixels
    if C_ == 256 and pixels >= 512:
        assert (got['counts'][0, :, :2] > 0).all()                # all 768 counters are live


@pytest.mark.parametrize('case', ['C=1', 'C=257', 'B=0', 'pixels=0', 'est NULL', 'gt NULL', 'counts NULL', 'dice NULL'])
def test_hard_dice_refusals(case):
    pixels, B, C_ = 257, 3, 7
    est, gt = PR.dice_case(pixels, B, C_)
    null = (case.split()[0],) if case.endswith('NULL') else ()
    if case.startswith('C='):
        C_ = int(case[2:])
    rc, got = dice_call(est, gt, 0 if case == 'B=0' else B, C_, 0 if case == 'pixels=0' else pixels, null)   # fetch(): nothing changed
    assert rc != 0, '%s was accepted' % case
