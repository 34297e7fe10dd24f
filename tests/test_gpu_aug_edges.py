"""The kernels of csrc/augment.hip (and aug_normal of csrc/philox.h) through the C ABI -- dfl_augment_batch called with
dfl_augment_args / dfl_augment_item built here -- against the numpy restatement tests/aug_ref.py over the case table of
tests/test_aug_edges_cpu.py: PIL's border rules, reflection beyond one period, non-finite maps, every flag combination,
landmark boundaries, erase boxes of every form, the optional arguments, what the entry point refuses, and the 64-bit key.

augment.hip is built with -ffp-contract=off and the restatement repeats its arithmetic operation by operation, so with the
model fed the device's own normals everything is held bit for bit, except where libm enters: the Box-Muller normals, powf of
the gamma step and expf of the heat maps, each with a bar stated where it is applied.  The 18 doubles of the three maps are
packed as the model reads them: the host's matrix construction is not part of the comparison.

Every device buffer is filled with a sentinel byte and fenced by guard bytes that must survive; the scratch is exactly
dfl_augment_scratch_bytes long; every call is made twice on fresh buffers and must return the same bytes."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from dfl_amd import _native as nat
import aug_ref as A
import test_aug_edges_cpu as T

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD, SENT = 256, 0xA5
OUTPUTS = ('x', 'masks', 'heats', 'lands_out', 'levels', 'noise', 'scratch')
OPTIONAL = ('labels', 'lands', 'masks', 'heats', 'lands_out', 'levels', 'noise')
RULES = {None: nat.AUG_LANDS_NONE, 'reference': nat.AUG_LANDS_REFERENCE, 'in_view': nat.AUG_LANDS_IN_VIEW}
WORST = {}


def note(kind, value, what):
    WORST[kind] = max(WORST.get(kind, 0.0), float(value))
    print('WORST %s %.4g  (%s; largest so far %.4g)' % (kind, value, what, WORST[kind]))


class Buf:
    """A payload of nbytes inside a device allocation of sentinel bytes, GUARD of them on either side."""

    def __init__(self, nbytes, data=None):
        self.n = int(nbytes)
        self.host = np.full(self.n + 2 * GUARD, SENT, np.uint8)
        if data is not None:
            self.host[GUARD:GUARD + self.n] = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        self.dev = torch.from_numpy(self.host.copy()).to(DEV)
        self.ptr = self.dev.data_ptr() + GUARD

    def fetch(self, what):
        after = self.dev.cpu().numpy()
        assert np.array_equal(after[:GUARD], self.host[:GUARD]) and np.array_equal(after[-GUARD:], self.host[-GUARD:]), \
            'guard bytes of %s were written' % what
        return after[GUARD:GUARD + self.n].copy()


def pack_item(prm, row, maps, n_box=None):
    """The dfl_augment_item of a parameter dict with explicit maps; nothing is validated (the kernel's rules are under test)."""
    it = nat.AugmentItem()
    for field, m in zip(('img_map', 'seg_map', 'land_map'), maps):
        getattr(it, field)[:] = [float(v) for v in m]
    it.noise_key = prm['noise_key']
    for b, (r0, c0, nr, nc, key) in enumerate(prm['boxes'][:5]):
        it.box[b][:] = (r0, c0, nr, nc)
        it.box_key[b] = key
    it.n_box = len(prm['boxes']) if n_box is None else n_box
    it.noise_sigma, it.gamma = prm['sigma'], prm['gamma']
    it.row, it.flags = row, prm['flags']
    return it


def call(proj, items, pad, labels=None, lands=None, C_=0, standardize=0, rule='reference', sigma=2.5, use=OPTIONAL,
         n_items=None, mutate=None, expect=0):
    """dfl_augment_batch on fenced buffers, two times over.  proj [B,H,W]; labels [B,H,W] / lands [B,2,L] or None; items: a
    list of dfl_augment_item.  use: which optional pointers are passed (every buffer is allocated either way).  mutate(args,
    bufs) changes the arguments just before the call.  -> {name: payload after the call}, inputs included."""
    B, H, W = proj.shape
    L = lands.shape[2] if lands is not None else 1
    Cn = max(C_, 1)
    Ho, Wo = H + 2 * pad, W + 2 * pad
    n = len(items)
    table = (nat.AugmentItem * max(n, 1))(*items)
    need = int(nat.lib().dfl_augment_scratch_bytes(max(n, 1), H, W, pad))
    assert need > 0
    shapes = {'x': (np.float32, (B, Ho, Wo)), 'masks': (np.float32, (B, Cn, H, W)), 'heats': (np.float32, (B, L, H, W)),
              'lands_out': (np.float32, (B, 2, L)), 'levels': (np.uint8, (max(n, 1), Ho, Wo)), 'noise': (np.float32, (max(n, 1), H, W)),
              'scratch': (np.uint8, (need,))}
    inputs = {'proj': proj, 'items': np.frombuffer(bytearray(table), np.uint8)}
    if labels is not None:
        inputs['labels'] = labels
    if lands is not None:
        inputs['lands'] = lands
    first = None
    for rep in range(2):
        bufs = {k: Buf(np.asarray(v).nbytes, v) for k, v in inputs.items()}
        bufs.update({k: Buf(np.dtype(dt).itemsize * int(np.prod(sh))) for k, (dt, sh) in shapes.items()})
        assert bufs['scratch'].ptr % 256 == 0
        a = nat.AugmentArgs(proj=bufs['proj'].ptr, x=bufs['x'].ptr, items=bufs['items'].ptr, scratch=bufs['scratch'].ptr,
                            n_items=n if n_items is None else n_items, B=B, H=H, W=W, pad=pad, C=C_, L=L if lands is not None else 0,
                            sigma=sigma, standardize=standardize, land_rule=RULES[rule])
        for k in OPTIONAL:
            if k in use and k in bufs:
                setattr(a, k, bufs[k].ptr)
        if mutate is not None:
            mutate(a, bufs)
        rc = nat.lib().dfl_augment_batch(C.addressof(a), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == expect, 'dfl_augment_batch returned %d, expected %d: %s' % (rc, expect, nat.lib().dfl_last_error().decode())
        got = {k: b.fetch(k) for k, b in bufs.items()}
        for k in inputs:
            assert np.array_equal(got[k], bufs[k].host[GUARD:GUARD + bufs[k].n]), 'input %s was written' % k
        if first is not None:
            for k in got:
                assert got[k].tobytes() == first[k].tobytes(), '%s differs between two calls on the same inputs' % k
        first = got
    out = {k: first[k].view(dt).reshape(sh) for k, (dt, sh) in shapes.items()}
    out['bytes'] = first
    return out


def untouched(a):
    return bool((np.asarray(a).reshape(-1).view(np.uint8) == SENT).all())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want, what):
    g, w = bits(got), bits(want)
    bad = np.argwhere(g != w)
    assert not len(bad), '%s: %d of %d values differ in their bits, first at %s: %r, model %r' % (
        what, len(bad), g.size, bad[0].tolist(), np.asarray(got)[tuple(bad[0])], np.asarray(want)[tuple(bad[0])])


# ---- the device's normals -------------------------------------------------------------------------------------------------
_NORMALS = {}


def device_normals(key, idx):
    """aug_normal(key, i) of the device for the indices idx: the noise plane of a one-item call with only the noise flag
    on a dummy image of enough pixels.  The normals_fn of the model, for the noise plane and the erase boxes."""
    idx = np.asarray(idx, dtype=np.int64)
    n = int(idx.max()) + 1
    have = _NORMALS.get(key)
    if have is None or have.size < n:
        W = 64
        H = max(-(-n // W), 2)
        proj = np.linspace(0.0, 1.0, H * W, dtype=np.float32).reshape(1, H, W)
        prm = dict(flags=A.NOISE, sigma=0.01, gamma=1.0, noise_key=key, boxes=[])
        o = call(proj, [pack_item(prm, 0, A.maps(H, W, 0, T.IDENT, False))], 0, use=('noise',), rule=None)
        have = _NORMALS[key] = o['noise'].reshape(-1)
    return have[idx]


@pytest.mark.parametrize('key', [0, 1, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1], ids=hex)
def test_device_normals_match_the_philox_restatement(key):
    n = 45 * 61
    z = device_normals(key, np.arange(n))
    want = A.normals(key, np.arange(n))
    err = float(np.abs(z.astype(np.float64) - want.astype(np.float64)).max())
    note('normal', err, 'key %#x' % key)
    assert np.isfinite(z).all()
    assert err <= 1e-5                  # the bar of test_gpu_augment.py::test_noise_field_matches_philox_restatement


def test_both_words_of_the_key_reach_the_generator():
    idx = np.arange(256)
    base = 0x0123456789abcdef
    planes = {k: device_normals(k, idx).tobytes() for k in (base, base ^ (1 << 40), base ^ (1 << 63), base ^ 1, base ^ (1 << 31))}
    assert len(set(planes.values())) == 5                   # a change in the high word alone, or in the low word alone, shows
    for k in planes:                                        # and each is the restatement's plane for that very key
        assert np.abs(np.frombuffer(planes[k], np.float32) - A.normals(k, idx)).max() <= 1e-5     # the bar above


# ---- one case against the model ---------------------------------------------------------------------------------------------
def batch_of(cases, rows, B):
    """Inputs of a batch whose row rows[k] holds case k (same shape, C and L); the other rows hold other random data."""
    c0 = cases[0]
    H, W, L = c0['H'], c0['W'], c0['L']
    rng = np.random.default_rng(B * 1000 + sum(rows))
    proj = rng.random((B, H, W), dtype=np.float32) * 7 - 3
    labels = rng.integers(0, c0['C'], (B, H, W)).astype(np.uint8)
    lands = rng.uniform(0, H, (B, 2, L)).astype(np.float32)
    built = []
    for c, r in zip(cases, rows):
        b = T.build(c)
        proj[r], labels[r], lands[r] = b['proj'], b['seg'], b['lands']
        built.append(b)
    return proj, labels, lands, built


def items_of(cases, built, rows, has_seg=True):
    return [pack_item(b['prm'], r, A.case_maps(c['H'], c['W'], c['pad'], b['prm'], has_seg)) for c, b, r in zip(cases, built, rows)]


def check_heats(got, lands_out, H, W, what, sigma=2.5):
    """expf against the float64 exp of the same fp32 argument, times knorm."""
    arg, knorm, finite = A.heat_arguments(lands_out, H, W, sigma)
    want = np.exp(arg.astype(np.float64)) * float(knorm)
    for l in range(arg.shape[0]):
        if not finite[l]:
            assert not got[l].any(), '%s: the heat map of non-finite landmark %d is not zero' % (what, l)
    f = np.nonzero(finite)[0]
    if len(f):
        err = np.abs(got[f].astype(np.float64) - want[f])
        # rtol 2^-21: expf within an ulp or so and one fp32 product; atol 2^-126: a result below the smallest normal may be flushed
        bound = 2.0 ** -21 * want[f] + 2.0 ** -126
        note('heat', float((err / bound).max()), what + ' (error / bound)')
        assert (err <= bound).all(), '%s: %d heat values off, worst error / bound %.3f' % (what, int((err > bound).sum()), float((err / bound).max()))


def check_standardised(x_std, x_raw, what):
    """(raw - mean) * inv with the float64 mean and unbiased variance of the device's own raw image."""
    v = x_raw.astype(np.float64).reshape(-1)
    mean = math.fsum(v) / v.size
    var = math.fsum((v - mean) ** 2) / (v.size - 1)
    with np.errstate(divide='ignore', invalid='ignore'):
        inv = np.float64(1.0) / np.sqrt(np.float64(var))
        want = (x_raw.astype(np.float64) - mean) * inv
    if var == 0.0:
        assert np.isnan(x_std).all() and np.isnan(want).all(), '%s: a constant image standardises to NaN' % what
        return
    # 4 * 2^-24 (|mean| inv + |x|): the mean rounded to fp32, the subtraction, inv rounded to fp32 and the product
    bound = 4.0 * 2.0 ** -24 * (abs(mean) * inv + np.abs(want))
    err = np.abs(x_std.astype(np.float64) - want)
    note('standardise', float((err / bound).max()), what + ' (error / bound)')
    assert (err <= bound).all(), '%s: %d standardised values off, worst error / bound %.3f' % (what, int((err > bound).sum()), float((err / bound).max()))


def check_item(o, k, row, c, b, m, what, use=OPTIONAL, labels=True):
    """Outputs of item k (batch row `row`) of a raw (standardize = 0) call against the model m of case c."""
    H, W, pad, C_ = c['H'], c['W'], c['pad'], c['C']
    gamma = bool(c['flags'] & A.GAMMA)
    exact = True
    if 'levels' in use:
        lev = o['levels'][k]
        if not gamma:
            bad = np.argwhere(lev != m['levels'])
            assert not len(bad), '%s: %d levels differ, first at %s: %d, model %d' % (
                what, len(bad), bad[0].tolist(), lev[tuple(bad[0])], m['levels'][tuple(bad[0])])
        else:
            # a level may differ by one, and only where a tap lies in the gamma window (aug_ref.gamma_window: two powf within
            # an ulp or so of the truth differ by 2^-23 in p, which four roundings carry to the 8-bit truncation)
            window, _ = A.gamma_window(b['proj'], b['prm'], pad, device_normals)
            diff = np.abs(lev.astype(np.int32) - m['levels'].astype(np.int32))
            print('GAMMA %s: %d of %d levels differ (%d output pixels have a tap in the window)' % (what, int((diff != 0).sum()), diff.size, int(window.sum())))
            assert diff.max() <= 1, '%s: a level differs by %d' % (what, int(diff.max()))
            assert not (diff != 0)[~window].any(), '%s: %d levels differ outside the gamma window' % (what, int((diff != 0)[~window].sum()))
            exact = not diff.any()
    else:
        assert untouched(o['levels'])
    if c['flags'] & A.NOISE and 'noise' in use:
        same_bits(o['noise'][k], m['noise'], what + ' noise')
    else:
        assert untouched(o['noise'][k]), '%s: the noise plane of an item without the flag (or without the pointer) was written' % what
    if exact:
        same_bits(o['x'][row], m['raw'], what + ' raw x')
    else:
        # a differing level: the pixels with the model's level, outside every erase box (a box's sigma sees its levels)
        keep = o['levels'][k] == m['levels']
        for (r0, c0, nr, nc, _) in A.erase_boxes(b['prm'], H + 2 * pad, W + 2 * pad) if c['flags'] & A.ERASE else []:
            keep[r0:r0 + nr, c0:c0 + nc] = False
        same_bits(o['x'][row][keep], m['raw'][keep], what + ' raw x at the model\'s levels outside the boxes')
    if labels and 'masks' in use:
        assert o['masks'][row].tobytes() == m['masks'].tobytes(), '%s: %d mask values differ' % (what, int((o['masks'][row] != m['masks']).sum()))
    else:
        assert untouched(o['masks'][row])
    if 'lands' in use and 'lands_out' in use:
        same_bits(o['lands_out'][row], m['lands'], what + ' lands_out')         # NaN and inf by their bits
        if 'heats' in use:
            check_heats(o['heats'][row], o['lands_out'][row], H, W, what)
        else:
            assert untouched(o['heats'][row])
    else:
        assert untouched(o['lands_out'][row]) and untouched(o['heats'][row])


def check_other_rows(o, rows, what):
    for k in ('x', 'masks', 'heats', 'lands_out'):
        for r in range(o[k].shape[0]):
            if r not in rows:
                assert untouched(o[k][r]), '%s: row %d of %s is not in items and was written' % (what, r, k)


@pytest.mark.parametrize('name', [c['name'] for c in T.CASES])
def test_case_matches_the_model(name):
    """Row 1 of a batch of 3: levels, raw x, masks, landmarks, heat maps, then the standardised x; rows 0 and 2 keep every byte."""
    c = T.BY_NAME[name]
    proj, labels, lands, (b,) = batch_of([c], [1], 3)
    items = items_of([c], [b], [1])
    m = T.model(name, normals_fn=device_normals)
    raw = call(proj, items, c['pad'], labels, lands, c['C'], standardize=0)
    check_item(raw, 0, 1, c, b, m, name)
    check_other_rows(raw, [1], name)
    std = call(proj, items, c['pad'], labels, lands, c['C'], standardize=1)
    check_standardised(std['x'][1], raw['x'][1], name)
    for k in ('masks', 'heats', 'lands_out', 'levels', 'noise'):
        assert std['bytes'][k].tobytes() == raw['bytes'][k].tobytes(), k
    check_other_rows(std, [1], name)


# ---- batches --------------------------------------------------------------------------------------------------------------
TRIO = ['16x16_p0_half', '16x16_p0_zoom4', '16x16_p0_inf_map']       # flags 2, 1, 8; one shape, C and L


def test_items_in_scrambled_row_order_are_independent():
    cases, rows = [T.BY_NAME[n] for n in TRIO], [5, 0, 3]
    proj, labels, lands, built = batch_of(cases, rows, 6)
    o = call(proj, items_of(cases, built, rows), 0, labels, lands, 3)
    for k, (c, b, r) in enumerate(zip(cases, built, rows)):
        check_item(o, k, r, c, b, T.model(c['name'], normals_fn=device_normals), 'batch item %d (%s)' % (k, c['name']))
    check_other_rows(o, rows, 'batch')
    for k, (c, b, r) in enumerate(zip(cases, built, rows)):
        alone = call(proj[r:r + 1], items_of([c], [b], [0]), 0, labels[r:r + 1], lands[r:r + 1], 3)
        for key in ('x', 'masks', 'heats', 'lands_out'):
            assert alone[key][0].tobytes() == o[key][r].tobytes(), (c['name'], key)
        assert alone['levels'][0].tobytes() == o['levels'][k].tobytes() and alone['noise'][0].tobytes() == o['noise'][k].tobytes()


def test_items_whose_row_is_outside_the_batch_are_skipped():
    cases = [T.BY_NAME[n] for n in TRIO]
    proj, labels, lands, built = batch_of(cases, [0, 1, 2], 3)
    o = call(proj, items_of(cases, built, [-1, 1, 3]), 0, labels, lands, 3)
    check_item(o, 1, 1, cases[1], built[1], T.model(TRIO[1], normals_fn=device_normals), 'between two skipped items')
    check_other_rows(o, [1], 'skipped items')
    assert untouched(o['levels'][0]) and untouched(o['levels'][2]) and untouched(o['noise'][0]) and untouched(o['noise'][2])
    o = call(proj, items_of(cases, built, [-1, 3, -(1 << 31)]), 0, labels, lands, 3, standardize=1)
    for k in ('x', 'masks', 'heats', 'lands_out', 'levels', 'noise'):
        assert untouched(o[k]), k


# ---- optional arguments ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('drop', [('labels', 'masks'), ('masks',), ('lands', 'heats'), ('heats',), ('levels', 'noise'), ()], ids=lambda d: '-'.join(d) or 'all')
def test_optional_pointers_as_null(drop):
    c = T.BY_NAME['16x16_p0_skew']                                      # invert + noise, L = 14
    proj, labels, lands, (b,) = batch_of([c], [1], 2)
    use = tuple(k for k in OPTIONAL if k not in drop)
    has_seg = 'labels' in use
    rule = 'reference' if has_seg else None                             # the model applies a rule to labelled items only
    m = T.model(c['name'], normals_fn=device_normals, land_rule=rule)
    o = call(proj, items_of([c], [b], [1]), 0, labels, lands, c['C'], use=use, rule=rule)
    check_item(o, 0, 1, c, b, m, 'without ' + (', '.join(drop) or 'nothing'), use=use, labels=has_seg)
    check_other_rows(o, [1], str(drop))


@pytest.mark.parametrize('rule', [None, 'reference', 'in_view'], ids=['none', 'reference', 'in_view'])
def test_land_rules_at_their_boundaries(rule):
    c = T.BY_NAME['5x7_p1_land_edges']
    proj, labels, lands, (b,) = batch_of([c], [0], 1)
    m = T.model(c['name'], normals_fn=device_normals, land_rule=rule)
    o = call(proj, items_of([c], [b], [0]), c['pad'], labels, lands, c['C'], rule=rule)
    check_item(o, 0, 0, c, b, m, 'land_rule %s' % rule)
    kept = np.isfinite(o['lands_out'][0]).all(0)
    print('kept under %s: %s' % (rule, kept.astype(int).tolist()))
    assert kept[:12].sum() == {None: 12, 'reference': 5, 'in_view': 8}[rule]       # tests/test_aug_edges_cpu.py lists which


def test_no_items_is_ok_and_writes_nothing():
    c = T.BY_NAME['5x7_p1_quarter']
    proj, labels, lands, (b,) = batch_of([c], [0], 2)
    o = call(proj, items_of([c], [b], [0]), c['pad'], labels, lands, c['C'], n_items=0, standardize=1)
    for k in OUTPUTS:
        assert untouched(o[k]), k

    def null_everything(a, bufs):
        for k in ('proj', 'x', 'items', 'scratch') + OPTIONAL:
            setattr(a, k, None)
    o = call(proj, items_of([c], [b], [0]), c['pad'], labels, lands, c['C'], n_items=0, mutate=null_everything)
    for k in OUTPUTS:
        assert untouched(o[k]), k


# ---- erase ----------------------------------------------------------------------------------------------------------------
HO, WO = 45, 61                                                        # the padded image of 37 x 53 pad 4
FIVE = [(1, 1, 5, 5, 41), (2, 2, 9, 3, 42), (30, 40, 5, 11, 43), (20, 0, 1, 61, 44), (0, 30, 45, 1, 45)]
ERASE = {
    'flag_without_boxes': ([], None),
    'five_boxes': (FIVE, None),
    'n_box_7_applies_five': (FIVE, 7),
    'second_overlaps_first': ([(5, 5, 12, 12, 1), (10, 10, 12, 12, 2)], None),
    'one_pixel': ([(7, 9, 1, 1, 3)], None),
    'one_row_and_one_column': ([(44, 0, 1, 61, 4), (0, 60, 45, 1, (1 << 64) - 1)], None),
    'below_and_above_256_pixels': ([(3, 3, 15, 17, 6), (20, 20, 16, 17, 1 << 63)], None),
    'whole_padded_image': ([(0, 0, HO, WO, 8)], None),
    'bottom_right_corner': ([(40, 50, 5, 11, 9)], None),
    'slot_1_one_column_too_wide': ([(1, 1, 5, 5, 41), (40, 50, 5, 12, 10), (20, 20, 3, 3, 11)], None),
    'slot_1_one_row_too_far': ([(1, 1, 5, 5, 41), (41, 50, 5, 11, 10), (20, 20, 3, 3, 11)], None),
    'slot_1_zero_rows': ([(1, 1, 5, 5, 41), (10, 10, 0, 4, 10), (20, 20, 3, 3, 11)], None),
    'slot_1_negative_corner': ([(1, 1, 5, 5, 41), (-1, 10, 4, 4, 10), (20, 20, 3, 3, 11)], None),
}
_ERASE_RUNS = {}


def erase_run(boxes, n_box, flags=A.ERASE):
    key = (tuple(boxes), n_box, flags)
    if key not in _ERASE_RUNS:
        c = dict(T.BY_NAME['37x53_p4_rot90'], flags=flags, boxes=list(boxes))
        proj, labels, lands, (b,) = batch_of([c], [0], 1)
        prm = b['prm']
        item = pack_item(prm, 0, A.case_maps(37, 53, 4, prm), n_box=n_box)
        o = call(proj, [item], 4, labels, lands, c['C'], use=('levels',))
        m = A.augment_item(b['proj'], b['seg'], None, prm, 4, c['C'], standardize=False, normals_fn=device_normals)
        _ERASE_RUNS[key] = (o, m)
    return _ERASE_RUNS[key]


@pytest.mark.parametrize('name', sorted(ERASE))
def test_erase_boxes(name):
    boxes, n_box = ERASE[name]
    o, m = erase_run(boxes, n_box)
    plain, _ = erase_run([], None, flags=0)
    assert np.array_equal(o['levels'][0], m['levels']) and np.array_equal(plain['levels'], o['levels'])
    same_bits(o['x'][0], m['raw'], name)
    applied = A.erase_boxes(dict(boxes=boxes), HO, WO)
    inside = np.zeros((HO, WO), bool)
    for (r0, c0, nr, nc, _) in applied:
        inside[r0:r0 + nr, c0:c0 + nc] = True
    same_bits(o['x'][0][~inside], plain['x'][0][~inside], name + ': pixels outside every applied box')
    changed = bits(o['x'][0]) != bits(plain['x'][0])
    if name == 'one_pixel':
        assert not changed.any()                                        # max - min of one pixel is 0: sigma 0, the pixel keeps its bits
    elif applied:
        assert changed[inside].mean() > 0.9, name
    if name.startswith('slot_1'):
        assert applied == boxes[:1]
        same_bits(o['x'][0], erase_run(boxes[:1], None)[0]['x'][0], name + ': box 0 alone')
    if name == 'n_box_7_applies_five':
        same_bits(o['x'][0], erase_run(FIVE, None)[0]['x'][0], name)
    if name == 'second_overlaps_first':
        # the second box's max - min includes the first's noise: it is not what the second box alone would add
        alone = erase_run(boxes[1:], None)[0]['x'][0]
        assert (bits(o['x'][0][17:22, 17:22]) != bits(alone[17:22, 17:22])).any()


# ---- refusals -------------------------------------------------------------------------------------------------------------
def _set(**kw):
    def f(a, bufs):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


def _lands_alias(a, bufs):
    a.lands_out = bufs['lands'].ptr


def _scratch_off(a, bufs):
    a.scratch = bufs['scratch'].ptr + 128


REFUSED = {
    'n_items_negative': _set(n_items=-1), 'n_items_above_B': _set(n_items=3), 'H_1': _set(H=1), 'W_1': _set(W=1), 'H_0': _set(H=0),
    'pad_negative': _set(pad=-1), 'proj_null': _set(proj=None), 'x_null': _set(x=None), 'items_null': _set(items=None),
    'scratch_null': _set(scratch=None), 'scratch_off_by_128': _scratch_off, 'masks_without_labels': _set(labels=None),
    'masks_with_C_0': _set(C=0, land_rule=0), 'masks_with_C_255': _set(C=255), 'lands_without_lands_out': _set(lands_out=None),
    'lands_with_L_0': _set(L=0), 'heats_without_lands': _set(lands=None), 'heats_with_sigma_0': _set(sigma=0.0),
    'land_rule_minus_1': _set(land_rule=-1), 'land_rule_3': _set(land_rule=3),
    'reference_rule_with_C_0': _set(C=0, masks=None, land_rule=1), 'lands_out_is_lands': _lands_alias,
    'padded_image_of_2_to_31_pixels': _set(H=46341, W=46341, pad=0),
}


@pytest.mark.parametrize('name', sorted(REFUSED))
def test_refused_arguments_launch_nothing(name):
    """One refused condition on otherwise valid arguments: ERR_INVALID_ARG and not a byte of any buffer changed."""
    c = T.BY_NAME['5x7_p1_quarter']
    proj, labels, lands, (b,) = batch_of([c], [1], 2)
    o = call(proj, items_of([c], [b], [1]), c['pad'], labels, lands, c['C'], standardize=1, mutate=REFUSED[name],
             expect=nat.ERR_INVALID_ARG)
    for k in OUTPUTS:
        assert untouched(o[k]), '%s: %s was written by a refused call' % (name, k)


def test_refusal_arguments_are_valid_before_the_change():
    c = T.BY_NAME['5x7_p1_quarter']
    proj, labels, lands, (b,) = batch_of([c], [1], 2)
    o = call(proj, items_of([c], [b], [1]), c['pad'], labels, lands, c['C'], standardize=1)
    assert not untouched(o['x'][1]) and untouched(o['x'][0])


def test_scratch_bytes_refuses_non_positive_sizes():
    f = nat.lib().dfl_augment_scratch_bytes
    assert f(1, 2, 2, 0) > 0
    for args in ((0, 4, 4, 0), (-1, 4, 4, 0), (2, 0, 4, 0), (2, -3, 4, 0), (2, 4, 0, 0), (2, 4, -1, 0)):
        assert f(*args) == -1, args
