"""dfl_ensemble_reduce (csrc/loss.hip) through its C ABI.

Reference: numpy fp32 in the kernel's order -- the nets' soft-max maps summed in net order, one division by the net count,
the first maximal class; heat maps (h - lo) / (hi - lo) with lo / hi the fp32 minimum / maximum of the net's cropped
tensor and the subtractions done in fp32, summed in net order, one division.  Every step is one IEEE add, subtract or
divide with nothing for the compiler to contract, so avg_seg, heat_out and the min/max table are expected BIT-EQUAL, and
the labels equal at every pixel (no margin mask).

Shapes: C = 7, L in {0, 3}; 1, 3, 8 nets (base pointers in registers) and 9 (the run-time loop of ens_final); a window
(7, 13) at (2, 5) of (12, 20) -- not centred, 13 % 64 != 0; (5, 515) at (1, 80) of (6, 600) -- second 512-column trip of
ens_minmax_partial, ragged; and (9, 9) of (9, 9), no crop.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from dfl_amd import _native as nat
from gpu_common import label_mask

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NC = 7
GUARD = 256
SENT = -4321.0

GEOMS = [(12, 20, 7, 13, 2, 5), (6, 600, 5, 515, 1, 80), (9, 9, 9, 9, 0, 0)]


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(n, dtype, fill):
    """(whole buffer, the n elements between two guard bands), all `fill`."""
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf, n, fill):
    b = buf.cpu()
    return bool((b[:GUARD] == fill).all()) and bool((b[GUARD + n:] == fill).all())


def reduce_ref(segs, heats, h, w, oy, ox, raw_heat):
    """numpy fp32, the kernel's order.  segs / heats: lists of [C, Hp, Wp] / [L, Hp, Wp] float32 arrays."""
    n = np.float32(len(segs))
    avg = None
    for s in segs:
        s = s[:, oy:oy + h, ox:ox + w]
        avg = s.copy() if avg is None else avg + s
    avg = avg / n
    assert avg.dtype == np.float32
    labels = np.argmax(avg, axis=0).astype(np.uint8)                  # the first maximal class
    heat, mm = None, []
    if heats:
        for t in heats:
            t = t[:, oy:oy + h, ox:ox + w]
            lo, hi = t.min(), t.max()
            mm.append((lo, hi))
            if not raw_heat:
                t = (t - lo) / (hi - lo)
            heat = t.copy() if heat is None else heat + t
        heat = heat / n
        assert heat.dtype == np.float32
    return labels, avg, heat, np.array(mm, dtype=np.float32)


def reduce_hip(segs, heats, h, w, oy, ox, raw_heat=0, want_avg=True, want_heat=True):
    """One dfl_ensemble_reduce call; outputs start as a sentinel between guard bands, minmax as NaN.  Returns numpy arrays
    (labels, avg or None, heat or None, minmax [nnets, 2] or None)."""
    lib = nat.lib()
    n, Hp, Wp = len(segs), segs[0].shape[1], segs[0].shape[2]
    L = heats[0].shape[0] if heats else 0
    sd = [torch.from_numpy(s).to(DEV).contiguous() for s in segs]
    hd = [torch.from_numpy(t).to(DEV).contiguous() for t in heats] if heats else []
    a = nat.EnsembleArgs()
    sp = torch.tensor([t.data_ptr() for t in sd], dtype=torch.int64).to(DEV)
    a.seg_ptrs = sp.data_ptr()
    lab_buf, lab = guarded(h * w, torch.uint8, 255)
    a.labels = lab.data_ptr()
    avg_buf = avg = heat_buf = heat = mm = hp = None
    if want_avg:
        avg_buf, avg = guarded(NC * h * w, torch.float32, SENT)
        a.avg_seg = avg.data_ptr()
    if L > 0:
        hp = torch.tensor([t.data_ptr() for t in hd], dtype=torch.int64).to(DEV)
        a.heat_ptrs = hp.data_ptr()
        mm = torch.full((2 * n * 65,), float('nan'), device=DEV)
        a.minmax = mm.data_ptr()
        if want_heat:
            heat_buf, heat = guarded(L * h * w, torch.float32, SENT)
            a.heat_out = heat.data_ptr()
    a.nnets, a.C, a.L, a.Hp, a.Wp, a.h, a.w, a.oy, a.ox = n, NC, L, Hp, Wp, h, w, oy, ox
    a.raw_heat = raw_heat
    nat.check(lib.dfl_ensemble_reduce(C.addressof(a), stream()), 'dfl_ensemble_reduce')
    torch.cuda.synchronize()
    assert guards_intact(lab_buf, h * w, 255)
    assert avg_buf is None or guards_intact(avg_buf, NC * h * w, SENT)
    assert heat_buf is None or guards_intact(heat_buf, L * h * w, SENT)
    return (lab.cpu().numpy().reshape(h, w), None if avg is None else avg.cpu().numpy().reshape(NC, h, w),
            None if heat is None else heat.cpu().numpy().reshape(L, h, w), None if mm is None else mm.cpu().numpy())


def bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def ulp_distance(got, ref):
    """Largest distance in units of the last place between two finite fp32 arrays of equal sign pattern."""
    return int(np.abs(bits(got).astype(np.int64) - bits(ref).astype(np.int64)).max())


_INPUTS = {}


def inputs(nnets, Hp, Wp):
    key = (nnets, Hp, Wp)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(7 * nnets + Hp + Wp)
        segs = [torch.softmax(3.0 * torch.randn(NC, Hp, Wp, generator=g), 0).float().numpy() for _ in range(nnets)]
        # heat maps of different range and offset per net, so the per-net min / max matter
        heats = [((k + 1) * 0.37 * torch.randn(3, Hp, Wp, generator=g) - 0.2 * k).float().numpy() for k in range(nnets)]
        _INPUTS[key] = (segs, heats)
    return _INPUTS[key]


@pytest.mark.parametrize('nnets', [1, 3, 8, 9])
@pytest.mark.parametrize('Hp,Wp,h,w,oy,ox', GEOMS)
def test_ensemble_reduce_is_bit_equal_to_fp32_in_net_order(Hp, Wp, h, w, oy, ox, nnets):
    segs, heats = inputs(nnets, Hp, Wp)
    for L in (0, 3):
        for raw in ((0, 1) if L else (0,)):
            rl, ravg, rheat, rmm = reduce_ref(segs, heats if L else [], h, w, oy, ox, raw)
            for want_avg in (True, False):
                for want_heat in ((True, False) if L else (False,)):
                    what = 'nets %d window %s L %d raw %d avg %d heat %d' % (nnets, (Hp, Wp, h, w, oy, ox), L, raw, want_avg, want_heat)
                    lab, avg, heat, mm = reduce_hip(segs, heats if L else [], h, w, oy, ox, raw, want_avg, want_heat)
                    assert np.array_equal(lab, rl), what + ': %d labels differ' % int((lab != rl).sum())
                    assert (avg is not None) == want_avg and (heat is not None) == (want_heat and L > 0)
                    if avg is not None:
                        assert np.array_equal(bits(avg), bits(ravg)), what + ': avg_seg differs by up to %d ulp' % ulp_distance(avg, ravg)
                    if heat is not None:
                        assert np.array_equal(bits(heat), bits(rheat)), what + ': heat_out differs by up to %d ulp' % ulp_distance(heat, rheat)
                    if mm is not None:
                        if want_heat and not raw:
                            assert np.array_equal(bits(mm[:2 * nnets].reshape(nnets, 2)), bits(rmm)), what + ': min/max table'
                        else:                                          # no normalisation: the scratch is not touched
                            assert bool(np.isnan(mm).all()), what


@pytest.mark.parametrize('nnets', [2, 4])
def test_ensemble_first_maximum_rule_on_exact_ties(nnets):
    """Soft-max inputs that are multiples of 2^-8 with 2 or 4 nets: the sums and the division are exact, so classes whose
    per-net values are permutations of one another tie exactly.  Pixels with equal maxima at classes (0, 3), (2, 5, 6) and
    all seven get the first of them; so does every accidental tie among the small random values elsewhere."""
    Hp, Wp, h, w, oy, ox = GEOMS[0]
    g = torch.Generator().manual_seed(nnets)
    ints = torch.randint(0, 8, (nnets, NC, Hp, Wp), generator=g).numpy().astype(np.int64)   # (few values: many accidental ties)
    top = np.array([200, 180, 160, 140][:nnets])
    ties = {(0, 0): (0, 3), (6, 12): (2, 5, 6), (3, 7): tuple(range(NC)), (0, 12): (2, 5, 6), (6, 0): (0, 3), (2, 1): (3, 4)}
    for (y, x), classes in ties.items():
        for j, c in enumerate(classes):
            ints[:, c, oy + y, ox + x] = np.roll(top, j)                # the same values in another net order: equal sums
    segs = [(ints[k] / 256.0).astype(np.float32) for k in range(nnets)]
    rl, ravg, _, _ = reduce_ref(segs, [], h, w, oy, ox, 0)
    for (y, x), classes in ties.items():
        col = ravg[:, y, x]
        assert all(col[c] == col.max() for c in classes) and int((col == col.max()).sum()) == len(classes)
        assert rl[y, x] == min(classes)
    sums = ints[:, :, oy:oy + h, ox:ox + w].sum(0)
    assert np.array_equal(ravg.astype(np.float64) * nnets * 256.0, sums)        # the fp32 reference is exact here
    assert int(((sums == sums.max(0, keepdims=True)).sum(0) > 1).sum()) > len(ties)   # and has accidental ties too
    lab, avg, _, _ = reduce_hip(segs, [], h, w, oy, ox)
    assert np.array_equal(bits(avg), bits(ravg))
    assert np.array_equal(lab, rl), 'labels differ at %s' % np.argwhere(lab != rl)[:8].tolist()
    for (y, x), classes in ties.items():
        assert lab[y, x] == min(classes), ((y, x), classes, int(lab[y, x]))


def test_ensemble_random_softmax_against_fp64():
    """Three nets at 40 x 56 (a window at (1, 3) of 44 x 64) against fp64: labels equal outside the project's margin mask
    (gpu_common.label_mask: top-2 margin under 1e-5 or under 2.5 x the measured deviation), which may cover 1% of the
    pixels at most; avg_seg within 4 * 2^-24 (two adds of partial sums up to 3 and one division, per unit of the result),
    normalised heat maps within 8 * 2^-24 (per net a subtraction, the range and a division, then the same sum)."""
    Hp, Wp, h, w, oy, ox = 44, 64, 40, 56, 1, 3
    segs, heats = inputs(3, Hp, Wp)
    lab, avg, heat, _ = reduce_hip(segs, heats, h, w, oy, ox)
    s64 = sum(torch.from_numpy(s).double()[:, oy:oy + h, ox:ox + w] for s in segs) / 3.0
    h64 = 0.0
    for t in heats:
        t = torch.from_numpy(t).double()[:, oy:oy + h, ox:ox + w]
        h64 = h64 + (t - t.min()) / (t.max() - t.min())
    h64 = h64 / 3.0
    d_avg = float((torch.from_numpy(avg).double() - s64).abs().max())
    d_heat = float((torch.from_numpy(heat).double() - h64).abs().max())
    print('ensemble against fp64: avg_seg %.3e, heat_out %.3e' % (d_avg, d_heat))
    assert d_avg <= 4 * 2.0 ** -24 and d_heat <= 8 * 2.0 ** -24
    mask = label_mask(s64[None], torch.from_numpy(avg)[None])[0]
    assert float(mask.double().mean()) <= 0.01
    ref = s64.argmax(0).to(torch.uint8)
    assert bool((torch.from_numpy(lab)[~mask] == ref[~mask]).all())
