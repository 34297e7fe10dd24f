"""The cross-entropy / focal term on the GPU against its numpy float64 restatement (ce_ref.py): both stages of dfl_ce_loss
through dfl_amd.ce and through the C entry, at the shapes where the row kernels take another path, with the bar that follows
from the arithmetic; determinism; and the two loss classes through util.center_crop against the existing Dice classes.

The bar, relative to the float64 reference on the same fp32 inputs: (16 + 2 gamma) 2^-24 per gradient element and for L_CE
(HIP's logf and powf are within 1 ulp and a division within about 2.5; an element is at most five such factors, and the error
of 1 - s enters powf gamma-fold), plus 2^-24 |result| wherever a float sum is rounded (the accumulated value and gradient).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfl_amd  # noqa: E402
from dfl_amd import _native as nat, boundary, ce  # noqa: E402
import boundary_ref as BR  # noqa: E402
import ce_ref as CR  # noqa: E402

pytestmark = pytest.mark.gpu

# one pixel; rows shorter than one 16-byte group; dense; rows that start at an odd column and are unaligned; 4200 rows: more
# than one pass of the capped grid of 1024 workgroups x 4 waves
SHAPES = {'one pixel': ((1, 2, 1, 1), None), 'short rows': ((2, 7, 5, 3), None), 'dense': ((2, 7, 9, 67), None),
          'window': ((2, 7, 9, 67), ((2, 7, 13, 71), 2, 3)), 'many rows': ((3, 7, 200, 5), None)}
GAMMAS = [0.0, 1.0, 2.0, 5.0]
W7 = (0.5, 2.0, 0.0, 1.25, 3.0, 0.75, 1.5)           # seven unequal weights, one of them 0 (two classes: the first two)
SENTINEL = -777.25
U = 2.0 ** -24


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda', torch.cuda.current_device())


def rel_bar(gamma):
    return (16 + 2 * gamma) * U


def weights_of(kind, C_):
    if kind == 'none':
        return None
    return W7[:C_] if C_ > 2 else (W7[0], W7[1])


_CASES = {}


def case(shape, kind='one-hot'):
    """(seg, target) as read-only fp32 numpy arrays, made once per (shape, kind)."""
    key = (shape, kind)
    if key not in _CASES:
        B, C_, h, w = shape
        seg = CR.softmax_noise(shape, seed=11 + h + 7 * w)
        g, t = CR.one_hot_labels(shape, seed=5 + h)
        rng = np.random.default_rng(23)
        if kind == 'soft':
            t = (rng.random(shape) * (rng.random(shape) < 0.6)).astype(np.float32)
        elif kind == 'outside':                      # the augmentation's "outside the frame": all masks 0 at some pixels
            out = rng.random((B, 1, h, w)) < 0.3
            t = np.where(out, np.float32(0), t).astype(np.float32)
            assert out.any() and not t.sum(axis=1)[out[:, 0]].any()
        elif kind == 'planted':                      # s = 1, s = 0, s = EPS / 2 and a denormal s, each at a target pixel
            assert h * w >= 8
            for k, s in enumerate((1.0, 0.0, CR.EPS / 2, 1e-41, 1.0, 0.0, CR.EPS / 2, 1e-41)):
                b, y, x = k % B, (3 * k) % h, (5 * k + 1) % w
                seg[b, g[b, y, x], y, x] = np.float32(s)
            assert 0 < float(np.float32(1e-41)) < np.finfo(np.float32).tiny
        seg.setflags(write=False)
        t.setflags(write=False)
        _CASES[key] = (seg, t)
    return _CASES[key]


def put(a, dev):
    return torch.from_numpy(np.array(a, order='C')).to(dev)


def placed(a, dev, where, fill=SENTINEL):
    """`a` on the device: dense, or (where = (full shape, r0, c0)) as a window of a larger contiguous tensor."""
    if where is None:
        t = put(a, dev)
        return t, t
    full, r0, c0 = where
    big = torch.full(full, fill, dtype=torch.float32, device=dev)
    view = big[..., r0:r0 + a.shape[2], c0:c0 + a.shape[3]]
    view.copy_(put(a, dev))
    assert not view.is_contiguous()
    return big, view


def check_value(got, seg, t, w, gamma, lam=1.0, onto=None):
    ref = lam * CR.value(seg, t, w, gamma)
    exact = ref if onto is None else onto + ref
    bar = rel_bar(gamma) * abs(ref) + (0.0 if onto is None else U * abs(exact))
    print('value', seg.shape, gamma, w is not None, got, exact, abs(got - exact), bar)
    assert abs(got - exact) <= bar


def check_grad(got, seg, t, w, gamma, lam=1.0, gs=1.0, onto=None):
    ref = CR.grad(seg, t, w, gamma, lam, gs)
    assert got.dtype == np.float32 and got.shape == ref.shape and np.isfinite(got).all()
    total = ref if onto is None else onto.astype(np.float64) + ref
    err = np.abs(got.astype(np.float64) - total)
    bar = rel_bar(gamma) * np.abs(ref) + (0.0 if onto is None else U * np.abs(total))
    print('gradient', seg.shape, gamma, w is not None, 'worst err / bar', float((err / np.maximum(bar, 1e-300)).max()))
    assert (err <= bar).all()
    dead = (np.ones(seg.shape[1]) if w is None else np.asarray(w)).reshape(1, -1, 1, 1) * t == 0
    if onto is None:
        assert not got[dead].any() and not np.signbit(got[dead]).any()            # exactly 0.0
    else:
        assert got[dead].tobytes() == onto[dead].tobytes()                        # left as they are


def entry(seg, tseg, stage, wgt=None, gamma=0.0, lam=1.0, loss=None, gs=None, dseg=None, acc_loss=0, acc_grad=0, null=(), **over):
    """dfl_ce_loss through the C entry; seg / tseg / dseg may be windows.  Returns the library's return code."""
    L = nat.lib()
    B, C_, h, wd = seg.shape
    a = ce._args(seg, tseg, lam, gamma, wgt)
    keep = None
    if stage == 1:
        keep = torch.empty(int(L.dfl_ce_loss_scratch_doubles(B, C_, h)), dtype=torch.float64, device=seg.device)
        a.loss, a.sums = loss.data_ptr(), keep.data_ptr()
    if dseg is not None:
        a.dseg = dseg.data_ptr()
        if not dseg.is_contiguous():
            a.dseg_sN, a.dseg_sC, a.dseg_sH = dseg.stride(0), dseg.stride(1), dseg.stride(2)
    a.stage, a.accumulate_loss, a.accumulate_grad = stage, acc_loss, acc_grad
    a.grad_scale = gs.data_ptr() if gs is not None else None
    for k, v in over.items():
        setattr(a, k, v)
    for k in null:
        setattr(a, k, None)
    rc = L.dfl_ce_loss(C.addressof(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del keep
    return rc


# ---- the plain term ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wkind', ['none', 'seven'])
@pytest.mark.parametrize('gamma', GAMMAS)
@pytest.mark.parametrize('name', list(SHAPES))
def test_value_and_gradient_against_the_float64_model(name, gamma, wkind):
    dev = _dev()
    shape, where = SHAPES[name]
    seg_np, t_np = case(shape)
    w = weights_of(wkind, shape[1])
    _, seg = placed(seg_np, dev, where)
    t = put(t_np, dev)
    value, grad = ce.cross_entropy_term(seg, t, class_weights=w, gamma=gamma)
    assert value.dtype == torch.float32 and value.dim() == 0 and grad.shape == shape and grad.is_contiguous()
    check_value(float(value.item()), seg_np, t_np, w, gamma)
    check_grad(grad.cpu().numpy(), seg_np, t_np, w, gamma)
    again_v, again_g = ce.cross_entropy_term(seg, t, class_weights=w, gamma=gamma)           # a second run: the same bits
    assert again_v.cpu().numpy().tobytes() == value.cpu().numpy().tobytes()
    assert again_g.cpu().numpy().tobytes() == grad.cpu().numpy().tobytes()
    # the assignment of pixels to threads follows the shape alone: a window, an aligned tensor and a strided target agree in bits
    if where is None and shape[3] > 1:
        _, sview = placed(seg_np, dev, ((shape[0], shape[1], shape[2] + 3, shape[3] + 5), 1, 1))
        _, tview = placed(t_np, dev, ((shape[0], shape[1], shape[2] + 2, shape[3] + 6), 2, 3), fill=0.5)
        v2, g2 = ce.cross_entropy_term(sview, tview, class_weights=w, gamma=gamma)
        assert v2.cpu().numpy().tobytes() == value.cpu().numpy().tobytes() and g2.cpu().numpy().tobytes() == grad.cpu().numpy().tobytes()


@pytest.mark.parametrize('gamma', GAMMAS)
@pytest.mark.parametrize('name', ['short rows', 'window', 'many rows'])
def test_lambda_scale_and_accumulation_through_the_c_entry(name, gamma):
    dev = _dev()
    shape, where = SHAPES[name]
    seg_np, t_np = case(shape)
    w = weights_of('seven', shape[1])
    _, seg = placed(seg_np, dev, where)
    t = put(t_np, dev)
    lam = float(np.float32(0.37))
    loss = torch.full((), 3.0, dtype=torch.float32, device=dev)
    assert entry(seg, t, 1, w, gamma, lam, loss=loss) == 0
    check_value(float(loss.item()), seg_np, t_np, w, gamma, lam)
    loss.fill_(3.0)
    assert entry(seg, t, 1, w, gamma, lam, loss=loss, acc_loss=1) == 0
    check_value(float(loss.item()), seg_np, t_np, w, gamma, lam, onto=3.0)
    half = torch.full((1,), 0.5, dtype=torch.float32, device=dev)
    for gs, scale in ((None, 1.0), (half, 0.5)):
        dense = torch.full(shape, SENTINEL, dtype=torch.float32, device=dev)
        assert entry(seg, t, 2, w, gamma, lam, gs=gs, dseg=dense) == 0
        check_grad(dense.cpu().numpy(), seg_np, t_np, w, gamma, lam, scale)
        # through a window into a sentinel-filled full-size tensor, at an aligned and at an odd column: the same bits, and
        # nothing outside the window is written
        for c0 in (4, 1):
            full = (shape[0], shape[1], shape[2] + 4, shape[3] + c0 + 3)
            big, view = placed(np.full(shape, SENTINEL, dtype=np.float32), dev, (full, 2, c0))
            assert entry(seg, t, 2, w, gamma, lam, gs=gs, dseg=view) == 0
            assert view.cpu().numpy().tobytes() == dense.cpu().numpy().tobytes()
            outside = torch.ones_like(big, dtype=torch.bool)
            outside[..., 2:2 + shape[2], c0:c0 + shape[3]] = False
            assert (big[outside] == SENTINEL).all()
        # added onto what is there; elements with w t == 0 keep their bits
        was = np.random.default_rng(3).normal(size=shape).astype(np.float32)
        for c0 in (0, 1):
            big, view = placed(was, dev, ((shape[0], shape[1], shape[2], shape[3] + c0 + 2), 0, c0))
            assert entry(seg, t, 2, w, gamma, lam, gs=gs, dseg=view, acc_grad=1) == 0
            check_grad(view.cpu().numpy(), seg_np, t_np, w, gamma, lam, scale, onto=was)


@pytest.mark.parametrize('gamma', GAMMAS)
@pytest.mark.parametrize('kind', ['soft', 'outside', 'planted'])
def test_soft_targets_empty_pixels_and_planted_probabilities(kind, gamma):
    dev = _dev()
    shape = (2, 7, 9, 67)
    seg_np, t_np = case(shape, kind)
    for w in (None, W7):
        _, seg = placed(seg_np, dev, ((2, 7, 13, 71), 2, 3))
        value, grad = ce.cross_entropy_term(seg, put(t_np, dev), class_weights=w, gamma=gamma)
        check_value(float(value.item()), seg_np, t_np, w, gamma)
        check_grad(grad.cpu().numpy(), seg_np, t_np, w, gamma)
        if kind == 'planted' and w is None:
            assert np.abs(grad.cpu().numpy()).max() > 2.0 ** 80      # below EPS the gradient is the formula at EPS, not zero


def test_refusals_leave_the_outputs_untouched():
    dev = _dev()
    shape = (2, 7, 5, 3)
    seg_np, t_np = case(shape)
    seg, t = put(seg_np, dev), put(t_np, dev)
    loss = torch.full((), SENTINEL, dtype=torch.float32, device=dev)
    dseg = torch.full(shape, SENTINEL, dtype=torch.float32, device=dev)
    E = nat.ERR_INVALID_ARG
    for stage in (0, 3):
        assert entry(seg, t, stage, loss=loss, dseg=dseg) == E
    assert entry(seg, t, 1, gamma=0.5, loss=loss) == E and entry(seg, t, 2, gamma=9.0, dseg=dseg) == E
    assert entry(seg, t, 1, lam=float('nan'), loss=loss) == E and entry(seg, t, 2, lam=float('inf'), dseg=dseg) == E
    assert entry(seg, t, 1, wgt=(1, 1, 1, -1, 1, 1, 1), loss=loss) == E and entry(seg, t, 2, wgt=(1, 1, 1, 1, 1, 1, float('nan')), dseg=dseg) == E
    assert entry(seg, t, 1, loss=loss, C=1) == E and entry(seg, t, 2, dseg=dseg, C=32) == E and entry(seg, t, 2, dseg=dseg, w=0) == E
    assert entry(seg, t, 1, loss=loss, null=('sums',)) == E and entry(seg, t, 2, dseg=None) == E and entry(seg, t, 2, dseg=dseg, null=('tseg',)) == E
    assert entry(seg, t, 1, loss=loss, null=('seg',)) == E and entry(seg, t, 1, loss=loss, null=('loss',)) == E
    assert entry(seg, t, 2, dseg=dseg, dseg_sN=105) == E
    assert loss.item() == SENTINEL and (dseg == SENTINEL).all()
    with pytest.raises(RuntimeError, match='class weights'):
        ce.cross_entropy_term(seg, t, class_weights=(1.0, 2.0))
    with pytest.raises(RuntimeError, match='shape'):
        ce.cross_entropy_term(seg, t[:, :6])
    with pytest.raises(ValueError, match='gamma'):
        ce.DiceCELoss2D(gamma=0.5)(seg, t)


# ---- the loss classes -------------------------------------------------------------------------------------------------------
B_, C_, H_, W_, PAD = 2, 7, 9, 67, (4, 6)             # the network output is 13 x 73: the centre crop starts at (2, 3)


def graph_nodes(loss):
    seen, todo = set(), [loss.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        todo.extend(f for f, _ in fn.next_functions)
    return len(seen)


def crop_run(criterion, out_np, target, dev, heat_np=None, theat=None, factor=None):
    """(loss, out.grad, heat.grad, nodes of the backward graph) of criterion on the centre crop of a larger requires_grad
    tensor."""
    out = put(out_np, dev).requires_grad_(True)
    crop = dfl_amd.center_crop(out, target.shape)
    heat = None
    if heat_np is None:
        loss = criterion(crop, target)
    else:
        heat = put(heat_np, dev).requires_grad_(True)
        loss = criterion((crop, dfl_amd.center_crop(heat, theat.shape)), (target, theat))
    nodes = graph_nodes(loss)
    (loss if factor is None else factor * loss).backward()
    return loss.detach(), out.grad.detach().clone(), None if heat is None else heat.grad.detach().clone(), nodes


def class_case(dev):
    shape = (B_, C_, H_, W_)
    _, t_np = case(shape)
    out_np = CR.softmax_noise((B_, C_, H_ + PAD[0], W_ + PAD[1]), seed=41)
    r0, c0 = PAD[0] // 2, PAD[1] // 2
    seg_np = np.ascontiguousarray(out_np[..., r0:r0 + H_, c0:c0 + W_])
    inner = np.zeros(out_np.shape, dtype=bool)
    inner[..., r0:r0 + H_, c0:c0 + W_] = True
    return shape, out_np, seg_np, t_np, put(t_np, dev), inner


def check_class(value, grad, base_value, base_grad, seg_np, t_np, inner, w, gamma, lam, shape, gs=1.0, extra=None):
    """value = (float)((double) base + lam L_ref), grad = base gradient + the CE gradient, each within the bar; the border of
    the uncropped gradient exactly zero.  extra: (value, value bar, gradient, gradient bar) of the boundary term that was added
    first, with the bars of test_gpu_boundary.py and the rounding of that float sum."""
    got = grad.cpu().numpy()
    assert not got[~inner].any() and not np.signbit(got[~inner]).any()
    ref = CR.grad(seg_np, t_np, w, gamma, lam, gs)
    L_ref = lam * CR.value(seg_np, t_np, w, gamma)
    base = base_grad.cpu().numpy()[inner].reshape(shape).astype(np.float64)
    total, gbar = base + ref, rel_bar(gamma) * np.abs(ref)
    exact, vbar = float(base_value.item()) + L_ref, rel_bar(gamma) * abs(L_ref)
    if extra is not None:
        gbar = gbar + extra[3] + U * np.abs(base + extra[2])
        vbar = vbar + extra[1] + 2 * U * abs(float(base_value.item()) + extra[0])
        total, exact = total + extra[2], exact + extra[0]
    err = np.abs(got[inner].reshape(shape).astype(np.float64) - total)
    assert (err <= gbar + U * np.abs(total)).all()
    print('class value', float(value.item()), exact, abs(float(value.item()) - exact), vbar + U * abs(exact))
    assert abs(float(value.item()) - exact) <= vbar + U * abs(exact)


@pytest.mark.parametrize('wkind', ['none', 'seven'])
@pytest.mark.parametrize('gamma', GAMMAS)
def test_dice_ce_class_through_center_crop(gamma, wkind):
    dev = _dev()
    shape, out_np, seg_np, t_np, target, inner = class_case(dev)
    w = weights_of(wkind, C_)
    lam = float(np.float32(0.3))
    dice_v, dice_g, _, dice_nodes = crop_run(dfl_amd.DiceLoss2D(skip_bg=True), out_np, target, dev)
    crit = dfl_amd.DiceCELoss2D(skip_bg=True, ce_wgt=lam, gamma=gamma, class_weights=w)
    v, g, _, nodes = crop_run(crit, out_np, target, dev)
    assert nodes == dice_nodes                                          # one node: the fast path of util._Crop.backward
    check_class(v, g, dice_v, dice_g, seg_np, t_np, inner, w, gamma, lam, shape)
    v2, g2, _, _ = crop_run(crit, out_np, target, dev)                    # a second run: the same bits
    assert v2.cpu().numpy().tobytes() == v.cpu().numpy().tobytes() and g2.cpu().numpy().tobytes() == g.cpu().numpy().tobytes()
    # an upstream factor scales the gradient
    _, dice_h, _, _ = crop_run(dfl_amd.DiceLoss2D(skip_bg=True), out_np, target, dev, factor=0.5)
    vh, gh, _, _ = crop_run(crit, out_np, target, dev, factor=0.5)
    assert vh.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()
    check_class(vh, gh, dice_v, dice_h, seg_np, t_np, inner, w, gamma, lam, shape, gs=0.5)
    # weight 0: the existing class, bit for bit; a changed weight takes effect at the next call
    crit.ce_wgt = 0.0
    v0, g0, _, _ = crop_run(crit, out_np, target, dev)
    assert v0.cpu().numpy().tobytes() == dice_v.cpu().numpy().tobytes() and g0.cpu().numpy().tobytes() == dice_g.cpu().numpy().tobytes()
    crit.boundary_wgt = 0.01
    vb, gb, _, _ = crop_run(dfl_amd.DiceBoundaryLoss2D(skip_bg=True, boundary_wgt=0.01), out_np, target, dev)
    v0, g0, _, _ = crop_run(crit, out_np, target, dev)
    assert v0.cpu().numpy().tobytes() == vb.cpu().numpy().tobytes() and g0.cpu().numpy().tobytes() == gb.cpu().numpy().tobytes()
    crit.boundary_wgt, crit.ce_wgt, crit.gamma = 0.0, 1.0, 0.0
    v1, g1, _, _ = crop_run(crit, out_np, target, dev)
    check_class(v1, g1, dice_v, dice_g, seg_np, t_np, inner, w, 0.0, 1.0, shape)


@pytest.mark.parametrize('gamma', [0.0, 2.0])
def test_all_three_terms_against_the_sum_of_the_references(gamma):
    dev = _dev()
    shape, out_np, seg_np, t_np, target, inner = class_case(dev)
    lam, beta = float(np.float32(0.3)), float(np.float32(0.01))
    for skip_bg in (False, True):
        dice_v, dice_g, _, dice_nodes = crop_run(dfl_amd.DiceLoss2D(skip_bg=skip_bg), out_np, target, dev)
        crit = dfl_amd.DiceCELoss2D(skip_bg=skip_bg, ce_wgt=lam, gamma=gamma, class_weights=W7, boundary_wgt=beta)
        v, g, _, nodes = crop_run(crit, out_np, target, dev)
        assert nodes == dice_nodes
        phi = boundary.signed_distance_maps(target).cpu().numpy()
        rb = BR.grad(phi, skip_bg, beta)
        Lb, mag, n = BR.term(seg_np, phi, skip_bg)
        extra = (beta * Lb, n * 2.0 ** -52 * mag, rb, 2.0 ** -22 * np.abs(rb))
        check_class(v, g, dice_v, dice_g, seg_np, t_np, inner, W7, gamma, lam, shape, extra=extra)


def test_dice_heat_map_ce_class_through_center_crop():
    dev = _dev()
    shape, out_np, seg_np, t_np, target, inner = class_case(dev)
    L_ = 4
    rng = np.random.default_rng(10)
    heat_np = rng.random((B_, L_, H_ + PAD[0], W_ + PAD[1])).astype(np.float32)
    theat = put(rng.random((B_, L_, H_, W_)).astype(np.float32), dev)
    lam, gamma = float(np.float32(0.3)), 2.0
    old = dfl_amd.DiceAndHeatMapLoss2D(skip_bg=False, heatmap_wgt=0.5)
    new = dfl_amd.DiceHeatMapCELoss2D(skip_bg=False, heatmap_wgt=0.5, ce_wgt=lam, gamma=gamma, class_weights=W7)
    v_old, g_old, gh_old, nodes_old = crop_run(old, out_np, target, dev, heat_np, theat)
    v_new, g_new, gh_new, nodes_new = crop_run(new, out_np, target, dev, heat_np, theat)
    assert nodes_new == nodes_old
    assert gh_new.cpu().numpy().tobytes() == gh_old.cpu().numpy().tobytes()                 # the heat gradient: the existing bits
    check_class(v_new, g_new, v_old, g_old, seg_np, t_np, inner, W7, gamma, lam, shape)
    # an upstream factor
    _, g_oldh, gh_oldh, _ = crop_run(old, out_np, target, dev, heat_np, theat, factor=0.5)
    v_h, g_h, gh_h, _ = crop_run(new, out_np, target, dev, heat_np, theat, factor=0.5)
    assert gh_h.cpu().numpy().tobytes() == gh_oldh.cpu().numpy().tobytes()
    check_class(v_h, g_h, v_old, g_oldh, seg_np, t_np, inner, W7, gamma, lam, shape, gs=0.5)
    # all three terms, against the boundary class plus the CE reference's bits of freedom
    new.boundary_wgt = 0.01
    phi = boundary.signed_distance_maps(target).cpu().numpy()
    beta = float(np.float32(0.01))
    rb = BR.grad(phi, False, beta)
    Lb, mag, n = BR.term(seg_np, phi, False)
    v3, g3, gh3, nodes3 = crop_run(new, out_np, target, dev, heat_np, theat)
    assert nodes3 == nodes_old and gh3.cpu().numpy().tobytes() == gh_old.cpu().numpy().tobytes()
    check_class(v3, g3, v_old, g_old, seg_np, t_np, inner, W7, gamma, lam, shape,
                extra=(beta * Lb, n * 2.0 ** -52 * mag, rb, 2.0 ** -22 * np.abs(rb)))
    # weight 0: the existing classes, bit for bit
    new.ce_wgt = 0.0
    vb, gb, ghb, _ = crop_run(dfl_amd.DiceHeatMapBoundaryLoss2D(skip_bg=False, heatmap_wgt=0.5, boundary_wgt=0.01), out_np, target, dev,
                              heat_np, theat)
    v0, g0, gh0, _ = crop_run(new, out_np, target, dev, heat_np, theat)
    assert v0.cpu().numpy().tobytes() == vb.cpu().numpy().tobytes() and g0.cpu().numpy().tobytes() == gb.cpu().numpy().tobytes()
    assert gh0.cpu().numpy().tobytes() == ghb.cpu().numpy().tobytes()
    new.boundary_wgt = 0.0
    v0, g0, gh0, _ = crop_run(new, out_np, target, dev, heat_np, theat)
    assert v0.cpu().numpy().tobytes() == v_old.cpu().numpy().tobytes() and g0.cpu().numpy().tobytes() == g_old.cpu().numpy().tobytes()
    assert gh0.cpu().numpy().tobytes() == gh_old.cpu().numpy().tobytes()
