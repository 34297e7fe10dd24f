"""The boundary loss on the GPU against its numpy restatement (boundary_ref.py): dfl_boundary_maps (exact where the squared
distance is a perfect square or the map is zero, one float32 ulp elsewhere), both stages of dfl_boundary_loss through the C
entry with the bars that follow from the arithmetic, determinism, refusals, and the two loss classes through
util.center_crop against the existing Dice classes."""
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
from dfl_amd import _native as nat, boundary  # noqa: E402
import boundary_ref as BR  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 9), (9, 1), (5, 7), (33, 130), (64, 64)]       # one row, one column, below a wave, ragged over the tiles, aligned
BATCH_CLASSES = [(B, C_) for B in (1, 3) for C_ in (2, 7, 16, 31)]   # 16 and 31 classes: more than one chunk of label sets
SENTINEL = -777.25


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda', torch.cuda.current_device())


_CASES = {}


def case(B, C_, h, w):
    """Labels, their model maps (computed once per case and left alone) and a seg of soft-max-like values.  Batch 3: class 1
    is absent from image 0 and a single pixel in image 2, image 1 is a single class."""
    key = (B, C_, h, w)
    if key not in _CASES:
        g = BR.random_labels(B, C_, h, w, seed=17 + 31 * C_ + h)
        if h * w > 1:
            g[g == 1] = 0
            g[-1, h // 2, w // 2] = 1                 # a one-pixel region
            if B == 3:
                g[1] = C_ - 1
        phi, d2 = BR.maps_of_labels(g, C_)
        rng = np.random.default_rng(5)
        e = np.exp(rng.normal(size=(B, C_, h, w)))
        seg = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
        for a in (g, phi, d2, seg):
            a.setflags(write=False)
        _CASES[key] = (g, phi, d2, seg)
    return _CASES[key]


def put(a, dev):
    return torch.from_numpy(np.array(a, order='C')).to(dev)


def window(a, dev, r0, c0, fill=SENTINEL):
    """`a` [B, C, h, w] as a window at (r0, c0) of a larger contiguous tensor filled with `fill`."""
    B, C_, h, w = a.shape
    big = torch.full((B, C_, h + r0 + 2, w + c0 + 3), fill, dtype=torch.float32, device=dev)
    view = big[..., r0:r0 + h, c0:c0 + w]
    view.copy_(put(a, dev))
    return big, view


def check_maps(got, phi, d2):
    assert got.dtype == np.float32 and got.shape == phi.shape
    root = np.sqrt(d2.astype(np.float64))
    exact = (root == np.rint(root)) | (phi == 0)
    assert np.array_equal(got[exact], phi[exact])
    assert (np.abs(got.astype(np.float64) - phi.astype(np.float64)) <= np.spacing(np.abs(phi)).astype(np.float64)).all()
    assert not np.signbit(got[got == 0]).any()


def loss_call(seg, phi, stage, skip_bg=False, beta=1.0, loss=None, gs=None, dseg=None, acc_loss=0, acc_grad=0, C_=None):
    """dfl_boundary_loss through the C entry; seg / dseg may be windows.  Returns the library's return code."""
    L = nat.lib()
    a = nat.BoundaryLossArgs()
    B, Cc, h, w = phi.shape
    a.B, a.C, a.h, a.w = B, (Cc if C_ is None else C_), h, w
    a.phi = phi.data_ptr()
    if seg is not None:
        a.seg, a.seg_sN, a.seg_sC, a.seg_sH = seg.data_ptr(), seg.stride(0), seg.stride(1), seg.stride(2)
    keep = None
    if stage == 1:
        keep = torch.empty(int(L.dfl_boundary_loss_scratch_doubles(B, Cc, h)), dtype=torch.float64, device=phi.device)
        a.loss, a.sums = loss.data_ptr(), keep.data_ptr()
    if dseg is not None:
        a.dseg = dseg.data_ptr()
        if not dseg.is_contiguous():
            a.dseg_sN, a.dseg_sC, a.dseg_sH = dseg.stride(0), dseg.stride(1), dseg.stride(2)
    a.skip_bg, a.stage, a.beta = int(skip_bg), stage, beta
    a.accumulate_loss, a.accumulate_grad = acc_loss, acc_grad
    a.grad_scale = gs.data_ptr() if gs is not None else None
    rc = L.dfl_boundary_loss(C.addressof(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del keep
    return rc


def value_bar(ref, mag, n, beta=1.0):
    """One rounding to float (2^-24, the bar grants 2^-23) and the two float64 sums of n exact products, kernel's and numpy's."""
    return 2.0 ** -23 * abs(beta * ref) + abs(beta) * n * 2.0 ** -52 * mag


# ---- maps -------------------------------------------------------------------------------------------------------------------
def test_one_pixel_images_are_all_zero():
    dev = _dev()
    for B, C_ in ((1, 2), (3, 7)):
        g = BR.random_labels(B, C_, 1, 1, 3)
        t = put(BR.one_hot(g, C_), dev)
        phi = boundary.signed_distance_maps(t)
        assert phi.shape == (B, C_, 1, 1) and phi.dtype == torch.float32
        got = phi.cpu().numpy()
        assert not got.any() and not np.signbit(got).any()
        seg = torch.rand((B, C_, 1, 1), device=dev)
        for skip_bg in (False, True):
            value, grad = boundary.boundary_term(seg, phi, skip_bg=skip_bg)
            assert value.item() == 0.0 and not np.signbit(value.item()) and not grad.cpu().numpy().any()


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('bc', BATCH_CLASSES, ids=lambda s: 'B%dC%d' % s)
def test_maps_against_the_model(shape, bc):
    dev = _dev()
    (B, C_), (h, w) = bc, shape
    g, phi, d2, _ = case(B, C_, h, w)
    onehot = BR.one_hot(g, C_)
    t = put(onehot, dev)
    got = boundary.signed_distance_maps(t)
    again = boundary.signed_distance_maps(t)
    check_maps(got.cpu().numpy(), phi, d2)
    assert torch.equal(got, again) and got.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()       # a second run: the same bits
    # a strided target -- a window of a larger tensor -- gives the bits of its contiguous copy
    big, view = window(onehot, dev, 1, 3, fill=9.0)
    assert not view.is_contiguous()
    assert boundary.signed_distance_maps(view).cpu().numpy().tobytes() == got.cpu().numpy().tobytes()
    # an image alone has the bits it has inside the batch
    if B > 1:
        for b in (0, B - 1):
            alone = boundary.signed_distance_maps(t[b:b + 1])
            assert alone.cpu().numpy().tobytes() == got[b:b + 1].cpu().numpy().tobytes()
    # what the class regions look like in these cases
    if B == 3 and h * w > 1:
        assert not phi[0, 1].any() and (phi[1] == 0).all() and int((g[2] == 1).sum()) == 1 and phi[2, 1].max() >= 1


def test_labels_are_the_first_maximum_of_any_values():
    """Ties and non-binary values: the label is torch.max's."""
    dev = _dev()
    rng = np.random.default_rng(11)
    B, C_, h, w = 2, 5, 9, 13
    t = rng.integers(-2, 3, size=(B, C_, h, w)).astype(np.float32) * 0.25            # few distinct values: ties everywhere
    t[0, :, 0, 0] = 0.5                                                              # all equal: label 0
    t[0, :, 0, 1] = [0.1, 0.7, 0.7, 0.7, -1.0]                                       # label 1
    g = BR.labels_of(t)
    assert g[0, 0, 0] == 0 and g[0, 0, 1] == 1
    tt = put(t, dev)
    assert np.array_equal(torch.from_numpy(t).max(dim=1)[1].numpy(), g)
    ties = int((np.sort(t, axis=1)[:, -1] == np.sort(t, axis=1)[:, -2]).sum())
    assert ties > 20
    phi, d2 = BR.maps_of_labels(g, C_)
    check_maps(boundary.signed_distance_maps(tt).cpu().numpy(), phi, d2)


# ---- value ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('bc', [(1, 2), (3, 7), (1, 31)], ids=lambda s: 'B%dC%d' % s)
def test_value_against_the_float64_model(shape, bc):
    dev = _dev()
    (B, C_), (h, w) = bc, shape
    _, _, _, seg_np = case(B, C_, h, w)
    phi = boundary.signed_distance_maps(put(BR.one_hot(case(B, C_, h, w)[0], C_), dev))
    phi_np = phi.cpu().numpy()                             # the model is evaluated on the kernel's own maps
    seg = put(seg_np, dev)
    for skip_bg in (False, True):
        ref, mag, n = BR.term(seg_np, phi_np, skip_bg)
        value, _ = boundary.boundary_term(seg, phi, skip_bg=skip_bg)
        again, _ = boundary.boundary_term(seg, phi, skip_bg=skip_bg)
        print('value', shape, bc, skip_bg, value.item(), ref, abs(value.item() - ref), value_bar(ref, mag, n))
        assert abs(float(value.item()) - ref) <= value_bar(ref, mag, n)
        assert value.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
        # seg through a window that starts at an odd column: the same assignment of pixels to threads, so the same bits
        for c0 in (1, 4):
            _, view = window(seg_np, dev, 2, c0)
            assert boundary.boundary_term(view, phi, skip_bg=skip_bg)[0].cpu().numpy().tobytes() == value.cpu().numpy().tobytes()
        # beta, and adding onto a value that is there
        beta = float(np.float32(0.37))
        loss = torch.full((), 3.0, dtype=torch.float32, device=dev)
        assert loss_call(seg, phi, 1, skip_bg, beta, loss=loss) == 0
        assert abs(float(loss.item()) - beta * ref) <= value_bar(ref, mag, n, beta)
        loss.fill_(3.0)
        assert loss_call(seg, phi, 1, skip_bg, beta, loss=loss, acc_loss=1) == 0
        exact = 3.0 + beta * ref
        print('accumulate', loss.item(), exact)
        assert abs(float(loss.item()) - exact) <= 2.0 ** -23 * abs(exact) + abs(beta) * n * 2.0 ** -52 * mag


# ---- gradient ---------------------------------------------------------------------------------------------------------------
def check_grad(got, ref, skip_bg):
    """Within 2^-22 |ref|: at most four float roundings of 2^-24 each; a skipped background channel exactly zero."""
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= 2.0 ** -22 * np.abs(ref)).all(), float((err - 2.0 ** -22 * np.abs(ref)).max())
    if skip_bg:
        assert not got[:, 0].any() and not np.signbit(got[:, 0]).any()


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('bc', [(1, 2), (3, 7), (1, 31)], ids=lambda s: 'B%dC%d' % s)
def test_gradient_against_the_model(shape, bc):
    dev = _dev()
    (B, C_), (h, w) = bc, shape
    g, _, _, seg_np = case(B, C_, h, w)
    phi = boundary.signed_distance_maps(put(BR.one_hot(g, C_), dev))
    phi_np = phi.cpu().numpy()
    beta = float(np.float32(0.37))
    half = torch.full((1,), 0.5, dtype=torch.float32, device=dev)
    for skip_bg in (False, True):
        _, plain = boundary.boundary_term(put(seg_np, dev), phi, skip_bg=skip_bg)
        check_grad(plain.cpu().numpy(), BR.grad(phi_np, skip_bg), skip_bg)
        for gs, scale in ((None, 1.0), (half, 0.5)):
            ref = BR.grad(phi_np, skip_bg, beta, scale)
            dense = torch.full((B, C_, h, w), SENTINEL, dtype=torch.float32, device=dev)
            assert loss_call(None, phi, 2, skip_bg, beta, gs=gs, dseg=dense) == 0
            check_grad(dense.cpu().numpy(), ref, skip_bg)
            # through a window into a sentinel-filled full-size tensor, at an aligned and at an odd column
            for c0 in (4, 1):
                big, view = window(np.full((B, C_, h, w), SENTINEL, dtype=np.float32), dev, 2, c0)
                assert loss_call(None, phi, 2, skip_bg, beta, gs=gs, dseg=view) == 0
                assert view.cpu().numpy().tobytes() == dense.cpu().numpy().tobytes()
                outside = torch.ones_like(big, dtype=torch.bool)
                outside[..., 2:2 + h, c0:c0 + w] = False
                assert (big[outside] == SENTINEL).all()
            # added onto what is there; a skipped background channel is left alone
            was = np.random.default_rng(3).normal(size=(B, C_, h, w)).astype(np.float32)
            for c0 in (0, 1):
                big, view = window(was, dev, 0, c0)
                assert loss_call(None, phi, 2, skip_bg, beta, gs=gs, dseg=view, acc_grad=1) == 0
                total = was.astype(np.float64) + ref
                err = np.abs(view.cpu().numpy().astype(np.float64) - total)
                assert (err <= 2.0 ** -22 * np.abs(ref) + 2.0 ** -24 * np.abs(total)).all()      # one more rounding: the sum's
                if skip_bg:
                    assert view[:, 0].cpu().numpy().tobytes() == was[:, 0].tobytes()


def test_gradient_added_onto_the_dice_gradient():
    """accumulate_grad onto the buffer dfl_dice_ncc_loss stage 2 filled, through the C entries of both."""
    dev = _dev()
    B, C_, h, w = 3, 7, 33, 130
    g, _, _, seg_np = case(B, C_, h, w)
    t = put(BR.one_hot(g, C_), dev)
    phi = boundary.signed_distance_maps(t)
    seg = put(seg_np, dev).requires_grad_(True)
    dfl_amd.DiceLoss2D(skip_bg=True)(seg, t).backward()          # stage 1, then stage 2 into a dense buffer
    dice = seg.grad.detach().clone()
    beta = float(np.float32(0.01))
    buf = dice.clone()
    assert loss_call(None, phi, 2, True, beta, dseg=buf, acc_grad=1) == 0
    ref = BR.grad(phi.cpu().numpy(), True, beta)
    total = dice.cpu().numpy().astype(np.float64) + ref
    err = np.abs(buf.cpu().numpy().astype(np.float64) - total)
    assert (err <= 2.0 ** -22 * np.abs(ref) + 2.0 ** -24 * np.abs(total)).all()
    assert torch.equal(buf[:, 0], dice[:, 0])


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    dev = _dev()
    L = nat.lib()
    B, C_, h, w = 2, 3, 5, 7
    t = put(BR.one_hot(BR.random_labels(B, C_, h, w, 1), C_), dev)
    phi = torch.full((B, C_, h, w), SENTINEL, dtype=torch.float32, device=dev)
    scratch = torch.empty(L.dfl_boundary_maps_scratch_bytes(B, C_, h, w), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def maps(B=B, C_=C_, h=h, w=w, tseg=t.data_ptr(), out=phi.data_ptr(), scr=scratch.data_ptr()):
        return L.dfl_boundary_maps(tseg, C_ * h * w, h * w, w, B, C_, h, w, out, scr, st)
    for kw in (dict(B=0), dict(C_=1), dict(C_=32), dict(h=0), dict(w=-2), dict(h=46342, w=1), dict(tseg=None), dict(scr=None),
               dict(scr=scratch.data_ptr() + 4)):
        assert maps(**kw) == nat.ERR_INVALID_ARG, kw
    assert maps(out=None) == nat.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (phi == SENTINEL).all()
    assert maps() == 0
    good = phi.clone()
    assert not (good == SENTINEL).any()
    seg = torch.rand((B, C_, h, w), device=dev)
    loss = torch.full((), SENTINEL, dtype=torch.float32, device=dev)
    dseg = torch.full((B, C_, h, w), SENTINEL, dtype=torch.float32, device=dev)
    for stage in (0, 3):
        assert loss_call(seg, good, stage, loss=loss, dseg=dseg) == nat.ERR_INVALID_ARG
    assert loss_call(seg, good, 1, loss=loss, C_=1) == nat.ERR_INVALID_ARG
    assert loss_call(seg, good, 2, dseg=dseg, C_=32) == nat.ERR_INVALID_ARG
    assert loss_call(seg, good, 1, beta=float('nan'), loss=loss) == nat.ERR_INVALID_ARG
    assert loss_call(seg, good, 2, dseg=None) == nat.ERR_INVALID_ARG
    assert loss.item() == SENTINEL and (dseg == SENTINEL).all()


# ---- the loss classes ---------------------------------------------------------------------------------------------------------
def _crop_run(criterion, out_np, target, dev, heat_np=None, theat=None):
    """loss and out.grad (and heat.grad) of criterion on the centre crop of a larger requires_grad tensor."""
    out = put(out_np, dev).requires_grad_(True)
    crop = dfl_amd.center_crop(out, target.shape)
    if heat_np is None:
        loss = criterion(crop, target)
        loss.backward()
        return loss.detach(), out.grad.detach().clone(), None
    heat = put(heat_np, dev).requires_grad_(True)
    loss = criterion((crop, dfl_amd.center_crop(heat, theat.shape)), (target, theat))
    loss.backward()
    return loss.detach(), out.grad.detach().clone(), heat.grad.detach().clone()


@pytest.mark.parametrize('pad', [8, 6], ids=['window at column 4', 'window at column 3'])
@pytest.mark.parametrize('skip_bg', [False, True])
def test_dice_boundary_class_through_center_crop(pad, skip_bg):
    dev = _dev()
    B, C_, h, w = 3, 7, 33, 130
    g, _, _, _ = case(B, C_, h, w)
    target = put(BR.one_hot(g, C_), dev)
    rng = np.random.default_rng(9)
    e = np.exp(rng.normal(size=(B, C_, h + pad, w + pad)))
    out_np = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    r0 = pad // 2
    beta = 0.01
    dice_value, dice_grad, _ = _crop_run(dfl_amd.DiceLoss2D(skip_bg=skip_bg), out_np, target, dev)
    crit = dfl_amd.DiceBoundaryLoss2D(skip_bg=skip_bg, boundary_wgt=beta)
    value, grad, _ = _crop_run(crit, out_np, target, dev)
    phi = boundary.signed_distance_maps(target).cpu().numpy()
    inner = np.zeros(grad.shape, dtype=bool)
    inner[..., r0:r0 + h, r0:r0 + w] = True
    got = grad.cpu().numpy()
    assert not got[~inner].any() and not np.signbit(got[~inner]).any()                      # the border: exactly zero
    ref = BR.grad(phi, skip_bg, float(np.float32(beta)))
    total = dice_grad.cpu().numpy()[inner].reshape(B, C_, h, w).astype(np.float64) + ref
    err = np.abs(got[inner].reshape(B, C_, h, w).astype(np.float64) - total)
    assert (err <= 2.0 ** -22 * np.abs(ref) + 2.0 ** -24 * np.abs(total)).all()
    seg_np = out_np[..., r0:r0 + h, r0:r0 + w]
    L_ref, mag, n = BR.term(seg_np, phi, skip_bg)
    exact = float(dice_value.item()) + float(np.float32(beta)) * L_ref
    assert abs(float(value.item()) - exact) <= 2.0 ** -23 * abs(exact) + n * 2.0 ** -52 * mag
    # weight 0: the existing class, bit for bit; a changed weight takes effect at the next call
    crit.boundary_wgt = 0.0
    v0, g0, _ = _crop_run(crit, out_np, target, dev)
    assert v0.cpu().numpy().tobytes() == dice_value.cpu().numpy().tobytes() and torch.equal(g0, dice_grad)
    assert g0.cpu().numpy().tobytes() == dice_grad.cpu().numpy().tobytes()
    crit.boundary_wgt = 0.5
    v5, g5, _ = _crop_run(crit, out_np, target, dev)
    exact = float(dice_value.item()) + 0.5 * L_ref
    assert abs(float(v5.item()) - exact) <= 2.0 ** -23 * abs(exact) + n * 2.0 ** -52 * mag
    ref5 = BR.grad(phi, skip_bg, 0.5)
    total5 = dice_grad.cpu().numpy()[inner].reshape(B, C_, h, w).astype(np.float64) + ref5
    err = np.abs(g5.cpu().numpy()[inner].reshape(B, C_, h, w).astype(np.float64) - total5)
    assert (err <= 2.0 ** -22 * np.abs(ref5) + 2.0 ** -24 * np.abs(total5)).all()
    # a second run: the same bits
    v5b, g5b, _ = _crop_run(crit, out_np, target, dev)
    assert v5b.cpu().numpy().tobytes() == v5.cpu().numpy().tobytes() and g5b.cpu().numpy().tobytes() == g5.cpu().numpy().tobytes()


def test_dice_heat_map_boundary_class_through_center_crop():
    dev = _dev()
    B, C_, L_, h, w, pad = 3, 7, 4, 33, 130, 8
    g, _, _, _ = case(B, C_, h, w)
    target = put(BR.one_hot(g, C_), dev)
    rng = np.random.default_rng(10)
    e = np.exp(rng.normal(size=(B, C_, h + pad, w + pad)))
    out_np = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    heat_np = rng.random((B, L_, h + pad, w + pad)).astype(np.float32)
    theat = put(rng.random((B, L_, h, w)).astype(np.float32), dev)
    beta = 0.01
    old = dfl_amd.DiceAndHeatMapLoss2D(skip_bg=False, heatmap_wgt=0.5)
    new = dfl_amd.DiceHeatMapBoundaryLoss2D(skip_bg=False, heatmap_wgt=0.5, boundary_wgt=beta)
    v_old, g_old, gh_old = _crop_run(old, out_np, target, dev, heat_np, theat)
    v_new, g_new, gh_new = _crop_run(new, out_np, target, dev, heat_np, theat)
    assert gh_new.cpu().numpy().tobytes() == gh_old.cpu().numpy().tobytes()                 # the heat gradient: the existing bits
    phi = boundary.signed_distance_maps(target).cpu().numpy()
    r0 = pad // 2
    inner = np.zeros(g_new.shape, dtype=bool)
    inner[..., r0:r0 + h, r0:r0 + w] = True
    got = g_new.cpu().numpy()
    assert not got[~inner].any()
    ref = BR.grad(phi, False, float(np.float32(beta)))
    total = g_old.cpu().numpy()[inner].reshape(B, C_, h, w).astype(np.float64) + ref
    err = np.abs(got[inner].reshape(B, C_, h, w).astype(np.float64) - total)
    assert (err <= 2.0 ** -22 * np.abs(ref) + 2.0 ** -24 * np.abs(total)).all()
    L_ref, mag, n = BR.term(out_np[..., r0:r0 + h, r0:r0 + w], phi, False)
    exact = float(v_old.item()) + float(np.float32(beta)) * L_ref
    assert abs(float(v_new.item()) - exact) <= 2.0 ** -23 * abs(exact) + n * 2.0 ** -52 * mag
    new.boundary_wgt = 0.0
    v0, g0, gh0 = _crop_run(new, out_np, target, dev, heat_np, theat)
    assert v0.cpu().numpy().tobytes() == v_old.cpu().numpy().tobytes()
    assert g0.cpu().numpy().tobytes() == g_old.cpu().numpy().tobytes() and gh0.cpu().numpy().tobytes() == gh_old.cpu().numpy().tobytes()
