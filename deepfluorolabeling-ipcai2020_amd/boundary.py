"""Boundary loss on the GPU (Kervadec et al., MIDL 2019; include/dfl_hip.h, "Boundary loss"): train on
where the outline lies, not only on how much overlaps.

``signed_distance_maps(target)`` turns a batch of one-hot targets into the signed distance maps phi on the device
(dfl_boundary_maps: arg-max, the exact distance transform of labels.edt, combine); ``boundary_term(seg, phi)`` is the plain
term mean(seg * phi) and its gradient phi / N.  ``DiceBoundaryLoss2D`` and ``DiceHeatMapBoundaryLoss2D`` are
``dice.DiceLoss2D`` and ``dice.DiceAndHeatMapLoss2D`` plus ``boundary_wgt`` times that term, each ONE autograd node: the
value is added onto the Dice value on the device and the gradient onto the Dice gradient inside the zero-bordered buffer
that ``util.center_crop``'s backward hands on as it is.

The weight 0.01 is where the paper that proposed the loss starts; nobody has tuned it on this data.
"""
import ctypes as C

import torch
import torch.nn.modules.loss

from . import _native as nat
from .dice import _LossFn, _view4

__all__ = ['signed_distance_maps', 'boundary_term', 'DiceBoundaryLoss2D', 'DiceHeatMapBoundaryLoss2D']

_SCRATCH = {}       # (device, B, C, h, w) -> the scratch of dfl_boundary_maps; one stream at a time uses a shape's scratch


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _maps(tseg_v):
    """phi of a kernel view (dice._view4) of the one-hot target."""
    B, Cc, h, w = tseg_v.shape
    lib = nat.lib()
    key = (str(tseg_v.device), B, Cc, h, w)
    scratch = _SCRATCH.get(key)
    if scratch is None:
        nbytes = nat.check(lib.dfl_boundary_maps_scratch_bytes(B, Cc, h, w), 'dfl_boundary_maps_scratch_bytes')
        scratch = _SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=tseg_v.device)
    phi = torch.empty((B, Cc, h, w), dtype=torch.float32, device=tseg_v.device)
    with torch.cuda.device(tseg_v.device):
        nat.check(lib.dfl_boundary_maps(tseg_v.data_ptr(), tseg_v.stride(0), tseg_v.stride(1), tseg_v.stride(2), B, Cc, h, w,
                                        phi.data_ptr(), scratch.data_ptr(), _stream(tseg_v)), 'dfl_boundary_maps')
    return phi


def signed_distance_maps(target):
    """One-hot target [B, C, h, w] on the device (any strided view with unit stride along w; C = 2..31) -> phi, fp32
    [B, C, h, w]: per class the Euclidean distance in pixels to the class's region outside it, minus the distance to its
    complement (less one) inside it, zero throughout for a class that is absent from the image or fills it.  The label of a
    pixel is the arg-max over the channels, the first maximum winning."""
    return _maps(_view4(target.detach(), 'target'))


def _args(seg_v, phi, skip_bg, beta):
    B, Cc, h, w = seg_v.shape
    if tuple(phi.shape) != (B, Cc, h, w) or phi.dtype != torch.float32 or not phi.is_contiguous() or phi.device != seg_v.device:
        raise RuntimeError('phi must be a contiguous fp32 tensor of shape %s on %s' % ((B, Cc, h, w), seg_v.device))
    a = nat.BoundaryLossArgs()
    a.seg, a.phi = seg_v.data_ptr(), phi.data_ptr()
    a.seg_sN, a.seg_sC, a.seg_sH = seg_v.stride(0), seg_v.stride(1), seg_v.stride(2)
    a.B, a.C, a.h, a.w = B, Cc, h, w
    a.skip_bg = 1 if skip_bg else 0
    a.beta = beta
    return a


def _value(a, loss, accumulate, stream):
    """Stage 1 of dfl_boundary_loss into the device scalar `loss`; returns the records it used (kept alive by the caller)."""
    sums = torch.empty(int(nat.lib().dfl_boundary_loss_scratch_doubles(a.B, a.C, a.h)), dtype=torch.float64, device=loss.device)
    a.loss, a.sums = loss.data_ptr(), sums.data_ptr()
    a.stage, a.accumulate_loss = 1, 1 if accumulate else 0
    nat.check(nat.lib().dfl_boundary_loss(C.addressof(a), stream), 'dfl_boundary_loss')
    return sums


def boundary_term(seg, phi, skip_bg=True):
    """(value, grad) of L_B = mean over b, c >= skip_bg, p of seg * phi: a device scalar and the dense gradient phi / N
    (zeros in a skipped background channel), N = B (C - skip_bg) h w.  The plain kernel call, for callers who keep their
    own maps."""
    seg_v = _view4(seg.detach(), 'input')
    a = _args(seg_v, phi, skip_bg, 1.0)
    loss = torch.empty((), dtype=torch.float32, device=seg_v.device)
    grad = torch.empty(tuple(seg_v.shape), dtype=torch.float32, device=seg_v.device)
    with torch.cuda.device(seg_v.device):
        sums = _value(a, loss, False, _stream(seg_v))
        a.stage, a.dseg, a.accumulate_grad = 2, grad.data_ptr(), 0
        nat.check(nat.lib().dfl_boundary_loss(C.addressof(a), _stream(seg_v)), 'dfl_boundary_loss')
    del sums
    return loss, grad


class _BoundaryLossFn(torch.autograd.Function):
    """dice._LossFn and the boundary term in one node.  Forward: _LossFn's forward (dfl_dice_ncc_loss stage 1), the maps,
    dfl_boundary_loss stage 1 adding onto the same device scalar.  Backward: _LossFn's backward writes the Dice gradient
    (into the zero-bordered buffer when the input is a centre-crop window), then dfl_boundary_loss stage 2 adds onto the
    same elements on the same stream.  Two nodes would make autograd sum two window views into a fresh dense tensor, and
    util._Crop.backward would fall to its generic path."""

    @staticmethod
    def forward(ctx, seg, heat, tseg, theat, skip_bg, dice_wgt, heat_wgt, boundary_wgt):
        loss = _LossFn.forward(ctx, seg, heat, tseg, theat, skip_bg, dice_wgt, heat_wgt)
        seg_v, tseg_v = ctx.keep[0], ctx.keep[1]
        phi = _maps(tseg_v)
        b = ctx.boundary = _args(seg_v, phi, skip_bg, boundary_wgt)
        with torch.cuda.device(seg_v.device):
            sums = _value(b, loss, True, _stream(seg_v))
        ctx.keep = ctx.keep + (phi, sums)
        return loss

    @staticmethod
    def backward(ctx, g):
        dseg, dheat = _LossFn.backward(ctx, g)[:2]
        if dseg is not None:
            a, b = ctx.args, ctx.boundary                # _LossFn.backward left the gradient's address and strides in a
            gs = g.detach().to(torch.float32).reshape(1).contiguous()
            b.stage, b.accumulate_grad = 2, 1
            b.grad_scale = gs.data_ptr()
            b.dseg, b.dseg_sN, b.dseg_sC, b.dseg_sH = a.dseg, a.dseg_sN, a.dseg_sC, a.dseg_sH
            with torch.cuda.device(dseg.device):
                nat.check(nat.lib().dfl_boundary_loss(C.addressof(b), _stream(dseg)), 'dfl_boundary_loss')
        return dseg, dheat, None, None, None, None, None, None


def _apply(seg, heat, tseg, theat, skip_bg, dice_wgt, heat_wgt, boundary_wgt):
    boundary_wgt = float(boundary_wgt)
    if boundary_wgt == 0.0:          # the existing node, bit for bit
        return _LossFn.apply(seg, heat, tseg, theat, skip_bg, dice_wgt, heat_wgt)
    return _BoundaryLossFn.apply(seg, heat, tseg, theat, skip_bg, dice_wgt, heat_wgt, boundary_wgt)


class DiceBoundaryLoss2D(torch.nn.modules.loss._Loss):
    """dice.DiceLoss2D plus ``boundary_wgt`` times the boundary term; ``boundary_wgt`` may be changed between calls."""

    def __init__(self, skip_bg=True, boundary_wgt=0.01):
        super().__init__()
        self.skip_bg = skip_bg
        self.boundary_wgt = boundary_wgt

    def forward(self, input, target):
        return _apply(input, None, target, None, self.skip_bg, 1.0, 0.0, self.boundary_wgt)


class DiceHeatMapBoundaryLoss2D(torch.nn.modules.loss._Loss):
    """dice.DiceAndHeatMapLoss2D plus ``boundary_wgt`` times the boundary term of the segmentation channels; the Dice and
    heat-map weights are what they are there."""

    def __init__(self, skip_bg=True, heatmap_wgt=0.5, boundary_wgt=0.01):
        super().__init__()
        assert (heatmap_wgt > 1.0e-8) and (heatmap_wgt < (1 + 1.0e-8))
        self.skip_bg = skip_bg
        self.heatmap_wgt = heatmap_wgt
        self.dice_wgt = 1 - heatmap_wgt
        self.boundary_wgt = boundary_wgt

    def forward(self, input, target):
        return _apply(input[0], input[1], target[0], target[1], self.skip_bg, float(self.dice_wgt), float(self.heatmap_wgt),
                      self.boundary_wgt)
