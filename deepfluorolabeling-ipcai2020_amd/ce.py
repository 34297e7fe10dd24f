"""Cross-entropy and focal terms on the GPU (include/dfl_hip.h, "Cross-entropy and focal term"): the
per-pixel likelihood of the target under the soft-max probabilities the head writes,

    L_CE = (1 / (B h w)) sum over b, c, p of  -w_c t (1 - s')^gamma log s',      s' = min(max(s, 2^-100), 1),

with class weights ``w_c`` (default all 1) and the focusing exponent ``gamma`` (0: plain cross-entropy; else 1..8).  Every
channel counts, background included: ``skip_bg`` belongs to Dice; a caller who wants no background gives ``w_0 = 0``.

``cross_entropy_term(seg, target)`` is the plain kernel call.  ``DiceCELoss2D`` and ``DiceHeatMapCELoss2D`` are
``dice.DiceLoss2D`` and ``dice.DiceAndHeatMapLoss2D`` plus ``boundary_wgt`` times the boundary term of ``boundary.py`` plus
``ce_wgt`` times this term, each ONE autograd node: the values are added onto the Dice value on the device and the gradients
onto the Dice gradient inside the zero-bordered buffer that ``util.center_crop``'s backward hands on as it is.
``balanced_class_weights(counts)`` is scikit-learn's "balanced" rule on the host.

Nobody has tuned ``ce_wgt``, ``gamma`` or the class weights on this data.
"""
import ctypes as C
import math

import torch
import torch.nn.modules.loss

from . import _native as nat
from . import boundary
from .boundary import _BoundaryLossFn, _stream
from .dice import _LossFn, _view4

__all__ = ['cross_entropy_term', 'balanced_class_weights', 'DiceCELoss2D', 'DiceHeatMapCELoss2D']


def balanced_class_weights(counts):
    """Pixel counts per class -> the weights w_c = total / (C n_c) of scikit-learn's class_weight='balanced', 0 for a class
    without pixels (C counts every class, the empty ones too).  A host function: (6, 3, 0, 3) -> (0.5, 1.0, 0.0, 1.0)."""
    counts = [int(n) for n in counts]
    if not counts or min(counts) < 0:
        raise ValueError('balanced_class_weights: counts must be non-negative, one per class: %r' % (counts,))
    total = sum(counts)
    return tuple(total / (len(counts) * n) if n > 0 else 0.0 for n in counts)


def _weights(class_weights, Cc):
    if class_weights is None:
        return (1.0,) * Cc
    if isinstance(class_weights, torch.Tensor):
        class_weights = class_weights.detach().cpu().tolist()
    w = tuple(float(v) for v in class_weights)
    if len(w) != Cc:
        raise RuntimeError('%d class weights for %d classes' % (len(w), Cc))
    return w


def _args(seg_v, tseg_v, ce_wgt, gamma, class_weights):
    if seg_v.shape != tseg_v.shape:
        raise RuntimeError('segmentation input %s and target %s differ in shape' % (tuple(seg_v.shape), tuple(tseg_v.shape)))
    B, Cc, h, w = seg_v.shape
    a = nat.CeLossArgs()
    a.seg, a.tseg = seg_v.data_ptr(), tseg_v.data_ptr()
    a.seg_sN, a.seg_sC, a.seg_sH = seg_v.stride(0), seg_v.stride(1), seg_v.stride(2)
    a.tseg_sN, a.tseg_sC, a.tseg_sH = tseg_v.stride(0), tseg_v.stride(1), tseg_v.stride(2)
    a.B, a.C, a.h, a.w = B, Cc, h, w
    setattr(a, 'lambda', float(ce_wgt))                  # (the header's name; Python reserves it)
    a.gamma = float(gamma)
    for c, v in enumerate(_weights(class_weights, Cc)[:len(a.class_wgt)]):
        a.class_wgt[c] = v
    return a


def _value(a, loss, accumulate, stream):
    """Stage 1 of dfl_ce_loss into the device scalar `loss`; returns the records it used (kept alive by the caller)."""
    sums = torch.empty(max(int(nat.lib().dfl_ce_loss_scratch_doubles(a.B, a.C, a.h)), 1), dtype=torch.float64, device=loss.device)
    a.loss, a.sums = loss.data_ptr(), sums.data_ptr()
    a.stage, a.accumulate_loss = 1, 1 if accumulate else 0
    nat.check(nat.lib().dfl_ce_loss(C.addressof(a), stream), 'dfl_ce_loss')
    return sums


def cross_entropy_term(seg, target, class_weights=None, gamma=0.0):
    """(value, grad) of L_CE: a device scalar and the dense gradient [B, C, h, w] (exact zeros where w_c t == 0).  The plain
    kernel call; seg and target may be strided views with unit stride along w."""
    seg_v, tseg_v = _view4(seg.detach(), 'input'), _view4(target.detach(), 'target')
    a = _args(seg_v, tseg_v, 1.0, gamma, class_weights)
    loss = torch.empty((), dtype=torch.float32, device=seg_v.device)
    grad = torch.empty(tuple(seg_v.shape), dtype=torch.float32, device=seg_v.device)
    with torch.cuda.device(seg_v.device):
        sums = _value(a, loss, False, _stream(seg_v))
        a.stage, a.dseg, a.accumulate_grad = 2, grad.data_ptr(), 0
        nat.check(nat.lib().dfl_ce_loss(C.addressof(a), _stream(seg_v)), 'dfl_ce_loss')
    del sums
    return loss, grad


class _CELossFn(torch.autograd.Function):
    """dice._LossFn, optionally the boundary term, and the cross-entropy term in one node.  Forward: _LossFn's forward (or
    boundary._BoundaryLossFn's, which is that plus the maps and dfl_boundary_loss stage 1), then dfl_ce_loss stage 1 adding
    onto the same device scalar.  Backward: theirs writes the gradient (into the zero-bordered buffer when the input is a
    centre-crop window), then dfl_ce_loss stage 2 adds onto the same elements on the same stream."""

    @staticmethod
    def forward(ctx, seg, heat, tseg, theat, skip_bg, dice_wgt, heat_wgt, boundary_wgt, ce_wgt, gamma, class_weights):
        ctx.with_boundary = boundary_wgt != 0.0
        if ctx.with_boundary:
            loss = _BoundaryLossFn.forward(ctx, seg, heat, tseg, theat, skip_bg, dice_wgt, heat_wgt, boundary_wgt)
        else:
            loss = _LossFn.forward(ctx, seg, heat, tseg, theat, skip_bg, dice_wgt, heat_wgt)
        seg_v, tseg_v = ctx.keep[0], ctx.keep[1]
        e = ctx.ce = _args(seg_v, tseg_v, ce_wgt, gamma, class_weights)
        with torch.cuda.device(seg_v.device):
            sums = _value(e, loss, True, _stream(seg_v))
        ctx.keep = ctx.keep + (sums,)
        return loss

    @staticmethod
    def backward(ctx, g):
        dseg, dheat = (_BoundaryLossFn if ctx.with_boundary else _LossFn).backward(ctx, g)[:2]
        if dseg is not None:
            a, e = ctx.args, ctx.ce                      # _LossFn.backward left the gradient's address and strides in a
            gs = g.detach().to(torch.float32).reshape(1).contiguous()
            e.stage, e.accumulate_grad = 2, 1
            e.grad_scale = gs.data_ptr()
            e.dseg, e.dseg_sN, e.dseg_sC, e.dseg_sH = a.dseg, a.dseg_sN, a.dseg_sC, a.dseg_sH
            with torch.cuda.device(dseg.device):
                nat.check(nat.lib().dfl_ce_loss(C.addressof(e), _stream(dseg)), 'dfl_ce_loss')
        return (dseg, dheat) + (None,) * 9


def _apply(seg, heat, tseg, theat, skip_bg, dice_wgt, heat_wgt, boundary_wgt, ce_wgt, gamma, class_weights):
    ce_wgt, gamma, boundary_wgt = float(ce_wgt), float(gamma), float(boundary_wgt)
    if ce_wgt == 0.0:                # the existing nodes, bit for bit
        return boundary._apply(seg, heat, tseg, theat, skip_bg, dice_wgt, heat_wgt, boundary_wgt)
    if not (math.isfinite(gamma) and (gamma == 0.0 or 1.0 <= gamma <= 8.0)):
        raise ValueError('gamma = %r: 0 (cross-entropy) or 1..8 (focal)' % (gamma,))
    if class_weights is not None:
        class_weights = _weights(class_weights, len(class_weights))
    return _CELossFn.apply(seg, heat, tseg, theat, skip_bg, dice_wgt, heat_wgt, boundary_wgt, ce_wgt, gamma, class_weights)


class DiceCELoss2D(torch.nn.modules.loss._Loss):
    """dice.DiceLoss2D plus ``ce_wgt`` times the cross-entropy / focal term plus ``boundary_wgt`` times the boundary term;
    ``ce_wgt``, ``gamma`` and ``boundary_wgt`` may be changed between calls."""

    def __init__(self, skip_bg=True, ce_wgt=1.0, gamma=0.0, class_weights=None, boundary_wgt=0.0):
        super().__init__()
        self.skip_bg = skip_bg
        self.ce_wgt, self.gamma, self.class_weights, self.boundary_wgt = ce_wgt, gamma, class_weights, boundary_wgt

    def forward(self, input, target):
        return _apply(input, None, target, None, self.skip_bg, 1.0, 0.0, self.boundary_wgt, self.ce_wgt, self.gamma,
                      self.class_weights)


class DiceHeatMapCELoss2D(torch.nn.modules.loss._Loss):
    """dice.DiceAndHeatMapLoss2D plus ``ce_wgt`` times the cross-entropy / focal term and ``boundary_wgt`` times the boundary
    term of the segmentation channels; the Dice and heat-map weights are what they are there."""

    def __init__(self, skip_bg=True, heatmap_wgt=0.5, ce_wgt=1.0, gamma=0.0, class_weights=None, boundary_wgt=0.0):
        super().__init__()
        assert (heatmap_wgt > 1.0e-8) and (heatmap_wgt < (1 + 1.0e-8))
        self.skip_bg = skip_bg
        self.heatmap_wgt = heatmap_wgt
        self.dice_wgt = 1 - heatmap_wgt
        self.ce_wgt, self.gamma, self.class_weights, self.boundary_wgt = ce_wgt, gamma, class_weights, boundary_wgt

    def forward(self, input, target):
        return _apply(input[0], input[1], target[0], target[1], self.skip_bg, float(self.dice_wgt), float(self.heatmap_wgt),
                      self.boundary_wgt, self.ce_wgt, self.gamma, self.class_weights)
