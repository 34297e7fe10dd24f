"""SGD, Adam and RMSprop, torch.optim.SGD / Adam / RMSprop semantics, on the flat parameter arena.

Reference: train.py:287-290 builds ``optim.SGD(net.parameters(), lr, momentum, weight_decay, nesterov)``, train.py:331-352
``optim.Adam(net.parameters(), lr, weight_decay)`` or ``optim.RMSprop(net.parameters(), lr, weight_decay, momentum)`` for
--optim adam|rmsprop (with --lr-sched none); ``optimizer.step()`` runs once per batch (train.py:423) and a resumed run loads
``optimizer-state-dict`` (:354-355).  torch runs a step as several multi-tensor kernels over ~140 tensors; here parameters
(UNet._flatten_parameters), gradients (plan.grad_flat) and each state tensor (one arena per state key) share one layout, so a
step is one dfl_sgd_step / dfl_adam_step / dfl_rmsprop_step launch per contiguous run of live parameters whose step counts are
equal (two runs for the paper network: the never-used ``downsample_convs[depth-1]`` has no gradient and, exactly as in torch, is
skipped -- no weight decay either), or -- when the network has a training plan with tiled weight layouts -- one
dfl_sgd_pack_tiled / dfl_optim_pack_tiled launch that updates every parameter inside the next step's weight re-layout.
Parameters whose tensors do not line up (foreign modules, accumulated gradients) are updated tensor by tensor with the same
kernel.  State is torch's, key for key (Adam and RMSprop: with a CPU float32 ``step`` per parameter), only for parameters that
received a gradient, so checkpoints move between these classes and torch.optim in both directions.  Adam and RMSprop differ from
torch's multi-tensor kernels by fp32 rounding only.  CPU tensors are refused: there is no fallback path.
"""
import ctypes as C
import math
import os
import weakref

import numpy as np
import torch
from torch.optim.optimizer import Optimizer, _get_scalar_dtype, required

from . import _native as nat


class _ArenaOptimizer(Optimizer):
    """What SGD, Adam and RMSprop share: state arenas, contiguous runs, the update inside the tiled re-layout."""
    FUSE_PACK = os.environ.get('DFL_SGD_PACK', '1') != '0'   # 0: no update inside the re-layout, for every optimizer
    NAME = ''
    REFUSED = ()                       # group flags no reference command line selects: (key, value that is refused)
    KEEPS_STEP = True                  # keeps torch's per-parameter 'step' tensor

    def __init__(self, params, defaults):
        for k, bad in self.REFUSED:
            if defaults[k] == bad:
                raise NotImplementedError('%s: %s=%r is not implemented in the HIP path (no reference command line selects it)'
                                          % (self.NAME, k, bad))
        super().__init__(params, defaults)
        self._lib = nat.lib()
        self._fused_cache = {}         # tiled job lists, see tiled_job_list

    # ---- per optimizer
    def _state_keys(self, group):
        raise NotImplementedError

    def _pads_ok(self, group):
        """Whether an update may run across the alignment padding between slices (merged runs, the plain jobs of the tiled
        update).  Adam and RMSprop: only when eps > 0, otherwise they would write 0/0 there."""
        return group['eps'] > 0

    def _launch_run(self, lib, group, t, pp, gp, sp, n, stream):
        raise NotImplementedError

    def _launch_tiled(self, lib, group, t, jobs, deltas, stream):
        """`jobs`: the job fields of the pack-args struct; `deltas`: element deltas of the state arenas to the parameters."""
        raise NotImplementedError

    # ---- state
    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            for k, v in self.defaults.items():
                if k != 'params':
                    group.setdefault(k, v)
            for p in group['params']:       # (old checkpoints keep the step count as a number, as torch.optim does)
                st = self.state.get(p, {})
                if self.KEEPS_STEP and len(st) != 0 and not torch.is_tensor(st.get('step')):
                    st['step'] = torch.tensor(float(st.get('step', 0)), dtype=_get_scalar_dtype())

    @staticmethod
    def _arena_layout(ps):
        """(base address, elements) of an arena laid out like the parameters `ps`, or None when they do not share one."""
        if not ps or not all(p.is_cuda and p.dtype == torch.float32 for p in ps) or len({p.device for p in ps}) != 1:
            return None
        base = min(p.data_ptr() for p in ps)
        end = max(p.data_ptr() + 4 * p.numel() for p in ps)
        span = (end - base) // 4
        if span > sum(p.numel() for p in ps) + 4 * len(ps):
            return None
        return base, span

    def _init_state(self, group):
        """torch's state for parameters that have a gradient and no state yet (zero tensors, step 0).  When the whole group is
        new and its parameters share one arena, each state key gets one arena with the same layout."""
        keys = self._state_keys(group)
        ps = [p for p in group['params'] if p.grad is not None and len(self.state.get(p, {})) == 0]
        if not ps or not (keys or self.KEEPS_STEP):
            return
        fresh = all(len(self.state.get(p, {})) == 0 for p in group['params'])
        lay = self._arena_layout(group['params']) if fresh else None
        flats = {k: torch.zeros(lay[1], dtype=torch.float32, device=ps[0].device) for k in keys} if lay else None
        for p in ps:                          # like torch: only parameters that received a gradient get state
            st = self.state[p]
            if self.KEEPS_STEP:
                st['step'] = torch.tensor(0.0, dtype=_get_scalar_dtype())
            for k in keys:
                if flats is not None:
                    o = (p.data_ptr() - lay[0]) // 4
                    st[k] = flats[k][o:o + p.numel()].view(p.shape)
                else:
                    st[k] = torch.zeros_like(p, memory_format=torch.preserve_format)

    def load_state_dict(self, state_dict):
        """torch restores every state tensor as a tensor of its own; put each state key back into one arena laid out like the
        parameters, so that a resumed run keeps the one-launch-per-run update (otherwise: one launch per tensor)."""
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            lay = self._arena_layout(group['params'])
            if lay is None:
                continue
            for k in self._state_keys(group):
                have = [p for p in group['params'] if torch.is_tensor(self.state.get(p, {}).get(k))]
                if not have:
                    continue
                flat = torch.zeros(lay[1], dtype=torch.float32, device=have[0].device)
                with torch.no_grad():
                    for p in have:
                        o = (p.data_ptr() - lay[0]) // 4
                        view = flat[o:o + p.numel()].view(p.shape)
                        view.copy_(self.state[p][k])
                        self.state[p][k] = view

    # ---- step
    def _fused(self, group, net, live, runs):
        """(plan, job fields, state deltas) of an update inside the tiled re-layout, or None: every live parameter at one step
        count, every tiled parameter live, gradients and state tensors laid out like the parameters (one delta each)."""
        if net is None or not self.FUSE_PACK or len(self.param_groups) != 1 or len({r[3] for r in runs}) != 1 \
                or not self._pads_ok(group):
            return None
        plan = net.plan_for_fused_update()
        if plan is None:
            return None
        deltas = []
        for j in range(len(runs[0][1])):
            d = {r[1][j] - r[0] for r in runs}
            if len(d) != 1:
                return None
            deltas.append(d.pop())
        if any(d % 16 for d in deltas):
            return None
        key = (id(plan),) + tuple(deltas) + tuple(p.data_ptr() for p in live)
        jl = tiled_job_list(self._fused_cache, net, plan, live, key)
        if jl is None:
            return None
        jobs_dev, njobs, tiles = jl
        jobs = dict(jobs_dev=jobs_dev.data_ptr(), njobs=njobs, total_tiles=tiles, grad_delta=deltas[0] // 4)
        return plan, jobs, [d // 4 for d in deltas[1:]]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = self._lib
        for group in self.param_groups:
            for k, bad in self.REFUSED:
                if group.get(k) == bad:
                    raise NotImplementedError('%s: %s=%r is not implemented in the HIP path (no reference command line selects it)'
                                              % (self.NAME, k, bad))
            live = [p for p in group['params'] if p.grad is not None]
            if not live:
                continue
            for p in live:
                if not p.is_cuda or not p.grad.is_cuda:
                    raise nat.DflError('%s needs parameters and gradients on the GPU (no CPU path)' % self.NAME)
                if p.dtype != torch.float32 or p.grad.dtype != torch.float32 or not p.grad.is_contiguous() or not p.is_contiguous():
                    raise nat.DflError('%s needs contiguous float32 parameters and gradients' % self.NAME)
            self._init_state(group)
            keys = self._state_keys(group)
            counts = [None] * len(live)
            if self.KEEPS_STEP:
                steps = [self.state[p]['step'] for p in live]
                torch._foreach_add_(steps, 1.0)   # torch's per-parameter step counts (CPU float32 scalars)
                counts = torch.stack([s.detach().to('cpu', torch.float64) for s in steps]).tolist()
            stream = torch.cuda.current_stream(live[0].device).cuda_stream
            # contiguous runs: parameter, gradient and state addresses all advance by the same number of bytes, one step count
            gap = 12 if self._pads_ok(group) else 0
            runs, cur = [], None
            for p, t in zip(live, counts):
                pp, n = p.data_ptr(), p.numel()
                other = (p.grad.data_ptr(),) + tuple(self.state[p][k].data_ptr() for k in keys)
                if cur is not None and t == cur[3] and all(o - c == pp - cur[0] for o, c in zip(other, cur[1])) \
                        and 0 <= pp - cur[0] - 4 * cur[2] <= gap:
                    cur[2] = (pp - cur[0]) // 4 + n          # absorbs the alignment padding between slices
                else:
                    cur = [pp, other, n, t]
                    runs.append(cur)
            from .unet import owner_of
            net = owner_of(live[0])
            fused = self._fused(group, net, live, runs)
            if fused is not None:
                # one pass over the weights: the workgroups of the tiled re-layout update their tile first
                plan, jobs, deltas = fused
                self._launch_tiled(lib, group, runs[0][3], jobs, deltas, stream)
            else:
                for pp, other, n, t in runs:
                    self._launch_run(lib, group, t, pp, other[0], other[1:], n, stream)
            # the kernel wrote behind autograd's back: bump the version counters like an in-place torch op would (the
            # network re-packs its weights when they move, and autograd must see saved tensors as modified)
            torch.autograd.graph.increment_version(live)
            if fused is not None:
                net.after_fused_update(plan, stream)
            elif net is not None:
                net.prepack()            # next step's weight re-layout starts now, behind the update kernels
        return loss


def tiled_job_list(cache, net, plan, live, key):
    """(device job list, jobs, tiles) of an update inside the tiled weight re-layout of `plan` (dfl_sgd_pack_tiled,
    dfl_optim_pack_tiled), or None: every tiled parameter must be among `live`.  The tiled jobs of the plan, then one
    DFL_PACK_PLAIN job per stretch of the other live parameters.  Cached in `cache` under `key` while `plan` lives."""
    hit = cache.get(key)
    if hit is not None and hit[0]() is plan:
        return hit[1:]
    raw, ntiled, tiles, tiled_src = plan._tiled_host
    ptrs = {p.data_ptr(): p.numel() for p in live}
    if any(ptrs.get(s) != n for s, n in tiled_src.items()):
        return None                      # a tiled parameter without a gradient (or a view of one): not this path
    plain, cur = [], None                # what has no tiled layout, adjacent slices merged (alignment padding absorbed)
    flat = getattr(net, '_param_flat', None)
    lo = flat.data_ptr() if flat is not None else 0
    hi = lo + 4 * flat.numel() if flat is not None else 0

    def in_arena(ptr):                   # only slices of the network's own flat arena are merged across a gap
        return lo <= ptr < hi
    for p in live:
        pp, n = p.data_ptr(), p.numel()
        if pp in tiled_src:
            cur = None
            continue
        if cur is not None and 0 <= pp - cur[0] - 4 * cur[1] <= 12 and in_arena(cur[0]) and in_arena(pp):
            cur[1] = (pp - cur[0]) // 4 + n          # (the gap is the arena's alignment padding: nobody else's memory)
        else:
            cur = [pp, n]
            plain.append(cur)
    arr = (nat.PackJob * (ntiled + len(plain)))()
    C.memmove(arr, raw, len(raw))
    for i, (pp, n) in enumerate(plain):
        a = arr[ntiled + i]
        a.src, a.A, a.B, a.C, a.kind, a.first_tile = pp, n, 1, 1, nat.PACK_PLAIN, tiles
        tiles += -(-n // nat.SGD_PLAIN_TILE)
    jobs_dev = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).to(live[0].device)
    if len(cache) >= 4:
        cache.clear()
    cache[key] = (weakref.ref(plan), jobs_dev, len(arr), tiles)
    return cache[key][1:]


def _number(x, what):
    if torch.is_tensor(x):
        raise NotImplementedError('%s as a Tensor is not implemented in the HIP path (capturable use only)' % what)
    return x


class SGD(_ArenaOptimizer):
    """torch.optim.SGD with momentum / Nesterov / weight decay (dampening refused)."""
    NAME = 'optim.SGD'
    KEEPS_STEP = False                 # (torch's SGD keeps no step count)

    def __init__(self, params, lr=required, momentum=0, dampening=0, weight_decay=0, nesterov=False):
        if lr is not required and lr < 0.0:
            raise ValueError('Invalid learning rate: {}'.format(lr))
        if momentum < 0.0:
            raise ValueError('Invalid momentum value: {}'.format(momentum))
        if weight_decay < 0.0:
            raise ValueError('Invalid weight_decay value: {}'.format(weight_decay))
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
        if dampening != 0:
            raise NotImplementedError('dampening != 0 is not implemented in the HIP path (no reference CLI selects it)')
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov)
        super().__init__(params, defaults)

    def _state_keys(self, group):
        return ('momentum_buffer',) if group['momentum'] != 0 else ()

    def _pads_ok(self, group):
        return True

    def _launch_run(self, lib, group, t, pp, gp, sp, n, stream):
        nat.check(lib.dfl_sgd_step(pp, gp, sp[0] if sp else None, n, group['lr'], group['momentum'], group['weight_decay'], 1.0,
                                   int(group['nesterov']), 0, stream), 'dfl_sgd_step')

    def _launch_tiled(self, lib, group, t, jobs, deltas, stream):
        a = nat.SgdPackArgs(buf_delta=deltas[0] if deltas else 0, lr=group['lr'], momentum=group['momentum'],
                            weight_decay=group['weight_decay'], grad_scale=1.0, nesterov=int(group['nesterov']), **jobs)
        nat.check(lib.dfl_sgd_pack_tiled(C.addressof(a), stream), 'dfl_sgd_pack_tiled')


class Adam(_ArenaOptimizer):
    """torch.optim.Adam (amsgrad, maximize, capturable, differentiable, fused and decoupled weight decay refused)."""
    NAME = 'optim.Adam'
    REFUSED = (('amsgrad', True), ('maximize', True), ('capturable', True), ('differentiable', True), ('fused', True),
               ('decoupled_weight_decay', True))

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        lr = _number(lr, 'lr')
        betas = (_number(betas[0], 'betas[0]'), _number(betas[1], 'betas[1]'))
        if not 0.0 <= lr:
            raise ValueError('Invalid learning rate: {}'.format(lr))
        if not 0.0 <= eps:
            raise ValueError('Invalid epsilon value: {}'.format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError('Invalid beta parameter at index 0: {}'.format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError('Invalid beta parameter at index 1: {}'.format(betas[1]))
        if not 0.0 <= weight_decay:
            raise ValueError('Invalid weight_decay value: {}'.format(weight_decay))
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                        capturable=capturable, differentiable=differentiable, fused=fused,
                        decoupled_weight_decay=decoupled_weight_decay)
        super().__init__(params, defaults)

    def _state_keys(self, group):
        return ('exp_avg', 'exp_avg_sq')

    @staticmethod
    def _coefs(group, t):
        """step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t), in double as torch computes them."""
        b1, b2 = group['betas']
        return group['lr'] / (1 - b1 ** t), math.sqrt(1 - b2 ** t)

    def _launch_run(self, lib, group, t, pp, gp, sp, n, stream):
        b1, b2 = group['betas']
        step_size, bc2_sqrt = self._coefs(group, t)
        nat.check(lib.dfl_adam_step(pp, gp, sp[0], sp[1], n, group['lr'], b1, b2, group['eps'], group['weight_decay'], step_size,
                                    bc2_sqrt, 1.0, stream), 'dfl_adam_step')

    def _launch_tiled(self, lib, group, t, jobs, deltas, stream):
        b1, b2 = group['betas']
        step_size, bc2_sqrt = self._coefs(group, t)
        a = nat.OptimPackArgs(kind=nat.OPTIM_ADAM, state1_delta=deltas[0], state2_delta=deltas[1], lr=group['lr'], eps=group['eps'],
                              weight_decay=group['weight_decay'], grad_scale=1.0, beta1=b1, beta2=b2, step_size=step_size,
                              bc2_sqrt=bc2_sqrt, **jobs)
        nat.check(lib.dfl_optim_pack_tiled(C.addressof(a), stream), 'dfl_optim_pack_tiled')


class RMSprop(_ArenaOptimizer):
    """torch.optim.RMSprop (centered, maximize, capturable and differentiable refused)."""
    NAME = 'optim.RMSprop'
    REFUSED = (('centered', True), ('maximize', True), ('capturable', True), ('differentiable', True))

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False, capturable=False,
                 foreach=None, maximize=False, differentiable=False):
        lr = _number(lr, 'lr')
        if not 0.0 <= lr:
            raise ValueError('Invalid learning rate: {}'.format(lr))
        if not 0.0 <= eps:
            raise ValueError('Invalid epsilon value: {}'.format(eps))
        if not 0.0 <= momentum:
            raise ValueError('Invalid momentum value: {}'.format(momentum))
        if not 0.0 <= weight_decay:
            raise ValueError('Invalid weight_decay value: {}'.format(weight_decay))
        if not 0.0 <= alpha:
            raise ValueError('Invalid alpha value: {}'.format(alpha))
        defaults = dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=centered, weight_decay=weight_decay,
                        capturable=capturable, foreach=foreach, maximize=maximize, differentiable=differentiable)
        super().__init__(params, defaults)

    def _state_keys(self, group):
        return ('square_avg', 'momentum_buffer') if group['momentum'] > 0 else ('square_avg',)

    def _launch_run(self, lib, group, t, pp, gp, sp, n, stream):
        nat.check(lib.dfl_rmsprop_step(pp, gp, sp[0], sp[1] if len(sp) > 1 else None, n, group['lr'], group['alpha'], group['eps'],
                                       group['weight_decay'], group['momentum'], 1.0, stream), 'dfl_rmsprop_step')

    def _launch_tiled(self, lib, group, t, jobs, deltas, stream):
        a = nat.OptimPackArgs(kind=nat.OPTIM_RMSPROP, state1_delta=deltas[0], state2_delta=deltas[1] if len(deltas) > 1 else 0,
                              lr=group['lr'], eps=group['eps'], weight_decay=group['weight_decay'], grad_scale=1.0,
                              alpha=group['alpha'], momentum=group['momentum'], **jobs)
        nat.check(lib.dfl_optim_pack_tiled(C.addressof(a), stream), 'dfl_optim_pack_tiled')
