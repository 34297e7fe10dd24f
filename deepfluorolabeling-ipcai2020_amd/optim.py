"""Adam and RMSprop, torch.optim.Adam / torch.optim.RMSprop semantics, on the flat parameter arena.

Reference: train.py:331-352 builds ``optim.Adam(net.parameters(), lr, weight_decay)`` or ``optim.RMSprop(net.parameters(), lr,
weight_decay, momentum)`` for --optim adam|rmsprop (with --lr-sched none) and loads ``optimizer-state-dict`` into it on resume
(:354-355).  The design is sgd.SGD's: parameters (UNet._flatten_parameters), gradients (plan.grad_flat) and each state tensor
(one arena per state key) share one layout, so a step is one dfl_adam_step / dfl_rmsprop_step launch per contiguous run of live
parameters whose step counts are equal (two runs for the paper network), or -- when the network has a training plan with tiled
weight layouts -- one dfl_optim_pack_tiled launch that updates every parameter inside the next step's weight re-layout.
State is torch's, key for key: a CPU float32 ``step`` per parameter and fp32 tensors, only for parameters that received a
gradient, so checkpoints move between this class and torch.optim in both directions.  Results differ from torch's
multi-tensor kernels by fp32 rounding only.  CPU tensors are refused: there is no fallback path.
"""
import ctypes as C
import math

import torch
from torch.optim.optimizer import Optimizer, _get_scalar_dtype

from . import _native as nat
from .sgd import SGD, tiled_job_list


class _ArenaOptimizer(Optimizer):
    """What Adam and RMSprop share: state arenas, contiguous runs, the update inside the tiled re-layout."""
    FUSE_PACK = SGD.FUSE_PACK          # DFL_SGD_PACK=0 switches the update inside the re-layout off for every optimizer
    NAME = ''
    REFUSED = ()                       # group flags no reference command line selects: (key, value that is refused)

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self.grad_scale = 1.0          # parallel.DataParallel leaves SUMMED gradients when asked to; see sgd.SGD
        self._lib = nat.lib()
        self._fused_cache = {}         # tiled job lists, see sgd.tiled_job_list

    # ---- per optimizer
    def _state_keys(self, group):
        raise NotImplementedError

    def _launch_run(self, lib, group, t, pp, gp, sp, n, stream):
        raise NotImplementedError

    def _pack_args(self, group, t):
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
                if len(st) != 0 and not torch.is_tensor(st.get('step')):
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
        ps = [p for p in group['params'] if p.grad is not None and len(self.state.get(p, {})) == 0]
        if not ps:
            return
        keys = self._state_keys(group)
        fresh = all(len(self.state.get(p, {})) == 0 for p in group['params'])
        lay = self._arena_layout(group['params']) if fresh else None
        flats = {k: torch.zeros(lay[1], dtype=torch.float32, device=ps[0].device) for k in keys} if lay else None
        for p in ps:                          # like torch: only parameters that received a gradient get state
            st = self.state[p]
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
    def _fused(self, group, net, live, runs, keys):
        """(plan, device job list, jobs, tiles, deltas) for dfl_optim_pack_tiled, or None: every live parameter at one step
        count, every tiled parameter live, gradients and state tensors laid out like the parameters (one delta each)."""
        if net is None or not self.FUSE_PACK or len(self.param_groups) != 1 or len({r[3] for r in runs}) != 1 or group['eps'] <= 0:
            return None                       # (eps = 0: the plain jobs would write 0/0 into the arena's alignment padding)
        plan = net.plan_for_fused_update()
        if plan is None:
            return None
        deltas = []
        for j in range(1 + len(keys)):
            d = {r[1][j] - r[0] for r in runs}
            if len(d) != 1:
                return None
            deltas.append(d.pop())
        if any(d % 16 for d in deltas):
            return None
        key = (id(plan), type(self).__name__) + tuple(deltas) + tuple(p.data_ptr() for p in live)
        jl = tiled_job_list(self._fused_cache, net, plan, live, key)
        if jl is None:
            return None
        return (plan,) + jl + tuple(d // 4 for d in deltas)

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
            steps = [self.state[p]['step'] for p in live]
            torch._foreach_add_(steps, 1.0)   # torch's per-parameter step counts (CPU float32 scalars)
            counts = torch.stack([s.detach().to('cpu', torch.float64) for s in steps]).tolist()
            stream = torch.cuda.current_stream(live[0].device).cuda_stream
            # contiguous runs: parameter, gradient and state addresses all advance by the same number of bytes, one step count
            gap = 12 if group['eps'] > 0 else 0
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
            fused = self._fused(group, net, live, runs, keys)
            if fused is not None:
                # one pass over the weights: the workgroups of the tiled re-layout update their tile first
                plan, jobs_dev, njobs, tiles = fused[:4]
                a = self._pack_args(group, runs[0][3])
                a.jobs_dev, a.njobs, a.total_tiles, a.grad_delta, a.state1_delta = jobs_dev.data_ptr(), njobs, tiles, fused[4], fused[5]
                a.state2_delta = fused[6] if len(fused) > 6 else 0
                a.grad_scale = self.grad_scale
                nat.check(lib.dfl_optim_pack_tiled(C.addressof(a), stream), 'dfl_optim_pack_tiled')
                torch.autograd.graph.increment_version(live)
                net.after_fused_update(plan, stream)
                continue
            for pp, other, n, t in runs:
                self._launch_run(lib, group, t, pp, other[0], other[1:], n, stream)
            # the kernel wrote behind autograd's back: bump the version counters like an in-place torch op would
            torch.autograd.graph.increment_version(live)
            if net is not None:
                net.prepack()            # next step's weight re-layout starts now, behind the update kernels
        return loss


def _number(x, what):
    if torch.is_tensor(x):
        raise NotImplementedError('%s as a Tensor is not implemented in the HIP path (capturable use only)' % what)
    return x


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
        for k, bad in self.REFUSED:
            if defaults[k] == bad:
                raise NotImplementedError('%s: %s=%r is not implemented in the HIP path (no reference command line selects it)'
                                          % (self.NAME, k, bad))
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
                                    bc2_sqrt, self.grad_scale, stream), 'dfl_adam_step')

    def _pack_args(self, group, t):
        b1, b2 = group['betas']
        step_size, bc2_sqrt = self._coefs(group, t)
        return nat.OptimPackArgs(kind=nat.OPTIM_ADAM, lr=group['lr'], eps=group['eps'], weight_decay=group['weight_decay'],
                                 beta1=b1, beta2=b2, step_size=step_size, bc2_sqrt=bc2_sqrt)


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
        for k, bad in self.REFUSED:
            if defaults[k] == bad:
                raise NotImplementedError('%s: %s=%r is not implemented in the HIP path (no reference command line selects it)'
                                          % (self.NAME, k, bad))
        super().__init__(params, defaults)

    def _state_keys(self, group):
        return ('square_avg', 'momentum_buffer') if group['momentum'] > 0 else ('square_avg',)

    def _launch_run(self, lib, group, t, pp, gp, sp, n, stream):
        nat.check(lib.dfl_rmsprop_step(pp, gp, sp[0], sp[1] if len(sp) > 1 else None, n, group['lr'], group['alpha'], group['eps'],
                                       group['weight_decay'], group['momentum'], self.grad_scale, stream), 'dfl_rmsprop_step')

    def _pack_args(self, group, t):
        return nat.OptimPackArgs(kind=nat.OPTIM_RMSPROP, lr=group['lr'], eps=group['eps'], weight_decay=group['weight_decay'],
                                 alpha=group['alpha'], momentum=group['momentum'])
