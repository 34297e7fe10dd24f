"""Execution plans for the U-Net: the graph builder that turns one (architecture, input shape, mode) into recorded
lists of libdfl_hip.so calls (forward, backward, weight re-layout) plus the HBM buffers they run on.

Reference being restated: UNet.forward / UNetConvBlock.forward / UNetUpBlock.forward
(train_test_code/unet.py:161-193, 226-233, 254-260) and their autograd.  Data layout: every internal activation
is NHWC fp32; torch.cat([up, bridge], 1) (unet.py:257) is free because both producers write straight into the two
channel halves of one buffer (pixel stride 2C); BatchNorm is never applied as a separate pass -- its scale/shift
ride on the next consumer's loads (see include/dfl_hip.h).

UNetPlan._build records in the order of the network: _levels (sizes, PlanError checks), _alloc_buffers, _down_forward and
_up_forward (one _block_forward per UNetConvBlock), _heads_forward; with gradients then _grad_arena, _heads_backward (the
landmark block included), _up_backward and _down_backward (one _block_backward per block, last block first; per layer the
BatchNorm-backward coefficients, then the gradient launches); last the pack program (_finish_pack) and _grad_ready_ops.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _native as nat
from ._native import (ConvArgs, WgradArgs, PackJob, BnFinalizeArgs, ColstatsArgs, BnBwdFinalizeArgs, BnReluBwdArgs,
                      AffineCopyArgs, PoolArgs, HeadFwdArgs, HeadBwdArgs, PackArgs, BnEvalArgs, UpsampleArgs, BnLiveJob, BnLiveArgs,
                      BnBwdLiveJob, BnBwdLiveArgs, MemsetArgs, ReduceJob, ReduceBatchArgs, Program)

BN_EPS = 1.0e-5
BN_MOMENTUM = 0.1


class Act:
    """An NHWC activation window: channels [0, C) of rows with pixel stride ld (in elements) starting at ptr; esz = bytes
    per element (4: fp32; 2: bf16 tensors of math mode 4)."""
    __slots__ = ('t', 'ptr', 'ld', 'N', 'H', 'W', 'C', 'esz')

    def __init__(self, t, ptr, ld, N, H, W, C, esz=4):
        self.t, self.ptr, self.ld, self.N, self.H, self.W, self.C, self.esz = t, ptr, ld, N, H, W, C, esz

    @property
    def M(self):
        return self.N * self.H * self.W

    @property
    def bf16(self):
        return int(self.esz == 2)

    def chan_slice(self, c0, c):
        return Act(self.t, self.ptr + self.esz * c0, self.ld, self.N, self.H, self.W, c, self.esz)


class PlanError(RuntimeError):
    pass


def _span(a):
    """Bytes an op touches through Act a: (first, end, row pitch, row width), pitch 0 = one dense run."""
    pitch, width = a.ld * a.esz, a.C * a.esz
    return (a.ptr, a.ptr + (a.M - 1) * pitch + width, pitch if width < pitch else 0, width)


def _flat(ptr, nbytes):
    return (int(ptr), int(ptr) + int(nbytes), 0, int(nbytes))


def _spans_meet(a, b):
    if a[0] >= b[1] or b[0] >= a[1]:
        return False
    if a[2] and a[2] == b[2]:                      # two channel windows of rows with one pitch (the halves of a concat buffer)
        off = (a[0] - b[0]) % a[2]
        return off < b[3] or off + a[3] > a[2]
    return True


class _Fork:
    """Dependency tracker of a forked program: ops of the main chain on stream 0, branch ops on one side stream.

    A branch op starts behind the main chain as it stands where the op is emitted (RECORD on the main chain, WAIT on the
    branch): it sees what the serial program showed it, so only the other direction needs bookkeeping.  Every branch op is
    followed by a RECORD of its own; a later main-chain op that writes what a pending branch op reads or writes, or reads
    what it writes, is given a WAIT for that op's event (and with it for every earlier branch op: one stream).  A main-chain
    op whose accesses are not declared (reads is None) waits for the whole branch.  Spans are (first, end, pitch, width)."""
    BRANCH = 1

    def __init__(self, prog):
        self.prog = prog
        self.pending = []           # (event, reads, writes) of the branch ops the main chain is not ordered behind, oldest first
        self.events = 0
        self.at_main = None         # event recorded behind the main chain's latest op
        self.seen = 0               # ops emitted through the tracker
        self.waits = 0              # WAITs given to the main chain

    def main(self, reads, writes):
        """In front of a main-chain op."""
        hit = -1
        for k, (_, r, w) in enumerate(self.pending):
            if reads is None or any(_spans_meet(x, y) for x in writes for y in r + w) or any(_spans_meet(x, y) for x in reads for y in w):
                hit = k
        if hit >= 0:
            self.prog.wait(self.pending[hit][0], 0)
            self.waits += 1
            del self.pending[:hit + 1]
        self.at_main = None
        self.seen += 1

    def fork(self):
        """In front of a branch op."""
        if self.at_main is None:
            self.at_main = self.events
            self.events += 1
            self.prog.record(self.at_main, 0)
            self.prog.wait(self.at_main, self.BRANCH)
        self.seen += 1

    def forked(self, reads, writes):
        """Behind the branch op just added."""
        self.prog.record(self.events, self.BRANCH)
        self.pending.append((self.events, list(reads), list(writes)))
        self.events += 1


# Diagnosis (tests/test_gpu_bf16_stepwise.py): plans built while this is True give every activation gradient its own buffer
# instead of the three shared scratch tensors, so that all of them can be read after a backward pass (UNetPlan.dbg names them).
KEEP_GRADS = False


class _Layer:
    """One 3x3 convolution of a block as its backward sees it (UNetPlan._block_forward)."""
    __slots__ = ('w', 'wname', 'relu', 'inp', 'gin', 'inp_aff', 'r', 'bn', 'live_bwd')

    def __init__(self, w, wname, relu, inp, gin, inp_aff, r, bn, live_bwd):
        # w / wname: the weight and its parameter prefix; relu: module name of the nn.ReLU behind it; inp: the input Act,
        # gin: what the convolution gathers from (inp, or its wrapped copy); inp_aff: BatchNorm (scale, shift) applied on
        # load; r: the saved ReLU output; bn: (gamma, mean, invstd, name) of the BatchNorm behind it, or None; live_bwd:
        # its backward takes live (sum dy, sum dy*r) totals
        self.w, self.wname, self.relu, self.inp, self.gin, self.inp_aff = w, wname, relu, inp, gin, inp_aff
        self.r, self.bn, self.live_bwd = r, bn, live_bwd


class _Block:
    """What the backward of one UNetConvBlock needs from its forward."""
    __slots__ = ('prefix', 'xin', 'out', 'convs', 'rw', 'last_r', 'last_live')

    def __init__(self, prefix, xin, out):
        self.prefix, self.xin, self.out = prefix, xin, out
        self.convs = []           # _Layer per 3x3 convolution, in forward order
        self.rw = None            # residual 1x1 weight (do_res)
        self.last_r = None        # saved ReLU output of the last layer if a BatchNorm follows it: the producer of dout leaves sums for it
        self.last_live = False    # ... and may leave them as live totals


class UNetPlan:
    # Switches: the DFL_* environment knobs are read once, at import; tests flip LIVE_BN, LIVE_HEAD and DPRE_OUT_BYTES.
    FUSE_BRB = os.environ.get('DFL_FUSE_BRB', '1') != '0'         # BatchNorm + ReLU backward inside the weight-/data-gradient staging (bf16 storage)
    FUSE_DOWN_STATS = os.environ.get('DFL_FUSE_DOWN_STATS', '1') != '0'   # ... and BN-backward sums from the strided-conv data gradient's scatter
    FLUSH_BYTES = int(float(os.environ.get('DFL_FLUSH_MB', '16')) * (1 << 20))   # queued sums flushed from here (4 / 16 / 64 MB: 0.414 / 0.373 / 0.367 ms per step)
    DPRE_OUT_BYTES = int(float(os.environ.get('DFL_DPRE_OUT_MB', '12')) * (1 << 20))   # data gradient also writes the operand it forms up to this size
    LIVE_BN = os.environ.get('DFL_LIVE_BN', '1') != '0'           # BatchNorm statistics completed by their consumers (live totals)
    LIVE_HEAD = os.environ.get('DFL_LIVE_HEAD', '1') != '0'       # ... and the head's backward kernel adds the sums of its dx itself (no colstats pass)
    # Forked backward: weight gradients and the batched sums run on a branch (dfl_op.stream 1) beside the data-gradient chain,
    # ordered by the _Fork tracker; 0 = the serial program, op for op what it was before the fork existed (tests flip FORK)
    FORK = os.environ.get('DFL_FORK', '1') != '0'
    FORK_RING = max(1, int(os.environ.get('DFL_FORK_RING', '2')))   # slots per backward scratch tensor of a forked program
    BN_R = nat.BN_R

    def __init__(self, cfg, params, buffers, N, H, W, training, need_grad, device, input_grad=False):
        """cfg: dict of the UNet constructor flags; params / buffers: name -> tensor (module state)."""
        self.cfg = cfg
        self.P = params
        self.Bf = buffers
        self.N, self.H, self.W = N, H, W
        self.training = training
        self.need_grad = need_grad
        self.input_grad = bool(input_grad and need_grad)    # d(loss)/d(input) as well (nn.Module semantics; no reference script asks)
        self.dx_in = None
        self.dev = device
        self.lib = nat.lib()
        self._keep = []
        self.fwd = Program()
        self.bwd = Program() if need_grad else None
        self._prep = Program()          # eval-mode BatchNorm scale / shift of an inference plan: part of its pack program
        self._pack_jobs = []
        self.busy = False
        self.graph = None               # hipGraph of the forward program (inference plans, captured on first use)
        self.generation = 0
        self._scratch = {}
        self._red_pending = []          # deferred sums (src, dst, n, stride, count), see _defer_sum
        self._red_bytes = 0
        self._red_flushes = []          # (index of the batch op in bwd, [dst pointers])
        self.partial_sum_bytes = 0      # bytes of fp32 partial sums the batched reductions of one backward pass read
        self._tiled_host = self._tiled_index = None     # the tiled pack launch, for optim.py (see _finish_pack)
        self.math = self.lib.dfl_get_math_mode()   # product arithmetic the plan is recorded for (split operand formats)
        # math mode 4, "bf16 storage": internal activations, their gradients and the GEMM copies of the weights are bf16
        # tensors (BASELINE configs[1] as named); statistics, losses, master weights and weight gradients stay fp32
        self.bf16 = self.math == 4
        self.adt = torch.bfloat16 if self.bf16 else torch.float32
        self.aesz = 2 if self.bf16 else 4
        self._packed_split = {}         # packed-weight address -> stored as split quads
        self.relu_out = {}              # nn.ReLU module name -> Act of its output (saved for backward; introspection for tests)
        self._tot_fwd, self._tot_bwd, self._live_jobs, self._live_bwd_pending = [None, 0], [None, 0], [], []
        self.dbg = {}                   # name -> Act / tensors of intermediate results (introspection for tests, see KEEP_GRADS)
        self.keep_grads = bool(KEEP_GRADS)
        self.pool_in = {}               # level -> Act the max-pool of that level reads
        # inference plans ask for the latency form of the bf16 convolution (include/dfl_hip.h: a hint the library honours for the
        # small problems of a batch-1 forward -- the per-image loops of util.py -- and ignores for everything else)
        self._latency_form = int(not training and not need_grad and os.environ.get('DFL_PLAN_LATENCY_FORM', '1') != '0')
        self._deps = _Fork(self.bwd) if (self.FORK and need_grad) else None      # the forward and the inference plans stay serial
        self._rings = {}                # backward scratch key -> [slots, next turn] (forked programs)
        self.host_jobs = {}             # device address of an uploaded job array -> the ctypes array (hazard checks read it)
        self._build()

    # ------------------------------------------------------------------------------------------ memory
    def _new(self, nelem, dtype=torch.float32):
        t = torch.empty(max(int(nelem), 1), dtype=dtype, device=self.dev)
        self._keep.append(t)
        return t

    def _const(self, n, value):
        """A plan-owned constant vector (shared per (length, value))."""
        key = ('const', int(n), float(value))
        t = self._scratch.get(key)
        if t is None:
            t = torch.full((int(n),), float(value), dtype=torch.float32, device=self.dev)
            self._keep.append(t)
            self._scratch[key] = t
        return t

    def _act(self, N, H, W, C):
        t = self._new(N * H * W * C, self.adt)
        return Act(t, t.data_ptr(), C, N, H, W, C, self.aesz)

    def _scratch_act(self, key, N, H, W, C):
        """Backward scratch shared by all blocks (stream order makes reuse safe)."""
        need = N * H * W * C
        t = self._scratch.get(key)
        if t is None or t.numel() < need:
            raise PlanError('scratch %s not sized' % key)
        if self.keep_grads:
            return self._act(N, H, W, C)
        if self._deps is not None:
            # forked program: a branch op (weight gradient) still reads the tensor handed out here when the main chain asks for
            # this key again -- it gets the next slot of a ring, so the WAIT the tracker gives its writer is for a branch op that is
            # FORK_RING uses back and has long finished: ordered by slack, not by a stall
            ring = self._rings.setdefault(key, [[t], 0])
            if len(ring[0]) < self.FORK_RING and ring[1] >= len(ring[0]):
                ring[0].append(self._new(t.numel(), t.dtype))
            t = ring[0][ring[1] % len(ring[0])]
            ring[1] = (ring[1] + 1) % self.FORK_RING
        return Act(t, t.data_ptr(), C, N, H, W, C, self.aesz)

    def _is_scratch(self, t, key):
        """t is (a ring slot of) the backward scratch tensor `key`."""
        return t is self._scratch.get(key) or any(t is s for s in self._rings.get(key, [[]])[0])

    # ------------------------------------------------------------------------------------------ weights
    def _pack(self, w, kind, flip=0):
        """Register a re-layout job of parameter w = [A][B][KH][KW] into the quad-packed GEMM operand dfl_conv2d reads
        (include/dfl_hip.h, dfl_pack_job); returns the destination tensor."""
        A, B, KH, KW = w.shape
        Cc = KH * KW
        K = {1: Cc * B, 2: Cc * A, 3: A}[kind]
        N = {1: A, 2: B, 3: Cc * B}[kind]
        cin = B if kind == 1 else A
        if self.bf16 and cin % 16 == 0:
            # bf16 chunk layout [K/16][N][16] of the patch-resident kernels (every layer but the 1-channel first one)
            dst = self._new((K + 15) // 16 * N * 16, torch.bfloat16)
            self._packed_split[dst.data_ptr()] = 2
            self._pack_jobs.append((w, dst, A, B, Cc, kind, flip, 2))
            return dst
        dst = self._new((K + 3) // 4 * N * 4)
        # split quads (hi4 | lo4 bf16) when the consuming conv will take the split-bf16 fast path: its input channels
        # (B for a forward operand, A for the transposed ones) must be a multiple of 16 and K large enough for the GEMM
        split = int(self.math in (1, 3) and cin % 16 == 0)
        self._packed_split[dst.data_ptr()] = split
        self._pack_jobs.append((w, dst, A, B, Cc, kind, flip, split))
        return dst

    def _pack_conv_fwd(self, w):      # Conv2d [Co][Ci][T]: k = (tap, ci), n = co
        return self._pack(w, 1)

    def _pack_conv_dgrad(self, w):    # stride-1 Conv2d data gradient: k = (flipped tap, co), n = ci
        return self._pack(w, 2, flip=1)

    def _pack_down_dgrad(self, w):    # Conv2d(k2,s2) data gradient, scatter form: k = co, n = (ab, ci)
        return self._pack(w, 3)

    def _pack_convT_fwd(self, w):     # ConvTranspose2d [Ci][Co][ab], scatter form: k = ci, n = (ab, co)
        return self._pack(w, 3)

    def _pack_convT_dgrad(self, w):   # ConvTranspose2d data gradient = conv 2x2 s2 over dy: k = (ab, co), n = ci
        return self._pack(w, 1)

    @staticmethod
    def _set_pack_job(a, job):
        """Fill PackJob a from a job of _pack: (src, dst, A, B, C, kind, flip, split)."""
        src, dst, A, B, Cc, kind, flip, split = job
        a.src, a.dst, a.A, a.B, a.C, a.kind, a.flip, a.split = src.data_ptr(), dst.data_ptr(), A, B, Cc, kind, flip, split

    def _upload(self, arr):
        """Address of a device copy of the ctypes array arr, kept alive by the plan."""
        t = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).to(self.dev)
        self._keep.append(t)
        self.host_jobs[t.data_ptr()] = arr
        return t.data_ptr()

    def _emit(self, prog, a, reads=None, writes=None, branch=False, **kw):
        """Add op a to prog and return its index.  In a forked backward program the op goes through the dependency tracker
        with the spans it reads and writes (_span / _flat): on the branch if asked, else on the main chain, behind a WAIT for
        whatever pending branch op it conflicts with -- for all of them if it declares nothing."""
        dep = self._deps if prog is self.bwd else None
        if dep is None:
            prog.add(a, **kw)
        elif branch:
            assert reads is not None and writes is not None, 'a branch op declares what it touches'
            dep.fork()
            prog.add(a, stream=dep.BRANCH, **kw)
            idx = len(prog) - 1
            dep.forked(reads or [], writes or [])
            return idx
        else:
            dep.main(reads, writes)
            prog.add(a, **kw)
        return len(prog) - 1

    def _finish_pack(self):
        """The pack program: the eval-mode BatchNorm prep of an inference plan, then the weight re-layouts.  The layouts of
        parameters that tile into 32 x 32 x C blocks go through dfl_pack_weights_tiled -- a flat list of tiles over all jobs, BOTH
        layouts of a parameter (forward operand and data-gradient operand) from one read of the fp32 master --, everything else
        (the first layer, heads, odd sizes) through dfl_pack_weights."""
        self.pack = Program()
        self.pack.extend(self._prep)
        tiled, rest, by_src = [], [], {}
        for job in self._pack_jobs:
            src, dst, A, B, Cc, kind, flip, split = job
            if A % 32 == 0 and B % 32 == 0 and Cc <= 9:
                k = src.data_ptr()
                if k in by_src and len(by_src[k]) == 1:
                    by_src[k].append(job)
                else:
                    by_src[k] = [job]
                    tiled.append(by_src[k])
            else:
                rest.append(job)
        if tiled:
            arr = (PackJob * len(tiled))()
            tiles = 0
            for a, group in zip(arr, tiled):
                self._set_pack_job(a, group[0])
                if len(group) > 1:
                    a.dst2, a.kind2, a.flip2, a.split2 = group[1][1].data_ptr(), group[1][5], group[1][6], group[1][7]
                a.first_tile = tiles
                tiles += (a.A // 32) * (a.B // 32)
            self._tiled_index = len(self.pack)       # what optim.py needs to update the weights inside this launch
            self.pack.add(PackArgs(jobs_dev=self._upload(arr), max_elems=tiles, njobs=len(tiled), tiled=1))
            srcs = [g[0][0].data_ptr() for g in tiled]
            if len(set(srcs)) == len(srcs):                   # (a parameter with a third layout: its second record would read
                self._tiled_host = (bytes(arr), len(tiled), tiles, {g[0][0].data_ptr(): g[0][0].numel() for g in tiled})   # what the first one writes)
        if rest:                                         # one dfl_pack_weights launch over a flat PackJob array
            arr = (PackJob * len(rest))()
            for a, job in zip(arr, rest):
                self._set_pack_job(a, job)
            mx = max(A * B * Cc for (_, _, A, B, Cc, _, _, _) in rest)
            self.pack.add(PackArgs(jobs_dev=self._upload(arr), max_elems=mx, njobs=len(rest)))

    # ------------------------------------------------------------------------------------------ op helpers
    def _conv(self, prog, x, w, y, KH, KW, stride, pad, Ntot, bias=None, in_aff=None, relu=0, add=None,
              add_aff=None, accumulate=0, scatter=0, stats=False, stat_other=None, Hout=None, Wout=None, x_split=0, brb=None,
              in_live=None, add_live=None, stat_totals=None, x_out=None, out_aff=None):
        """in_live / add_live: (totals, gamma, beta, count) of a live BatchNorm instead of the (scale, shift) vectors of in_aff /
        add_aff; stat_totals: the producer adds its statistics there instead of leaving partial rows (include/dfl_hip.h)."""
        a = ConvArgs()
        a.x, a.w, a.y = x.ptr, w.data_ptr(), y.ptr
        a.w_split = self._packed_split.get(w.data_ptr(), 0)
        a.x_split = x_split
        a.x_bf16, a.y_bf16 = x.bf16, y.bf16
        if (add is not None and add.bf16 != y.bf16) or (stat_other is not None and stat_other.bf16 != y.bf16):
            raise PlanError('internal: mixed element types in a convolution epilogue')
        a.bias = nat.ptr(bias)
        if in_aff is not None:
            a.in_scale, a.in_shift = in_aff[0].data_ptr(), in_aff[1].data_ptr()
        if in_live is not None:
            a.in_tot, a.in_gamma, a.in_beta, a.in_count = in_live[0], in_live[1].data_ptr(), in_live[2].data_ptr(), float(in_live[3])
            a.bn_eps = BN_EPS
        if add_live is not None:
            a.add_tot, a.add_gamma, a.add_beta, a.add_count = add_live[0], add_live[1].data_ptr(), add_live[2].data_ptr(), float(add_live[3])
            a.bn_eps = BN_EPS
        if brb is not None:
            # the operand is the BatchNorm + ReLU backward of (x = dy, r) formed while the patch is staged (dfl_conv_args.x_mode)
            r_act, coef = brb
            a.x_mode, a.x2, a.ldx2 = 1, r_act.ptr, r_act.ld
            if isinstance(coef, dict):               # live statistics: the kernel derives A, B, C from the totals itself
                a.in_tot, a.in_gamma, a.in_mean, a.in_invstd = coef['tot'], coef['gamma'].data_ptr(), coef['mean'].data_ptr(), coef['invstd'].data_ptr()
                a.in_count = float(coef['count'])
            else:
                a.in_scale = nat.ptr(coef)
            if x_out is not None:
                a.x_out, a.ldxo = x_out.ptr, x_out.ld
        if add is not None:
            a.add, a.ldadd = add.ptr, add.ld
            if add_aff is not None:
                a.add_scale, a.add_shift = add_aff[0].data_ptr(), add_aff[1].data_ptr()
        a.N, a.Hin, a.Win, a.Cin, a.ldx = x.N, x.H, x.W, x.C, x.ld
        a.KH, a.KW, a.stride, a.pad = KH, KW, stride, pad
        a.Hout, a.Wout = (y.H, y.W) if Hout is None else (Hout, Wout)
        a.Ntot, a.ldy = Ntot, y.ld
        a.relu, a.accumulate, a.scatter2x2 = relu, accumulate, scatter
        a.latency_form = self._latency_form
        self._out_aff_taken = False
        if out_aff is not None:
            # the consumer's eval-mode BatchNorm applied by this (producing) kernel: only the latency form does that
            a.out_scale, a.out_shift = out_aff[0].data_ptr(), out_aff[1].data_ptr()
            if self.lib.dfl_conv_config(C.addressof(a)) == 16 + nat.CONV_CFG_LATENCY:
                self._out_aff_taken = True
            else:
                a.out_scale, a.out_shift = None, None
        sp = nat.check(self.lib.dfl_conv_suggest_splits(C.addressof(a)), 'dfl_conv_suggest_splits')
        if sp > 1:
            M = x.N * (x.H * x.W if scatter else a.Hout * a.Wout)
            a.splits = sp
            a.partial = self._shared_scratch('conv_partial', sp * M * Ntot).data_ptr()
        partials = None
        if stat_totals is not None:
            a.stat_totals = stat_totals
            if stat_other is not None:
                a.stat_other, a.ldso = stat_other.ptr, stat_other.ld
            partials = ('live', stat_totals)
        elif stats:
            gm = nat.check(self.lib.dfl_conv_grid_m(C.addressof(a)), 'dfl_conv_grid_m')
            partials = self._new(gm * 2 * Ntot)
            a.stat_partials = partials.data_ptr()
            if stat_other is not None:
                a.stat_other, a.ldso = stat_other.ptr, stat_other.ld
            partials = (partials, 4 * gm if scatter else gm)    # scatter2x2: rows = (row block, 2x2 position), Ntot / 4 columns
        if prog is self.bwd and self._deps is not None:
            reads = [_span(t) for t in (x, add, stat_other, brb[0] if brb is not None else None) if t is not None]
            if accumulate:
                reads.append(_span(y))
            writes = [_span(y)] + ([_span(x_out)] if (brb is not None and x_out is not None) else [])
            if a.partial:
                writes.append(_flat(a.partial, 4 * a.splits * x.N * (x.H * x.W if scatter else a.Hout * a.Wout) * Ntot))
            if a.stat_partials:
                writes.append(_flat(a.stat_partials, 4 * partials[0].numel()))
            if a.stat_totals:
                writes.append(_flat(a.stat_totals, 8 * self.BN_R * 2 * (Ntot // 4 if scatter else Ntot)))
            self._emit(prog, a, reads, writes)
        else:
            prog.add(a)
        return partials

    def _wgrad(self, prog, g, d, dw, KH, KW, stride, pad, Hout, Wout, in_aff=None, d_split=0, brb=None,
               bias_out=None, bias_plain=False):
        """bias_plain: d is the operand itself (materialised through dfl_conv_args.x_out) and the kernel still leaves its column
        sums -- the bias gradient -- per pixel slice."""
        a = WgradArgs()
        a.d_split = d_split
        a.g_bf16, a.d_bf16 = g.bf16, d.bf16
        a.g, a.d, a.dw = g.ptr, d.ptr, dw.data_ptr()
        if in_aff is not None:
            a.in_scale, a.in_shift = in_aff[0].data_ptr(), in_aff[1].data_ptr()
        a.N, a.Hin, a.Win, a.Cg, a.ldg = g.N, g.H, g.W, g.C, g.ld
        a.KH, a.KW, a.stride, a.pad = KH, KW, stride, pad
        a.Hout, a.Wout, a.Cm, a.ldd = Hout, Wout, d.C, d.ld
        if brb is not None:
            r_act, coef = brb                       # d = dy; the operand is formed from (dy, r) while the patch is staged (d_mode)
            a.d_mode, a.d2, a.ldd2 = 1, r_act.ptr, r_act.ld
            if isinstance(coef, dict):               # live statistics (include/dfl_hip.h)
                a.coef_tot, a.bn_gamma, a.bn_mean, a.bn_invstd = coef['tot'], coef['gamma'].data_ptr(), coef['mean'].data_ptr(), coef['invstd'].data_ptr()
                a.bn_count = float(coef['count'])
            else:
                a.coef = nat.ptr(coef)
        a.splits = 1
        s = nat.check(self.lib.dfl_wgrad_suggest_splits(C.addressof(a)), 'dfl_wgrad_suggest_splits')
        a.splits = s
        bias_job = None
        if (brb is not None or bias_plain) and bias_out is not None:
            # the column sums of that operand = the layer's bias gradient, one row per pixel slice
            bpart = self._new(s * d.C)
            a.bias_partial = bpart.data_ptr()
            bias_job = (bpart.data_ptr(), bias_out.data_ptr(), d.C, d.C, s, 1)    # queued BEHIND the launch that writes the rows (below): a
                                                                                  # batched sum flushed from here would read them unwritten
        n = d.C * g.C * KH * KW
        if s > 1:
            big = 4 * n >= self.FLUSH_BYTES
            part = self._shared_scratch('wg_partial', s * n) if big else self._new(s * n)   # deferred sums keep their own slices
            a.partial = part.data_ptr()
        if prog is self.bwd and self._deps is not None:
            # on the branch: nothing on the main chain consumes a weight gradient (the sums that finish it follow it there)
            reads = [_span(g), _flat(d.t.data_ptr(), d.t.numel() * d.t.element_size()) if d_split else _span(d)]
            if brb is not None:
                reads.append(_span(brb[0]))
                if isinstance(brb[1], dict):
                    reads.append(_flat(brb[1]['tot'], 8 * self.BN_R * 2 * d.C))
                elif brb[1] is not None:
                    reads.append(_flat(brb[1].data_ptr(), 4 * brb[1].numel()))
            writes = [_flat(a.partial, 4 * s * n) if s > 1 else _flat(a.dw, 4 * n)]
            if a.bias_partial:
                writes.append(_flat(a.bias_partial, 4 * s * d.C))
            self._emit(prog, a, reads, writes, branch=True)
        else:
            prog.add(a)
        if bias_job is not None:
            self._red_pending.append(bias_job)
            self._red_bytes += 4 * d.C
        if s > 1:
            self._defer_sum(prog, part.data_ptr(), dw.data_ptr(), n, n, s, KH * KW)

    # Small sums (bias gradients, pixel-slice partials of narrow layers) are not launched one by one: they queue up
    # and one dfl_reduce_batch finishes the queue once FLUSH_BYTES of gradient are waiting (and at the end of backward).
    def _defer_sum(self, prog, src, dst, n, stride, count, T=1):
        self._red_pending.append((src, dst, n, stride, count, T))
        self._red_bytes += 4 * n
        self._maybe_flush(prog)

    def _maybe_flush(self, prog):
        if self._red_bytes >= self.FLUSH_BYTES:
            self._flush_sums(prog)

    def _flush_sums(self, prog):
        self._flush_live_bwd(prog)
        jobs = self._red_pending
        if not jobs:
            return
        arr = (ReduceJob * len(jobs))()
        blocks = 0
        for a, (src, dst, n, stride, count, T) in zip(arr, jobs):
            a.src, a.dst, a.n, a.stride, a.count, a.first_block, a.T = src, dst, n, stride, count, blocks, T
            blocks += nat.check(self.lib.dfl_reduce_job_blocks(n, count), 'dfl_reduce_job_blocks')
        self.partial_sum_bytes += sum(4 * n * count for (_, _, n, _, count, _) in jobs)
        # (on the branch of a forked program: behind the weight gradients whose slices it sums, and nothing on the main chain reads a sum)
        idx = self._emit(prog, ReduceBatchArgs(jobs_dev=self._upload(arr), njobs=len(jobs), total_blocks=blocks),
                         [_flat(src, 4 * ((count - 1) * stride + n)) for (src, _, n, stride, count, _) in jobs],
                         [_flat(dst, 4 * n) for (_, dst, n, _, _, _) in jobs], branch=True)
        self._red_flushes.append((idx, [j[1] for j in jobs]))
        self._red_pending, self._red_bytes = [], 0

    def _dz_for(self, g, N, H, W, Cc, fused):
        """Scratch for the data gradient a layer hands to the layer below.  With the BatchNorm + ReLU backward folded into the
        data-gradient kernel that kernel READS the incoming gradient g while it writes: never the same buffer -- 'dz' and 'dpre0'
        (idle in that mode) alternate."""
        key = 'dpre0' if fused and self._is_scratch(g.t, 'dz') else 'dz'
        return self._scratch_act(key, N, H, W, Cc)

    def _bn_totals(self, Cc, bwd=False):
        """Address of [BN_R][2][C] doubles inside the plan's totals arena of the forward (backward) pass, zeroed by one memset at
        the start of that program."""
        need = self.BN_R * 2 * Cc
        ar = self._tot_bwd if bwd else self._tot_fwd
        if ar[0] is None:
            ar[0] = self._new(sum(self.chans) * self.bd * 2 * self.BN_R * 2, torch.float64)
        assert ar[1] + need <= ar[0].numel()
        ptr = ar[0].data_ptr() + 8 * ar[1]
        ar[1] += need
        return ptr

    def _flush_live_bwd(self, prog):
        """One batched launch for the BatchNorm parameter gradients (and residual bias gradients) of the live layers queued so far."""
        jobs = self._live_bwd_pending
        if not jobs:
            return
        arr = (BnBwdLiveJob * len(jobs))()
        for a, j in zip(arr, jobs):
            a.totals, a.save_mean, a.save_invstd = j['tot'], j['mean'].data_ptr(), j['invstd'].data_ptr()
            a.dgamma, a.dbeta, a.sum_out, a.C = j['dgamma'].data_ptr(), j['dbeta'].data_ptr(), nat.ptr(j['sum_out']), j['C']
        dsts = [j[k].data_ptr() for j in jobs for k in ('dgamma', 'dbeta', 'sum_out') if j[k] is not None]
        reads = [_flat(j['tot'], 8 * self.BN_R * 2 * j['C']) for j in jobs]
        reads += [_flat(j[k].data_ptr(), 4 * j['C']) for j in jobs for k in ('mean', 'invstd')]
        idx = self._emit(prog, BnBwdLiveArgs(jobs_dev=self._upload(arr), njobs=len(jobs), max_C=max(j['C'] for j in jobs)),
                         reads, [_flat(j[k].data_ptr(), 4 * j['C']) for j in jobs for k in ('dgamma', 'dbeta', 'sum_out') if j[k] is not None],
                         branch=True)
        self._red_flushes.append((idx, dsts))
        self._live_bwd_pending = []

    def _finish_live_bn(self):
        """The zero fill in front of the forward program and the one batched finalize behind its last BatchNorm layer."""
        jobs = self._live_jobs
        if not jobs:
            return
        arr = (BnLiveJob * len(jobs))()
        for a, j in zip(arr, jobs):
            a.totals, a.gamma, a.beta = j['totals'], j['gamma'].data_ptr(), j['beta'].data_ptr()
            a.running_mean = self.Bf[j['bname'] + '.running_mean'].data_ptr()
            a.running_var = self.Bf[j['bname'] + '.running_var'].data_ptr()
            a.num_batches_tracked = self.Bf[j['bname'] + '.num_batches_tracked'].data_ptr()
            a.scale, a.shift, a.save_mean, a.save_invstd = (j[k].data_ptr() for k in ('scale', 'shift', 'mean', 'invstd'))
            a.count, a.C, a.eps, a.momentum = j['count'], j['C'], BN_EPS, BN_MOMENTUM
        self.fwd.add(BnLiveArgs(jobs_dev=self._upload(arr), njobs=len(jobs), max_C=max(j['C'] for j in jobs)))
        self.fwd.insert(0, MemsetArgs(ptr=self._tot_fwd[0].data_ptr(), bytes=8 * self._tot_fwd[1]))

    def _shared_scratch(self, key, nelem):
        t = self._scratch.get(key)
        if t is None or t.numel() < nelem:
            t = self._new(nelem)
            self._scratch[key] = t
        return t

    def _colsum(self, prog, a, out):
        """out[c] = sum over pixels of a[:, c]."""
        nb = self.lib.dfl_rowblock_count(a.M, a.C)
        part = self._new(nb * 2 * a.C)
        self._emit(prog, ColstatsArgs(a=a.ptr, b=None, partials=part.data_ptr(), M=a.M, C=a.C, lda=a.ld, ldb=0, nblocks=nb,
                                        bf16=a.bf16), [_span(a)], [_flat(part.data_ptr(), 4 * part.numel())])
        self._defer_sum(prog, part.data_ptr(), out.data_ptr(), a.C, 2 * a.C, nb)

    # ------------------------------------------------------------------------------------------ circular padding
    # pad_mode='circular' (unet.py:211-212: nn.Conv2d(..., padding=1, padding_mode='circular')).  No reference CLI selects
    # it, so it is built from what exists rather than as a third addressing mode of every kernel: the input is copied into a
    # tensor with a one-pixel wrapped frame (9 window copies) and the convolution runs UNPADDED on that; backward, the data
    # gradient comes out on the framed grid (a "full" correlation) and the frame is folded back onto the pixels it copies
    # (9 window copies, 8 of them accumulating).  BatchNorm-on-load keeps working: every framed pixel is a real pixel.
    _WRAP = ((-1, 0, 1), (0, 1, None), (0, None, 1))      # (source start or -1 = last, destination start or None = last, extent or None = all)

    def _wrap_regions(self, H, W):
        out = []
        for sy, dy, h in ((H - 1, 0, 1), (0, 1, H), (0, H + 1, 1)):
            for sx, dx, w in ((W - 1, 0, 1), (0, 1, W), (0, W + 1, 1)):
                out.append((sy, sx, dy, dx, h, w))
        return out

    def _wrap_pad(self, prog, x):
        """Act [N, H+2, W+2, C] holding x with a wrapped one-pixel frame (raw values: an affine-on-load still applies)."""
        n = x.N * (x.H + 2) * (x.W + 2) * x.C
        t = self._new(n, torch.bfloat16 if x.esz == 2 else torch.float32)
        xp = Act(t, t.data_ptr(), x.C, x.N, x.H + 2, x.W + 2, x.C, x.esz)
        for sy, sx, dy, dx, h, w in self._wrap_regions(x.H, x.W):
            self._emit(prog, AffineCopyArgs(x=x.ptr, y=xp.ptr, N=x.N, H=h, W=w, C=x.C, ldx=x.ld, xH=x.H, xW=x.W, xoy=sy, xox=sx,
                                    ldy=xp.ld, yH=xp.H, yW=xp.W, yoy=dy, yox=dx, bf16=x.bf16))
        return xp

    def _wrap_fold(self, prog, dxp, dx, accumulate=0):
        """dx (+)= the framed gradient dxp folded back: the adjoint of _wrap_pad."""
        regs = self._wrap_regions(dx.H, dx.W)
        regs.sort(key=lambda r: 0 if (r[4] == dx.H and r[5] == dx.W) else 1)     # the interior first: it may overwrite
        for i, (sy, sx, dy, dx_, h, w) in enumerate(regs):
            self._emit(prog, AffineCopyArgs(x=dxp.ptr, y=dx.ptr, N=dx.N, H=h, W=w, C=dx.C, ldx=dxp.ld, xH=dxp.H, xW=dxp.W, xoy=dy, xox=dx_,
                                    ldy=dx.ld, yH=dx.H, yW=dx.W, yoy=sy, yox=sx, accumulate=(accumulate if i == 0 else 1), bf16=dx.bf16))

    def _framed_grad(self, like):
        """Scratch Act for a data gradient on the framed grid of `like` ([N, H+2, W+2, C])."""
        n = like.N * (like.H + 2) * (like.W + 2) * like.C
        t = self._new(n, self.adt)
        return Act(t, t.data_ptr(), like.C, like.N, like.H + 2, like.W + 2, like.C, self.aesz)

    # ------------------------------------------------------------------------------------------ build
    def _build(self):
        self._levels()
        self._alloc_buffers()
        self._down_forward()
        self._up_forward()
        self._finish_live_bn()
        self._heads_forward()
        if self.need_grad:
            self._grad_arena()
            dout, sums = self._heads_backward()
            dout, sums = self._up_backward(dout, sums)
            self._down_backward(dout, sums)
            self._finish_backward()
        self._finish_pack()
        if self.need_grad:
            self._grad_ready_ops()

    def _levels(self):
        """Architecture flags, channel count and spatial size of every level (input / output of its block, down then up)."""
        cfg = self.cfg
        self.depth, self.bd, self.bn, self.do_res = cfg['depth'], cfg['block_depth'], cfg['batch_norm'], cfg['do_res']
        self.pad = 1 if cfg['padding'] else 0
        self.circular = bool(self.pad) and cfg.get('pad_mode', 'zeros') == 'circular'
        self.upsample = cfg.get('up_mode', 'upconv') == 'upsample'
        self.chans = [2 ** (cfg['wf'] + i) for i in range(self.depth)]
        for c in self.chans:
            if c % 4 != 0:
                raise PlanError('channel counts must be multiples of 4 (wf >= 2)')
            if self.bf16 and c % 16 != 0:
                raise PlanError('math mode 4 (bf16 storage) needs channel counts that are multiples of 16 (wf >= 4); this '
                                'network has a %d-channel level' % c)
        self.shrink = 0 if self.pad else 2 * self.bd
        self.hin, self.win, self.hout, self.wout = [self.H], [self.W], [], []
        for i in range(self.depth):
            ho, wo = self.hin[i] - self.shrink, self.win[i] - self.shrink
            if ho < 1 or wo < 1:
                raise PlanError('input %dx%d too small for this architecture' % (self.H, self.W))
            self.hout.append(ho)
            self.wout.append(wo)
            if i != self.depth - 1:
                if ho < 2 or wo < 2:
                    raise PlanError('input %dx%d too small for this architecture' % (self.H, self.W))
                self.hin.append(ho // 2)
                self.win.append(wo // 2)
        if self.do_res and self.shrink != 0:
            raise PlanError('do_res=True needs padding=True: the 1x1 residual and the unpadded 3x3 stack differ in '
                            'size (the reference fails at unet.py:231 for the same reason)')
        self.up_hw = []          # size of the up-sampled tensor of up block j (level i = depth-2-j)
        uh, uw = self.hout[-1], self.wout[-1]
        for i in reversed(range(self.depth - 1)):
            uh, uw = 2 * uh, 2 * uw
            self.up_hw.append((uh, uw))
            uh, uw = uh - self.shrink, uw - self.shrink

    def _alloc_buffers(self):
        """Backward scratch, the input activation, and the concat buffers of the up path: allocated up front so that the
        down blocks write their bridge half directly."""
        N, chans = self.N, self.chans
        if self.need_grad:
            # backward scratch: sized for the largest [M][C] any block produces
            sizes = [N * self.hin[i] * self.win[i] * chans[i] for i in range(self.depth)]
            sizes += [N * uh * uw * chans[self.depth - 2 - j] for j, (uh, uw) in enumerate(self.up_hw)]
            mx = max(sizes)
            self._scratch['dpre0'] = self._new(mx, self.adt)
            self._scratch['dpre1'] = self._new(mx, self.adt)
            self._dpre_turn = 0
            self._scratch['dz'] = self._new(mx, self.adt)
            if self.bf16 and self.FUSE_BRB and self.DPRE_OUT_BYTES > 0:
                self._scratch['dmat'] = self._new(mx, self.adt)   # operand materialised by the data-gradient kernel (x_out)
        Cin0 = self.cfg['in_channels']
        if self.bf16 and Cin0 > 4:
            # multi-channel inputs enter the patch-resident kernels as bf16 (the 1..4-channel case keeps the fp32 image:
            # the direct first-layer kernels read it as is)
            if Cin0 % 16 != 0:
                raise PlanError('math mode 4 (bf16 storage) takes 1..4 or a multiple of 16 input channels')
            self.x_in = self._new(N * self.H * self.W * Cin0, torch.bfloat16)
            self._x0 = Act(self.x_in, self.x_in.data_ptr(), Cin0, N, self.H, self.W, Cin0, 2)
        else:
            self.x_in = self._new(N * self.H * self.W * Cin0)
            self._x0 = Act(self.x_in, self.x_in.data_ptr(), Cin0, N, self.H, self.W, Cin0)
        self.cat, self.dcat, self.direct_bridge = {}, {}, {}
        for j, i in enumerate(reversed(range(self.depth - 1))):
            ch, cw = self.up_hw[j]
            self.cat[i] = self._act(N, ch, cw, 2 * chans[i])
            self.direct_bridge[i] = (ch == self.hout[i] and cw == self.wout[i])
            if self.need_grad:
                self.dcat[i] = self._act(N, ch, cw, 2 * chans[i])

    # ------------------------------------------------------------------ one residual conv block, forward
    def _block_forward(self, prefix, xin, out, first=False):
        """Forward ops of UNetConvBlock `prefix` reading xin, writing out; returns the _Block its backward needs."""
        P, fwd, N, Cout = self.P, self.fwd, self.N, out.C
        blk = _Block(prefix, xin, out)
        cur, cur_aff, cur_live = xin, None, None
        step = 3 if self.bn else 2
        for d in range(self.bd):
            wname = '%s.block.%d' % (prefix, d * step)
            w, b = P[wname + '.weight'], P[wname + '.bias']
            wp = self._pack_conv_fwd(w)
            Ho, Wo = cur.H - (0 if self.pad else 2), cur.W - (0 if self.pad else 2)
            r = self._act(N, Ho, Wo, Cout)
            gin = self._wrap_pad(fwd, cur) if self.circular else cur     # what the convolution (and its weight gradient) gathers from
            live, live_bwd = self._live_stats(d, xin, cur, gin, Cout, first)
            tot = self._bn_totals(Cout) if live else None
            # inference: the BatchNorm between this convolution and the block's next one is applied by THIS kernel where it runs in
            # latency form (dfl_conv_args.out_scale: the consumer's two roundings, bit for bit) -- the consumer then reads its operand
            # plain instead of converting 8 channels per lane and k-step on its way into the matrix instruction
            pre_aff = None
            if self.bn and not self.training and not self.need_grad and not self.circular and self.pad == 1 and d < self.bd - 1:
                pre_aff = (self._new(Cout), self._new(Cout))
            part = self._conv(fwd, gin, wp, r, 3, 3, 1, 0 if self.circular else self.pad, Cout, bias=b,
                              in_aff=None if cur_live is not None else cur_aff, in_live=cur_live, relu=1,
                              stats=self.bn and self.training, stat_totals=tot, out_aff=pre_aff)
            out_aff_taken = pre_aff is not None and self._out_aff_taken
            relu = '%s.block.%d' % (prefix, d * step + 1)     # module name of the nn.ReLU (tests read its mask)
            aff, bnrec, cur_live = None, None, None
            if self.bn:
                bname = '%s.block.%d' % (prefix, d * step + 2)
                aff, bnrec = self._bn_forward(bname, part, tot, pre_aff if out_aff_taken else None, N * Ho * Wo, Cout)
                if live:
                    cur_live = (tot, P[bname + '.weight'], P[bname + '.bias'], N * Ho * Wo)
            blk.convs.append(_Layer(w, wname, relu, cur, gin, cur_aff, r, bnrec, live_bwd))
            self.relu_out[relu] = r
            cur, cur_aff = r, (None if out_aff_taken else aff)       # (out_aff_taken: r holds BN(ReLU(.)) already)
        assert cur.H == xin.H - self.shrink and cur.W == xin.W - self.shrink
        if self.do_res:
            blk.rw, rb = P[prefix + '.res_conv1x1.weight'], P[prefix + '.res_conv1x1.bias']
            self._conv(fwd, xin, self._pack_conv_fwd(blk.rw), out, 1, 1, 1, 0, Cout, bias=rb,
                       add=cur, add_aff=None if cur_live is not None else cur_aff, add_live=cur_live)
            if not self.training and not self.need_grad:
                self._pair_last_two()
        else:
            a = AffineCopyArgs(x=cur.ptr, y=out.ptr, N=N, H=cur.H, W=cur.W, C=Cout, ldx=cur.ld, xH=cur.H, xW=cur.W,
                               ldy=out.ld, yH=out.H, yW=out.W, bf16=cur.bf16)
            if cur_aff is not None:
                a.scale, a.shift = cur_aff[0].data_ptr(), cur_aff[1].data_ptr()
            fwd.add(a)
        self.dbg['out:' + prefix] = out
        self.dbg['xin:' + prefix] = xin
        # pre-BatchNorm output of the block's last conv: what a producer of this block's dout needs for fused_in ...
        last = blk.convs[-1]
        blk.last_r = last.r if last.bn is not None else None
        blk.last_live = bool(last.bn is not None and last.live_bwd)      # ... and may leave them as live totals
        return blk

    def _live_stats(self, d, xin, cur, gin, Cout, first):
        """(live, live_bwd) of layer d of a block reading xin: its forward statistics are live totals, and its backward can take
        live (sum dy, sum dy*r) -- its consumers derive the coefficients."""
        # Live statistics (round 4): this layer's BatchNorm is not finalised by a launch between producer and consumer --
        # the producing patch kernel adds its sums to the layer's totals, the consuming patch kernel (next 3x3, or the
        # residual 1x1 whose epilogue adds BN(r)) derives scale / shift itself; ONE batched launch at the end of the forward
        # pass leaves the vectors the backward pass and the module state need.  Both kernels must be patch kernels.
        # (the network's first block: its 1-channel layers run the direct kernels, which take part as well -- the 3x3 row
        # form as a producer, the 1x1 form as the consumer of "+ BN(r)", the 3x3 weight gradient as a consumer of A, B, C)
        patch_in = lambda t: bool(t.bf16) and t.C % 16 == 0            # a convolution reading t runs the bf16 patch kernels
        one_ch = lambda t: (not t.bf16) and t.C == 1 and Cout in (8, 16, 32, 64) and self.pad == 1
        # (round 5) fp32 tensors: the GEMM kernels take part as well -- producer: any of them (statistics tail, K-slice finish
        # kernel); consumers: the fast gather of the next 3x3 (its scale / shift table in LDS) and the residual 1x1's "+ BN(r)"
        # (the consumer's table form needs the FAST gather, which needs tensors below 2 GiB -- a larger activation keeps
        # the finalize launch and the generic kernel instead of failing in dfl_conv2d)
        small = lambda t: t.N * t.H * t.W * t.ld * 4 < (1 << 31) - 4096
        gemm_in = lambda t: (not t.bf16) and t.C % 16 == 0 and small(t)
        can = self.LIVE_BN and self.bn and self.training and not self.circular
        inner = d < self.bd - 1
        if self.bf16:
            live = can and (patch_in(gin) or one_ch(gin)) and (inner or (self.do_res and (patch_in(xin) or one_ch(xin))))
        else:
            live = (can and gemm_in(gin) and Cout % 16 == 0 and gin.N * gin.H * gin.W * 2 * Cout * 4 < (1 << 31) - 4096
                    and (inner or self.do_res))
        live_bwd = (can and self.bf16 and self.FUSE_BRB and self.need_grad
                    and (patch_in(cur) or (one_ch(cur) and d == 0 and first and not self.input_grad)))
        return live, live_bwd

    def _bn_forward(self, bname, part, tot, out_aff, count, Cout):
        """Scale / shift of BatchNorm `bname` behind a convolution (applied by the consumer on load) and the statistics its
        backward reads.  Training: the live batched finalize (tot), or a finalize launch over the producer's partials;
        eval: the running statistics.  out_aff: the producer already applies scale / shift.  Returns (aff, bn record)."""
        P, Bf, fwd = self.P, self.Bf, self.fwd
        gamma, beta = P[bname + '.weight'], P[bname + '.bias']
        scale, shift = out_aff if out_aff is not None else (self._new(Cout), self._new(Cout))
        mean, invstd = self._new(Cout), self._new(Cout)
        if self.training and tot is not None:
            self._live_jobs.append(dict(totals=tot, gamma=gamma, beta=beta, bname=bname, scale=scale, shift=shift, mean=mean,
                                        invstd=invstd, count=count, C=Cout))
        elif self.training:
            fwd.add(BnFinalizeArgs(partials=part[0].data_ptr(), gamma=gamma.data_ptr(), beta=beta.data_ptr(),
                                   running_mean=Bf[bname + '.running_mean'].data_ptr(),
                                   running_var=Bf[bname + '.running_var'].data_ptr(),
                                   num_batches_tracked=Bf[bname + '.num_batches_tracked'].data_ptr(),
                                   scale=scale.data_ptr(), shift=shift.data_ptr(),
                                   save_mean=mean.data_ptr(), save_invstd=invstd.data_ptr(),
                                   count=count, nblocks=part[1], C=Cout, eps=BN_EPS, momentum=BN_MOMENTUM))
        else:
            # eval mode: scale / shift depend on parameters and running statistics only -- constants between two
            # forwards of an inference loop (util.test_dataset, seg_dataset_ensemble: one image after the other).
            # Inference plans compute them in the PACK program (re-run when a parameter, a buffer or a training
            # forward has touched them, UNet._ensure_packed) instead of 22 launches in every forward (round 4).
            (fwd if self.need_grad else self._prep).add(
                BnEvalArgs(gamma=gamma.data_ptr(), beta=beta.data_ptr(),
                           running_mean=Bf[bname + '.running_mean'].data_ptr(),
                           running_var=Bf[bname + '.running_var'].data_ptr(),
                           scale=scale.data_ptr(), shift=shift.data_ptr(), C=Cout, eps=BN_EPS))
            if self.need_grad:
                # gradients through eval-mode BatchNorm (nn.Module semantics of unet.py:161-193): the statistics
                # are the running ones -- mean is the buffer itself, 1/sqrt(var + eps) is the scale of (gamma = 1)
                ones, zeros = self._const(Cout, 1.0), self._const(Cout, 0.0)
                mean = Bf[bname + '.running_mean']
                fwd.add(BnEvalArgs(gamma=ones.data_ptr(), beta=zeros.data_ptr(), running_mean=mean.data_ptr(),
                                   running_var=Bf[bname + '.running_var'].data_ptr(),
                                   scale=invstd.data_ptr(), shift=self._new(Cout).data_ptr(), C=Cout, eps=BN_EPS))
        self.dbg['bn:' + bname] = (scale, shift, mean, invstd)
        return (scale, shift), (gamma, mean, invstd, bname)

    def _pair_last_two(self):
        """Inference: a block's last 3x3 convolution and its residual 1x1 run as ONE launch where the library can
        (dfl_conv2d_pair: the latency form of a batch-1 forward -- 11 launches less in its chain of 44)."""
        fwd = self.fwd
        if len(fwd) < 2 or not isinstance(fwd.structs[-2], ConvArgs):
            return
        pk = self.lib.dfl_conv_pair_ok(C.addressof(fwd.structs[-2]), C.addressof(fwd.structs[-1]))
        if pk not in (1, 2):
            return
        b_ = fwd.pop()
        a_ = fwd.pop()
        if pk == 2:        # K-sliced: the partial sums of BOTH products go through a buffer of twice the size
            Mp = a_.N * a_.Hout * a_.Wout
            a_.partial = self._shared_scratch('pair_partial', 2 * a_.splits * Mp * a_.Ntot).data_ptr()
        fwd.keep += [a_, b_]
        fwd.add(nat.ConvPairArgs(a=C.addressof(a_), b=C.addressof(b_)))

    # ------------------------------------------------------------------ forward: down path, up path, heads
    def _down_forward(self):
        """Encoder blocks; a block's output is the bridge half of its level's concat buffer where the sizes agree (a crop
        copy fills it otherwise), then max-pool or the strided convolution makes the next level's input."""
        N, fwd = self.N, self.fwd
        x = self._x0
        self._down = []         # per level: dict(blk, crop, nxt)
        for i in range(self.depth):
            Ci = self.chans[i]
            last = i == self.depth - 1
            if not last and self.direct_bridge[i]:
                out = self.cat[i].chan_slice(Ci, Ci)
            else:
                out = self._act(N, self.hout[i], self.wout[i], Ci)
            rec = dict(blk=self._block_forward('down_path.%d' % i, x, out, first=(i == 0)))
            self._down.append(rec)
            if last:
                break
            if not self.direct_bridge[i]:
                ch, cw = self.up_hw[self.depth - 2 - i]
                oy, ox = (self.hout[i] - ch) // 2, (self.wout[i] - cw) // 2
                dst = self.cat[i].chan_slice(Ci, Ci)
                fwd.add(AffineCopyArgs(x=out.ptr, y=dst.ptr, N=N, H=ch, W=cw, C=Ci, ldx=out.ld, xH=out.H, xW=out.W,
                                       xoy=oy, xox=ox, ldy=dst.ld, yH=ch, yW=cw, bf16=out.bf16))
                rec['crop'] = (oy, ox, ch, cw)
            nxt = self._act(N, self.hin[i + 1], self.win[i + 1], Ci)
            if self.cfg['max_pool']:
                self.pool_in[i] = out
                fwd.add_pool(PoolArgs(x=out.ptr, y=nxt.ptr, N=N, H=out.H, W=out.W, C=Ci, ldx=out.ld, ldy=nxt.ld,
                                      bf16=out.bf16), backward=False)
            else:
                dw_, db_ = self.P['downsample_convs.%d.weight' % i], self.P['downsample_convs.%d.bias' % i]
                self._conv(fwd, out, self._pack_conv_fwd(dw_), nxt, 2, 2, 2, 0, Ci, bias=db_)
            rec['nxt'] = nxt
            self.dbg['nxt:%d' % i] = nxt
            x = nxt

    def _up_forward(self):
        """Decoder: up-sampling into the up half of each level's concat buffer, then the block; its output is self.feat."""
        N, fwd = self.N, self.fwd
        self._up = []           # per up block j: dict(blk, u, level, name, w)
        u = self._down[-1]['blk'].out
        for j, i in enumerate(reversed(range(self.depth - 1))):
            Ci = self.chans[i]
            name = 'up_path.%d' % j
            ch, cw = self.up_hw[j]
            up_half = self.cat[i].chan_slice(0, Ci)
            if self.upsample:
                # up_mode='upsample' (unet.py:242-244): bilinear x2, then a 1x1 convolution.  Both are linear, the convolution is
                # pointwise and the interpolation weights sum to one: conv(up(x)) = up(conv(x)) with the bias added once -- the 1x1
                # runs on the small grid, dfl_upsample2x_fwd spreads its result into the up half of the concat buffer
                uw_, ub_ = self.P[name + '.up.1.weight'], self.P[name + '.up.1.bias']
                ylow = self._act(N, u.H, u.W, Ci)
                self._conv(fwd, u, self._pack_conv_fwd(uw_), ylow, 1, 1, 1, 0, Ci, bias=ub_)
                fwd.add(UpsampleArgs(x=ylow.ptr, y=up_half.ptr, N=N, H=u.H, W=u.W, C=Ci, ldx=ylow.ld, ldy=up_half.ld, bf16=ylow.bf16),
                        nat.OP_UPSAMPLE_FWD)
            else:
                uw_, ub_ = self.P[name + '.up.weight'], self.P[name + '.up.bias']
                self._conv(fwd, u, self._pack_convT_fwd(uw_), up_half, 1, 1, 1, 0, 4 * Ci, bias=ub_, scatter=1, Hout=ch, Wout=cw)
            out = self._act(N, ch - self.shrink, cw - self.shrink, Ci)
            self.dbg['cat:%d' % j] = self.cat[i]
            blk = self._block_forward(name + '.conv_block', self.cat[i], out)
            self._up.append(dict(blk=blk, u=u, level=i, name=name, w=uw_))
            u = out
        self.feat = u

    def _heads_forward(self):
        """Landmark block (if any) and the head call(s) on the decoder output."""
        cfg, N, fwd, u = self.cfg, self.N, self.fwd, self.feat
        NC, L = cfg['n_classes'], cfg['num_lands']
        F = u.C
        self.NC, self.L = NC, L
        w_seg = self.P['seg_conv.weight']
        w_l1 = self.P['lands_1x1.0.weight'] if L > 0 else None
        w_l2 = self.P.get('lands_1x1.1.weight') if L > 0 else None
        NM = w_l1.shape[0] if L > 0 else 0
        # lands_num_1x1 > 2 (unet.py:146-156): the 1x1 convolutions behind the first one are bias-free and have no
        # non-linearity between them, i.e. ONE linear map  W_k ... W_2 W_1  (L x NM).  The head kernels run with that product
        # (fold_tail, re-made whenever weights change) and the gradient they return for it is taken apart afterwards
        # (unfold_tail_grads):  dW_j = (W_k ... W_{j+1})^T  G  (W_{j-1} ... W_1)^T.
        self.tail_names = []
        j = 1
        while L > 0 and ('lands_1x1.%d.weight' % j) in self.P:
            self.tail_names.append('lands_1x1.%d.weight' % j)
            j += 1
        self.w_l2_eff = self.g_l2_eff = None
        if len(self.tail_names) > 1:
            self.w_l2_eff = self._new(L * NM).view(L, NM, 1, 1)
            self.g_l2_eff = self._new(L * NM).view(L, NM, 1, 1)
            w_l2 = self.w_l2_eff
        # lands_block_depth > 0 (unet.py:108-137,185-187): bias-only 3x3 convolutions F -> F/2 (-> F/2 ...) in front of the
        # landmark 1x1.  Their output lb is written next to a copy of the features into ONE wider tensor [u | lb], and the
        # head kernels run on that with widened weight matrices -- w_seg' = [w_seg | 0], w_l1' = [0 | W1[:, :F/2] | W1[:, F/2:]]
        # (fold_tail) -- so seg sees u, the landmark branch sees cat(lb, logits), and no kernel changes.  Their gradients come
        # back as columns of the widened matrices and of dx (unfold_tail_grads; the lb columns of dx feed the convolutions'
        # backward, the u columns go on into the decoder).
        lbd = int(cfg.get('lands_block_depth', 0)) if L > 0 else 0
        self.lb_layers = []
        self.eff_heads = None
        head_x, Fh = u, F
        # Unpadded (padding=False) the landmark block's valid 3x3 convolutions shrink lb against the features by lbd pixels per
        # side; the reference crops the logits to lb (unet.py:185-187), so the heat maps come out SMALLER than the
        # segmentation.  The head kernels then run twice: on u with the segmentation matrix alone (the full-size seg), and on
        # [crop(u) | lb] with the widened matrices (heat maps; its soft-max output, a crop of seg, stays in a plan buffer).
        self.split_heads = lbd > 0 and not cfg['padding']
        hl, wl = u.H, u.W
        if lbd > 0:
            F2 = F // 2
            if F2 % (16 if self.bf16 else 4) != 0:
                raise PlanError('lands_block_depth > 0 needs F/2 = %d channels to be a multiple of %d in this arithmetic' % (F2, 16 if self.bf16 else 4))
            if not self.pad:
                hl, wl = u.H - 2 * lbd, u.W - 2 * lbd
                if hl < 1 or wl < 1:
                    raise PlanError('input %dx%d too small for lands_block_depth=%d without padding' % (self.H, self.W, lbd))
            Fh = F + F2
            uw = self._act(N, hl, wl, Fh)
            fwd.add(AffineCopyArgs(x=u.ptr, y=uw.ptr, N=N, H=hl, W=wl, C=F, ldx=u.ld, xH=u.H, xW=u.W, xoy=(u.H - hl) // 2, xox=(u.W - wl) // 2,
                                   ldy=uw.ld, yH=hl, yW=wl, bf16=u.bf16))
            src = u
            for j in range(lbd):
                wname, bname = 'lands_block.%d.weight' % j, 'lands_block.%d.bias' % j
                ho_, wo_ = src.H - (0 if self.pad else 2), src.W - (0 if self.pad else 2)
                dst = uw.chan_slice(F, F2) if j == lbd - 1 else self._act(N, ho_, wo_, F2)
                gin = self._wrap_pad(fwd, src) if self.circular else src
                self._conv(fwd, gin, self._pack_conv_fwd(self.P[wname]), dst, 3, 3, 1, 0 if self.circular else self.pad, F2,
                           bias=self.P[bname], Hout=ho_, Wout=wo_)
                self.lb_layers.append((src, dst, wname, bname, gin, ho_, wo_))
                src = dst
            self.eff_heads = dict(F=F, F2=F2, w_seg=self._new(NC * Fh).view(NC, Fh, 1, 1).zero_(),
                                  w_l1=self._new(NM * (Fh + NC)).view(NM, Fh + NC, 1, 1).zero_(),
                                  g_seg=self._new(NC * Fh).view(NC, Fh, 1, 1), g_l1=self._new(NM * (Fh + NC)).view(NM, Fh + NC, 1, 1))
            head_x = uw
        sm = 1 if cfg['do_soft_max'] else 0
        self.head_fwd_seg = None
        if self.split_heads:
            self.head_fwd_seg = HeadFwdArgs(x=u.ptr, w_seg=self.P['seg_conv.weight'].data_ptr(), N=N, H=u.H, W=u.W, F=F, ldx=u.ld,
                                            NC=NC, NM=0, L=0, softmax=sm, x_bf16=u.bf16)
            fwd.add(self.head_fwd_seg, volatile=True)
            self.seg_crop = self._new(N * NC * hl * wl)         # soft-max of the landmark call: what its backward recomputes from
        if self.eff_heads is not None:
            w_seg, w_l1 = self.eff_heads['w_seg'], self.eff_heads['w_l1']
        self.head_fwd = HeadFwdArgs(x=head_x.ptr, w_seg=w_seg.data_ptr(), w_l1=nat.ptr(w_l1), w_l2=nat.ptr(w_l2),
                                    N=N, H=hl, W=wl, F=Fh, ldx=head_x.ld, NC=NC, NM=NM, L=L, softmax=sm, x_bf16=u.bf16)
        fwd.add(self.head_fwd, volatile=True)       # writes the caller-owned outputs: addresses change per call
        self._head_in = (head_x, w_seg, w_l1, w_l2, NM)
        self.out_hw = (u.H, u.W)
        self.heat_hw = (hl, wl)

    # ------------------------------------------------------------------ backward program
    def _grad_arena(self):
        """Flat gradient arena in parameters() order."""
        self.grad_names = [k for k in self.P.keys()]
        offs, tot = {}, 0
        for k in self.grad_names:
            offs[k] = tot
            tot += (self.P[k].numel() + 3) // 4 * 4          # keep every slice 16-byte aligned
        self.grad_flat = self._new(tot).zero_()
        self.G = {k: self.grad_flat[offs[k]:offs[k] + self.P[k].numel()].view(self.P[k].shape) for k in self.grad_names}
        self.grad_offsets = offs
        self.dead_params = set()
        if not self.cfg['max_pool']:
            self.dead_params.add('downsample_convs.%d.weight' % (self.depth - 1))    # never used in forward
            self.dead_params.add('downsample_convs.%d.bias' % (self.depth - 1))

    def _heads_backward(self):
        """Backward of the head call(s) and of the landmark block; returns (gradient of the decoder output, the sums its
        producer left for the last block's BatchNorm backward, or None)."""
        G, L, u = self.G, self.L, self.feat
        head_x, w_seg, w_l1, w_l2, NM = self._head_in
        g_seg = self.eff_heads['g_seg'] if self.eff_heads is not None else G['seg_conv.weight']
        g_l1 = (self.eff_heads['g_l1'] if self.eff_heads is not None else G['lands_1x1.0.weight']) if L > 0 else None
        g_l2 = None
        if L > 0 and w_l2 is not None:
            g_l2 = self.g_l2_eff if self.g_l2_eff is not None else G['lands_1x1.1.weight']
        hl, wl = self.heat_hw
        self.head_bwd_seg = dfeat_a = None
        if self.split_heads:
            self.g_seg_full = self._new(self.NC * u.C).view(self.NC, u.C, 1, 1)
            self.head_bwd_seg, dfeat_a, _ = self._head_backward(u, u.H, u.W, self.P['seg_conv.weight'], None, None, 0, 0,
                                                                self.g_seg_full, None, None)
            self.dseg_zero = self._new(self.N * self.NC * hl * wl).zero_()
        last = self._up[-1]['blk'] if self._up else self._down[-1]['blk']
        live_r = (last.last_r if (self.LIVE_BN and self.LIVE_HEAD and not self.lb_layers and not self.split_heads and last.last_live)
                  else None)
        self.head_bwd, dfeat, sums = self._head_backward(head_x, hl, wl, w_seg, w_l1, w_l2, NM, L, g_seg, g_l1, g_l2, live_r=live_r)
        self.dbg['dfeat'] = dfeat
        if self.lb_layers:
            return self._lands_block_backward(dfeat, dfeat_a), None
        return dfeat, sums

    def _head_backward(self, x_act, H_, W_, ws, w1, w2, nm, nl, gs, g1, g2, live_r=None):
        """HeadBwdArgs + its weight gradients on x_act [N,H_,W_,Fx]; returns (args, dx Act, live sums).  live_r: the saved ReLU
        output behind the BatchNorm dx enters -- the matrix-core kernel then adds (sum dx, sum dx*r) to that layer's live
        totals itself (live sums: ('live', totals), or None)."""
        N, NC, Fx, bwd = self.N, self.NC, x_act.C, self.bwd
        sld = self.lib.dfl_head_scratch_ld_for(Fx, NC, nm, nl)
        M_ = N * H_ * W_
        dx = self._act(N, H_, W_, Fx)
        fused_head = bool(x_act.bf16) and Fx == 32 and NC <= 8 and nm <= 24 and nl <= 16
        hb = HeadBwdArgs(x=x_act.ptr, w_seg=ws.data_ptr(), w_l1=nat.ptr(w1), w_l2=nat.ptr(w2), dx=dx.ptr, N=N, H=H_, W=W_, F=Fx,
                         ldx=x_act.ld, lddx=dx.ld, NC=NC, NM=nm, L=nl, softmax=1 if self.cfg['do_soft_max'] else 0, scratch_ld=sld,
                         x_bf16=x_act.bf16)
        # bf16 features of the paper's width: the head kernel takes its three weight gradients itself (include/dfl_hip.h);
        # otherwise it leaves a per-pixel scratch row and three 1x1 weight-gradient launches follow
        live = None
        # mirrors head_mfma_ok (csrc/head.hip), whose 16-byte alignment of w_seg is taken for granted here
        mfma_head = fused_head and (nl == 0 or w2 is not None) and x_act.ld % 8 == 0
        if mfma_head and live_r is not None:
            tot = self._bn_totals(Fx, bwd=True)
            hb.stat_other, hb.ldso, hb.stat_totals = live_r.ptr, live_r.ld, tot
            live = ('live', tot)
        if fused_head:
            part = self._new(4096 * nat.check(self.lib.dfl_head_wgrad_blocks(M_), 'dfl_head_wgrad_blocks'))
            hb.wg_partial = part.data_ptr()
            hb.dw_seg = gs.data_ptr()
            if nl > 0:
                hb.dw_l1 = g1.data_ptr()
                if w2 is not None:
                    hb.dw_l2 = g2.data_ptr()
        else:
            scratch = self._new(M_ * sld)
            hb.scratch = scratch.data_ptr()
        self._emit(bwd, hb, volatile=True)                 # reads the caller-owned seg / dseg / dheat
        if not fused_head:
            off = [self.lib.dfl_head_scratch_off_for(Fx, NC, nm, nl, k) for k in range(5)]
            sact = lambda o, c: Act(scratch, scratch.data_ptr() + 4 * o, sld, N, H_, W_, c)
            self._wgrad(bwd, sact(off[0], Fx), sact(off[1], NC), gs, 1, 1, 1, 0, H_, W_)
            if nl > 0:
                self._wgrad(bwd, sact(off[0], Fx + NC), sact(off[2], nm), g1, 1, 1, 1, 0, H_, W_)
                if w2 is not None:
                    self._wgrad(bwd, sact(off[3], nm), sact(off[4], nl), g2, 1, 1, 1, 0, H_, W_)
        return hb, dx, live

    def _lands_block_backward(self, dfeat, dfeat_a):
        """Backward of the landmark block: the lb columns of dfeat through its 3x3 convolutions (bias sums, weight gradients,
        data gradients), the first one's data gradient added onto the u columns, which then enter the decoder.  dfeat_a:
        the full-size feature gradient of the segmentation call (split heads).  Returns the gradient of the decoder output."""
        N, G, bwd, u = self.N, self.G, self.bwd, self.feat
        F, Fh = u.C, dfeat.C
        hl, wl = self.heat_hw
        if self.split_heads:
            # the u columns of the landmark call's dx belong to the centre window of the full-size feature gradient
            dout = dfeat_a
            src_u = dfeat.chan_slice(0, F)
            self._emit(bwd, AffineCopyArgs(x=src_u.ptr, y=dout.ptr, N=N, H=hl, W=wl, C=F, ldx=src_u.ld, xH=hl, xW=wl, ldy=dout.ld,
                                   yH=u.H, yW=u.W, yoy=(u.H - hl) // 2, yox=(u.W - wl) // 2, accumulate=1, bf16=dout.bf16))
        else:
            dout = dfeat.chan_slice(0, F)
        d = dfeat.chan_slice(F, Fh - F)
        for j in reversed(range(len(self.lb_layers))):
            src, dst, wname, bname, gin, ho_, wo_ = self.lb_layers[j]
            self._colsum(bwd, d, G[bname])
            self._wgrad(bwd, gin, d, G[wname], 3, 3, 1, 0 if self.circular else self.pad, ho_, wo_)
            wd = self._pack_conv_dgrad(self.P[wname])
            tgt = dout if j == 0 else self._act(N, src.H, src.W, Fh - F)
            if self.circular:
                dzp = self._framed_grad(src)
                self._conv(bwd, d, wd, dzp, 3, 3, 1, 2, src.C)
                self._wrap_fold(bwd, dzp, tgt, accumulate=1 if j == 0 else 0)
            else:
                self._conv(bwd, d, wd, tgt, 3, 3, 1, 2 - self.pad, src.C, accumulate=1 if j == 0 else 0)
            if j > 0:
                d = tgt
        return dout

    def _up_backward(self, dout, sums):
        """Decoder backward, last block first.  Column sums ride on the kernels that produce the tensors: the conv that
        completes dcat leaves sum(dy) (the transposed conv's bias gradient), the conv that produces du leaves the
        BatchNorm-backward sums of the block that consumes du.  Returns (du, sums) of the deepest down block."""
        N, G, bwd = self.N, self.G, self.bwd
        for j in reversed(range(len(self._up))):
            rec = self._up[j]
            i = rec['level']
            Ci = self.chans[i]
            st = self._block_backward(rec['blk'], dout, self.dcat[i], fused_in=sums, dxin_stats=True)
            dy = self.dcat[i].chan_slice(0, Ci)                  # gradient of the transposed-conv output
            uin = rec['u']
            bias_name = rec['name'] + ('.up.1.bias' if self.upsample else '.up.bias')
            if st is not None:                                   # rows of (sum v, sum v^2) over all 2*Ci columns of dcat
                self._defer_sum(bwd, st[0].data_ptr(), G[bias_name].data_ptr(), Ci, 4 * Ci, st[1])
            else:
                self._colsum(bwd, dy, G[bias_name])              # (upsample: the adjoint preserves column sums)
            du = self._act(N, uin.H, uin.W, uin.C)
            self.dbg['du:%d' % j] = du
            consumer = self._up[j - 1]['blk'] if j > 0 else self._down[-1]['blk']
            r_last = consumer.last_r
            if self.upsample:
                # gradient of the small-grid 1x1 result = adjoint of the interpolation applied to dy; then an ordinary 1x1 layer
                dylow = self._act(N, uin.H, uin.W, Ci)
                self._emit(bwd, UpsampleArgs(x=dylow.ptr, y=dy.ptr, N=N, H=uin.H, W=uin.W, C=Ci, ldx=dylow.ld, ldy=dy.ld, bf16=dy.bf16),
                           kind=nat.OP_UPSAMPLE_BWD)
                self._wgrad(bwd, uin, dylow, G[rec['name'] + '.up.1.weight'], 1, 1, 1, 0, uin.H, uin.W)
                sums = self._conv(bwd, dylow, self._pack_conv_dgrad(rec['w']), du, 1, 1, 1, 0, uin.C,
                                  stats=r_last is not None, stat_other=r_last,
                                  stat_totals=self._bn_totals(uin.C, bwd=True) if (r_last is not None and consumer.last_live) else None)
            else:
                # dW[ci][co][ab] = sum x[i,j][ci] * dy[2i+a,2j+b][co]
                self._wgrad(bwd, dy, uin, G[rec['name'] + '.up.weight'], 2, 2, 2, 0, uin.H, uin.W)
                wd = self._pack_convT_dgrad(rec['w'])
                sums = self._conv(bwd, dy, wd, du, 2, 2, 2, 0, uin.C, stats=r_last is not None, stat_other=r_last,
                                  stat_totals=self._bn_totals(uin.C, bwd=True) if (r_last is not None and consumer.last_live) else None)
            dout = du
        return dout, sums

    def _down_backward(self, dout, sums):
        """Encoder backward, deepest block first: a block's output gradient is its bridge gradient (+ crop padding) plus
        the down-sampling gradient; the conv that completes a block-input gradient leaves the down-sampling bias gradient."""
        N, G, bwd = self.N, self.G, self.bwd
        dnxt = dnxt_sums = None          # gradient of the next level's input, and its column sums (from that block's backward)
        for i in reversed(range(self.depth)):
            rec = self._down[i]
            blk = rec['blk']
            out = blk.out
            Ci = self.chans[i]
            if i != self.depth - 1:
                sums = None
                if self.direct_bridge[i]:
                    dout = self.dcat[i].chan_slice(Ci, Ci)
                else:
                    dout = self._act(N, out.H, out.W, Ci)
                    oy, ox, ch, cw = rec['crop']
                    src = self.dcat[i].chan_slice(Ci, Ci)
                    self._emit(bwd, MemsetArgs(ptr=dout.ptr, bytes=dout.esz * dout.M * Ci))
                    self._emit(bwd, AffineCopyArgs(x=src.ptr, y=dout.ptr, N=N, H=ch, W=cw, C=Ci, ldx=src.ld, xH=ch, xW=cw,
                                           ldy=dout.ld, yH=out.H, yW=out.W, yoy=oy, yox=ox, bf16=src.bf16))
                nxt = rec['nxt']
                if self.cfg['max_pool']:
                    self._emit(bwd, PoolArgs(x=out.ptr, y=dnxt.ptr, dx=dout.ptr, N=N, H=out.H, W=out.W, C=Ci, ldx=out.ld,
                                             ldy=dnxt.ld, lddx=dout.ld, bf16=out.bf16), kind=nat.OP_POOL_BWD)
                else:
                    wname = 'downsample_convs.%d' % i
                    if dnxt_sums is not None:
                        self._defer_sum(bwd, dnxt_sums[0].data_ptr(), G[wname + '.bias'].data_ptr(), Ci, 2 * Ci, dnxt_sums[1])
                    else:
                        self._colsum(bwd, dnxt, G[wname + '.bias'])
                    self._wgrad(bwd, out, dnxt, G[wname + '.weight'], 2, 2, 2, 0, nxt.H, nxt.W)
                    wd = self._pack_down_dgrad(self.P[wname + '.weight'])
                    # the last kernel that writes dout leaves sum(dout), sum(dout * r_last) for the block's first BN backward
                    r_last = blk.last_r
                    # (the scatter visits the 2*H' x 2*W' pixels it writes: with an odd out.H / out.W the last row / column of
                    # dout holds bridge gradient only and would be missing from the sums -- then the separate pass takes them)
                    want = (self.FUSE_DOWN_STATS and r_last is not None and bool(dout.bf16) and bool(r_last.bf16)
                            and out.H == 2 * nxt.H and out.W == 2 * nxt.W)
                    sums = self._conv(bwd, dnxt, wd, dout, 1, 1, 1, 0, 4 * Ci, accumulate=1, scatter=1,
                                      Hout=out.H, Wout=out.W, stats=want, stat_other=r_last if want else None,
                                      stat_totals=self._bn_totals(Ci, bwd=True) if (want and blk.last_live) else None)
            xin = blk.xin
            if i > 0:
                dxin = self._act(N, xin.H, xin.W, xin.C)
            elif self.input_grad:
                if self.bf16:
                    raise PlanError('gradients with respect to the network input are implemented for the fp32-tensor arithmetic '
                                    'modes only (DFL_MATH=fp32 / bf16x3 / bf16x6 / bf16), not for bf16 storage')
                dxin = self.dx_in = self._act(N, xin.H, xin.W, xin.C)
            else:
                dxin = None
            dnxt_sums = self._block_backward(blk, dout, dxin, fused_in=sums,
                                             dxin_stats=dxin is not None and i > 0 and not self.cfg['max_pool'])
            dnxt = dxin

    # ------------------------------------------------------------------ one residual conv block, backward
    def _block_backward(self, blk, dout, dxin, fused_in=None, dxin_stats=False):
        """dout: Act with d(loss)/d(block output); dxin: Act to receive d/d(xin) (None for the net input).
        fused_in: BatchNorm-backward sums of dout -- (partials, rows) of sum(dout), sum(dout * r_last) per channel, or
        ('live', totals) -- when the kernel that wrote dout already left them (saves this block's first statistics pass).
        dxin_stats: let the LAST kernel that writes dxin leave its column sums; returns them as (partials, rows) -- the
        caller's bias gradient."""
        self.dbg['dout:' + blk.prefix] = dout
        if dxin is not None:
            self.dbg['dxin:' + blk.prefix] = dxin
        if self.do_res:
            self._wgrad(self.bwd, blk.xin, dout, self.G[blk.prefix + '.res_conv1x1.weight'], 1, 1, 1, 0, blk.xin.H, blk.xin.W)
        g, sums = dout, fused_in
        for d in reversed(range(self.bd)):
            self.dbg['g:' + blk.convs[d].relu] = g
            coef = self._bn_backward_coef(blk, d, g, sums)
            g, sums = self._layer_backward(blk, d, g, coef, dout, dxin, dxin_stats)
            self._maybe_flush(self.bwd)
        return sums

    def _bn_backward_coef(self, blk, d, g, sums):
        """Coefficients of the BatchNorm backward of layer d for incoming gradient g (None: no BatchNorm), from the sums
        g's producer left (live totals or partial rows) or from a statistics pass of its own; queues the BatchNorm parameter
        gradients and, for the block's last layer, the residual bias gradient (column sums of g)."""
        cv, G, bwd = blk.convs[d], self.G, self.bwd
        r, Cout = cv.r, cv.r.C
        res_bias = G[blk.prefix + '.res_conv1x1.bias'] if (self.do_res and d == self.bd - 1) else None
        if cv.bn is None:
            if res_bias is not None:
                self._colsum(bwd, g, res_bias)
            return None
        gamma, mean, invstd, bname = cv.bn
        if sums is not None and sums[0] == 'live':
            # live statistics: the producer of g added (sum g, sum g*r) to this layer's totals; the two consumers
            # of the coefficients derive A, B, C themselves, the parameter gradients leave with the next batched launch
            assert cv.live_bwd
            self._live_bwd_pending.append(dict(tot=sums[1], mean=mean, invstd=invstd, dgamma=G[bname + '.weight'],
                                               dbeta=G[bname + '.bias'], C=Cout, sum_out=res_bias))
            return dict(tot=sums[1], gamma=gamma, mean=mean, invstd=invstd, count=r.M)
        if sums is None:
            nb = self.lib.dfl_rowblock_count(r.M, Cout)
            part = self._new(nb * 2 * Cout)
            self._emit(bwd, ColstatsArgs(a=g.ptr, b=r.ptr, partials=part.data_ptr(), M=r.M, C=Cout, lda=g.ld,
                                         ldb=r.ld, nblocks=nb, bf16=r.bf16),
                       [_span(g), _span(r)], [_flat(part.data_ptr(), 4 * part.numel())])
            sums = (part, nb)
        part, prow = sums
        coef = self._new(3 * Cout)
        self.dbg['coef:' + cv.relu] = coef
        self._emit(bwd, BnBwdFinalizeArgs(partials=part.data_ptr(), gamma=gamma.data_ptr(),
                                  save_mean=mean.data_ptr(), save_invstd=invstd.data_ptr(),
                                  dgamma=G[bname + '.weight'].data_ptr(),
                                  dbeta=G[bname + '.bias'].data_ptr(), coef=coef.data_ptr(),
                                  count=r.M if self.training else 0,      # 0: fixed (running) statistics
                                  nblocks=prow, C=Cout),
                   [_flat(part.data_ptr(), 4 * part.numel())],
                   [_flat(coef.data_ptr(), 12 * Cout), _flat(G[bname + '.weight'].data_ptr(), 4 * Cout), _flat(G[bname + '.bias'].data_ptr(), 4 * Cout)])
        if res_bias is not None:
            # residual bias gradient = column sums of dout, already in the same partials
            self._defer_sum(bwd, part.data_ptr(), res_bias.data_ptr(), Cout, 2 * Cout, prow)
        return coef

    def _layer_backward(self, blk, d, g, coef, dout, dxin, dxin_stats):
        """Gradient emission of layer d for incoming gradient g: the BatchNorm + ReLU backward (written as dpre, or formed
        by its two consumers), the weight gradient and the data gradient -- into scratch for layer d-1, or for layer 0 into
        dxin, onto which the residual 1x1 data gradient accumulates.  Returns (the gradient written, the sums its producer
        left: BatchNorm-backward sums of layer d-1, or the column sums of dxin)."""
        cv, G, bwd, N = blk.convs[d], self.G, self.bwd, self.N
        r, inp, Cout, pad, circ = cv.r, cv.inp, cv.r.C, self.pad, self.circular
        # two dpre buffers alternate: a layer's dpre is never the buffer its incoming gradient lives in (the case when
        # _dz_for handed out 'dpre0' as the data gradient of a fused layer above)
        self._dpre_turn ^= 1
        if self._is_scratch(g.t, 'dpre%d' % self._dpre_turn):
            self._dpre_turn ^= 1
        # BatchNorm + ReLU backward folded into its two consumers (bf16 patch kernels; round 3): the weight-gradient
        # and data-gradient kernels form [r > 0] * (A dy + B r + C) from (dy, r) while they stage their patches --
        # dpre is never written (one tensor pass and one launch per layer less), the bias-gradient sums come out
        # of the weight-gradient kernel.  The 1-channel first layer (direct kernels) keeps the materialised form ...
        fuse_brb = self.FUSE_BRB and bool(r.bf16) and bool(inp.bf16) and inp.C % 16 == 0 and g.bf16 == r.bf16
        # ... but the network's first layer (1-channel fp32 input, no data gradient): the row form of the direct
        # weight-gradient kernel does the same while it reads its d rows
        if (self.FUSE_BRB and bool(r.bf16) and g.bf16 == r.bf16 and not inp.bf16 and inp.C == 1
                and d == 0 and dxin is None and Cout in (8, 16, 32, 64)):
            fuse_brb = True
        brb = (r, coef) if fuse_brb else None
        dsplit = 0
        if fuse_brb:
            dpre = g                          # what the consumers are given as their "d" / "x": dy itself
        else:
            dpre = self._scratch_act('dpre%d' % self._dpre_turn, N, r.H, r.W, Cout)
            nb = self.lib.dfl_rowblock_count(r.M, Cout)
            bpart = self._new(nb * Cout)
            # dpre feeds exactly two GEMMs (weight gradient: dense operand; data gradient: gathered operand);
            # with split-bf16 products it is written split once here instead of being split by every tile of both
            dsplit = int(self.math in (1, 3) and Cout % 16 == 0 and inp.C % 4 == 0 and inp.C * 9 > 12)
            self._emit(bwd, BnReluBwdArgs(dy=g.ptr, r=r.ptr, coef=nat.ptr(coef), dpre=dpre.ptr,
                                  partials=bpart.data_ptr(), M=r.M, C=Cout, lddy=g.ld, ldr=r.ld, ldo=dpre.ld,
                                  nblocks=nb, split_out=dsplit, bf16=r.bf16),
                       [_span(g), _span(r)] + ([_flat(coef.data_ptr(), 12 * Cout)] if coef is not None else []),
                       # (a split operand is laid out over the whole slot)
                       [_flat(dpre.t.data_ptr(), dpre.t.numel() * dpre.t.element_size()) if dsplit else _span(dpre),
                        _flat(bpart.data_ptr(), 4 * bpart.numel())])
            self._defer_sum(bwd, bpart.data_ptr(), G[cv.wname + '.bias'].data_ptr(), Cout, Cout, nb)
        # Small tensors (deep levels: many (cm, cg) tiles, each of which would form the operand again): the data-gradient
        # kernel, which forms it anyway, writes it once (x_out) and the weight gradient -- emitted BEHIND it -- reads it
        dmat = None
        if (fuse_brb and bool(inp.bf16) and not circ and pad == 1 and (d > 0 or dxin is not None)
                and 'dmat' in self._scratch and r.M * Cout * 2 <= self.DPRE_OUT_BYTES):
            dmat = self._scratch_act('dmat', N, r.H, r.W, Cout)
            self.dbg['dmat:' + cv.relu] = dmat
        if dmat is None:
            self._layer_wgrad(cv, dpre, d_split=dsplit, brb=brb)
        sums = None
        if circ and (d > 0 or dxin is not None):
            # data gradient on the framed grid, folded back onto the pixels the frame copies (see _wrap_pad)
            wd = self._pack_conv_dgrad(cv.w)
            dzp = self._framed_grad(inp)
            self._conv(bwd, dpre, wd, dzp, 3, 3, 1, 2, inp.C, x_split=dsplit, brb=brb)
            if d > 0:
                g = self._dz_for(g, N, inp.H, inp.W, Cout, fuse_brb)
                self._wrap_fold(bwd, dzp, g)
            else:
                self._wrap_fold(bwd, dzp, dxin)
                if self.do_res:
                    sums = self._conv(bwd, dout, self._pack_conv_dgrad(blk.rw), dxin, 1, 1, 1, 0, blk.xin.C,
                                      accumulate=1, stats=dxin_stats)
        elif d > 0:
            wd = self._pack_conv_dgrad(cv.w)
            dz = self._dz_for(g, N, inp.H, inp.W, Cout, fuse_brb)
            prev = blk.convs[d - 1]
            if prev.bn is not None:
                # the data-gradient conv leaves sum(dz), sum(dz*r) per channel for the next BN backward
                sums = self._conv(bwd, dpre, wd, dz, 3, 3, 1, 2 - pad, Cout, stats=True, stat_other=prev.r,
                                  x_split=dsplit, brb=brb, x_out=dmat,
                                  stat_totals=self._bn_totals(Cout, bwd=True) if prev.live_bwd else None)
            else:
                self._conv(bwd, dpre, wd, dz, 3, 3, 1, 2 - pad, Cout, x_split=dsplit, brb=brb, x_out=dmat)
            g = dz
        elif dxin is not None:
            # dxin = (3x3 data gradient of the first conv) + (1x1 data gradient of the residual branch).  The 3x3 one
            # writes, the cheap 1x1 one accumulates on top: the big kernel keeps its simple epilogue (and, on the wide
            # levels, the row-tiled form), the column sums of the finished dxin come from the 1x1 kernel.
            wd = self._pack_conv_dgrad(cv.w)
            sums = self._conv(bwd, dpre, wd, dxin, 3, 3, 1, 2 - pad, blk.xin.C,
                              x_split=dsplit, stats=dxin_stats and not self.do_res, brb=brb, x_out=dmat)
            if self.do_res:
                sums = self._conv(bwd, dout, self._pack_conv_dgrad(blk.rw), dxin, 1, 1, 1, 0, blk.xin.C,
                                  accumulate=1, stats=dxin_stats)
        if dmat is not None:
            self._layer_wgrad(cv, dmat, bias_plain=True)
        return g, sums

    def _layer_wgrad(self, cv, d, **kw):
        """Weight and bias gradient of a block's 3x3 layer cv from operand d: dpre, dy itself (brb), or the operand the data
        gradient materialised (bias_plain)."""
        self._wgrad(self.bwd, cv.gin, d, self.G[cv.wname + '.weight'], 3, 3, 1, 0 if self.circular else self.pad, cv.r.H, cv.r.W,
                    in_aff=cv.inp_aff, bias_out=self.G[cv.wname + '.bias'], **kw)

    def _finish_backward(self):
        """The last batched sums, and the zero fill of the backward totals arena in front of the program."""
        self._flush_sums(self.bwd)
        if self._deps is not None:
            # every op of a forked program has passed the tracker (the zero fill below leads the program: in front of every fork)
            if self._deps.seen != sum(1 for k in self.bwd.kinds if k not in (nat.OP_RECORD, nat.OP_WAIT)):
                raise PlanError('internal: a backward op was recorded past the dependency tracker')
        if self._tot_bwd[0] is not None:
            self.bwd.insert(0, MemsetArgs(ptr=self._tot_bwd[0].data_ptr(), bytes=8 * self._tot_bwd[1]))
            # every op index recorded while the program was emitted moved up by one (the flushes' indices
            # stayed behind and data-parallel buckets were cut one op early)
            self._red_flushes = [(idx + 1, dsts) for idx, dsts in self._red_flushes]

    def _grad_ready_ops(self):
        """Index of the last backward op that writes each parameter gradient (data-parallel bucket scheduling)."""
        by_ptr = {self.G[k].data_ptr(): k for k in self.grad_names}
        self.grad_ready_op = {}
        for idx, st in enumerate(self.bwd.structs):
            for field in ('dw', 'dst', 'out', 'dgamma', 'dbeta', 'dw_seg', 'dw_l1', 'dw_l2'):   # (dw_*: head_bwd's own weight gradients)
                name = by_ptr.get(getattr(st, field, None))
                if name is not None:
                    self.grad_ready_op[name] = idx
        for idx, dsts in self._red_flushes:
            for d in dsts:
                name = by_ptr.get(d)
                if name is not None:
                    self.grad_ready_op[name] = max(idx, self.grad_ready_op.get(name, -1))
        last = len(self.bwd.structs) - 1
        if self.g_l2_eff is not None:            # taken apart after the last op (unfold_tail_grads)
            for name in self.tail_names:
                self.grad_ready_op[name] = last
        if self.eff_heads is not None:
            for name in ('seg_conv.weight', 'lands_1x1.0.weight'):
                self.grad_ready_op[name] = last

    # ------------------------------------------------------------------------------------------ folded 1x1 tail
    def fold_tail(self):
        """w_l2_eff = W_k ... W_1 of the landmark 1x1 convolutions behind the first (tiny torch matmuls on the current stream)."""
        if self.eff_heads is not None:           # lands_block_depth > 0: widened head matrices (see the heads section)
            e = self.eff_heads
            F, F2 = e['F'], e['F2']
            e['w_seg'][:, :F].copy_(self.P['seg_conv.weight'])
            w1 = self.P['lands_1x1.0.weight']
            e['w_l1'][:, F:F + F2].copy_(w1[:, :F2])
            e['w_l1'][:, F + F2:].copy_(w1[:, F2:])
        if self.w_l2_eff is None:
            return
        mats = [self.P[n].view(self.P[n].shape[0], self.P[n].shape[1]) for n in self.tail_names]
        eff = mats[0]
        for m in mats[1:]:
            eff = m @ eff
        self.w_l2_eff.view(eff.shape).copy_(eff)

    def unfold_tail_grads(self):
        """Gradients of the folded 1x1 convolutions from the gradient of their product (see the heads section)."""
        if self.eff_heads is not None and self.need_grad:
            e = self.eff_heads
            F, F2 = e['F'], e['F2']
            if self.split_heads:                   # full-size segmentation call + the logits' path into the landmark call
                torch.add(self.g_seg_full, e['g_seg'][:, :F], out=self.G['seg_conv.weight'])
            else:
                self.G['seg_conv.weight'].copy_(e['g_seg'][:, :F])
            g1 = self.G['lands_1x1.0.weight']
            g1[:, :F2].copy_(e['g_l1'][:, F:F + F2])
            g1[:, F2:].copy_(e['g_l1'][:, F + F2:])
        if self.g_l2_eff is None:
            return
        mats = [self.P[n].view(self.P[n].shape[0], self.P[n].shape[1]) for n in self.tail_names]
        G = self.g_l2_eff.view(mats[-1].shape[0], mats[0].shape[1])
        k = len(mats)
        below = [None] * k                       # below[j] = W_{j-1} ... W_1 (None: identity)
        for j in range(1, k):
            below[j] = mats[j - 1] if below[j - 1] is None else mats[j - 1] @ below[j - 1]
        above = None                             # W_k ... W_{j+1}
        for j in reversed(range(k)):
            g = G if above is None else above.t() @ G
            if below[j] is not None:
                g = g @ below[j].t()
            self.G[self.tail_names[j]].view(g.shape).copy_(g)
            above = mats[j] if above is None else above @ mats[j]

    # ------------------------------------------------------------------------------------------ run
    def run_pack_rest(self, stream):
        """The pack program without its tiled launch: what is left to do after dfl_sgd_pack_tiled / dfl_optim_pack_tiled (optim.py)
        has written the tiled layouts together with the update."""
        i, n = self._tiled_index, len(self.pack)
        if i > 0:
            self.pack.run(stream, 0, i)
        if n - i - 1 > 0:
            self.pack.run(stream, i + 1, n - i - 1)

    def new_outputs(self):
        N = self.N
        h, w = self.out_hw
        hl, wl = self.heat_hw
        seg = torch.empty((N, self.NC, h, w), dtype=torch.float32, device=self.dev)
        heat = torch.empty((N, self.L, hl, wl), dtype=torch.float32, device=self.dev) if self.L > 0 else None
        return seg, heat

    def bind_outputs(self, seg, heat):
        """Point the head op(s) of the forward program at the caller-owned output tensors."""
        if self.split_heads:
            self.head_fwd_seg.seg = seg.data_ptr()
            self.head_fwd.seg = self.seg_crop.data_ptr()
        else:
            self.head_fwd.seg = seg.data_ptr()
        self.head_fwd.heat = nat.ptr(heat)

    def bind_grads(self, seg, dseg, dheat):
        """Point the head op(s) of the backward program at the forward's seg and the incoming gradients (dheat may be None)."""
        if self.split_heads:
            self.head_bwd_seg.seg, self.head_bwd_seg.dseg = seg.data_ptr(), dseg.data_ptr()
            self.head_bwd.seg, self.head_bwd.dseg = self.seg_crop.data_ptr(), self.dseg_zero.data_ptr()
        else:
            self.head_bwd.seg, self.head_bwd.dseg = seg.data_ptr(), dseg.data_ptr()
        self.head_bwd.dheat = nat.ptr(dheat)

    def grads(self):
        return [None if k in self.dead_params else self.G[k] for k in self.grad_names]

    def act_nchw(self, act):
        """Copy of an internal NHWC activation window as an fp32 NCHW tensor (introspection for tests and diagnosis)."""
        esz = act.esz
        base = act.t.view(-1)
        off = (act.ptr - base.data_ptr()) // esz
        v = base.as_strided((act.N, act.H, act.W, act.C), (act.H * act.W * act.ld, act.W * act.ld, act.ld, 1), off)
        return v.permute(0, 3, 1, 2).float().contiguous()
