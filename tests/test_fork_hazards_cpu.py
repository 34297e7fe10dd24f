"""The happens-before checker of forked programs (dfl_amd.hazards) on hand-written op lists, and on the planner's programs.

Nothing is launched: the checker reads argument structs, streams and RECORD / WAIT ops.  The lists below use made-up
addresses; a list with a missing wait must be flagged, the corrected one must pass, and the executor's own rules (the fork of
a side stream's first op, the join at the end of a range, a WAIT for an event of an earlier range) are honoured as
include/dfl_hip.h states them.
"""
import pytest
import torch

import dfl_amd
from dfl_amd import _native as nat
from dfl_amd import hazards
from dfl_amd.plan import UNetPlan

A, B, P, Q = 0x100000, 0x200000, 0x300000, 0x400000      # made-up device addresses, 1 MB apart


def fill(ptr, nbytes=4096):
    """An op that WRITES [ptr, ptr + nbytes)."""
    return nat.MemsetArgs(ptr=ptr, bytes=nbytes)


def colsum(src, part, M=16, C=16, ld=16):
    """An op that READS M rows of C floats at src (row stride ld) and WRITES its partial rows at part."""
    return nat.ColstatsArgs(a=src, b=None, partials=part, M=M, C=C, lda=ld, ldb=0, nblocks=1, bf16=0)


def program(ops):
    """ops: (struct, stream) | ('record', event, stream) | ('wait', event, stream)."""
    p = nat.Program()
    for op in ops:
        if op[0] == 'record':
            p.record(op[1], op[2])
        elif op[0] == 'wait':
            p.wait(op[1], op[2])
        else:
            p.add(op[0], stream=op[1])
    return p


def test_missing_wait_is_flagged_and_the_corrected_list_passes():
    # the branch reads A while the main chain moves on and rewrites it: write-after-read
    racy = [(fill(A), 0), (colsum(A, P), 1), (fill(B), 0), (fill(A), 0)]
    assert hazards.unordered_conflicts(program(racy)) == [(1, 3)]
    fixed = [(fill(A), 0), (colsum(A, P), 1), ('record', 0, 1), (fill(B), 0), ('wait', 0, 0), (fill(A), 0)]
    assert hazards.unordered_conflicts(program(fixed)) == []
    # a wait for the wrong event, or on the wrong stream, orders nothing
    wrong = [(fill(A), 0), (colsum(A, P), 1), ('record', 0, 1), (fill(B), 0), ('wait', 1, 0), (fill(A), 0)]
    assert hazards.unordered_conflicts(program(wrong)) == [(1, 5)]
    wrong = [(fill(A), 0), (colsum(A, P), 1), ('record', 0, 1), (fill(B), 0), ('wait', 0, 2), (fill(A), 0)]
    assert hazards.unordered_conflicts(program(wrong)) == [(1, 5)]
    # a record placed in FRONT of the reader does not cover it
    early = [(fill(A), 0), ('record', 0, 1), (colsum(A, P), 1), ('wait', 0, 0), (fill(A), 0)]
    assert hazards.unordered_conflicts(program(early)) == [(2, 4)]


def test_every_kind_of_conflict_and_only_conflicts():
    # read-after-write: the main chain reads what the branch wrote
    assert hazards.unordered_conflicts(program([(colsum(A, P), 1), (colsum(P, Q, M=1, C=32, ld=32), 0)])) == [(0, 1)]
    # write-after-write
    assert hazards.unordered_conflicts(program([(colsum(A, P), 1), (fill(P, 64), 0)])) == [(0, 1)]
    # two readers of one tensor, writers of different ones: nothing to order
    assert hazards.unordered_conflicts(program([(colsum(A, P), 1), (colsum(A, Q), 0)])) == []
    # one stream: program order
    assert hazards.unordered_conflicts(program([(colsum(A, P), 1), (fill(A), 1), (fill(P), 1)])) == []
    # the two channel halves of a concat buffer (rows of 32 floats, 16 each) do not meet; overlapping windows do
    lo, hi = colsum(A, P, C=16, ld=32), nat.ColstatsArgs(a=B, b=None, partials=A + 64, M=1, C=8, lda=8, ldb=0, nblocks=1, bf16=0)
    assert hazards.unordered_conflicts(program([(lo, 1), (hi, 0)])) == [(0, 1)]           # hi writes 64 bytes at A + 64: the other half ...
    spans = {0: ([(A, A + 15 * 128 + 64, 128, 64)], []), 1: ([], [(A + 64, A + 64 + 15 * 128 + 64, 128, 64)])}
    assert hazards.unordered_conflicts(program([(lo, 1), (hi, 0)]), spans=spans) == []    # ... as a strided window of the same rows: disjoint
    spans[1] = ([], [(A + 32, A + 32 + 15 * 128 + 64, 128, 64)])
    assert hazards.unordered_conflicts(program([(lo, 1), (hi, 0)]), spans=spans) == [(0, 1)]
    # an op kind the checker does not know touches everything
    pool = nat.PoolArgs(x=Q, y=Q, dx=Q, N=1, H=2, W=2, C=4, ldx=4, ldy=4, lddx=4)
    p = nat.Program()
    p.add(colsum(A, P), stream=1)
    p.add(pool, nat.OP_POOL_BWD)
    assert hazards.unordered_conflicts(p) == [(0, 1)]


def test_the_executors_fork_and_range_rules():
    # a side stream's first op starts behind the main chain as it stands: no RECORD / WAIT needed for what came before
    assert hazards.unordered_conflicts(program([(fill(A), 0), (colsum(A, P), 1)])) == []
    # ... but only its FIRST op: later ones need their own order
    racy = [(colsum(B, Q), 1), (fill(A), 0), (colsum(A, P), 1)]
    assert hazards.unordered_conflicts(program(racy)) == [(1, 2)]
    fixed = [(colsum(B, Q), 1), (fill(A), 0), ('record', 3, 0), ('wait', 3, 1), (colsum(A, P), 1)]
    assert hazards.unordered_conflicts(program(fixed)) == []
    # two side streams are ordered against each other like any two streams
    assert hazards.unordered_conflicts(program([(fill(A), 1), (colsum(A, P), 2)])) == [(0, 1)]
    assert hazards.unordered_conflicts(program([(fill(A), 1), ('record', 0, 1), ('wait', 0, 2), (colsum(A, P), 2)])) == []
    # ranges: every range is joined at its end, so a cut between a reader and the later writer orders them; the wait whose
    # event was recorded in the earlier range is skipped, and the range it sits in is still whole
    full = program([(fill(A), 0), (colsum(A, P), 1), ('record', 0, 1), (fill(B), 0), ('wait', 0, 0), (fill(A), 0),
                    ('record', 1, 0), ('wait', 1, 1), (colsum(A, Q), 1)])
    assert hazards.unordered_conflicts(full) == []
    for cut in range(1, len(full)):
        assert hazards.unordered_conflicts(full, 0, cut) == [] and hazards.unordered_conflicts(full, cut, len(full) - cut) == []
    # a wait for an event that was never recorded in the range orders nothing inside it
    stale = program([(fill(A), 0), (colsum(A, P), 1), ('wait', 9, 0), (fill(A), 0)])
    assert hazards.unordered_conflicts(stale) == [(1, 3)]


def test_spans_come_from_the_argument_structs():
    """Extents of the two gradient ops: pixels x pitch from N, H, W, C, ld and the element size, partial slices from splits."""
    c = nat.ConvArgs(x=A, y=B, x2=P, x_mode=1, x_out=Q, ldxo=32, N=2, Hin=5, Win=7, Cin=32, ldx=64, ldx2=32, KH=3, KW=3, stride=1, pad=1,
                     Hout=5, Wout=7, Ntot=16, ldy=16, x_bf16=1, y_bf16=1, in_scale=0x500000)
    rd, wr = hazards.op_spans(c, nat.OP_CONV)
    assert (A, A + 69 * 128 + 64, 128, 64) in rd and (P, P + 70 * 64, 0, 64) in rd and (0x500000, 0x500000 + 12 * 32, 0, 12 * 32) in rd
    assert (B, B + 70 * 32, 0, 32) in wr and (Q, Q + 70 * 64, 0, 64) in wr and len(wr) == 2
    w = nat.WgradArgs(g=A, d=B, dw=P, partial=Q, bias_partial=0x500000, N=2, Hin=5, Win=7, Cg=16, ldg=16, KH=3, KW=3, stride=1, pad=1,
                      Hout=5, Wout=7, Cm=32, ldd=64, splits=3, g_bf16=1, d_bf16=1)
    rd, wr = hazards.op_spans(w, nat.OP_WGRAD)
    assert rd == [(A, A + 70 * 32, 0, 32), (B, B + 69 * 128 + 64, 128, 64)]
    assert wr == [(Q, Q + 4 * 3 * 32 * 16 * 9, 0, 4 * 3 * 32 * 16 * 9), (0x500000, 0x500000 + 4 * 3 * 32, 0, 4 * 3 * 32)]
    w.splits = 1
    assert hazards.op_spans(w, nat.OP_WGRAD)[1][0] == (P, P + 4 * 32 * 16 * 9, 0, 4 * 32 * 16 * 9)


CASES = [
    ('paper 64x64 b2', dict(n_classes=7, depth=6, wf=5, batch_norm=True, padding=True, max_pool=False, num_lands=14, do_res=True, block_depth=2), 2, 64),
    ('paper 96x96 b3', dict(n_classes=7, depth=6, wf=5, batch_norm=True, padding=True, max_pool=False, num_lands=14, do_res=True, block_depth=2), 3, 96),
    ('d3 res bn', dict(n_classes=5, depth=3, wf=4, batch_norm=True, padding=True, max_pool=False, do_res=True, block_depth=2), 2, 32),
    ('d3 nores nobn pool', dict(n_classes=5, depth=3, wf=4, batch_norm=False, padding=True, max_pool=True, do_res=False, block_depth=2), 2, 32),
    ('d3 circular', dict(n_classes=5, depth=3, wf=4, batch_norm=True, padding=True, pad_mode='circular', max_pool=False, do_res=True, block_depth=2), 2, 32),
    ('d3 valid upsample', dict(n_classes=5, depth=3, wf=4, batch_norm=True, padding=False, max_pool=True, do_res=False, block_depth=1, up_mode='upsample'), 2, 44),
]


@pytest.mark.parametrize('mode', [0, 4])
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_planned_programs_pass_and_need_every_wait_they_hold(case, mode, monkeypatch):
    """The forked backward program of a training plan (addresses only: recorded on the CPU) has no unordered conflict, is the
    serial program plus streams and RECORD / WAIT ops, and holds no wait on the main chain that the checker can do without."""
    _, cfg, N, H = case
    lib = nat.lib()
    prev = lib.dfl_get_math_mode()
    nat.check(lib.dfl_set_math_mode(mode), 'dfl_set_math_mode')
    try:
        net = dfl_amd.UNet(1, **cfg)
        Pm, Bf = net._state()
        monkeypatch.setattr(UNetPlan, 'FORK', False)
        serial = UNetPlan(net._cfg, Pm, Bf, N, H, H, True, True, torch.device('cpu'))
        monkeypatch.setattr(UNetPlan, 'FORK', True)
        plan = UNetPlan(net._cfg, Pm, Bf, N, H, H, True, True, torch.device('cpu'))
    finally:
        nat.check(lib.dfl_set_math_mode(prev), 'dfl_set_math_mode')
    sync = (nat.OP_RECORD, nat.OP_WAIT)
    assert all(s == 0 for s in serial.bwd.streams + serial.fwd.streams + plan.fwd.streams) and not any(k in sync for k in serial.bwd.kinds)
    real = [i for i, k in enumerate(plan.bwd.kinds) if k not in sync]
    assert [plan.bwd.kinds[i] for i in real] == serial.bwd.kinds
    assert [type(plan.bwd.structs[i]) for i in real] == [type(s) for s in serial.bwd.structs]
    branch = [i for i in real if plan.bwd.streams[i] != 0]
    assert branch and all(plan.bwd.streams[i] == 1 for i in branch)
    assert all(isinstance(plan.bwd.structs[i], (nat.WgradArgs, nat.ReduceBatchArgs, nat.BnBwdLiveArgs)) for i in branch)
    assert sum(isinstance(s, nat.WgradArgs) for s in plan.bwd.structs) == sum(1 for i in branch if isinstance(plan.bwd.structs[i], nat.WgradArgs))
    for prog in (plan.fwd, plan.bwd):
        assert hazards.unordered_conflicts(prog, host_jobs=plan.host_jobs) == []
    # every range is a whole program of its own (data-parallel bucket cuts)
    ready = sorted(set(plan.grad_ready_op.values()))
    for cut in ready[:: max(1, len(ready) // 6)]:
        assert hazards.unordered_conflicts(plan.bwd, 0, cut + 1, host_jobs=plan.host_jobs) == []
        assert hazards.unordered_conflicts(plan.bwd, cut + 1, len(plan.bwd) - cut - 1, host_jobs=plan.host_jobs) == []
    # without any one of its main-chain waits the program races
    waits = [i for i, (k, s) in enumerate(zip(plan.bwd.kinds, plan.bwd.streams)) if k == nat.OP_WAIT and s == 0]
    for i in waits:
        q = nat.Program()
        for j in range(len(plan.bwd)):
            if j != i:
                q.add(plan.bwd.structs[j], plan.bwd.kinds[j], plan.bwd.streams[j])
        assert hazards.unordered_conflicts(q, host_jobs=plan.host_jobs), 'main-chain wait at op %d orders nothing' % i
