"""Happens-before checker for recorded programs with side streams (include/dfl_hip.h, "Side streams").

unordered_conflicts(program) replays the executor's ordering rules on paper -- program order per stream, RECORD / WAIT, the fork
of a side stream's first op and nothing else -- and reports every pair of ops on different streams that touch the same bytes,
at least one of them writing, without being ordered.  What an op touches is derived here from its ARGUMENT STRUCT (pointers,
N, H, W, C, ld, element size), not from what the planner declared to its own tracker (plan._Fork): the two are meant to disagree
when one of them is wrong.  An op kind this module does not know touches everything, so it must be ordered against every op of
another stream -- which is also how the planner treats the ops it does not declare.
"""
import ctypes as C

from . import _native as nat

EVERYTHING = None


def _rows(ptr, rows, ld, width, esz):
    """Span (first, end, pitch, width) in bytes of `rows` rows of `width` elements with row stride ld."""
    if not ptr or rows <= 0 or width <= 0:
        return None
    pitch, wb = ld * esz, width * esz
    return (ptr, ptr + (rows - 1) * pitch + wb, pitch if wb < pitch else 0, wb)


def _bytes(ptr, n):
    return (ptr, ptr + n, 0, n) if ptr and n > 0 else None


def spans_meet(a, b):
    if a[0] >= b[1] or b[0] >= a[1]:
        return False
    if a[2] and a[2] == b[2]:                      # channel windows of rows with one pitch: compare the columns
        off = (a[0] - b[0]) % a[2]
        return off < b[3] or off + a[3] > a[2]
    return True


def _jobs(struct, job_type, host_jobs):
    arr = host_jobs.get(struct.jobs_dev) if host_jobs else None
    if arr is None:
        return None
    return [arr[k] for k in range(struct.njobs)]


def op_spans(st, kind, host_jobs=None):
    """(reads, writes) of one op as lists of spans, or EVERYTHING."""
    tot = 8 * nat.BN_R * 2                         # bytes per channel of a live-totals block [BN_R][2][C] of doubles
    rd, wr = [], []
    if isinstance(st, nat.MemsetArgs):
        wr.append(_bytes(st.ptr, st.bytes))
    elif isinstance(st, nat.ConvArgs):
        ex, ey = (2 if st.x_bf16 else 4), (2 if st.y_bf16 else 4)
        pin, pout = st.N * st.Hin * st.Win, st.N * st.Hout * st.Wout
        cy = st.Ntot // 4 if st.scatter2x2 else st.Ntot
        rd.append(_rows(st.x, pin, st.ldx, st.Cin, ex))
        if st.x_mode:
            rd.append(_rows(st.x2, pin, st.ldx2, st.Cin, ex))
            rd.append(_bytes(st.in_tot, tot * st.Cin) if st.in_tot else _bytes(st.in_scale, 12 * st.Cin))
        rd.append(_rows(st.add, pout, st.ldadd, st.Ntot, ey))
        rd.append(_rows(st.stat_other, pout, st.ldso, cy, ey))
        y = _rows(st.y, pout, st.ldy, cy, ey)
        wr.append(y)
        if st.accumulate:
            rd.append(y)
        wr.append(_rows(st.x_out, pin, st.ldxo, st.Cin, 2))
        if st.splits > 1:
            wr.append(_bytes(st.partial, 4 * st.splits * (pin if st.scatter2x2 else pout) * st.Ntot))
        if st.stat_partials:
            gm = nat.check(nat.lib().dfl_conv_grid_m(C.addressof(st)), 'dfl_conv_grid_m')
            wr.append(_bytes(st.stat_partials, 4 * gm * 2 * st.Ntot))      # ([4 gm][2][Ntot / 4] with scatter2x2: the same bytes)
        wr.append(_bytes(st.stat_totals, tot * cy))
    elif isinstance(st, nat.WgradArgs):
        eg, ed = (2 if st.g_bf16 else 4), (2 if st.d_bf16 else 4)
        pin, pout = st.N * st.Hin * st.Win, st.N * st.Hout * st.Wout
        n = st.Cm * st.Cg * st.KH * st.KW
        rd.append(_rows(st.g, pin, st.ldg, st.Cg, eg))
        rd.append(_rows(st.d, pout, st.ldd, st.Cm, ed))
        if st.d_mode:
            rd.append(_rows(st.d2, pout, st.ldd2, st.Cm, ed))
            rd.append(_bytes(st.coef_tot, tot * st.Cm) if st.coef_tot else _bytes(st.coef, 12 * st.Cm))
        s = max(st.splits, 1)
        wr.append(_bytes(st.partial, 4 * s * n) if s > 1 else _bytes(st.dw, 4 * n))
        wr.append(_bytes(st.bias_partial, 4 * s * st.Cm))
    elif isinstance(st, nat.ReduceBatchArgs):
        jobs = _jobs(st, nat.ReduceJob, host_jobs)
        if jobs is None:
            return EVERYTHING
        for j in jobs:
            rd.append(_bytes(j.src, 4 * ((j.count - 1) * j.stride + j.n)))
            wr.append(_bytes(j.dst, 4 * j.n))
    elif isinstance(st, nat.BnBwdLiveArgs):
        jobs = _jobs(st, nat.BnBwdLiveJob, host_jobs)
        if jobs is None:
            return EVERYTHING
        for j in jobs:
            rd += [_bytes(j.totals, tot * j.C), _bytes(j.save_mean, 4 * j.C), _bytes(j.save_invstd, 4 * j.C)]
            wr += [_bytes(j.dgamma, 4 * j.C), _bytes(j.dbeta, 4 * j.C), _bytes(j.sum_out, 4 * j.C)]
    elif isinstance(st, nat.ColstatsArgs):
        e = 2 if st.bf16 else 4
        rd += [_rows(st.a, st.M, st.lda, st.C, e), _rows(st.b, st.M, st.ldb, st.C, e)]
        wr.append(_bytes(st.partials, 4 * st.nblocks * 2 * st.C))
    elif isinstance(st, nat.BnBwdFinalizeArgs):
        rd.append(_bytes(st.partials, 4 * st.nblocks * 2 * st.C))
        wr += [_bytes(st.dgamma, 4 * st.C), _bytes(st.dbeta, 4 * st.C), _bytes(st.coef, 12 * st.C)]
    elif isinstance(st, nat.BnReluBwdArgs):
        e = 2 if st.bf16 else 4
        rd += [_rows(st.dy, st.M, st.lddy, st.C, e), _rows(st.r, st.M, st.ldr, st.C, e), _bytes(st.coef, 12 * st.C)]
        wr += [_rows(st.dpre, st.M, st.ldo, st.C, e), _bytes(st.partials, 4 * st.nblocks * st.C)]
    else:
        return EVERYTHING
    return [s for s in rd if s is not None], [s for s in wr if s is not None]


def _conflict(a, b):
    """a, b: (reads, writes) or EVERYTHING."""
    if a is EVERYTHING or b is EVERYTHING:
        return True
    (ra, wa), (rb, wb) = a, b
    return (any(spans_meet(x, y) for x in wa for y in rb + wb) or any(spans_meet(x, y) for x in ra for y in wb))


def unordered_conflicts(prog, start=0, count=None, spans=None, host_jobs=None, n_streams=nat.MAX_SIDE_STREAMS + 1):
    """[(i, j)]: ops i < j of range [start, start + count) on different streams that conflict and are not ordered.
    spans: index -> (reads, writes) to use instead of op_spans (hand-written lists)."""
    end = len(prog) if count is None else start + count
    clock = [[0] * n_streams for _ in range(n_streams)]      # clock[s][t]: ops of stream t that stream s is ordered behind
    used = [False] * n_streams
    events = {}
    ops = []                                                 # (index, stream, clock behind the op, spans)
    for i in range(start, end):
        s, kind, st = prog.streams[i], prog.kinds[i], prog.structs[i]
        if s != 0 and not used[s]:
            used[s] = True
            clock[s] = [max(a, b) for a, b in zip(clock[s], clock[0])]      # fork: behind the caller's stream as it stands
        if kind == nat.OP_RECORD:
            events[st.event] = list(clock[s])
        elif kind == nat.OP_WAIT:
            if st.event in events:                            # (recorded in an earlier range: skipped by the executor)
                clock[s] = [max(a, b) for a, b in zip(clock[s], events[st.event])]
        else:
            clock[s][s] += 1
            sp = spans[i] if spans is not None and i in spans else op_spans(st, kind, host_jobs)
            ops.append((i, s, list(clock[s]), sp))
    bad = []
    for b in range(len(ops)):
        j, sj, cj, spj = ops[b]
        for a in range(b):
            i, si, ci, spi = ops[a]
            if si != sj and cj[si] < ci[si] and _conflict(spi, spj):
                bad.append((i, j))
    return bad
