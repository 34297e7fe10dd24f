"""The forked backward program on the GPU: weight gradients and batched sums on a branch of the backward hipGraph.

For every shape below two networks are built from one seed, one with the serial planner (UNetPlan.FORK = False: the program as it
was before the fork existed) and one with the forked planner, and both take three training steps on the same batch.  Nothing a
branch computes depends on WHEN it runs, so every comparison here is for equal bits.

Shapes: the paper preset at 64 x 64 batch 2 (levels down to 2 x 2) and 96 x 96 batch 3 (odd patch edges), and a depth-3 net at
32 x 32 with the residual branch and BatchNorm on and off, and with circular padding, which is forked through the same tracker.
The depth-3 net has wf = 3 in fp32 and wf = 4 in bf16 storage: that arithmetic takes channel counts that are multiples of 16.
"""
import functools

import pytest
import torch

import dfl_amd
from dfl_amd import _native as nat
from dfl_amd import hazards
from dfl_amd.plan import UNetPlan

pytestmark = pytest.mark.gpu

PAPER = dict(n_classes=7, depth=6, wf=5, batch_norm=True, padding=True, max_pool=False, num_lands=14, do_res=True, block_depth=2)
D3 = dict(n_classes=7, depth=3, batch_norm=True, padding=True, max_pool=False, num_lands=14, do_res=True, block_depth=2)
CASES = {
    'paper64b2': (PAPER, 2, 64),
    'paper96b3': (PAPER, 3, 96),
    'd3': (D3, 2, 32),
    'd3_nores': (dict(D3, do_res=False), 2, 32),
    'd3_nobn': (dict(D3, batch_norm=False), 2, 32),
    'd3_nores_nobn': (dict(D3, do_res=False, batch_norm=False), 2, 32),
    'd3_circular': (dict(D3, pad_mode='circular'), 2, 32),
}
MODES = {'bf16s': 4, 'fp32': 0}
SYNC = (nat.OP_RECORD, nat.OP_WAIT)


def _batch(N, H, dev):
    g = torch.Generator().manual_seed(17)
    x = torch.randn(N, 1, H, H, generator=g)
    lab = torch.randint(0, 7, (N, H - 4, H - 4), generator=g)
    tseg = torch.nn.functional.one_hot(lab, 7).permute(0, 3, 1, 2).float().contiguous()
    theat = torch.rand(N, 14, H - 4, H - 4, generator=g) * 0.02
    return x.to(dev), tseg.to(dev), theat.to(dev)


def _train(cfg, N, H, fork, steps=3):
    """Three SGD steps of a fresh network; returns what they computed and the network (its training plan alive)."""
    old = UNetPlan.FORK
    UNetPlan.FORK = fork
    try:
        torch.manual_seed(5)
        net = dfl_amd.UNet(1, **cfg).to('cuda').train()
        opt = torch.optim.SGD(net.parameters(), lr=0.05, momentum=0.9)
        crit = dfl_amd.DiceAndHeatMapLoss2D(skip_bg=False, heatmap_wgt=0.5)
        x, tseg, theat = _batch(N, H, 'cuda')
        out = {}
        for k in range(steps):
            opt.zero_grad(set_to_none=True)
            seg, heat = net(x)
            loss = crit((dfl_amd.center_crop(seg, tseg.shape), dfl_amd.center_crop(heat, theat.shape)), (tseg, theat))
            loss.backward()
            out['seg%d' % k], out['heat%d' % k], out['loss%d' % k] = seg.detach().clone(), heat.detach().clone(), loss.detach().clone()
            for name, p in net.named_parameters():
                if p.grad is not None:
                    out['grad%d:%s' % (k, name)] = p.grad.detach().clone()
            opt.step()
            for name, p in net.named_parameters():
                out['param%d:%s' % (k, name)] = p.detach().clone()
        torch.cuda.synchronize()
        plan = net._last_train_plan()
        assert (plan._deps is not None) == fork
        return out, net, plan, (x, tseg, theat)
    finally:
        UNetPlan.FORK = old


@functools.lru_cache(maxsize=None)
def _pair(case, mode):
    cfg, N, H = CASES[case]
    if 'wf' not in cfg:
        cfg = dict(cfg, wf=4 if mode == 'bf16s' else 3)
    lib = nat.lib()
    prev = lib.dfl_get_math_mode()
    nat.check(lib.dfl_set_math_mode(MODES[mode]), 'dfl_set_math_mode')
    try:
        serial = _train(cfg, N, H, False)
        forked = _train(cfg, N, H, True)
        # one more forward of the forked network, its backward bound to fixed output gradients: the replays below start here
        out, net, plan, (x, _, _) = forked
        seg, heat = net(x)
        g = torch.Generator().manual_seed(23)
        hold = (torch.randn(seg.shape, generator=g).to('cuda') * 1e-3, torch.randn(heat.shape, generator=g).to('cuda') * 1e-3)
        plan.bind_grads(seg, hold[0], hold[1])
        stream = torch.cuda.current_stream().cuda_stream
        net.run_program(plan, plan.bwd, stream)
        torch.cuda.synchronize()
        ref = plan.grad_flat.clone()
    finally:
        nat.check(lib.dfl_set_math_mode(prev), 'dfl_set_math_mode')
    return dict(serial=serial, forked=forked, ref=ref, hold=(seg, heat) + hold, stream=stream)


ALL = [(c, m) for c in CASES for m in MODES]


@pytest.fixture(autouse=True, scope='module')
def _drop_networks():
    yield
    _pair.cache_clear()


def _stale(plan, ref, upto=None):
    """Names of the live gradients (those complete behind op `upto`) whose bits differ from ref."""
    bad = []
    for k, v in plan.grad_ready_op.items():
        if k in plan.dead_params or (upto is not None and v > upto):
            continue
        o, n = (plan.G[k].data_ptr() - plan.grad_flat.data_ptr()) // 4, plan.P[k].numel()
        if not torch.equal(plan.grad_flat[o:o + n], ref[o:o + n]):
            bad.append(k)
    return bad


@pytest.mark.parametrize('case,mode', ALL)
def test_checker_passes_on_the_recorded_programs(case, mode):
    """(a) No unordered conflict in the forward and backward training programs as recorded on the device, whole and cut at the
    data-parallel bucket boundaries; the serial plan has no side-stream op at all."""
    st = _pair(case, mode)
    plan, splan = st['forked'][2], st['serial'][2]
    assert all(s == 0 for s in splan.bwd.streams) and not any(k in SYNC for k in splan.bwd.kinds)
    assert [k for k in plan.bwd.kinds if k not in SYNC] == splan.bwd.kinds
    assert any(s == 1 for s in plan.bwd.streams) and all(s == 0 for s in plan.fwd.streams)
    for prog in (plan.fwd, plan.bwd):
        assert hazards.unordered_conflicts(prog, host_jobs=plan.host_jobs) == []
    for cut in sorted(set(plan.grad_ready_op.values())):
        assert hazards.unordered_conflicts(plan.bwd, 0, cut + 1, host_jobs=plan.host_jobs) == []


@pytest.mark.parametrize('case,mode', ALL)
def test_three_steps_equal_the_serial_program_bit_for_bit(case, mode):
    """(b) seg, heat, loss, every gradient and every updated parameter of three steps."""
    st = _pair(case, mode)
    a, b = st['serial'][0], st['forked'][0]
    assert set(a) == set(b) and any(k.startswith('grad2:') for k in a)
    diff = [k for k in a if not torch.equal(a[k], b[k])]
    assert not diff, '%d of %d tensors differ: %s' % (len(diff), len(a), diff[:6])


@pytest.mark.parametrize('case,mode', ALL)
def test_replays_are_bit_stable_graphed_and_op_by_op(case, mode):
    """(b, c) The forked backward replayed 20 times as hipGraphs gives the same gradient arena every time, and the op-by-op
    replay (dfl_exec: real streams and events) gives the same bits as the graph."""
    st = _pair(case, mode)
    _, net, plan, _ = st['forked']
    stream, ref = st['stream'], st['ref']
    assert net.graphs_on(plan)
    for k in range(20):
        plan.grad_flat.fill_(float('nan'))
        net.run_program(plan, plan.bwd, stream)
        assert not _stale(plan, ref), 'graphed replay %d differs' % k
    for k in range(3):
        plan.grad_flat.fill_(float('nan'))
        plan.bwd.run(stream)
        assert not _stale(plan, ref), 'op-by-op replay %d differs from the graph' % k


@pytest.mark.parametrize('case,mode', ALL)
def test_one_graph_per_run_and_ranges_leave_final_gradients(case, mode):
    """(d) Forks and joins do not cut the backward hipGraph: as many graphs, with as many nodes, as the serial program has.
    A range replay up to a bucket cut leaves every gradient of the earlier buckets final over a NaN-filled arena."""
    st = _pair(case, mode)
    (_, net, plan, _), (_, snet, splan, _) = st['forked'], st['serial']
    stream, ref = st['stream'], st['ref']
    chunks, schunks = plan.bwd.graph_chunks(stream), splan.bwd.graph_chunks(stream)
    runs = sum(1 for i in range(len(plan.bwd)) if not plan.bwd.volatile[i] and (i == 0 or plan.bwd.volatile[i - 1]))
    assert len([g for _, _, g in chunks if g is not None]) == len([g for _, _, g in schunks if g is not None]) <= runs
    assert [g.nodes for _, _, g in chunks if g is not None] == [g.nodes for _, _, g in schunks if g is not None]
    assert all(g is not None or all(plan.bwd.volatile[f:f + c]) or c < 2 for f, c, g in chunks)
    ready = {k: v for k, v in plan.grad_ready_op.items() if k not in plan.dead_params}
    cuts = sorted(set(ready.values()))
    for cut in (cuts[len(cuts) // 3], cuts[2 * len(cuts) // 3]):
        plan.grad_flat.fill_(float('nan'))
        net.run_program(plan, plan.bwd, stream, 0, cut + 1)
        torch.cuda.synchronize()
        assert not _stale(plan, ref, cut), 'not final behind op %d' % cut
        net.run_program(plan, plan.bwd, stream, cut + 1, len(plan.bwd) - cut - 1)
        torch.cuda.synchronize()
        assert not _stale(plan, ref)
