"""dfl_amd.Adam / dfl_amd.RMSprop on the GPU (the reference's --optim adam|rmsprop, train.py:331-352): the flat kernels against
an fp64 restatement of torch's formulas, the optimizers against torch.optim on the same gradients (one launch per contiguous
run), the update inside the tiled weight re-layout bit-identical to update launches followed by the re-layout, state dicts
moving both ways between torch.optim and these classes, and train.py --optim adam|rmsprop with a resume."""
import io
import os

import numpy as np
import pytest
import torch

import dfl_amd
from dfl_amd import _native as nat
import noise_floor as NF
import problems as PR
from gpu_common import hip_net, hip_step, math_mode_set

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CFG = dict(n_classes=4, depth=3, wf=3, batch_norm=True, padding=True, max_pool=False, num_lands=3)
DEAD = 'downsample_convs.2.weight'         # the never-used last down-sampling convolution: no gradient, no state
# (name, ours, torch's, constructor arguments, state keys)
KINDS = {
    'adam': (dfl_amd.Adam, torch.optim.Adam, dict(lr=1e-3, weight_decay=1e-3), ('exp_avg', 'exp_avg_sq')),
    'rmsprop_mom': (dfl_amd.RMSprop, torch.optim.RMSprop, dict(lr=1e-3, weight_decay=1e-3, momentum=0.9),
                    ('square_avg', 'momentum_buffer')),
    'rmsprop': (dfl_amd.RMSprop, torch.optim.RMSprop, dict(lr=1e-3, weight_decay=1e-3), ('square_avg',)),
}
STEP_FN = {'adam': 'dfl_adam_step', 'rmsprop_mom': 'dfl_rmsprop_step', 'rmsprop': 'dfl_rmsprop_step'}


class Spy:
    """Counts the calls (and records the arguments) of some library entry points, forwards everything."""
    def __init__(self, real, names):
        self._real, self.calls = real, {k: [] for k in names}

    def __getattr__(self, k):
        f = getattr(self._real, k)
        if k in self.calls:
            def counted(*a):
                self.calls[k].append(a)
                return f(*a)
            return counted
        return f


# ---- 1. kernels against an fp64 restatement of torch's _multi_tensor_adam / _multi_tensor_rmsprop -----------------------
def _close(actual, ref, what):
    """relative 1e-5 per element, with a floor of 1e-6 of the tensor's largest value (elements that cancel to near zero)"""
    a, r = actual.detach().double().cpu().numpy(), np.asarray(ref)
    bar = 1e-5 * np.abs(r) + 1e-6 * np.abs(r).max()
    bad = np.abs(a - r) > bar
    assert not bad.any(), '%s: %d elements off, worst rel %.3e' % (what, int(bad.sum()), float((np.abs(a - r) / (np.abs(r) + 1e-30)).max()))


def test_adam_kernel_matches_fp64_formulas():
    n, lr, b1, b2, eps, wd, gs = 1003, 1e-2, 0.9, 0.999, 1e-8, 1e-2, 0.5
    g = torch.Generator().manual_seed(11)
    p = torch.randn(n, generator=g)
    m, v = torch.zeros(n), torch.zeros(n)
    P, M, V = p.double().numpy().copy(), m.double().numpy().copy(), v.double().numpy().copy()
    pd, md, vd = p.to(DEV), m.to(DEV), v.to(DEV)
    lib = nat.lib()
    for t in range(1, 6):
        gr = torch.randn(n, generator=g)
        grd = gr.to(DEV)
        step_size, bc2 = lr / (1 - b1 ** t), (1 - b2 ** t) ** 0.5
        nat.check(lib.dfl_adam_step(pd.data_ptr(), grd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, lr, b1, b2, eps, wd, step_size,
                                    bc2, gs, None), 'dfl_adam_step')
        G = gr.double().numpy() * gs + wd * P
        M = M + (1 - b1) * (G - M)
        V = b2 * V + (1 - b2) * G * G
        P = P - step_size * M / (np.sqrt(V) / bc2 + eps)
    torch.cuda.synchronize()
    _close(pd, P, 'p')
    _close(md, M, 'exp_avg')
    _close(vd, V, 'exp_avg_sq')


@pytest.mark.parametrize('mom', [0.0, 0.9])
def test_rmsprop_kernel_matches_fp64_formulas(mom):
    n, lr, alpha, eps, wd, gs = 1003, 1e-3, 0.99, 1e-8, 1e-2, 2.0
    g = torch.Generator().manual_seed(12)
    p = torch.randn(n, generator=g)
    P, S, B = p.double().numpy().copy(), np.zeros(n), np.zeros(n)
    pd, sd = p.to(DEV), torch.zeros(n, device=DEV)
    bd = torch.zeros(n, device=DEV) if mom else None
    lib = nat.lib()
    for t in range(1, 6):
        gr = torch.randn(n, generator=g)
        grd = gr.to(DEV)
        nat.check(lib.dfl_rmsprop_step(pd.data_ptr(), grd.data_ptr(), sd.data_ptr(), None if bd is None else bd.data_ptr(), n, lr,
                                       alpha, eps, wd, mom, gs, None), 'dfl_rmsprop_step')
        G = gr.double().numpy() * gs + wd * P
        S = alpha * S + (1 - alpha) * G * G
        avg = np.sqrt(S) + eps
        if mom:
            B = mom * B + G / avg
            P = P - lr * B
        else:
            P = P - lr * G / avg
    torch.cuda.synchronize()
    _close(pd, P, 'p')
    _close(sd, S, 'square_avg')
    if mom:
        _close(bd, B, 'momentum_buffer')


# ---- 2. against torch.optim on a network, on the same gradients ------------------------------------------------------
def _grads_into(src, dst):
    for pa, pb in zip(src.parameters(), dst.parameters()):
        pb.grad = None if pa.grad is None else pa.grad.detach().clone()


def _forward_backward(net, x):
    for p in net.parameters():
        p.grad = None
    seg, heat = net(x)
    (seg.square().mean() + heat.square().mean()).backward()


def _assert_same(na, oa, nb, ob, keys):
    """rtol 2e-5, atol 2e-6 -- for the state tensors atol 2e-6 of the tensor's largest value: RMSprop's momentum buffer holds
    sums of g / sqrt(square_avg) of magnitude 10 and more, where one fp32 rounding of a cancelling sum is already 1e-6"""
    for (k, pa), pb in zip(na.named_parameters(), nb.parameters()):
        np.testing.assert_allclose(pa.detach().cpu().numpy(), pb.detach().cpu().numpy(), rtol=2e-5, atol=2e-6, err_msg=k)
        if pa in oa.state:
            for s in keys:
                ref = ob.state[pb][s].cpu().numpy()
                np.testing.assert_allclose(oa.state[pa][s].cpu().numpy(), ref, rtol=2e-5, atol=2e-6 * max(1.0, float(np.abs(ref).max())),
                                           err_msg='%s %s' % (k, s))
            assert float(oa.state[pa]['step']) == float(ob.state[pb]['step']), k


@pytest.mark.parametrize('kind', list(KINDS))
def test_matches_torch_optim_one_launch_per_run(kind):
    ours, theirs, kw, keys = KINDS[kind]
    torch.manual_seed(5)
    na = dfl_amd.UNet(1, **CFG).to(DEV)
    nb = dfl_amd.UNet(1, **CFG).to(DEV)
    nb.load_state_dict(na.state_dict())
    oa = ours(na.parameters(), **kw)
    oa.FUSE_PACK = False                    # the update launches themselves (the update inside the re-layout: test 3)
    ob = theirs(nb.parameters(), **kw)
    x = torch.randn(2, 1, 32, 32, device=DEV)
    spy = None
    for step in range(4):
        _forward_backward(na, x)
        _grads_into(na, nb)
        if step == 3:
            spy = Spy(oa._lib, ['dfl_adam_step', 'dfl_rmsprop_step', 'dfl_optim_pack_tiled'])
            oa._lib = spy
        oa.step()
        ob.step()
        if step == 1:                       # the group's lr is written between steps
            oa.param_groups[0]['lr'] = ob.param_groups[0]['lr'] = 3e-4
    torch.cuda.synchronize()
    _assert_same(na, oa, nb, ob, keys)
    dead = dict(na.named_parameters())[DEAD]
    assert dead.grad is None and dead not in oa.state
    live = [p for p in na.parameters() if p.grad is not None]
    calls = spy.calls[STEP_FN[kind]]
    assert len(calls) == 2 and sum(a[4] for a in calls) >= sum(p.numel() for p in live), [a[4] for a in calls]
    assert not spy.calls['dfl_optim_pack_tiled']
    sd = oa.state_dict()
    assert len(sd['state']) == len(live)
    assert all(list(st.keys()) == ['step'] + list(keys) for st in sd['state'].values())
    assert all(st['step'].device.type == 'cpu' and st['step'].dtype == torch.float32 and float(st['step']) == 4
               for st in sd['state'].values())
    # every state key lives in one arena
    for s in keys:
        assert len({oa.state[p][s].untyped_storage().data_ptr() for p in live}) == 1, s


# ---- 3. the update inside the tiled weight re-layout ------------------------------------------------------------------
def _fused_vs_unfused(kind):
    ours, _, kw, keys = KINDS[kind]
    pr = PR.REGISTRY['paper__paper_sc_l14__b2']()
    res = []
    for fuse in (True, False):
        net = hip_net(pr)
        opt = ours(net.parameters(), **kw)
        opt.FUSE_PACK = fuse
        spy = Spy(opt._lib, [STEP_FN[kind], 'dfl_optim_pack_tiled'])
        opt._lib = spy
        seq = []
        for step in range(3):
            opt.zero_grad()
            out, seg, loss = hip_step(pr, net)
            seq.append((seg.detach().clone(), loss.item()))
            opt.step()
            if step == 0:
                opt.param_groups[0]['lr'] = 5e-4
        net.eval()
        with torch.no_grad():
            o = net(pr.x.to(DEV))
        seq.append(((o[0] if isinstance(o, tuple) else o).clone(), 0.0))
        torch.cuda.synchronize()
        res.append((net, opt, seq, {k: len(v) for k, v in spy.calls.items()}))
    (na, oa, sa, ca), (nb, ob, sb, cb) = res
    assert NF.train_plan(na)._tiled_host is not None, 'no tiled layouts in this problem: nothing was tested'
    assert ca == {STEP_FN[kind]: 0, 'dfl_optim_pack_tiled': 3}, ca
    assert cb['dfl_optim_pack_tiled'] == 0 and cb[STEP_FN[kind]] >= 3, cb
    for (s1, l1), (s2, l2) in zip(sa, sb):
        assert torch.equal(s1, s2) and l1 == l2
    for (k, pa), pb in zip(na.named_parameters(), nb.parameters()):
        assert torch.equal(pa, pb), k
        if pa.grad is not None:
            for s in keys:
                assert torch.equal(oa.state[pa][s], ob.state[pb][s]), (k, s)


@pytest.mark.parametrize('kind', ['adam', 'rmsprop_mom'])
def test_update_inside_the_weight_relayout_in_the_parity_arithmetics(math_mode, kind):
    _fused_vs_unfused(kind)


@pytest.mark.parametrize('kind', list(KINDS))
def test_update_inside_the_weight_relayout_in_bf16_storage(kind):
    with math_mode_set('bf16s'):
        _fused_vs_unfused(kind)


# ---- 4. state dicts between torch.optim and these classes -------------------------------------------------------------
def _through_a_file(sd):
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    return torch.load(buf, map_location='cpu', weights_only=False)


@pytest.mark.parametrize('kind', list(KINDS))
def test_state_dict_moves_both_ways(kind):
    ours, theirs, kw, keys = KINDS[kind]
    torch.manual_seed(7)
    x = torch.randn(2, 1, 32, 32, device=DEV)
    # ours -> torch
    na = dfl_amd.UNet(1, **CFG).to(DEV)
    oa = ours(na.parameters(), **kw)
    for _ in range(2):
        _forward_backward(na, x)
        oa.step()
    nb = dfl_amd.UNet(1, **CFG).to(DEV)
    nb.load_state_dict(na.state_dict())
    ob = theirs(nb.parameters(), **kw)
    ob.load_state_dict(_through_a_file(oa.state_dict()))
    _forward_backward(na, x)
    _grads_into(na, nb)
    oa.step()
    ob.step()
    torch.cuda.synchronize()
    _assert_same(na, oa, nb, ob, keys)
    # torch -> ours: the states go back into one arena per key, so the next step is one launch per run again
    nc = dfl_amd.UNet(1, **CFG).to(DEV)
    nc.load_state_dict(nb.state_dict())
    oc = ours(nc.parameters(), **kw)
    oc.load_state_dict(_through_a_file(ob.state_dict()))
    live = [p for p in nc.parameters() if p in oc.state]
    assert len(live) == len(ob.state)
    for s in keys:
        assert len({oc.state[p][s].untyped_storage().data_ptr() for p in live}) == 1, s
        assert all(oc.state[p][s].is_cuda for p in live)
    assert all(oc.state[p]['step'].device.type == 'cpu' for p in live)
    oc.FUSE_PACK = False
    spy = Spy(oc._lib, [STEP_FN[kind]])
    oc._lib = spy
    _forward_backward(nc, x)                # (the gradients of nc's own backward: the arena the runs need)
    _grads_into(nc, nb)
    ob.step()
    oc.step()
    torch.cuda.synchronize()
    assert len(spy.calls[STEP_FN[kind]]) == 2
    _assert_same(nc, oc, nb, ob, keys)


# ---- 5. train.py --optim adam | rmsprop ---------------------------------------------------------------------------------
@pytest.mark.parametrize('kind, extra', [('adam', ['--init-lr', '1e-3']), ('rmsprop', ['--init-lr', '1e-4', '--momentum', '0.9'])])
def test_train_resume_with_adam_and_rmsprop(tmp_path, kind, extra):
    from test_gpu_entrypoints import make_file, run, NC, L
    cwd = str(tmp_path)
    make_file(os.path.join(cwd, 'data.npz'))
    common = ['data.npz', '--train-pats', '1', '--valid-pats', '2', '--num-classes', str(NC), '--unet-img-dim', '48',
              '--batch-size', '4', '--unet-num-lvls', '3', '--unet-init-feats-exp', '3', '--unet-batch-norm', '--unet-padding',
              '--unet-no-max-pool', '--use-lands', '--wgt-decay', '1e-4', '--optim', kind, '--lr-sched', 'none',
              '--checkpoint-net', 'ck.pt', '--train-loss-txt', 'tl.txt', '--valid-loss-txt', 'vl.txt', '--seed', '3'] + extra
    out = run('train.py', common + ['--max-num-epochs', '2'], cwd)
    assert 'optimizer: {}, LR schedule: none'.format(kind) in out and 'Exiting - maximum number of epochs performed!' in out
    out = run('train.py', common + ['--max-num-epochs', '3'], cwd)
    assert 'loading state from checkpoint...' in out and 'Epoch: 002' in out and 'Epoch: 001' not in out
    ck = torch.load(os.path.join(cwd, 'ck.pt'), map_location='cpu', weights_only=False)
    assert ck['epoch'] == 3 and ck['optim-type'] == kind
    tl = [float(v) for v in open(os.path.join(cwd, 'tl.txt')).read().split('\n')[:-1]]
    assert len(tl) == 3 * 2 and all(np.isfinite(tl))                     # 8 images / batch 4, 3 epochs
    assert sum(tl[-2:]) < sum(tl[:2]), tl                                # the loss falls
    # the checkpoint's optimizer state is torch's: it loads into torch.optim over the reference-keyed model
    net = dfl_amd.UNet(n_classes=NC, depth=3, wf=3, batch_norm=True, padding=True, max_pool=False, num_lands=L)
    net.load_state_dict(ck['model-state-dict'])
    _, theirs, _, keys = KINDS['adam' if kind == 'adam' else 'rmsprop_mom']
    topt = theirs(net.parameters(), lr=1e-3)
    topt.load_state_dict(ck['optimizer-state-dict'])
    ps = list(net.parameters())
    assert 0 < len(topt.state) == len(ck['optimizer-state-dict']['state']) < len(ps)   # parameters without a gradient: no state
    assert ps[[k for k, _ in net.named_parameters()].index(DEAD)] not in topt.state
    for p, st in topt.state.items():
        assert list(st.keys()) == ['step'] + list(keys)
        assert float(st['step']) == 6 and st['step'].device.type == 'cpu'  # 2 steps per epoch, 3 epochs across the resume
        assert all(st[k].shape == p.shape for k in keys)
    for p in ps:
        p.grad = torch.zeros_like(p) if p in topt.state else None
    topt.step()                                                             # and steps on the CPU
    assert all(torch.isfinite(p).all() for p in ps)


# ---- 6. no CPU path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['adam', 'rmsprop_mom'])
def test_cpu_tensors_are_refused(kind):
    ours, _, kw, _ = KINDS[kind]
    net = dfl_amd.UNet(1, **CFG)
    opt = ours(net.parameters(), **kw)
    for p in net.parameters():
        p.grad = torch.ones_like(p)
    with pytest.raises(nat.DflError, match='GPU'):
        opt.step()
    assert len(opt.state) == 0
