"""CPU-side checks of dfl_amd.Adam / dfl_amd.RMSprop and their C ABI (no kernel is launched): the entry points are declared
and exported, the struct mirror matches, bad arguments are refused with a message, and the Python classes take torch's
constructor arguments, refuse what the HIP path does not implement, and keep torch's param_groups keys."""
import ctypes as C
import os
import re

import pytest
import torch

import dfl_amd
from conftest import ROOT
from dfl_amd import _native as nat

NEW = ('dfl_adam_step', 'dfl_rmsprop_step', 'dfl_optim_pack_tiled')
CFG = dict(n_classes=4, depth=3, wf=3, batch_norm=True, padding=True, max_pool=False, num_lands=3)
P = 0x10000                # a fake, aligned device address: only argument checks run, nothing is dereferenced


def test_new_symbols_are_declared_and_exported():
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dfl_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(dfl_[a-z0-9_]+)\s*\(', hdr))
    lib = C.CDLL(nat.LIB_PATH)
    for f in NEW:
        assert f in declared and f in nat.EXPORTS and hasattr(lib, f), f
    assert 'dfl_optim_pack_args' in hdr and '#define DFL_OPTIM_ADAM 1' in hdr and '#define DFL_OPTIM_RMSPROP 2' in hdr


def test_optim_pack_args_mirror_matches_the_library():
    L = nat.lib()
    k = nat._SIZEOF_ORDER.index(nat.OptimPackArgs)
    assert k == len(nat._SIZEOF_ORDER) - 1
    assert L.dfl_sizeof(k) == C.sizeof(nat.OptimPackArgs) > 0
    assert L.dfl_sizeof(k + 1) == -1


def _adam(L, **kw):
    a = dict(p=P, g=P + 4096, m=P + 8192, v=P + 12288, n=10, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, step_size=1e-2,
             bc2=0.0316, gs=1.0)
    a.update(kw)
    return L.dfl_adam_step(a['p'], a['g'], a['m'], a['v'], a['n'], a['lr'], a['b1'], a['b2'], a['eps'], a['wd'], a['step_size'],
                           a['bc2'], a['gs'], None)


def _rms(L, **kw):
    a = dict(p=P, g=P + 4096, sq=P + 8192, buf=P + 12288, n=10, lr=1e-2, alpha=0.99, eps=1e-8, wd=0.0, mom=0.9, gs=1.0)
    a.update(kw)
    return L.dfl_rmsprop_step(a['p'], a['g'], a['sq'], a['buf'], a['n'], a['lr'], a['alpha'], a['eps'], a['wd'], a['mom'], a['gs'], None)


@pytest.mark.parametrize('kw, msg', [(dict(p=None), b'bad args'), (dict(g=None), b'bad args'), (dict(m=None), b'bad args'),
                                     (dict(v=None), b'bad args'), (dict(n=0), b'bad args'), (dict(m=P + 12288), b'alias'),
                                     (dict(b1=1.0), b'coefficients'), (dict(b2=-0.1), b'coefficients'),
                                     (dict(eps=-1.0), b'coefficients'), (dict(wd=-1e-4), b'coefficients'),
                                     (dict(step_size=1e-4), b'coefficients'), (dict(bc2=0.0), b'coefficients'),
                                     (dict(bc2=1.5), b'coefficients'), (dict(lr=float('nan')), b'coefficients')])
def test_adam_step_refuses_bad_arguments(kw, msg):
    L = nat.lib()
    assert _adam(L, **kw) == -1
    assert msg in L.dfl_last_error() and b'dfl_adam_step' in L.dfl_last_error()


@pytest.mark.parametrize('kw, msg', [(dict(p=None), b'bad args'), (dict(g=None), b'bad args'), (dict(sq=None), b'bad args'),
                                     (dict(n=-3), b'bad args'), (dict(buf=None), b'momentum buffer'),
                                     (dict(mom=0.0), b'momentum buffer'), (dict(mom=-0.5), b'coefficients'),
                                     (dict(alpha=-1.0), b'coefficients'), (dict(lr=float('inf')), b'coefficients'),
                                     (dict(sq=P), b'alias')])
def test_rmsprop_step_refuses_bad_arguments(kw, msg):
    L = nat.lib()
    assert _rms(L, **kw) == -1
    assert msg in L.dfl_last_error() and b'dfl_rmsprop_step' in L.dfl_last_error()


def _pack(**kw):
    a = dict(jobs_dev=P, njobs=3, total_tiles=40, kind=nat.OPTIM_ADAM, grad_delta=1 << 20, state1_delta=2 << 20, state2_delta=3 << 20,
             lr=1e-3, eps=1e-8, weight_decay=0.0, grad_scale=1.0, beta1=0.9, beta2=0.999, step_size=1e-2, bc2_sqrt=0.0316,
             alpha=0.99, momentum=0.0)
    a.update(kw)
    return nat.OptimPackArgs(**a)


@pytest.mark.parametrize('kw, msg', [(dict(jobs_dev=None), b'empty job list'), (dict(njobs=0), b'empty job list'),
                                     (dict(total_tiles=0), b'empty job list'), (dict(kind=0), b'kind'), (dict(kind=3), b'kind'),
                                     (dict(grad_delta=6), b'16-byte'), (dict(state1_delta=(2 << 20) + 2), b'16-byte'),
                                     (dict(state2_delta=(3 << 20) + 1), b'16-byte'), (dict(state1_delta=1 << 20), b'overlap'),
                                     (dict(state2_delta=0), b'overlap'), (dict(grad_delta=0), b'overlap'),
                                     (dict(beta1=1.0), b'Adam coefficients'), (dict(step_size=1e-4), b'Adam coefficients'),
                                     (dict(kind=nat.OPTIM_RMSPROP, momentum=-1.0), b'RMSprop coefficients'),
                                     (dict(kind=nat.OPTIM_RMSPROP, alpha=float('nan')), b'RMSprop coefficients'),
                                     (dict(kind=nat.OPTIM_RMSPROP, momentum=0.9, state2_delta=2 << 20), b'overlap')])
def test_optim_pack_tiled_refuses_bad_arguments(kw, msg):
    L = nat.lib()
    a = _pack(**kw)
    assert L.dfl_optim_pack_tiled(C.addressof(a), None) == -1
    assert msg in L.dfl_last_error() and b'dfl_optim_pack_tiled' in L.dfl_last_error()
    assert L.dfl_optim_pack_tiled(None, None) == -1


def test_constructors_validate_like_torch():
    net = dfl_amd.UNet(1, **CFG)
    for bad in (dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            torch.optim.Adam(net.parameters(), **bad)
        with pytest.raises(ValueError):
            dfl_amd.Adam(net.parameters(), **bad)
    for bad in (dict(lr=-1.0), dict(eps=-1e-8), dict(momentum=-0.1), dict(weight_decay=-1.0), dict(alpha=-0.5)):
        with pytest.raises(ValueError):
            torch.optim.RMSprop(net.parameters(), **bad)
        with pytest.raises(ValueError):
            dfl_amd.RMSprop(net.parameters(), **bad)


@pytest.mark.parametrize('cls, kw', [(dfl_amd.Adam, dict(amsgrad=True)), (dfl_amd.Adam, dict(maximize=True)),
                                     (dfl_amd.Adam, dict(capturable=True)), (dfl_amd.Adam, dict(differentiable=True)),
                                     (dfl_amd.Adam, dict(fused=True)), (dfl_amd.Adam, dict(decoupled_weight_decay=True)),
                                     (dfl_amd.Adam, dict(lr=torch.tensor(1e-3))), (dfl_amd.RMSprop, dict(centered=True)),
                                     (dfl_amd.RMSprop, dict(maximize=True)), (dfl_amd.RMSprop, dict(capturable=True)),
                                     (dfl_amd.RMSprop, dict(differentiable=True))])
def test_options_without_a_hip_path_are_refused(cls, kw):
    net = dfl_amd.UNet(1, **CFG)
    with pytest.raises(NotImplementedError):
        cls(net.parameters(), **kw)


@pytest.mark.parametrize('ours, theirs, kw', [(dfl_amd.Adam, torch.optim.Adam, dict(lr=1e-3, weight_decay=1e-4)),
                                              (dfl_amd.Adam, torch.optim.Adam, dict()),
                                              (dfl_amd.RMSprop, torch.optim.RMSprop, dict(lr=1e-3, weight_decay=1e-4, momentum=0.9)),
                                              (dfl_amd.RMSprop, torch.optim.RMSprop, dict())])
def test_param_groups_match_torch(ours, theirs, kw):
    net = dfl_amd.UNet(1, **CFG)
    a, b = ours(net.parameters(), **kw), theirs(net.parameters(), **kw)
    ga, gb = a.state_dict()['param_groups'], b.state_dict()['param_groups']
    assert [sorted(g.keys()) for g in ga] == [sorted(g.keys()) for g in gb]
    assert ga == gb
    # a torch state dict without state loads, and the group settings survive the round trip
    a.load_state_dict(b.state_dict())
    assert a.state_dict()['param_groups'] == gb


def test_exported_from_the_package():
    assert 'Adam' in dfl_amd.__all__ and 'RMSprop' in dfl_amd.__all__
    assert issubclass(dfl_amd.Adam, torch.optim.Optimizer) and issubclass(dfl_amd.RMSprop, torch.optim.Optimizer)


@pytest.mark.parametrize('cls', [dfl_amd.Adam, dfl_amd.RMSprop])
def test_cpu_tensors_are_refused(cls):
    net = dfl_amd.UNet(1, **CFG)
    opt = cls(net.parameters(), lr=1e-3)
    for p in net.parameters():
        p.grad = torch.ones_like(p)
    with pytest.raises(nat.DflError, match='GPU'):
        opt.step()
