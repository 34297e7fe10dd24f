"""dfl_drr_expose on the GPU (csrc/expose.hip) against tests/expose_ref.py, the numpy restatement of DESIGN.md
section 17.

Bars: the float32 output lies within 8 x the floors of tests/golden/floors/expose.json -- the largest |float32 model -
float64 model| of the same case (tests/expose_floor.py; both sides the model, never the kernel) -- of the float64 model
fed the kernel's own normals.  The normals agree with tests/aug_ref.py to 1e-5, the bar of tests/test_gpu_augment.py.
The uint16 output is the float32 output of the same launch, clamped and rounded half to even, bit for bit.

Sizes: 45 x 61 (one tile across, three down with a remainder), 5 x 7 (smaller than a tile and, at rho = 8, than the
halo), 53 x 199 (three tiles and a remainder both ways); 61 and 199 are odd, so uint16 rows are only 2-byte aligned.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests'))
import aug_ref as A  # noqa: E402
import expose_floor as FL  # noqa: E402
import expose_ref as X  # noqa: E402
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat, synth  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
KQ, KE = [q for q, _ in X.KEYS], [e for _, e in X.KEYS]
_ATT, _RUNS = {}, {}


def _att(name):
    if name not in _ATT:
        _ATT[name] = torch.from_numpy(X.inputs(name).copy()).to(DEV)
    return _ATT[name]


def _run(name, sigma, noise):
    """(I float32, I uint16, z1, z2) as numpy, of one case: two launches on the same inputs, computed once."""
    key = (name, sigma, noise)
    if key not in _RUNS:
        kw = dict(blur_sigma_px=sigma, keys_q=KQ if noise else None, keys_e=KE if noise else None, **X.PARAMS)
        f, z1, z2 = synth.expose(_att(name), u16=False, want_normals=True, **kw)
        q = synth.expose(_att(name), u16=True, **kw)
        _RUNS[key] = tuple(None if t is None else t.cpu().numpy() for t in (f, q, z1, z2))
    return _RUNS[key]


@pytest.mark.parametrize('name', ['scene', 'corner', 'smooth'])
def test_noise_planes_are_the_augmentation_normals(name):
    att = X.inputs(name)
    n = att.shape[1] * att.shape[2]
    _, _, z1, z2 = _run(name, 1.0, True)
    assert z1.shape == att.shape == z2.shape and z1.dtype == np.float32
    planes = []
    for v in range(3):
        for z, key in ((z1[v], KQ[v]), (z2[v], KE[v])):
            want = A.normals(key, np.arange(n)).reshape(att.shape[1:])
            err = float(np.abs(z - want).max())
            print('expose %s view %d: normals max |error| %.2e' % (name, v, err))
            assert err <= 1e-5
            planes.append(z)
    for i in range(len(planes)):
        for j in range(i + 1, len(planes)):
            assert not np.array_equal(planes[i], planes[j])
    if n >= 1000:                                             # mean and standard deviation within 5 standard errors
        allz = np.concatenate([p.reshape(-1) for p in planes]).astype(np.float64)
        m = allz.size
        assert abs(allz.mean()) <= 5.0 / np.sqrt(m) and abs(allz.std() - 1.0) <= 5.0 / np.sqrt(2.0 * m)
    # the blur radius does not move the normals
    assert np.array_equal(_run(name, 0.0, True)[2], z1) and np.array_equal(_run(name, 2.5, True)[3], z2)


@pytest.mark.parametrize('name,sigma,noise', X.CASES)
def test_float_output_matches_the_model(name, sigma, noise):
    f, _, z1, z2 = _run(name, sigma, noise)
    assert (z1 is None) == (not noise) and (z2 is None) == (not noise)
    w, rho = X.taps(sigma)
    assert rho == {0.0: 0, 1.0: 3, 2.5: 8}[sigma]
    want = X.expose(X.inputs(name), w, z1=z1, z2=z2, dtype=np.float64, **X.PARAMS)
    bar = FL.bar(name, sigma, noise)
    err = float(np.abs(f.astype(np.float64) - want).max())
    print('expose %s sigma %g noise %d: max |error| %.3e (bar %.3e, largest value %.1f)' % (name, sigma, noise, err, bar, np.abs(want).max()))
    assert f.dtype == np.float32 and f.shape == want.shape
    assert err <= bar, (err, bar)


def test_exact_cases():
    att = X.inputs('scene')
    miss = att == 0
    assert miss.mean() > 0.2
    f = _run('scene', 0.0, False)[0]
    top = np.float32(np.float32(X.PARAMS['gain']) * np.float32(X.PARAMS['photons']))
    assert (f[miss] == top).all() and (f[~miss] <= top).all() and (f[~miss] < top).any()
    # a constant field stays constant under the blur, within the bar
    const = torch.full((3, 45, 61), 0.75, dtype=torch.float32, device=DEV)
    for sigma in (1.0, 2.5):
        g = synth.expose(const, blur_sigma_px=sigma, u16=False, **X.PARAMS).cpu().numpy().astype(np.float64)
        w, _ = X.taps(sigma)
        value = float(X.expose(np.full((1, 1), 0.75, np.float32), w, **X.PARAMS)[0, 0])
        spread = float(g.max() - g.min())
        print('expose constant field sigma %g: spread %.3e, value %.4f (model %.4f)' % (sigma, spread, g.mean(), value))
        assert spread <= FL.bar('scene', sigma, False)
        assert float(np.abs(g - value).max()) <= FL.bar('scene', sigma, False)


@pytest.mark.parametrize('name,sigma,noise', X.CASES)
def test_uint16_is_the_rounded_float_output(name, sigma, noise):
    f, q, _, _ = _run(name, sigma, noise)
    assert q.dtype == np.uint16 and q.shape == f.shape
    assert np.array_equal(q, X.quantise(f))


@pytest.mark.parametrize('name', ['scene', 'smooth'])
def test_uint16_saturates_and_clamps(name):
    att = _att(name)
    for kw, what in ((dict(photons=5000.0, gain=40.0, electronic_sigma=4.0), 'top'),
                     (dict(photons=50.0, gain=1.5, electronic_sigma=400.0), 'bottom')):
        f = synth.expose(att, blur_sigma_px=1.0, keys_q=KQ, keys_e=KE, u16=False, **kw).cpu().numpy()
        q = synth.expose(att, blur_sigma_px=1.0, keys_q=KQ, keys_e=KE, u16=True, **kw).cpu().numpy()
        assert np.array_equal(q, X.quantise(f))
        if what == 'top':
            assert (f > 65535).mean() > 0.05 and (q[f > 65535] == 65535).all() and (q < 65535).any()
        else:
            assert (f < 0).mean() > 0.05 and (q[f < 0] == 0).all() and (q > 0).any()
    # ties go to the even neighbour: gain photons = k + 0.5 exactly on rays that miss
    z = torch.zeros((1, 3, 5), dtype=torch.float32, device=DEV)
    for k in (2, 3, 1000, 1001):
        q = synth.expose(z, photons=k + 0.5, gain=1.0, electronic_sigma=0.0, blur_sigma_px=0.0, u16=True).cpu().numpy()
        assert (q == (k if k % 2 == 0 else k + 1)).all(), (k, q)


def test_determinism_and_independence_of_the_batch():
    for name, sigma in (('scene', 1.0), ('smooth', 2.5), ('corner', 2.5)):
        att = _att(name)
        kw = dict(blur_sigma_px=sigma, **X.PARAMS)
        a = synth.expose(att, keys_q=KQ, keys_e=KE, u16=False, **kw)
        b = synth.expose(att, keys_q=KQ, keys_e=KE, u16=False, **kw)
        assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), _run(name, sigma, True)[0])
        one = synth.expose(att[1:2], keys_q=KQ[1:2], keys_e=KE[1:2], u16=False, **kw)
        assert torch.equal(one[0], a[1])
        one16 = synth.expose(att[1:2], keys_q=KQ[1:2], keys_e=KE[1:2], u16=True, **kw)
        assert np.array_equal(one16[0].cpu().numpy(), _run(name, sigma, True)[1][1])
    # one noise term alone: the other adds exactly nothing and needs no key
    att = _att('scene')
    clean = _run('scene', 1.0, False)[0]
    q_only = synth.expose(att, blur_sigma_px=1.0, keys_q=KQ, u16=False, **X.PARAMS).cpu().numpy()
    e_only = synth.expose(att, blur_sigma_px=1.0, keys_e=KE, u16=False, **X.PARAMS).cpu().numpy()
    zero_e = synth.expose(att, blur_sigma_px=1.0, keys_q=KQ, keys_e=KE, u16=False, **dict(X.PARAMS, electronic_sigma=0.0)).cpu().numpy()
    assert not np.array_equal(q_only, clean) and not np.array_equal(e_only, clean) and not np.array_equal(q_only, e_only)
    assert np.array_equal(q_only, zero_e)


def test_refusals_leave_the_outputs_untouched():
    att = _att('corner')
    V, R, Cn = att.shape
    SENT = 12345.0
    out = torch.full((V, R, Cn), SENT, dtype=torch.float32, device=DEV)
    z1, z2 = torch.full_like(out, SENT), torch.full_like(out, SENT)
    keys = torch.from_numpy(np.array(KQ, np.uint64).view(np.int64)).to(DEV)
    taps, rho = X.taps(1.0)
    full = np.zeros(2 * nat.EXPOSE_MAX_RADIUS + 1, np.float32)
    full[:taps.size] = taps
    L = nat.lib()

    def mk(**k):
        base = dict(att=att.data_ptr(), out=out.data_ptr(), key_q=keys.data_ptr(), key_e=keys.data_ptr(), z1=z1.data_ptr(),
                    z2=z2.data_ptr(), taps=(nat.f32 * full.size)(*full), rho=rho, V=V, R=R, C=Cn, u16=0, quantum=1, electronic=1,
                    photons=5000.0, gain=1.5, electronic_sigma=4.0)
        return nat.ExposeArgs(**dict(base, **k))

    stream = torch.cuda.current_stream(DEV).cuda_stream
    for kw, word in ((dict(att=None), b'required'), (dict(out=None), b'required'), (dict(V=0), b'sizes'), (dict(R=0), b'sizes'),
                     (dict(C=0), b'sizes'), (dict(V=-1), b'sizes'), (dict(R=65536, C=32768), b'2^31'), (dict(rho=9), b'rho'),
                     (dict(rho=-1), b'rho'), (dict(photons=0.0), b'photons'), (dict(photons=-1.0), b'photons'),
                     (dict(photons=float('nan')), b'photons'), (dict(gain=0.0), b'gain'), (dict(gain=-2.0), b'gain'),
                     (dict(electronic_sigma=-0.5), b'electronic_sigma'), (dict(key_q=None), b'key_q'), (dict(key_e=None), b'key_e'),
                     (dict(V=65536), b'65535')):
        a = mk(**kw)
        assert L.dfl_drr_expose(C.addressof(a), stream) == -1, kw
        assert word in L.dfl_last_error() and b'dfl_drr_expose' in L.dfl_last_error(), (kw, L.dfl_last_error())
    assert L.dfl_drr_expose(None, stream) == -1 and b'null' in L.dfl_last_error()
    torch.cuda.synchronize(DEV)
    for t in (out, z1, z2):
        assert bool((t == SENT).all())
    # a noise flag that is off needs no key; and the same block, valid, does write
    a = mk(key_q=None, key_e=None, quantum=0, electronic=0, z1=None, z2=None)
    assert L.dfl_drr_expose(C.addressof(a), stream) == 0
    torch.cuda.synchronize(DEV)
    assert np.array_equal(out.cpu().numpy(), _run('corner', 1.0, False)[0]) and bool((z1 == SENT).all())
    with pytest.raises(nat.DflError, match='GPU'):
        synth.expose(att.cpu())
    with pytest.raises(nat.DflError, match='radius'):
        synth.expose(att, blur_sigma_px=2.7)
