"""The numpy restatement of the detector model, written from those semantics: the model the GPU
tests compare csrc/expose.hip against, and the inputs of those tests.

    T = exp(-att);  B = blur of T along rows, then along columns, indices clamped to the image, each sum from tap 0
    upwards;  N = photons B;  noisy = N + sqrt(N) z1 + electronic_sigma z2;  I = gain noisy

dtype=np.float64 is the reference; dtype=np.float32 is the same model in the kernel's precision, every product and sum
rounded separately, which tests/expose_floor.py compares with the reference to find what fp32 can do at all.  The
normals z1, z2 are inputs (None: that term is off): the GPU test feeds the kernel's own planes, the floor tool those of
tests/aug_ref.py.  The taps are the float32 taps the host passes to the kernel, promoted to dtype.
"""
import numpy as np

MAX_RADIUS = 8
TILE = (16, 64)                                   # csrc/expose.hip: rows x columns of a workgroup's tile


def taps(sigma_px):
    """(float32 taps [2 rho + 1], rho): a float64 Gaussian at -rho..rho, rho = ceil(3 sigma), normalised, rounded."""
    rho = int(np.ceil(3.0 * float(sigma_px)))
    if rho > MAX_RADIUS:
        raise ValueError('rho %d > %d' % (rho, MAX_RADIUS))
    if rho == 0:
        return np.ones(1, np.float32), 0
    k = np.arange(-rho, rho + 1, dtype=np.float64)
    w = np.exp(-0.5 * (k / float(sigma_px)) ** 2)
    return (w / w.sum()).astype(np.float32), rho


def blur(T, w, dtype):
    """Separable blur of [..., R, C]: rows first (along the column index), then columns, clamped indices."""
    w = np.asarray(w, np.float32).astype(dtype)
    rho = (w.size - 1) // 2
    if rho == 0:
        return (w[0] * T).astype(dtype)
    R, C = T.shape[-2:]
    ci = np.clip(np.arange(C)[None, :] + np.arange(-rho, rho + 1)[:, None], 0, C - 1)
    ri = np.clip(np.arange(R)[None, :] + np.arange(-rho, rho + 1)[:, None], 0, R - 1)
    acc = np.zeros(T.shape, dtype)
    for k in range(w.size):
        acc = (acc + (w[k] * T[..., :, ci[k]]).astype(dtype)).astype(dtype)
    out = np.zeros(T.shape, dtype)
    for k in range(w.size):
        out = (out + (w[k] * acc[..., ri[k], :]).astype(dtype)).astype(dtype)
    return out


def expose(att, w, photons, gain, electronic_sigma, z1=None, z2=None, dtype=np.float64):
    """I [..., R, C] in dtype from float32 line integrals; z1 / z2 None switches that term off."""
    dt = dtype
    a = np.asarray(att, np.float32).astype(dt)
    T = np.exp(-a).astype(dt)
    B = blur(T, w, dt)
    N = (dt(np.float32(photons)) * B).astype(dt)
    noisy = N
    if z1 is not None:
        noisy = (noisy + (np.sqrt(N).astype(dt) * np.asarray(z1, np.float32).astype(dt)).astype(dt)).astype(dt)
    if z2 is not None:
        noisy = (noisy + (dt(np.float32(electronic_sigma)) * np.asarray(z2, np.float32).astype(dt)).astype(dt)).astype(dt)
    return (dt(np.float32(gain)) * noisy).astype(dt)


def quantise(I):
    """float32 intensities -> uint16: clamped to [0, 65535], rounded half to even."""
    return np.rint(np.clip(np.asarray(I, np.float32), np.float32(0), np.float32(65535))).astype(np.uint16)


# ---- the test inputs ---------------------------------------------------------------------------------------------------
KEYS = ((0x0123456789ABCDEF, 0xFEDCBA9876543210), (0x9E3779B97F4A7C15, 0x0000000100000001), (0xDEADBEEFCAFEF00D, 0x7))
SIGMAS = (0.0, 1.0, 2.5)
PARAMS = dict(photons=5000.0, gain=1.5, electronic_sigma=4.0)
SMOOTH_SIZE = (3 * TILE[0] + 5, 3 * TILE[1] + 7)          # three tiles and a remainder in both directions
_INPUTS = {}


def inputs(name):
    """att float32 [3, R, C] of a named case: 'scene' (the tilted scene's two exact views and their mean, 45 x 61),
    'corner' (a 5 x 7 window of it cut around its largest value: the scene's own four corners hold only rays that miss)
    and 'smooth' (an analytic field, 53 x 199).  Shared: do not write to them."""
    if name in _INPUTS:
        return _INPUTS[name]
    if name in ('scene', 'corner'):
        import drr_ref as D
        v0, v1 = (D.model('tilted', 'exact', v)[0] for v in (0, 1))
        a = np.stack([v0, v1, 0.5 * (v0 + v1)]).astype(np.float32)
        if name == 'corner':
            r, c = np.unravel_index(int(np.argmax(a[0])), a[0].shape)
            r, c = min(max(r - 4, 0), a.shape[1] - 5), min(max(c - 6, 0), a.shape[2] - 7)
            a = np.ascontiguousarray(a[:, r:r + 5, c:c + 7])
    elif name == 'smooth':
        R, C = SMOOTH_SIZE
        r, c = np.meshgrid(np.arange(R, dtype=np.float64), np.arange(C, dtype=np.float64), indexing='ij')
        a = np.stack([1.5 + 1.2 * np.sin(0.11 * r + 0.3 * v) * np.cos(0.07 * c - 0.2 * v) + 0.002 * (r + c) for v in range(3)])
        a = np.maximum(a, 0).astype(np.float32)
    else:
        raise KeyError(name)
    a.setflags(write=False)
    _INPUTS[name] = a
    return a


CASES = [(name, sigma, noise) for name in ('scene', 'corner', 'smooth') for sigma in SIGMAS for noise in (False, True)]


def case_key(name, sigma, noise):
    return '%s/sigma%g/%s' % (name, sigma, 'noise' if noise else 'clean')
