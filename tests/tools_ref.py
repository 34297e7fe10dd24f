"""The numpy restatement of the tool semantics (include/dfl_hip.h, "Tools"), written from those
words: the model the tests compare csrc/drr_tools.hip against, its test cases, a brute-force check of the model itself and
its own statement of the culling rectangle.

The model consumes what the kernel consumes -- float32 capsules (a, b, r, mu) and the float32 qscale -- promoted to
`dtype`.  dtype=np.float64 is the reference; dtype=np.float32 carries out the kernel's stated arithmetic step for step
(every product and sum rounded on its own, dots summed x, y, z from the left), which tests/tools_floor.py compares with the
reference to find what float32 can do at all.

A capsule is every point within r of the segment [a, b], in mm in the camera projective frame; the ray of pixel (c, r) is
t d, t >= 0, d = Q [c, r, 1]; the chord is |d| times the measure of the t inside the capsule: smallest entry to largest
exit over the sphere about a, the sphere about b and the cylinder cut to the slab between its end planes, clipped at
t >= 0.  A ray with |u_perp|^2 <= PARALLEL takes the spheres alone.
"""
import numpy as np

import drr_ref as D

PARALLEL = 1e-10
MAX_TOOLS = 64
RECORD = np.dtype([('a', np.float32, 3), ('b', np.float32, 3), ('r', np.float32), ('mu', np.float32)])


def records(capsules):
    """[(a, b, r, mu)] in float64 -> the float32 values the kernel reads."""
    out = np.zeros(len(capsules), RECORD)
    for k, (a, b, r, mu) in enumerate(capsules):
        out[k] = (np.asarray(a, np.float64), np.asarray(b, np.float64), r, mu)
    return out


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def rays(qscale, H, W, dtype=np.float64, pixels=None):
    """(u [3][R] unit directions, ok [R]) of the pixels of an H x W grid in row-major order, or of pixels = (rows, cols)."""
    dt = dtype
    if pixels is None:
        rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        rr, cc = rr.reshape(-1), cc.reshape(-1)
    else:
        rr, cc = np.asarray(pixels[0]).reshape(-1), np.asarray(pixels[1]).reshape(-1)
    c, r = cc.astype(dt), rr.astype(dt)
    q = np.asarray(qscale, np.float32).reshape(-1).astype(dt)
    d = [q[3 * k] * c + q[3 * k + 1] * r + q[3 * k + 2] for k in range(3)]
    nd = np.sqrt(_dot(d, d))
    ok = (nd > 0) & np.isfinite(nd)
    with np.errstate(divide='ignore', invalid='ignore'):
        u = [np.where(ok, x / nd, 0).astype(dt) for x in d]
    return u, ok


def _sphere(u, p, rr, t0, t1):
    tc = _dot(u, p)
    q = [p[k] - tc * u[k] for k in range(3)]                  # the offset as a vector, then its square
    h2 = rr - _dot(q, q)
    hit = h2 >= 0
    h = np.sqrt(np.where(hit, h2, 0))
    return np.where(hit, np.fmin(t0, tc - h), t0), np.where(hit, np.fmax(t1, tc + h), t1)


def valid(rec):
    """A record with a field that is not finite or with r <= 0 contributes nothing."""
    vals = np.array(list(rec['a']) + list(rec['b']) + [rec['r'], rec['mu']], np.float64)
    return bool(np.isfinite(vals).all() and rec['r'] > 0)


def chord(rec, u, dtype=np.float64):
    """The chord in mm [R] of one record along the unit rays u."""
    dt = dtype
    a, b = [dt(x) for x in rec['a']], [dt(x) for x in rec['b']]
    r = dt(rec['r'])
    R = u[0].shape
    if not valid(rec):
        return np.zeros(R, dt)
    rr = r * r
    t0, t1 = np.full(R, np.inf, dt), np.full(R, -np.inf, dt)
    t0, t1 = _sphere(u, a, rr, t0, t1)
    t0, t1 = _sphere(u, b, rr, t0, t1)
    w = [b[k] - a[k] for k in range(3)]
    L = np.sqrt(_dot(w, w))
    if L > 0:
        e = [w[k] / L for k in range(3)]
        ue = _dot(u, e)
        p = [u[k] - ue * e[k] for k in range(3)]              # u_perp
        A = _dot(p, p)
        ae = _dot(a, e)
        s = [a[k] - ae * e[k] for k in range(3)]              # a_perp
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            tcyl = _dot(p, s) / A
            q = [s[k] - tcyl * p[k] for k in range(3)]
            h2 = rr - _dot(q, q)
            hit = (A > dt(PARALLEL)) & (h2 >= 0)
            h = np.sqrt(np.where(hit, h2 / A, 0))
            c0, c1 = tcyl - h, tcyl + h
            s0, s1 = ae / ue, (ae + L) / ue
            z = ue == 0
            k0 = np.where(z, c0, np.fmax(c0, np.fmin(s0, s1)))
            k1 = np.where(z, c1, np.fmin(c1, np.fmax(s0, s1)))
            keep = hit & np.where(z, bool(-ae >= 0 and -ae <= L), k1 >= k0)
        t0, t1 = np.where(keep, np.fmin(t0, k0), t0), np.where(keep, np.fmax(t1, k1), t1)
    with np.errstate(invalid='ignore'):
        return np.fmax(t1 - np.fmax(t0, dt(0)), dt(0)).astype(dt)


def add(views, qscale, H, W, dtype=np.float64, pixels=None):
    """(s, tool_len), each [V, H, W] (or [V, len(pixels)]): per view sum_j mu_j len_j and sum_j len_j, j ascending, in
    `dtype`.  views = [records] (tools_ref.records)."""
    dt = dtype
    u, ok = rays(qscale, H, W, dt, pixels)
    S, T = [], []
    for recs in views:
        s, tl = np.zeros(u[0].shape, dt), np.zeros(u[0].shape, dt)
        for rec in recs:
            if not valid(rec):
                continue
            ln = np.where(ok, chord(rec, u, dt), dt(0)).astype(dt)
            s = (s + dt(rec['mu']) * ln).astype(dt)
            tl = (tl + ln).astype(dt)
        S.append(s)
        T.append(tl)
    S, T = np.stack(S), np.stack(T)
    if pixels is None:
        return S.reshape(-1, H, W), T.reshape(-1, H, W)
    return S, T


def brute_chord(cap, d, samples=200000, t_max=None):
    """The chord of one float64 capsule (a, b, r, mu) along the ray t d by sampling: |d| dt times the number of samples
    t_k = (k + 1/2) dt, k < samples, within r of the segment.  Returns (chord, |d| dt)."""
    a, b, r = np.asarray(cap[0], np.float64), np.asarray(cap[1], np.float64), float(cap[2])
    d = np.asarray(d, np.float64)
    if t_max is None:
        t_max = (max(np.linalg.norm(a), np.linalg.norm(b)) + 2 * r) / np.linalg.norm(d)
    dt = t_max / samples
    x = ((np.arange(samples) + 0.5) * dt)[:, None] * d[None, :]
    w = b - a
    L2 = float(w @ w)
    lam = np.clip(((x - a) @ w) / L2, 0, 1) if L2 > 0 else np.zeros(samples)
    dist = np.linalg.norm(x - (a[None, :] + lam[:, None] * w[None, :]), axis=1)
    step = np.linalg.norm(d) * dt
    return float((dist <= r).sum() * step), step


# ---- the culling rectangle: this file's own statement of the rule -------------------------------------------------------
def pixel_rect(cap, Q, H, W):
    """(c0, r0, c1, r1), inclusive, or (0, 0, -1, -1) when empty.  With P = inv(Q), a point X projects to
    (P X)[:2] / (P X)[2], and (P X)[2] / |P[2]| is its distance in mm from the plane through the source that the rays
    leave.  If either end lies within r of that plane (or behind it): the whole image.  Else the box of the two projected
    ends, grown along each axis by r max_ends |P[axis] - x_end P[2]| / ((P X)[2]_nearer - r |P[2]|) -- the most a point
    within r of the segment can project away from the segment's own projection -- plus one pixel, clamped to the image."""
    a, b, r = np.asarray(cap[0], np.float64), np.asarray(cap[1], np.float64), float(cap[2])
    P = np.linalg.inv(np.asarray(Q, np.float64).reshape(3, 3))
    n = np.linalg.norm(P[2])
    wa, wb = float(P[2] @ a), float(P[2] @ b)
    near = min(wa, wb) - r * n
    if not near > 0:
        return 0, 0, W - 1, H - 1
    box = []
    for axis, size in ((0, W), (1, H)):
        xa, xb = float(P[axis] @ a) / wa, float(P[axis] @ b) / wb
        grow = r * max(np.linalg.norm(P[axis] - xa * P[2]), np.linalg.norm(P[axis] - xb * P[2])) / near + 1.0
        lo, hi = int(np.floor(min(xa, xb) - grow)), int(np.ceil(max(xa, xb) + grow))
        if hi < 0 or lo > size - 1:
            return 0, 0, -1, -1
        box.append((max(lo, 0), min(hi, size - 1)))
    return box[0][0], box[1][0], box[0][1], box[1][1]


# ---- cases -------------------------------------------------------------------------------------------------------------
WINDOW = (8, 18, 5, 7)                        # first row, first column, rows, columns of the window of the tilted grid


def grid(name):
    """(Q float64, H, W): 'full' is the 45 x 61 grid of drr_ref's tilted scene, 'window' a 5 x 7 window of it."""
    S = D.scene('tilted')
    if name == 'full':
        return S['Q'], S['rows'], S['cols']
    r0, c0, h, w = WINDOW
    return S['Q'] @ np.array([[1.0, 0, c0], [0, 1.0, r0], [0, 0, 1.0]]), h, w


def _at(c, r, depth=800.0):
    """The point at `depth` mm along the ray of pixel (c, r) of the full grid (its direction has z = -1)."""
    return depth * (D.scene('tilted')['Q'] @ np.array([c, r, 1.0]))


def _many(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ctr = _at(rng.uniform(0, 60), rng.uniform(0, 44), 800 + rng.uniform(-40, 40))
        v = rng.standard_normal(3)
        half = 0.5 * rng.uniform(5, 15) * v / np.linalg.norm(v)
        out.append((ctr - half, ctr + half, rng.uniform(0.5, 1.5), rng.uniform(0.2, 0.8)))
    return out


def _cases():
    oblique = (np.array([-18.0, -12.0, -790.0]), np.array([15.0, 10.0, -815.0]), 1.0, 0.5)
    crossing = [(_at(5, 5, 780), _at(55, 40, 820), 0.9, 0.5), (_at(50, 4, 815), _at(8, 41, 790), 1.3, 0.3)]
    through = _at(30.4, 22.3, 1.0)                                        # a direction between pixels
    return {
        'bead_on_ray': ('full', [[(_at(20, 10, 803.7), _at(20, 10, 803.7), 0.75, 0.5)]]),
        'bead_between': ('full', [[(_at(20.5, 10.5, 760), _at(20.5, 10.5, 760), 0.75, 0.5)]]),
        'oblique_wire': ('full', [[oblique]]),
        'wire_along_ray': ('full', [[(_at(25, 20, 760), _at(25, 20, 840), 0.8, 0.5)]]),
        'wire_leaves_image': ('full', [[(_at(-20, 5, 790), _at(80, 35, 810), 1.2, 0.5)]]),
        'wire_through_source_plane': ('full', [[(-100.0 * through, 700.0 * through, 1.5, 0.5)]]),
        'crossing_wires': ('full', [crossing]),
        'many_short_wires': ('full', [_many(MAX_TOOLS, 11)]),
        'three_views': ('full', [[], [oblique], crossing + _many(3, 12)]),
        'window': ('window', [[(_at(21, 10), _at(21, 10), 0.75, 0.5), (_at(16, 7, 790), _at(27, 14, 805), 0.6, 0.4)],
                              [(_at(20.5, 9.5, 820), _at(20.5, 9.5, 820), 0.75, 0.5)]]),
    }


_CASES = {}
_MODELS = {}


def cases():
    """{name: (grid name, [[(a, b, r, mu) float64] per view])}, computed once."""
    if not _CASES:
        _CASES.update(_cases())
    return _CASES


def model(name, dtype=np.float64):
    """(s, tool_len) [V, H, W] of a case, computed once and shared: do not write to them."""
    key = (name, np.dtype(dtype).name)
    if key not in _MODELS:
        g, views = cases()[name]
        Q, H, W = grid(g)
        s, tl = add([records(v) for v in views], Q.astype(np.float32), H, W, dtype)
        s.setflags(write=False)
        tl.setflags(write=False)
        _MODELS[key] = (s, tl)
    return _MODELS[key]
