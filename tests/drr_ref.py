"""The numpy restatement of the DRR semantics, written from those semantics: the model the
GPU tests compare csrc/drr.hip against, the two test scenes, and the exclusion rules of the comparisons.

The model consumes the kernel's own argument records -- the fp32-rounded o, M, boxes and mask of every object and the
fp32 qscale -- promoted to `dtype`, so that only the kernel's arithmetic is under test.  dtype=np.float64 is the
reference; dtype=np.float32 is the same model in the kernel's precision, which tests/drr_floor.py compares with the
reference to find what fp32 can do at all.

Exact mode is the sorted merge of the three axes' plane crossings, all rays of an object at once: per axis the t of
every plane of the box, those outside (t0, t1) pushed to infinity, the three lists and {t0, t1} sorted together; a
segment between two finite neighbours lies in the voxel its midpoint falls into.
"""
import numpy as np

OBJECT_DTYPE = np.dtype([('o', np.float32, 3), ('M', np.float32, 9), ('box_lo', np.int32, 3), ('box_hi', np.int32, 3),
                         ('mask', np.uint32)])
MASKS = (0x1e, 0x20, 0x40)                    # pelvis {1, 2, 3, 4}, left femur {5}, right femur {6}
N_LABELS = 7
STEP_MM = 0.5
NEAR_INTEGER = 1e-4                           # trilinear: s (t1 - t0) / step this close to an integer -> N may differ by one


# ---- geometry ----------------------------------------------------------------------------------------------------------
def rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    R = np.eye(4)
    i, j = [(1, 2), (0, 2), (0, 1)][axis]
    R[i, i] = R[j, j] = c
    R[i, j], R[j, i] = -s, s
    return R


def c2i(I2P, P, E):
    return np.linalg.inv(I2P) @ P @ np.linalg.inv(E)


def label_box(lab, mask):
    """Inclusive (x, y, z) index box of the voxels whose label is in the mask; empty: ((0, 0, 0), (-1, -1, -1))."""
    adm = ((mask >> lab.astype(np.uint32)) & 1).astype(bool) & (lab < 16)
    if not adm.any():
        return (0, 0, 0), (-1, -1, -1)
    z, y, x = np.nonzero(adm)
    return (int(x.min()), int(y.min()), int(z.min())), (int(x.max()), int(y.max()), int(z.max()))


def pack(c2is, masks, Q, lab, tight=True, interp='exact'):
    """Records [n_obj] of OBJECT_DTYPE from float64 matrices, as dfl_amd.drr.pack_objects makes them."""
    nz, ny, nx = lab.shape
    out = np.zeros(len(c2is), OBJECT_DTYPE)
    for n, (A, mask) in enumerate(zip(c2is, masks)):
        lo, hi = label_box(lab, mask) if tight else ((0, 0, 0), (nx - 1, ny - 1, nz - 1))
        if tight and interp == 'trilinear' and hi[0] >= lo[0]:
            lo = tuple(max(a - 1, 0) for a in lo)
            hi = tuple(min(a + 1, b) for a, b in zip(hi, (nx - 1, ny - 1, nz - 1)))
        out[n]['o'], out[n]['M'] = A[:3, 3], (A[:3, :3] @ Q).reshape(-1)
        out[n]['box_lo'], out[n]['box_hi'], out[n]['mask'] = lo, hi, mask
    return out


# ---- the model ---------------------------------------------------------------------------------------------------------
def _dot(m, c, r):
    return m[0] * c + m[1] * r + m[2]


def _setup(rec, c, r, dt):
    """o [3], d [3][R], the clipped range t0, t1 [R] and which rays hit the box."""
    o = rec['o'].astype(dt)
    M = rec['M'].astype(dt)
    lo, hi = rec['box_lo'], rec['box_hi']
    d = [_dot(M[3 * a:3 * a + 3], c, r) for a in range(3)]
    t0 = np.zeros(c.shape, dt)
    t1 = np.full(c.shape, np.inf, dt)
    ok = np.ones(c.shape, bool)
    half = dt(0.5)
    with np.errstate(divide='ignore', invalid='ignore'):
        for a in range(3):
            z = d[a] == 0
            ta = (dt(lo[a]) - half - o[a]) / d[a]
            tb = (dt(hi[a] + 1) - half - o[a]) / d[a]
            t0 = np.where(z, t0, np.maximum(t0, np.minimum(ta, tb)))
            t1 = np.where(z, t1, np.minimum(t1, np.maximum(ta, tb)))
            ok &= np.where(z, (o[a] >= dt(lo[a]) - half) & (o[a] < dt(hi[a]) + half), True)
    ok &= (t1 > t0) & np.isfinite(t1)
    return o, d, t0, t1, ok


def _admit(mask):
    lut = np.zeros(256, bool)
    lut[:16] = [(int(mask) >> l) & 1 for l in range(16)]
    return lut


def render(mu, lab, recs, qscale, H, W, interp='exact', step_mm=STEP_MM, dtype=np.float64, n_labels=N_LABELS, pixels=None):
    """att [H, W], plen [n_labels, H, W] (zeros for trilinear) and frac [n_obj, H, W] = s (t1 - t0) / step_mm of every
    object (nan where the ray misses its box).  pixels = (rows, cols) index arrays: only those rays, outputs [len]."""
    dt = dtype
    if pixels is None:
        rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        rr, cc = rr.reshape(-1), cc.reshape(-1)
    else:
        rr, cc = np.asarray(pixels[0]).reshape(-1), np.asarray(pixels[1]).reshape(-1)
    c, r = cc.astype(dt), rr.astype(dt)
    q = np.asarray(qscale, np.float32).reshape(-1).astype(dt)
    qv = [_dot(q[3 * a:3 * a + 3], c, r) for a in range(3)]
    s = np.sqrt(qv[0] * qv[0] + qv[1] * qv[1] + qv[2] * qv[2])
    mu = mu.astype(dt)
    nz, ny, nx = lab.shape
    R = c.size
    att = np.zeros(R, dt)
    plen = np.zeros((n_labels, R), dt)
    frac = np.full((len(recs), R), np.nan)
    half = dt(0.5)
    for n, rec in enumerate(recs):
        lo, hi = rec['box_lo'], rec['box_hi']
        if (hi < lo).any():
            continue
        o, d, t0, t1, ok = _setup(rec, c, r, dt)
        adm = _admit(rec['mask'])
        frac[n] = np.where(ok, (s * (t1 - t0) / dt(step_mm)).astype(np.float64), np.nan)
        if interp == 'exact':
            lists = [t0[:, None], t1[:, None]]
            with np.errstate(divide='ignore', invalid='ignore'):
                for a in range(3):
                    k = np.arange(lo[a], hi[a] + 2).astype(dt)
                    t = (k[None, :] - half - o[a]) / d[a][:, None]
                    inside = (t > t0[:, None]) & (t < t1[:, None]) & (d[a] != 0)[:, None]
                    lists.append(np.where(inside, t, dt(np.inf)))
                ts = np.sort(np.concatenate(lists, 1), 1)
                seg = np.isfinite(ts[:, 1:]) & ok[:, None]
                ln = np.where(seg, ts[:, 1:] - ts[:, :-1], 0).astype(dt) * s[:, None]
                mid = np.where(seg, (ts[:, 1:] + ts[:, :-1]) * half, 0).astype(dt)
                idx = [np.clip(np.floor(np.where(seg, o[a] + mid * d[a][:, None], lo[a]) + half).astype(np.int64), lo[a], hi[a])
                       for a in range(3)]
            lv = lab[idx[2], idx[1], idx[0]]
            m = adm[lv] & seg
            att += (np.where(m, ln * mu[idx[2], idx[1], idx[0]], 0).astype(dt)).sum(1, dtype=dt)
            for l in range(n_labels):
                plen[l] += np.where(m & (lv == l), ln, 0).astype(dt).sum(1, dtype=dt)
        else:
            span = np.where(ok, t1 - t0, 0).astype(dt)
            nf = np.maximum(dt(1), np.ceil(s * span / dt(step_mm))).astype(dt)
            N = np.where(ok, nf, 0).astype(np.int64)
            k = np.arange(max(int(N.max()), 1)).astype(dt)
            live = k[None, :] < N[:, None]
            t = (np.where(ok, t0, 0).astype(dt)[:, None] + (k[None, :] + half) * (span / nf)[:, None]).astype(dt)
            t = np.where(live, t, 0).astype(dt)
            i0, i1, w = [], [], []
            for a, size in enumerate((nx, ny, nz)):
                p = (o[a] + t * d[a][:, None]).astype(dt)
                f = np.floor(p)
                w.append((p - f).astype(dt))
                i0.append(np.clip(f.astype(np.int64), 0, size - 1))
                i1.append(np.clip(f.astype(np.int64) + 1, 0, size - 1))

            def v(x, y, z):
                return np.where(adm[lab[z, y, x]], mu[z, y, x], 0).astype(dt)

            a00 = v(i0[0], i0[1], i0[2]) + w[0] * (v(i1[0], i0[1], i0[2]) - v(i0[0], i0[1], i0[2]))
            a10 = v(i0[0], i1[1], i0[2]) + w[0] * (v(i1[0], i1[1], i0[2]) - v(i0[0], i1[1], i0[2]))
            a01 = v(i0[0], i0[1], i1[2]) + w[0] * (v(i1[0], i0[1], i1[2]) - v(i0[0], i0[1], i1[2]))
            a11 = v(i0[0], i1[1], i1[2]) + w[0] * (v(i1[0], i1[1], i1[2]) - v(i0[0], i1[1], i1[2]))
            b0 = a00 + w[1] * (a10 - a00)
            b1 = a01 + w[1] * (a11 - a01)
            val = np.where(live, b0 + w[2] * (b1 - b0), 0).astype(dt)
            att += ((s * span / nf).astype(dt) * val.sum(1, dtype=dt)).astype(dt)
    if pixels is None:
        return att.reshape(H, W), plen.reshape(n_labels, H, W), frac.reshape(len(recs), H, W)
    return att, plen, frac


def label_map(plen, min_len_mm=1.0):
    """The lowest l >= 1 with the largest plen[l], or 0 if that length is below min_len_mm."""
    if plen.shape[0] < 2:
        return np.zeros(plen.shape[1:], np.uint8)
    arg = plen[1:].argmax(0) + 1                                   # argmax returns the first of equal ones
    return np.where(plen[1:].max(0) >= min_len_mm, arg, 0).astype(np.uint8)


def near_tie(plen, band, min_len_mm=1.0):
    """Pixels whose label the band could change: the top length is within `band` of min_len_mm, or it is above
    min_len_mm and within `band` of the runner-up."""
    top = np.sort(plen[1:], 0)[::-1]
    second = top[1] if top.shape[0] > 1 else np.zeros_like(top[0])
    return (np.abs(top[0] - min_len_mm) <= band) | ((top[0] > min_len_mm) & (top[0] - second <= band))


def near_integer(frac):
    """Rays on which some object's s (t1 - t0) / step lies within NEAR_INTEGER of an integer."""
    f = np.where(np.isnan(frac), 0.5, frac)
    return (np.abs(f - np.round(f)) <= NEAR_INTEGER).any(0)


# ---- scenes ------------------------------------------------------------------------------------------------------------
ELLIPSOIDS = (((12, 22, 26), (9, 14, 18), 1), ((26, 22, 26), (8, 13, 17), 2), ((19, 22, 40), (6, 6, 8), 3),
              ((19, 30, 14), (5, 5, 6), 4), ((8, 12, 10), (5, 6, 8), 5), ((29, 12, 10), (5, 6, 8), 6))


def phantom(nx=37, ny=45, nz=53, scale=1.0):
    """(labels uint8 [z, y, x], HU float32): six overlapping ellipsoids labelled 1..6; HU = a smooth blob
    + 700 (label > 0) + a small sinusoid.  scale stretches the ellipsoids with the volume."""
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing='ij')
    x, y, z = x / scale, y / scale, z / scale
    lab = np.zeros((nz, ny, nx), np.uint8)
    for ctr, rad, l in ELLIPSOIDS:
        lab[((x - ctr[0]) / rad[0]) ** 2 + ((y - ctr[1]) / rad[1]) ** 2 + ((z - ctr[2]) / rad[2]) ** 2 < 1] = l
    blob = np.exp(-(((x - 18) / 16.0) ** 2 + ((y - 22) / 20.0) ** 2 + ((z - 26) / 24.0) ** 2) ** 2)
    hu = (-1000 + 1000 * blob + 700 * (lab > 0) + 40 * np.sin(0.9 * x + 0.7 * y + 0.5 * z)).astype(np.float32)
    return lab, hu


def hu_to_mu(hu, mu_water=0.02):
    return (mu_water * np.maximum(hu.astype(np.float64) + 1000, 0) / 1000).astype(np.float32)


_SCENES = {}


def scene(kind):
    """'tilted': E and the three poses are general rotations that differ, non-integer principal point.  'aligned':
    E = identity, one axis-aligned pose for all objects, principal point (32, 16) -- powers of two, so that in fp32 too
    pixel (32, 16) looks straight down the z axis with two direction components exactly 0 -- and whole pixel rows share
    plane crossings.
    Volume 37 x 45 x 53, spacing (0.8, 0.75, 1.1), detector 45 rows x 61 columns of 1 mm, focal length 1000 mm, the
    objects near z = -800 of the camera frame.  Returned arrays are shared: do not write to them."""
    if kind in _SCENES:
        return _SCENES[kind]
    aligned = kind == 'aligned'
    lab, hu = phantom()
    nz, ny, nx = lab.shape
    I2P = np.eye(4)
    I2P[:3, :3] = np.diag([0.8, 0.75, 1.1])
    I2P[:3, 3] = [-20.0, 15.5, 120.25]
    rows, cols, f = 45, 61, 1000.0
    pp = (32.0, 16.0) if aligned else (30.3, 22.6)
    K = np.array([[-f, 0, pp[0]], [0, -f, pp[1]], [0, 0, 1]])
    E = np.eye(4)
    if not aligned:
        E = rot(0, 0.3) @ rot(1, -0.2) @ rot(2, 0.4)
        E[:3, 3] = [5, -7, 3]
    ctr = (I2P @ np.array([(nx - 1) / 2, (ny - 1) / 2, (nz - 1) / 2, 1]))[:3]

    def pose(R, shift):
        V2C = np.eye(4)                                   # volume physical frame -> camera projective frame
        V2C[:3, :3] = R[:3, :3]
        V2C[:3, 3] = np.array(shift) - R[:3, :3] @ ctr
        return np.linalg.inv(V2C) @ E                     # V2C = E inv(P)

    if aligned:
        poses = [pose(np.eye(4), (-1.6, 4.8, -800))] * 3          # centred on detector pixel (30, 22)
    else:
        poses = [pose(rot(0, 0.5) @ rot(2, 0.3), (3, -4, -800)), pose(rot(0, 0.6) @ rot(2, 0.25), (6, -2, -790)),
                 pose(rot(0, 0.4) @ rot(1, 0.2), (-1, -6, -810))]
    S = dict(kind=kind, lab=lab, hu=hu, mu=hu_to_mu(hu), I2P=I2P, K=K, E=E, poses=poses, rows=rows, cols=cols,
             Q=-np.linalg.inv(K))
    for a in (lab, hu, S['mu']):
        a.setflags(write=False)
    _SCENES[kind] = S
    return S


def perturbed(S):
    """The poses of the second view: every object turned about the volume's centre and shifted a little, each
    differently."""
    nz, ny, nx = S['lab'].shape
    ctr = (S['I2P'] @ np.array([(nx - 1) / 2, (ny - 1) / 2, (nz - 1) / 2, 1]))[:3]
    out = []
    for n, P in enumerate(S['poses']):
        D = rot(0, 0.04 + 0.01 * n) @ rot(1, -0.03 + 0.02 * n) @ rot(2, 0.05 - 0.015 * n)
        D[:3, 3] = ctr - D[:3, :3] @ ctr + np.array([1.5 - n, -2.0 + 0.7 * n, 4.0 - 2.5 * n])
        out.append(D @ P)
    return out


def scene_views(S):
    """[[C2I per object] per view]: the scene's own poses, then the perturbed ones."""
    return [[c2i(S['I2P'], P, S['E']) for P in poses] for poses in (S['poses'], perturbed(S))]


_MODELS = {}


def model(kind, interp, view, tight=True, dtype=np.float64):
    """(att, plen, frac, recs) of one view of a scene, computed once and shared."""
    key = (kind, interp, view, tight, np.dtype(dtype).name)
    if key not in _MODELS:
        S = scene(kind)
        recs = pack(scene_views(S)[view], MASKS, S['Q'], S['lab'], tight, interp)
        att, plen, frac = render(S['mu'], S['lab'], recs, S['Q'].astype(np.float32), S['rows'], S['cols'], interp, dtype=dtype)
        for a in (att, plen, frac):
            a.setflags(write=False)
        _MODELS[key] = (att, plen, frac, recs)
    return _MODELS[key]
