"""numpy model of the rasteriser (include/dfl_hip.h "Rasteriser", csrc/raster.hip): the vertex stage, depth and shading
step by step in float32 -- every product and sum rounded on its own, as the kernel is built with -ffp-contract=off --
and coverage in int64.  dtype=np.float64 gives the variant whose depth and shading carry no float32 rounding: clip
values, weights, depth and colour in float64.  What the definition decides in whole numbers is the float32 stage's in
both: the snapped coordinates (so the coverage is the same) and, where both variants see the same triangle, the texel
of a NEAREST lookup -- a sample centre that lies on a texel edge (the source view puts the detector's texel grid on the
sample grid) is a tie that either arithmetic breaks by its last bit, and the variant measures rounding, not ties.  The
texel choice itself is held exactly: against the float32 model on the GPU and against a texture laid out by hand.

A scene is a list of Rec.  draw() returns what dfl_raster_draw writes."""
import numpy as np

UNLIT, TEXTURED = 1, 2
SMALL_BOX = 16
GUARD = 4194304.0
DRAWN, NEAR, GUARDED, DEGENERATE = 0, 1, 2, 3
F32 = np.float32


class Rec:
    def __init__(self, pos, tris, mvp, first_prim=0, nrm=None, uv=None, tex=None, nmat=None, rgb=(1, 1, 1), flags=0):
        self.pos = np.ascontiguousarray(pos, F32).reshape(-1, 3)
        self.tris = np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
        self.mvp = np.asarray(mvp, np.float64).astype(F32).reshape(16)          # the host's one rounding
        self.nmat = (np.eye(3) if nmat is None else np.asarray(nmat, np.float64)).astype(F32).reshape(9)
        self.nrm = None if nrm is None else np.ascontiguousarray(nrm, F32).reshape(-1, 3)
        self.uv = None if uv is None else np.ascontiguousarray(uv, F32).reshape(-1, 2)
        self.tex = None if tex is None else np.ascontiguousarray(tex, np.uint8)
        self.rgb = np.asarray(rgb, np.float64).astype(F32).reshape(3)
        self.flags, self.first_prim = int(flags), int(first_prim)


def _row(m, k, x, y, z, n=4):
    """((m[nk] x + m[nk+1] y) + m[nk+2] z) (+ m[nk+3]) in the dtype of x."""
    t = x.dtype.type
    r = (t(m[n * k]) * x + t(m[n * k + 1]) * y) + t(m[n * k + 2]) * z
    return r + t(m[n * k + 3]) if n == 4 else r


def vertex_stage(rec, Ws, Hs, znear, dtype=F32):
    """status [T], X, Y int64 [T, 3] (always from the float32 stage), zd, w [T, 3] in dtype."""
    T = len(rec.tris)
    ok_idx = np.all((rec.tris >= 0) & (rec.tris < len(rec.pos)), axis=1) if T else np.zeros(0, bool)
    p = rec.pos[np.where(ok_idx[:, None], rec.tris, 0)] if len(rec.pos) else np.zeros((T, 3, 3), F32)
    out = {}
    with np.errstate(all='ignore'):
        for t in (F32, dtype):
            x, y, z = (p[..., k].astype(t) for k in range(3))
            c = [_row(rec.mvp, k, x, y, z) for k in range(4)]
            w = c[3]
            fin = np.isfinite(c[0]) & np.isfinite(c[1]) & np.isfinite(c[2]) & np.isfinite(w)
            behind = ~fin | (w < t(znear))
            px = (c[0] / w + t(1)) * (t(0.5) * t(Ws))
            py = (t(1) - c[1] / w) * (t(0.5) * t(Hs))
            X, Y = np.rint(t(256) * px), np.rint(t(256) * py)
            out[t] = (behind, X, Y, c[2] / w, w)
            if dtype is F32:
                break
    behind, X, Y, _, _ = out[F32]
    _, _, _, zd, w = out[dtype]
    guard = ~((np.abs(X) <= GUARD) & (np.abs(Y) <= GUARD))
    near_t, guard_t = behind.any(1), (guard & ~behind).any(1)
    keep = ok_idx & ~near_t & ~guard_t
    Xi = np.where(keep[:, None], X, 0).astype(np.int64)
    Yi = np.where(keep[:, None], Y, 0).astype(np.int64)
    A = (Xi[:, 1] - Xi[:, 0]) * (Yi[:, 2] - Yi[:, 0]) - (Yi[:, 1] - Yi[:, 0]) * (Xi[:, 2] - Xi[:, 0])
    status = np.full(T, DRAWN)
    status[A == 0] = DEGENERATE
    status[guard_t] = GUARDED
    status[near_t] = NEAR
    status[~ok_idx] = DEGENERATE
    return status, Xi, Yi, A, zd, w


def boxes(X, Y, Ws, Hs):
    i0 = np.maximum((X.min(1) + 127) >> 8, 0)
    i1 = np.minimum((X.max(1) - 128) >> 8, Ws - 1)
    j0 = np.maximum((Y.min(1) + 127) >> 8, 0)
    j1 = np.minimum((Y.max(1) - 128) >> 8, Hs - 1)
    return i0, i1, j0, j1


def edges(X, Y, A, i, j):
    """E [n, 3] (int64, orientation normalised) and the coverage of samples (i, j) by triangles X, Y, A (all [n, ...])."""
    s = np.sign(A)
    Px, Py = 256 * i + 128, 256 * j + 128
    E = np.empty((len(A), 3), np.int64)
    inside = np.ones(len(A), bool)
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        dx, dy = s * (X[:, b] - X[:, a]), s * (Y[:, b] - Y[:, a])
        E[:, k] = dx * (Py - Y[:, a]) - dy * (Px - X[:, a])
        inside &= (E[:, k] > 0) | ((E[:, k] == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))
    return E, inside


def candidates(scene, Ws, Hs, znear, dtype=F32):
    """Every (sample, triangle) pair that is covered, before the depth test: a dict of equally long arrays, plus counts."""
    cols = dict(pix=[], rec=[], tri=[], E=[], A=[], zd=[], w=[])
    counts = np.zeros(4, np.int64)
    n_large = 0
    for r, rec in enumerate(scene):
        status, X, Y, A, zd, w = vertex_stage(rec, Ws, Hs, znear, dtype)
        counts += np.bincount(status, minlength=4)
        i0, i1, j0, j1 = boxes(X, Y, Ws, Hs)
        live = np.nonzero((status == DRAWN) & (i0 <= i1) & (j0 <= j1))[0]
        if not len(live):
            continue
        bw, bh = (i1 - i0 + 1)[live], (j1 - j0 + 1)[live]
        n_large += int(np.sum((bw > SMALL_BOX) | (bh > SMALL_BOX)))
        small = (bw <= 32) & (bh <= 32)
        groups = []
        sm = live[small]
        if len(sm):                                       # all small boxes at once, one offset at a time
            for dj in range(int(bh[small].max())):
                for di in range(int(bw[small].max())):
                    sel = sm[(i0[sm] + di <= i1[sm]) & (j0[sm] + dj <= j1[sm])]
                    groups.append((sel, i0[sel] + di, j0[sel] + dj))
        for t in live[~small]:                            # a large box: all its samples at once
            jj, ii = np.mgrid[j0[t]:j1[t] + 1, i0[t]:i1[t] + 1]
            groups.append((np.full(ii.size, t), ii.reshape(-1), jj.reshape(-1)))
        for sel, i, j in groups:
            if not len(sel):
                continue
            E, inside = edges(X[sel], Y[sel], A[sel], i, j)
            sel, E, i, j = sel[inside], E[inside], i[inside], j[inside]
            cols['pix'].append(j * Ws + i)
            cols['rec'].append(np.full(len(sel), r))
            cols['tri'].append(sel)
            cols['E'].append(E)
            cols['A'].append(np.abs(A[sel]))
            cols['zd'].append(zd[sel])
            cols['w'].append(w[sel])
    shapes = dict(E=(0, 3), zd=(0, 3), w=(0, 3))
    kinds = dict(zd=dtype, w=dtype)
    c = {k: (np.concatenate(v) if v else np.zeros(shapes.get(k, (0,)), kinds.get(k, np.int64))) for k, v in cols.items()}
    c['counts'], c['n_large'] = counts, n_large
    return c


def depths(c, dtype=F32):
    """l [n, 3] and depth [n] of the candidates in dtype; the validity 0 <= depth <= 1."""
    with np.errstate(all='ignore'):
        l = c['E'].astype(dtype) / c['A'].astype(dtype)[:, None]
        zd = c['zd'].astype(dtype)
        d = (l[:, 0] * zd[:, 0] + l[:, 1] * zd[:, 1]) + l[:, 2] * zd[:, 2]
    ok = (d >= 0) & (d <= 1)
    return l, np.where(d == 0, dtype(0), d), ok


def winners(scene, c, l, d, ok, S):
    """Per sample the candidate with the least (depth, primitive id): index into the candidates, -1 for background."""
    prim = np.array([rec.first_prim for rec in scene], np.int64)[c['rec']] + c['tri'] if len(c['pix']) else np.zeros(0, np.int64)
    idx = np.nonzero(ok)[0]
    order = idx[np.lexsort((prim[idx], d[idx], c['pix'][idx]))]
    first = np.ones(len(order), bool)
    first[1:] = c['pix'][order][1:] != c['pix'][order][:-1]
    win = np.full(S, -1, np.int64)
    win[c['pix'][order][first]] = order[first]
    return win, prim


def _mix(b, q):
    return (b[:, 0] * q[:, 0] + b[:, 1] * q[:, 1]) + b[:, 2] * q[:, 2]


def shade(scene, c, l, win, ambient, diffuse, background, dtype=F32, texels=None):
    """Sample colours before quantisation, [S, 3] in dtype, and the texel (column, row) of every textured sample, [S, 2]
    (-1 elsewhere).  texels = (ids, texel) of the float32 stage: taken over where ids equals this stage's winner."""
    t = dtype
    S = len(win)
    out = np.empty((S, 3), t)
    texel_of = np.full((S, 2), -1, np.int64)
    out[:] = np.asarray(background, np.float64).astype(F32).astype(t)
    with np.errstate(all='ignore'):
        for r, rec in enumerate(scene):
            px = np.nonzero((win >= 0) & (c['rec'][np.maximum(win, 0)] == r))[0]
            if not len(px):
                continue
            k = win[px]
            b = l[k].astype(t) / c['w'][k].astype(t)
            b = b / ((b[:, 0] + b[:, 1]) + b[:, 2])[:, None]
            vi = rec.tris[c['tri'][k]]
            base = np.repeat(rec.rgb.astype(t)[None], len(px), 0)
            if rec.flags & TEXTURED:
                th, tw = rec.tex.shape
                u = _mix(b, rec.uv[vi][:, :, 0].astype(t))
                v = _mix(b, rec.uv[vi][:, :, 1].astype(t))
                fx = np.minimum(np.maximum(np.floor(u * t(tw)), t(0)), t(tw - 1))
                fy = np.minimum(np.maximum(np.floor(v * t(th)), t(0)), t(th - 1))
                fx, fy = np.where(np.isnan(fx), 0, fx).astype(np.int64), np.where(np.isnan(fy), 0, fy).astype(np.int64)
                if texels is not None:
                    same = texels[0][px] == rec.first_prim + c['tri'][k]
                    fx, fy = np.where(same, texels[1][px, 0], fx), np.where(same, texels[1][px, 1], fy)
                texel_of[px, 0], texel_of[px, 1] = fx, fy
                texel = rec.tex[fy, fx].astype(t) / t(255)
                base = base * texel[:, None]
            if not rec.flags & UNLIT:
                n = [_mix(b, rec.nrm[vi][:, :, a].astype(t)) for a in range(3)]
                rr = [_row(rec.nmat, a, n[0], n[1], n[2], 3) for a in range(3)]
                ln = np.sqrt((rr[0] * rr[0] + rr[1] * rr[1]) + rr[2] * rr[2])
                facing = np.where(ln > 0, np.abs(rr[2]) / np.where(ln > 0, ln, 1), t(0)).astype(t)
                base = base * (t(F32(ambient)) + t(F32(diffuse)) * facing)[:, None]
            out[px] = base
    return out, texel_of


def to_bytes(col):
    t = col.dtype.type
    with np.errstate(all='ignore'):
        u = np.minimum(np.maximum(col, t(0)), t(1))
        u = np.where(np.isnan(col), t(0), u)
        return np.rint(t(255) * u).astype(np.uint8)


def resolve(samples, W, H, ssaa):
    s = samples.reshape(H, ssaa, W, ssaa, 3).astype(np.int64).sum(axis=(1, 3))
    return ((s + ssaa * ssaa // 2) // (ssaa * ssaa)).astype(np.uint8)


def draw(scene, W, H, ssaa=1, znear=1e-3, ambient=0.2, diffuse=0.8, background=(0, 0, 0), dtype=F32, own_texels=False):
    """dict(rgb uint8 [H, W, 3], ids int32 [Hs, Ws], depth dtype [Hs, Ws], counts [4], colour [Hs, Ws, 3] before quantisation,
    samples uint8 [Hs, Ws, 3], n_large)."""
    Ws, Hs = W * ssaa, H * ssaa
    c = candidates(scene, Ws, Hs, znear, dtype)
    l, d, ok = depths(c, dtype)
    win, prim = winners(scene, c, l, d, ok, Ws * Hs)
    ids = np.where(win >= 0, prim[np.maximum(win, 0)] if len(prim) else 0, -1).astype(np.int64)
    depth = np.where(win >= 0, d[np.maximum(win, 0)] if len(d) else 0, np.inf).astype(dtype)
    texels = None
    if dtype is not F32 and not own_texels:          # (own_texels: the variant's own choice, for the floor to count the ties)
        first = draw(scene, W, H, ssaa, znear, ambient, diffuse, background)
        texels = (first['ids'].reshape(-1).astype(np.int64), first['texel'])
    col, texel_of = shade(scene, c, l, win, ambient, diffuse, background, dtype, texels)
    samples = to_bytes(col)
    return dict(rgb=resolve(samples, W, H, ssaa),
                ids=np.where(ids < 0, 0xffffffff, ids).astype(np.uint32).view(np.int32).reshape(Hs, Ws),
                depth=depth.reshape(Hs, Ws), counts=c['counts'], colour=col.reshape(Hs, Ws, 3),
                samples=samples.reshape(Hs, Ws, 3), n_large=c['n_large'], texel=texel_of, cand=c, l=l, d=d, ok=ok, win=win)
