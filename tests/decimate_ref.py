"""numpy model of dfl_amd.mesh.decimate (csrc/decimate.hip), one function per stage.  Every
floating-point expression is written out in the kernels' order, in float64 on the fp32 positions, one rounding per
product and sum (numpy never contracts); the row loops of the kernels become loops over the position in the row with the
edges side by side.  Integer stages (topology, minima, flags, remap) need no order."""
import math

import numpy as np

KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX_ROUNDS = 64


def _row_ptr(row, n_rows):
    p = np.zeros(n_rows + 1, np.int64)
    np.add.at(p, row + 1, 1)
    return np.cumsum(p)


def topology(tris, V):
    """What mesh.decimate builds every round: the neighbour CSR (row_ptr, col) with use and eid aligned with col, the
    undirected edges (edge_u < edge_v, ascending) and the vertex-triangle CSR (vt_ptr, vt_tri)."""
    t = tris.astype(np.int64)
    T = len(t)
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    ek = np.stack([a * V + b, b * V + a, b * V + c, c * V + b, c * V + a, a * V + c], 1).reshape(-1)
    uk, cnt = np.unique(ek, return_counts=True)
    row, col = np.divmod(uk, V)
    und = row < col
    eid = np.searchsorted(uk[und], np.minimum(row, col) * V + np.maximum(row, col))
    vk = np.sort((t * (3 * T) + np.arange(3 * T).reshape(-1, 3)).reshape(-1))
    vrow, rem = np.divmod(vk, 3 * T)
    i32 = lambda x: np.ascontiguousarray(x, np.int32)            # noqa: E731
    return dict(row_ptr=i32(_row_ptr(row, V)), col=i32(col), use=i32(cnt), eid=i32(eid), edge_u=i32(row[und]),
                edge_v=i32(col[und]), vt_ptr=i32(_row_ptr(vrow, V)), vt_tri=i32(rem // 3))


def _f64(pos):
    p = pos.astype(np.float64)
    return p[..., 0], p[..., 1], p[..., 2]


def _normal(p0, p1, p2):
    """(p1 - p0) x (p2 - p0), each point an (x, y, z) triple of arrays."""
    ux, uy, uz = p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]
    wx, wy, wz = p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]
    return uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cost(q, p):
    x, y, z = p
    r0 = ((q[0] * x + q[1] * y) + q[2] * z) + q[3]
    r1 = ((q[1] * x + q[4] * y) + q[5] * z) + q[6]
    r2 = ((q[2] * x + q[5] * y) + q[7] * z) + q[8]
    r3 = ((q[3] * x + q[6] * y) + q[8] * z) + q[9]
    return ((x * r0 + y * r1) + z * r2) + r3


def _round32(p):
    return tuple(c.astype(np.float32).astype(np.float64) for c in p)


def quadrics(pos, tris, tp):
    """Q [V, 10] fp64 (aa ab ac ad bb bc bd cc cd dd): the sum of K_t over each vertex's triangles in vt_tri order."""
    V, T = len(pos), len(tris)
    p0, p1, p2 = (_f64(pos[tris[:, k]]) for k in range(3))
    n = _normal(p0, p1, p2)
    l = np.sqrt(_dot(n, n))
    d = -_dot(n, p0)
    ls = np.where(l == 0.0, 1.0, l)
    pairs = ((n[0], n[0]), (n[0], n[1]), (n[0], n[2]), (n[0], d), (n[1], n[1]), (n[1], n[2]), (n[1], d), (n[2], n[2]), (n[2], d),
             (d, d))
    K = np.stack([np.where(l == 0.0, 0.0, (a * b) / ls) for a, b in pairs], 1)
    vt_ptr, vt_tri = tp['vt_ptr'].astype(np.int64), tp['vt_tri']
    cnt = np.diff(vt_ptr)
    Q = np.zeros((V, 10))
    for k in range(int(cnt.max()) if V else 0):
        s = cnt > k
        Q[s] = Q[s] + K[vt_tri[vt_ptr[:-1][s] + k]]
    return Q


def _flips(pos, tris, tp, w, u, v, x, active):
    """bool per edge: a triangle at w without both u and v turns when u and v move to x."""
    vt_ptr, vt_tri = tp['vt_ptr'].astype(np.int64), tp['vt_tri']
    cnt = np.diff(vt_ptr)[w]
    bad = np.zeros(len(w), bool)
    for j in range(int(cnt[active].max()) if active.any() else 0):
        s = np.flatnonzero(active & (cnt > j))
        t = vt_tri[vt_ptr[w[s]] + j]
        idx = tris[t]                                              # [n, 3]
        us, vs = u[s][:, None], v[s][:, None]
        moved = (idx == us) | (idx == vs)
        both = (idx == us).any(1) & (idx == vs).any(1)
        p = [_f64(pos[idx[:, k]]) for k in range(3)]
        xs = tuple(c[s] for c in x)
        pm = [tuple(np.where(moved[:, k], xs[i], p[k][i]) for i in range(3)) for k in range(3)]
        n0, n1 = _normal(*p), _normal(*pm)
        d = _dot(n0, n1)
        turn = ~(d > 0.0) | ~(d * d >= 0.04 * (_dot(n0, n0) * _dot(n1, n1)))
        bad[s] |= turn & ~both
    return bad


def collapse_keys(pos, tris, tp, Q):
    """(key [E] uint64, cand [E, 3] fp32, the per-edge intermediates as a dict for the tests)."""
    V = len(pos)
    row_ptr, col, use = tp['row_ptr'].astype(np.int64), tp['col'].astype(np.int64), tp['use']
    u, v = tp['edge_u'].astype(np.int64), tp['edge_v'].astype(np.int64)
    E = len(u)
    deg = np.diff(row_ptr)
    rows = np.repeat(np.arange(V), deg)
    held = np.zeros(V, bool)
    held[rows[use != 2]] = True
    ok = ~held[u] & ~held[v]
    dkeys = rows * V + col                                         # ascending
    common = np.zeros(E, np.int64)
    deg_ok = np.ones(E, bool)
    for j in range(int(deg[u].max()) if E else 0):
        s = np.flatnonzero(deg[u] > j)
        w = col[row_ptr[u[s]] + j]
        want = v[s] * V + w
        at = np.minimum(np.searchsorted(dkeys, want), len(dkeys) - 1)
        member = dkeys[at] == want
        common[s] += member
        deg_ok[s] &= ~member | (deg[w] >= 5)
    ok &= (common == 2) & deg_ok & (deg[u] + deg[v] - 4 >= 3)
    with np.errstate(all='ignore'):
        q = [Q[u, i] + Q[v, i] for i in range(10)]
        pu, pv = _f64(pos[u]), _f64(pos[v])
        mid = tuple((pu[i] + pv[i]) * 0.5 for i in range(3))
        c00, c01, c02 = q[4] * q[7] - q[5] * q[5], q[2] * q[5] - q[1] * q[7], q[1] * q[5] - q[2] * q[4]
        c11, c12, c22 = q[0] * q[7] - q[2] * q[2], q[1] * q[2] - q[0] * q[5], q[0] * q[4] - q[1] * q[1]
        det = (q[0] * c00 + q[1] * c01) + q[2] * c02
        t3 = ((q[0] + q[4]) + q[7]) / 3.0
        well = det > 1e-3 * ((t3 * t3) * t3)
        s = (-(((c00 * q[3] + c01 * q[6]) + c02 * q[8]) / det), -(((c01 * q[3] + c11 * q[6]) + c12 * q[8]) / det),
             -(((c02 * q[3] + c12 * q[6]) + c22 * q[8]) / det))
        dm = tuple(s[i] - mid[i] for i in range(3))
        de = tuple(pu[i] - pv[i] for i in range(3))
        solved = well & (_dot(dm, dm) <= 4.0 * _dot(de, de))
        xs = _round32(s)
        m32 = _round32(mid)
        cm, cu, cv = _cost(q, m32), _cost(q, pu), _cost(q, pv)
        fx, fc = m32, cm
        take_u = cu < fc
        fx, fc = tuple(np.where(take_u, pu[i], fx[i]) for i in range(3)), np.where(take_u, cu, fc)
        take_v = cv < fc
        fx, fc = tuple(np.where(take_v, pv[i], fx[i]) for i in range(3)), np.where(take_v, cv, fc)
        x = tuple(np.where(solved, xs[i], fx[i]) for i in range(3))
        cost = np.where(solved, _cost(q, xs), fc)
        cost = np.where(cost > 0.0, cost, 0.0)
        ok_topo = ok.copy()
        ok &= ~_flips(pos, tris, tp, u, u, v, x, ok_topo) & ~_flips(pos, tris, tp, v, u, v, x, ok_topo)
        bits = cost.astype(np.float32).view(np.uint32).astype(np.uint64)
    key = np.where(ok, (bits << np.uint64(32)) | np.arange(E, dtype=np.uint64), KEY_NONE)
    cand = np.where(ok[:, None], np.stack(x, 1), 0.0).astype(np.float32)
    return key, cand, dict(topo=ok_topo, solved=solved, held=held, cost=cost)


def select_m1(key, tp):
    V = len(tp['row_ptr']) - 1
    rows = np.repeat(np.arange(V), np.diff(tp['row_ptr'].astype(np.int64)))
    m1 = np.full(V, KEY_NONE, np.uint64)
    np.minimum.at(m1, rows, key[tp['eid']])
    return m1


def select_m2(m1, tp):
    V = len(m1)
    rows = np.repeat(np.arange(V), np.diff(tp['row_ptr'].astype(np.int64)))
    m2 = m1.copy()
    np.minimum.at(m2, rows, m1[tp['col']])
    return m2


def select_flags(key, m2, tp):
    return ((key != KEY_NONE) & (m2[tp['edge_u']] == key) & (m2[tp['edge_v']] == key)).astype(np.uint8)


def budget_cut(key, sel, remaining):
    """take [E] uint8: the selected edges, the `remaining` lowest keys of them when there are more."""
    idx = np.flatnonzero(sel)
    if len(idx) > remaining:
        idx = idx[np.argsort(key[idx], kind='stable')[:remaining]]
    take = np.zeros(len(sel), np.uint8)
    take[idx] = 1
    return take


def apply(pos, tris, tp, take, cand):
    """(remap [V] int32, pos_out [V, 3] fp32, tris_out [T, 3] int32, degen [T] uint8)."""
    e = np.flatnonzero(take)
    remap = np.arange(len(pos), dtype=np.int32)
    remap[tp['edge_v'][e]] = tp['edge_u'][e]
    pos_out = pos.copy()
    pos_out[tp['edge_u'][e]] = cand[e]
    tris_out = remap[tris]
    degen = ((tris_out[:, 0] == tris_out[:, 1]) | (tris_out[:, 1] == tris_out[:, 2]) | (tris_out[:, 2] == tris_out[:, 0]))
    return remap, pos_out, tris_out, degen.astype(np.uint8)


def compact(remap, pos_out, tris_out, degen):
    keep = remap == np.arange(len(remap))
    new_id = (np.cumsum(keep) - 1).astype(np.int32)
    return pos_out[keep], new_id[tris_out[degen == 0]]


def budget(reduction, T):
    return int(math.floor(float(reduction) * T)) // 2


def one_round(pos, tris, remaining):
    """(pos', tris', collapses, stages) of one round on the current mesh."""
    tp = topology(tris, len(pos))
    Q = quadrics(pos, tris, tp)
    key, cand, _ = collapse_keys(pos, tris, tp, Q)
    m1 = select_m1(key, tp)
    m2 = select_m2(m1, tp)
    sel = select_flags(key, m2, tp)
    take = budget_cut(key, sel, remaining)
    n = int(take.sum())
    st = dict(tp=tp, Q=Q, key=key, cand=cand, m1=m1, m2=m2, sel=sel, take=take)
    if n == 0:
        return pos, tris, 0, st
    return compact(*apply(pos, tris, tp, take, cand)) + (n, st)


def decimate(pos, tris, reduction=0.25, max_rounds=MAX_ROUNDS):
    """(pos', tris', info) as mesh.decimate; info also lists the collapses of every round."""
    pos, tris = np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(tris, np.int32)
    B = budget(reduction, len(tris))
    done, per_round = 0, []
    while done < B and len(per_round) < max_rounds:
        pos, tris, n, _ = one_round(pos, tris, B - done)
        if n == 0:
            break
        done += n
        per_round.append(n)
    return pos, tris, dict(collapses=done, rounds=len(per_round), budget=B, per_round=per_round)


# ---- meshes of the tests ------------------------------------------------------------------------------------------------
TETRA = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)      # closed, consistently wound
TETRA_IDS = np.array([1, 2, 4, 6], np.int32)                                  # of 8: 0, 3, 5 and 7 are in no triangle
FAN = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]], np.int32)                   # three triangles on the edge (0, 1)


def random_points(V, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (V, 3)).astype(np.float32)


def torus_grid(n, m, seed=0, jitter=0.02):
    """A closed n x m grid on a torus (V = n m, every degree 6), vertices jittered so that no two costs tie."""
    i, j = np.mgrid[:n, :m]
    th, ph = 2 * np.pi * i / n, 2 * np.pi * j / m
    pos = np.stack([(1 + 0.4 * np.cos(ph)) * np.cos(th), (1 + 0.4 * np.cos(ph)) * np.sin(th), 0.4 * np.sin(ph)], -1).reshape(-1, 3)
    pos += np.random.default_rng(seed).uniform(-jitter, jitter, pos.shape)
    a, b, c, d = i * m + j, ((i + 1) % n) * m + j, ((i + 1) % n) * m + (j + 1) % m, i * m + (j + 1) % m
    tris = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], 2).reshape(-1, 3)
    return pos.astype(np.float32), tris.astype(np.int32)


def uv_sphere(rings, seg, seed=0, jitter=0.01):
    """A closed sphere of two poles and rings x seg points (V = rings seg + 2), jittered."""
    phi = np.pi * np.arange(1, rings + 1) / (rings + 1)
    th = 2 * np.pi * np.arange(seg) / seg
    ring = np.stack([np.outer(np.sin(phi), np.cos(th)), np.outer(np.sin(phi), np.sin(th)), np.repeat(np.cos(phi)[:, None], seg, 1)],
                    -1).reshape(-1, 3)
    pos = np.concatenate([[[0, 0, 1]], ring, [[0, 0, -1]]])
    pos += np.random.default_rng(seed).uniform(-jitter, jitter, pos.shape)
    at = lambda k, j: 1 + k * seg + j % seg        # noqa: E731
    tris = []
    for j in range(seg):
        tris.append((0, at(0, j), at(0, j + 1)))
        for k in range(rings - 1):
            a, b, c, d = at(k, j), at(k + 1, j), at(k + 1, j + 1), at(k, j + 1)
            tris += [(a, b, c), (a, c, d)]
        tris.append((len(pos) - 1, at(rings - 1, j + 1), at(rings - 1, j)))
    return pos.astype(np.float32), np.array(tris, np.int32)
