"""Fixed scenes for the rasteriser tests (tests/test_raster_cpu.py, tests/test_gpu_raster.py, tests/raster_floor.py):
nothing here is random at test time.  A scene is dict(specs, view, proj, W, H, ssaa, near); a spec is a dict of numpy
arrays in the vocabulary of dfl_amd.raster.Mesh.  recs() turns a scene into the model's records (tests/raster_ref.py)
by the arithmetic of dfl_amd.raster.records: fp64 products, one rounding to fp32."""
import numpy as np

import raster_ref as RR

W0, H0 = 64, 48


def pixel_proj(W, H):
    """(x, y, z) in samples of a W x H image and depth -> clip, w = 1."""
    P = np.eye(4)
    P[0, 0], P[0, 3] = 2.0 / W, -1.0
    P[1, 1], P[1, 3] = -2.0 / H, 1.0
    return P


def spec(pos, tris, rgb=(1.0, 1.0, 1.0), nrm=None, uv=None, tex=None, unlit=None, matrix=None):
    return dict(pos=np.asarray(pos, np.float32).reshape(-1, 3), tris=np.asarray(tris, np.int32).reshape(-1, 3),
                rgb=tuple(rgb), nrm=None if nrm is None else np.asarray(nrm, np.float32).reshape(-1, 3),
                uv=None if uv is None else np.asarray(uv, np.float32).reshape(-1, 2), tex=tex,
                unlit=(nrm is None) if unlit is None else unlit, matrix=np.eye(4) if matrix is None else np.asarray(matrix, np.float64))


def scene(specs, W=W0, H=H0, ssaa=1, view=None, proj=None, near=1e-3):
    return dict(specs=list(specs), W=W, H=H, ssaa=ssaa, near=near, view=np.eye(4) if view is None else view,
                proj=pixel_proj(W, H) if proj is None else proj)


def recs(sc):
    out, first = [], 0
    for s in sc['specs']:
        mv = sc['view'] @ s['matrix']
        out.append(RR.Rec(s['pos'], s['tris'], sc['proj'] @ mv, first_prim=first, nrm=s['nrm'], uv=s['uv'], tex=s['tex'],
                          nmat=np.linalg.inv(mv[:3, :3]).T, rgb=s['rgb'],
                          flags=(RR.UNLIT if s['unlit'] else 0) | (RR.TEXTURED if s['tex'] is not None else 0)))
        first += len(s['tris'])
    return out


def model(sc, dtype=np.float32, **kw):
    return RR.draw(recs(sc), sc['W'], sc['H'], sc['ssaa'], znear=sc['near'], dtype=dtype, **kw)


def tri(p0, p1, p2, **kw):
    return spec([p0, p1, p2], [[0, 1, 2]], **kw)


def small_cloud(n, W, H, seed):
    """n small triangles (1 to 4 samples) spread over the image by a fixed linear congruential sequence."""
    v = np.empty(n * 8)
    x = seed
    for k in range(len(v)):
        x = (1103515245 * x + 12345) % 2 ** 31
        v[k] = x / 2.0 ** 31
    v = v.reshape(n, 8)
    c = np.stack([v[:, 0] * (W + 8) - 4, v[:, 1] * (H + 8) - 4], 1)
    pos = np.empty((n, 3, 3))
    for k in range(3):
        pos[:, k, 0] = c[:, 0] + 3.0 * (v[:, 2 + 2 * k] - 0.5)
        pos[:, k, 1] = c[:, 1] + 3.0 * (v[:, 3 + 2 * k] - 0.5)
        pos[:, k, 2] = 0.1 + 0.8 * v[:, (k + 5) % 8]
    return spec(pos.reshape(-1, 3), np.arange(3 * n).reshape(n, 3))


def box_triangle(x0, y0, n, z=0.5):
    """A right triangle whose bounding box holds exactly n x n sample centres, from sample (x0, y0)."""
    return [(x0 + 0.25, y0 + 0.25, z), (x0 + n - 0.25, y0 + 0.25, z), (x0 + 0.25, y0 + n - 0.25, z)]


def perspective_pair():
    """Two interpenetrating triangles and a far quad under a real perspective camera (w differs at every corner)."""
    import dfl_amd.raster as R
    view = R.look_at((0.3, 0.4, 5.0), (0, 0, 0), (0, 1, 0))
    proj = R.perspective(40.0, W0 / H0, 1.0, 20.0)
    a = tri((-1.5, -1.0, -1.0), (1.5, -0.8, 1.0), (0.0, 1.3, 0.2), rgb=(1.0, 0.2, 0.1),
            nrm=[(0.2, 0.1, 1.0), (-0.3, 0.2, 0.9), (0.0, -0.4, 0.8)])
    b = tri((-1.4, 0.9, 1.0), (1.2, 1.0, -1.0), (0.1, -1.4, 0.1), rgb=(0.1, 0.9, 0.3),
            nrm=[(0.0, 0.0, 1.0), (0.5, 0.0, 0.5), (0.0, 0.6, 0.6)])
    q = spec([(-2.5, -2, -2), (2.5, -2, -2.5), (2.5, 2, -2), (-2.5, 2, -1.5)], [[0, 1, 2], [0, 2, 3]], rgb=(0.8, 0.8, 0.8),
             nrm=[(0, 0, 1)] * 4)
    return view, proj, [a, b, q]


def texture(th=5, tw=7):
    return ((np.arange(th * tw).reshape(th, tw) * 37 + 11) % 256).astype(np.uint8)


def cases():
    """name -> scene: the cases of the issue that compare ids and depth bits (64 x 48 unless the name says otherwise)."""
    c = {}
    c['pixel_centres'] = scene([tri((4.5, 4.5, 0.3), (30.5, 4.5, 0.3), (4.5, 25.5, 0.6))])
    c['shared_edge'] = scene([spec([(5.5, 6.5, 0.2), (40.5, 9.5, 0.4), (35.5, 36.5, 0.7), (8.5, 30.5, 0.5)], [[0, 1, 2], [0, 2, 3]])])
    c['back_facing'] = scene([tri((10, 5, 0.5), (12, 40, 0.5), (50, 20, 0.25))])
    c['interpenetrating'] = scene([tri((2, 3, 0.1), (60, 8, 0.9), (20, 45, 0.5), rgb=(1, 0, 0)),
                                   tri((3, 40, 0.1), (58, 44, 0.2), (30, 2, 0.95), rgb=(0, 1, 0))])
    dup = [(6, 6, 0.5), (50, 10, 0.5), (20, 42, 0.5)]
    c['coplanar_duplicates'] = scene([tri(*dup, rgb=(1, 0, 0)), tri(*dup, rgb=(0, 0, 1)), tri(*dup[::-1], rgb=(0, 1, 0))])
    c['degenerate_and_offscreen'] = scene([tri((5, 5, 0.5), (20, 20, 0.5), (35, 35, 0.5)),
                                           tri((-30, -30, 0.5), (-5, -20, 0.5), (-10, -2, 0.5)),
                                           tri((-20, 10, 0.4), (30, -15, 0.4), (40, 70, 0.6)),
                                           tri((3, 3, 0.5), (3, 3, 0.5), (9, 9, 0.5))])
    view, proj, three = perspective_pair()
    c['perspective'] = scene(three, view=view, proj=proj, near=1.0)
    # one corner behind the near plane: dropped whole, while its neighbour stays
    c['behind_near'] = scene([tri((-1.0, -1.0, 0.0), (1.0, -1.0, 0.0), (0.0, 0.5, 4.5)), three[0]], view=view, proj=proj, near=1.0)
    c['guard_band'] = scene([tri((10, 10, 0.5), (40, 12, 0.5), (20000, 30, 0.5)), tri((10, 20, 0.6), (40, 22, 0.6), (16000, 40, 0.6)),
                             tri((5, 5, 0.7), (30, 8, 0.7), (12, 30, 0.7))])
    c['both_paths'] = scene([spec([(-3, -2, 0.9), (70, -3, 0.8), (72, 50, 0.9), (-4, 52, 0.85)], [[0, 1, 2], [0, 2, 3]], rgb=(0.5, 0.5, 0.5)),
                             small_cloud(300, W0, H0, 7)])
    n = RR.SMALL_BOX
    c['box_threshold'] = scene([tri(*box_triangle(2, 3, n)), tri(*box_triangle(24, 5, n + 1)), tri(*box_triangle(44, 20, n - 1, 0.4)),
                                spec(box_triangle(1, 26, n + 1, 0.3) + box_triangle(20, 28, n, 0.6), [[0, 1, 2], [3, 4, 5]])])
    c['67x45'] = scene([spec([(-3, -2, 0.9), (70, -3, 0.8), (72, 50, 0.9)], [[0, 1, 2]]), small_cloud(200, 67, 45, 11)], W=67, H=45)
    c['1x1'] = scene([tri((-2, -2, 0.5), (4, -1, 0.5), (0, 5, 0.25)), tri((0.6, 0.6, 0.1), (0.9, 0.6, 0.1), (0.6, 0.9, 0.1))], W=1, H=1)
    for s in (1, 2, 3, 4):
        sp = [spec(np.asarray(x['pos'], np.float64) * [s, s, 1], x['tris'], rgb=x['rgb']) for x in
              (c['interpenetrating']['specs'] + [small_cloud(150, W0, H0, 5)])]
        c['ssaa%d' % s] = scene(sp, ssaa=s, proj=pixel_proj(W0 * s, H0 * s))
    c['empty'] = scene([])
    c['empty_record'] = scene([spec(np.zeros((0, 3)), np.zeros((0, 3))), tri((4, 4, 0.5), (30, 6, 0.5), (10, 30, 0.5)),
                               spec(np.zeros((3, 3)), np.zeros((0, 3)))])
    # two records sharing buffers under different matrices (instances); a third shifted in depth in front of the first
    base = spec([(0, 0, 0.5), (18, 2, 0.5), (5, 16, 0.5)], [[0, 1, 2]])
    inst = []
    for dx, dy, dz in ((3, 4, 0.0), (30, 20, 0.0), (6, 6, -0.25)):
        M = np.eye(4)
        M[:3, 3] = (dx, dy, dz)
        inst.append(dict(base, matrix=M, rgb=(dx / 30.0, dy / 20.0, 1.0)))
    c['instances'] = scene(inst)
    c['bad_index'] = scene([spec([(3, 3, 0.5), (30, 5, 0.5), (10, 30, 0.5)], [[0, 1, 2], [0, 1, 3], [-1, 1, 2]])])
    return c


def contention(equal):
    """4096 copies of one small triangle over sample (10, 7): depth falls with the index, or all equal."""
    n = 4096
    z = np.full(n, 0.5) if equal else 0.9 - 0.8 * np.arange(n) / n
    one = np.array([(9.75, 6.75), (11.4, 6.9), (10.2, 8.3)])
    pos = np.concatenate([np.repeat(one[None], n, 0), np.repeat(z[:, None, None], 3, 1)], 2)
    return scene([spec(pos.reshape(-1, 3), np.arange(3 * n).reshape(n, 3))])


def shading_scene():
    """Lit, unlit and textured records under the perspective camera: the fixture of the shading bars."""
    view, proj, three = perspective_pair()
    tex = texture()
    # a textured unlit quad whose uv reach 0 and 1 exactly, and a lit textured one
    quad = [(-2.2, -1.6, 0.6), (-0.2, -1.6, 0.8), (-0.2, -0.2, 0.9), (-2.2, -0.2, 0.7)]
    uvq = [(0, 0), (1, 0), (1, 1), (0, 1)]
    t_unlit = spec(quad, [[0, 1, 2], [0, 2, 3]], uv=uvq, tex=tex, unlit=True)
    quad2 = [(0.3, 0.2, 1.2), (2.1, 0.3, 1.3), (2.0, 1.5, 1.1), (0.2, 1.4, 1.25)]
    t_lit = spec(quad2, [[0, 1, 2], [0, 2, 3]], uv=uvq, tex=tex, nrm=[(0.1, 0.2, 1.0)] * 4, rgb=(1.0, 0.9, 0.8))
    flat = tri((-2.0, 0.4, 1.0), (-0.6, 0.5, 1.4), (-1.2, 1.6, 1.1), rgb=(0.25, 0.5, 0.75))       # unlit, plain
    return scene(three + [t_unlit, t_lit, flat], view=view, proj=proj, near=1.0)


def texel_edges():
    """An unlit textured quad in sample space whose texels are 4 x 4 samples each: sample centres never fall on a texel
    edge, the corner uv are exactly 0 and 1, and a second quad runs its uv from just inside 0 to just inside 1."""
    tex = texture(4, 8)
    q1 = spec([(0, 0, 0.5), (32, 0, 0.5), (32, 16, 0.5), (0, 16, 0.5)], [[0, 1, 2], [0, 2, 3]], uv=[(0, 0), (1, 0), (1, 1), (0, 1)],
              tex=tex, unlit=True)
    e = 1e-6
    q2 = spec([(0, 20, 0.5), (32, 20, 0.5), (32, 36, 0.5), (0, 36, 0.5)], [[0, 1, 2], [0, 2, 3]],
              uv=[(e, e), (1 - e, e), (1 - e, 1 - e), (e, 1 - e)], tex=tex, unlit=True, rgb=(1.0, 0.5, 0.25))
    return scene([q1, q2])


def texel_ties():
    """A lit textured quad over 30 x 15 samples with an 8 x 4 texture: 3.75 samples per texel, so every other texel edge
    passes through sample centres -- ties that float32 and float64 break by their last bit."""
    tex = texture(4, 8)
    q = spec([(0, 0, 0.5), (30, 0, 0.5), (30, 15, 0.5), (0, 15, 0.5)], [[0, 1, 2], [0, 2, 3]], uv=[(0, 0), (1, 0), (1, 1), (0, 1)],
             tex=tex, nrm=[(0.3, 0.2, 1.0)] * 4, rgb=(1.0, 0.8, 0.6))
    return scene([q])
