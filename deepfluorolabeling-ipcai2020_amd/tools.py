"""Surgical tools in rendered views: straight wires, drills and screws as analytic capsules, beads as spheres, added to
the line integrals of dfl_amd.drr.render by csrc/drr_tools.hip (dfl_drr_tools) before dfl_amd.synth.expose turns them
into detector counts.  include/dfl_hip.h ("Tools") is the definition, DESIGN.md section 27 the discussion,
tests/tools_ref.py the numpy restatement.

A capsule (a, b, r, mu) is every point within r mm of the segment [a, b]; a and b are in mm in the camera projective
frame -- the frame drr.Obj.c2i maps from, the source at its origin -- and mu is per mm.  The ray of output pixel (c, r) of
a drr.Grid is t Q [c, r, 1], t >= 0.  Every pixel gets sum_j mu_j len_j added, len_j the chord of capsule j along its ray.
Metal adds to the tissue it displaces, overlapping capsules count twice, the attenuation is monoenergetic, and the label
map is not touched.

Tensors on the CPU are refused: there is no CPU path.
"""
import ctypes as C

import numpy as np
import torch

from . import _native as nat

__all__ = ['Capsule', 'pixel_rect', 'pack', 'add_tools', 'sample_tools', 'lands_in_camera', 'TOOL_DTYPE', 'TOOL_DEFAULTS',
           'UNIFORMS_PER_TOOL', 'NORMALS_PER_TOOL']

TOOL_DTYPE = np.dtype([('a', np.float32, 3), ('b', np.float32, 3), ('r', np.float32), ('mu', np.float32), ('rect', np.int32, 4)])
assert TOOL_DTYPE.itemsize == C.sizeof(nat.ToolsCapsule) == 48
# Parameters of sample_tools, not measurements of any instrument or alloy
TOOL_DEFAULTS = dict(bead_prob=0.25, anchor_sigma_mm=30.0, length_mm=(60.0, 220.0), wire_radius_mm=(0.5, 1.6), bead_radius_mm=0.75,
                     tool_mu=0.5)
UNIFORMS_PER_TOOL, NORMALS_PER_TOOL = 5, 6


class Capsule:
    """(a, b, r, mu) in float64, checked: finite, r > 0, mu >= 0.  a == b is a bead."""

    def __init__(self, a, b, r, mu):
        self.a, self.b = np.array(a, np.float64).reshape(-1), np.array(b, np.float64).reshape(-1)
        self.r, self.mu = float(r), float(mu)
        if self.a.shape != (3,) or self.b.shape != (3,):
            raise nat.DflError('tools.Capsule: a and b must have three components each')
        if not (np.isfinite(self.a).all() and np.isfinite(self.b).all() and np.isfinite(self.r) and np.isfinite(self.mu)):
            raise nat.DflError('tools.Capsule: a value that is not finite (a %s, b %s, r %r, mu %r)' % (self.a, self.b, r, mu))
        if not self.r > 0:
            raise nat.DflError('tools.Capsule: r must be positive, got %r' % (r,))
        if not self.mu >= 0:
            raise nat.DflError('tools.Capsule: mu must not be negative, got %r' % (mu,))

    def row(self):
        """float64 [8]: a, b, r, mu -- a row of 'tools/capsules'."""
        return np.concatenate([self.a, self.b, [self.r, self.mu]])

    @classmethod
    def from_row(cls, row):
        row = np.asarray(row, np.float64).reshape(-1)
        if row.size != 8:
            raise nat.DflError('tools.Capsule.from_row: 8 numbers (a, b, r, mu) expected, got %d' % row.size)
        return cls(row[0:3], row[3:6], row[6], row[7])


def pixel_rect(capsule, grid):
    """(c0, r0, c1, r1), inclusive: a rectangle of output pixels outside which the capsule's chord is 0; (0, 0, -1, -1)
    when it misses the image.  The two ends are projected through inv(Q); the box around them grows by the projected
    radius at the nearer end -- per axis r |row - x row_2| / (w - r |row_2|), with the rows of inv(Q), w the nearer
    end's third component and x the projected end that makes it larger -- plus one pixel, and is clamped to the image.  A
    capsule that reaches within r of the plane through the source that the rays leave (or behind it) gets the whole image."""
    P = np.linalg.inv(grid.Q)
    n = float(np.linalg.norm(P[2]))
    pa, pb = P @ capsule.a, P @ capsule.b
    near = min(pa[2], pb[2]) - capsule.r * n
    if not near > 0:
        return 0, 0, grid.W - 1, grid.H - 1
    xa, xb = pa[:2] / pa[2], pb[:2] / pb[2]
    lo, hi = [], []
    for axis, size in ((0, grid.W), (1, grid.H)):
        reach = max(np.linalg.norm(P[axis] - xa[axis] * P[2]), np.linalg.norm(P[axis] - xb[axis] * P[2]))
        grow = capsule.r * reach / near + 1.0
        l, h = int(np.floor(min(xa[axis], xb[axis]) - grow)), int(np.ceil(max(xa[axis], xb[axis]) + grow))
        if h < 0 or l > size - 1:
            return 0, 0, -1, -1
        lo.append(max(l, 0))
        hi.append(min(h, size - 1))
    return lo[0], lo[1], hi[0], hi[1]


def pack(capsules_per_view, grid, cull=True):
    """The kernel's records, a numpy array [views, n] of TOOL_DTYPE rounded from float64; n = the most capsules any view
    has, shorter views padded with r = 0 records.  cull=False gives every capsule the whole image."""
    views = [list(v) for v in capsules_per_view]
    if not views:
        raise nat.DflError('tools.pack: no views')
    n = max(len(v) for v in views)
    if n > nat.TOOLS_MAX:
        raise nat.DflError('tools.pack: a view with %d capsules (at most %d are supported)' % (n, nat.TOOLS_MAX))
    out = np.zeros((len(views), n), TOOL_DTYPE)
    out['rect'] = (0, 0, -1, -1)
    for v, caps in enumerate(views):
        for j, cap in enumerate(caps):
            if not isinstance(cap, Capsule):
                raise nat.DflError('tools.pack: a tools.Capsule expected, got %s' % type(cap).__name__)
            out[v, j] = (cap.a, cap.b, cap.r, cap.mu, pixel_rect(cap, grid) if cull else (0, 0, grid.W - 1, grid.H - 1))
    return out


def tools_args(att, grid, recs, want_len=False):
    """(ToolsArgs, tool_len or None, tensors to keep alive) for packed records [views, n]: the upload, the freshly
    allocated output and the argument block of dfl_drr_tools, nothing launched."""
    if not torch.is_tensor(att) or not att.is_cuda:
        raise nat.DflError('tools.add_tools needs its tensor on the GPU (no CPU path)')
    if att.dim() != 3 or att.dtype != torch.float32 or not att.is_contiguous():
        raise nat.DflError('tools.add_tools: att must be a contiguous float32 [V, H, W], got %s %s' % (att.dtype, tuple(att.shape)))
    V, H, W = att.shape
    recs = np.asarray(recs)
    if recs.dtype != TOOL_DTYPE or recs.ndim != 2 or recs.shape[0] != V:
        raise nat.DflError('tools.add_tools: records [%d, n] of tools.TOOL_DTYPE expected (tools.pack), got shape %s' % (V, recs.shape))
    if (H, W) != (grid.H, grid.W):
        raise nat.DflError('tools.add_tools: att is %d x %d, the grid %d x %d' % (H, W, grid.H, grid.W))
    if recs.shape[1] > nat.TOOLS_MAX:
        raise nat.DflError('tools.add_tools: a view with %d capsules (at most %d are supported)' % (recs.shape[1], nat.TOOLS_MAX))
    dev, n = att.device, recs.shape[1]
    d_recs = torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(-1)).to(dev) if n else None
    tool_len = None
    if want_len:                                                             # no capsule anywhere: nothing is launched
        tool_len = (torch.empty if n else torch.zeros)((V, H, W), dtype=torch.float32, device=dev)
    a = nat.ToolsArgs(att=att.data_ptr(), tool_len=nat.ptr(tool_len), tools=nat.ptr(d_recs),
                      qscale=(nat.f32 * 9)(*grid.Q.astype(np.float32).reshape(-1)), views=V, H=H, W=W, n_tools=n)
    return a, tool_len, [att, d_recs]


def add_tools(att, grid, capsules_per_view, want_len=False, cull=True):
    """att [V, H, W] (float32, on the GPU, modified in place) += sum_j mu_j len_j of every view's capsules
    ([[Capsule]], one list per view, at most 64 each) on the rays of `grid`, in one launch.  Returns tool_len [V, H, W]
    (sum_j len_j in mm) with want_len, else None.  cull=False passes whole-image rectangles: the same bits, slower."""
    if not torch.is_tensor(att) or not att.is_cuda:
        raise nat.DflError('tools.add_tools needs its tensor on the GPU (no CPU path)')
    views = [list(v) for v in capsules_per_view]
    if att.dim() != 3 or len(views) != att.shape[0]:
        raise nat.DflError('tools.add_tools: %d lists of capsules for att of shape %s ([V, H, W] expected)' % (len(views), tuple(att.shape)))
    a, tool_len, keep = tools_args(att, grid, pack(views, grid, cull), want_len)
    with torch.cuda.device(att.device):
        nat.call('dfl_drr_tools', a, torch.cuda.current_stream(att.device).cuda_stream)
    del keep                                                      # stream order keeps the upload alive until the kernel ran
    return tool_len


def lands_in_camera(E, P_pelvis, lands3d):
    """float64 [L, 3]: 3D landmarks of the volume's physical frame in the camera projective frame under a pelvis pose:
    E inv(P_pelvis) X."""
    X = np.array([np.asarray(v, np.float64).reshape(-1)[:3] for v in (lands3d.values() if isinstance(lands3d, dict) else lands3d)])
    M = np.asarray(E, np.float64).reshape(4, 4) @ np.linalg.inv(np.asarray(P_pelvis, np.float64).reshape(4, 4))
    return (M[:3, :3] @ X.reshape(-1, 3).T).T + M[:3, 3]


def sample_tools(rng, lands_cam, max_tools, bead_prob=TOOL_DEFAULTS['bead_prob'], anchor_sigma_mm=TOOL_DEFAULTS['anchor_sigma_mm'],
                 length_mm=TOOL_DEFAULTS['length_mm'], wire_radius_mm=TOOL_DEFAULTS['wire_radius_mm'],
                 bead_radius_mm=TOOL_DEFAULTS['bead_radius_mm'], tool_mu=TOOL_DEFAULTS['tool_mu']):
    """[Capsule]: n tools around the landmarks lands_cam [L, 3] (camera projective frame), n uniform in 0..max_tools.

    Draws, in this order: n = rng.integers(0, max_tools + 1); then per tool rng.random(5) = (kind, landmark, length,
    where the anchor lies along the wire, radius) and rng.standard_normal(6) = (anchor offset [3], direction [3]),
    whatever the tool's kind -- a bead uses the first two uniforms and the first three normals only -- so the stream does
    not depend on the outcome.  A tool is a bead (radius bead_radius_mm) when kind < bead_prob, else a wire; its anchor is
    landmark floor(landmark L) plus anchor_sigma_mm times the offset; a wire's direction is the normalised direction
    draw, its length and radius uniform in length_mm and wire_radius_mm, and it runs from anchor - f length dir to
    anchor + (1 - f) length dir.  mu = tool_mu for every tool.  All of these are parameters, not measurements."""
    lands = np.asarray(lands_cam, np.float64).reshape(-1, 3)
    if lands.shape[0] < 1 or not np.isfinite(lands).all():
        raise nat.DflError('tools.sample_tools: at least one finite landmark is needed')
    max_tools = int(max_tools)
    if not 0 <= max_tools <= nat.TOOLS_MAX:
        raise nat.DflError('tools.sample_tools: max_tools must be 0..%d, got %d' % (nat.TOOLS_MAX, max_tools))
    (l0, l1), (r0, r1) = (float(x) for x in length_mm), (float(x) for x in wire_radius_mm)
    if not (0 <= float(bead_prob) <= 1 and float(anchor_sigma_mm) >= 0 and 0 < l0 <= l1 and 0 < r0 <= r1 and float(bead_radius_mm) > 0
            and float(tool_mu) >= 0 and np.isfinite([l1, r1, float(anchor_sigma_mm), float(bead_radius_mm), float(tool_mu)]).all()):
        raise nat.DflError('tools.sample_tools: bad parameters (bead_prob in 0..1, sigma >= 0, 0 < lo <= hi for lengths and radii, '
                           'bead radius > 0, mu >= 0)')
    n = int(rng.integers(0, max_tools + 1))
    out = []
    for _ in range(n):
        u, g = rng.random(UNIFORMS_PER_TOOL), rng.standard_normal(NORMALS_PER_TOOL)
        anchor = lands[min(int(u[1] * lands.shape[0]), lands.shape[0] - 1)] + float(anchor_sigma_mm) * g[0:3]
        if u[0] < float(bead_prob):
            out.append(Capsule(anchor, anchor, bead_radius_mm, tool_mu))
            continue
        norm = float(np.linalg.norm(g[3:6]))
        direction = g[3:6] / norm if norm > 0 else np.array([0.0, 0.0, 1.0])
        length = l0 + (l1 - l0) * u[2]
        out.append(Capsule(anchor - u[3] * length * direction, anchor + (1.0 - u[3]) * length * direction, r0 + (r1 - r0) * u[4], tool_mu))
    return out
