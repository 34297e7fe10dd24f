"""Plain numpy restatement of the boundary loss (include/dfl_hip.h, "Boundary loss"), written from the definitions and not
from the kernels: labels by first-maximum arg-max, the signed distance maps on the brute-force distance transform of
surface_ref.py, the term in float64 and its gradient.  Shared by test_boundary_cpu.py (against scipy.ndimage and
torch.autograd) and test_gpu_boundary.py (against the kernels).
"""
import numpy as np

import surface_ref as SR


def labels_of(tseg):
    """[B, C, h, w] -> uint8 [B, h, w]: argmax over the channels, the first maximum winning (numpy's rule and torch.max's)."""
    return np.argmax(tseg, axis=1).astype(np.uint8)


def maps_of_labels(g, C):
    """uint8 [B, h, w] -> (phi float32 [B, C, h, w], d2 int64 [B, C, h, w]): d2 is the squared distance phi was taken from
    (0 where phi is 0 by the empty / whole-image rule).  The root in float64, one rounding to float32."""
    B, h, w = g.shape
    phi = np.zeros((B, C, h, w), dtype=np.float32)
    d2 = np.zeros((B, C, h, w), dtype=np.int64)
    for b in range(B):
        for c in range(C):
            inside = g[b] == c
            if not inside.any() or inside.all():
                continue
            to_in = SR.edt(g[b], (c,), False).astype(np.int64)
            to_out = SR.edt(g[b], tuple(l for l in range(C) if l != c), False).astype(np.int64)
            d2[b, c] = np.where(inside, to_out, to_in)
            root = np.sqrt(d2[b, c].astype(np.float64))
            phi[b, c] = np.where(inside, (1.0 - root).astype(np.float32), root.astype(np.float32))
    return phi, d2


def maps(tseg):
    return maps_of_labels(labels_of(tseg), tseg.shape[1])[0]


def one_hot(g, C, dtype=np.float32):
    return (g[:, None] == np.arange(C, dtype=g.dtype)[None, :, None, None]).astype(dtype)


def count(shape, skip_bg):
    B, C, h, w = shape
    return B * (C - (1 if skip_bg else 0)) * h * w


def term(seg, phi, skip_bg):
    """(L_B, sum of |seg * phi| / N, number of terms), all sums in float64 (the products of two floats are exact there)."""
    c0 = 1 if skip_bg else 0
    prod = seg[:, c0:].astype(np.float64) * phi[:, c0:].astype(np.float64)
    N = count(seg.shape, skip_bg)
    return prod.sum() / N, np.abs(prod).sum() / N, prod.size


def grad(phi, skip_bg, beta=1.0, grad_scale=1.0):
    """float64: grad_scale * beta * phi / N, zeros in a skipped background channel."""
    out = grad_scale * beta * phi.astype(np.float64) / count(phi.shape, skip_bg)
    if skip_bg:
        out[:, 0] = 0.0
    return out


def random_labels(B, C, h, w, seed):
    """Blocky random label maps: a coarse random grid of labels, enlarged, then a sprinkle of single pixels."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, C, size=(B, (h + 3) // 4, (w + 4) // 5))
    g = np.repeat(np.repeat(coarse, 4, axis=1), 5, axis=2)[:, :h, :w]
    speck = rng.random(g.shape) < 0.03
    g[speck] = rng.integers(0, C, size=int(speck.sum()))
    return np.ascontiguousarray(g.astype(np.uint8))
