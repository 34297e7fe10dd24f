"""Plain numpy restatement of the boundary distances (include/dfl_hip.h, "Boundary distances"), written from the definitions
and not from the kernels: sites of a label set, the squared distance transform by brute force over the sites, the two
directed multisets of surface distances and HD / HDp / ASSD.  Shared by test_surface_cpu.py (against scipy.ndimage and
numpy's own percentile) and test_gpu_surface.py (against the kernels).  The patterns are those of labels_ref.py.
"""
import numpy as np

NONE = 2147483647          # DFL_LABEL_EDT_NONE


def sites(seg, labels, boundary):
    """bool [H, W]: the pixels whose value is in `labels` (values >= 32 are never in a set); with `boundary` only those
    with a 4-neighbour not in the set, a neighbour outside the image counting as not in the set."""
    m = np.isin(seg, [l for l in labels if l < 32])
    if not boundary:
        return m
    pad = np.zeros((seg.shape[0] + 2, seg.shape[1] + 2), dtype=bool)
    pad[1:-1, 1:-1] = m
    inner = pad[:-2, 1:-1] & pad[2:, 1:-1] & pad[1:-1, :-2] & pad[1:-1, 2:]
    return m & ~inner


def dist2_to(site_mask):
    """int32 [H, W]: min over the sites q of drow^2 + dcol^2, NONE everywhere when there is no site.  Every pixel against
    every site, the sites taken one image row at a time: the minimum over all sites is the minimum over the rows q' of
    (the minimum over the sites of row q'), and drow^2 is the same for all of those.  No search structure, no early end."""
    H, W = site_mask.shape
    if not site_mask.any():
        return np.full((H, W), NONE, dtype=np.int32)
    out = np.full((H, W), np.iinfo(np.int64).max, dtype=np.int64)
    col = np.arange(W, dtype=np.int64)
    row = np.arange(H, dtype=np.int64)
    for q in range(H):
        cols = np.flatnonzero(site_mask[q])
        if cols.size:
            dcol2 = ((col[:, None] - cols[None, :]) ** 2).min(axis=1)           # [W]: against every site of row q
            np.minimum(out, ((row - q) ** 2)[:, None] + dcol2[None, :], out=out)
    assert out.max() < NONE
    return out.astype(np.int32)


_CACHE = {}


def edt(seg, labels, boundary):
    key = (seg.shape, seg.tobytes(), tuple(sorted(labels)), bool(boundary))
    if key not in _CACHE:
        _CACHE[key] = dist2_to(sites(seg, labels, boundary))
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


def edt_stack(segs, label_sets, boundary):
    """uint8 [B, H, W], S label sets -> int32 [B, S, H, W]"""
    return np.stack([np.stack([edt(seg, s, boundary) for s in label_sets]) for seg in segs])


def directed(est, gt, label):
    """The two multisets of SQUARED surface distances of `label` in one image, each sorted: direction 0 from the boundary
    of est to the boundary of gt, direction 1 the other way (NONE where the other boundary is empty)."""
    e, g = sites(est, (label,), True), sites(gt, (label,), True)
    return np.sort(edt(gt, (label,), True)[e]), np.sort(edt(est, (label,), True)[g])


def stats(est, gt, num_classes):
    """What dfl_label_surface_stats returns for one image: n int32 [C-1, 2], max2 int32 [C-1, 2], sum float64 [C-1, 2]."""
    n = np.zeros((num_classes - 1, 2), dtype=np.int32)
    max2 = np.zeros_like(n)
    total = np.zeros((num_classes - 1, 2), dtype=np.float64)
    for l in range(1, num_classes):
        d = directed(est, gt, l)
        n[l - 1] = [d[0].size, d[1].size]
        if d[0].size and d[1].size:
            max2[l - 1] = [d[0].max(), d[1].max()]
            total[l - 1] = [np.sqrt(d[0].astype(np.float64)).sum(), np.sqrt(d[1].astype(np.float64)).sum()]
    return n, max2, total


def kth2(est, gt, label, rank):
    """The squared distance of 0-based `rank` in the ascending union of both directions; -1 outside it."""
    u = np.sort(np.concatenate(directed(est, gt, label)))
    return int(u[rank]) if 0 <= rank < u.size else -1


def metrics(est, gt, num_classes, spacing=1.0, percentile=95.0):
    """One image -> dict of [C-1] arrays: hd, hdp, assd, mean_est_to_gt, mean_gt_to_est (float64), n_est, n_gt (int32), by
    the formulas of the header; both boundaries empty: 0.0, exactly one empty: inf."""
    keys = ('hd', 'hdp', 'assd', 'mean_est_to_gt', 'mean_gt_to_est')
    out = {k: np.zeros(num_classes - 1, dtype=np.float64) for k in keys}
    out['n_est'] = np.zeros(num_classes - 1, dtype=np.int32)
    out['n_gt'] = np.zeros(num_classes - 1, dtype=np.int32)
    for l in range(1, num_classes):
        d0, d1 = directed(est, gt, l)
        out['n_est'][l - 1], out['n_gt'][l - 1] = d0.size, d1.size
        if d0.size == 0 and d1.size == 0:
            continue
        if d0.size == 0 or d1.size == 0:
            for k in keys:
                out[k][l - 1] = np.inf
            continue
        r0, r1 = np.sqrt(d0.astype(np.float64)), np.sqrt(d1.astype(np.float64))
        u = np.sort(np.concatenate([d0, d1]))
        N = u.size
        pos = percentile / 100.0 * (N - 1)
        lo = int(np.floor(pos))
        hi = min(lo + 1, N - 1)
        k_lo, k_hi = np.sqrt(np.float64(u[lo])), np.sqrt(np.float64(u[hi]))
        out['hd'][l - 1] = np.sqrt(np.float64(max(d0.max(), d1.max()))) * spacing
        out['hdp'][l - 1] = (k_lo + (pos - lo) * (k_hi - k_lo)) * spacing
        out['mean_est_to_gt'][l - 1] = r0.sum() / d0.size * spacing
        out['mean_gt_to_est'][l - 1] = r1.sum() / d1.size * spacing
        out['assd'][l - 1] = (r0.sum() / d0.size + r1.sum() / d1.size) / 2.0 * spacing
    return out


def metrics_stack(est, gt, num_classes, spacing=1.0, percentile=95.0):
    per = [metrics(e, g, num_classes, spacing, percentile) for e, g in zip(est, gt)]
    return {k: np.stack([p[k] for p in per]) for k in per[0]}


def distances(est, gt, label):
    """The two directed arrays of distances (float64, sqrt of the squared ones) for numpy's max / percentile / mean."""
    d0, d1 = directed(est, gt, label)
    return np.sqrt(d0.astype(np.float64)), np.sqrt(d1.astype(np.float64))


def shifted_rectangles():
    """A filled 15 x 24 rectangle of label 1 in a 40 x 50 image and its copy shifted by (3, 4): HD 5.0, 74 boundary pixels
    each way, HD95 4.08001865665148, ASSD 3.1027798811266067."""
    est = np.zeros((40, 50), dtype=np.uint8)
    gt = np.zeros_like(est)
    gt[8:23, 10:34] = 1
    est[11:26, 14:38] = 1
    return est, gt
