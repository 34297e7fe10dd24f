"""Plain numpy float64 restatement of the outline cost (include/dfl_hip.h, "Outline cost"), written
from the definitions on surface_ref.sites and surface_ref.dist2_to: the truncated chamfer distance between the boundaries
of label sets in a moving and a fixed label map.  Shared by test_outline_cpu.py, test_gpu_outline.py (against
dfl_sim_outline) and outline_floor.py (the registrations the model alone solves).

A label set is a tuple of labels here (values >= 32 are never in a set) and a 32-bit word in the C API; `labels_of`
turns a word into the tuple.
"""
import numpy as np

import surface_ref as SR

NONE = SR.NONE


def labels_of(word):
    return tuple(l for l in range(32) if (int(word) >> l) & 1)


def d2_stack(seg, label_sets):
    """uint8 [H, W], S label sets -> int32 [S, H, W]: the squared distance to the boundary sites of every set."""
    return np.stack([SR.dist2_to(SR.sites(seg, s, True)) for s in label_sets])


def truncated(d2, cap):
    return np.minimum(np.sqrt(d2.astype(np.float64)), np.float64(cap))


def from_d2(d2m, d2f, cap):
    """int32 [S, H, W] of the moving and of the fixed map -> (counts int32 [S, 2] = nM, nF; sums float64 [S, 2] = a, b;
    cost).  A pixel is a boundary site of a map exactly where that map's own distance is 0."""
    S = d2m.shape[0]
    counts = np.zeros((S, 2), np.int32)
    sums = np.zeros((S, 2), np.float64)
    c = []
    for k in range(S):
        M, F = d2m[k] == 0, d2f[k] == 0
        nM, nF = int(M.sum()), int(F.sum())
        counts[k] = nM, nF
        if nM > 0 and nF > 0:
            a, b = truncated(d2f[k][M], cap).sum(), truncated(d2m[k][F], cap).sum()
            sums[k] = a, b
            c.append((a / nM + b / nF) / (2.0 * np.float64(cap)))
        elif nM > 0 or nF > 0:
            c.append(1.0)
    return counts, sums, (float(np.mean(c)) if c else 1.0)


def cost(m, f, label_sets, cap):
    """One moving map m and one fixed map f, uint8 [H, W] -> (counts, sums, cost) by the definitions."""
    return from_d2(d2_stack(m, label_sets), d2_stack(f, label_sets), cap)


def cost_stack(ms, fs, label_sets, cap, fixed_of=None):
    """ms [V, H, W] against fs [F, H, W] (view v against fs[fixed_of[v]], or fs[0]) -> counts [V, S, 2], sums [V, S, 2],
    cost [V]."""
    fd = [d2_stack(f, label_sets) for f in fs]
    out = [from_d2(d2_stack(m, label_sets), fd[0 if fixed_of is None else int(fixed_of[v])], cap) for v, m in enumerate(ms)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out])


# ---- one cost evaluation of the registration, by the model ----------------------------------------------------------------
DEFAULT_SETS = ((1,), (2,), (3,), (4,), (5,), (6,))         # one set per label of the three objects' masks


def render_labels(S, poses):
    """The winner-takes-all label map [H, W] uint8 of the tilted scene under three cam-to-*-vol poses: the exact model
    with tight boxes (drr_ref.render, drr_ref.label_map)."""
    import drr_ref as D
    recs = D.pack([D.c2i(S['I2P'], P, S['E']) for P in poses], D.MASKS, S['Q'], S['lab'], True, 'exact')
    plen = D.render(S['mu'], S['lab'], recs, S['Q'].astype(np.float32), S['rows'], S['cols'], 'exact')[1]
    return D.label_map(plen)


def model_cost_fn(S, start_poses, moving, fixed_seg, pose_deltas, cap, label_sets=DEFAULT_SETS):
    """cost_fn([n, 6]) -> [n] for dfl_amd.register.cma_es: reg_ref.model_cost_fn with the outline cost against the label
    map `fixed_seg`."""
    import reg_ref as R
    ctr = R.volume_centre(S)
    d2f = d2_stack(fixed_seg, label_sets)

    def fn(thetas):
        out = []
        for Dm in pose_deltas(thetas, ctr):
            poses = [Dm @ P if n in moving else P for n, P in enumerate(start_poses)]
            out.append(from_d2(d2_stack(render_labels(S, poses), label_sets), d2f, cap)[2])
        return np.array(out)

    return fn
