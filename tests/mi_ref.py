"""The numpy restatement of the mutual-information cost (include/dfl_hip.h, "Mutual information"):
what the GPU tests hold csrc/sim_mi.hip to, bit for bit where integers are concerned.

Every float32 step is rounded on its own, as the kernel's are (csrc/build.sh compiles sim_mi.hip with -ffp-contract=off);
the joint histogram is int64 in units of 1 / UNIT pixel; the cost and the table of the adjoint are float64.  unit=None is
the unquantised variant: the same float32 fraction, used as an exact float64 weight.  cost64 is the whole cost in float64
from float64 pixels, for central differences (tests/mi_floor.py).
"""
import numpy as np

UNIT, MAX_BINS, SKIP = 4096, 64, 255
F32 = np.float32


def counted(fixed, mask=None):
    """bool [H, W]: the fixed value is finite and the mask byte (if any) non-zero."""
    on = np.isfinite(np.asarray(fixed, F32))
    return on if mask is None else on & (np.asarray(mask) != 0)


def prepare(fixed, mask, Bf):
    """(fbin uint8 [H, W], info float64 [4] = n, lo_f, hi_f, 0): dfl_sim_mi_prepare."""
    f = np.asarray(fixed, F32)
    on = counted(f, mask)
    n = int(on.sum())
    fbin = np.full(f.shape, SKIP, np.uint8)
    if n == 0:
        return fbin, np.zeros(4)
    lo, hi = f[on].min(), f[on].max()
    with np.errstate(all='ignore'):
        d = F32(hi - lo)
        x = ((f - lo).astype(F32) * (F32(Bf) / d)).astype(F32)
        k = np.where(x >= F32(Bf), Bf - 1, np.where(x > 0, np.floor(x), 0))      # NaN (0 x inf) is bin 0
    k = k.astype(np.int64) if d > 0 else np.zeros(f.shape, np.int64)
    fbin[on] = k[on]
    return fbin, np.array([n, float(lo), float(hi), 0.0])


def scale(lo, hi, Bm):
    """(s float32, void): s = float32(Bm - 1) / (hi - lo); void unless lo, hi, hi - lo and s are finite and hi > lo."""
    lo, hi = F32(lo), F32(hi)
    with np.errstate(all='ignore'):
        d = F32(hi - lo)
        s = F32(Bm - 1) / d
    ok = np.isfinite(lo) and np.isfinite(hi) and hi > lo and np.isfinite(d) and np.isfinite(s)
    return s, not ok


def weights(m, lo, hi, Bm):
    """(a int64 [H, W], fraction float32 [H, W], q int64 [H, W]) of moving values for a range that is not void."""
    lo, hi = F32(lo), F32(hi)
    s, _ = scale(lo, hi, Bm)
    c = np.fmin(np.fmax(np.asarray(m, F32), lo), hi)                  # NaN counts as lo
    x = ((c - lo).astype(F32) * s).astype(F32)
    a = np.where(x >= F32(Bm - 1), Bm - 2, np.floor(x)).astype(np.int64)
    fr = (x - a.astype(F32)).astype(F32)
    q = np.floor((fr * F32(UNIT)).astype(F32) + F32(0.5)).astype(np.int64)
    return a, fr, q


def hist(m, fbin, lo, hi, Bf, Bm, unit=UNIT):
    """The joint histogram [Bm, Bf] of one view: int64 in units of 1 / unit, or float64 with unit=None; zeros when void."""
    h = np.zeros((Bm, Bf), np.int64 if unit else np.float64)
    if scale(lo, hi, Bm)[1]:
        return h
    on = np.asarray(fbin) != SKIP
    a, fr, q = weights(m, lo, hi, Bm)
    w1 = q if unit else fr.astype(np.float64)
    w0 = (unit - q) if unit else 1.0 - w1
    b = np.asarray(fbin).astype(np.int64)
    np.add.at(h, (a[on], b[on]), w0[on])
    np.add.at(h, (a[on] + 1, b[on]), w1[on])
    return h


def mi(h):
    """sum over h > 0 of (h / N) log(h N / (h_a h_b)), float64; 0 for an empty histogram."""
    hf = np.asarray(h).astype(np.float64)
    N = float(np.asarray(h).sum())
    if N == 0:
        return 0.0
    ha = np.asarray(h).sum(1).astype(np.float64)[:, None]
    hb = np.asarray(h).sum(0).astype(np.float64)[None]
    nz = hf > 0
    return float(((hf / N) * np.log(np.where(nz, (hf * N) / np.where(nz, ha * hb, 1.0), 1.0)))[nz].sum())


def cost(moving, fbin, mrange, Bf, Bm, unit=UNIT):
    """[V] float64 (or a float for [H, W]): -MI of every view against one prepared image; NaN for a void range."""
    moving = np.asarray(moving)
    mv = moving[None] if moving.ndim == 2 else moving
    lo, hi = mrange
    if scale(lo, hi, Bm)[1]:
        out = np.full(mv.shape[0], np.nan)
    else:
        out = np.array([-mi(hist(v, fbin, lo, hi, Bf, Bm, unit)) for v in mv])
    return out[0] if moving.ndim == 2 else out


def table(h, unit=UNIT):
    """ell[a][b] = log(max(h, 1)) - log(max(h_a, 1)), float64 (unit=None: the floor is 1e-300, not 1)."""
    one = 1 if unit else 1e-300
    return np.log(np.maximum(h, one).astype(np.float64)) - np.log(np.maximum(np.asarray(h).sum(1, keepdims=True), one).astype(np.float64))


def adjoint(m, fbin, lo, hi, Bf, Bm, unit=UNIT, row_term=1.0):
    """float64 [H, W]: -(s / n) (ell[a + 1][b] - ell[a][b]) at a counted pixel with lo < m < hi, else exactly 0; what
    dfl_sim_mi_bwd rounds to float32.  row_term scales the -log h_a term: the tests show that 0 and -1 are caught."""
    m = np.asarray(m, F32)
    out = np.zeros(m.shape)
    s, void = scale(lo, hi, Bm)
    on = np.asarray(fbin) != SKIP
    n = int(on.sum())
    if void or n == 0:
        return out
    h = hist(m, fbin, lo, hi, Bf, Bm, unit)
    one = 1 if unit else 1e-300
    ell = np.log(np.maximum(h, one).astype(np.float64)) - row_term * np.log(np.maximum(h.sum(1, keepdims=True), one).astype(np.float64))
    a, _, _ = weights(m, lo, hi, Bm)
    b = np.where(on, np.asarray(fbin), 0).astype(np.int64)
    g = -(float(s) / n) * (ell[a + 1, b] - ell[a, b])
    inside = on & (m > F32(lo)) & (m < F32(hi))
    out[inside] = g[inside]
    return out


def cost64(m, fbin, lo, hi, Bf, Bm):
    """The unquantised cost of float64 pixels in float64 throughout: what central differences are taken of."""
    on = np.asarray(fbin) != SKIP
    s = (Bm - 1) / (float(hi) - float(lo))
    x = (np.clip(np.asarray(m, np.float64), float(lo), float(hi)) - float(lo)) * s
    a = np.minimum(np.floor(x), Bm - 2).astype(np.int64)
    fr = x - a
    b = np.asarray(fbin).astype(np.int64)
    h = np.zeros((Bm, Bf))
    np.add.at(h, (a[on], b[on]), 1.0 - fr[on])
    np.add.at(h, (a[on] + 1, b[on]), fr[on])
    return -mi(h)


def start_range(view):
    """The default range of register(similarity='mi'): (0, 1.25 max of the start view), float32."""
    return F32(0), F32(F32(1.25) * np.asarray(view, F32).max())
