"""Plain numpy / Python restatement of the label clean-up (include/dfl_hip.h, "Clean-up of predicted label maps"), written
from the definitions and not from the kernels: breadth-first flood fill for root / area / info, the remove and fill rules,
the disc dilation -- and the builders of the test patterns (fixed seeds).  Shared by test_labels_cpu.py (against
scipy.ndimage) and test_gpu_labels.py (against the kernels, bit for bit).
"""
import functools
from collections import deque

import numpy as np

NUM_CLASSES = 7


# ------------------------------------------------------------------------------------------------------ the restatement
def components(seg, connectivity):
    """seg uint8 [H, W] -> (root int32, area int32, info uint32), each [H, W].  root[p] = smallest flat index (row * W + col)
    of the pixels connected to p through pixels of the same value; area / info at the root pixel only: pixel count; bit 31 =
    touches the image border, bits 0..30 = union of 1 << min(v, 30) over the values v of the 4-neighbours of the component's
    pixels that lie outside the component."""
    assert connectivity in (4, 8)
    H, W = seg.shape
    Wp = W + 2                                                # a frame of -1 around the image: no bounds tests below
    pad = np.full((H + 2, Wp), -1, dtype=np.int64)
    pad[1:-1, 1:-1] = seg
    val = pad.ravel().tolist()
    four = (-Wp, Wp, -1, 1)
    steps = four if connectivity == 4 else four + (-Wp - 1, -Wp + 1, Wp - 1, Wp + 1)
    comp = [-1] * len(val)                                    # padded index -> flat index of the root
    root = np.zeros((H, W), dtype=np.int32)
    area = np.zeros((H, W), dtype=np.int32)
    info = np.zeros((H, W), dtype=np.uint32)
    for r in range(H):
        for c in range(W):
            start = (r + 1) * Wp + c + 1
            if comp[start] >= 0:
                continue
            me, v = r * W + c, val[start]                     # row-major scan: the first pixel met is the smallest index
            comp[start] = me
            members, queue = [start], deque([start])
            while queue:
                p = queue.popleft()
                for s in steps:
                    q = p + s
                    if val[q] == v and comp[q] < 0:
                        comp[q] = me
                        members.append(q)
                        queue.append(q)
            bits = 0
            for p in members:
                for s in four:
                    q = p + s
                    if val[q] < 0:
                        bits |= 1 << 31                       # a neighbour outside the image: p is on the border
                    elif comp[q] != me:
                        bits |= 1 << min(val[q], 30)
            area[r, c] = len(members)
            info[r, c] = bits
            for p in members:
                root[p // Wp - 1, p % Wp - 1] = me
    return root, area, info


def remove(seg, comp, num_classes, keep, min_area):
    """-> (out, removed [C]): of the labels 1..C-1 a component stays when area >= min_area and, with keep == 'largest', when it
    is the largest of its label in the image (ties: smallest root); the others become 0."""
    root, area, _ = comp
    out = seg.copy()
    removed = np.zeros(num_classes, dtype=np.int32)
    flat_root, flat_area, flat_seg = root.ravel(), area.ravel(), seg.ravel()
    roots = np.flatnonzero(flat_area > 0)
    for l in range(1, num_classes):
        mine = [int(p) for p in roots if flat_seg[p] == l]
        if not mine:
            continue
        best = min(mine, key=lambda p: (-int(flat_area[p]), p))
        for p in mine:
            if flat_area[p] >= min_area and (keep == 'all' or p == best):
                continue
            out[root == p] = 0
            removed[l] += int(flat_area[p])
    return out, removed


def fill(seg, comp, num_classes, fill_below):
    """-> (out, filled [C]): a component of value 0 that does not touch the border, has area <= fill_below and whose
    neighbours are all of one label l with 1 <= l < min(C, 30) becomes l."""
    root, area, _ = comp
    H, W = seg.shape
    out = seg.copy()
    filled = np.zeros(num_classes, dtype=np.int32)
    for p in np.flatnonzero((area.ravel() > 0) & (seg.ravel() == 0)):
        inside = root == p
        rows, cols = np.nonzero(inside)
        if rows.min() == 0 or cols.min() == 0 or rows.max() == H - 1 or cols.max() == W - 1 or rows.size > fill_below:
            continue
        around = set()
        for dr, dc in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            rr, cc = rows + dr, cols + dc
            around.update(int(v) for v, i in zip(seg[rr, cc], inside[rr, cc]) if not i)
        if len(around) == 1:
            l = around.pop()
            if 1 <= l < min(num_classes, 30):
                out[inside] = l
                filled[l] += rows.size
    return out, filled


def clean(segs, num_classes=NUM_CLASSES, connectivity=8, keep='largest', min_area=0, fill_holes=0):
    """segs uint8 [B, H, W] -> (cleaned, {'removed': int32 [B, C], 'filled': int32 [B, C]}): labels.clean."""
    out = np.empty_like(segs)
    removed = np.zeros((segs.shape[0], num_classes), dtype=np.int32)
    filled = np.zeros_like(removed)
    for b in range(segs.shape[0]):
        out[b], removed[b] = remove(segs[b], _components_cached(segs[b], connectivity), num_classes, keep, min_area)
        if fill_holes > 0:
            out[b], filled[b] = fill(out[b], _components_cached(out[b], 4), num_classes, fill_holes)
    return out, {'removed': removed, 'filled': filled}


_CACHE = {}


def _components_cached(seg, connectivity):
    key = (seg.shape, connectivity, seg.tobytes())
    if key not in _CACHE:
        _CACHE[key] = components(seg, connectivity)
    return _CACHE[key]


def components_stack(segs, connectivity):
    out = [_components_cached(s, connectivity) for s in segs]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def dilate(seg, labels, radius):
    """uint8 [H, W]: 1 where a pixel of the image within Euclidean distance `radius` has a value in `labels`."""
    H, W = seg.shape
    hit = np.isin(seg, list(labels))
    out = np.zeros((H, W), dtype=bool)
    for dr in range(-radius, radius + 1):
        for dc in range(-radius, radius + 1):
            if dr * dr + dc * dc > radius * radius:
                continue
            # out[r, c] |= hit[r + dr, c + dc] where that pixel exists
            r_lo, r_hi = max(0, -dr), min(H, H - dr)
            c_lo, c_hi = max(0, -dc), min(W, W - dc)
            if r_lo < r_hi and c_lo < c_hi:
                out[r_lo:r_hi, c_lo:c_hi] |= hit[r_lo + dr:r_hi + dr, c_lo + dc:c_hi + dc]
    return out.astype(np.uint8)


# ------------------------------------------------------------------------------------------------------ the patterns
def _put(img, r, c, v):
    """Draw with clipping: the small shapes keep what fits."""
    if 0 <= r < img.shape[0] and 0 <= c < img.shape[1]:
        img[r, c] = v


def spiral(H, W, tile):
    """A one-pixel-wide spiral of label 1 from the corner inwards, one pixel of background between its turns."""
    img = np.zeros((H, W), dtype=np.uint8)

    def free(r, c):
        return 0 <= r < H and 0 <= c < W and img[r, c] == 0
    r, c, dr, dc = 0, 0, 0, 1
    img[0, 0] = 1
    turns = 0
    while turns < 2:
        nr, nc = r + dr, c + dc
        ahead = (nr + dr, nc + dc)
        if free(nr, nc) and (free(*ahead) or not (0 <= ahead[0] < H and 0 <= ahead[1] < W)):
            r, c, turns = nr, nc, 0
            img[r, c] = 1
        else:
            dr, dc, turns = dc, -dr, turns + 1
    return img


def serpentine(H, W, tile):
    """Every other row full of label 2, joined alternately at the right and the left end: one path half the image long."""
    img = np.zeros((H, W), dtype=np.uint8)
    img[0::2, :] = 2
    for k, r in enumerate(range(1, H, 2)):
        if r + 1 < H:
            img[r, W - 1 if k % 2 == 0 else 0] = 2
    return img


def checkerboard(H, W, tile):
    r, c = np.mgrid[0:H, 0:W]
    return (1 + (r + c) % 2).astype(np.uint8)


def comb(H, W, tile):
    """Teeth in every other column that join only along the last row."""
    img = np.zeros((H, W), dtype=np.uint8)
    img[:, 0::2] = 3
    img[H - 1, :] = 3
    return img


def two_u(H, W, tile):
    """Two U shapes of label 4 whose arms lie in the first tile and whose bends lie across a tile border: one bends below
    the first tile row, one right of the first tile column.  Each has a tail, and the tails' ends touch only diagonally
    across the far corner of the first tile: (th, tw - 1) and (th - 1, tw)."""
    th, tw = tile
    img = np.zeros((H, W), dtype=np.uint8)
    for r in range(1, th + 1):                 # arms down columns 1 and 3, bend in row th (the tile below)
        _put(img, r, 1, 4)
        _put(img, r, 3, 4)
    for c in range(1, tw):                     # ... and the tail along row th up to the corner
        _put(img, th, c, 4)
    for c in range(5, tw + 1):                 # arms along rows 1 and 3, bend in column tw (the tile to the right)
        _put(img, 1, c, 4)
        _put(img, 3, c, 4)
    for r in range(1, th):                     # ... and the tail down column tw up to the corner
        _put(img, r, tw, 4)
    return img


def _random(H, W, density, seed):
    rng = np.random.default_rng(seed)
    lab = rng.integers(1, NUM_CLASSES, size=(H, W))
    return np.where(rng.random((H, W)) < density, lab, 0).astype(np.uint8)


def random_sparse(H, W, tile):
    return _random(H, W, 0.35, 11)


def random_dense(H, W, tile):
    return _random(H, W, 0.85, 12)


def all_zero(H, W, tile):
    return np.zeros((H, W), dtype=np.uint8)


def all_one_label(H, W, tile):
    return np.full((H, W), 5, dtype=np.uint8)


def tie(H, W, tile):
    """Two components of label 1 with the same area (and a smaller third): the first in row-major order is kept."""
    img = np.zeros((H, W), dtype=np.uint8)
    for r0, c0 in ((1, 6), (4, 1)):
        for dr in range(2):
            for dc in range(3):
                _put(img, r0 + dr, c0 + dc, 1)
    _put(img, 8, 8, 1)
    return img


def diagonal_ring(H, W, tile):
    """Diamond rings of label 2 closed only diagonally: one around a hole of 1 pixel, one around a hole of 5 pixels."""
    img = np.zeros((H, W), dtype=np.uint8)
    for r0, c0, rad in ((2, 2, 1), (4, 7, 2)):
        for dr in range(-rad, rad + 1):
            _put(img, r0 + dr, c0 + rad - abs(dr), 2)
            _put(img, r0 + dr, c0 - rad + abs(dr), 2)
    return img


def hole_two_labels(H, W, tile):
    """A one-pixel hole whose ring is half label 1, half label 2: not filled."""
    img = np.zeros((H, W), dtype=np.uint8)
    for dr in range(3):
        for dc in range(3):
            if (dr, dc) != (1, 1):
                _put(img, 1 + dr, 1 + dc, 1 if dc < 2 else 2)
    return img


def hole_at_border(H, W, tile):
    """A pocket of background that label 3 closes against the image border: not filled."""
    img = np.zeros((H, W), dtype=np.uint8)
    for c in range(1, 4):
        _put(img, 1, c, 3)
    _put(img, 0, 1, 3)
    _put(img, 0, 3, 3)
    for r in range(3, 6):                      # and a closed ring of label 3 further in: filled
        for c in range(3, 6):
            if (r, c) != (4, 4):
                _put(img, r, c, 3)
    return img


def beyond_classes(H, W, tile):
    """Value 9 >= num_classes: copied through by remove (islands included), and a hole in it is not filled."""
    img = np.zeros((H, W), dtype=np.uint8)
    for r in range(1, 4):
        for c in range(1, 4):
            if (r, c) != (2, 2):
                _put(img, r, c, 9)
    _put(img, 6, 6, 9)
    _put(img, 6, 1, 1)
    _put(img, 8, 3, 1)
    _put(img, 8, 4, 1)
    return img


def blobs(B, H, W, seed=5):
    """[B, H, W] of 7 labels in large blobs: the arg-max of seven box-smoothed random fields, speckled with a few stray
    pixels and pin-holes as a network's output is."""
    rng = np.random.default_rng(seed)
    f = rng.random((B, NUM_CLASSES, H, W))
    for _ in range(6):
        f = (f + np.roll(f, 1, 2) + np.roll(f, -1, 2) + np.roll(f, 1, 3) + np.roll(f, -1, 3)) / 5.0
    f[:, 0] += 0.01                                           # some more background
    seg = f.argmax(1).astype(np.uint8)
    noise = rng.random((B, H, W))
    seg[noise < 0.01] = rng.integers(0, NUM_CLASSES, size=int((noise < 0.01).sum()))
    return seg


PATTERNS = {f.__name__: f for f in (spiral, serpentine, checkerboard, comb, two_u, random_sparse, random_dense, all_zero,
                                    all_one_label, tie, diagonal_ring, hole_two_labels, hole_at_border, beyond_classes)}


def shapes(tile):
    th, tw = tile
    return [(1, 1), (1, 2 * tw + 5), (2 * th + 3, 1), (th - 1, tw + 1), (3 * th + 7, 3 * tw + 5)]


@functools.lru_cache(maxsize=None)
def pattern(name, H, W, tile):
    img = PATTERNS[name](H, W, tile)
    assert img.shape == (H, W) and img.dtype == np.uint8
    img.setflags(write=False)
    return img
