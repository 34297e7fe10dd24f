"""numpy float64 restatement of the preprocessing arithmetic, written with plain loops: crop, log,
rotate by 180 degrees where flagged, reduce by boxes that are clipped on the bottom and right edges.  A helper for
tests/test_preprocess_cpu.py and tests/test_gpu_preprocess.py, not a test."""
import numpy as np


def out_size(R, C, crop, f):
    return -(-(R - 2 * crop) // f), -(-(C - 2 * crop) // f)


def _window(img, rot, crop):
    """The crop window of one image, rotated by 180 degrees when rot."""
    R, C = img.shape
    w = img[crop:R - crop, crop:C - crop]
    return w[::-1, ::-1] if rot else w


def projs(pixels, rot180, crop, f, log=True, min_intensity=1.0):
    """[N, R, C] intensities -> [N, Ro, Co] float64 box means of log(I0) - log(max(I, min)), or of I."""
    pixels = np.asarray(pixels)
    N, R, C = pixels.shape
    Ro, Co = out_size(R, C, crop, f)
    out = np.zeros((N, Ro, Co), np.float64)
    for n in range(N):
        w = _window(pixels[n].astype(np.float64), rot180[n], crop)
        if log:
            w = np.maximum(w, float(min_intensity))
            w = np.log(w.max()) - np.log(w)
        for i in range(Ro):
            for j in range(Co):
                box = w[i * f:(i + 1) * f, j * f:(j + 1) * f]          # numpy clips the slice at the window's edge
                out[n, i, j] = box.sum() / box.size
    return out


def segs(labels, rot180, crop, f):
    """[N, R, C] uint8 labels -> [N, Ro, Co] uint8: the most frequent label of each box, ties to the smallest."""
    labels = np.asarray(labels)
    N, R, C = labels.shape
    Ro, Co = out_size(R, C, crop, f)
    out = np.zeros((N, Ro, Co), np.uint8)
    for n in range(N):
        w = _window(labels[n], rot180[n], crop)
        for i in range(Ro):
            for j in range(Co):
                counts = np.bincount(w[i * f:(i + 1) * f, j * f:(j + 1) * f].ravel(), minlength=16)
                out[n, i, j] = int(np.argmax(counts))                  # argmax returns the first of equal maxima
    return out


def restore(small, rot180, R, C, crop, f):
    """[N, Ro, Co] labels -> [N, R, C]: every pixel of the crop window takes its box's label, the border is 0."""
    small = np.asarray(small)
    N = small.shape[0]
    Rc, Cc = R - 2 * crop, C - 2 * crop
    out = np.zeros((N, R, C), np.uint8)
    for n in range(N):
        for r in range(Rc):
            for c in range(Cc):
                rr, cc = (Rc - 1 - r, Cc - 1 - c) if rot180[n] else (r, c)
                out[n, crop + r, crop + c] = small[n, rr // f, cc // f]
    return out


def restore_fast(small, rot180, R, C, crop, f):
    """restore() by repetition instead of loops, for images of the published size."""
    small = np.asarray(small)
    Rc, Cc = R - 2 * crop, C - 2 * crop
    out = np.zeros((small.shape[0], R, C), np.uint8)
    for n in range(small.shape[0]):
        w = np.repeat(np.repeat(small[n], f, 0), f, 1)[:Rc, :Cc]
        out[n, crop:R - crop, crop:C - crop] = w[::-1, ::-1] if rot180[n] else w
    return out


def map_lands(lands, rot180, R, C, crop, f):
    """[N, 2, L] (column, row) of pixel centres -> coordinates of the preprocessed image."""
    lands = np.asarray(lands, np.float64)
    out = np.zeros_like(lands)
    for n in range(lands.shape[0]):
        for l in range(lands.shape[2]):
            x, y = lands[n, 0, l] - crop, lands[n, 1, l] - crop
            if rot180[n]:
                x, y = (C - 2 * crop) - 1 - x, (R - 2 * crop) - 1 - y
            out[n, 0, l], out[n, 1, l] = (x + 0.5) / f - 0.5, (y + 0.5) / f - 0.5
    return out


def unmap_lands(lands, rot180, R, C, crop, f):
    lands = np.asarray(lands, np.float64)
    out = np.zeros_like(lands)
    for n in range(lands.shape[0]):
        for l in range(lands.shape[2]):
            x, y = (lands[n, 0, l] + 0.5) * f - 0.5, (lands[n, 1, l] + 0.5) * f - 0.5
            if rot180[n]:
                x, y = (C - 2 * crop) - 1 - x, (R - 2 * crop) - 1 - y
            out[n, 0, l], out[n, 1, l] = x + crop, y + crop
    return out
