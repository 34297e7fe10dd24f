"""The three weight layouts of dfl_pack_job, restated in numpy from their descriptions in include/dfl_hip.h (not from the kernels
of csrc/bn_elem.hip): what tests/test_gpu_pack.py and tests/test_gpu_finalize.py compare the device's bytes with.

A parameter is a contiguous src[A][B][C] (C = KH*KW).  A job reads it as the matrix W[K][N] of one of three index maps
  kind 1: k = c*B + b,  n = a
  kind 2: k = c'*A + a, n = b,  c = C-1-c' with flip, else c = c'
  kind 3: k = a,        n = c*B + b
and stores W, rows k >= K zero, in one of three formats
  fp32 quads   [ceil(K/4)][N][4]    w[(k/4)*N*4 + n*4 + k%4] = W(k, n)
  split quads  the same 16-byte slots, each holding the 4 hi bf16 of its values, then their 4 lo bf16:
               hi = bf16(v), lo = bf16(v - float(hi)), both rounded to nearest even
  bf16 chunks  [ceil(K/16)][N][16]  w[(k/16)*N*16 + n*16 + k%16] = bf16(W(k, n))
Every encoder returns the destination's raw bytes (a uint8 array).  numpy only; torch on the CPU rounds to bf16."""
import numpy as np
import torch


def dims(kind, A, B, C):
    """(K, N) of the matrix a job of this kind builds from src[A][B][C]."""
    return {1: (C * B, A), 2: (C * A, B), 3: (A, C * B)}[kind]


def matrix(w, kind, flip=0):
    """W[K][N] of parameter w = [A][B][C] (or [A][B][KH][KW]), in w's dtype."""
    w = np.asarray(w)
    A, B = w.shape[:2]
    w = w.reshape(A, B, -1)
    C = w.shape[2]
    K, N = dims(kind, A, B, C)
    a, b, c = np.indices((A, B, C))
    if kind == 1:
        k, n = c * B + b, a
    elif kind == 2:
        k, n = (C - 1 - c if flip else c) * A + a, b        # c' of element c: the flip is its own inverse
    else:
        k, n = a, c * B + b
    W = np.zeros((K, N), dtype=w.dtype)
    W[k, n] = w
    return W


def _slots(W, rows):
    """[ceil(K/rows)][N][rows] of W[K][N] as fp32, the rows behind K zero."""
    K, N = W.shape
    Kr = -(-K // rows)
    full = np.zeros((Kr * rows, N), dtype=np.float32)
    full[:K] = W
    return np.ascontiguousarray(full.reshape(Kr, rows, N).transpose(0, 2, 1))


def _bf16(v):
    """(bit patterns as uint16, values as fp32) of fp32 v rounded to bf16, nearest even."""
    r = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(torch.bfloat16)
    return r.view(torch.int16).numpy().view(np.uint16), r.float().numpy()


def quads(W):
    return _slots(W, 4).view(np.uint8).reshape(-1)


def split_quads(W):
    v = _slots(W, 4)
    hi, hif = _bf16(v)
    lo, _ = _bf16(v - hif)
    return np.ascontiguousarray(np.concatenate([hi, lo], axis=2)).view(np.uint8).reshape(-1)


def chunks(W):
    return np.ascontiguousarray(_bf16(_slots(W, 16))[0]).view(np.uint8).reshape(-1)


def encode(w, kind, flip, split):
    """The bytes a job (kind, flip, split) leaves in its destination."""
    return (quads, split_quads, chunks)[split](matrix(w, kind, flip))


def nbytes(kind, A, B, C, split):
    K, N = dims(kind, A, B, C)
    return -(-K // 16) * N * 32 if split == 2 else -(-K // 4) * N * 16
