"""tests/pack_ref.py means what include/dfl_hip.h says: its index maps give the convolutions they are named for (fp64, one small
case each), and its three formats decode back to the matrix.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pack_ref as PK

F64 = torch.float64
N_IMG, H, W_, CI, CO = 2, 6, 5, 3, 4


def rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


def rows(t):
    """NCHW -> [pixels][channels], the GEMM's row per pixel."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).numpy()


def im2col(x, KH, KW, stride, pad):
    """[N*Ho*Wo][(tap, channel)] of an NCHW tensor: column k = (ky*KW + kx) * C + c."""
    x = F.pad(x, (pad, pad, pad, pad))
    Ho, Wo = (x.shape[2] - KH) // stride + 1, (x.shape[3] - KW) // stride + 1
    cols = [rows(x[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]) for ky in range(KH) for kx in range(KW)]
    return np.concatenate(cols, axis=1)


def scatter2x2(y, n, h, w):
    """[pixels][(ab, channel)] -> NCHW at twice the size: pixel (i, j), tap ab = 2a + b lands at (2i + a, 2j + b)."""
    Cc = y.shape[1] // 4
    t = torch.from_numpy(y).reshape(n, h, w, 2, 2, Cc)
    return t.permute(0, 5, 1, 3, 2, 4).reshape(n, Cc, 2 * h, 2 * w)


def same(got, ref):
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12)       # fp64 sums of at most 36 products of N(0, 1) values


def test_kind1_is_the_forward_operand_of_conv2d():
    x, w = rand(N_IMG, CI, H, W_, seed=1), rand(CO, CI, 3, 3, seed=2)
    same(im2col(x, 3, 3, 1, 1) @ PK.matrix(w.numpy(), 1), rows(F.conv2d(x, w, padding=1)))


def test_kind2_flipped_is_the_data_gradient_of_a_stride1_conv2d():
    dy, w = rand(N_IMG, CO, H, W_, seed=3), rand(CO, CI, 3, 3, seed=4)
    same(im2col(dy, 3, 3, 1, 1) @ PK.matrix(w.numpy(), 2, flip=1), rows(F.conv_transpose2d(dy, w, padding=1)))


def test_kind2_unflipped_correlates_with_the_transposed_weight():
    dy, w = rand(N_IMG, CO, H, W_, seed=5), rand(CO, CI, 3, 3, seed=6)
    same(im2col(dy, 3, 3, 1, 1) @ PK.matrix(w.numpy(), 2, flip=0), rows(F.conv2d(dy, w.transpose(0, 1), padding=1)))


def test_kind3_is_conv_transpose2d_k2_s2_in_scatter_form():
    x, w = rand(N_IMG, CI, H, W_, seed=7), rand(CI, CO, 2, 2, seed=8)
    y = scatter2x2(rows(x) @ PK.matrix(w.numpy(), 3), N_IMG, H, W_)
    same(y.numpy(), F.conv_transpose2d(x, w, stride=2).numpy())


def test_kind3_is_the_data_gradient_of_conv2d_k2_s2_in_scatter_form():
    dy, w = rand(N_IMG, CO, H, W_, seed=9), rand(CO, CI, 2, 2, seed=10)        # UNetPlan._pack_down_dgrad
    dx = scatter2x2(rows(dy) @ PK.matrix(w.numpy(), 3), N_IMG, H, W_)
    same(dx.numpy(), F.conv_transpose2d(dy, w, stride=2).numpy())


def test_kind1_is_the_data_gradient_of_conv_transpose2d_k2_s2():
    dy, w = rand(N_IMG, CO, 2 * H, 2 * W_, seed=11), rand(CI, CO, 2, 2, seed=12)   # UNetPlan._pack_convT_dgrad
    same(im2col(dy, 2, 2, 2, 0) @ PK.matrix(w.numpy(), 1), rows(F.conv2d(dy, w, stride=2)))


# ---------------------------------------------------------------------------------------------------- formats
# K = 27 / 63 / 7: no multiple of 4 or of 16, so every format has zero rows to show
FORMAT_CASES = [(7, 3, 9, 1, 0), (7, 3, 9, 2, 1), (7, 3, 9, 2, 0), (7, 3, 9, 3, 0), (16, 32, 4, 1, 0)]


def bf16_values(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32)


def decode(raw, K, N, split):
    """W[K][N] (and the rows behind K) from a destination's bytes, read by the address formulas of the header."""
    k, n = np.indices((-(-K // (16 if split == 2 else 4)) * (16 if split == 2 else 4), N))
    if split == 0:
        return raw.view(np.float32)[(k // 4) * N * 4 + n * 4 + k % 4]
    h = bf16_values(raw.view(np.uint16))
    if split == 2:
        return h[(k // 16) * N * 16 + n * 16 + k % 16]
    slot = ((k // 4) * N + n) * 8
    return h[slot + k % 4].astype(np.float64) + h[slot + 4 + k % 4].astype(np.float64)


@pytest.mark.parametrize('A,B,Cc,kind,flip', FORMAT_CASES)
@pytest.mark.parametrize('split', [0, 1, 2])
def test_formats_decode_back_to_the_matrix(A, B, Cc, kind, flip, split):
    g = torch.Generator().manual_seed(100 + A + kind)
    w = torch.randn(A, B, Cc, generator=g)
    if split != 1:
        w = w.bfloat16().float()                   # bf16-representable: quads and chunks round-trip exactly
    w = w.numpy()
    Wm = PK.matrix(w, kind, flip)
    K, N = PK.dims(kind, A, B, Cc)
    assert Wm.shape == (K, N)
    raw = PK.encode(w, kind, flip, split)
    assert raw.dtype == np.uint8 and raw.size == PK.nbytes(kind, A, B, Cc, split)
    back = decode(raw, K, N, split)
    assert not back[K:].any(), 'rows k >= K are zero'
    if split == 1:
        # hi = v (1 + d1), |d1| <= 2^-9; lo = (v - hi)(1 + d2), |d2| <= 2^-9: hi + lo = v + (v - hi) d2, within 2^-18 |v|
        # -- the issue's bound of 2^-16 is the format's promise
        assert np.all(np.abs(back[:K] - Wm.astype(np.float64)) <= 2.0 ** -16 * np.abs(Wm))
    else:
        assert np.array_equal(back[:K], Wm)


def test_matrix_places_every_element_once():
    A, B, Cc = 5, 3, 4
    w = np.arange(1, A * B * Cc + 1, dtype=np.float32).reshape(A, B, Cc)
    for kind, flip in ((1, 0), (2, 0), (2, 1), (3, 0)):
        Wm = PK.matrix(w, kind, flip)
        assert np.array_equal(np.sort(Wm.reshape(-1)), w.reshape(-1))
