"""The weight re-layouts dfl_pack_weights and dfl_pack_weights_tiled (the "weight pack" half of csrc/bn_elem.hip) through the C
ABI, byte for byte against tests/pack_ref.py: the numpy restatement of the three index maps and three formats of
include/dfl_hip.h (tests/test_pack_ref_cpu.py holds that model to the convolutions it is named for).

The master and every destination lie between NaN sentinels (Buf of tests/test_gpu_streaming.py): a destination starts as NaN
all over, the guard words on both sides must come back untouched, no NaN may remain inside, and every call runs twice from the same
inputs with the same bytes.  The shapes are the smallest at which each branch and each edge guard of pack_kernel can go wrong."""
import numpy as np
import pytest
import torch

from dfl_amd import _native as nat
import pack_ref as PK
from test_gpu_streaming import Buf, DEV, assert_bits, stream
from test_gpu_finalize import fetch, sync, table, twice

pytestmark = pytest.mark.gpu
KINDS = [(1, 0), (2, 0), (2, 1), (3, 0)]


def lib():
    return nat.lib()


def master(shape, seed):
    """A parameter [A][B][C] between sentinels (read only) and its values."""
    A, B, Cc = shape
    w = torch.randn(A, B, Cc, generator=torch.Generator().manual_seed(seed))
    b = Buf((1,), A * B * Cc, A * B * Cc, False)
    b.set(w.reshape(1, -1))
    return b, w.numpy()


def layout(kind, shape, split):
    """A destination of exactly the layout's size: 4-byte slots of the quad formats, bf16 of the chunks."""
    n = PK.nbytes(kind, *shape, split) // (2 if split == 2 else 4)
    return Buf((1,), n, n, split == 2).allow()


def fetched(b, split, what):
    """(None, bits) of a destination after the call: guards intact (Buf.fetch), no NaN left in the layout's own number format."""
    _, bits = fetch(b, what, finite=False)
    halves = bits.view(torch.int16) if split else None              # both quad-split halves and the chunks are bf16
    vals = halves.view(torch.bfloat16) if split else bits.view(torch.float32)
    assert not bool(torch.isnan(vals).any()), '%s: %d NaN left in the destination' % (what, int(torch.isnan(vals).sum()))
    return None, bits


def assert_layout(bits, w, kind, flip, split, what):
    ref = torch.from_numpy(PK.encode(w, kind, flip, split))
    assert_bits(bits.contiguous().view(torch.uint8), ref, what + ' against pack_ref')


def record(rec, src, dst, shape, kind, flip, split):
    rec.src, rec.dst, (rec.A, rec.B, rec.C), rec.kind, rec.flip, rec.split = src, dst, shape, kind, flip, split


def flat_once(jobs, max_elems, what):
    """One dfl_pack_weights launch over jobs = [(master Buf, shape, kind, flip, split, destination Buf)]."""
    def once():
        arr = (nat.PackJob * len(jobs))()
        srcs = {id(j[0]): j[0].upload() for j in jobs}             # jobs may share a master: one upload each
        for rec, (src, shape, kind, flip, split, dst) in zip(arr, jobs):
            record(rec, srcs[id(src)], dst.upload(), shape, kind, flip, split)
        tab = table(arr)
        sync(lib().dfl_pack_weights(tab.data_ptr(), len(jobs), max_elems, stream()), what)
        for src, *_ in jobs:
            src.fetch(what + ': the master')
        return [fetched(dst, split, '%s job %d' % (what, i)) for i, (_, _, _, _, split, dst) in enumerate(jobs)]
    return [r[1] for r in twice(once, what)]


def flat_check(shape, kind, flip, split, seed=0):
    """One job in one launch, as the plan sizes it; returns the destination's bits."""
    src, w = master(shape, 1000 + seed + shape[0] * shape[1])
    what = 'dfl_pack_weights %s kind %d flip %d split %d' % (shape, kind, flip, split)
    bits, = flat_once([(src, shape, kind, flip, split, layout(kind, shape, split))], shape[0] * shape[1] * shape[2], what)
    assert_layout(bits, w, kind, flip, split, what)
    return bits


# ---------------------------------------------------------------------------------------------------- dfl_pack_weights, one job
# pack_kernel tiles a job (32 x 32 x C tiles through LDS) when C <= PK_CMAX = 9 and its k-run channel count -- B for kind 1, A for
# kinds 2 and 3 -- is a multiple of 16 (split 2) or of 4 (splits 0, 1); everything else goes element by element.  (A, B, KH = KW):
#                 splits 0, 1                                        split 2
#   (64,32,3)     tiled, full tiles                                  tiled, full tiles
#   (48,20,3)     tiled: nb = 20, na = 16 in the second tile         kind 1 (B = 20): element-wise, K = 180 zero-padded to 192;
#                                                                    kinds 2, 3 (A = 48): tiled, nb = 20, na = 16
#   (40,48,3)     tiled: nb = 16 and na = 8 in the second tiles      kind 1 (B = 48): tiled, nb = 16 (the second block of 16 k is
#                                                                    skipped), na = 8;  kinds 2, 3 (A = 40): element-wise
#   (80,48,2)     tiled: na = 16 in the third tile, nb = 16          tiled: kinds 2, 3 skip the second block of 16 k at na = 16
#   (36,33,3)     kind 1 (B = 33): element-wise; kinds 2, 3          element-wise (33, 36 are no multiples of 16)
#                 (A = 36): tiled, last tile 4 high and 1 wide
#   (33,36,1)     kind 1 (B = 36): tiled, last tile 1 high and       element-wise
#                 4 wide; kinds 2, 3 (A = 33): element-wise
#   (32,1,3)      the first layer.  kind 1 (B = 1): element-wise,    kind 1: element-wise, K = 9 padded to 16;
#                 K = 9 padded to 12; kinds 2, 3: tiled, nb = 1      kinds 2, 3: tiled, nb = 1
#   (7,5,3)       element-wise, K = 45 / 63 / 7                      element-wise
#   (6,10,2)      element-wise, K = 40 / 24 / 6                      element-wise
#   (128,64,1)    tiled, 4 x 2 full tiles, C = 1                     tiled
#   (16,16,2)     tiled, one tile of 16 x 16                         tiled: one block of 16 k
#   (16,16,4)     C = 16 > PK_CMAX: element-wise (the LDS tile       element-wise
#                 holds 9 taps)
FLAT_SHAPES = [(64, 32, 3), (48, 20, 3), (40, 48, 3), (80, 48, 2), (36, 33, 3), (33, 36, 1), (32, 1, 3), (7, 5, 3), (6, 10, 2),
               (128, 64, 1), (16, 16, 2), (16, 16, 4)]


def cube(s):
    return (s[0], s[1], s[2] * s[2])


@pytest.mark.parametrize('split', [0, 1, 2])
@pytest.mark.parametrize('shape', FLAT_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_pack_weights_every_branch_and_edge(shape, split):
    for kind, flip in KINDS:
        flat_check(cube(shape), kind, flip, split)


@pytest.mark.parametrize('shape', [(64, 32, 3), (48, 20, 3), (7, 5, 3), (32, 1, 3), (128, 64, 1), (16, 16, 2), (6, 10, 2)])
def test_pack_weights_layout(shape):
    """All three index maps of dfl_pack_weights (tiled and element-wise paths), fp32 quads."""
    for kind, flip in ((1, 0), (2, 1), (2, 0), (3, 0)):
        flat_check(cube(shape), kind, flip, 0, seed=1)


def test_pack_bf16_chunk_layout():
    for (A, B, KK, kind, flip) in ((32, 16, 3, 1, 0), (32, 16, 3, 2, 1), (64, 32, 1, 1, 0), (48, 16, 2, 3, 0), (16, 32, 2, 1, 0)):
        flat_check((A, B, KK * KK), kind, flip, 2, seed=2)


# ---------------------------------------------------------------------------------------------------- several jobs in one launch
# one job per branch: cells tiled (na = 16 in the second tile), cells element-wise, quads tiled (nb = 20, na = 8), quads element-wise
FOUR_BRANCHES = [((48, 32, 9), 2, 1, 2), ((48, 20, 9), 1, 0, 2), ((40, 20, 9), 1, 0, 1), ((7, 5, 9), 3, 0, 0)]


@pytest.mark.parametrize('max_elems', ['max', 1])       # 1: one workgroup per job walks every tile (the barrier at the loop's top)
def test_pack_weights_four_branches_in_one_launch(max_elems):
    jobs, ws = [], []
    for i, (shape, kind, flip, split) in enumerate(FOUR_BRANCHES):
        src, w = master(shape, 2000 + i)
        jobs.append((src, shape, kind, flip, split, layout(kind, shape, split)))
        ws.append(w)
    mx = max(s[0] * s[1] * s[2] for s, *_ in FOUR_BRANCHES) if max_elems == 'max' else 1
    what = 'dfl_pack_weights, four jobs, max_elems %d' % mx
    for i, bits in enumerate(flat_once(jobs, mx, what)):
        _, kind, flip, split = FOUR_BRANCHES[i]
        assert_layout(bits, ws[i], kind, flip, split, '%s, job %d' % (what, i))


@pytest.mark.parametrize('split', [0, 1, 2])
def test_pack_weights_workgroups_without_a_tile_write_nothing(split):
    """A two-tile job in the widest grid (1024 workgroups): 1022 of them have nothing to do."""
    shape = (64, 32, 9)
    src, w = master(shape, 2100)
    jobs = [(src, shape, kind, flip, split, layout(kind, shape, split)) for kind, flip in ((1, 0), (2, 1))]
    what = 'dfl_pack_weights, two tiles under 1024 workgroups, split %d' % split
    for (_, _, kind, flip, _, _), bits in zip(jobs, flat_once(jobs, 1024 * 2048, what)):
        assert_layout(bits, w, kind, flip, split, what)


# ---------------------------------------------------------------------------------------------------- dfl_pack_weights_tiled
# pack_tile: one workgroup per 32 x 32 x C tile of all jobs, found by the binary search `jobs[mid].first_tile <= blockIdx.x`;
# a job = (shape, (kind, flip, split), second layout or None)
TILED_JOBS = [((32, 32, 1), (1, 0, 0), None),                      # a first job of a single tile
              ((64, 32, 9), (1, 0, 2), (2, 1, 1)),                 # formats mixed as test_gpu_finalize.PACK_JOBS mixes them
              ((32, 64, 4), (3, 0, 1), (1, 0, 2)),
              ((64, 64, 1), (2, 0, 0), (3, 0, 0)),
              ((32, 96, 9), (2, 1, 2), None)]


def tiled_once(jobs, what):
    """One dfl_pack_weights_tiled launch over jobs = [(master Buf, shape, (kind, flip, split), first destination,
    None | (kind, flip, split), second destination | None)]; the bits of every destination, in order."""
    def once():
        arr, tiles = (nat.PackJob * len(jobs))(), 0
        for rec, (src, shape, l1, d1, l2, d2) in zip(arr, jobs):
            record(rec, src.upload(), d1.upload(), shape, *l1)
            if l2 is not None:
                rec.dst2, (rec.kind2, rec.flip2, rec.split2) = d2.upload(), l2
            rec.first_tile = tiles
            tiles += (shape[0] // 32) * (shape[1] // 32)
        tab = table(arr)
        sync(lib().dfl_pack_weights_tiled(tab.data_ptr(), len(jobs), tiles, stream()), what)
        res = []
        for i, (src, _, l1, d1, l2, d2) in enumerate(jobs):
            src.fetch(what + ': the master')
            res += [fetched(d, l[2], '%s job %d' % (what, i)) for l, d in ((l1, d1), (l2, d2)) if l is not None]
        return res
    return [r[1] for r in twice(once, what)]


@pytest.mark.parametrize('which', [(0,), (0, 1), (0, 1, 2, 3, 4), (4, 3)], ids=['one_job', 'two_jobs', 'five_jobs', 'no_single_tile_first'])
def test_pack_weights_tiled_job_lists(which):
    jobs, expect = [], []
    for k in which:
        shape, l1, l2 = TILED_JOBS[k]
        src, w = master(shape, 3000 + k)
        jobs.append((src, shape, l1, layout(l1[0], shape, l1[2]), l2, None if l2 is None else layout(l2[0], shape, l2[2])))
        expect += [(w, l, k) for l in (l1, l2) if l is not None]
    what = 'dfl_pack_weights_tiled, jobs %s' % (which,)
    for bits, (w, (kind, flip, split), k) in zip(tiled_once(jobs, what), expect):
        assert_layout(bits, w, kind, flip, split, '%s, job %d kind %d flip %d split %d' % (what, k, kind, flip, split))


@pytest.mark.parametrize('shape', [(64, 32, 3), (32, 64, 1), (128, 96, 2), (64, 64, 3)])
@pytest.mark.parametrize('split', [0, 1])
def test_pack_weights_tiled_quad_layouts(shape, split):
    """dfl_pack_weights_tiled writes the fp32 quad layouts and the split hi | lo bf16 quads too: both layouts of a job, bit for bit
    what pack_ref gives and what dfl_pack_weights writes."""
    shape = cube(shape)
    for l1, l2 in (((1, 0), (2, 1)), ((3, 0), (1, 0)), ((2, 0), (3, 0))):
        src, w = master(shape, 4000 + shape[0] * shape[1] + shape[2])
        l1, l2 = l1 + (split,), l2 + (split,)
        what = 'dfl_pack_weights_tiled %s split %d, kinds %d + %d' % (shape, split, l1[0], l2[0])
        got = tiled_once([(src, shape, l1, layout(l1[0], shape, split), l2, layout(l2[0], shape, split))], what)
        for bits, (kind, flip, _) in zip(got, (l1, l2)):
            assert_layout(bits, w, kind, flip, split, what)
            flat, = flat_once([(src, shape, kind, flip, split, layout(kind, shape, split))], shape[0] * shape[1] * shape[2], what + ', flat')
            assert_bits(bits, flat, what + ': tiled against dfl_pack_weights')
