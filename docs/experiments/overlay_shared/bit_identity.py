#!/usr/bin/env python3
"""Every overlay call of tests/test_gpu_overlay.py and tests/test_gpu_fullres_overlay.py under two builds of the library,
byte for byte:
    python docs/experiments/overlay_shared/bit_identity.py PARENT_LIBRARY [NEW_LIBRARY (default: the tree's own)]
Each library runs in a fresh child process (DFL_LIB_OVERRIDE) with this tree's Python.  A child calls the fixture tests of
the two files as they stand (every overlay_*.npz and fullres_*.npz: fixtures, stamps, batch against single, resizes,
chunking, the blend table) and, with the input recipe of tools/bench_overlay.py and tools/bench_fullres_overlay.py, one
1536^2 x 4 call of render (tiles and canvas) and of render_full_res.  It keeps what every call of overlay.render,
overlay.render_full_res and overlay.resize_bilinear returns and the scratch buffer the call made (filled with NaN before the
library writes it).  The blend test calls the C entry point itself: it is held to Pillow's table, not recorded.
Exit status 1 if an array differs."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
S, B = 1536, 4


def child(path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
    import torch
    from dfl_amd import overlay
    import test_gpu_fullres_overlay as TF
    import test_gpu_overlay as TO
    out, made = {}, []
    make_scratch = overlay._scratch

    def scratch(img):
        made.append(make_scratch(img).fill_(float('nan')))
        return made[-1]

    def recorded(name, fn):
        def call(*args, **kw):
            del made[:]
            res = fn(*args, **kw)
            torch.cuda.synchronize()
            tag = '%03d %s' % (len({k.split('/')[0] for k in out}), name)
            out[tag + '/out'] = res.cpu().numpy().copy()
            for t in made:
                out[tag + '/scratch'] = t.cpu().numpy()
            return res
        return call

    overlay._scratch = scratch
    for name in ('render', 'render_full_res', 'resize_bilinear'):
        setattr(overlay, name, recorded(name, getattr(overlay, name)))
    for name in TO.FIXTURES:
        TO.test_render_is_bit_identical_to_the_reference(name)
    TO.test_kernel_ellipse_matches_every_reachable_pillow_stamp()
    TO.test_batch_of_11_equals_single_renders_and_the_grid()
    for name in TF.RESIZE:
        TF.test_resize_is_bit_identical_to_pillow(name)
    for name in TF.OVERLAYS:
        TF.test_overlay_is_bit_identical_to_the_reference(name)
    TF.test_chunking_does_not_change_the_canvas()
    TF.test_text_blend_matches_pillow_for_every_coverage_and_background()
    g = torch.Generator(device='cuda').manual_seed(0)                       # tools/bench_overlay.py
    imgs = torch.rand((B, S, S), device='cuda', generator=g)
    segs = (torch.rand((B, S, S), device='cuda', generator=g) * 8).to(torch.uint8)
    lands = torch.rand((B, 14, 2), device='cuda', generator=g) * S
    for grid in (False, True):
        overlay.render(imgs, segs=segs, gt_lands=lands, radius=16.0, grid=grid)
    rng = np.random.default_rng(0)                                          # tools/bench_fullres_overlay.py
    marks = [[('FH-l' if l == 0 else 'FH-r' if l == 1 else 'L%02d' % l, rng.uniform(0, S, 2).astype(np.float32))
              for l in range(14)] for _ in range(B)]
    overlay.render_full_res(imgs, segs, [b % 2 for b in range(B)], marks, [(1, 1)] * B)
    np.savez(path, **out)
    print('%d arrays of %d calls -> %s (library: %s)' % (len(out), len({k.split('/')[0] for k in out}), os.path.basename(path),
                                                        os.environ.get('DFL_LIB_OVERRIDE', "the tree's own")))


def run(lib, path):
    env = dict(os.environ)
    env.pop('DFL_LIB_OVERRIDE', None)
    if lib is not None:
        env['DFL_LIB_OVERRIDE'] = os.path.abspath(lib)
    subprocess.run([sys.executable, os.path.abspath(__file__), '--child', path], env=env, check=True, timeout=300)
    return np.load(path)


def main():
    with tempfile.TemporaryDirectory() as d:
        a = run(sys.argv[1], os.path.join(d, 'parent.npz'))
        b = run(sys.argv[2] if len(sys.argv) > 2 else None, os.path.join(d, 'new.npz'))   # only after the first child ended cleanly
        assert sorted(a.files) == sorted(b.files), 'the two runs hold different arrays'
        diff = [k for k in sorted(a.files) if a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
        print('%d arrays of %d calls, %d differ' % (len(a.files), len({k.split('/')[0] for k in a.files}), len(diff)))
        for k in diff:
            print('  DIFFERS %s' % k)
    return 1 if diff else 0


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--child':
        child(sys.argv[2])
    else:
        sys.exit(main())
