"""Times of one optimiser generation of dfl_amd.register on one GPU, split into its three parts.

tools/bench_drr.py's phantom (384 x 320 x 400 voxels of 0.8 mm, three label blobs under three poses) on the training
grid, crop 50 and factor 8 (180 x 180), lambda = 32 candidates per generation; the fixed image is the exact DRR at the
phantom's poses and the candidates are drawn around a start 2 units away in every parameter.

  render      dfl_drr_render, trilinear, step 1 mm, tight boxes, 32 views
  similarity  dfl_sim_gradncc on those 32 views (two kernels), and the same cost computed with torch ops on the device
              (conv2d Sobel, float64 sums) as the yardstick for the kernel
  patch       dfl_sim_patch_gradncc on the same views (two kernels; radius 7, stride 4: 41 x 41 patches of 15 x 15), timed
              the same way, and a whole generation of register(similarity='patch') next to one with the global cost
  gradient    one cost-and-gradient evaluation of the quasi-Newton finish (register(refine=K)) on ONE view: the render, the
              adjoint of the similarity (dfl_sim_gradncc_bwd) and the pose gradient (dfl_drr_pose_grad) timed as calls with
              device events, the whole evaluation (with packing, uploads, the copy and the chain on the host) by the wall
              clock, next to one cost evaluation of one view; in render-equivalents = (render + adjoint + pose gradient) / render
  weighted    the weighted patch cost and the patch adjoint (dfl_sim_patch_eval): the forward on the 32 views
              and the adjoint of one view (device events), and in alternating windows of this process a one-view cost-and-gradient
              evaluation next to the global one (check: within 5 % plus the spread) and a generation next to one with the uniform
              patch cost (check: within 1 % plus the spread)
  many        16 problems with lambda = 32 (register_many) against the same 16 one after the other, in this
              process and run, alternating windows: (i) a generation of register_many against a generation of each of 16
              register() calls, (ii) one lockstep cost-and-gradient round of the finish against 16 single evaluations (wall
              clock), (iii) one dfl_sim_bank_gradncc launch for 512 views against 16 dfl_sim_gradncc launches of 32 (device
              events); (i) and (ii) carry a check: together is no slower than the loop beyond the spread between windows
  host        what is left of a whole generation of register(): sampling, the batched packing, the upload of the
              records, the copy of 32 doubles and the CMA-ES update

Render and similarity are timed with device events around back-to-back calls of the C entry points (argument blocks
built once), after a warm-up, `reps` windows of at least --window seconds each; the median is reported with the
spread.  A generation is timed by the wall clock around register() over enough generations to fill a window (it ends
with a copy to the host, so the device is idle when the clock stops).  There is no earlier implementation to compare
against.

    python tools/bench_register.py [--window 0.3] [--reps 5] [--out profiles/register_bench.json]
"""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import bench_drr as B  # noqa: E402

FACTOR, LAMBDA, STEP_MM = 8, 32, 1.0
MANY = 16                        # problems of the register_many comparison
PATCH_RADIUS, PATCH_STRIDE = 7, 4
THETA0 = (2.0, -2.0, 2.0, 2.0, -2.0, 2.0)


def torch_cost(moving, fixed):
    """The semantics of DESIGN.md section 16 with torch ops on the device, no mask: [V] float64."""
    import torch
    kx = torch.tensor([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]], device=moving.device)
    k = torch.stack([kx, kx.t()])[:, None]
    gm = torch.nn.functional.conv2d(moving[:, None], k).double().flatten(2)          # [V, 2, n]
    gf = torch.nn.functional.conv2d(fixed[None, None], k).double().flatten(2)        # [1, 2, n]
    gm = gm - gm.mean(2, keepdim=True)
    gf = gf - gf.mean(2, keepdim=True)
    ncc = (gm * gf).sum(2) / torch.sqrt((gm * gm).sum(2) * (gf * gf).sum(2))
    return 1.0 - 0.5 * ncc.sum(1)


def windows(fn, window, reps):
    fn_ms = B.timed(fn, 1)                                                            # warm-up
    iters = max(int(1e3 * window / max(B.timed(fn, 1), 1e-3)) + 1, 1)
    ms = [B.timed(fn, iters) for _ in range(reps)]
    return {'ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4), 'calls_per_window': iters,
            'first_call_ms': round(fn_ms, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=0.3, help='seconds of work per timed window, at least')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'register_bench.json'))
    args = ap.parse_args()
    import torch
    from dfl_amd import _native as nat, drr, register as reg
    if not torch.cuda.is_available():
        raise SystemExit('bench_register.py needs a GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda', 0)
    mu, lab = B.phantom(dev)
    vol = drr.Volume(mu, lab)
    f = 1000.0 / B.PIXEL_MM
    K = np.array([[-f, 0, 767.5], [0, -f, 767.5], [0, 0, 1]])
    G, (H, W) = drr.training_grid(B.DET, B.DET, B.CROP, FACTOR)
    grid = drr.Grid(-np.linalg.inv(K) @ G, H, W)
    I2P = np.eye(4)
    I2P[:3, :3] *= B.SPACING
    I2P[:3, 3] = [-150.0, -120.0, -160.0]
    c2is = B.poses(1)[0]
    objects = [drr.Obj(A, m) for A, m in zip(c2is, drr.DEFAULT_MASKS)]
    E = np.eye(4)
    poses = {k: I2P @ A for k, A in zip(drr.POSES, c2is)}                             # P = I2P C2I E
    geom = drr.Geometry(K, E, poses, I2P, G, objects, grid)
    fixed = drr.render(vol, objects, grid, want_labels=False)[0]
    stream = torch.cuda.current_stream(dev).cuda_stream
    prop = torch.cuda.get_device_properties(dev)
    # the candidates of one generation around the start
    ctr = reg.volume_centre(vol.shape, I2P)
    thetas = np.asarray(THETA0)[None] + 2.0 * np.random.default_rng(0).standard_normal((LAMBDA, 6))
    A = np.linalg.inv(I2P)[None] @ reg.pose_deltas(thetas, ctr) @ I2P[None]
    views = [[drr.Obj(A[v] @ ob.c2i, ob.mask) for ob in objects] for v in range(LAMBDA)]
    a, (att, _, _), keep = drr.render_args(vol, views, grid, interp='trilinear', step_mm=STEP_MM, want_labels=False)
    sim = reg.Similarity(fixed, None, LAMBDA)
    sa = sim.args(att)
    nat.call('dfl_drr_render', a, stream)
    nat.call('dfl_sim_gradncc', sa, stream)
    ours, theirs = sim.out.cpu().numpy(), torch_cost(att, fixed).cpu().numpy()
    assert np.abs(ours - theirs).max() <= 1e-5, (ours, theirs)                        # float32 conv2d against float32 Sobel sums
    res = {'tool': 'tools/bench_register.py --window %g --reps %d (device events around back-to-back calls for render and similarity; '
                   'wall clock around register() for a generation; median of the repetitions)' % (args.window, args.reps),
           'date': datetime.date.today().isoformat(), 'device': torch.cuda.get_device_name(dev),
           'arch': getattr(prop, 'gcnArchName', ''), 'compute_units': prop.multi_processor_count, 'torch': torch.__version__,
           'hip': torch.version.hip, 'volume': [B.NX, B.NY, B.NZ], 'output': [H, W], 'lambda': LAMBDA, 'step_mm': STEP_MM,
           'bytes_read_per_generation_by_the_similarity': LAMBDA * H * W * 4,
           'largest_difference_kernel_torch': float(np.abs(ours - theirs).max())}
    res['render'] = windows(lambda: nat.call('dfl_drr_render', a, stream), args.window, args.reps)
    res['similarity'] = windows(lambda: nat.call('dfl_sim_gradncc', sa, stream), args.window, args.reps)
    res['similarity_torch_ops'] = windows(lambda: torch_cost(att, fixed), args.window, args.reps)
    psim = reg.PatchSimilarity(fixed, None, LAMBDA, PATCH_RADIUS, PATCH_STRIDE)
    pa = psim.args(att)
    nat.call('dfl_sim_patch_gradncc', pa, stream)
    pcost = psim.out.cpu().numpy()
    assert np.isfinite(pcost).all() and (pcost > 0).all() and (pcost < 2).all(), pcost
    res['similarity_patch'] = dict(windows(lambda: nat.call('dfl_sim_patch_gradncc', pa, stream), args.window, args.reps),
                                   radius=PATCH_RADIUS, stride=PATCH_STRIDE, patches=psim.patches,
                                   patches_counting=psim.pcount.cpu().numpy().tolist())
    res['pack_poses_host_ms'] = None
    t0 = time.perf_counter()
    for _ in range(50):
        drr.pack(vol, A[:, None] @ np.stack([ob.c2i for ob in objects])[None], [ob.mask for ob in objects], grid, 'trilinear', True)
    res['pack_poses_host_ms'] = round((time.perf_counter() - t0) / 50 * 1e3, 4)

    def generation(**kw):
        reg.register(vol, geom, fixed, theta0=THETA0, popsize=LAMBDA, generations=3, step_mm=STEP_MM, **kw)  # warm-up
        gens, per = 20, []
        for rep in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            reg.register(vol, geom, fixed, theta0=THETA0, popsize=LAMBDA, generations=gens, step_mm=STEP_MM, seed=rep, **kw)
            dt = time.perf_counter() - t0
            if rep == 0:                                                              # size the window from the first run
                gens = max(int(args.window / (dt / (gens + 1))) + 1, 5)
                continue
            per.append(1e3 * dt / (gens + 1))                                         # + 1: the evaluation of the final mean
        return {'ms': round(statistics.median(per), 4), 'min_ms': round(min(per), 4), 'max_ms': round(max(per), 4),
                'generations_per_window': gens}

    res['generation'] = generation()
    res['generation_patch'] = generation(similarity='patch', patch_radius=PATCH_RADIUS, patch_stride=PATCH_STRIDE)
    g, gp = res['generation'], res['generation_patch']
    spread = max(g['max_ms'] - g['min_ms'], gp['max_ms'] - gp['min_ms'])
    res['patch_generation_check'] = {'rule': 'generation_patch.ms <= generation.ms * 1.01 + the larger spread (max - min) of the two',
                                     'spread_ms': round(spread, 4), 'limit_ms': round(g['ms'] * 1.01 + spread, 4),
                                     'ok': bool(gp['ms'] <= g['ms'] * 1.01 + spread)}
    # one evaluation of the quasi-Newton finish: one view at the start pose
    th1 = np.asarray(THETA0)[None]
    back, masks = np.linalg.inv(I2P), [ob.mask for ob in objects]
    c2i1 = (back[None] @ reg.pose_deltas(th1, ctr) @ I2P[None])[:, None] @ np.stack([ob.c2i for ob in objects])[None]
    xis1 = back[None, None] @ reg.pose_delta_jacobians(th1, ctr) @ (np.linalg.inv(reg.pose_deltas(th1, ctr)) @ I2P[None])[:, None]
    recs1 = drr.pack(vol, c2i1, masks, grid, 'trilinear', True)
    a1, (att1, _, _), keep1 = drr.args_for_records(vol, recs1, grid, 'trilinear', STEP_MM)
    nat.call('dfl_drr_render', a1, stream)
    sim1 = reg.Similarity(fixed, None, 1)
    d_att1 = sim1.cost_and_adjoint(att1)[1]
    level1 = reg._Level(vol, grid, fixed, None, 1, STEP_MM)

    def wall(fn, n=40):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        return round((time.perf_counter() - t0) / n * 1e3, 4)       # fn ends with a copy to the host

    grad = {'render': windows(lambda: nat.call('dfl_drr_render', a1, stream), args.window, args.reps),
            'adjoint': windows(lambda: sim1.cost_and_adjoint(att1), args.window, args.reps),
            'pose_gradient': windows(lambda: drr.pose_gradient(vol, recs1, grid, d_att1, None, STEP_MM), args.window, args.reps),
            'cost_wall_ms': wall(lambda: level1.costs(c2i1, masks)),
            'cost_and_gradient_wall_ms': wall(lambda: level1.costs_and_grads(c2i1, masks, xis1, [0, 1, 2]))}
    grad['render_equivalents'] = round((grad['render']['ms'] + grad['adjoint']['ms'] + grad['pose_gradient']['ms']) / grad['render']['ms'], 2)
    res['gradient_one_view'] = grad
    del keep1
    print('one view: render %.4f ms, adjoint %.4f ms, pose gradient %.4f ms = %.2f render-equivalents; wall clock of an evaluation: cost '
          '%.3f ms, cost and gradient %.3f ms' % (grad['render']['ms'], grad['adjoint']['ms'], grad['pose_gradient']['ms'],
                                                   grad['render_equivalents'], grad['cost_wall_ms'], grad['cost_and_gradient_wall_ms']), flush=True)
    # the weighted patch cost and the patch adjoint, next to what they stand beside: the forward next to
    # dfl_sim_patch_gradncc, the adjoint next to dfl_sim_gradncc_bwd, a one-view evaluation next to the global one and a generation
    # next to one with the uniform patch cost -- the last two in alternating windows of this process
    wsim = reg.PatchSimilarity(fixed, None, LAMBDA, PATCH_RADIUS, PATCH_STRIDE, weight='variance')
    wa = wsim.args(att)
    nat.call('dfl_sim_patch_eval', wa, stream)
    wcost = wsim.out.cpu().numpy()
    assert np.isfinite(wcost).all() and (wcost > 0).all() and (wcost < 2).all(), wcost
    wsim1 = reg.PatchSimilarity(fixed, None, 1, PATCH_RADIUS, PATCH_STRIDE, weight='variance')
    wpatch = reg._patch_params(PATCH_RADIUS, PATCH_STRIDE, None) + ('variance',)
    wlevel1 = reg._Level(vol, grid, fixed, None, 1, STEP_MM, wpatch)

    def alternating(fa, fb):
        """`reps` windows of fa and fb in turn (each returns ms per unit): (medians, min and max of each, the larger spread)."""
        fa(), fb()
        a, b = [], []
        for _ in range(args.reps):
            a.append(fa())
            b.append(fb())
        return a, b, max(max(a) - min(a), max(b) - min(b))

    def evaluation(level):
        n = max(int(args.window / (1e-3 * grad['cost_and_gradient_wall_ms'])) + 1, 10)
        return lambda: wall(lambda: level.costs_and_grads(c2i1, masks, xis1, [0, 1, 2]), n)

    ea, eb, espread = alternating(evaluation(level1), evaluation(wlevel1))
    eg, ew = statistics.median(ea), statistics.median(eb)

    def generations_of(**kw):
        gens = max(res['generation']['generations_per_window'], 5)

        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            reg.register(vol, geom, fixed, theta0=THETA0, popsize=LAMBDA, generations=gens, step_mm=STEP_MM, similarity='patch',
                         patch_radius=PATCH_RADIUS, patch_stride=PATCH_STRIDE, **kw)
            return 1e3 * (time.perf_counter() - t0) / (gens + 1)
        return run

    ga, gb, gspread = alternating(generations_of(), generations_of(patch_weight='variance'))
    gu, gw = statistics.median(ga), statistics.median(gb)
    res['weighted_patch'] = {
        'radius': PATCH_RADIUS, 'stride': PATCH_STRIDE, 'patches': wsim.patches,
        'similarity': windows(lambda: nat.call('dfl_sim_patch_eval', wa, stream), args.window, args.reps),
        'adjoint_one_view': windows(lambda: wsim1.cost_and_adjoint(att1), args.window, args.reps),
        'global_adjoint_one_view_ms': grad['adjoint']['ms'],
        'cost_and_gradient': {'global_wall_ms': round(eg, 4), 'global_min_max_ms': [round(min(ea), 4), round(max(ea), 4)],
                              'weighted_patch_wall_ms': round(ew, 4), 'weighted_patch_min_max_ms': [round(min(eb), 4), round(max(eb), 4)],
                              'spread_ms': round(espread, 4), 'limit_ms': round(eg * 1.05 + espread, 4),
                              'rule': 'weighted_patch_wall_ms <= global_wall_ms * 1.05 + the larger spread (max - min) of the two',
                              'ok': bool(ew <= eg * 1.05 + espread)},
        'generation': {'uniform_patch_ms': round(gu, 4), 'uniform_patch_min_max_ms': [round(min(ga), 4), round(max(ga), 4)],
                       'weighted_patch_ms': round(gw, 4), 'weighted_patch_min_max_ms': [round(min(gb), 4), round(max(gb), 4)],
                       'spread_ms': round(gspread, 4), 'limit_ms': round(gu * 1.01 + gspread, 4),
                       'rule': 'weighted_patch_ms <= uniform_patch_ms * 1.01 + the larger spread (max - min) of the two',
                       'ok': bool(gw <= gu * 1.01 + gspread)}}
    wp = res['weighted_patch']
    print('weighted patch cost: similarity %.4f ms (uniform %.4f), adjoint of one view %.4f ms (global %.4f); one-view cost and gradient %.3f '
          'ms (global %.3f, limit %.3f: %s); generation %.3f ms (uniform patch %.3f, limit %.3f: %s)'
          % (wp['similarity']['ms'], res['similarity_patch']['ms'], wp['adjoint_one_view']['ms'], grad['adjoint']['ms'], ew, eg,
             wp['cost_and_gradient']['limit_ms'], 'ok' if wp['cost_and_gradient']['ok'] else 'ABOVE', gw, gu, wp['generation']['limit_ms'],
             'ok' if wp['generation']['ok'] else 'ABOVE'), flush=True)
    # N problems at once (register_many) against the same N one after the other, in this process
    N = MANY
    offsets = 1.5 * np.random.default_rng(1).standard_normal((N, 6))
    geoms, fixeds = [], []
    for t in offsets:                                                                 # every problem: its own poses and fixed image
        Dn = reg.pose_delta(t, ctr)
        named = {k: Dn @ P for k, P in poses.items()}
        obs = [drr.Obj(back @ named[k] @ np.linalg.inv(E), ob.mask) for k, ob in zip(drr.POSES, objects)]
        geoms.append(drr.Geometry(K, E, named, I2P, G, obs, grid))
        fixeds.append(drr.render(vol, obs, grid, want_labels=False)[0])
    fixed_n = torch.stack(fixeds).contiguous()
    theta_n = np.tile(np.asarray(THETA0), (N, 1))

    def pair(many, loop, unit):
        """`reps` windows of both, alternating; ms per `unit` of each, their ratio and the check against the spread."""
        many(), loop()                                                                # warm-up
        a, b = [], []
        for _ in range(args.reps):
            for fn, into in ((many, a), (loop, b)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = fn()
                torch.cuda.synchronize()
                into.append(1e3 * (time.perf_counter() - t0) / n)
        spread = max(max(a) - min(a), max(b) - min(b))
        ma, mb = statistics.median(a), statistics.median(b)
        return {'unit': unit, 'together_ms': round(ma, 4), 'together_min_max_ms': [round(min(a), 4), round(max(a), 4)],
                'one_after_the_other_ms': round(mb, 4), 'one_after_the_other_min_max_ms': [round(min(b), 4), round(max(b), 4)],
                'ratio_together_over_loop': round(ma / mb, 4), 'spread_ms': round(spread, 4),
                'rule': 'together_ms <= one_after_the_other_ms + the larger spread (max - min) of the two', 'ok': bool(ma <= mb + spread)}

    gens_many = max(int(args.window / (N * 1e-3 * res['generation']['ms'])) + 1, 3)

    def many_generations():
        reg.register_many(vol, geoms, fixed_n, theta0=theta_n, popsize=LAMBDA, generations=gens_many, step_mm=STEP_MM)
        return gens_many + 1                                                          # + 1: the evaluation of the final means

    def loop_generations():
        for i in range(N):
            reg.register(vol, geoms[i], fixed_n[i], theta0=theta_n[i], popsize=LAMBDA, generations=gens_many, step_mm=STEP_MM)
        return gens_many + 1

    many = {'problems': N, 'lambda': LAMBDA, 'generations_per_window': gens_many,
            'generation': pair(many_generations, loop_generations, 'one generation of %d problems (%d views)' % (N, N * LAMBDA))}
    # one round of the finish: a cost-and-gradient evaluation of every problem at its start
    probs = [reg._Problem(vol.shape, g_, (0, 1, 2), None, None, reg.ROT_UNIT, None, 0.0) for g_ in geoms]
    c2i_n = [p.c2is_of(th1) for p in probs]
    xis_n = [p.xis_of(th1) for p in probs]
    level_n = reg._Level(vol, grid, None, None, N, STEP_MM, None, bank=(fixed_n, None))
    levels_1 = [reg._Level(vol, grid, fixed_n[i], None, 1, STEP_MM) for i in range(N)]
    which = np.arange(N, dtype=np.int32)
    rounds = max(int(args.window / (N * 1e-3 * grad['cost_and_gradient_wall_ms'])) + 1, 3)

    def round_together():
        for _ in range(rounds):
            recs, att_n, alive = level_n._render(np.concatenate(c2i_n), masks)
            both, piv = level_n._cost_and_moments(recs, att_n, *level_n.sim.cost_and_adjoint(att_n, which))
            for k in range(N):
                reg._theta_chain(both[k:k + 1], piv[k:k + 1], xis_n[k], [0, 1, 2])
        return rounds

    def round_loop():
        for _ in range(rounds):
            for k in range(N):
                levels_1[k].costs_and_grads(c2i_n[k], masks, xis_n[k], [0, 1, 2])
        return rounds

    many['gradient_round'] = pair(round_together, round_loop, 'one cost-and-gradient evaluation of each of %d problems' % N)
    # the similarity alone: one bank launch for N lambda views against N launches of lambda views
    att_many = att.repeat(N, 1, 1).contiguous()
    bank = reg.SimilarityBank(fixed_n, None, N * LAMBDA)
    ba = bank.args(att_many, bank.fixed_of(np.repeat(which, LAMBDA), N * LAMBDA))
    sims = [reg.Similarity(fixed_n[i], None, LAMBDA) for i in range(N)]
    sas = [s_.args(att_many[i * LAMBDA:(i + 1) * LAMBDA]) for i, s_ in enumerate(sims)]
    nat.call('dfl_sim_bank_gradncc', ba, stream)
    for sa_ in sas:
        nat.call('dfl_sim_gradncc', sa_, stream)
    assert torch.equal(bank.out, torch.cat([s_.out for s_ in sims]))                  # the same bits, as the tests hold
    one_launch = windows(lambda: nat.call('dfl_sim_bank_gradncc', ba, stream), args.window, args.reps)
    n_launches = windows(lambda: [nat.call('dfl_sim_gradncc', sa_, stream) for sa_ in sas], args.window, args.reps)
    many['similarity'] = {'bank_launch_%d_views' % (N * LAMBDA): one_launch, '%d_launches_of_%d_views' % (N, LAMBDA): n_launches,
                          'ratio_bank_over_launches': round(one_launch['ms'] / n_launches['ms'], 4)}
    res['many'] = many
    print('%d problems, lambda %d: generation %.3f ms together, %.3f ms one after the other (ratio %.3f, %s); gradient round %.3f ms '
          'together, %.3f ms one after the other (ratio %.3f, %s); similarity %.4f ms in one bank launch, %.4f ms in %d launches (ratio %.3f)'
          % (N, LAMBDA, many['generation']['together_ms'], many['generation']['one_after_the_other_ms'],
             many['generation']['ratio_together_over_loop'], 'ok' if many['generation']['ok'] else 'SLOWER',
             many['gradient_round']['together_ms'], many['gradient_round']['one_after_the_other_ms'],
             many['gradient_round']['ratio_together_over_loop'], 'ok' if many['gradient_round']['ok'] else 'SLOWER',
             one_launch['ms'], n_launches['ms'], N, many['similarity']['ratio_bank_over_launches']), flush=True)
    res['host_side'] = {'ms': round(res['generation']['ms'] - res['render']['ms'] - res['similarity']['ms'], 4)}
    print('180 x 180, lambda 32: generation %.3f ms = render %.3f + similarity %.3f (torch ops %.3f) + host %.3f (of which packing %.3f)'
          % (res['generation']['ms'], res['render']['ms'], res['similarity']['ms'], res['similarity_torch_ops']['ms'], res['host_side']['ms'],
             res['pack_poses_host_ms']), flush=True)
    print('patch cost (radius %d, stride %d, %d patches): similarity %.4f ms (global %.4f), generation %.3f ms (global %.3f, limit %.3f: %s)'
          % (PATCH_RADIUS, PATCH_STRIDE, psim.patches, res['similarity_patch']['ms'], res['similarity']['ms'], gp['ms'], g['ms'],
             res['patch_generation_check']['limit_ms'], 'ok' if res['patch_generation_check']['ok'] else 'TOO SLOW'), flush=True)
    del keep
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
