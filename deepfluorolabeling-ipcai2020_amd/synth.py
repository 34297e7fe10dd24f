"""Synthetic training data from the CT: poses sampled around the acquired ones, rendered by dfl_amd.drr, turned into
detector images by csrc/expose.hip (dfl_drr_expose) and written as a full-resolution file or as a training file.
'gt-seg', 'gt-landmarks' and 'gt-poses' are exact by construction.  DESIGN.md section 17 is the specification;
tests/expose_ref.py restates the detector model in numpy.

Poses (float64 numpy on the host; P_o = the acquired cam-to-*-vol (fullres.gt_poses) maps the camera world frame to the volume):

    seed          synthetic view n starts from acquired projection n mod (number of acquired projections)
    common motion Wm = register.pose_delta([w, t_w], c_w, rot_unit=1): the rotation exp(hat w) about c_w, then the
                  translation t_w, in the camera world frame; P_o' = P_o inv(Wm) for all three bones.
                  c_w = inv(P_pelvis) (centroid of the 3D landmarks); w ~ N(0, rot_sigma_deg) per axis (degrees);
                  t_w = E[:3, :3]^T t_c with t_c ~ N(0, trans_sigma_mm[x, y, z]) in the camera projective frame
    articulation  P_f'' = A_f P_f', A_f = pose_delta([a, 0], FH, 1) about the femoral head 'FH-l' / 'FH-r' in the volume's
                  physical frame, a ~ N(0, femur_sigma_deg) per axis; no such landmark: no articulation
    acceptance    at least min_lands 3D landmarks project (under the new pelvis pose) inside the crop window
                  [crop, cols - 1 - crop] x [crop, rows - 1 - crop]; else the motion is drawn again, 20 draws at most
    fov flags     1 when the femoral head projects (under that femur's new pose) inside the detector, else 0; without the
                  landmark the seed's flag

Every draw takes 12 normals from numpy.random.default_rng([seed, specimen index]) in the order w, t_c, a_left, a_right,
whatever the specimen has, so the stream of one specimen does not depend on another.  The noise keys of view n do not
come from that stream (noise_keys): its image noise does not depend on how many draws were rejected.

Tools (tools > 0; dfl_amd.tools): view n of specimen k draws up to `tools` capsules around the
landmarks from its own stream numpy.random.default_rng([seed, k, 1, n]) and adds their line integrals between the render
and the detector model.  The pose stream and the noise keys do not move; tools = 0 takes no draw and makes no launch.

Tensors on the CPU and a machine without a GPU are refused: there is no CPU path.
"""
import numpy as np
import torch

from . import _native as nat
from . import drr, fullres, h5lite, preprocess, register
from . import tools as tools_mod

__all__ = ['gaussian_taps', 'noise_keys', 'expose', 'expose_args', 'draw_motion', 'apply_motion', 'lands_in_window', 'fov_flags',
           'sample_pose', 'sample_poses', 'tool_rng', 'synthesize', 'MAX_DRAWS', 'DEFAULTS']

MAX_DRAWS = 20
FEMUR_HEADS = ('FH-l', 'FH-r')
DEFAULTS = dict(rot_sigma_deg=10.0, trans_sigma_mm=(20.0, 20.0, 50.0), femur_sigma_deg=5.0, min_lands=4, photons=20000.0,
                gain=2.0, electronic_sigma=3.0, blur_sigma_px=1.0)
_M64 = (1 << 64) - 1


# ---- the detector model ------------------------------------------------------------------------------------------------
def gaussian_taps(sigma_px):
    """(taps float32 [2 rho + 1], rho): a float64 Gaussian of sigma_px sampled at -rho..rho, rho = ceil(3 sigma),
    normalised to sum 1 and rounded to float32.  sigma 0 gives ([1], 0); rho above 8 is refused."""
    sigma = float(sigma_px)
    if not (sigma >= 0.0 and np.isfinite(sigma)):
        raise nat.DflError('synth.gaussian_taps: blur_sigma_px must not be negative, got %r' % (sigma_px,))
    rho = int(np.ceil(3.0 * sigma))
    if rho > nat.EXPOSE_MAX_RADIUS:
        raise nat.DflError('synth.gaussian_taps: blur_sigma_px %g needs a radius of %d pixels (at most %d are supported)'
                           % (sigma, rho, nat.EXPOSE_MAX_RADIUS))
    if rho == 0:
        return np.ones(1, np.float32), 0
    k = np.arange(-rho, rho + 1, dtype=np.float64)
    w = np.exp(-0.5 * (k / sigma) ** 2)
    return (w / w.sum()).astype(np.float32), rho


def _mix64(x):
    """The finaliser of splitmix64 (Steele, Lea, Flood 2014) on a 64-bit integer."""
    x &= _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def noise_keys(seed, specimen, view):
    """(key_q, key_e), the 64-bit Philox keys of the quantum and the electronic noise of one synthetic view:
    mix64(mix64(mix64(seed) + specimen + 1) + 2 view + which), which = 0, 1 -- three chained splitmix64 finalisers, a
    bijection of the last argument for fixed earlier ones."""
    base = _mix64(_mix64(int(seed)) + int(specimen) + 1)
    return _mix64(base + 2 * int(view)), _mix64(base + 2 * int(view) + 1)


def _key_tensor(keys, V, dev, what):
    keys = [int(k) & _M64 for k in keys]
    if len(keys) != V:
        raise nat.DflError('synth.expose: %d %s keys for %d views' % (len(keys), what, V))
    return torch.from_numpy(np.array(keys, np.uint64).view(np.int64)).to(dev)


def expose_args(att, photons, gain, electronic_sigma, blur_sigma_px, keys_q=None, keys_e=None, u16=True, want_normals=False):
    """(ExposeArgs, (out, z1, z2), tensors to keep alive): the argument block of dfl_drr_expose and its freshly allocated
    outputs, nothing launched.  keys_q / keys_e None switches that noise term off."""
    if not torch.is_tensor(att) or not att.is_cuda:
        raise nat.DflError('synth.expose needs its tensor on the GPU (no CPU path)')
    if att.dim() != 3 or att.dtype != torch.float32:
        raise nat.DflError('synth.expose: att must be float32 [V, R, C], got %s %s' % (att.dtype, tuple(att.shape)))
    att = att.detach().contiguous()
    V, R, Cn = att.shape
    taps, rho = gaussian_taps(blur_sigma_px)
    dev = att.device
    kq = None if keys_q is None else _key_tensor(keys_q, V, dev, 'quantum')
    ke = None if keys_e is None else _key_tensor(keys_e, V, dev, 'electronic')
    out = torch.empty((V, R, Cn), dtype=torch.uint16 if u16 else torch.float32, device=dev)
    z1 = torch.empty((V, R, Cn), dtype=torch.float32, device=dev) if want_normals and kq is not None else None
    z2 = torch.empty((V, R, Cn), dtype=torch.float32, device=dev) if want_normals and ke is not None else None
    full = np.zeros(2 * nat.EXPOSE_MAX_RADIUS + 1, np.float32)
    full[:taps.size] = taps
    a = nat.ExposeArgs(att=att.data_ptr(), out=out.data_ptr(), key_q=nat.ptr(kq), key_e=nat.ptr(ke), z1=nat.ptr(z1), z2=nat.ptr(z2),
                       taps=(nat.f32 * full.size)(*full), rho=rho, V=V, R=R, C=Cn, u16=int(bool(u16)), quantum=int(kq is not None),
                       electronic=int(ke is not None), photons=float(photons), gain=float(gain),
                       electronic_sigma=float(electronic_sigma))
    return a, (out, z1, z2), [att, kq, ke]


def expose(att, photons=DEFAULTS['photons'], gain=DEFAULTS['gain'], electronic_sigma=DEFAULTS['electronic_sigma'],
           blur_sigma_px=DEFAULTS['blur_sigma_px'], keys_q=None, keys_e=None, u16=True, want_normals=False):
    """Line integrals att [V, R, C] (float32, on the GPU) -> detector intensities [V, R, C], uint16 or float32:
    gain (N + sqrt(N) z1 + electronic_sigma z2), N = photons blur(exp(-att)); want_normals also returns (z1, z2)."""
    a, (out, z1, z2), keep = expose_args(att, photons, gain, electronic_sigma, blur_sigma_px, keys_q, keys_e, u16, want_normals)
    dev = out.device
    with torch.cuda.device(dev):
        nat.call('dfl_drr_expose', a, torch.cuda.current_stream(dev).cuda_stream)
    del keep
    return (out, z1, z2) if want_normals else out


# ---- poses -------------------------------------------------------------------------------------------------------------
def draw_motion(rng, rot_sigma_deg=DEFAULTS['rot_sigma_deg'], trans_sigma_mm=DEFAULTS['trans_sigma_mm'],
                femur_sigma_deg=DEFAULTS['femur_sigma_deg']):
    """One draw: {'rot_deg' [3], 'trans_mm' [3] (camera frame), 'femur_deg' [2, 3] (left, right)}; 12 normals."""
    z = rng.standard_normal(12)
    ts = np.asarray(trans_sigma_mm, np.float64).reshape(3)
    return {'rot_deg': z[0:3] * float(rot_sigma_deg), 'trans_mm': z[3:6] * ts, 'femur_deg': z[6:12].reshape(2, 3) * float(femur_sigma_deg)}


def apply_motion(poses, E, lands3d, motion):
    """The seed poses {name: P} under one draw: {name: P''} (module docstring)."""
    P = {k: np.asarray(poses[k], np.float64).reshape(4, 4) for k in drr.POSES}
    E = np.asarray(E, np.float64).reshape(4, 4)
    pts = np.array([np.asarray(v, np.float64).reshape(-1)[:3] for v in lands3d.values()]).reshape(-1, 3)
    c_w = (np.linalg.inv(P[drr.POSES[0]]) @ np.append(pts.mean(0), 1.0))[:3]
    theta = np.concatenate([np.radians(motion['rot_deg']), E[:3, :3].T @ np.asarray(motion['trans_mm'], np.float64)])
    back = np.linalg.inv(register.pose_delta(theta, c_w, 1.0))
    out = {k: P[k] @ back for k in drr.POSES}
    for side, name in enumerate(FEMUR_HEADS):
        if name in lands3d:
            fh = np.asarray(lands3d[name], np.float64).reshape(-1)[:3]
            A = register.pose_delta(np.concatenate([np.radians(motion['femur_deg'][side]), np.zeros(3)]), fh, 1.0)
            out[drr.POSES[1 + side]] = A @ out[drr.POSES[1 + side]]
    return out


def lands_in_window(K, E, P_pelvis, lands3d, rows, cols, crop):
    """How many 3D landmarks project inside the crop window under the pelvis pose."""
    uv = drr.project(K, E, P_pelvis, [np.asarray(v, np.float64).reshape(-1)[:3] for v in lands3d.values()])
    ok = (uv[0] >= crop) & (uv[0] <= cols - 1 - crop) & (uv[1] >= crop) & (uv[1] <= rows - 1 - crop) & np.isfinite(uv).all(0)
    return int(ok.sum())


def fov_flags(K, E, poses, lands3d, rows, cols, seed_flags=(0, 0)):
    """(left, right): 1 when the femoral head projects inside the detector under that femur's pose."""
    out = []
    for side, name in enumerate(FEMUR_HEADS):
        if name not in lands3d:
            out.append(int(seed_flags[side]))
            continue
        uv = drr.project(K, E, poses[drr.POSES[1 + side]], np.asarray(lands3d[name], np.float64).reshape(-1)[:3])[:, 0]
        out.append(int(0 <= uv[0] <= cols - 1 and 0 <= uv[1] <= rows - 1))
    return tuple(out)


def sample_pose(rng, poses, K, E, lands3d, rows, cols, crop, specimen='?', rot_sigma_deg=DEFAULTS['rot_sigma_deg'],
                trans_sigma_mm=DEFAULTS['trans_sigma_mm'], femur_sigma_deg=DEFAULTS['femur_sigma_deg'],
                min_lands=DEFAULTS['min_lands'], max_draws=MAX_DRAWS):
    """({name: P''}, number of draws): draws until at least min_lands landmarks lie in the crop window; after max_draws
    rejected draws raises, naming the specimen."""
    if not lands3d:
        raise nat.DflError('synth: specimen %s has no 3D landmarks' % specimen)
    for n in range(1, int(max_draws) + 1):
        new = apply_motion(poses, E, lands3d, draw_motion(rng, rot_sigma_deg, trans_sigma_mm, femur_sigma_deg))
        if lands_in_window(K, E, new[drr.POSES[0]], lands3d, rows, cols, crop) >= int(min_lands):
            return new, n
    raise nat.DflError('synth: specimen %s: %d draws in a row left fewer than %d landmarks inside the crop window (smaller '
                       'sigmas, a smaller crop or min_lands would help)' % (specimen, int(max_draws), int(min_lands)))


def sample_poses(seed, specimen_index, specimen, seeds, views, K, E, lands3d, rows, cols, crop, **kw):
    """[({name: P''}, index of the seed projection, draws)] for synthetic views 0..views-1 of one specimen; `seeds` is
    the list of the acquired projections' {name: P}."""
    rng = np.random.default_rng([int(seed), int(specimen_index)])
    out = []
    for n in range(int(views)):
        s = n % len(seeds)
        new, draws = sample_pose(rng, seeds[s], K, E, lands3d, rows, cols, crop, specimen, **kw)
        out.append((new, s, draws))
    return out


def tool_rng(seed, specimen_index, view):
    """The stream the tools of one synthetic view are drawn from: apart from the pose stream [seed, specimen index]."""
    return np.random.default_rng([int(seed), int(specimen_index), 1, int(view)])


# ---- the pipeline ------------------------------------------------------------------------------------------------------
def _copy(src, out, path, to=None):
    """Copy group or dataset `path` of an open h5lite file into the writer (at `to`), as it is stored."""
    node, to = src[path], to or path
    if isinstance(node, h5lite.Group):
        out.create_group(to)
        for k in node.keys():
            _copy(src, out, path.rstrip('/') + '/' + k, to.rstrip('/') + '/' + k)
        return
    v = node[()]
    if isinstance(v, (bytes, str)):
        out[to] = v
    elif np.asarray(v).dtype.kind in 'iuf':
        out[to] = np.asarray(v)
    else:
        out.create_dataset(to, data=np.asarray(v), dtype=np.asarray(v).dtype)


def synthesize(src, dst, views, seed=0, layout='preprocessed', specimens=None, crop=50, factor=8,
               rot_sigma_deg=DEFAULTS['rot_sigma_deg'], trans_sigma_mm=DEFAULTS['trans_sigma_mm'],
               femur_sigma_deg=DEFAULTS['femur_sigma_deg'], min_lands=DEFAULTS['min_lands'], photons=DEFAULTS['photons'],
               gain=DEFAULTS['gain'], electronic_sigma=DEFAULTS['electronic_sigma'], blur_sigma_px=DEFAULTS['blur_sigma_px'],
               noise=True, bones_only=False, volumes=True, chunk=8, compression=None, device=None, report=None, tools=0,
               tool_options=None, tool_mask=False):
    """A file of `views` synthetic projections per specimen from the full-resolution file `src` (its CT, 3D annotation,
    3D landmarks, projection parameters and acquired poses).  layout 'full-res' writes the reference's full-resolution
    layout (volumes=False leaves out 'vol' and 'vol-seg'); 'preprocessed' the training file that
    preprocess.convert_file(crop, factor) makes of it, without the detour.  crop also bounds the acceptance window;
    factor is used by 'preprocessed' only.  tools > 0 adds up to that many capsules per view (tools.sample_tools with the
    keyword arguments tool_options); 'full-res' then also writes 'projections/NNN/tools/capsules' (float64 [n, 8]: a, b, r,
    mu; views that drew a capsule) and, with tool_mask, 'projections/NNN/tools/mask/pixels' (uint8, 1 where a ray crosses a
    tool; every view); 'preprocessed' keeps its datasets: the tools are in the pixels and nowhere else.
    Returns [(specimen id, index, views, rejected draws)]; report(line) gets one line per specimen."""
    if layout not in ('full-res', 'preprocessed'):
        raise nat.DflError("synth.synthesize: layout must be 'full-res' or 'preprocessed', got %r" % (layout,))
    tools, tool_options = int(tools), dict(tool_options or {})
    if not 0 <= tools <= nat.TOOLS_MAX:
        raise nat.DflError('synth.synthesize: tools must be 0..%d per view, got %d' % (nat.TOOLS_MAX, tools))
    unknown = sorted(set(tool_options) - set(tools_mod.TOOL_DEFAULTS))
    if unknown:
        raise nat.DflError('synth.synthesize: unknown tool option %s (known: %s)' % (', '.join(unknown), ', '.join(sorted(tools_mod.TOOL_DEFAULTS))))
    if not torch.cuda.is_available():
        raise nat.DflError('synth.synthesize: no GPU visible (the renderer and the detector model are HIP kernels; no CPU path)')
    if int(views) < 1 or int(chunk) < 1:
        raise nat.DflError('synth.synthesize: views and chunk must be at least 1')
    gaussian_taps(blur_sigma_px)
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    views, chunk, pre = int(views), int(chunk), layout == 'preprocessed'
    kw_pose = dict(rot_sigma_deg=rot_sigma_deg, trans_sigma_mm=trans_sigma_mm, femur_sigma_deg=femur_sigma_deg, min_lands=min_lands)
    f = fullres.Source(src)
    try:
        if not pre and f.h5 is None:
            raise nat.DflError("synth.synthesize: layout 'full-res' copies groups as they are stored and needs an HDF5 source, not .npz")
        K, E, R, Cn = fullres.proj_params(f)
        Ro, Co = preprocess.out_size(R, Cn, crop, factor if pre else 1)
        specimens = fullres.specimens(f, specimens, 'synth.synthesize: %s' % src)
        lands3d = {s: fullres.volume_landmarks(f, s) for s in specimens}
        land_names = preprocess.land_order(set().union(*[set(v) for v in lands3d.values()]))
        if pre:
            for s in specimens:
                lack = [n for n in land_names if n not in lands3d[s]]
                if lack:
                    raise nat.DflError('synth.synthesize: specimen %s has no landmark %s' % (s, ', '.join(lack)))
        grid = drr.Grid(-np.linalg.inv(K), R, Cn)                          # the full detector grid: G = identity
        kw_img = dict(compression='gzip', chunks=(R, Cn)) if compression else {}      # one chunk per image
        done = []
        out = h5lite.File(dst, 'w')
        try:
            if pre:
                preprocess.write_land_names(out, land_names)
            else:
                _copy(f.h5, out, 'proj-params')
            for k, s in enumerate(specimens):
                acquired = fullres.n_projections(f, s)
                if acquired < 1:
                    raise nat.DflError('synth.synthesize: specimen %s has no acquired projection to start from' % s)
                seeds = [dict(poses=fullres.gt_poses(f, pfx), rot=int(fullres.rot180(f, pfx)), fov=fullres.femur_fov(f, pfx, default=0),
                              pfx=pfx) for pfx in (fullres.projection_prefix(s, p) for p in range(acquired))]
                plan = sample_poses(seed, k, s, [sd['poses'] for sd in seeds], views, K, E, lands3d[s], R, Cn, crop, **kw_pose)
                I2P = drr.inds_to_phys(*fullres.volume_frame(f, s))
                volume = drr.read_volume(f, s, dev, cast_labels=True)
                names = list(lands3d[s]) if not pre else land_names
                pts = np.array([lands3d[s][n] for n in names]).reshape(-1, 3)
                if pre:
                    grp, d_projs, d_segs = preprocess.create_specimen(out, k + 1, views, Ro, Co, compression)
                    lands2d = np.zeros((views, 2, len(names)), np.float64)
                else:
                    for g in (('/vol', '/vol-seg') if volumes else ()) + ('/vol-landmarks',):
                        _copy(f.h5, out, s + g)
                for n0 in range(0, views, chunk):
                    part = plan[n0:n0 + chunk]
                    objs = [drr.default_objects(E, poses, I2P, bones_only) for poses, _, _ in part]
                    att, _, lab = drr.render(volume, objs, grid, interp='exact', want_plen=False, want_labels=True, tight_boxes=True)
                    caps, tlen = [[] for _ in part], None
                    if tools > 0:
                        caps = [tools_mod.sample_tools(tool_rng(seed, k, n0 + j), tools_mod.lands_in_camera(E, poses[drr.POSES[0]], lands3d[s]),
                                                       tools, **tool_options) for j, (poses, _, _) in enumerate(part)]
                        tlen = tools_mod.add_tools(att, grid, caps, want_len=tool_mask and not pre)
                    keys = [noise_keys(seed, k, n0 + j) for j in range(len(part))]
                    img = expose(att, photons, gain, electronic_sigma, blur_sigma_px, keys_q=[q for q, _ in keys] if noise else None,
                                 keys_e=[e for _, e in keys] if noise else None, u16=True)
                    rots = [seeds[sd]['rot'] for _, sd, _ in part]
                    uv = [drr.project(K, E, poses[drr.POSES[0]], pts) for poses, _, _ in part]
                    if pre:
                        d_projs[n0:n0 + len(part)] = preprocess.preprocess_projs(img, rots, crop, factor).cpu().numpy()
                        d_segs[n0:n0 + len(part)] = preprocess.preprocess_segs(lab, rots, crop, factor).cpu().numpy()
                        lands2d[n0:n0 + len(part)] = np.stack(uv)
                        continue
                    img, lab = img.cpu().numpy(), lab.cpu().numpy()
                    mask = None if tlen is None else (tlen > 0).to(torch.uint8).cpu().numpy()
                    for j, (poses, sd, _) in enumerate(part):
                        pfx, spfx = fullres.projection_prefix(s, n0 + j), seeds[sd]['pfx']
                        out.create_dataset(pfx + 'image/pixels', data=img[j], dtype=np.uint16, **kw_img)
                        out.create_dataset(pfx + 'gt-seg/pixels', data=lab[j], dtype=np.uint8, **kw_img)
                        for g in ('image/', 'gt-seg/'):
                            for item in ('dir-mat', 'origin', 'spacing'):
                                if item in f.children(spfx + g):
                                    _copy(f.h5, out, spfx + g + item, pfx + g + item)
                        for l, name in enumerate(names):
                            out[pfx + 'gt-landmarks/' + name] = uv[j][:, l].reshape(2, 1)
                        for name in drr.POSES:
                            out[pfx + 'gt-poses/' + name] = poses[name]
                        for side, flag in zip(('left', 'right'), fov_flags(K, E, poses, lands3d[s], R, Cn, seeds[sd]['fov'])):
                            out[pfx + 'gt-poses/%s-femur-good-fov' % side] = np.int64(flag)
                        out[pfx + 'rot-180-for-up'] = np.int64(seeds[sd]['rot'])
                        if caps[j]:
                            out[pfx + 'tools/capsules'] = np.stack([cap.row() for cap in caps[j]])
                        if mask is not None:
                            out.create_dataset(pfx + 'tools/mask/pixels', data=mask[j], dtype=np.uint8, **kw_img)
                if pre:
                    out[grp + '/lands'] = preprocess.map_lands(lands2d, [seeds[sd]['rot'] for _, sd, _ in plan], R, Cn, crop,
                                                               factor).astype(np.float32)
                rejected = sum(d - 1 for _, _, d in plan)
                done.append((s, k + 1, views, rejected))
                if report is not None:
                    where = '%02d' % (k + 1) if pre else s
                    size = '%d x %d' % ((Ro, Co) if pre else (R, Cn))
                    report('%s -> %s: %d synthetic projections from %d acquired, %s, %d draws rejected'
                           % (s, where, views, acquired, size, rejected))
                del volume
        finally:
            out.close()
    finally:
        f.close()
    return done
