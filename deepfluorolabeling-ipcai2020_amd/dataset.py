"""GPU-resident counterpart of the reference loader (train_test_code/dataset.py), deterministic part only.

The reference's ``RandomDataAugDataSet.__getitem__`` (dataset.py:98-328) reflect-pads and standardises the projection,
synthesises L Gaussian heat maps and returns float one-hot masks -- on the host, per item, every step; train.py then
copies the float tensors to the GPU (train.py:395-403: 45 MB per batch-16 step).  Here the RAW arrays (fp32
projections, uint8 labels, 2xL landmark coordinates) live in HBM and ``dfl_prep_batch`` builds a whole batch of
network inputs and targets in two launches.  Same item protocol -- ``ds[i]`` and the batches of
``ds.batches(...)`` are the tuples ``(proj, mask, lands, heat)`` train.py:393 unpacks -- so the training loop is
unchanged.  Random augmentation (dataset.py:107-283) runs on the device too: ``DeviceAugment`` draws the per-item
parameters on the host and ``dfl_augment_batch`` does the per-pixel work.
"""
import math
import random

import numpy as np
import torch

from . import _native as nat


def calc_pad_amount(padded_dim, cur_dim):
    """dataset.py:26-40 -- odd differences round up."""
    assert padded_dim > cur_dim
    pad = (padded_dim - cur_dim) / 2
    return int(pad) + 1 if pad != int(pad) else int(pad)


def affine_inverse_map(center, angle, translate, scale, shear):
    """torchvision's _get_inverse_affine_matrix: the inverse of T(translate) C RSS C^-1 (RSS = rotation by angle degrees
    with x / y shear in degrees, times scale; C = translation by center) as the 6 coefficients of the source point."""
    rot, sx, sy = math.radians(angle), math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [v / scale for v in (d, -b, 0.0, -c, a, 0.0)]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty) + cx
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty) + cy
    return m


class DeviceAugment:
    """The reference's random augmentation (dataset.py:107-283) with parameters drawn here and pixels done on the device.

    Per item of the training set, with probability ``prob``: invert (p 0.5), noise sigma ~ U(0.005, 0.01), gamma ~
    U(0.7, 1.3), affine (rotation ~ U(-5, 5) degrees, translation = uniform direction x U(0, 1) x 20 px, scale ~
    U(0.9, 1.1), shear ~ U(-1, 1) degrees on each axis), erase (p 0.25: 1..5 boxes, sides round(N(0,1) 0.15 n + 0.15 n)
    rejection-sampled into (0, n], corners uniform), plus a 64-bit noise key per item and per box.

    The draws of an epoch come from ``numpy.random.Generator(SeedSequence((seed, epoch, rank)))`` in dataset-index order,
    so an item's augmentation depends on (seed, epoch, rank, index) only -- not on the shuffle, the batch size or where a
    run was resumed.  Call ``set_epoch(e)`` at the start of every epoch (as with DistributedSampler): without it every
    epoch repeats epoch 0's draws.

    ``land_rule``: 'reference' drops (sets to inf) an augmented landmark by the test of dataset.py:245-247 as written
    (its ``orig_s_shape`` is the (C, H, W) one-hot shape: x < 0, x > H-1, y < 0, y < C-1); 'in_view' by the intended test
    (outside [0, W-1] x [0, H-1]).  Either way every finite landmark gets a heat map (dataset.py:313)."""

    RULES = {'reference': nat.AUG_LANDS_REFERENCE, 'in_view': nat.AUG_LANDS_IN_VIEW}

    def __init__(self, seed, prob=0.5, land_rule='reference', rank=0):
        if land_rule not in self.RULES:
            raise ValueError("land_rule must be 'reference' or 'in_view'")
        if not 0.0 <= prob <= 1.0:
            raise ValueError('prob must lie in [0, 1]')
        self.seed, self.prob, self.land_rule, self.rank = int(seed), float(prob), land_rule, int(rank)
        self.set_epoch(0)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)
        self._drawn = None

    def __repr__(self):
        return 'DeviceAugment(seed={}, prob={}, land_rule={!r}, rank={})'.format(self.seed, self.prob, self.land_rule, self.rank)

    def draw(self, n, H, W):
        """This epoch's parameters of the items 0..n-1 of an (H x W, after the loader's pad) training set: a list with
        None for the items left alone and a dict for the augmented ones (flags, sigma, gamma, angle, translate, scale,
        shear, noise_key, boxes [(row, col, rows, cols, key)])."""
        rng = np.random.default_rng(np.random.SeedSequence((self.seed, self.epoch, self.rank)))
        aug = rng.random(n) < self.prob
        inv = rng.random(n) < 0.5
        sigma = rng.uniform(0.005, 0.01, n)
        gamma = rng.uniform(0.7, 1.3, n)
        direction = rng.standard_normal((n, 2))
        mag = rng.random(n) * 20.0
        angle = rng.uniform(-5.0, 5.0, n)
        shear = rng.uniform(-1.0, 1.0, (n, 2))
        scale = rng.uniform(0.9, 1.1, n)
        erase = rng.random(n) < 0.25
        nbox = rng.integers(1, 6, n)
        keys = rng.integers(0, 1 << 64, (n, 6), dtype=np.uint64, endpoint=False)
        mean = np.array([H * 0.15, W * 0.15], np.float32)
        out = []
        for i in range(n):
            if not aug[i]:
                out.append(None)
                continue
            t = direction[i] / np.linalg.norm(direction[i]) * mag[i]
            flags = nat.AUG_NOISE | nat.AUG_GAMMA | (nat.AUG_INVERT if inv[i] else 0) | (nat.AUG_ERASE if erase[i] else 0)
            boxes = []
            if erase[i]:
                for b in range(int(nbox[i])):
                    while True:
                        dims = np.round(rng.standard_normal(2).astype(np.float32) * mean + mean).astype(np.int64)
                        if 0 < dims[0] <= H and 0 < dims[1] <= W:
                            break
                    r0 = int(rng.integers(0, H - dims[0], endpoint=True))
                    c0 = int(rng.integers(0, W - dims[1], endpoint=True))
                    boxes.append((r0, c0, int(dims[0]), int(dims[1]), int(keys[i, 1 + b])))
            out.append(dict(flags=flags, sigma=float(sigma[i]), gamma=float(gamma[i]), angle=float(angle[i]),
                            translate=(float(t[0]), float(t[1])), scale=float(scale[i]),
                            shear=(float(shear[i, 0]), float(shear[i, 1])), noise_key=int(keys[i, 0]), boxes=boxes))
        return out

    def params(self, indices, n, H, W):
        """Parameters of the dataset items ``indices`` (of n) for this epoch (drawn once per epoch)."""
        if self._drawn is None or self._drawn[0] != (n, H, W):
            self._drawn = ((n, H, W), self.draw(n, H, W))
        return [self._drawn[1][i] for i in indices]

    @staticmethod
    def item(prm, row, H, W, pad, has_seg):
        """The dfl_augment_item of one augmented item: the PIL inverse maps of the projection's and the labels' padded
        frames (centred at width / 2, height / 2, torchvision's PIL path) and the forward landmark map (centre
        (shape[-2] / 2 + 0.5, shape[-1] / 2 + 0.5) of the label map, dataset.py:209-219)."""
        ch, cw = (H + 1) // 2, (W + 1) // 2
        args = (prm['angle'], prm['translate'], prm['scale'], prm['shear'])
        it = nat.AugmentItem()
        it.img_map[:] = affine_inverse_map(((W + 2 * (cw + pad)) * 0.5, (H + 2 * (ch + pad)) * 0.5), *args)
        it.seg_map[:] = affine_inverse_map(((W + 2 * cw) * 0.5, (H + 2 * ch) * 0.5), *args)
        sh = (H, W) if has_seg else (H + 2 * pad, W + 2 * pad)
        a = affine_inverse_map((sh[0] / 2.0 + 0.5, sh[1] / 2.0 + 0.5), *args)
        it.land_map[:] = [float(v) for v in np.linalg.inv(np.array([a[0:3], a[3:6], [0.0, 0.0, 1.0]]))[:2].reshape(-1)]
        it.noise_key = prm['noise_key']
        boxes = prm['boxes']
        if len(boxes) > 5:
            raise ValueError('at most 5 erase boxes per item')
        for b, (r0, c0, nr, nc, key) in enumerate(boxes):
            if not (0 <= r0 and 0 < nr and r0 + nr <= H + 2 * pad and 0 <= c0 and 0 < nc and c0 + nc <= W + 2 * pad):
                raise ValueError('erase box outside the image')
            it.box[b][:] = (r0, c0, nr, nc)
            it.box_key[b] = key
        it.n_box = len(boxes)
        it.noise_sigma, it.gamma = prm['sigma'], prm['gamma']
        it.row, it.flags = row, prm['flags']
        return it


class DeviceDataSet(torch.utils.data.Dataset):
    """projs [N,1,H,W] fp32, segs [N,H,W] integer labels (or [N,C,H,W] one-hot, converted), lands [N,2,L] (row 0 = x)."""

    def __init__(self, projs, segs, lands=None, proj_pad_dim=0, num_classes=None, device=None, sigma=2.5):
        dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        if dev.type != 'cuda':
            raise nat.DflError('dataset.DeviceDataSet builds its batches with dfl_prep_batch on the GPU (no CPU path)')
        projs = torch.as_tensor(projs)
        assert projs.dim() == 4 and projs.shape[1] == 1
        self.projs = projs.to(dev, torch.float32).contiguous()
        N, _, H, W = projs.shape
        self.segs = None
        self.num_classes = num_classes
        if segs is not None:
            segs = torch.as_tensor(segs)
            if segs.dim() == 4:                      # the reference keeps float one-hot masks; labels are 1 byte per pixel
                self.num_classes = segs.shape[1]
                segs = segs.argmax(dim=1)
            assert segs.shape == (N, H, W)
            assert self.num_classes is not None and 0 < self.num_classes <= 255
            self.segs = segs.to(dev, torch.uint8).contiguous()
        self.lands = None
        if lands is not None:
            lands = torch.as_tensor(lands)
            assert lands.shape[0] == N and lands.shape[1] == 2
            self.lands = lands.to(dev, torch.float32).contiguous()
        self.extra_pad = calc_pad_amount(proj_pad_dim, W) if proj_pad_dim > 0 else 0
        self.do_norm_01_scale = True
        self.include_heat_map = self.lands is not None
        self.heat_sigma = float(sigma)
        self.prob_of_aug = 0.0
        self.augment = None             # a DeviceAugment: random augmentation of every item this dataset prepares
        self.dev = dev
        self._lib = nat.lib()
        self._scratch = {}

    def __len__(self):
        return self.projs.shape[0]

    def _prepare(self, idx, aug_params=None, probe=None):
        if self.prob_of_aug > 0 and self.augment is None:
            raise NotImplementedError('prob_of_aug > 0: set dataset.augment = DeviceAugment(seed) instead (the draws and '
                                      'the probability are its own)')
        index_list = [int(i) for i in idx]
        idx = torch.as_tensor(index_list, dtype=torch.long, device=self.dev)
        B = int(idx.numel())
        _, _, H, W = self.projs.shape
        p = self.extra_pad
        raw = self.projs.index_select(0, idx)
        x = torch.empty((B, 1, H + 2 * p, W + 2 * p), dtype=torch.float32, device=self.dev)
        a = nat.PrepArgs(proj=raw.data_ptr(), x=x.data_ptr(), B=B, H=H, W=W, pad=p, standardize=int(self.do_norm_01_scale),
                         sigma=self.heat_sigma)
        keep = [raw]
        masks = lands = heats = None
        if self.segs is not None:
            lab = self.segs.index_select(0, idx)
            masks = torch.empty((B, self.num_classes, H, W), dtype=torch.float32, device=self.dev)
            a.labels, a.masks, a.C = lab.data_ptr(), masks.data_ptr(), self.num_classes
            keep.append(lab)
        if self.lands is not None:
            lands = self.lands.index_select(0, idx)
            if self.include_heat_map:
                L = lands.shape[-1]
                heats = torch.empty((B, L, 1, H, W), dtype=torch.float32, device=self.dev)
                a.lands, a.heats, a.L = lands.data_ptr(), heats.data_ptr(), L
        sc = self._scratch.get(B)
        if sc is None:
            sc = self._scratch[B] = torch.empty(self._lib.dfl_prep_scratch_doubles(B), dtype=torch.float64, device=self.dev)
        a.scratch = sc.data_ptr()
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        nat.call('dfl_prep_batch', a, stream)
        if self.augment is not None or aug_params is not None:
            lands = self._augment(index_list, aug_params, raw, x, masks, lands, heats, stream, probe)
        return x, masks, lands, heats

    def _augment(self, index_list, aug_params, raw, x, masks, lands, heats, stream, probe=None):
        """dfl_augment_batch over the rows whose item is augmented (the others keep dfl_prep_batch's output).
        aug_params: explicit per-row parameters (DeviceAugment.draw's form) instead of the sampler's.  probe: a dict that
        receives 'rows', the warped 8-bit 'levels' and the 'noise' normals of the augmented rows (tests)."""
        _, _, H, W = self.projs.shape
        p = self.extra_pad
        if aug_params is None:
            aug_params = self.augment.params(index_list, len(self), H + 2 * p, W + 2 * p)
        rows = [(r, prm) for r, prm in enumerate(aug_params) if prm is not None]
        if not rows:
            return lands
        B = len(index_list)
        table = (nat.AugmentItem * len(rows))(*[DeviceAugment.item(prm, r, H, W, p, self.segs is not None) for r, prm in rows])
        host = torch.frombuffer(bytearray(table), dtype=torch.uint8).pin_memory()
        items = torch.empty(host.numel(), dtype=torch.uint8, device=self.dev)
        items.copy_(host, non_blocking=True)
        rule = self.augment.land_rule if self.augment is not None else 'reference'
        a = nat.AugmentArgs(proj=raw.data_ptr(), x=x.data_ptr(), items=items.data_ptr(), n_items=len(rows), B=B, H=H, W=W,
                            pad=p, standardize=int(self.do_norm_01_scale), sigma=self.heat_sigma,
                            land_rule=DeviceAugment.RULES[rule] if self.segs is not None else nat.AUG_LANDS_NONE)
        keep = [host, items]
        if masks is not None:
            lab = self.segs.index_select(0, torch.as_tensor(index_list, dtype=torch.long, device=self.dev))
            a.labels, a.masks, a.C = lab.data_ptr(), masks.data_ptr(), self.num_classes
            keep.append(lab)
        elif self.num_classes is not None:
            a.C = self.num_classes
        if lands is not None:
            out = lands.clone()
            a.lands, a.lands_out, a.L = lands.data_ptr(), out.data_ptr(), lands.shape[-1]
            if heats is not None:
                a.heats = heats.data_ptr()
            keep.append(lands)
            lands = out
        nbytes = int(self._lib.dfl_augment_scratch_bytes(B, H, W, p))
        sc = self._scratch.get(('aug', B))
        if sc is None:
            sc = self._scratch[('aug', B)] = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        a.scratch = sc.data_ptr()
        if probe is not None:
            probe['rows'] = [r for r, _ in rows]
            probe['levels'] = torch.zeros((len(rows), H + 2 * p, W + 2 * p), dtype=torch.uint8, device=self.dev)
            probe['noise'] = torch.zeros((len(rows), H, W), dtype=torch.float32, device=self.dev)
            a.levels, a.noise = probe['levels'].data_ptr(), probe['noise'].data_ptr()
        nat.call('dfl_augment_batch', a, stream)
        return lands

    def __getitem__(self, i):
        x, masks, lands, heats = self._prepare([int(i)])
        return (x[0], masks[0] if masks is not None else None, lands[0] if lands is not None else None,
                heats[0] if heats is not None else None)

    def batches(self, batch_size, shuffle=False, drop_last=False, shard=None):
        """What ``DataLoader(ds, batch_size, shuffle)`` yields for the reference's dataset (train.py:365-372), already on
        the GPU.  Data parallel: ``shard=(rank, world)`` -- every rank must draw the SAME permutation (same ``random``
        seed); a step's global minibatch is ``batch_size * world`` consecutive entries of it and rank r takes the r-th
        contiguous slice of ``batch_size``.  A ragged tail is cut into equal non-empty slices (both losses
        are means over images, so equal shards keep mean-of-means exact); what does not divide is left out this epoch."""
        order = list(range(len(self)))
        if shuffle:
            random.shuffle(order)
        rank, world = shard if shard is not None else (0, 1)
        step = batch_size * world
        for s in range(0, len(order), step):
            glob = order[s:s + step]
            if len(glob) < step and drop_last:
                break
            per = batch_size if len(glob) == step else len(glob) // world
            if per == 0:
                break
            yield self._prepare(glob[rank * per:(rank + 1) * per])


RandomDataAugDataSet = DeviceDataSet      # the reference's class name (dataset.py:42)


def _open_container(path):
    """name -> array view of the preprocessed container: the reference's HDF5 layout (hdf5_layouts/Readme.md:105-117:
    '<pat>/projs', '<pat>/segs', '<pat>/lands', 'land-names/num-lands'), read with the dependency-free reader of
    h5lite.py (h5py is absent from the build and GPU images; when it IS installed it takes the files whose HDF5 features
    h5lite refuses), or an .npz with the same names (slashes kept)."""
    if str(path).endswith('.npz'):
        z = np.load(path)
        return (lambda k: z[k]), (lambda: None)
    from . import h5lite
    try:
        f = h5lite.File(path, 'r')
        f.keys()
    except h5lite.H5Error as e:
        try:
            import h5py
        except ImportError:
            raise e
        f = h5py.File(path, 'r')
    return (lambda k: f[k][()]), f.close


def get_num_lands_from_dataset(h5_file_path):
    """dataset.py:339-346."""
    get, close = _open_container(h5_file_path)
    n = int(get('land-names/num-lands'))
    close()
    return n


def get_land_names_from_dataset(h5_file_path):
    """dataset.py:348-365: the strings 'land-names/land-XX' (bytes or str in the file)."""
    get, close = _open_container(h5_file_path)
    names = []
    for l in range(int(get('land-names/num-lands'))):
        s = get('land-names/land-{:02d}'.format(l))
        if isinstance(s, np.ndarray):
            s = s.item() if s.ndim == 0 else s.tobytes()
        if isinstance(s, (bytes, np.bytes_)):
            s = s.decode()
        assert isinstance(s, str)
        names.append(s)
    close()
    return names


class NpzFile:
    """Write side of the container for hosts without h5py: the few methods of an ``h5py.File`` opened for writing that
    test_ensemble.py / util.seg_dataset* use (create_group, item assignment, create_dataset with the chunking /
    compression keywords accepted and ignored, flush, close), collected in memory and written as ONE compressed .npz with
    the same dataset names (slashes kept) on close()."""

    class _Group:
        def __init__(self, owner, prefix):
            self._o, self._p = owner, prefix

        def __setitem__(self, k, v):
            self._o._d[self._p + '/' + k] = np.asarray(v)

        def create_dataset(self, name, shape, dtype='f4', **kw):
            return self._o.create_dataset(self._p + '/' + name, shape, dtype=dtype, **kw)

    def __init__(self, path, mode='w'):
        assert mode == 'w', 'NpzFile is the write side; dataset._open_container reads'
        self._path, self._d, self._closed = path, {}, False

    def create_group(self, name):
        return NpzFile._Group(self, name)

    def __setitem__(self, k, v):
        self._d[k] = np.asarray(v)

    def create_dataset(self, name, shape, dtype='f4', **kw):
        self._d[name] = np.zeros(shape, dtype=np.dtype(dtype))
        return self._d[name]

    def flush(self):
        pass

    def close(self):
        if not self._closed:
            with open(self._path, 'wb') as f:          # (np.savez would append '.npz' to a bare path)
                np.savez_compressed(f, **self._d)
            self._closed = True


def open_output_container(path):
    """The reference writes its results with ``h5.File(path, 'w')`` (test_ensemble.py:121): here the same calls go to
    h5lite.File (HDF5 written without h5py: chunked + gzip datasets streamed chunk by chunk, readable by h5py / h5dump);
    a path ending in .npz gets an NpzFile with the same dataset names."""
    if str(path).endswith('.npz'):
        return NpzFile(path)
    from . import h5lite
    return h5lite.File(path, 'w')


def get_dataset(h5_file_path, pat_inds, num_classes, pad_img_dim=0, no_seg=False, minmax=None, data_aug=False,
                train_valid_split=None, train_valid_idx=None, dup_data_w_left_right_flip=False, device=None, augment=None):
    """dataset.py:367-555: concatenates the patients' arrays, marks out-of-view landmarks with inf (:421-429), optional
    min/max scaling (:384-395, :513-516), optional train/validation split (:524-551).  ``augment`` (a DeviceAugment)
    augments the training set -- the whole set without a split, never the validation part (:546-549)."""
    if data_aug:
        raise NotImplementedError('data_aug=True promises the reference\'s host-side random stream, which is not reproduced: '
                                  'pass augment=DeviceAugment(seed) for the same augmentation on the device (DESIGN.md section 9)')
    if augment is not None and not isinstance(augment, DeviceAugment):
        raise TypeError('augment must be a DeviceAugment')
    if dup_data_w_left_right_flip:
        raise NotImplementedError('dup_data_w_left_right_flip is not implemented (no reference CLI default selects it)')
    get, close = _open_container(h5_file_path)
    projs, segs, lands = [], [], []
    for pat_idx in pat_inds:
        g = '{:02d}'.format(pat_idx)
        p = np.asarray(get(g + '/projs'), dtype=np.float32)
        assert p.ndim == 3
        projs.append(p)
        if not no_seg:
            segs.append(np.asarray(get(g + '/segs')))
        lands.append(np.asarray(get(g + '/lands'), dtype=np.float32))
    close()
    projs = torch.from_numpy(np.concatenate(projs))
    H, W = projs.shape[-2:]
    lands = torch.from_numpy(np.concatenate(lands))
    assert torch.all(torch.isfinite(lands))
    x, y = lands[:, 0], lands[:, 1]
    oob = (x < 0) | (x > W - 1) | (y < 0) | (y > H - 1)
    x[oob] = math.inf
    y[oob] = math.inf
    segs = torch.from_numpy(np.concatenate(segs)) if segs else None
    scaled = None
    if minmax is not None and minmax is not False:
        lo, hi = (float(projs.min()), float(projs.max())) if minmax is True else (float(minmax[0]), float(minmax[1]))
        assert hi - lo > 1.0e-6
        projs = (projs - lo) / (hi - lo)
        scaled = (lo, hi)
    projs = projs.unsqueeze(1)

    def make(sel):
        ds = DeviceDataSet(projs[sel] if sel is not None else projs,
                           None if segs is None else (segs[sel] if sel is not None else segs),
                           lands[sel] if sel is not None else lands, proj_pad_dim=pad_img_dim, num_classes=num_classes,
                           device=device)
        ds.rob_orig_img_shape = (H, W)
        ds.rob_data_is_scaled = scaled is not None
        if scaled is not None:
            ds.rob_minmax = scaled
        return ds

    if train_valid_split is not None and train_valid_split > 0:
        assert 0.0 < train_valid_split < 1.0
        n = projs.shape[0]
        num_train = int(math.ceil(train_valid_split * n))
        inds = list(range(n))
        if train_valid_idx is None or train_valid_idx[0] is None or train_valid_idx[1] is None:
            random.shuffle(inds)
            train_inds, valid_inds = inds[:num_train], inds[num_train:]
        else:
            train_inds, valid_inds = train_valid_idx
            assert len(train_inds) == num_train and len(valid_inds) == n - num_train
        train_ds = make(train_inds)
        train_ds.augment = augment
        return train_ds, make(valid_inds), train_inds, valid_inds
    ds = make(None)
    ds.augment = augment
    return ds
