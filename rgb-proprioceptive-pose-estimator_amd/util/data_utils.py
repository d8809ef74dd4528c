"""Batch layout and device staging for the train step.

The reference's MultiEpisodeDataset (util/data_utils.py:10-204) steps a Robosuite/MuJoCo simulator to
produce episodes; that simulator and its CPU image preprocessing are out of scope (SURVEY.md section 2,
row 7).  What the train step depends on is kept: the time-major layout (`__getitem__(t)` returns all
episodes at timestep t, util/data_utils.py:62-73), the 6-tuple, `refresh_data`, `env.horizon`, and
`standardize_quat`.  SyntheticEpisodeDataset fills the same tensors with seeded Robosuite-shaped data
(ImageNet-normalised uint8 noise images, workspace-bounded positions, unit quaternions with w >= 0,
proprioception = truth + N(0, noise_scale I) with the quaternion renormalised, util/data_utils.py:162-176),
generated directly in HBM.  RecordedEpisodeDataset reads episodes recorded from the simulator elsewhere back from a file, raw, and
leaves every image transform to the device; ResidentEpisodeDataset keeps that file in HBM and WindowSampler draws shuffled minibatches
from it on the device.  FrameAugment, DepthAugment and MeasurementNoise draw what varies between train steps -- the frame and depth
augmentation and the measurement noise -- on the device as well, keyed by (seed, step); TrainInputs runs the four in front of the model.
"""
import math

import numpy as np
import torch
from torch.utils.data import Dataset

MOTIONS = {"random", "up", "up_random"}
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


PIL_PRECISION_BITS = 32 - 8 - 2


def pil_bilinear_tables(in_size, out_size):
    """Tap tables of Pillow's antialiased 8-bit bilinear resample along one axis (what `Resize(256)` on a PIL image runs,
    util/data_utils.py:48-54 of the reference): (bounds [out, 2] int32 = first input index and tap count, weights [out, ksize]
    int32 in 22-bit fixed point).  Host side, double precision, exactly Pillow's arithmetic (Resample.c precompute_coeffs +
    normalize_coeffs_8bpc); the device kernels only multiply-accumulate with them (csrc/norm.hip resize_*_kernel)."""
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    xx = np.arange(out_size, dtype=np.float64)
    center = (xx + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)       # (int) truncation of non-negative values
    xmin = np.where(center - support + 0.5 < 0, 0, xmin)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    taps = np.arange(ksize, dtype=np.float64)[None, :]
    t = np.abs((taps + xmin[:, None] - center[:, None] + 0.5) / filterscale)
    w = np.where((t < 1.0) & (taps < xmax[:, None]), 1.0 - t, 0.0)
    ww = w.sum(1, keepdims=True)
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    kk = np.floor(0.5 + w * (1 << PIL_PRECISION_BITS)).astype(np.int32)   # weights are >= 0 for the triangle filter: (int)(0.5 + v)
    kk = np.where(taps < xmax[:, None], kk, 0).astype(np.int32)
    return np.stack([xmin, xmax], 1).astype(np.int32), kk


def pil_bilinear_tables_f64(in_size, out_size):
    """Tap tables of Pillow's 32-bit-float bilinear resample along one axis (what `Resize(256)` runs on the mode-F image that
    ToPILImage makes of a float32 depth frame, util/data_utils.py:55-60 of the reference): (bounds [out, 2] int32 as in
    `pil_bilinear_tables`, weights [out, ksize] float64).  Resample.c precompute_coeffs, operation for operation: the filter argument
    is MULTIPLIED by 1 / filterscale, and the weights are summed in ascending tap order before the division -- the device kernel
    (csrc/depth_stage.hip) reproduces Pillow's pixels bit for bit only from bit-identical weights."""
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    xx = np.arange(out_size, dtype=np.float64)
    center = (xx + 0.5) * scale
    xmin = np.where(center - support + 0.5 < 0, 0, (center - support + 0.5).astype(np.int64))
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    taps = np.arange(ksize, dtype=np.float64)[None, :]
    t = np.abs((taps + xmin[:, None] - center[:, None] + 0.5) * ss)
    w = np.where((t < 1.0) & (taps < xmax[:, None]), 1.0 - t, 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for k in range(ksize):   # (np.sum pairs its additions up; Pillow adds tap by tap)
        ww = ww + w[:, k]
    ww = ww[:, None]
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    return np.stack([xmin, xmax], 1).astype(np.int32), np.ascontiguousarray(w)


def resized_hw(h, w, size=256):
    """torchvision.transforms.Resize(int) geometry: the shorter side becomes `size`, the longer int(size * long / short)."""
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


def crop_origin(h, w, ch, cw):
    """torchvision.transforms.CenterCrop: int(round((h - ch) / 2.0)), Python rounding (half to even)."""
    return int(round((h - ch) / 2.0)), int(round((w - cw) / 2.0))


def standardize_quat(quat):
    """(x,y,z,w) quaternion with a non-negative w (reference: util/data_utils.py:207-211)."""
    return -quat if quat[-1] < 0 else quat


def random_poses(lead, generator, device):
    pos = torch.rand(*lead, 3, generator=generator, device=device)
    pos = pos * torch.tensor([0.7, 0.7, 0.5], device=device) + torch.tensor([-0.35, -0.35, 0.8], device=device)
    q = torch.randn(*lead, 4, generator=generator, device=device)
    q = q / q.norm(dim=-1, keepdim=True)
    q = torch.where(q[..., 3:4] < 0, -q, q)
    return torch.cat([pos, q], dim=-1)


def noisy_measurement(x0, scale, z):
    """measurement = truth + sqrt(scale) z, the quaternion part renormalised (util/data_utils.py:162-167 of the reference): x0 (..., 7)
    true poses, `scale` a variance, z a standard-normal draw of x0's shape"""
    xb = x0 + (scale ** 0.5) * z
    q = xb[..., 3:]
    return torch.cat([xb[..., :3], q / q.norm(dim=-1, keepdim=True)], dim=-1)


def synthetic_batch(lead, seed, hw=224, with_depth=False, noise_scale=0.001, device="cuda"):
    """Seeded Robosuite-shaped batch with leading dims `lead` ((N,) or (S, N)), created on `device`."""
    lead = tuple(lead)
    g = torch.Generator(device=device).manual_seed(int(seed))
    u8 = torch.randint(0, 256, (*lead, 3, hw, hw), generator=g, device=device, dtype=torch.uint8)
    mean = torch.tensor(IMAGENET_MEAN, device=device).view(3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=device).view(3, 1, 1)
    img = (u8.float() / 255.0 - mean) / std
    depth = torch.rand(*lead, 1, hw, hw, generator=g, device=device) if with_depth else None
    x0, x1, obj = (random_poses(lead, g, device) for _ in range(3))
    x0bar = noisy_measurement(x0, noise_scale, torch.randn(*lead, 7, generator=g, device=device))
    return {"img": img, "depth": depth, "x0bar": x0bar, "x0": x0, "x1": x1, "obj": obj}


class _TimestepItems(Dataset):
    """`len()` = the horizon and `dataset[t]` = the reference's 6-tuple of all episodes at timestep t (util/data_utils.py:62-73), read
    from `self.data`; fields the dataset does not have are torch.empty garbage, as in the reference"""

    def __len__(self):
        return self.data["measurement_self"].size(1)

    def __getitem__(self, index):
        d = self.data
        img = d["imgs"][:, index]
        depth = d["depths"][:, index] if self.use_depth else torch.empty(0, device=img.device)
        x0bar = d["measurement_self"][:, index]
        x0 = d["true_self"][:, index]
        x1 = d["true_other"][:, index] if self.is_two_arm else torch.empty_like(x0)
        obj = d["true_obj"][:, index] if self.obj_name is not None else torch.empty_like(x0)
        return img, depth, x0bar, x0, x1, obj


class SyntheticEpisodeDataset(_TimestepItems):
    """MultiEpisodeDataset-shaped source of seeded synthetic episodes, resident on `device`."""

    frame_dtype = torch.float32   # preprocessed (normalised) images: nothing for FrameAugment to work on

    def __init__(self, horizon=20, use_depth=False, obj_name=None, is_two_arm=False, motion="random", seed=1234, hw=224,
                 device="cuda", env_name="Synthetic"):
        if motion not in MOTIONS:
            raise ValueError("Invalid motion specified. {} supported, {} requested.".format(MOTIONS, motion))
        self.data = None
        self.obj_name = obj_name
        self.use_depth = use_depth
        self.is_two_arm = is_two_arm
        self.motion = motion
        self.seed, self.hw, self.device = seed, hw, device
        self._refreshes = 0
        # train() only reads type(env).__name__ and env.horizon (util/learn_utils.py:84-89)
        self.env = type(env_name, (), {})()
        self.env.horizon = horizon

    def refresh_data(self, num_episodes, camera_name=None, noise_scale=0.001):
        b = synthetic_batch((num_episodes, self.env.horizon), self.seed + self._refreshes, self.hw, self.use_depth, noise_scale, self.device)
        self._refreshes += 1
        self.data = {"imgs": b["img"], "depths": b["depth"], "measurement_self": b["x0bar"], "true_self": b["x0"],
                     "true_other": b["x1"], "true_obj": b["obj"]}

    def chunk(self, t0, length):
        """Time-major chunk (S, N, ...) of timesteps [t0, t0+length): what DataLoader(batch_size=S, shuffle=False) stacks."""
        d = self.data
        sl = slice(t0, t0 + length)
        tm = lambda x: x[:, sl].transpose(0, 1).contiguous()
        img = tm(d["imgs"])
        depth = tm(d["depths"]) if self.use_depth else None
        x1 = tm(d["true_other"]) if self.is_two_arm else None
        obj = tm(d["true_obj"]) if self.obj_name is not None else None
        return img, depth, tm(d["measurement_self"]), tm(d["true_self"]), x1, obj


class RecordedEpisodeDataset(_TimestepItems):
    """MultiEpisodeDataset-shaped source of episodes RECORDED from the simulator elsewhere and read back from one `.npz` file: the
    keys of the reference's `MultiEpisodeDataset.data` (util/data_utils.py:85-92), raw instead of transformed --

        imgs       (E, T, Hs, Ws, 3) uint8      camera frames as robosuite returns them
        depths     (E, T, Hs, Ws, 1) float32    optional; needed for use_depth
        true_self  (E, T, 7) float32            end-effector pose (x, y, z, qx, qy, qz, qw)
        true_other (E, T, 7) float32            optional; needed for a two-arm environment
        true_obj   (E, T, 7) float32            optional; needed for obj_name
        env_name   string                       optional, default "Recorded"; "TwoArm" in it means two arms, as in the reference
        lengths    (E,) int32 or int64          optional; 1 <= lengths[e] <= T: episode e has lengths[e] timesteps, and rows
                                                [lengths[e], T) of its per-step arrays are padding that never influences a result

    A file without `lengths` is dense: every episode has T timesteps, `lengths` is None here and nothing below applies.  With it,
    `len(dataset)` and `env.horizon` stay T, the padded horizon; after refresh_data `selected_lengths` (host) and data["lengths"] hold
    the lengths of the selection, and `valid(t0, S)` marks the rows of a lockstep chunk that exist.

    The data stays on the HOST: `__getitem__(t)` hands out the reference's 6-tuple of host tensors with frames and depth raw, and
    train() moves them through FramePrefetcher; resize, crop and normalisation run on the device (rpe_stage_frames_u8[_resized],
    rpe_stage_depth_f32_resized).  `refresh_data` walks through the file: each call selects the next `num_episodes` episodes in
    file order, wrapping around, and draws fresh measurement noise (util/data_utils.py:162-167)."""

    _POSES = ("true_self", "true_other", "true_obj")
    frame_dtype = torch.uint8

    def __init__(self, path, use_depth=False, obj_name=None, seed=1234):
        with np.load(path, allow_pickle=False) as f:
            arrays = {k: f[k] for k in f.files}
        env_name = str(arrays.pop("env_name")) if "env_name" in arrays else "Recorded"
        self._check(arrays)
        lengths = arrays.pop("lengths", None)
        self.lengths = None if lengths is None else lengths.astype(np.int64)   # host, per episode in the file; None: a dense file
        self.selected_lengths = None
        self._valid_lengths = None          # the selection's lengths on the device valid() builds its masks on
        self.is_two_arm = "TwoArm" in env_name
        if use_depth and "depths" not in arrays:
            raise ValueError("{}: use_depth needs the 'depths' array".format(path))
        if obj_name is not None and "true_obj" not in arrays:
            raise ValueError("{}: obj_name={!r} needs the 'true_obj' array".format(path, obj_name))
        if self.is_two_arm and "true_other" not in arrays:
            raise ValueError("{}: a two-arm environment ({}) needs the 'true_other' array".format(path, env_name))
        self.path, self.use_depth, self.obj_name, self.seed = path, use_depth, obj_name, seed
        self.episodes = {k: torch.from_numpy(v) for k, v in arrays.items() if k != "depths" or use_depth}
        self.num_recorded = arrays["imgs"].shape[0]
        self.data = None
        self._next = 0
        self._gen = torch.Generator().manual_seed(int(seed))
        # train() only reads type(env).__name__ and env.horizon (util/learn_utils.py:84-89)
        self.env = type(env_name, (), {})()
        self.env.horizon = arrays["imgs"].shape[1]

    @staticmethod
    def file_lengths(path):
        """the `lengths` array of an episode file, or None for a dense one; reads nothing else of the file"""
        with np.load(path, allow_pickle=False) as f:
            return f["lengths"] if "lengths" in f.files else None

    @classmethod
    def _check(cls, arrays):
        """ValueError unless the arrays have the file format's ranks, dtypes and matching leading dimensions"""
        unknown = set(arrays) - {"imgs", "depths", "lengths"} - set(cls._POSES)
        if unknown:
            raise ValueError("unknown arrays {}: the file holds imgs, depths, true_self, true_other, true_obj, lengths, env_name".format(sorted(unknown)))
        for need in ("imgs", "true_self"):
            if need not in arrays:
                raise ValueError("the '{}' array is required".format(need))
        imgs = arrays["imgs"]
        if imgs.dtype != np.uint8 or imgs.ndim != 5 or imgs.shape[-1] != 3 or 0 in imgs.shape:
            raise ValueError("imgs must be uint8 (E, T, Hs, Ws, 3); got {} {}".format(imgs.dtype, imgs.shape))
        if "depths" in arrays:
            d = arrays["depths"]
            if d.dtype != np.float32 or d.shape != imgs.shape[:-1] + (1,):
                raise ValueError("depths must be float32 {}; got {} {}".format(imgs.shape[:-1] + (1,), d.dtype, d.shape))
        for k in cls._POSES:
            if k in arrays and (arrays[k].dtype != np.float32 or arrays[k].shape != imgs.shape[:2] + (7,)):
                raise ValueError("{} must be float32 {}; got {} {}".format(k, imgs.shape[:2] + (7,), arrays[k].dtype, arrays[k].shape))
        if "lengths" in arrays:
            n = arrays["lengths"]
            if n.dtype not in (np.int32, np.int64) or n.shape != imgs.shape[:1]:
                raise ValueError("lengths must be int32 or int64 {}; got {} {}".format(imgs.shape[:1], n.dtype, n.shape))
            bad = np.flatnonzero((n < 1) | (n > imgs.shape[1]))
            if bad.size:
                raise ValueError("lengths must lie in [1, T = {}]; got {} for episode {}".format(imgs.shape[1], int(n[bad[0]]), int(bad[0])))

    @classmethod
    def save(cls, path, env_name="Recorded", lengths=None, **arrays):
        """Write an episode file: imgs=, true_self= and optionally depths=, true_other=, true_obj= (numpy arrays or tensors), checked
        against the format above.  lengths= (E,) integers: the episodes' numbers of timesteps when the arrays are padded to one T."""
        arrays["lengths"] = lengths
        arrays = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrays.items() if v is not None}
        cls._check(arrays)
        with open(path, "wb") as f:   # (np.savez would append ".npz" to a bare name)
            np.savez(f, env_name=np.array(str(env_name)), **arrays)
        return path

    @classmethod
    def pack(cls, path, episodes, env_name="Recorded"):
        """Write episodes of unequal length as one file: `episodes` is a list of dicts of per-step arrays without the episode
        dimension -- imgs (T_e, Hs, Ws, 3), true_self (T_e, 7), ... -- which are padded with zeros to the longest and written with
        `lengths`.  ValueError when the keys, the dtypes or the frame geometry differ between episodes."""
        eps = [{k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in ep.items() if v is not None} for ep in episodes]
        if not eps:
            raise ValueError("pack: no episodes")
        first = eps[0]
        lengths = []
        for i, ep in enumerate(eps):
            if set(ep) != set(first):
                raise ValueError("pack: episode {} holds {}, episode 0 holds {}".format(i, sorted(ep), sorted(first)))
            steps = {v.shape[0] if v.ndim else -1 for v in ep.values()}
            if len(steps) != 1 or min(steps) < 1:
                raise ValueError("pack: the arrays of episode {} must share one number of timesteps, at least 1; got {}".format(
                    i, {k: v.shape[:1] for k, v in ep.items()}))
            for k, v in ep.items():
                if v.dtype != first[k].dtype or v.shape[1:] != first[k].shape[1:]:
                    raise ValueError("pack: {} of episode {} is {} {} per step, of episode 0 {} {}".format(
                        k, i, v.dtype, v.shape[1:], first[k].dtype, first[k].shape[1:]))
            lengths.append(steps.pop())
        t = max(lengths)
        arrays = {k: np.zeros((len(eps), t) + first[k].shape[1:], dtype=first[k].dtype) for k in first}
        for i, ep in enumerate(eps):
            for k, v in ep.items():
                arrays[k][i, :lengths[i]] = v
        return cls.save(path, env_name=env_name, lengths=np.asarray(lengths, dtype=np.int32), **arrays)

    def _select(self, num_episodes):
        """-> the numbers of the next `num_episodes` episodes in file order, wrapping around (also kept as the list `selected`)"""
        if num_episodes > self.num_recorded:
            raise ValueError("{} holds {} episodes; {} were asked for".format(self.path, self.num_recorded, num_episodes))
        sel = (torch.arange(num_episodes) + self._next) % self.num_recorded
        self._next = int(self._next + num_episodes) % self.num_recorded
        self.selected = sel.tolist()
        if self.lengths is not None:
            self.selected_lengths = self.lengths[sel.numpy()]
            self._valid_lengths = None
        return sel

    def peek_lengths(self, num_episodes):
        """the lengths of the episodes the NEXT refresh_data(num_episodes) will select (host; nothing is selected); None for a dense file"""
        if self.lengths is None:
            return None
        if num_episodes > self.num_recorded:
            raise ValueError("{} holds {} episodes; {} were asked for".format(self.path, self.num_recorded, num_episodes))
        return self.lengths[(np.arange(int(num_episodes)) + self._next) % self.num_recorded]

    def _lengths_on_device(self):
        """the selection's lengths as an int32 device tensor (N,): one upload per refresh"""
        if self._valid_lengths is None:
            dev = torch.device("cuda", torch.cuda.current_device())
            self._valid_lengths = torch.from_numpy(self.selected_lengths.astype(np.int32)).to(dev)
        return self._valid_lengths

    def valid(self, t0, length):
        """-> (length, N) uint8 device tensor, time-major like a chunk: 1 where timestep t0 + s of the n-th selected episode exists
        (t0 + s < its length), 0 where it is padding; None for a dense file.  Built on the device from the lengths."""
        if self.lengths is None:
            return None
        if self.selected_lengths is None:
            raise ValueError("{}: refresh_data has not selected any episodes yet".format(type(self).__name__))
        n = self._lengths_on_device()
        steps = torch.arange(int(t0), int(t0) + int(length), dtype=torch.int32, device=n.device)
        return (steps[:, None] < n[None, :]).to(torch.uint8)

    def _measure(self, x0, noise_scale):
        """a fresh measurement of the true poses x0, its noise drawn from the dataset's host generator"""
        return noisy_measurement(x0, noise_scale, torch.randn(x0.shape, generator=self._gen))

    def refresh_data(self, num_episodes, camera_name=None, noise_scale=0.001):
        sel = self._select(num_episodes)
        data = {k: v[sel] for k, v in self.episodes.items()}
        data["measurement_self"] = self._measure(data["true_self"], noise_scale)
        if self.lengths is not None:
            data["lengths"] = torch.from_numpy(self.selected_lengths)
        self.data = data


def window_counts(num_episodes, horizon, sequence_length, stride):
    """(K, M): start positions per episode K = (T - S) // stride + 1 and windows M = E K of `num_episodes` episodes of `horizon`
    timesteps cut into windows of `sequence_length` whose starts lie `stride` apart (a tail shorter than a window is not a window)"""
    e, t, s, k = int(num_episodes), int(horizon), int(sequence_length), int(stride)
    if k < 1:
        raise ValueError("the window stride must be at least 1; got {!r}".format(stride))
    if s < 1 or s > t:
        raise ValueError("a window of {} timesteps does not fit episodes of {}".format(s, t))
    if e < 1:
        raise ValueError("no episodes are selected ({!r})".format(num_episodes))
    per_episode = (t - s) // k + 1
    return per_episode, e * per_episode


def ragged_window_counts(lengths, sequence_length, stride):
    """(K_e per episode as a list, M): episode e of `lengths[e]` timesteps has K_e = (len_e - S) // stride + 1 windows of
    `sequence_length` whose starts lie `stride` apart, none when it is shorter than a window"""
    s, k = int(sequence_length), int(stride)
    if k < 1:
        raise ValueError("the window stride must be at least 1; got {!r}".format(stride))
    if s < 1:
        raise ValueError("a window needs at least 1 timestep; got {!r}".format(sequence_length))
    per_episode = [(int(n) - s) // k + 1 if int(n) >= s else 0 for n in lengths]
    if not per_episode:
        raise ValueError("no episodes are selected")
    return per_episode, sum(per_episode)


class ResidentEpisodeDataset(RecordedEpisodeDataset):
    """RecordedEpisodeDataset with the whole file resident in device memory: same file format, same constructor plus `device`, same
    `refresh_data` -- the next `num_episodes` episodes in file order, wrapping, with measurement noise from the same host generator, so
    the measurements equal the parent's for the same seed and call sequence.  The arrays are uploaded ONCE, raw; a refresh writes the
    selected episode numbers (`sel`) and their measurements into fixed device buffers in place, so a captured step sees it.  The
    measurement pool is laid out like the others, (E_file, T, 7): one (episode, timestep) index addresses every array.
    `chunk(t0, S)` is the lockstep batch the parent would have staged, gathered on the device (rpe_gather_rows), which train() and
    evaluate_episodes prefer; `sampler(...)` draws shuffled minibatches of any size (WindowSampler).  `__getitem__` returns device
    tensors.  A file with `lengths` has them uploaded once as well (`lengths_dev`, int32, one entry per episode in the file): the
    sampler's launch and `valid` read them through `sel`, so both follow a refresh without a copy."""

    def __init__(self, path, use_depth=False, obj_name=None, seed=1234, device="cuda"):
        super().__init__(path, use_depth=use_depth, obj_name=obj_name, seed=seed)
        self.device = torch.device(device)
        self._true_self_host = self.episodes["true_self"]     # the noise is drawn on the host, as the parent draws it
        self.pool = {k: v.to(self.device).contiguous() for k, v in self.episodes.items()}
        self.pool["measurement_self"] = self.pool["true_self"].clone()   # only the selected episodes' rows are ever read
        self.episodes = None                                  # (the host copy of the pixels is not kept)
        self.sel = torch.zeros(self.num_recorded, dtype=torch.int32, device=self.device)   # the first num_selected entries count
        self.lengths_dev = None if self.lengths is None else torch.from_numpy(self.lengths.astype(np.int32)).to(self.device)
        self.num_selected = 0
        self.selected = []

    def __len__(self):
        return self.env.horizon

    def refresh_data(self, num_episodes, camera_name=None, noise_scale=0.001):
        sel = self._select(num_episodes)
        meas = self._measure(self._true_self_host[sel], noise_scale)
        sel_dev = sel.to(self.device)
        self.sel[:num_episodes].copy_(sel_dev.to(torch.int32))                      # in place: captured launches read these buffers
        self.pool["measurement_self"].index_copy_(0, sel_dev, meas.to(self.device))
        self.num_selected = int(num_episodes)
        if self.lengths is not None:
            self.data = {"lengths": torch.from_numpy(self.selected_lengths)}

    def _lengths_on_device(self):
        return self.lengths_dev[self.sel[:self.num_selected].long()]

    def _need_refresh(self):
        if self.num_selected < 1:
            raise ValueError("{}: refresh_data has not selected any episodes yet".format(type(self).__name__))

    def _batch(self, index, length, out=None):
        """the six-tuple (img, depth, x0bar, x0, x1, obj), time-major (length, N, ...), of the windows `index` names; fields the
        file or the model does not have are None"""
        from .. import ops
        t = self.env.horizon
        keys = ("imgs", "depths" if self.use_depth else None, "measurement_self", "true_self", "true_other" if self.is_two_arm else None,
                "true_obj" if self.obj_name is not None else None)
        return tuple(None if k is None else ops.gather_rows(self.pool[k], index, length, t, out=None if out is None else out[i])
                     for i, k in enumerate(keys))

    def chunk(self, t0, length):
        """Time-major chunk (S, N, ...) of timesteps [t0, t0 + length) of the selected episodes: what RecordedEpisodeDataset hands
        train() through _host_chunks and FramePrefetcher, gathered on the device."""
        self._need_refresh()
        if not (0 <= t0 and length >= 1 and t0 + length <= self.env.horizon):
            raise ValueError("chunk [{}, {}) leaves the episodes' {} timesteps".format(t0, t0 + length, self.env.horizon))
        e = self.num_selected
        index = torch.empty(1 + 2 * e, dtype=torch.int32, device=self.device)
        index[0] = 0
        index[1::2] = self.sel[:e]
        index[2::2] = int(t0)
        return self._batch(index, length)

    def __getitem__(self, t):
        """the reference's 6-tuple of all selected episodes at timestep t, device tensors (absent fields: empty, as the parent's)"""
        img, depth, x0bar, x0, x1, obj = (None if v is None else v[0] for v in self.chunk(int(t), 1))
        return (img, depth if depth is not None else torch.empty(0, device=self.device), x0bar, x0,
                x1 if x1 is not None else torch.empty_like(x0), obj if obj is not None else torch.empty_like(x0))

    def sampler(self, batch_size, sequence_length=1, stride=None, shuffle=True, seed=0):
        """-> WindowSampler over the episodes the last refresh_data selected"""
        return WindowSampler(self, batch_size, sequence_length, stride, shuffle, seed)


WORKSPACE_LO = (-0.35, -0.35, 0.8)    # the workspace of `random_poses`
WORKSPACE_HI = (0.35, 0.35, 1.3)

# six colours per body, all eighteen distinct: which body a pixel shows, and which way the body is turned, can be read off the frame
BOX_FACE_COLOURS = (((220, 40, 40), (255, 140, 0), (160, 30, 90), (250, 200, 60), (120, 20, 20), (255, 100, 150)),      # own end effector: reds
                    ((40, 60, 220), (0, 160, 255), (90, 40, 170), (60, 220, 230), (20, 30, 120), (150, 130, 255)),      # other arm: blues
                    ((40, 180, 60), (160, 230, 40), (20, 110, 70), (200, 255, 150), (10, 70, 20), (100, 200, 160)))     # object: greens


def look_at_camera(eye, target, up, vfov_deg, hs, ws):
    """(3, 4) float64 camera matrix in the overlay's convention ([u w, v w, w] = P [x, y, z, 1], u the column and v the row as stored,
    row 0 at the top of the picture, pixel centres at integers) of a pinhole camera at `eye` looking at `target`, square pixels,
    vertical field of view `vfov_deg`, principal point ((ws - 1) / 2, (hs - 1) / 2); w is the distance along the viewing direction"""
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, up)
    right = right / np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])
    focal = (hs / 2.0) / math.tan(math.radians(vfov_deg) / 2.0)
    K = np.array([[focal, 0.0, (ws - 1) / 2.0], [0.0, focal, (hs - 1) / 2.0], [0.0, 0.0, 1.0]])
    return K @ np.concatenate([R, (-R @ eye)[:, None]], axis=1)


class BoxScene:
    """The scene of rendered episodes (DESIGN.md "Rendered episodes": the specification and its numpy restatement exist, the device
    renderer does not yet): a camera matrix `P` (3, 4) float64, the frame size, the depth range [near, far], `bodies` -- (half extents,
    six face colours) each, body g drawn at pose g of a frame -- a checkered ground `plane` (z0, checker size, colour, colour) or None,
    the `sky` colour and `ss` (1: one ray per pixel, 2: four)."""

    def __init__(self, P, hs, ws, near, far, bodies, plane=None, sky=(150, 180, 220), ss=1):
        self.P = np.array(P, dtype=np.float64)
        self.hs, self.ws, self.near, self.far = int(hs), int(ws), float(near), float(far)
        self.bodies = [(tuple(float(v) for v in h), tuple(tuple(int(v) for v in c) for c in cols)) for h, cols in bodies]
        self.plane, self.sky, self.ss = plane, tuple(sky), int(ss)
        if self.P.shape != (3, 4):
            raise ValueError("BoxScene: P is a (3, 4) camera matrix; got shape {}".format(self.P.shape))
        if not (1 <= self.hs <= 4096 and 1 <= self.ws <= 4096):
            raise ValueError("BoxScene: frames are 1..4096 pixels a side; got {} x {}".format(hs, ws))
        for h, cols in self.bodies:
            if len(set(cols)) != 6:
                raise ValueError("BoxScene: a body has six DISTINCT face colours (its orientation is read off them); got {}".format(cols))

    @classmethod
    def default(cls, hs=256, ws=256, ss=1):
        """the scene of the rendered task: a camera at (1.6, 0, 1.45) looking at the middle of the workspace of `random_poses` from
        the front, 45 degrees of vertical field of view; boxes of 10 x 8 x 12 cm for the two end effectors and a 12 cm cube for the
        object; a grey checkered table 10 cm below the workspace"""
        P = look_at_camera((1.6, 0.0, 1.45), (0.0, 0.0, 1.0), (0.0, 0.0, 1.0), 45.0, hs, ws)
        bodies = [((0.05, 0.04, 0.06), BOX_FACE_COLOURS[0]), ((0.05, 0.04, 0.06), BOX_FACE_COLOURS[1]), ((0.06, 0.06, 0.06), BOX_FACE_COLOURS[2])]
        return cls(P, hs, ws, 0.1, 10.0, bodies, plane=(0.7, 0.1, (110, 110, 110), (170, 170, 170)), sky=(150, 180, 220), ss=ss)

    def camera_matrix(self):
        """(3, 4) float64: what ops.project_poses / render_episodes take as the camera of frames of this scene"""
        return self.P.copy()


def scene_trajectories(num_episodes, horizon, motion="random", seed=0):
    """(E, T, 3, 7) float32 poses (x, y, z, qx, qy, qz, qw) of three bodies -- own end effector, other arm, object -- over E episodes of
    T timesteps, host numpy, from np.random.default_rng(seed) alone.  Starts are uniform in the workspace of `random_poses`;
    "random": a walk whose velocity is AR(1) (v <- 0.8 v + 0.02 N(0, I)), reflected at the workspace walls; "up": x and y stay, z rises
    linearly to the top of the workspace; "up_random": the walk in x and y, the rise in z.  The orientation is a random walk on the
    unit quaternions (q <- normalise(q + 0.1 N(0, I))), stored with w >= 0 (`standardize_quat`)."""
    if motion not in MOTIONS:
        raise ValueError("Invalid motion specified. {} supported, {} requested.".format(MOTIONS, motion))
    e, t = int(num_episodes), int(horizon)
    if e < 1 or t < 1:
        raise ValueError("scene_trajectories: at least one episode of one timestep; got {} x {}".format(num_episodes, horizon))
    rng = np.random.default_rng(int(seed))
    lo, hi = np.array(WORKSPACE_LO), np.array(WORKSPACE_HI)
    pos = rng.uniform(lo, hi, size=(e, 3, 3))
    vel = 0.02 * rng.standard_normal((e, 3, 3))
    q = rng.standard_normal((e, 3, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    z_start = pos[..., 2].copy()
    out = np.empty((e, t, 3, 7), dtype=np.float64)
    walk = (True, True, motion == "random") if motion != "up" else (False, False, False)
    for k in range(t):
        if motion != "random":
            pos[..., 2] = z_start + (hi[2] - z_start) * (k / (t - 1) if t > 1 else 0.0)
        out[:, k, :, :3] = pos
        out[:, k, :, 3:] = np.where(q[..., 3:] < 0, -q, q)
        step_v = 0.8 * vel + 0.02 * rng.standard_normal((e, 3, 3))
        step_q = 0.1 * rng.standard_normal((e, 3, 4))
        vel = step_v
        for i in range(3):
            if not walk[i]:
                continue
            p = pos[..., i] + vel[..., i]
            over, under = p > hi[i], p < lo[i]
            p = np.where(over, 2 * hi[i] - p, np.where(under, 2 * lo[i] - p, p))
            vel[..., i] = np.where(over | under, -vel[..., i], vel[..., i])
            pos[..., i] = np.clip(p, lo[i], hi[i])
        q = q + step_q
        q /= np.linalg.norm(q, axis=-1, keepdims=True)
    return out.astype(np.float32)


class _DeviceStepCounter:
    """What WindowSampler, FrameAugment, DepthAugment and MeasurementNoise share: `seed`; a step counter that lives in device memory
    once there is a device to keep it on (`_state`, an int32 tensor whose element 0 the launch itself advances) and on the host before
    that (`_step0`); and the buffers a launch writes beside its output (`_kept`)."""

    def __init__(self, seed):
        self.seed = int(seed)
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError("seed must fit 64 unsigned bits; got {!r}".format(seed))
        self._state = None          # int32 device tensor, element 0 = the step counter
        self._step0 = 0             # the counter while there is no device tensor yet
        self._keep = {}

    @staticmethod
    def _wrap_i32(step):
        """a 32-bit counter value as the int32 that holds the same bits"""
        return step - (1 << 32) if step >= (1 << 31) else step

    def _device_state(self, device):
        if self._state is None or self._state.device != device:
            self._state = torch.tensor([self._wrap_i32(self.step)], dtype=torch.int32, device=device)
        return self._state

    def _kept(self, key, make):
        """the buffer(s) `make()` made for `key` the first time it was asked for.  Never freed or replaced while the object lives: a
        captured call has their addresses, whatever shapes the object is called with afterwards."""
        if key not in self._keep:
            self._keep[key] = make()
        return self._keep[key]

    @property
    def step(self):
        """the step counter: the number of calls so far, replays of a captured call included (reads the device)"""
        return self._step0 if self._state is None else int(self._state[0].item()) & 0xFFFFFFFF

    def state_dict(self):
        return {"seed": self.seed, "step": self.step}

    def load_state_dict(self, sd):
        seed, step = int(sd["seed"]), int(sd["step"])
        if not (0 <= seed < 2 ** 64 and 0 <= step < 2 ** 32):
            raise ValueError("{}.load_state_dict: seed / step out of range: {!r}".format(type(self).__name__, sd))
        self.seed = seed
        self._step0 = step
        if self._state is not None:   # in place: a captured call keeps reading this tensor
            self._state.fill_(self._wrap_i32(step))


class WindowSampler(_DeviceStepCounter):
    """Shuffled minibatches of `batch_size` windows of `sequence_length` consecutive timesteps from a ResidentEpisodeDataset, drawn
    on the device (rpe_sample_windows + rpe_gather_rows; DESIGN.md "Minibatch sampling").  stride=None: window starts
    `sequence_length` apart -- the reference's chunk grid, in shuffled order; stride=1: every offset.  An epoch is the M = E K windows
    of the E selected episodes, each visited once, under a keyed permutation that changes with the epoch; a batch may straddle two
    epochs.  The order is a function of (seed, step) alone; the step counter lives in device memory and every call advances it, also
    a call replayed from a captured graph.  A call returns the six-tuple (img, depth, x0bar, x0, x1, obj), time-major (S, N, ...),
    in buffers the sampler owns: the next call overwrites them, and a captured consumer keeps their addresses.  refresh_data between
    calls changes the episodes and measurements the next call reads (the same number of episodes must stay selected).
    A dataset with `lengths` (episodes of unequal length) goes through rpe_sample_windows_ragged: the window table is built on the
    device at every launch from the lengths of whatever is selected, a window never reaches into padding, and an episode shorter than
    a window is never drawn.  `windows_per_episode` is a list there; it, `num_windows` and `steps_per_epoch` follow the current
    selection (host lengths), and a selection with fewer windows than a batch is a ValueError at the next call.

        sampler = dataset.sampler(256, shuffle=True, seed=0)
        for _ in range(sampler.steps_per_epoch):
            img, depth, x0bar, x0, x1, obj = sampler()
    """

    def __init__(self, dataset, batch_size, sequence_length=1, stride=None, shuffle=True, seed=0):
        dataset._need_refresh()
        self.dataset = dataset
        self.batch_size, self.sequence_length = int(batch_size), int(sequence_length)
        self.stride = self.sequence_length if stride is None else int(stride)
        self.shuffle = bool(shuffle)
        super().__init__(seed)
        if self.batch_size < 1:
            raise ValueError("batch_size must be at least 1; got {!r}".format(batch_size))
        self.num_episodes = dataset.num_selected
        self.ragged = dataset.lengths is not None
        self._counted = None        # (the selection counted, its (windows per episode, windows))
        self.check_windows()
        dev = dataset.device
        self.index = torch.zeros(1 + 2 * self.batch_size, dtype=torch.int32, device=dev)   # [0] the step used, then (episode, t0) per window
        self._state = torch.zeros(1, dtype=torch.int32, device=dev)                         # the counter: on the dataset's device at once

    def _counts(self):
        """(windows per episode, windows) of the current selection: K and M = E K, or on a ragged dataset the list of K_e and their sum"""
        ds = self.dataset
        if not self.ragged:
            if self._counted is None:   # E and T do not change: once
                self._counted = (None, window_counts(self.num_episodes, ds.env.horizon, self.sequence_length, self.stride))
        elif self._counted is None or self._counted[0] is not ds.selected_lengths:   # (refresh_data makes a new array)
            if not 1 <= self.sequence_length <= ds.env.horizon:
                raise ValueError("a window of {} timesteps does not fit episodes of {}".format(self.sequence_length, ds.env.horizon))
            self._counted = (ds.selected_lengths, ragged_window_counts(ds.selected_lengths, self.sequence_length, self.stride))
        return self._counted[1]

    @property
    def windows_per_episode(self):
        return self._counts()[0]

    @property
    def num_windows(self):
        return self._counts()[1]

    @property
    def steps_per_epoch(self):
        return self.num_windows // self.batch_size

    def check_windows(self):
        """ValueError when the current selection holds fewer windows than a batch"""
        if self.num_windows < self.batch_size:
            raise ValueError("a batch of {} windows needs at least as many windows; {} episodes of {} timesteps give {} (sequence_length {}, stride {})".format(
                self.batch_size, self.num_episodes, "up to {}".format(self.dataset.env.horizon) if self.ragged else self.dataset.env.horizon,
                self.num_windows, self.sequence_length, self.stride))

    def desc_fields(self):
        """the integers of rpe_sample_desc"""
        return dict(seed=self.seed, E=self.num_episodes, T=self.dataset.env.horizon, S=self.sequence_length, stride=self.stride, N=self.batch_size,
                    shuffle=int(self.shuffle))

    def buffers(self):
        """the six-tuple of buffers every call writes and returns (made on first use and kept: a captured call has their addresses)"""
        ds, s, n = self.dataset, self.sequence_length, self.batch_size
        new = lambda k: torch.empty((s, n) + tuple(ds.pool[k].shape[2:]), dtype=ds.pool[k].dtype, device=ds.device)
        return self._kept("out", lambda: (new("imgs"), new("depths") if ds.use_depth else None, new("measurement_self"), new("true_self"),
                                          new("true_other") if ds.is_two_arm else None, new("true_obj") if ds.obj_name is not None else None))

    def __call__(self):
        from .. import ops
        ds = self.dataset
        if ds.num_selected != self.num_episodes:
            raise ValueError("the sampler was made for {} selected episodes; refresh_data has selected {} since".format(self.num_episodes, ds.num_selected))
        if self.ragged:
            self.check_windows()   # the selection may have changed
            ops.sample_windows_ragged(ops.sample_desc(**self.desc_fields()), ds.sel, ds.lengths_dev, self._state, out=self.index)
        else:
            ops.sample_windows(ops.sample_desc(**self.desc_fields()), ds.sel, self._state, out=self.index)
        return ds._batch(self.index, self.sequence_length, out=self.buffers())


NOISE_SUM_STD = 147.8005   # standard deviation of the sum of four uniform bytes: sqrt(4 (256^2 - 1) / 12)
ERASE_FILL_MEAN = (124, 116, 104)   # the ImageNet mean in bytes: normalises to ~0


def _q16(f):
    return int(round(65536.0 * f))


def _jitter_range(name, amount):
    """torchvision's ColorJitter range for a non-negative amount: factors in [max(0, 1 - a), 1 + a], as Q16 integers"""
    a = float(amount)
    if not 0.0 <= a <= 3.0:
        raise ValueError("{} must lie in [0, 3] (factors up to 4); got {!r}".format(name, amount))
    return _q16(max(0.0, 1.0 - a)), _q16(1.0 + a)


BLUR_LEVELS, BLUR_DIRS, BLUR_MAX_RADIUS, BLUR_TAP_SUM = 8, 16, 8, 2048


def blur_gaussian_taps(sigma):
    """(R, [w_0 .. w_R]): the integer half-kernel of a Gaussian of standard deviation `sigma` pixels as rpe_blur_frames_u8 takes it --
    R = min(8, max(1, ceil(3 sigma))), w_k = round(2048 g_k / sum g) with g_k = exp(-k^2 / 2 sigma^2) over k = -R .. R, and w_0 set
    so that w_0 + 2 (w_1 + .. + w_R) = 2048 exactly.  sigma = 0: R = 0, the identity."""
    sigma = float(sigma)
    if not 0.0 <= sigma <= 4.0:
        raise ValueError("a blur sigma must lie in [0, 4] pixels; got {!r}".format(sigma))
    if sigma == 0.0:
        return 0, [BLUR_TAP_SUM]
    r = min(BLUR_MAX_RADIUS, max(1, int(math.ceil(3.0 * sigma))))
    g = [math.exp(-k * k / (2.0 * sigma * sigma)) for k in range(r + 1)]
    total = g[0] + 2.0 * sum(g[1:])
    w = [int(round(BLUR_TAP_SUM * v / total)) for v in g]
    w[0] = BLUR_TAP_SUM - 2 * sum(w[1:])
    return r, w


def blur_directions(nd=BLUR_DIRS):
    """the Q8 components (cx, cy) of `nd` motion directions over 180 degrees: round(256 cos(pi d / nd)), round(256 sin(pi d / nd))"""
    return ([int(round(256.0 * math.cos(math.pi * d / nd))) for d in range(nd)], [int(round(256.0 * math.sin(math.pi * d / nd))) for d in range(nd)])


class FrameAugment(_DeviceStepCounter):
    """Label-preserving augmentation of raw uint8 camera frames on the device (rpe_augment_frames_u8; DESIGN.md "Frame
    augmentation"): brightness / contrast / saturation jitter with torchvision's ranges (`brightness=b`: a factor in
    [max(0, 1 - b), 1 + b]), sensor noise of `noise_std` grey levels, and random erasing of one rectangle per frame with probability
    `erase_prob`, each side a fraction `erase_scale` = (lo, hi) of the frame's, filled with `erase_fill`: "mean" (the ImageNet mean,
    which normalises to ~0), "noise" (random bytes) or an (r, g, b) tuple.  No crop, shift or flip: the labels are absolute poses
    seen by a fixed camera.  The random numbers are drawn on the device from (seed, step); the step counter lives in device memory
    and every call advances it, also a call replayed from a captured graph.
    Blur (rpe_blur_frames_u8; DESIGN.md "Frame blur") runs in front of all that, optics first: with probability `blur_prob` a frame
    is defocused by a Gaussian whose sigma is one of 8 levels spread over `blur_sigma` = (lo, hi) pixels, with probability
    `motion_blur_prob` it is smeared along one of 16 directions over an odd length of 3 .. `motion_blur_max_length` pixels, otherwise
    it stays sharp.  With both probabilities 0 (the default) no blur launch is issued.
    per_episode: frames (S, N, Hs, Ws, 3) share their jitter, blur and occluder along S (one episode keeps them through the chunk);
    the noise is always per frame.  A 4-D batch (B, Hs, Ws, 3) draws per frame.

        aug = FrameAugment(brightness=0.2, contrast=0.2, noise_std=2.0, erase_prob=0.25)
        frames = aug(frames)                # uint8 device frames -> a new uint8 tensor of the same shape
    """

    def __init__(self, brightness=0., contrast=0., saturation=0., noise_std=0., erase_prob=0., erase_scale=(0.1, 0.3), erase_fill="mean",
                 per_episode=True, seed=0, blur_prob=0., blur_sigma=(0.5, 2.0), motion_blur_prob=0., motion_blur_max_length=9):
        self.qb = _jitter_range("brightness", brightness)
        self.qc = _jitter_range("contrast", contrast)
        self.qs = _jitter_range("saturation", saturation)
        if not float(noise_std) >= 0.0:
            raise ValueError("noise_std must not be negative; got {!r}".format(noise_std))
        self.noise_q = _q16(float(noise_std) / NOISE_SUM_STD)
        if self.noise_q > 4 * 65536:
            raise ValueError("noise_std {!r} is beyond the kernel's range ({:.0f} grey levels)".format(noise_std, 4 * NOISE_SUM_STD))
        if not 0.0 <= float(erase_prob) <= 1.0:
            raise ValueError("erase_prob must lie in [0, 1]; got {!r}".format(erase_prob))
        self.erase_thresh = min(2 ** 32 - 1, int(round(float(erase_prob) * 2 ** 32)))
        lo, hi = (float(v) for v in erase_scale)
        if not 0.0 < lo <= hi <= 1.0:
            raise ValueError("erase_scale must be (lo, hi) with 0 < lo <= hi <= 1; got {!r}".format(erase_scale))
        self.erase_scale = (lo, hi)
        if erase_fill == "mean":
            self.fill_mode, self.fill_rgb = 0, ERASE_FILL_MEAN
        elif erase_fill == "noise":
            self.fill_mode, self.fill_rgb = 1, ERASE_FILL_MEAN
        else:
            try:
                rgb = tuple(int(v) for v in erase_fill)
            except (TypeError, ValueError):
                rgb = ()
            if len(rgb) != 3 or not all(0 <= v <= 255 for v in rgb):
                raise ValueError('erase_fill is "mean", "noise" or an (r, g, b) tuple of bytes; got {!r}'.format(erase_fill))
            self.fill_mode, self.fill_rgb = 0, rgb
        self.per_episode = bool(per_episode)
        pg, pm = float(blur_prob), float(motion_blur_prob)
        if not (0.0 <= pg <= 1.0 and 0.0 <= pm <= 1.0 and pg + pm <= 1.0):
            raise ValueError("blur_prob and motion_blur_prob must lie in [0, 1] with a sum of at most 1; got {!r}, {!r}".format(blur_prob, motion_blur_prob))
        self.gauss_thresh = min(2 ** 32 - 1, int(round(pg * 2 ** 32)))
        self.motion_thresh = min(2 ** 32 - 1 - self.gauss_thresh, int(round(pm * 2 ** 32)))
        try:
            lo, hi = (float(v) for v in blur_sigma)
        except (TypeError, ValueError):
            raise ValueError("blur_sigma is (lo, hi) in pixels; got {!r}".format(blur_sigma))
        if not 0.0 <= lo <= hi <= 4.0:
            raise ValueError("blur_sigma must be (lo, hi) with 0 <= lo <= hi <= 4; got {!r}".format(blur_sigma))
        self.blur_sigma = (lo, hi)
        ns = 1 if lo == hi else BLUR_LEVELS
        self.blur_sigmas = [lo + (hi - lo) * s / (ns - 1) if ns > 1 else lo for s in range(ns)]
        self.blur_levels = [blur_gaussian_taps(v) for v in self.blur_sigmas]   # (R, taps) per level
        if isinstance(motion_blur_max_length, bool) or int(motion_blur_max_length) != motion_blur_max_length or not 3 <= motion_blur_max_length <= 15 \
                or motion_blur_max_length % 2 == 0:
            raise ValueError("motion_blur_max_length must be an odd integer in [3, 15]; got {!r}".format(motion_blur_max_length))
        self.motion_blur_max_length = int(motion_blur_max_length)
        self.blur_dirs = blur_directions()
        super().__init__(seed)
        self.last_params = None     # device table of the last call: [0] the step used, then per stream qb qc qs erase top left h w
        self.last_blur_params = None   # device table of the last call's blur: [0] the step used, then per stream kind level L d (None: blur off)
        self.last_geometry = None   # (Hs, Ws, frames, group) of the last call

    def erase_bounds(self, size):
        """erase_scale as pixel bounds (lo, hi) of a side of `size` pixels, 1 <= lo <= hi <= size"""
        lo = min(size, max(1, int(round(self.erase_scale[0] * size))))
        return lo, min(size, max(lo, int(round(self.erase_scale[1] * size))))

    def desc_fields(self, hs, ws, group=0):
        """the integers of rpe_augment_desc for frames of hs x ws"""
        (eh_lo, eh_hi), (ew_lo, ew_hi) = self.erase_bounds(hs), self.erase_bounds(ws)
        return dict(seed=self.seed, qb_lo=self.qb[0], qb_hi=self.qb[1], qc_lo=self.qc[0], qc_hi=self.qc[1], qs_lo=self.qs[0], qs_hi=self.qs[1],
                    noise_q=self.noise_q, erase_thresh=self.erase_thresh, eh_lo=eh_lo, eh_hi=eh_hi, ew_lo=ew_lo, ew_hi=ew_hi, fill_mode=self.fill_mode,
                    fill_r=self.fill_rgb[0], fill_g=self.fill_rgb[1], fill_b=self.fill_rgb[2], group=int(group))

    @property
    def blurs(self):
        """whether a call issues the blur launches"""
        return self.gauss_thresh != 0 or self.motion_thresh != 0

    def blur_desc_fields(self, group=0):
        """the arguments of ops.blur_desc (rpe_blur_desc)"""
        return dict(seed=self.seed, gauss_thresh=self.gauss_thresh, motion_thresh=self.motion_thresh, radius=[r for r, _ in self.blur_levels],
                    taps=[list(w) for _, w in self.blur_levels], n_lengths=(self.motion_blur_max_length - 1) // 2, dir_cx=list(self.blur_dirs[0]),
                    dir_cy=list(self.blur_dirs[1]), group=int(group))

    @staticmethod
    def check_frames(frames):
        """ValueError unless `frames` are uint8 device frames, channels last: (B, Hs, Ws, 3) or (S, N, Hs, Ws, 3), contiguous"""
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8:
            raise ValueError("FrameAugment takes raw uint8 frames; got {}".format(getattr(frames, "dtype", type(frames))))
        if frames.dim() not in (4, 5) or frames.shape[-1] != 3 or not frames.is_contiguous() or frames.numel() == 0:
            raise ValueError("FrameAugment takes channels-last frames (B, Hs, Ws, 3) or (S, N, Hs, Ws, 3), contiguous; got {}".format(tuple(frames.shape)))
        if not frames.is_cuda:
            raise ValueError("FrameAugment runs on the device only (there is no CPU path); got a {} tensor".format(frames.device))

    def __call__(self, frames, out=None):
        from .. import ops
        self.check_frames(frames)
        hs, ws = frames.shape[-3:-1]
        group = frames.shape[1] if self.per_episode and frames.dim() == 5 else 0
        b = frames.numel() // (hs * ws * 3)
        state = self._device_state(frames.device)
        params, sums = self._kept((b, group, frames.device), lambda: (torch.empty(1 + 8 * (group or b), dtype=torch.int32, device=frames.device),
                                                                      torch.empty(b, dtype=torch.int64, device=frames.device)))
        if self.blurs:   # optics first: the blur reads the step counter, the augmentation launch behind it advances it
            blurred, bparams = self._kept(("blur", tuple(frames.shape), group, frames.device),
                                          lambda: (torch.empty_like(frames), torch.empty(1 + 4 * (group or b), dtype=torch.int32, device=frames.device)))
            frames = ops.blur_frames_u8(frames, ops.blur_desc(**self.blur_desc_fields(group)), state, out=blurred, params=bparams)
            self.last_blur_params = bparams
        out = ops.augment_frames_u8(frames, ops.augment_desc(**self.desc_fields(hs, ws, group)), state, out=out, params=params, sums=sums)
        self.last_params = params
        self.last_geometry = (int(hs), int(ws), int(b), int(group))   # what DepthAugment(share_erase=self) checks its own batch against
        return out



DEPTH_NOISE_T_STD = math.sqrt(2.0 * (2 ** 32 - 1))   # standard deviation of the kernel's integer T: Var T = 4 * 6 * (65536^2 - 1) / 12


class DepthAugment(_DeviceStepCounter):
    """Depth-sensor augmentation of raw fp32 depth frames on the device (rpe_augment_depth_f32; DESIGN.md "Depth augmentation"), the
    depth side of FrameAugment.  Per pixel d, in this order:
      noise=(s0, s1, s2): d + N(0, sd^2) with sd = s0 + s1 d + s2 d^2 -- constant, linear and quadratic in range, in the units of the
          recorded depth values (robosuite: the normalised z-buffer); one or two values set the leading coefficients
      quant=q: rounded to multiples of q (round half even)
      clamp=(lo, hi): limited to [lo, hi]
      drop_prob=p: the pixel becomes `hole_value` with probability p
      holes=(lo, hi): lo..hi rectangles per frame (at most 4), each side a fraction `hole_scale` = (lo, hi) of the frame's, set to
          `hole_value`
      share_erase=<the FrameAugment of the RGB frames>: the rectangle that augmentation erased in a frame becomes `occluder_value`
          here, so that the occluder hides depth as well; call it on the RGB frames of the batch FIRST
    No crop, shift, flip or global rescale: the labels are absolute poses seen by a fixed camera.  The random numbers are drawn on the
    device from (seed, step) under purposes of their own, so one seed given to FrameAugment and DepthAugment yields independent draws;
    the step counter lives in device memory and every call advances it, also a call replayed from a captured graph.
    per_frame=False: frames (S, N, ...) share their holes along S (one episode keeps them through the chunk) -- the grouping
    FrameAugment(per_episode=True) uses; noise and dropout are always per frame and per pixel.  A 4-D batch draws per frame.
    Takes contiguous fp32 device tensors (..., Hs, Ws, 1), as recorded, or (..., 1, H, W), as the synthetic dataset hands them out.

        daug = DepthAugment(noise=(0.001, 0.0, 0.002), drop_prob=0.01, holes=(0, 2), share_erase=aug)
        frames = aug(frames); depth = daug(depth)      # a new fp32 tensor of the same shape
    """

    def __init__(self, noise=(0., 0., 0.), drop_prob=0., holes=(0, 0), hole_scale=(0.02, 0.15), hole_value=0., quant=0., clamp=None, occluder_value=0.,
                 per_frame=False, seed=0, share_erase=None):
        try:
            sig = tuple(float(v) for v in (noise if isinstance(noise, (tuple, list)) else (noise,)))
        except (TypeError, ValueError):
            sig = ()
        if not 1 <= len(sig) <= 3 or not all(math.isfinite(v) and v >= 0.0 for v in sig):
            raise ValueError("noise is one to three finite, non-negative standard-deviation coefficients (s0, s1, s2); got {!r}".format(noise))
        self.noise = sig + (0.0,) * (3 - len(sig))
        self.n = tuple(v / DEPTH_NOISE_T_STD for v in self.noise)   # in double: the kernel never sees a square root
        if not 0.0 <= float(drop_prob) <= 1.0:
            raise ValueError("drop_prob must lie in [0, 1]; got {!r}".format(drop_prob))
        self.drop_thresh = min(2 ** 32 - 1, int(round(float(drop_prob) * 2 ** 32)))
        try:
            h_lo, h_hi = (int(v) for v in holes)
        except (TypeError, ValueError):
            raise ValueError("holes is (lo, hi), the number of rectangles per frame; got {!r}".format(holes))
        if not 0 <= h_lo <= h_hi <= 4:
            raise ValueError("holes must be (lo, hi) with 0 <= lo <= hi <= 4; got {!r}".format(holes))
        self.holes = (h_lo, h_hi)
        lo, hi = (float(v) for v in hole_scale)
        if not 0.0 < lo <= hi <= 1.0:
            raise ValueError("hole_scale must be (lo, hi) with 0 < lo <= hi <= 1; got {!r}".format(hole_scale))
        self.hole_scale = (lo, hi)
        self.quant = float(quant)
        if not (math.isfinite(self.quant) and self.quant >= 0.0):
            raise ValueError("quant must be finite and not negative; got {!r}".format(quant))
        self.inv_quant = 1.0 / self.quant if self.quant > 0.0 else 0.0
        if not math.isfinite(self.inv_quant):
            raise ValueError("quant {!r} is too small: 1 / quant is not finite".format(quant))
        if clamp is None:
            self.clamp = (-math.inf, math.inf)
        else:
            lo, hi = (float(v) for v in clamp)
            if not lo <= hi:   # (false for a NaN as well)
                raise ValueError("clamp must be (lo, hi) with lo <= hi; got {!r}".format(clamp))
            self.clamp = (lo, hi)
        self.hole_value, self.occluder_value = float(hole_value), float(occluder_value)
        self.per_frame = bool(per_frame)
        super().__init__(seed)
        if share_erase is not None and not isinstance(share_erase, FrameAugment):
            raise ValueError("share_erase takes the FrameAugment of the RGB frames; got {!r}".format(type(share_erase).__name__))
        self.share_erase = share_erase
        self.last_params = None     # device table of the last call: [0] the step used, then per stream count and 4 x (top, left, h, w)

    def hole_bounds(self, size):
        """hole_scale as pixel bounds (lo, hi) of a side of `size` pixels, 1 <= lo <= hi <= size"""
        lo = min(size, max(1, int(round(self.hole_scale[0] * size))))
        return lo, min(size, max(lo, int(round(self.hole_scale[1] * size))))

    def desc_fields(self, hs, ws, group=0):
        """the arguments of ops.depth_augment_desc for frames of hs x ws"""
        (hh_lo, hh_hi), (hw_lo, hw_hi) = self.hole_bounds(hs), self.hole_bounds(ws)
        return dict(seed=self.seed, n0=self.n[0], n1=self.n[1], n2=self.n[2], q=self.quant, inv_q=self.inv_quant, lo=self.clamp[0], hi=self.clamp[1],
                    drop_thresh=self.drop_thresh, hole_lo=self.holes[0], hole_hi=self.holes[1], hh_lo=hh_lo, hh_hi=hh_hi, hw_lo=hw_lo, hw_hi=hw_hi,
                    hole_value=self.hole_value, occluder_value=self.occluder_value, group=int(group))

    @staticmethod
    def check_depth(depth):
        """ValueError unless `depth` is a contiguous fp32 device tensor (B, Hs, Ws, 1) / (S, N, Hs, Ws, 1) or (B, 1, H, W) / (S, N, 1, H, W);
        -> (Hs, Ws)"""
        from ..ops import depth_frame_hw
        if not isinstance(depth, torch.Tensor) or depth.dtype != torch.float32:
            raise ValueError("DepthAugment takes fp32 depth frames; got {}".format(getattr(depth, "dtype", type(depth))))
        if depth.dim() not in (4, 5) or not depth.is_contiguous() or depth.numel() == 0:
            raise ValueError("DepthAugment takes depth frames (B, Hs, Ws, 1) / (S, N, Hs, Ws, 1) or (B, 1, H, W) / (S, N, 1, H, W), contiguous; got {}".format(
                tuple(depth.shape)))
        hw = depth_frame_hw(depth.shape)
        if not depth.is_cuda:
            raise ValueError("DepthAugment runs on the device only (there is no CPU path); got a {} tensor".format(depth.device))
        return hw

    def group_of(self, shape):
        """the `group` of a batch of `shape`: N for windows (S, N, ...) unless per_frame, else 0"""
        return int(shape[1]) if not self.per_frame and len(shape) == 5 else 0

    def shared_table(self, hs, ws, b, group):
        """(rgb_params, rgb_group) of the launch: the table share_erase's last call wrote, checked against this batch's geometry and
        grouping; (None, 0) without share_erase"""
        aug = self.share_erase
        if aug is None:
            return None, 0
        if aug.last_params is None:
            raise ValueError("DepthAugment(share_erase=...): the FrameAugment has not run yet -- augment the RGB frames of the batch first")
        seen = getattr(aug, "last_geometry", None)
        if seen != (int(hs), int(ws), int(b), int(group)):
            raise ValueError("DepthAugment(share_erase=...): the RGB augmentation saw (Hs, Ws, frames, group) = {!r}, the depth frames are {!r}: "
                             "the two must see the same geometry and grouping".format(seen, (int(hs), int(ws), int(b), int(group))))
        return aug.last_params, int(group)

    def __call__(self, depth, out=None):
        from .. import ops
        hs, ws = self.check_depth(depth)
        group = self.group_of(depth.shape)
        b = depth.numel() // (hs * ws)
        rgb_params, rgb_group = self.shared_table(hs, ws, b, group)
        state = self._device_state(depth.device)
        params = self._kept((b, group, depth.device), lambda: torch.empty(1 + ops.DEPTH_AUGMENT_ROW * (group or b), dtype=torch.int32, device=depth.device))
        out = ops.augment_depth_f32(depth, ops.depth_augment_desc(**self.desc_fields(hs, ws, group)), state, out=out, params=params,
                                    rgb_params=rgb_params, rgb_group=rgb_group)
        self.last_params = params
        return out



class MeasurementNoise(_DeviceStepCounter):
    """The measurement of the robot's own pose, x0bar = x0 + N(0, scale I) with the quaternion renormalised (what `refresh_data`
    draws on the host once per refresh, util/data_utils.py:162-167 of the reference), drawn on the device at EVERY call
    (rpe_measurement_noise; DESIGN.md "Measurement noise").  `scale` is a variance, as `noise_scale` is, or a sequence of 1..8
    variances: every lane then draws one of them per call, for its whole window.  `correlation` in [0, 1) is the AR(1) coefficient of
    the noise along the S timesteps of a window (0: white); it restarts with every window, stationary with unit variance.  The random
    numbers are a function of (seed, step); the step counter lives in device memory and every call advances it, also a call replayed
    from a captured graph.  Takes a contiguous fp32 device tensor (B, 7) -- lanes = rows -- or (S, N, 7), time-major.

        noise = MeasurementNoise([0.001, 0.01], correlation=0.5, seed=0)
        x0bar = noise(x0)                   # a new tensor; noise(x0, out=buf) writes buf (buf may be x0)
    """

    def __init__(self, scale=0.001, correlation=0.0, seed=0):
        from ..ops import measure_scales
        self.scales = measure_scales(scale)
        self.correlation = float(correlation)
        if not 0.0 <= self.correlation < 1.0:
            raise ValueError("correlation must lie in [0, 1); got {!r}".format(correlation))
        super().__init__(seed)
        self.last_picks = None      # device table of the last call: [0] the step used, then each lane's scale index

    @staticmethod
    def check_poses(x0):
        """ValueError unless `x0` is a contiguous fp32 device tensor (B, 7) or (S, N, 7); -> (S, N)"""
        if not isinstance(x0, torch.Tensor) or x0.dtype != torch.float32:
            raise ValueError("MeasurementNoise takes fp32 poses; got {}".format(getattr(x0, "dtype", type(x0))))
        if x0.dim() not in (2, 3) or x0.shape[-1] != 7 or not x0.is_contiguous() or x0.numel() == 0:
            raise ValueError("MeasurementNoise takes poses (B, 7) or (S, N, 7), contiguous; got {}".format(tuple(x0.shape)))
        if not x0.is_cuda:
            raise ValueError("MeasurementNoise runs on the device only (there is no CPU path); got a {} tensor".format(x0.device))
        return (1, x0.shape[0]) if x0.dim() == 2 else (x0.shape[0], x0.shape[1])

    def desc_fields(self, s, n):
        """the arguments of ops.measure_desc for S = s timesteps of N = n lanes"""
        return dict(seed=self.seed, S=int(s), N=int(n), scales=self.scales, correlation=self.correlation)

    def __call__(self, x0, out=None):
        from .. import ops
        s, n = self.check_poses(x0)
        if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.shape != x0.shape or out.device != x0.device
                                or not out.is_contiguous()):
            raise ValueError("MeasurementNoise: out must be a contiguous fp32 tensor of x0's shape on its device")
        desc = ops.measure_desc(**self.desc_fields(s, n))
        state = self._device_state(x0.device)
        picks = self._kept((n, x0.device), lambda: torch.zeros(1 + n, dtype=torch.int32, device=x0.device))
        out = ops.measurement_noise(x0, desc, state, picks=picks, out=out)
        self.last_picks = picks
        return out


def model_batch(batch, requires_sequence):
    """A time-major six-tuple (S, N, ...) as the model takes it: a model without a sequence walks S = 1 and takes the tensors without
    that dimension (the reference squeezes the leading batch-of-1 dim, util/learn_utils.py:141-149 there).  Views: the addresses stay."""
    return tuple(batch) if requires_sequence else tuple(None if t is None else t[0] for t in batch)


class TrainInputs:
    """The device stages between a dataset and the model in a train step, all optional, as ONE object that train() and GraphedTrainStep
    both build and call ("Input stages").  They run in one fixed order on the six-tuple
    (img, depth, x0bar, x0, x1, obj):

        sampler            draws the batch itself (its own buffers)
        measurement_noise  reads x0 (field 3), its result replaces x0bar (field 2)
        augment            reads the raw frames (field 0), its result replaces them
        depth_augment      reads the raw depth (field 1), its result replaces it

    The one constraint on the order: depth_augment comes after augment, because a DepthAugment(share_erase=augment) reads the table
    the RGB augmentation of the same step wrote.  Everything else is free -- each stage has a counter of its own and writes a tensor
    of its own -- and the remaining fields pass through as they are.  The stages are validated here, once, against the model and the
    dataset (only `use_depth`, and with a sampler `requires_sequence` / `sequence_length`, are read of the model)."""

    def __init__(self, model, dataset=None, sampler=None, measurement_noise=None, augment=None, depth_augment=None):
        if measurement_noise is not None and not isinstance(measurement_noise, MeasurementNoise):
            raise ValueError("measurement_noise=... takes a util.data_utils.MeasurementNoise; got {!r}".format(type(measurement_noise).__name__))
        if depth_augment is not None:
            if not isinstance(depth_augment, DepthAugment):
                raise ValueError("depth_augment=... takes a util.data_utils.DepthAugment; got {!r}".format(type(depth_augment).__name__))
            if not getattr(model, "use_depth", False):
                raise ValueError("depth_augment=... needs a model built with use_depth; {} does not read depth".format(type(model).__name__))
            if depth_augment.share_erase is not None and depth_augment.share_erase is not augment:
                raise ValueError("depth_augment.share_erase must be the FrameAugment given as augment=... to the same call: the occluder is shared "
                                 "with the RGB frames of the same step")
        if augment is not None and getattr(dataset, "frame_dtype", torch.uint8) != torch.uint8:
            raise ValueError("augment=... needs raw uint8 frames (RecordedEpisodeDataset); {} hands out {} images".format(
                type(dataset).__name__, dataset.frame_dtype))
        self.model, self.sampler = model, None
        self.measurement_noise, self.augment, self.depth_augment = measurement_noise, augment, depth_augment
        if sampler is not None:
            self.draw_from(sampler)

    def draw_from(self, sampler):
        """make `sampler` (a WindowSampler) the source of the batches (train() has none before its first refresh)"""
        want = self.model.sequence_length if self.model.requires_sequence else 1
        if sampler.sequence_length != want:
            raise ValueError("the model takes windows of {} timesteps; the sampler draws {}".format(want, sampler.sequence_length))
        self.sampler = sampler

    @property
    def _passes(self):
        return self.measurement_noise is None and self.augment is None and self.depth_augment is None

    @staticmethod
    def _depth(batch):
        if batch[1] is None:
            raise ValueError("depth_augment=... needs a batch with depth frames; this one has none")
        return batch[1]

    def fed_like(self, static):
        """-> the six-tuple a captured step feeds the model for the fixed inputs `static`: `static` with a new buffer in every slot a
        stage writes (`static` itself without one), after the stages' own checks of what they will read"""
        if self._passes:
            return static
        fed = list(static)
        if self.augment is not None:
            self.augment.check_frames(static[0])
            fed[0] = torch.empty_like(static[0])
        if self.measurement_noise is not None:
            self.measurement_noise.check_poses(static[3])
            fed[2] = torch.empty_like(static[3])
        if self.depth_augment is not None:
            self.depth_augment.check_depth(self._depth(static))
            fed[1] = torch.empty_like(static[1])
        return tuple(fed)

    def __call__(self, batch=None, out=None):
        """-> what the model is fed for `batch`.  With a sampler the batch is drawn here: pass None, or -- the captured step -- the
        views of the sampler's buffers that are to be read.  out: a six-tuple (`fed_like`) whose slots the stages write; without it
        every stage returns a new tensor and the batch's own are not written."""
        if self.sampler is not None:
            drawn = self.sampler()
            if batch is None:
                batch = model_batch(drawn, self.model.requires_sequence)
        if self._passes:
            return batch
        fed, out = list(batch), out or (None,) * 6
        if self.measurement_noise is not None:
            fed[2] = self.measurement_noise(batch[3].contiguous(), out=out[2])
        if self.augment is not None:
            fed[0] = self.augment(batch[0], out=out[0])
        if self.depth_augment is not None:   # after `augment`: the RGB table of this step exists
            fed[1] = self.depth_augment(self._depth(batch).contiguous(), out=out[1])
        return tuple(fed)



class FramePrefetcher:
    """Host -> device staging of raw simulator frames, double buffered.

    replaces: the per-tensor synchronous pageable `.cuda()` of util/learn_utils.py:130-138 fed by the CPU transform
    (util/data_utils.py:48-54).  `batches` yields tuples of CPU tensors; uint8 frame tensors stay uint8 -- 50 MB instead of
    154 MB of fp32 per 256 frames -- and are cropped / normalised on the device by the trunk (`rpe_stage_frames_u8`).  Every
    tensor goes through a pinned staging buffer and an asynchronous copy on a side stream into one of `depth` device slots;
    the consumer's stream waits for that copy only, so batch k+1 crosses PCIe while batch k trains.

        for frames, x0bar, target in FramePrefetcher(loader, device):
            loss = criterion(model(frames, None, x0bar), target)
    """

    def __init__(self, batches, device="cuda", depth=2):
        self.batches, self.device, self.depth = batches, torch.device(device), max(2, int(depth))
        self.stream = torch.cuda.Stream(device=self.device)
        self._pinned = [None] * self.depth   # per slot: list of pinned host buffers
        self._dev = [None] * self.depth      # per slot: list of device buffers
        self._ready = [None] * self.depth    # per slot: copy-finished event
        self._free = [None] * self.depth     # per slot: consumer-finished event (the slot may be overwritten after it)
        self._src_keep = [None] * self.depth   # per slot: the host tensors its last copy read

    def _stage(self, slot, batch):
        items = list(batch) if isinstance(batch, (tuple, list)) else [batch]
        if self._dev[slot] is None or len(self._dev[slot]) != len(items) or any(
                (d is None) != (t is None) or (t is not None and (d.shape != t.shape or d.dtype != t.dtype or
                                                                   ((self._pinned[slot][i] is None) != t.is_pinned())))
                for i, (d, t) in enumerate(zip(self._dev[slot], items))):
            self._pinned[slot] = [None if (t is None or t.is_pinned()) else torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in items]
            self._dev[slot] = [None if t is None else torch.empty(t.shape, dtype=t.dtype, device=self.device) for t in items]
        if self._free[slot] is not None:
            self.stream.wait_event(self._free[slot])      # the previous consumer of this slot is done with it
        # The slot's pinned staging buffers are the SOURCE of its previous asynchronous H2D copy, which may not even have
        # started yet (it queues behind `_free[slot]` on the copy stream while the training thread runs ahead of the GPU):
        # the host must not overwrite them before that copy has finished.
        if self._ready[slot] is not None and any(p is not None for p in self._pinned[slot]):
            self._ready[slot].synchronize()
        src = []
        for p, t in zip(self._pinned[slot], items):
            if t is None or t.is_pinned():
                src.append(t)                               # already page-locked (DataLoader(pin_memory=True)): DMA straight from it
            else:
                p.copy_(t)                                  # host memcpy into the pinned buffer (on the caller's thread: keep
                src.append(p)                               # loaders pinning, or this copy is what the GPU waits for)
        self._src_keep[slot] = src                          # sources stay alive until the slot is staged again
        with torch.cuda.stream(self.stream):
            for d, p in zip(self._dev[slot], src):
                if p is not None:
                    d.copy_(p, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._ready[slot] = ev

    def __iter__(self):
        it = iter(self.batches)
        slot, pending = 0, []
        try:
            for _ in range(self.depth - 1):
                self._stage(slot, next(it))
                pending.append(slot)
                slot = (slot + 1) % self.depth
        except StopIteration:
            pass
        while pending:
            cur = pending.pop(0)
            try:
                self._stage(slot, next(it))
                pending.append(slot)
                slot = (slot + 1) % self.depth
            except StopIteration:
                pass
            torch.cuda.current_stream(self.device).wait_event(self._ready[cur])
            yield tuple(self._dev[cur])
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(self.device))
            self._free[cur] = done
