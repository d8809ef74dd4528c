"""The pose overlay on the GPU: the drawing kernel against the numpy oracle (tests/_overlay_oracle.py) byte for byte from hand-built
integer draw lists, the projection kernel against the oracle's float64 for equality on screened rows, `render_episodes` end to end
against the oracle fed with the evaluation's own tensors, every side effect it must not have, and the script.  ResNet-18 models with
latent 32 and hidden 32, as tests/test_gpu_evaluate.py builds them."""
import functools

import numpy as np
import pytest
import torch

import _overlay_oracle as oo

pytestmark = pytest.mark.gpu

SHAPES = ((1, 7, 5), (3, 16, 16), (2, 33, 31), (4, 64, 48))      # (F, Hs, Ws): rows of 15, 48, 93 and 144 bytes
FPE, LIST = 2, 12                                                # frames per episode of the hand-built lists, and their length
ALPHAS = (0, 77, 256)
INV = oo.INVALID


def _ops():
    from rgb_proprioceptive_pose_estimator_amd import ops, torch_ops  # noqa: F401  (torch_ops: registers torch.ops.rpe.*)
    return ops


def _lu():
    from rgb_proprioceptive_pose_estimator_amd.util import learn_utils
    return learn_utils


def _guarded(nbytes, guard):
    """a device buffer of nbytes behind `guard` bytes of 0xA5 and in front of 64 more -> (whole buffer, the view between the guards)"""
    buf = torch.full((guard + nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[guard:guard + nbytes]


def _guards_intact(buf, guard, nbytes):
    b = buf.cpu().numpy()
    return bool((b[:guard] == 0xA5).all() and (b[guard + nbytes:] == 0xA5).all())


def _device_style(s):
    return _ops().overlay_style(s["rgb"], s["alpha_q8"], s["r_q4"], s["hw_q4"], s["axis_rgb"], s["trail"], s["trail_r_q4"])


# ---------------------------------------------------------------------------------------------------------------- drawing
def _pose(c, tips=((40, 0), (0, 40), (-28, -28))):
    """centre c (Q4) and three tips at the given offsets (None: no tip)"""
    return [list(c)] + [[INV, INV] if t is None else [c[0] + t[0], c[1] + t[1]] for t in tips]


def _draw_list(hs, ws):
    """LIST hand-built frames of three pose sets: (points (LIST, 3, 4, 2), bars (LIST, 2), {what: frame})"""
    W, H = 16 * (ws - 1), 16 * (hs - 1)
    mid = (W // 2 + 3, H // 2 - 5)
    none = [[INV, INV]] * 4
    scenes = [
        ("inside", [_pose(mid), none, none]),
        ("corners", [_pose((0, 0)), _pose((W, H), ((-40, 0), (0, -40), None)), none]),
        ("left_top", [_pose((-16, mid[1])), _pose((mid[0], -16)), none]),
        ("right_bottom", [_pose((W + 16, mid[1])), _pose((mid[0], H + 16)), none]),
        ("outside", [_pose((W + 16 * 40, mid[1])), _pose((mid[0], -16 * 30)), _pose((-16 * 50, -16 * 50))]),
        ("sentinels", [[[INV, INV]] + _pose(mid)[1:], _pose((mid[0] + 24, mid[1]), (None, (0, 40), None)), [[mid[0], INV]] + _pose(mid)[1:]]),
        ("zero_axis", [_pose(mid, ((0, 0), (0, 0), (33, -9))), none, none]),
        ("long_axis", [_pose(mid, ((oo.AXIS_Q4 + 1, 0), (0, -oo.AXIS_Q4 - 1), (oo.AXIS_Q4, -oo.AXIS_Q4))), _pose((oo.CLAMP_Q4 + 1, mid[1])), none]),
        ("overlap", [_pose(mid), _pose((mid[0] + 20, mid[1] + 12)), _pose((mid[0] - 9, mid[1] + 30), ((64, 8), None, (-8, -64)))]),
        ("overlap2", [_pose((mid[0] + 30, mid[1])), _pose((mid[0] + 30, mid[1])), _pose((mid[0] + 31, mid[1] + 1))]),
        ("edge_axes", [_pose((W - 8, 8), ((120, 0), (0, -120), (-120, 120))), none, _pose((8, H - 8), ((-120, 0), (0, 120), (120, -120)))]),
        ("far_trail", [_pose((W // 4, H // 4)), _pose((3 * W // 4, H // 4)), _pose((W // 2, 3 * H // 4))]),
    ]
    assert len(scenes) == LIST
    points = np.array([s for _, s in scenes], dtype=np.int64).astype(np.int32)
    lengths = (0, ws // 2, ws, ws + 7, -3, 1)
    bars = np.array([[lengths[i % 6], lengths[(i + 2) % 6]] for i in range(LIST)], dtype=np.int32)
    return points, bars, {name: i for i, (name, _) in enumerate(scenes)}


def _styles(alpha):
    """set 0: a trail of N = 3 (longer than an episode of FPE = 2); set 1: always half transparent, so that the order of overlapping sets
    shows; set 2: a trail of 1 and the widest shapes"""
    return [oo.style((250, 10, 20), alpha, 52, 18, ((255, 0, 0), (0, 255, 0), (0, 0, 255)), 3, 30),
            oo.style((10, 240, 30), 200, 40, 25, ((200, 200, 0), (0, 200, 200), (200, 0, 200)), 0, 0),
            oo.style((20, 30, 245), alpha, 70, 9, ((90, 0, 0), (0, 90, 0), (0, 0, 90)), 1, 44)]


def _bar_px(hs):
    return max(1, hs // 8)


BAR_RGB = ((9, 8, 7), (200, 100, 50))


@functools.lru_cache(maxsize=None)
def _draw_case(F, hs, ws):
    """frames, the draw list and the oracle's pictures of one shape, computed once and shared by the three alignments"""
    rng = np.random.default_rng(F * 10000 + hs * 100 + ws)
    frames = rng.integers(0, 256, (LIST, hs, ws, 3), dtype=np.uint8)
    points, bars, where = _draw_list(hs, ws)
    want = {}
    for alpha in ALPHAS:
        for flip in (False, True):
            for bar_px in (0, _bar_px(hs)):
                want[alpha, flip, bar_px] = oo.draw_poses(frames, points, bars, _styles(alpha), frames_per_episode=FPE, first=0, bar_px=bar_px, bar_rgb=BAR_RGB, flip=flip)
    for a in (frames, points, bars, *want.values()):
        a.setflags(write=False)
    return frames, points, bars, where, want


@pytest.mark.parametrize("guard", [16, 4, 3])      # the destination's alignment picks 16-byte, 4-byte or single-byte units
@pytest.mark.parametrize("F,hs,ws", SHAPES)
def test_draw_equals_the_oracle(F, hs, ws, guard):
    ops = _ops()
    frames, points, bars, where, want = _draw_case(F, hs, ws)
    dev_frames, dev_points, dev_bars = (torch.from_numpy(a.copy()).cuda() for a in (frames, points, bars))
    n = F * hs * ws * 3
    for (alpha, flip, bar_px), pictures in want.items():
        styles = [_device_style(s) for s in _styles(alpha)]
        for first in range(0, LIST, F):
            buf, view = _guarded(n, guard)
            got = ops.draw_poses_u8(dev_frames[first:first + F], dev_points, dev_bars, styles, frames_per_episode=FPE, first=first, bar_px=bar_px,
                                    bar_colours=BAR_RGB, flip=flip, out=view.view(F, hs, ws, 3))
            assert got.data_ptr() == view.data_ptr()
            assert np.array_equal(got.cpu().numpy(), pictures[first:first + F]), (alpha, flip, bar_px, first)
            assert _guards_intact(buf, guard, n), (alpha, flip, bar_px, first)
    # what the oracle's pictures must show, so that the comparison above means what it says
    plain, mirrored = want[256, False, 0], want[256, True, 0]
    o = where["outside"]
    assert np.array_equal(plain[o], frames[o]) and np.array_equal(mirrored[o], frames[o, ::-1])          # nothing inside: identical up to the flip
    assert np.array_equal(want[0, False, 0][where["inside"]], frames[where["inside"]])                    # alpha 0 draws nothing
    if hs >= 16:
        assert not np.array_equal(plain[where["inside"]], frames[where["inside"]])
        # FPE = 2: frame 2 starts the second episode and shows nothing of frames 0 and 1 (set 0 has N = 3); frame 1 shows frame 0's centres
        cleared = points.copy()
        cleared[:2] = INV
        alone = oo.draw_poses(frames[2:3], cleared, bars, _styles(256), frames_per_episode=FPE, first=2)
        assert np.array_equal(alone[0], plain[2])
        no_trail = [dict(s, trail=0) for s in _styles(256)]
        assert not np.array_equal(oo.draw_poses(frames[1:2], points, bars, no_trail, frames_per_episode=FPE, first=1)[0], plain[1])
        # the order of two overlapping sets shows: the same shapes, sets 0 and 1 drawn the other way round
        ov = where["overlap"]
        swapped = points.copy()
        swapped[ov, [0, 1]] = points[ov, [1, 0]]
        st = _styles(256)
        assert not np.array_equal(oo.draw_poses(frames[ov:ov + 1], swapped, bars, [st[1], st[0], st[2]], frames_per_episode=1, first=ov)[0],
                                  oo.draw_poses(frames[ov:ov + 1], points, bars, st, frames_per_episode=1, first=ov)[0])
    # the dispatcher's entry is the same launch
    styles = _styles(77)
    flat = [v for s in styles for v in ops.overlay_style_to_list(_device_style(s))]
    bp = _bar_px(hs)
    assert np.array_equal(torch.ops.rpe.draw_poses_u8(dev_frames[:F], dev_points, dev_bars, flat, FPE, 0, bp, [c for rgb in BAR_RGB for c in rgb], True).cpu().numpy(),
                          want[77, True, bp][:F])


def test_draw_a_list_with_nothing_inside_is_a_copy():
    """every unit size, flip on and off, two tiles per frame with a partial last one: sentinel and outside points only"""
    ops = _ops()
    hs, ws = 72, 80                                # rows of 240 bytes; 17280 bytes a frame: 1080 16-byte units
    rng = np.random.default_rng(1)
    frames = torch.from_numpy(rng.integers(0, 256, (3, hs, ws, 3), dtype=np.uint8)).cuda()
    points = torch.full((3, 2, 4, 2), INV, dtype=torch.int32)
    points[1, 0] = torch.tensor(_pose((16 * 200, 16 * 10)))
    points[2, 1] = torch.tensor(_pose((-16 * 40, 16 * 10)))
    bars = torch.zeros((3, 2), dtype=torch.int32)
    styles = [_device_style(oo.style(trail=2)), _device_style(oo.style(trail=0))]
    for guard in (16, 4, 3):
        for flip in (False, True):
            buf, view = _guarded(frames.numel(), guard)
            got = ops.draw_poses_u8(frames, points.cuda(), bars.cuda(), styles, frames_per_episode=3, flip=flip, out=view.view(3, hs, ws, 3))
            assert torch.equal(got, frames.flip(1) if flip else frames) and _guards_intact(buf, guard, frames.numel()), (guard, flip)


# ---------------------------------------------------------------------------------------------------------------- projection
WIDTH, POS_FULL, ORI_FULL, AXIS_LEN = 640, 0.125, 0.5, 0.05     # (the full-scale values are powers of two: err = full gives exactly WIDTH)


def _cameras():
    K = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])
    c, s = np.cos(0.3), np.sin(0.3)
    R0, t0 = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.array([[1, 0, 0], [0, np.cos(0.2), -np.sin(0.2)], [0, np.sin(0.2), np.cos(0.2)]]), np.array([0.1, -0.05, 0.4])
    R1, t1 = np.diag([1.0, -1.0, -1.0]), np.array([0.0, 0.0, 2.0])          # looking down from z = 2: w = 2 - z, exactly
    return np.stack([K @ np.concatenate([R, t[:, None]], 1) for R, t in ((R0, t0), (R1, t1))]), ((R0, t0), (R1, t1))


def _random_frame(rng, G, extr):
    """G poses in front of one of the two cameras, unnormalised quaternions, two errors -> (poses (G, 7), camera number, (pos_err, ori_err))"""
    ci = int(rng.integers(0, 2))
    R, t = extr[ci]
    Xc = np.stack([rng.uniform(-0.5, 0.5, G), rng.uniform(-0.4, 0.4, G), rng.uniform(0.8, 2.5, G)], 1)
    X = (Xc - t) @ R                                                          # R^T (Xc - t)
    q = rng.normal(size=(G, 4)) * rng.uniform(0.2, 3.0, (G, 1))
    return np.concatenate([X, q], 1).astype(np.float32), ci, (np.float32(rng.uniform(0, 0.2)), np.float32(rng.uniform(0, 0.7)))


def _near_integer(v):
    return abs(v - np.round(v)) < 1e-6


def _flagged(detail):
    """whether the floor of a value the oracle computed for this frame could fall either way within 1e-6: a 16 u + 0.5 inside the clamp, a
    bar value inside (0, WIDTH), or a w within 1e-6 of the near threshold"""
    pts, barv = detail
    for a, b, w in pts:
        if np.isfinite(w) and abs(w - oo.NEAR) < 1e-6:
            return True
        if np.isfinite(w) and w > oo.NEAR:
            if any(np.isfinite(x) and abs(x) <= oo.CLAMP_Q4 + 1 and _near_integer(x) for x in (a, b)):
                return True
    return any(np.isfinite(v) and 0 < v < WIDTH and _near_integer(v) for v in barv)


@functools.lru_cache(maxsize=None)
def _projection_case(n, G):
    """n screened frames with the special rows planted as far as n allows -> (poses, cam, cam_index, pos_err, ori_err, {name: row}, want)"""
    rng = np.random.default_rng(1000 * n + G)
    cam, extr = _cameras()
    rows, redrawn = [], 0
    for _ in range(n):
        for attempt in range(10):
            poses, ci, errs = _random_frame(rng, G, extr)
            detail = []
            oo.project_poses(poses[None], cam, [ci], AXIS_LEN, [errs[0]], [errs[1]], POS_FULL, ORI_FULL, WIDTH, detail)
            if not _flagged(detail[0]):
                break
            redrawn += 1
        else:
            raise AssertionError("ten draws in a row were screened out")
        rows.append((poses, ci, errs))
    assert redrawn < 0.01 * n, redrawn
    poses = np.stack([r[0] for r in rows])
    cam_index = np.array([r[1] for r in rows], dtype=np.int32)
    pos_err, ori_err = np.array([r[2][0] for r in rows], dtype=np.float32), np.array([r[2][1] for r in rows], dtype=np.float32)
    down = lambda x, y, z: (x, y, z)                                          # world = camera 1's (x, -y, 2 - z): given in world coordinates
    special = {
        "behind": (1, down(0.1, 0.1, 3.0), None, None),                       # w = 2 - 3
        "threshold": (1, down(0.25, -0.125, 2.0 - oo.NEAR), None, None),      # w = 2^-10 exactly (0 x + 0 y is 0, 2 - z is exact): invalid
        "above_threshold": (1, down(0.0, 0.0, 2.0 - 2 * oo.NEAR), None, None),
        "nan": (0, (np.nan, 0.0, 1.0), None, None),
        "inf": (1, (0.1, np.inf, 1.0), None, None),
        "nan_quat": (1, (0.1, 0.1, 1.0), (0.0, np.nan, 0.0, 1.0), None),
        "zero_quat": (1, (0.1, 0.1, 1.0), (0.0, 0.0, 0.0, 0.0), None),
        "long_quat": (1, (0.1, 0.1, 1.0), (30.0, -40.0, 0.0, 120.0), None),
        "clamp": (1, (4000.0, -4000.0, 1.0), None, None),
        "close": (1, (0.001, 0.001, 1.99), (0.0, 0.0, 0.0, 1.0), None),       # 1 cm under the camera: the z tip behind it, the others 2500 px away
        "err_zero": (1, (0.2, 0.1, 1.0), None, (0.0, 0.0)),
        "err_full": (1, (0.2, 0.1, 1.0), None, (POS_FULL, ORI_FULL)),
        "err_over": (1, (0.2, 0.1, 1.0), None, (7.0, np.inf)),
        "err_nan": (1, (0.2, 0.1, 1.0), None, (np.nan, np.nan)),
        "bad_camera": (7, (0.2, 0.1, 1.0), None, None),
    }
    where = {}
    for i, (name, (ci, X, q, errs)) in enumerate(special.items()):
        at = 2 * i                                                            # every special row has random neighbours
        if at < n:
            poses[at, 0, :3] = X
            if q is not None:
                poses[at, 0, 3:] = q
            cam_index[at] = ci
            if errs is not None:
                pos_err[at], ori_err[at] = errs
            where[name] = at
    detail = []
    want = oo.project_poses(poses, cam, cam_index, AXIS_LEN, pos_err, ori_err, POS_FULL, ORI_FULL, WIDTH, detail)
    # the planted rows are exact by construction where they sit on a boundary (w = 2^-10, err / full = 0 or 1); nowhere else may a floor hang
    # on the last bits
    for name, at in where.items():
        if name == "threshold":
            assert detail[at][0][0][2] == oo.NEAR
        elif name in ("err_zero", "err_full"):
            assert detail[at][1] == ([0.0, 0.0] if name == "err_zero" else [float(WIDTH), float(WIDTH)])
        else:
            assert not _flagged(detail[at]), name
    for a in (poses, cam, cam_index, pos_err, ori_err, *want):
        a.setflags(write=False)
    return poses, cam, cam_index, pos_err, ori_err, where, want


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_project_equals_the_float64_oracle(n, G):
    ops = _ops()
    poses, cam, cam_index, pos_err, ori_err, where, (want_points, want_bars) = _projection_case(n, G)
    dev = lambda a: torch.from_numpy(a.copy()).cuda()
    points, bars = ops.project_poses(dev(poses), dev(cam), dev(cam_index), AXIS_LEN, dev(pos_err), dev(ori_err), POS_FULL, ORI_FULL, WIDTH)
    points, bars = points.cpu().numpy(), bars.cpu().numpy()
    assert points.shape == (n, G, 4, 2) and bars.shape == (n, 2) and points.dtype == bars.dtype == np.int32
    bad = np.argwhere(points != want_points)
    assert bad.size == 0, (bad[:5], points[tuple(bad[0][:2])], want_points[tuple(bad[0][:2])])
    assert np.array_equal(bars, want_bars)
    # what the planted rows must show (on the oracle's side: the device equals it)
    w = want_points
    assert (w[where["behind"], 0] == INV).all()
    if n > 30:
        assert (w[where["threshold"], 0] == INV).all() and (w[where["above_threshold"], 0, 0] != INV).all()
        assert (w[where["nan"], 0] == INV).all() and (w[where["inf"], 0] == INV).all() and (w[where["bad_camera"]] == INV).all()
        for name in ("nan_quat", "zero_quat"):
            assert (w[where[name], 0, 0] != INV).all() and (w[where[name], 0, 1:] == INV).all()
        assert (w[where["long_quat"], 0] != INV).all()
        assert tuple(w[where["clamp"], 0, 0]) == (oo.CLAMP_Q4, oo.CLAMP_Q4)
        assert (w[where["close"], 0, 0] != INV).all() and (w[where["close"], 0, 1:] == INV).all()
        assert want_bars[where["err_zero"]].tolist() == [0, 0] and want_bars[where["err_full"]].tolist() == [WIDTH, WIDTH]
        assert want_bars[where["err_over"]].tolist() == [WIDTH, WIDTH] and want_bars[where["err_nan"]].tolist() == [0, 0]
        random_rows = np.setdiff1d(np.arange(n), list(where.values()))
        assert (w[random_rows] != INV).all()                                                          # the random rows are in front of their camera, axes and all
    # without errors: no bars; and the dispatcher's entry is the same launch
    p2, b2 = ops.project_poses(dev(poses), dev(cam), dev(cam_index), AXIS_LEN)
    assert np.array_equal(p2.cpu().numpy(), want_points) and not b2.any().item()
    p3, b3 = torch.ops.rpe.project_poses(dev(poses), dev(cam), dev(cam_index), AXIS_LEN, dev(pos_err), dev(ori_err), POS_FULL, ORI_FULL, WIDTH)
    assert np.array_equal(p3.cpu().numpy(), want_points) and np.array_equal(b3.cpu().numpy(), want_bars)


# ---------------------------------------------------------------------------------------------------------------- end to end
E, T, HS, WS = 2, 3, 32, 40
PARAMS = {"camera_name": "frontview", "noise_scale": 0.001}
CAMERA = np.array([[30.0, 0, 8, 12], [0, 26.0, 6, 9], [0, 0, 1.0, 1.5]])     # the recorded poses lie in [0, 1]^3: inside the 32 x 40 frame


def _poses(rng, e, t):
    q = rng.normal(size=(e, t, 4))
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    return np.concatenate([rng.random((e, t, 3)), np.where(q[..., 3:] < 0, -q, q)], -1).astype(np.float32)


def _episode_file(tmp_path, two_arm=False, seed=0):
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset
    rng = np.random.default_rng(seed)
    return RecordedEpisodeDataset.save(str(tmp_path / ("episodes_%d.npz" % two_arm)), env_name="TwoArmLift" if two_arm else "Lift",
                                       imgs=rng.integers(0, 256, (E, T, HS, WS, 3), dtype=np.uint8), true_self=_poses(rng, E, T),
                                       true_other=_poses(rng, E, T) if two_arm else None, true_obj=_poses(rng, E, T))


def _model(kind, seed=5):
    from rgb_proprioceptive_pose_estimator_amd import models as M
    torch.manual_seed(seed)
    if kind == "td":
        m = M.TemporallyDependentStateEstimator(32, 32, 18, 32, 2, 0.1, False, (9,), False, False, compute_dtype=torch.float32)
    else:
        m = M.NaiveObjectStateEstimator("cube", [32], 18, 32, False, (9,), False, False, False, compute_dtype=torch.float32)
    return m.cuda()


def _oracle_render(ev, frames, camera, draw, lu, *, axis_len=0.05, radius=4.0, axis_width=1.5, trail=8, bars=True, pos_full=0.1, ori_full=0.5, alpha=1.0, flip=True):
    """render_episodes restated on the oracle, from the evaluation's tensors"""
    from rgb_proprioceptive_pose_estimator_amd import ops
    src = {"truth": ev.truth, "estimate": ev.poses, "measurement": ev.measurements}
    e, t = ev.truth.shape[:2]
    poses = np.stack([src[s].cpu().numpy().reshape(e * t, 7) for s in draw], 1)
    cam = np.asarray(camera, dtype=np.float64)
    per_episode = cam.ndim == 3
    cam = cam.reshape(-1, cam.shape[-2], 4)[:, :3]
    cam_index = np.arange(e * t) // t if per_episode else np.zeros(e * t, dtype=np.int64)
    hs, ws = frames.shape[2:4]
    bar_px = max(1, hs // 32) if bars else 0
    pe, oe = (ev.pos_err.cpu().numpy().reshape(-1), ev.ori_err.cpu().numpy().reshape(-1)) if bars else (None, None)
    points, bar_len = oo.project_poses(poses, cam, cam_index, axis_len, pe, oe, pos_full, ori_full, ws if bars else 0)
    r_q4 = int(round(radius * 16))
    styles = [oo.style(lu.OVERLAY_COLOURS[s], int(round(alpha * 256)), r_q4, int(round(axis_width * 8)), ops.OVERLAY_AXIS_COLOURS, trail, r_q4 // 2) for s in draw]
    bar_rgb = (lu.OVERLAY_COLOURS["estimate"] if "estimate" in draw else lu.OVERLAY_COLOURS[draw[0]], lu.OVERLAY_ORI_BAR_COLOUR)
    out = oo.draw_poses(np.asarray(frames).reshape(e * t, hs, ws, 3), points, bar_len, styles, frames_per_episode=t, first=0, bar_px=bar_px, bar_rgb=bar_rgb, flip=flip)
    return out.reshape(e, t, hs, ws, 3)


def _snapshot(model, ev):
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    carried = {k: tuple(x.clone() for x in hc) for k, hc in getattr(model, "_carried", {}).items()}
    tensors = {k: getattr(ev, k).clone() for k in ("outputs", "poses", "pos_err", "ori_err", "truth", "measurements")}
    return state, carried, tensors, (model.training, model.rollout), ev.stats.copy()


def _unchanged(model, ev, snap):
    state, carried, tensors, flags, stats = snap
    now = model.state_dict()
    raw = lambda a: a.reshape(-1).view(torch.uint8) if a.dtype.is_floating_point else a      # (bytes: a NaN equals itself)
    same = lambda a, b: torch.equal(raw(a), raw(b))
    assert list(now) == list(state) and all(same(now[k].contiguous(), state[k].contiguous()) for k in state)
    now_c = getattr(model, "_carried", {})
    assert list(now_c) == list(carried) and all(same(x, y) for k in carried for x, y in zip(now_c[k], carried[k]))
    assert all(same(getattr(ev, k).contiguous(), v.contiguous()) for k, v in tensors.items())
    assert (model.training, model.rollout) == flags and np.array_equal(ev.stats, stats, equal_nan=True)


@pytest.mark.parametrize("kind", ["td", "no"])
def test_render_episodes_equals_the_oracle(kind, tmp_path):
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset
    lu = _lu()
    two_arm = kind == "td"
    ds = RecordedEpisodeDataset(_episode_file(tmp_path, two_arm), obj_name=None if two_arm else "cube")
    model = _model(kind).train()
    ev = lu.evaluate_episodes(model, ds, E, PARAMS, max_frames=4)
    frames = ds.data["imgs"]
    assert tuple(frames.shape) == (E, T, HS, WS, 3) and not frames.is_cuda
    snap = _snapshot(model, ev)
    got = lu.render_episodes(ev, frames, CAMERA)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (E, T, HS, WS, 3)
    want = _oracle_render(ev, frames.numpy(), CAMERA, ("truth", "estimate"), lu)
    assert np.array_equal(got.cpu().numpy(), want)
    assert not np.array_equal(want, frames.numpy()[:, :, ::-1])                    # (something was drawn)
    # frames on the host or on the device, as tensor or array, in chunks of 1, 4 and 64, into a destination: the same bytes
    dev_frames = frames.cuda()
    for fr, chunk in ((frames, 1), (frames, 4), (frames.numpy(), 64), (dev_frames, 1), (dev_frames, 4), (dev_frames, 64)):
        assert torch.equal(lu.render_episodes(ev, fr, CAMERA, chunk=chunk), got), chunk
    out = torch.zeros((E, T, HS, WS, 3), dtype=torch.uint8, device="cuda")
    assert lu.render_episodes(ev, dev_frames, CAMERA, out=out) is out and torch.equal(out, got)
    with pytest.raises(ValueError, match="overlaps"):
        lu.render_episodes(ev, dev_frames, CAMERA, out=dev_frames)
    # the other options, and one camera per episode given as (E, 4, 4) in upright coordinates and converted
    opts = dict(draw=("measurement", "estimate", "truth"), axis_len=0.2, radius=2.5, axis_width=3.0, trail=1, bars=False, alpha=0.3, flip=False)
    P4 = np.stack([np.vstack([CAMERA, [0, 0, 0, 1.0]]), np.vstack([CAMERA * 1.25, [0, 0, 0, 1.0]])])
    stored = lu.flip_camera_rows(P4, HS)
    got2 = lu.render_episodes(ev, dev_frames, torch.from_numpy(stored), **opts)
    want2 = _oracle_render(ev, frames.numpy(), stored, opts["draw"], lu, **{k: v for k, v in opts.items() if k != "draw"})
    assert np.array_equal(got2.cpu().numpy(), want2)
    _unchanged(model, ev, snap)
    assert torch.equal(dev_frames.cpu(), frames)


def test_rollout_script_writes_the_video(tmp_path, capsys):
    from PIL import Image
    from rgb_proprioceptive_pose_estimator_amd.scripts.rollout import main
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset
    lu = _lu()
    path = _episode_file(tmp_path)
    cam = str(tmp_path / "camera.npy")
    np.save(cam, CAMERA)
    common = ["--model", "no", "--latent_dim", "32", "--hidden_dim", "32", "--obj_name", "cube", "--dtype", "f32", "--episodes", path,
              "--n_episodes", str(E), "--camera_matrix", cam]
    outs, gif, npy, npy2, npy3 = str(tmp_path / "outs.npy"), str(tmp_path / "v.gif"), str(tmp_path / "v.npy"), str(tmp_path / "v2.npy"), str(tmp_path / "v3.npy")
    res = main(common + ["--batched", "--video_out", npy, "--out", outs])
    assert "wrote %d frames" % (E * T) in capsys.readouterr().out
    video = np.load(npy)
    assert video.dtype == np.uint8 and video.shape == (E * T, HS, WS, 3)
    ds = RecordedEpisodeDataset(path, obj_name="cube")
    ds.refresh_data(E, None, 0.001)
    assert np.array_equal(video, lu.render_episodes(res, ds.data["imgs"], CAMERA).cpu().numpy().reshape(E * T, HS, WS, 3))
    main(common + ["--video_out", gif, "--out", outs])                                  # (the video flags imply --batched)
    with Image.open(gif) as im:
        assert im.n_frames == E * T and im.size == (WS, HS)
    # the reference's second pass: the estimates come from the first run's --out file, the model does not run
    main(common + ["--video_out", npy2, "--model_outputs_file", outs])
    assert open(npy2, "rb").read() == open(npy, "rb").read()
    # positions only, as the reference writes them: discs without axes; and the other flags reach render_episodes
    pos_only = str(tmp_path / "positions.npy")
    np.save(pos_only, np.load(outs)[:, :3])
    main(common + ["--video_out", npy3, "--model_outputs_file", pos_only, "--video_episodes", "1", "--video_draw", "estimate", "--no_flip", "--no_bars",
                   "--trail", "0", "--axis_len", "0.1"])
    short = np.load(npy3)
    assert short.shape == (T, HS, WS, 3)
    ev = types_namespace(poses=torch.cat([torch.from_numpy(np.load(outs)[:T, :3]), torch.zeros(T, 4)], 1).reshape(1, T, 7).cuda(), truth=res.truth[:1],
                         measurements=None, pos_err=res.pos_err[:1], ori_err=res.ori_err[:1], noise_scales=None)
    want = _oracle_render(ev, ds.data["imgs"][:1].numpy(), CAMERA, ("estimate",), lu, axis_len=0.1, trail=0, bars=False, flip=False)
    assert np.array_equal(short, want.reshape(T, HS, WS, 3))


def types_namespace(**kw):
    import types
    return types.SimpleNamespace(**kw)
