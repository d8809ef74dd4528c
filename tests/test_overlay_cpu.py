"""CPU side of the pose overlay: the numpy oracle's own properties (tests/_overlay_oracle.py -- the kernels are compared with it for
equality in tests/test_gpu_overlay.py), flip_camera_rows, the C ABI's declarations and refusals, the dispatcher entries, the argument
checks of render_episodes / write_video and the script's flags."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import _overlay_oracle as oo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("rpe_project_poses", "rpe_draw_poses_u8")


def _lu():
    from rgb_proprioceptive_pose_estimator_amd.util import learn_utils
    return learn_utils


# -- the oracle -------------------------------------------------------------------------------------------------------------------

def test_disc_area_and_symmetry():
    hs = ws = 21
    c = 16 * 10                                         # centred on pixel (10, 10)
    cov = oo.disc_cover(hs, ws, c, c, 16 * 5)
    area = cov.sum() / 4.0
    assert abs(area - np.pi * 25) <= 0.02 * np.pi * 25, area
    assert np.array_equal(cov, cov[::-1]) and np.array_equal(cov, cov[:, ::-1]) and np.array_equal(cov, cov.T)
    assert cov.max() == 4 and cov[0].max() == 0
    assert oo.disc_cover(hs, ws, c, c, 0).sum() == 0   # no subsample lies on a pixel centre


@pytest.mark.parametrize("tip", [(16 * 30, 16 * 12), (16 * 12 + 5, 16 * 33 - 7), (16 * 31 + 3, 16 * 29 + 9), (16 * 2, 16 * 3)])
def test_capsule_area(tip):
    hs = ws = 48
    cu, cv, hw = 16 * 14 + 3, 16 * 15 - 2, 40           # half-width 2.5 px
    cov = oo.capsule_cover(hs, ws, cu, cv, tip[0], tip[1], hw)
    length = np.hypot(tip[0] - cu, tip[1] - cv) / 16.0
    want = 2 * (hw / 16.0) * length + np.pi * (hw / 16.0) ** 2
    assert abs(cov.sum() / 4.0 - want) <= 0.02 * want, (cov.sum() / 4.0, want)
    # a zero-length capsule is the disc of its half-width
    assert np.array_equal(oo.capsule_cover(hs, ws, cu, cv, cu, cv, hw), oo.disc_cover(hs, ws, cu, cv, hw))


def test_zero_coverage_keeps_the_bytes():
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (2, 9, 11, 3), dtype=np.uint8)
    img = frames[0].astype(np.int64)
    oo.blend(img, (1, 2, 3), np.zeros((9, 11), dtype=np.int64))
    assert np.array_equal(img, frames[0])
    full = frames[0].astype(np.int64)
    oo.blend(full, (1, 2, 3), np.full((9, 11), 1024, dtype=np.int64))
    assert (full == np.array([1, 2, 3])).all()
    pts = np.full((2, 2, 4, 2), oo.INVALID, dtype=np.int32)
    pts[1, 0, 0] = (16 * 400, 16 * 3)                   # outside the frame
    pts[1, 1, 0] = (16 * 5, 16 * 4)
    styles = [oo.style(), oo.style(alpha_q8=0, trail=1)]     # ... and a set of no opacity
    bars = np.zeros((2, 2), dtype=np.int32)
    assert np.array_equal(oo.draw_poses(frames, pts, bars, styles, frames_per_episode=2), frames)
    assert np.array_equal(oo.draw_poses(frames, pts, bars, styles, frames_per_episode=2, flip=True), frames[:, ::-1])


def test_int64_bound_at_the_extreme_clamps():
    """the longest axis, the widest half-width, the farthest subsample behind the box test: the oracle's asserts hold and the products are
    what the kernel's comment says"""
    assert oo.V_MAX == 2 ** 13 + 2 ** 8 + 8 and oo.DOT_MAX < 2 ** 28 and oo.DOT_MAX ** 2 < 2 ** 56
    assert oo.MAX_RADIUS_Q4 ** 2 * 2 * oo.AXIS_Q4 ** 2 == 2 ** 43
    hs, ws = 530, 530
    for c, t in (((0, 0), (oo.AXIS_Q4, oo.AXIS_Q4)), ((oo.AXIS_Q4, 0), (0, oo.AXIS_Q4)), ((-oo.CLAMP_Q4, -oo.CLAMP_Q4), (-oo.CLAMP_Q4 + oo.AXIS_Q4, -oo.CLAMP_Q4)),
                 ((oo.CLAMP_Q4, oo.CLAMP_Q4), (oo.CLAMP_Q4 - oo.AXIS_Q4, oo.CLAMP_Q4 - oo.AXIS_Q4))):
        cov = oo.capsule_cover(hs, ws, c[0], c[1], t[0], t[1], oo.MAX_RADIUS_Q4)       # (asserts inside)
        assert cov.max() <= 4
    assert oo.capsule_cover(hs, ws, 0, 0, oo.AXIS_Q4, oo.AXIS_Q4, oo.MAX_RADIUS_Q4).sum() > 0
    with pytest.raises(AssertionError):
        oo.capsule_cover(8, 8, 0, 0, oo.AXIS_Q4 + 1, 0, 1)
    assert not oo.axis_ok(0, 0, oo.AXIS_Q4 + 1, 0) and oo.axis_ok(0, 0, oo.AXIS_Q4, -oo.AXIS_Q4)
    assert not oo.point_ok(oo.CLAMP_Q4 + 1, 0) and not oo.point_ok(0, oo.INVALID) and oo.point_ok(-oo.CLAMP_Q4, oo.CLAMP_Q4)


def test_projection_rules_of_the_oracle():
    P = np.array([[100.0, 0, 20, 0], [0, 100.0, 16, 0], [0, 0, 1.0, 0]])
    eye = np.float32([0, 0, 0, 1])
    poses = np.zeros((5, 1, 7), dtype=np.float32)
    poses[:, 0, 3:] = eye
    poses[0, 0, :3] = (0.1, -0.05, 2.0)
    poses[1, 0, :3] = (0.1, -0.05, -2.0)               # behind
    poses[2, 0, :3] = (0.1, -0.05, oo.NEAR)            # at the threshold: invalid
    poses[3, 0, :3] = (np.nan, 0, 2.0)
    poses[4, 0, :3] = (0.1, -0.05, 2.0)
    poses[4, 0, 3:] = 0                                 # no orientation: a centre without tips
    pts, bars = oo.project_poses(poses, P[None], np.zeros(5, dtype=np.int32), 0.1, np.float32([0, 0.05, 0.1, np.nan, 7]), np.float32([0.25] * 5), 0.1, 0.5, 40)
    assert tuple(pts[0, 0, 0]) == (16 * 25, int(np.floor(16 * 13.5 + 0.5)))
    assert tuple(pts[0, 0, 1]) == (16 * 30, 16 * 13 + 8) and tuple(pts[0, 0, 2]) == (16 * 25, 16 * 18 + 8)     # x and y axes: 0.1 m = 5 px
    assert (pts[1:4] == oo.INVALID).all() and tuple(pts[4, 0, 0]) == tuple(pts[0, 0, 0]) and (pts[4, 0, 1:] == oo.INVALID).all()
    assert bars.tolist() == [[0, 20], [20, 20], [40, 20], [0, 20], [40, 20]]
    far = poses[:1].copy()
    far[0, 0, :3] = (1e6, -1e6, 1.0)
    pts, _ = oo.project_poses(far, P[None], np.zeros(1, dtype=np.int32), 0.1)
    assert tuple(pts[0, 0, 0]) == (oo.CLAMP_Q4, -oo.CLAMP_Q4)
    long_axis, _ = oo.project_poses(poses[:1], P[None], np.zeros(1, dtype=np.int32), 50.0)      # the x and y tips 2500 px away; the z tip near the centre
    assert (long_axis[0, 0, 1:3] == oo.INVALID).all() and (long_axis[0, 0, 3] != oo.INVALID).all() and tuple(long_axis[0, 0, 0]) == (16 * 25, 216)


def test_flip_camera_rows():
    lu = _lu()
    rng = np.random.default_rng(3)
    hs = 37
    P = np.array([[120.0, 3, 18, 2], [-2, 118.0, 17, 1], [0.01, -0.02, 1.0, 0.3]])
    Pf = lu.flip_camera_rows(P, hs)
    assert Pf.dtype == np.float64 and np.array_equal(Pf, oo.flip_camera_rows(P, hs)) and P[1, 1] == 118.0
    X = np.concatenate([rng.uniform(-0.2, 0.2, (50, 2)), rng.uniform(1, 3, (50, 1)), np.ones((50, 1))], 1)
    a, b = X @ P.T, X @ Pf.T
    assert np.allclose(b[:, 0] / b[:, 2], a[:, 0] / a[:, 2], rtol=0, atol=1e-12)
    assert np.allclose(b[:, 1] / b[:, 2], hs - 1 - a[:, 1] / a[:, 2], rtol=0, atol=1e-10)
    P4 = np.vstack([P, [0, 0, 0, 1.0]])
    assert np.array_equal(lu.flip_camera_rows(P4, hs)[:3], Pf) and np.array_equal(lu.flip_camera_rows(np.stack([P, P]), hs)[1], Pf)
    with pytest.raises(ValueError):
        lu.flip_camera_rows(np.zeros((3, 3)), hs)


# -- the C ABI ------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_and_bound():
    from rgb_proprioceptive_pose_estimator_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "rpe_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.EXPORTS and hasattr(_lib.raw, name), name
    end = header.index("} rpe_overlay_style;")
    body = re.sub(r"/\*.*?\*/", "", header[header.rindex("typedef struct {", 0, end):end], flags=re.S)
    declared = [n for n in re.findall(r"\b([A-Za-z_0-9]+)(?=(?:\[\d+\])?[,;])", body)]
    assert declared == [n for n, _ in _lib.OverlayStyle._fields_] == ["rgb", "axis_rgb", "alpha_q8", "r_q4", "hw_q4", "trail", "trail_r_q4"]
    S = _lib.OverlayStyle
    assert ctypes.sizeof(S) == 32 and (S.rgb.offset, S.axis_rgb.offset, S.alpha_q8.offset, S.trail_r_q4.offset) == (0, 3, 12, 28)
    for macro, value in (("RPE_OVERLAY_CLAMP_Q4", _lib.OVERLAY_CLAMP_Q4), ("RPE_OVERLAY_AXIS_Q4", _lib.OVERLAY_AXIS_Q4), ("RPE_OVERLAY_MAX_SETS", 4),
                         ("RPE_OVERLAY_MAX_TRAIL", 64), ("RPE_OVERLAY_MAX_RADIUS_Q4", 256), ("RPE_OVERLAY_MAX_SIDE", 4096)):
        assert int(re.search(r"#define %s\s+(\d+)" % macro, header).group(1)) == value
    assert float(re.search(r"#define RPE_OVERLAY_NEAR\s+([0-9.]+)", header).group(1)) == _lib.OVERLAY_NEAR == oo.NEAR
    assert (_lib.OVERLAY_INVALID, _lib.OVERLAY_CLAMP_Q4, _lib.OVERLAY_AXIS_Q4) == (oo.INVALID, oo.CLAMP_Q4, oo.AXIS_Q4)
    s = ops.overlay_style((1, 2, 3), 77, 50, 9, ((4, 5, 6), (7, 8, 9), (10, 11, 12)), 3, 20)
    assert ops.overlay_style_to_list(s) == list(range(1, 13)) + [77, 50, 9, 3, 20] and len(ops.OVERLAY_STYLE_FIELDS) == 17
    assert ops.overlay_style_to_list(ops.overlay_style_from_list(ops.overlay_style_to_list(s))) == ops.overlay_style_to_list(s)


def test_overlay_style_refusals():
    from rgb_proprioceptive_pose_estimator_amd import ops
    ops.overlay_style(alpha_q8=0, r_q4=256, hw_q4=256, trail=64, trail_r_q4=256)
    for kw in (dict(alpha_q8=257), dict(alpha_q8=-1), dict(r_q4=257), dict(r_q4=-1), dict(hw_q4=257), dict(trail_r_q4=300), dict(trail=65), dict(trail=-1),
               dict(colour=(1, 2)), dict(colour=(0, 0, 256)), dict(colour=7), dict(axis_colours=((1, 2, 3),) * 2), dict(axis_colours=((1, 2, 3), (1, 2, 3), (1, 2, -3)))):
        with pytest.raises(ValueError, match="overlay_style"):
            ops.overlay_style(**kw)
    with pytest.raises(ValueError):
        ops.overlay_style_from_list([0] * 16)


def test_rejected_arguments_need_no_device():
    """bad arguments come back as a status before anything is launched"""
    from rgb_proprioceptive_pose_estimator_amd import _lib, ops
    raw = _lib.raw
    one = ctypes.c_void_p(16)   # never dereferenced: every call below is refused
    good = (ops.overlay_style(),)
    rgb6 = (ctypes.c_ubyte * 6)()

    def draw(n=1, hs=8, ws=8, first=0, styles=good, fpe=1, bar_px=0, frames=one, rgb=rgb6):
        arr = (_lib.OverlayStyle * max(1, len(styles)))(*styles)
        return raw.rpe_draw_poses_u8(frames, one, n, hs, ws, one, one, first, len(styles), arr, fpe, bar_px, rgb, 0, None)

    def bad_style(**kw):
        s = ops.overlay_style()
        for k, v in kw.items():
            setattr(s, k, v)
        return (s,)

    for kw in (dict(n=0), dict(first=-1), dict(hs=0), dict(ws=0), dict(hs=4097), dict(ws=4097), dict(styles=()), dict(styles=good * 5), dict(fpe=0),
               dict(bar_px=5), dict(bar_px=-1), dict(frames=None), dict(bar_px=1, rgb=None), dict(styles=bad_style(alpha_q8=257)), dict(styles=bad_style(r_q4=257)),
               dict(styles=bad_style(hw_q4=-1)), dict(styles=bad_style(trail=65)), dict(styles=bad_style(trail_r_q4=257))):
        assert draw(**kw) != 0, kw
        assert b"draw_poses_u8" in raw.rpe_last_error()

    def project(F=1, G=1, C=1, axis=0.05, pe=None, oe=None, pf=0.1, of=0.5, width=0, poses=one):
        return raw.rpe_project_poses(poses, one, one, F, G, C, axis, pe, oe, pf, of, width, one, one, None)

    for kw in (dict(F=0), dict(G=0), dict(G=5), dict(C=0), dict(axis=float("nan")), dict(pf=0.0), dict(of=-1.0), dict(pf=float("inf")), dict(width=-1),
               dict(width=4097), dict(pe=one), dict(oe=one), dict(poses=None)):
        assert project(**kw) != 0, kw
        assert b"project_poses" in raw.rpe_last_error()

    # the Python face says the same in words, before any pointer is taken
    f = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    pts, bars = torch.zeros((2, 1, 4, 2), dtype=torch.int32), torch.zeros((2, 2), dtype=torch.int32)
    for args, kw in (((f.float(), pts, bars, good), {}), ((f[0], pts, bars, good), {}), ((f, pts, bars, good * 2), {}), ((f, pts, bars, ()), {}),
                     ((f, pts.long(), bars, good), {}), ((f, pts, bars[:1], good), {}), ((f, pts, bars, good), dict(first=1)), ((f, pts, bars, good), dict(first=-1)),
                     ((f, pts, bars, good), dict(frames_per_episode=0)), ((f, pts, bars, good), dict(bar_px=5)), ((f, pts, bars, good), dict(bar_colours=((1, 2, 3),))),
                     ((f, pts, bars, good), dict(out=torch.zeros((2, 8, 8, 3)))), ((f, pts, bars, [dict()]), {})):
        with pytest.raises(ValueError, match="draw_poses_u8"):
            ops.draw_poses_u8(*args, **kw)
    with pytest.raises(ValueError, match="4096"):
        ops.draw_poses_u8(torch.zeros((1, 1, 4097, 3), dtype=torch.uint8), pts, bars, good)
    poses, cam, ci = torch.zeros((2, 1, 7)), torch.zeros((1, 3, 4), dtype=torch.float64), torch.zeros(2, dtype=torch.int32)
    for args, kw in (((poses.double(), cam, ci), {}), ((torch.zeros((2, 5, 7)), cam, ci), {}), ((poses, cam.float(), ci), {}), ((poses, cam[0], ci), {}),
                     ((poses, cam, ci.long()), {}), ((poses, cam, ci[:1]), {}), ((poses, cam, ci), dict(pos_err=torch.zeros(2))),
                     ((poses, cam, ci), dict(pos_err=torch.zeros(2), ori_err=torch.zeros(3))), ((poses, cam, ci), dict(pos_full=0.0)),
                     ((poses, cam, ci), dict(axis_len=float("inf"))), ((poses, cam, ci), dict(width=5000))):
        with pytest.raises(ValueError, match="project_poses"):
            ops.project_poses(*args, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):     # valid arguments on the host: refused, not computed some other way
        ops.project_poses(poses, cam, ci)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.draw_poses_u8(f, pts, bars, good)


def test_dispatcher_entries():
    from rgb_proprioceptive_pose_estimator_amd import ops
    import rgb_proprioceptive_pose_estimator_amd.torch_ops as T
    for name in ("project_poses", "draw_poses_u8"):
        assert name in T.NAMES and getattr(torch.ops.rpe, name).default._schema.name == "rpe::" + name
    s = torch.ops.rpe.project_poses.default._schema
    assert [a.name for a in s.arguments] == ["poses", "cam", "cam_index", "axis_len", "pos_err", "ori_err", "pos_full", "ori_full", "width"]
    assert not any(a.alias_info is not None for a in s.arguments)
    s = torch.ops.rpe.draw_poses_u8.default._schema
    assert [a.name for a in s.arguments] == ["frames", "points", "bars", "styles", "frames_per_episode", "first", "bar_px", "bar_colours", "flip"]
    assert not any(a.alias_info is not None for a in s.arguments)
    style = ops.overlay_style_to_list(ops.overlay_style())
    with pytest.raises(NotImplementedError):     # the HIP key only: no CPU kernel to fall back to
        torch.ops.rpe.project_poses(torch.zeros(2, 1, 7), torch.zeros((1, 3, 4), dtype=torch.float64), torch.zeros(2, dtype=torch.int32), 0.05, None, None, 0.1, 0.5, 0)
    with pytest.raises(NotImplementedError):
        torch.ops.rpe.draw_poses_u8(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), torch.zeros((2, 1, 4, 2), dtype=torch.int32), torch.zeros((2, 2), dtype=torch.int32),
                                    style, 1, 0, 0, [0] * 6, False)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        poses = torch.empty(6, 3, 7, device="cuda")
        pts, bars = torch.ops.rpe.project_poses(poses, torch.empty((2, 3, 4), dtype=torch.float64, device="cuda"), torch.empty(6, dtype=torch.int32, device="cuda"),
                                                0.05, None, None, 0.1, 0.5, 0)
        assert pts.shape == (6, 3, 4, 2) and bars.shape == (6, 2) and pts.dtype == bars.dtype == torch.int32
        pic = torch.ops.rpe.draw_poses_u8(torch.empty((4, 7, 5, 3), dtype=torch.uint8, device="cuda"), pts, bars, style * 3, 3, 2, 0, [0] * 6, True)
        assert pic.shape == (4, 7, 5, 3) and pic.dtype == torch.uint8


# -- render_episodes, write_video ---------------------------------------------------------------------------------------------------

def _evaluation(e=2, t=3, k=None):
    lead = (e, t) if k is None else (k, e, t)
    z = lambda *s: torch.zeros(*s)
    return types.SimpleNamespace(poses=z(*lead, 7), pos_err=z(*lead), ori_err=z(*lead), truth=z(e, t, 7), measurements=z(*lead, 7),
                                 noise_scales=None if k is None else [0.0] * k)


def test_render_episodes_checks_its_arguments():
    lu = _lu()
    ev, P = _evaluation(), np.eye(4)[:3]
    frames = torch.zeros((2, 3, 8, 10, 3), dtype=torch.uint8)
    for kw in (dict(frames=frames.float()), dict(frames=frames.numpy().astype(np.float32)), dict(frames=frames[0]), dict(frames=frames[:, :2]),
               dict(frames=frames[..., :2]), dict(draw=()), dict(draw=("truth", "truth")), dict(draw=("pose",)), dict(camera=np.eye(3)),
               dict(camera=np.zeros((3, 3, 4))), dict(camera=np.zeros((2, 2, 4))), dict(alpha=1.5), dict(alpha=-0.1), dict(radius=-1), dict(radius=17),
               dict(axis_width=40), dict(trail=65), dict(chunk=0), dict(scale=1), dict(colours={"pose": (1, 2, 3)}), dict(colours={"truth": (1, 2, 300)})):
        args = dict(dict(frames=frames, camera=P), **kw)
        with pytest.raises(ValueError):
            lu.render_episodes(ev, args.pop("frames"), args.pop("camera"), **args)
    with pytest.raises(ValueError, match="scale"):
        lu.render_episodes(_evaluation(k=2), frames, P, scale=2)
    no_meas = _evaluation()
    no_meas.measurements = None
    with pytest.raises(ValueError, match="measurement"):
        lu.render_episodes(no_meas, frames, P, draw=("measurement",))
    with pytest.raises(RuntimeError, match="no CPU fallback"):     # everything valid, on the host
        lu.render_episodes(ev, frames, P)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lu.render_episodes(_evaluation(k=2), frames.numpy(), np.stack([np.eye(4)] * 2), scale=1, draw=("measurement", "truth", "estimate"))


def test_write_video(tmp_path):
    from PIL import Image
    lu = _lu()
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (2, 3, 12, 16, 3), dtype=np.uint8)
    npy = lu.write_video(torch.from_numpy(frames), str(tmp_path / "v.npy"))
    back = np.load(npy)
    assert back.dtype == np.uint8 and np.array_equal(back, frames.reshape(6, 12, 16, 3))
    gif = lu.write_video(frames, str(tmp_path / "v.GIF"), fps=20)
    with Image.open(gif) as im:
        assert im.n_frames == 6 and im.size == (16, 12) and im.info["duration"] == 50
    for path, fr, kw in ((str(tmp_path / "v.mp4"), frames, {}), (str(tmp_path / "v"), frames, {}), (npy, frames.astype(np.float32), {}), (npy, frames[0, 0, 0], {}),
                         (npy, frames, dict(fps=0))):
        with pytest.raises(ValueError):
            lu.write_video(fr, path, **kw)
    with pytest.raises(ValueError, match=r"\.npy.*\.gif"):
        lu.write_video(frames, str(tmp_path / "v.mp4"))


# -- the script ---------------------------------------------------------------------------------------------------------------------

def test_script_refuses_in_one_line(tmp_path):
    from rgb_proprioceptive_pose_estimator_amd.scripts.rollout import main
    cam = str(tmp_path / "cam.npy")
    np.save(cam, np.eye(4)[:3])
    bad = str(tmp_path / "bad.npy")
    np.save(bad, np.eye(3))
    eps = str(tmp_path / "episodes.npz")         # never opened: every call below ends before
    base = ["--episodes", eps, "--camera_matrix", cam, "--n_episodes", "2"]
    for argv, word in ((["--video_out", "x.gif", "--camera_matrix", cam], "--episodes"), (["--video_out", "x.gif", "--episodes", eps], "--camera_matrix"),
                       (["--record_video", "--episodes", eps], "--camera_matrix"), (["--record_video"], "--episodes"),
                       (base + ["--video_out", "x.mp4"], ".gif"), (base + ["--video_out", "x"], ".gif"),
                       (["--camera_matrix", cam], "--video_out"), (["--video_fps", "5"], "--video_out"), (["--video_episodes", "1"], "--video_out"),
                       (["--video_draw", "truth"], "--video_out"), (["--axis_len", "0.1"], "--video_out"), (["--trail", "3"], "--video_out"),
                       (["--no_flip"], "--video_out"), (["--no_bars"], "--video_out"), (["--model_outputs_file", "m.npy"], "--video_out"),
                       (base + ["--video_out", "x.gif", "--video_fps", "0"], "--video_fps"), (base + ["--video_out", "x.gif", "--video_episodes", "3"], "--video_episodes"),
                       (base + ["--video_out", "x.gif", "--video_episodes", "0"], "--video_episodes"),
                       (base + ["--video_out", "x.gif", "--video_draw", "truth", "truth"], "--video_draw"), (base + ["--video_out", "x.gif", "--trail", "65"], "--trail"),
                       (base + ["--video_out", "x.npy", "--model_outputs_file", "m.npy", "--noise_scales", "0.1"], "--model_outputs_file"),
                       (["--episodes", eps, "--camera_matrix", bad, "--video_out", "x.gif"], "--camera_matrix"),
                       (["--episodes", eps, "--camera_matrix", str(tmp_path / "none.npy"), "--video_out", "x.gif"], "--camera_matrix")):
        with pytest.raises(SystemExit) as e:
            main(["--model", "no"] + argv)
        msg = str(e.value)
        assert msg.startswith("rollout.py: ") and word in msg and "\n" not in msg, (argv, msg)
    with pytest.raises(SystemExit):               # argparse's own refusal of an unknown pose set
        main(["--model", "no"] + base + ["--video_out", "x.gif", "--video_draw", "pose"])
