"""Model construction and inspection helpers.  Mirrors util/model_utils.py of the reference: `set_parameter_requires_grad`,
`import_resnet` (:110-147) and `visualize_layer` (:10-107), the latter split into `capture_layer` (the layer's output as a
tensor), `render_layer` (the picture as an array) and `visualize_layer` (show it, or write a PNG).

What a layer string means is the reference's: `tns` with t = f (ResNet: f0 conv1's raw output, f9 bn1 after its in-place ReLU,
f1..f4 the layer1..layer4 outputs), a (aux_nets[n] BEFORE the product with the depth feature) or d (depth_nets[n]); s = `s` shows
channel 0, anything else every channel on an n x n grid, n = ceil(sqrt(C)), each tile autoscaled to its own range and drawn with
row 0 at the bottom.  The values are what the native engine holds after an inference forward (BatchNorm folded into the convs),
in its compute dtype, widened exactly to fp32 by the capture kernel (csrc/capture.hip).

Deliberate differences from the reference's function: only the trunk and the heads run (the fc / LSTM tail is not needed for
any layer on offer), so it works for all five model classes and every input the models accept -- also where the reference's
own forward fails behind the captured layer (`n`, `no` with proprioception, `td`'s unregistered heads); the carried LSTM
state and the BatchNorm running statistics are untouched; no forward hook is left on the module; every malformed or unavailable
layer string raises ValueError before any device work (the reference raises AttributeError / IndexError, some of them after its
forward).  Like the reference it leaves the model in eval().  Do not call it between a training forward and its backward: the
capture forward reuses the trunk's workspace.
"""
import os
import warnings

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..engine import ResNet50Trunk
from .data_utils import ERASE_FILL_MEAN

# An ImageNet checkpoint in torchvision's resnet50 state_dict format, if one is available locally.
# The reference fetches it over the network (torchvision pretrained=True); there is no egress here.
PRETRAINED_ENV = "RPE_RESNET50_WEIGHTS"


def set_parameter_requires_grad(model, feature_extracting):
    """Freeze every parameter when feature extracting (util/model_utils.py:110-113)."""
    if feature_extracting:
        for param in model.parameters():
            param.requires_grad = False


def import_resnet(num_layers, output_dim, feature_extract=True, use_pretrained=True, compute_dtype=torch.bfloat16):
    """ResNet feature extractor with its fc replaced by Linear(fc.in_features, output_dim) (2048; 512 for resnet18).

    Same contract as util/model_utils.py:116-147: validates `num_layers` against the reference's
    option set (which spells 34 as 32), freezes the body iff `feature_extract and use_pretrained`,
    the new fc is always trainable, returns (model, 224).  Every member the reference can build has a native launch
    plan: the bottleneck networks 50 / 101 / 152 and the BasicBlock network 18 (fc input 512); "32" passes the reference's
    assert and then fails in `getattr(models, "resnet32")` -- the same AttributeError is raised here.  Every caller of the
    reference passes 50 (scripts/train_model.py:63).
    """
    options = {18, 32, 50, 101, 152}
    assert num_layers in options, "Invalid layer size specified. Options are: {}".format(options)
    if num_layers == 32:   # util/model_utils.py:136: getattr(models, "resnet32") -- torchvision has no such model
        raise AttributeError("module 'torchvision.models' has no attribute 'resnet32'")
    model = ResNet50Trunk(1000, compute_dtype=compute_dtype, depth=num_layers)
    if use_pretrained:
        path = os.environ.get(PRETRAINED_ENV)
        if path and os.path.exists(path):
            model.load_state_dict(torch.load(path, map_location="cpu"))
        else:
            warnings.warn("use_pretrained=True but no local ImageNet checkpoint (set %s): the network fetch the reference "
                          "performs is unavailable offline; continuing from the random initialisation" % PRETRAINED_ENV)
    set_parameter_requires_grad(model, (feature_extract and use_pretrained))
    model.fc = nn.Linear(model.fc.in_features, output_dim)
    return model, 224


def lr_param_groups(model, trunk_lr_scale=None):
    """What the optimizer is built over (addition; the reference passes model.parameters(): scripts/train_model.py:228).  No scale, or a
    scale of 1: the plain parameter list.  Otherwise two groups that partition model.parameters() exactly once, in its order: the
    ResNet trunk's parameters with `lr_scale` = trunk_lr_scale (scripts.train_model.build_optimizer turns it into lr * scale), and
    everything else.  The unregistered early-feature heads of the `td` model are not in model.parameters(), so no optimizer has
    ever seen them, and they are in neither group."""
    params = list(model.parameters())
    if trunk_lr_scale is None or trunk_lr_scale == 1:
        return params
    if not trunk_lr_scale > 0.0:
        raise ValueError("invalid trunk_lr_scale %r: a value > 0" % (trunk_lr_scale,))
    trunk = {id(p) for p in model.trunk.parameters()}
    groups = [{"params": [p for p in params if id(p) in trunk], "lr_scale": float(trunk_lr_scale)}, {"params": [p for p in params if id(p) not in trunk]}]
    return [g for g in groups if g["params"]]


# ---------------------------------------------------------------------------------------------------------------------------------
# layer capture / visualisation (util/model_utils.py:10-107 of the reference)
# ---------------------------------------------------------------------------------------------------------------------------------
FEATURE_LAYERS = (0, 9, 1, 2, 3, 4)   # f0 conv1, f9 bn1, f1..f4 layer1..layer4


def parse_layer(layer, need_mode=False):
    """'tns' -> (t, n, single).  t in f / a / d, n a digit, single = (s == 's'); the third character is optional unless
    `need_mode`.  A bad first letter raises the reference's ValueError (util/model_utils.py:60), every other malformed string a
    ValueError of its own (the reference: IndexError after its forward)."""
    if not isinstance(layer, str) or len(layer) < 1:
        raise ValueError("Layer must be a string of the form 'tns' (e.g. 'f9m'); got: {!r}".format(layer))
    if layer[0] not in ("f", "d", "a"):
        raise ValueError("Layer must begin with 'f', 'd', or 'a'! Got: {}".format(layer[0]))
    if len(layer) < (3 if need_mode else 2):
        raise ValueError("Layer must be of the form 'tns' (type, number, [s]ingle / [m]ultiple); got: {!r}".format(layer))
    if layer[1] not in "0123456789":
        raise ValueError("Layer number must be a digit; got: {!r}".format(layer))
    return layer[0], int(layer[1]), len(layer) > 2 and layer[2] == "s"


def check_layer(model, kind, n):
    """ValueError unless `model` has layer (kind, n); no device work.  Returns the index into the model's aux heads (a / d)."""
    if kind == "f":
        if n not in FEATURE_LAYERS:
            raise ValueError("ResNet layers f0 (conv1), f9 (bn1) and f1..f4 (layer1..layer4) exist; got: f{}".format(n))
        return None
    hooks = getattr(model, "_hooks", None)
    if getattr(model, "aux_nets", None) is None or not hooks:
        raise ValueError("{} has no aux / depth heads (layer {}{})".format(type(model).__name__, kind, n))
    if n >= len(hooks):
        raise ValueError("{}{}: the model has {} aux / depth head(s)".format(kind, n, len(hooks)))
    if kind == "d" and not model.use_depth:
        raise ValueError("d{}: the model was built with use_depth=False, its depth heads never run".format(n))
    return n


def _as_image_batch(img):
    """-> (lead shape, frames?) of an image argument: float (..., 3, H, W) or raw uint8 frames (..., Hs, Ws, 3), up to two leading
    dimensions (sequence-shaped input is flattened as the models do)."""
    if not isinstance(img, torch.Tensor) or img.dim() < 3 or img.dim() > 5:
        raise ValueError("img must be a (3,H,W), (B,3,H,W) or (S,N,3,H,W) tensor (uint8 frames: channels last)")
    frames = img.dtype == torch.uint8
    if (img.shape[-1] if frames else img.shape[-3]) != 3:
        raise ValueError("img must have 3 channels; got shape {}".format(tuple(img.shape)))
    return tuple(img.shape[:-3]), frames


def _capture(model, layer, img, depth, need_mode):
    """-> (planes [B,C,H,W] fp32, minmax [B,C,2] fp32, lead shape, single)"""
    kind, n, single = parse_layer(layer, need_mode)
    head = check_layer(model, kind, n)
    lead, frames = _as_image_batch(img)
    trunk = model.trunk
    hw = tuple(trunk.crop_hw) if frames else tuple(img.shape[-2:])
    if head is not None:
        hooked = model._hooks[head]
        if hooked != 9 and hw != (224, 224):
            raise ValueError("hooks other than bn1 are sized for 224x224 inputs (as the reference's dummy forward is)")
        if kind == "d" and depth is None:
            raise ValueError("d{}: the depth head needs the depth image".format(n))
    model.eval()
    model._materialize(img.device)   # (raises for CPU tensors: there is no CPU path)
    x = img.reshape(-1, *img.shape[-3:]).contiguous()
    if not frames:
        x = x.float()
    b = x.shape[0]
    if depth is not None and kind == "d":
        if frames and depth.dim() >= 3 and tuple(depth.shape[-3:]) == tuple(x.shape[1:3]) + (1,):
            # raw channels-last depth beside raw frames (the models' shape rule, models/_core.py): the depth transform on the device
            depth = ops.stage_depth(depth.reshape(b, *x.shape[1:3]).float(), tuple(trunk.crop_hw), trunk.resize_to)
        depth = depth.reshape(b, 1, *depth.shape[-2:])
    rows = torch.empty((1, ops.pad4(model.latent_dim)), dtype=torch.float32, device=x.device)
    # Every image goes through the trunk on its own, on the batch-1 plan a rollout frame uses: the engine picks its reduction
    # order by the number of output rows (few rows: the long reductions of the deep layers are split), so a frame's values would
    # otherwise depend on how many other frames ride along; and a capture of an odd batch size then neither allocates a plan of
    # its own nor evicts the training plan (ResNet50Trunk.max_plans).  Each frame's planes kernel writes its slice of the result.
    # f0 is conv1's RAW output, which the folded inference stem does not write: without a conv1 hook of its own the model keeps it
    # for these forwards only.  The switch changes the packed inference copy of conv1's weight, which captured rollout frames
    # replay as it stands, so one more forward with the switch back restores it (same bytes: the packing is deterministic).
    raw_stem = kind == "f" and n == 0 and not trunk.keep_stem_raw
    planes = minmax = None
    with torch.no_grad():
        if raw_stem:
            trunk.keep_stem_raw = True
        try:
            for i in range(b):
                plan = trunk.run(x[i:i + 1], rows, False)
                if kind == "f":
                    v = plan.hooked_feature(n)
                else:
                    _, h, w, _ = plan.hooked_feature(model._hooks[head]).shape
                    v = model._aux_ops[head].parts(plan, None if depth is None else depth[i:i + 1], kind).view(1, h // 2, w // 2, 1)
                if planes is None:
                    _, h, w, c = v.shape
                    planes = torch.empty((b, c, h, w), dtype=torch.float32, device=x.device)
                    minmax = torch.empty((b, c, 2), dtype=torch.float32, device=x.device)
                ops.feature_planes(v, image=0, out=planes[i], minmax=minmax[i])
        finally:
            if raw_stem:
                trunk.keep_stem_raw = False
                trunk.run(x[:1], rows, False)
    return planes, minmax, lead, single


def capture_layer(model, layer, img, depth=None):
    """What layer `layer` ('tn', see the module docstring; a third character is ignored) holds for `img`, as an fp32 tensor on the
    model's device: img (3,H,W) -> (C',H',W'); (B,3,H,W) -> (B,C',H',W'); (S,N,3,H,W) -> (S*N,C',H',W').  a / d layers have
    C' = 1.  uint8 frames (..., Hs, Ws, 3) go through the trunk's own resize / crop / normalise staging."""
    planes, _, lead, _ = _capture(model, layer, img, depth, need_mode=False)
    return planes[0] if not lead else planes


def layer_index_image(model, layer, img, depth=None, *, gutter=1, flip_y=True):
    """The picture of `render_layer` before the colour lookup: (uint8 index image as a numpy array, (C, H, W, cols) of the grid).
    One image only ((3,H,W), or leading dimensions of size 1)."""
    planes, minmax, lead, single = _capture(model, layer, img, depth, need_mode=True)
    if planes.shape[0] != 1:
        raise ValueError("one image at a time can be drawn; got a batch of {}".format(planes.shape[0]))
    planes, minmax = planes[0], minmax[0]
    if single:
        planes, minmax = planes[:1], minmax[:1]
    c, h, w = planes.shape
    cols = int(np.ceil(np.sqrt(c)))
    idx = ops.feature_mosaic(planes, minmax, cols, gutter=gutter, flip_y=flip_y)
    return idx.cpu().numpy(), (c, h, w, cols)


def colour_table():
    """256 x 3 uint8: matplotlib's default colormap (viridis) when matplotlib is importable, a grey ramp otherwise."""
    try:
        import matplotlib
        return np.ascontiguousarray(matplotlib.colormaps["viridis"](np.arange(256), bytes=True)[:, :3])
    except Exception:
        return np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)


def render_layer(model, layer, img, depth=None, *, gutter=1, flip_y=True):
    """The reference's figure for `layer` ('tns') as a uint8 (rows, cols, 3) array: every tile autoscaled to its own range on the
    device (rpe_feature_mosaic), coloured on the host; gutters and unused grid cells are white."""
    idx, (c, h, w, cols) = layer_index_image(model, layer, img, depth, gutter=gutter, flip_y=flip_y)
    rgb = colour_table()[idx]
    oy, ox = np.arange(idx.shape[0]), np.arange(idx.shape[1])
    blank = (oy % (h + gutter) >= h)[:, None] | (ox % (w + gutter) >= w)[None, :]
    blank |= ((oy // (h + gutter))[:, None] * cols + (ox // (w + gutter))[None, :]) >= c
    rgb[blank] = 255
    return rgb


def visualize_layer(model, layer, img, depth=None, *, out=None):
    """Visualizes the output of a layer of `model` (util/model_utils.py:10-107).  Without `out` the picture is shown with
    matplotlib; with `out` it is written there as a PNG and no window is opened."""
    rgb = render_layer(model, layer, img, depth)
    if out is not None:
        from PIL import Image
        Image.fromarray(rgb).save(out, format="PNG")
        return out
    import matplotlib.pyplot as plt
    plt.figure()
    plt.imshow(rgb)
    plt.setp(plt.gcf().get_axes(), xticks=[], yticks=[])
    plt.show()
    return None


# ---------------------------------------------------------------------------------------------------------------------------------
# occlusion sensitivity (no counterpart in the reference): which pixels of a raw frame the predicted pose depends on
# ---------------------------------------------------------------------------------------------------------------------------------
SALIENCY_KINDS = ("position", "orientation")


def _yx_pair(v, name):
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError("{} is an int or a (y, x) pair; got {!r}".format(name, v))
        y, x = v
    else:
        y = x = v
    if int(y) != y or int(x) != x:
        raise ValueError("{} must be whole numbers of pixels; got {!r}".format(name, v))
    return int(y), int(x)


def occlusion_grid(hs, ws, patch, stride):
    """The grid of rectangles of an occlusion-sensitivity map of an hs x ws frame -> (Gy, Gx, tops, lefts).  `patch` and `stride` are
    an int or a (y, x) pair.  Gy = ceil((hs - ph) / sy) + 1 rows of rectangles, row gy at tops[gy] = min(gy * sy, hs - ph): the last
    row is clamped to the frame's edge; columns alike.  Rectangle k = gy * Gx + gx.  Pure host code (csrc/saliency.hip and
    rpe_occlusion_grid apply the same rule).  ValueError unless 1 <= patch <= frame and 1 <= stride <= patch on both axes (a stride
    beyond the rectangle would leave pixels that no rectangle covers)."""
    (ph, pw), (sy, sx) = _yx_pair(patch, "patch"), _yx_pair(stride, "stride")
    hs, ws = int(hs), int(ws)
    if hs < 1 or ws < 1:
        raise ValueError("the frame size must be positive; got {}x{}".format(hs, ws))
    if not (1 <= ph <= hs and 1 <= pw <= ws):
        raise ValueError("the rectangle must be at least 1x1 and no larger than the {}x{} frame; got patch {}x{}".format(hs, ws, ph, pw))
    if not (1 <= sy <= ph and 1 <= sx <= pw):
        raise ValueError("the stride must be at least 1 and no larger than the rectangle ({}x{}), so that every pixel is covered; got stride "
                         "{}x{}".format(ph, pw, sy, sx))
    if hs * ws * 3 >= 2 ** 31:
        raise ValueError("frames of {}x{} pixels are too large (hs * ws must stay below 2^31 / 3)".format(hs, ws))
    gy, gx = -(-(hs - ph) // sy) + 1, -(-(ws - pw) // sx) + 1
    return gy, gx, [min(g * sy, hs - ph) for g in range(gy)], [min(g * sx, ws - pw) for g in range(gx)]


class OcclusionSensitivity:
    """What `occlusion_sensitivity` returns.  Index 0 of `scores`, `maps` and `minmax` is position (the pose's own length unit), index 1
    orientation (radians).
        scores   (2, Gy, Gx) fp32, device: how far the prediction moved with rectangle (gy, gx) covered (with `truth`: the change in error)
        maps     (2, Hs, Ws) fp32, device: per pixel the mean score of the rectangles covering it
        minmax   (2, 2) fp32, device: each map's (lowest, highest) finite value
        baseline (7,) fp32, device: the prediction for the frame as it is
        patch, stride (y, x) pairs; grid = (Gy, Gx); fill the three bytes the rectangles were set to"""

    def __init__(self, scores, maps, minmax, baseline, patch, stride, grid, fill):
        self.scores, self.maps, self.minmax, self.baseline = scores, maps, minmax, baseline
        self.patch, self.stride, self.grid, self.fill = tuple(patch), tuple(stride), tuple(grid), tuple(fill)


def _single_frame(img):
    if not isinstance(img, torch.Tensor):
        raise ValueError("img must be one raw uint8 frame (Hs, Ws, 3) as a tensor")
    if img.dtype != torch.uint8:
        raise ValueError("occlusion sensitivity works on one RAW uint8 frame (Hs, Ws, 3): the rectangles are defined on the recorded frame, in "
                         "front of the trunk's resize / crop / normalise staging; got a {} image".format(str(img.dtype).split(".")[-1]))
    if img.dim() < 3 or img.shape[-1] != 3 or any(n != 1 for n in img.shape[:-3]):
        raise ValueError("img must be one frame (Hs, Ws, 3), leading dimensions of size 1 allowed; got shape {}".format(tuple(img.shape)))
    return img.reshape(img.shape[-3:]).contiguous()


def occlusion_sensitivity(model, img, depth=None, self_measurement=None, *, patch=32, stride=16, fill=ERASE_FILL_MEAN, truth=None, batch=64, output=-1):
    """Occlusion sensitivity of `model`'s predicted pose for one frame -> OcclusionSensitivity.

    One rectangle of the grid (`occlusion_grid`) at a time is set to the colour `fill` (default: util.data_utils.ERASE_FILL_MEAN, the
    colour --aug_erase_prob fills with), the model predicts, and the rectangle's score is how far the prediction moved: the distance
    in position and the rotation angle in orientation (rpe_pose_displacement; exactly 0 where the prediction did not change).  With
    `truth` (7,) the score is the distance to `truth` minus the unoccluded prediction's distance to `truth`: the signed change in error.

    img: one raw uint8 frame (Hs, Ws, 3) on the model's device; float images raise ValueError.  depth / self_measurement: the frame's
    depth image and measured pose, repeated for every row; depth is NOT occluded (the choice util.data_utils.FrameAugment makes: its
    erasing covers the colour frame only).  self_measurement=None stands for the identity pose (0, 0, 0, 0, 0, 0, 1).  output: which of
    a tuple of outputs to score, -1 the last (the two-arm models' own-arm head is 0).

    The K rectangles run in chunks of B = min(batch, 1 + K) rows: row 0 of EVERY chunk is the frame as it is and the last chunk is
    padded with further copies, so that all forwards run at one batch size -- the engine picks its reduction order by the number of
    rows, and predictions from different batch sizes are not comparable bit for bit.  The reference prediction is row 0 of the first
    chunk.  Sequence models are called with S = 1, N = B and `rollout` off, so every row starts from the zero state and the carried
    (h, c) are neither read nor written.  With its inputs on the device the call makes no host synchronisation; model.training, model.rollout, the carried state,
    parameters and buffers are left as they were.  The call may create one engine plan of batch B, which under
    ResNet50Trunk.max_plans can evict the least recently used plan."""
    frame = _single_frame(img)
    hs, ws = frame.shape[:2]
    gy, gx, _, _ = occlusion_grid(hs, ws, patch, stride)
    (ph, pw), (sy, sx) = _yx_pair(patch, "patch"), _yx_pair(stride, "stride")
    fill = tuple(int(c) for c in fill)
    if len(fill) != 3:
        raise ValueError("fill is three bytes (r, g, b); got {!r}".format(fill))
    if int(batch) < 2:
        raise ValueError("batch must be at least 2 (the unoccluded frame and one rectangle); got {!r}".format(batch))
    dev = frame.device
    if truth is not None:
        truth = torch.as_tensor(truth, dtype=torch.float32).to(dev).reshape(-1).contiguous()
        if truth.numel() != 7:
            raise ValueError("truth is one pose (7,); got {} values".format(truth.numel()))
    desc = ops.occlusion_desc(hs, ws, ph, pw, sy, sx, *fill)
    k = gy * gx
    b = min(int(batch), 1 + k)
    per = b - 1
    nchunks = -(-k // per)
    seq = bool(getattr(model, "requires_sequence", False))
    lead = (1, b) if seq else (b,)

    def rows_of(t, tail, name):   # one frame's tensor, repeated for every row of a chunk
        t = t.to(dev)
        if t.numel() != int(np.prod(tail)):
            raise ValueError("{} must hold one frame's {} values; got shape {}".format(name, "x".join(map(str, tail)), tuple(t.shape)))
        return t.reshape((1,) * len(lead) + tuple(tail)).expand(lead + tuple(tail)).contiguous()

    if self_measurement is None:   # the identity pose, made on the device: no copy from the host
        self_measurement = torch.zeros(7, dtype=torch.float32, device=dev)
        self_measurement[6:].fill_(1.0)
    x0bar = rows_of(torch.as_tensor(self_measurement, dtype=torch.float32), (7,), "self_measurement")
    if depth is not None:
        d3 = tuple(depth.shape[-3:]) if depth.dim() >= 3 else (1,) + tuple(depth.shape)
        depth = rows_of(depth, d3, "depth")

    batch_u8 = torch.empty(lead + (hs, ws, 3), dtype=torch.uint8, device=dev)
    dist = torch.empty((2, nchunks, b), dtype=torch.float32, device=dev)
    was_training, was_rollout = model.training, model.rollout
    first = None
    model.eval()
    model.rollout = False
    try:
        with torch.no_grad():
            for c in range(nchunks):
                ops.occlude_grid_u8(frame, desc, b, c * per, out=batch_u8.view(b, hs, ws, 3))
                out = model(batch_u8, depth, x0bar)
                if isinstance(out, (tuple, list)):
                    out = out[output]
                pred = out.reshape(b, 7)
                if pred.dtype != torch.float32 or not pred.is_contiguous():
                    pred = pred.float().contiguous()
                if first is None:
                    first = pred   # (kept alive: the reference pose is read from its row 0 by every chunk)
                ops.pose_displacement(pred, first[0] if truth is None else truth, pos=dist[0, c], ori=dist[1, c])
    finally:
        model.rollout = was_rollout
        model.train(was_training)
    if truth is not None:
        dist = dist - dist[:, 0, 0].reshape(2, 1, 1)
    scores = dist[:, :, 1:].reshape(2, nchunks * per)[:, :k].contiguous().view(2, gy, gx)
    maps, minmax = ops.saliency_map(scores, desc)
    return OcclusionSensitivity(scores, maps, minmax, first[0].clone(), (ph, pw), (sy, sx), (gy, gx), fill)


_TABLES = {}


def _device_colour_table(device):
    """colour_table() on `device`, uploaded once"""
    key = (device.type, device.index)
    t = _TABLES.get(key)
    if t is None:
        t = _TABLES[key] = torch.from_numpy(np.ascontiguousarray(colour_table(), dtype=np.uint8)).to(device)
    return t


def _saliency_index(which):
    if which not in SALIENCY_KINDS:
        raise ValueError("which is one of {}; got {!r}".format(SALIENCY_KINDS, which))
    return SALIENCY_KINDS.index(which)


def render_saliency(result, frame, which="position", *, alpha=0.5, fade=False):
    """The map `which` ('position' / 'orientation') of an OcclusionSensitivity drawn over its frame -> uint8 (Hs, Ws, 3) numpy array.
    The map is autoscaled to its own range and coloured through `colour_table()`; `alpha` in [0, 1] is the weight of the colour
    (alpha_q8 = round(alpha * 256)); with `fade` the weight grows with the value, so the cold part of the frame stays readable
    (rpe_saliency_overlay_u8).  Pixels without a finite value show the frame."""
    i = _saliency_index(which)
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError("alpha lies in [0, 1]; got {!r}".format(alpha))
    frame = _single_frame(frame).to(result.maps.device)
    if tuple(frame.shape[:2]) != tuple(result.maps.shape[1:]):
        raise ValueError("the frame is {}x{} but the map {}x{}".format(*frame.shape[:2], *result.maps.shape[1:]))
    out = ops.saliency_overlay_u8(frame, result.maps[i], result.minmax[i], _device_colour_table(frame.device), int(round(float(alpha) * 256)), fade)
    return out.cpu().numpy()


def visualize_saliency(model, img, depth=None, self_measurement=None, *, which="position", out=None, alpha=0.5, fade=False, result=None, **kwargs):
    """Shows the occlusion-sensitivity map `which` of `model` for the frame `img` over the frame; with `out` the picture is written
    there as a PNG and no window is opened (as `visualize_layer`).  kwargs go to `occlusion_sensitivity` (patch, stride, fill, truth,
    batch, output); `result`: an OcclusionSensitivity of the same frame to draw instead of computing one.  Returns the result."""
    if result is None:
        result = occlusion_sensitivity(model, img, depth, self_measurement, **kwargs)
    rgb = render_saliency(result, img, which, alpha=alpha, fade=fade)
    if out is not None:
        from PIL import Image
        Image.fromarray(rgb).save(out, format="PNG")
        return result
    import matplotlib.pyplot as plt
    plt.figure()
    plt.imshow(rgb)
    plt.setp(plt.gcf().get_axes(), xticks=[], yticks=[])
    plt.show()
    return result
