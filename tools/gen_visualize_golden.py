"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/visualize_*.npz by running the REFERENCE's own visualize_layer
(util/model_utils.py:10-107, imported through oracle/ref_stubs.py as oracle/gen_golden.py does) with matplotlib.pyplot.imshow
replaced by a recorder.  Run in the build container only, from the repository root:

    python -B tools/gen_visualize_golden.py <path to a checkout of the reference>

What is stored per layer (f0 f9 f1 f2 f3 f4 a0 d0; tests/_visualize_cases.py has the two configurations): the shapes of the arrays
the reference handed to imshow for the 's' and the 'm' picture, and the arrays themselves -- whole where they are small, otherwise
per-channel min / max / mean, three whole channels (0, the widest and a constant one) and a strided sample.  Only numbers the
reference computed travel; none of its text does.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

import matplotlib  # noqa: E402

matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402

from oracle import ref_stubs  # noqa: E402
from _visualize_cases import LAYERS, SAMPLE_STRIDE, VIS_CASES, WHOLE_MAX, case_inputs, grid_cols, oracle_maps, perturbed_state  # noqa: E402

ref_stubs.install()
if len(sys.argv) < 2 or not os.path.isdir(sys.argv[1]):
    raise SystemExit(__doc__)
sys.path.insert(0, sys.argv[1])
from models.naive import NaiveObjectStateEstimator  # noqa: E402
from models.time_sensitive import TemporallyDependentObjectStateEstimator  # noqa: E402
from util.model_utils import visualize_layer  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
# malformed / unavailable layer strings: what the reference raises for each is recorded (class names only)
BAD_LAYERS = ("x0m", "f5m", "f9", "f", "a1m", "d1m", "a0")


def build(kind, cfg):
    if kind == "no":
        return NaiveObjectStateEstimator("cube", list(cfg["hidden"]), cfg.get("depth", 50), cfg["latent_dim"], False, (9,), cfg["use_depth"], False,
                                         cfg["no_proprioception"])
    return TemporallyDependentObjectStateEstimator("hammer", cfg["hidden"], cfg.get("depth", 50), cfg["latent_dim"], 2, 0.1, False, (9,),
                                                   cfg["use_depth"], False, cfg["no_proprioception"])


def record(model, layer, img, depth):
    """the arrays one visualize_layer call hands to imshow, and how many axes end with row 0 at the BOTTOM (imshow's own y axis
    runs downwards, i.e. is 'inverted' in matplotlib's terms; the reference's invert_yaxis() turns it upwards)"""
    seen = []
    real = plt.imshow
    plt.imshow = lambda a, *k, **kw: (seen.append(np.array(a, copy=True)), real(np.zeros((2, 2))))[1]
    plt.show = lambda *a, **k: None
    try:
        visualize_layer(model, layer, img, depth)
        flipped = sum(not ax.yaxis_inverted() for ax in plt.gcf().get_axes())
    finally:
        plt.imshow = real
        plt.close("all")
    return seen, flipped


def run_case(name):
    kind, cfg, wseed, _ = VIS_CASES[name]
    torch.manual_seed(0)
    model = build(kind, cfg)
    sd = perturbed_state(kind, cfg, wseed)
    res = model.load_state_dict({k: v for k, v in sd.items() if not k.startswith("~")}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    img, depth = case_inputs(name)
    if kind == "no":
        vimg, vdepth = img[0], depth                 # (3,H,W): the function adds the batch dimension itself
    else:
        vimg, vdepth = img, depth.unsqueeze(0)       # (1,3,H,W) -> (1,1,3,H,W) inside, as the reference's script hands it over
        model.eval()
        model.rollout = True
        model.reset_initial_state(1)
    m64 = oracle_maps(kind, cfg, sd, img, depth, torch.float64)
    m32 = oracle_maps(kind, cfg, sd, img, depth, torch.float32)
    rec = {}
    for layer in LAYERS:
        assert m64[layer].abs().max().item() < 100, (name, layer, m64[layer].abs().max().item())
        with torch.no_grad():
            one, f1 = record(model, layer + "s", vimg, vdepth)
            many, fm = record(model, layer + "m", vimg, vdepth)
        full = np.stack(many).astype(np.float32)
        c, h, w = full.shape
        assert len(one) == 1 and f1 == 1 and fm == c and np.array_equal(one[0], full[0])   # 's' shows channel 0; every tile is flipped
        assert len(plt.get_fignums()) == 0
        err = np.abs(full.astype(np.float64) - m64[layer][0].numpy()).max() / np.abs(m64[layer][0].numpy()).max()
        d32 = np.abs(full - m32[layer][0].numpy()).max()
        rng = full.max(axis=(1, 2)) - full.min(axis=(1, 2))
        print("%s %-3s C=%4d %3dx%-3d n=%2d  min %9.4f max %9.4f  dead channels %3d  vs oracle fp32 %.1e  vs fp64 (rel) %.1e"
              % (name, layer, c, h, w, grid_cols(c), full.min(), full.max(), int((rng == 0).sum()), d32, err))
        rec[layer + "_shape"] = np.array(full.shape)
        rec[layer + "_s_tiles"] = np.array([a.shape for a in one])
        rec[layer + "_m_tiles"] = np.array([a.shape for a in many])
        rec[layer + "_cmin"] = full.min(axis=(1, 2))
        rec[layer + "_cmax"] = full.max(axis=(1, 2))
        rec[layer + "_cmean"] = full.astype(np.float64).mean(axis=(1, 2))
        if full.size <= WHOLE_MAX:
            rec[layer + "_whole"] = full
        else:
            dead = np.flatnonzero(rng == 0)
            pick = [0, int(np.argmax(rng)), int(dead[0]) if dead.size else c // 2]
            rec[layer + "_chan_idx"] = np.array(pick)
            rec[layer + "_chans"] = full[pick]
            rec[layer + "_sample"] = full.reshape(-1)[::SAMPLE_STRIDE]
    if kind == "no":
        names = []
        for bad in BAD_LAYERS:
            try:
                with torch.no_grad():
                    record(model, bad, vimg, vdepth)
                names.append("")
            except Exception as e:   # noqa: BLE001 -- the class is what is recorded
                names.append(type(e).__name__)
            print("%s layer %-5r -> %s" % (name, bad, names[-1] or "no exception"))
        rec["bad_layers"] = np.array(BAD_LAYERS)
        rec["bad_raises"] = np.array(names)
    path = os.path.join(OUT, "visualize_%s.npz" % name)
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    print("%s: %d bytes" % (path, size))
    assert size <= 1000 * 1000, size


if __name__ == "__main__":
    for case in VIS_CASES:
        run_case(case)
