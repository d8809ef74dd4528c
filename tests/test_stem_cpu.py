"""Self-tests of the front end's references and bounds (tests/_stem_bounds.py) and of the coverage of its cases (tests/_stem_cases.py), on
the CPU: no GPU, no kernel.

- every case reaches the code path named beside it (the launchers' arithmetic restated in _stem_cases.py);
- the references are torch's conv2d and its autograd in fp64, and oracle.pil_resize.reference_transform on a golden frame;
- ops.frames_route decides as engine.py does, and crop_origin is int(round(.)) (half to even);
- soundness: torch-fp32 restatements of the kernels in the kernels' own association -- the forward's K walk in steps of one 64-byte row,
  the BN sums per 128-row tile, the weight gradient's steps of BMK rows per split and the splits in slab order (and reversed: the atomic
  form has no order), the staging's multiply-subtract both separate and contracted to an FMA, colsum's eight row lanes -- stay at
  <= 0.5 of every bound on the very cases of the GPU test;
- power: each fault of FAULTS, injected into a restatement, is rejected by a bound or an exact comparison on at least one case; printed
  beside it on how many of those cases the checks this suite had before pass it."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bounds as B
import _stem_bounds as SB
import _stem_cases as C

F32 = torch.float32
PAD = C.PAD
SENT = -12345.5
OLD_TOL = {F32: 2e-5, torch.bfloat16: 2e-2, torch.float16: 3e-3}        # test_gpu_ops.tol

FAULTS = ["a crop one row low", "mean / std channels swapped", "channel 3 not zeroed", "a border element written",
          "truncation instead of round-to-nearest-even", "scale applied after the 16-bit rounding", "scale applied to wd as well",
          "tap row 7 included in the forward", "rows past M entering the BN sums", "second image of a tile read at the first image's offset",
          "ties -> floor in crop_origin", "vertical pass skipped", "horizontal intermediate not rounded to 8 bits"]


def _name(dtype):
    return str(dtype)[6:]


def _fma(a, b, c):
    """fmaf through double: the product of two fp32 is exact in 53 bits"""
    return (a.double() * b.double() + c.double()).float()


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _ratio(got, ref, bnd):
    return B.check(got, ref, bnd, "")[1]


def _once(got, ref, bnd, dtype):
    return 0.0 if dtype == F32 else float(B.rounding_excess(got, ref, dtype, bnd).max())


def rel_err(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-12))


def _trunc(v, dtype):
    """fp32 -> dtype rounded toward zero (a 16-bit type)"""
    r = v.to(dtype)
    b = _bits(r).clone()
    over = (r.float().abs() > v.abs()) & torch.isfinite(v)
    b[over] -= 1
    return b.view(dtype).view(r.shape)


# ------------------------------------------------------------------ coverage
def test_cases_reach_their_paths():
    t = {s: C.fwd_tiles(*s) for s in C.STEM_SHAPES}
    m, tiles = t[(1, 8, 8)]
    assert m == 16 and len(tiles) == 1                                                              # a single ragged tile
    m, tiles = t[(3, 10, 14)]
    assert m == 105 and len(tiles) == 1 and tiles[0]["b1"] - tiles[0]["b0"] == 2                    # one tile, three images, ragged
    m, tiles = t[(5, 12, 20)]
    assert m == 300 and tiles[-1]["rows"] == 44 and tiles[1]["mid"] and tiles[1]["b0"] == 2 and tiles[1]["b1"] == 4
    m, tiles = t[(2, 30, 18)]
    assert m == 270 and tiles[1]["cut"] and tiles[1]["mid"]                                         # the edge falls inside an output row
    m, tiles = t[(2, 16, 32)]
    assert m == 256 and not any(x["mid"] for x in tiles) and all(x["rows"] == 128 for x in tiles)   # aligned
    m, tiles = t[(130, 8, 8)]
    assert all(x["b1"] - x["b0"] == 7 for x in tiles[:-1]) and sum(x["b0"] > 0 for x in tiles) >= len(tiles) - 1 and tiles[-1]["rows"] == 32
    m, tiles = t[(1, 64, 48)]
    assert len(tiles) == 6 and all(x["rows"] == 128 and x["b0"] == 0 for x in tiles)
    assert any(h > w for _, h, w in C.STEM_SHAPES) and any(w > h for _, h, w in C.STEM_SHAPES)
    # the old shape reaches neither a ragged tile nor a tile of several images (tile_b0 is every row's image there)
    m, tiles = C.fwd_tiles(*C.OLD_SHAPE)
    assert m % C.BM == 0 and not any(x["b1"] != x["b0"] for x in tiles)
    # the weight gradient: one split and several, an M that is no multiple of the reduction step -- in every type
    for dtype in C.DTYPES:
        plans = [C.wgrad_plan(*s, dtype) for s in C.STEM_SHAPES]
        assert any(p["splits"] == 1 for p in plans) and any(p["splits"] > 1 for p in plans) and any(p["M"] % p["bmk"] for p in plans)
        assert any(p["splits"] > 1 and p["M"] % p["rows_per_split"] for p in plans)                 # a ragged last split
    # the largest tensor of the GPU test is the staged 130 x 14 x 14 x 4 image
    assert max(b * (h + 6) * (w + 6) * 4 for b, h, w in C.STEM_SHAPES) == 130 * 14 * 14 * 4
    # packing: both tables reach the tiles, the mixed one the element-wise path, with a chunk that straddles two layers
    mixed, tiled = C.pack_paths(C.PACK_TABLE), C.pack_paths(C.PACK_TABLE_TILED)
    assert all(p["tiled"] for p in tiled) and any(p["tiled"] for p in mixed) and any(not p["tiled"] for p in mixed)
    assert any(p["straddles"] for p in mixed)
    starts, _ = C.pack_starts(C.PACK_TABLE)
    for l in (3, 4, 5):       # behind the 48 x 9 x 24 layer every start is off a chunk boundary: element-wise although the dims allow tiles
        assert starts[l] % C.CHUNK and not any(p["tiled"] for p in mixed if p["layer"] >= 2)
    # the resize cases reach the four modes, the down-scaling one windows wider than three taps
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import pil_bilinear_tables
    modes = {(hs != hr, ws != wr) for _, _, hs, ws, hr, wr, _, _, _ in C.RESIZE_CASES}
    assert modes == {(True, True), (False, True), (True, False), (False, False)}
    assert pil_bilinear_tables(40, 26)[1].shape[1] > 3 and pil_bilinear_tables(24, 16)[1].shape[1] > 3
    for _, _, hs, ws, hr, wr, h, w, wins in C.RESIZE_CASES:
        assert all(0 <= t and t + h <= hr and 0 <= l and l + w <= wr for t, l in wins)
    up = C.RESIZE_CASES[0]
    assert (0, 0) in up[8] and (up[4] - up[6], up[5] - up[7]) in up[8] and any(t % 2 and l % 2 for t, l in up[8])
    assert any((hs - h) % 2 and (ws - w) % 2 for _, hs, ws, h, w in C.FRAME_GEOMS)


def test_routing_is_the_engines():
    """ops.frames_route against engine.py's rule, and crop_origin against int(round(.)); the engine still states that rule"""
    from rgb_proprioceptive_pose_estimator_amd import engine, ops
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import crop_origin, resized_hw
    assert "(hr, wr) == (hs, ws) and (hs - h) % 2 == 0 and (ws - w) % 2 == 0" in inspect.getsource(engine)
    n_plain = n_window = 0
    for hs in range(8, 24):
        for ws in range(10, 26):
            for size in (min(hs, ws), 16):
                hr, wr = resized_hw(hs, ws, size)
                if hr < 8 or wr < 10:
                    with pytest.raises(ValueError):
                        ops.frames_route(hs, ws, 8, 10, size)
                    continue
                plain = (hr, wr) == (hs, ws) and (hs - 8) % 2 == 0 and (ws - 10) % 2 == 0
                want = ("plain",) if plain else ("window", hr, wr, int(round((hr - 8) / 2.0)), int(round((wr - 10) / 2.0)))
                assert ops.frames_route(hs, ws, 8, 10, size) == want
                n_plain, n_window = n_plain + plain, n_window + (not plain)
    assert n_plain and n_window
    for hs, ws, h, w in C.ODD_CROPS:
        assert crop_origin(hs, ws, h, w) == (int(round((hs - h) / 2.0)), int(round((ws - w) / 2.0)))
        assert ops.frames_route(hs, ws, h, w, min(hs, ws))[0] == "window"
    assert crop_origin(13, 15, 8, 8) == (2, 4)            # 2.5 -> 2, 3.5 -> 4


# ------------------------------------------------------------------ restatements: stem
def stage_image_k(img, dtype, mutant=None, fill=SENT):
    """nchw_to_nhwc4_kernel into a sentinel-filled x4"""
    b, _, h, w = img.shape
    x4 = torch.full((b, h + 2 * PAD, w + 2 * PAD, 4), fill, dtype=dtype)
    v = img.permute(0, 2, 3, 1)
    x4[:, PAD:PAD + h, PAD:PAD + w, :3] = _trunc(v, dtype) if (mutant == "truncation instead of round-to-nearest-even" and dtype != F32) else v.to(dtype)
    if mutant != "channel 3 not zeroed":
        x4[:, PAD:PAD + h, PAD:PAD + w, 3] = 0
    if mutant == "a border element written":
        x4[b - 1, PAD + h, PAD, 0] = 0
    return x4


def staged_faults(x4, ref, bnd, dtype, exact=None):
    """the GPU test's checks of a staged x4 -> the names of those that fail"""
    b, hp, wp, _ = x4.shape
    h, w = hp - 2 * PAD, wp - 2 * PAD
    inner = x4[:, PAD:PAD + h, PAD:PAD + w]
    bad = []
    if bool(_bits(inner[..., 3]).any()):
        bad.append("channel 3")
    bm = SB.x4_border(b, h, w)
    if not _same_bits(x4[bm], torch.full_like(x4[bm], SENT)):
        bad.append("border")
    got = inner[..., :3]
    if exact is not None:
        nan = torch.isnan(exact)
        if not (bool((torch.isnan(got) == nan).all()) and bool((_bits(got) == _bits(exact))[~nan].all())):
            bad.append("bits")
    else:
        if _ratio(got, ref, bnd) > 1.0:
            bad.append("bound")
        if _once(got, ref, bnd, dtype) > 1.0:
            bad.append("once")
    return bad


def im2col8(x4f):
    """x4 [B, H + 6, W + 6, 4] fp32 -> [M, 8, 32]: row m's tap row r is the 8 pixels (2 oh + r, 2 ow .. + 7) x 4 channels"""
    b = x4f.shape[0]
    cols = F.unfold(x4f.permute(0, 3, 1, 2), 8, stride=2)
    return cols.view(b, 4, 8, 8, -1).permute(0, 4, 2, 3, 1).reshape(-1, 8, 32)


def stem_fwd_k(x4, wp, shape, dtype, bias=None, relu=0, mutant=None):
    """nt_kernel<MODE_STEM>: K = 224 walked in steps of one 64-byte row (32 elements in 16 bits, 16 in fp32), fp32 accumulation; the BN
    sums per 128-row tile; or the role-3 epilogue -> (y in dtype, st [tiles, 2, 64] fp32)"""
    b, h, w = shape
    ho, wo = C.out_hw(h, w)
    hw, m = ho * wo, b * ho * wo
    rows = im2col8(x4.float())
    if mutant == "second image of a tile read at the first image's offset":
        i = torch.arange(m)
        rows = rows[((i // C.BM * C.BM) // hw) * hw + i % hw]
    nrow = 8 if mutant == "tap row 7 included in the forward" else 7
    a, wm = rows[:, :nrow].reshape(m, nrow * 32), wp.float().view(64, 8, 32)[:, :nrow].reshape(64, nrow * 32)
    bk = 4 * C.CE[dtype]
    acc = torch.zeros(m, 64)
    for k in range(0, nrow * 32, bk):
        acc = acc + a[:, k:k + bk] @ wm[:, k:k + bk].t()
    if bias is not None:
        v = acc + bias
        return (v.clamp_min(0) if relu else v).to(dtype).view(b, ho, wo, 64), None
    _, tiles = C.fwd_tiles(b, h, w)
    st = torch.zeros(len(tiles), 2, 64)
    for t, tl in enumerate(tiles):
        blk = acc[tl["m0"]:tl["m0"] + tl["rows"]]
        st[t, 0], st[t, 1] = blk.sum(0), (blk * blk).sum(0)
        if mutant == "rows past M entering the BN sums":          # (a masked row's address is the tile's first row's)
            st[t, 0] += (C.BM - tl["rows"]) * acc[tl["m0"]]
            st[t, 1] += (C.BM - tl["rows"]) * acc[tl["m0"]] ** 2
    return acc.to(dtype).view(b, ho, wo, 64), st


def stem_wgrad_k(x4, dy, shape, dtype, reverse=False):
    """tn_kernel<64, 256, MODE_CONV>: per split of M, steps of BMK rows accumulated in fp32; the splits' tiles summed in slab order
    (reverse: some other order, as the atomic form may take) -> dw_packed [64, 8, 8, 4]"""
    plan = C.wgrad_plan(*shape, dtype)
    m, rps, bmk = plan["M"], plan["rows_per_split"], plan["bmk"]
    a, p = im2col8(x4.float()).reshape(m, 256), dy.float().reshape(m, 64)
    parts = []
    for s in range(plan["splits"]):
        m1 = min(m, (s + 1) * rps)
        acc = torch.zeros(64, 256)
        for k in range(s * rps, m1, bmk):
            e = min(k + bmk, m1)
            acc = acc + p[k:e].t() @ a[k:e]
        parts.append(acc)
    tot = torch.zeros(64, 256)
    for part in (reversed(parts) if reverse else parts):
        tot = tot + part
    return tot.view(64, 8, 8, 4)


def stats_ratio(st, r):
    acc = r.acc.reshape(-1, 64)
    eb = B.bound(B.Ref(acc, r.Q.reshape(acc.shape), r.K), F32)
    tot, sq = st.sum(0), acc * acc
    return max(_ratio(tot[0], acc.sum(0), B.sum_bound(acc, eb)), _ratio(tot[1], sq.sum(0), B.sum_bound(sq, 2 * acc.abs() * eb + eb * eb + B.U32 * sq)))


_STEM = {}


def _stem(dtype, shape):
    """case, staged image, packed weights and references, computed once"""
    key = (dtype, shape)
    if key not in _STEM:
        d = C.stem_case(dtype, shape)
        b, h, w = shape
        x4 = stage_image_k(d["img"], dtype, fill=0.0)
        wp, wps = SB.pack_stem_ref(d["w"], None, dtype), SB.pack_stem_ref(d["w"], d["scale"], dtype)
        _STEM[key] = dict(d, x4=x4, wp=wp, wps=wps, r=SB.stem_fwd_ref(x4, wp, h, w), r2=SB.stem_fwd_ref(x4, wps, h, w),
                          rw=SB.stem_wgrad_ref(x4, d["dy"], h, w))
    return _STEM[key]


def fwd_faults(dtype, shape, mutant):
    """the GPU test's checks of the statistics form on a (mutated) restatement -> the names of those that fail"""
    s = _stem(dtype, shape)
    y, st = stem_fwd_k(s["x4"], s["wp"], shape, dtype, mutant=mutant)
    bad = []
    bnd = B.bound(s["r"], dtype)
    if _ratio(y, s["r"].acc, bnd) > 1.0 or _once(y, s["r"].acc, bnd, dtype) > 1.0:
        bad.append("y")
    if stats_ratio(st, s["r"]) > 1.0:
        bad.append("stats")
    poisoned = s["wp"].clone()
    poisoned[:, 7] = C.NAN
    if not _same_bits(stem_fwd_k(s["x4"], poisoned, shape, dtype, mutant=mutant)[0], y):
        bad.append("tap row 7 is read")
    return bad


def test_references_are_torch():
    """the stem references are F.conv2d and its autograd in fp64; the staging reference is oracle.pil_resize.reference_transform"""
    import os
    from oracle.pil_resize import crop_origin, reference_transform, resized_hw
    for shape in ((3, 10, 14), (2, 30, 18)):
        s = _stem(torch.bfloat16, shape)
        b, h, w = shape
        img = SB.x4_image(s["x4"], h, w).double()
        wt = SB.packed_weight(s["wp"]).double().requires_grad_(True)
        y = F.conv2d(img, wt, None, 2, 3)
        assert float((y.detach().permute(0, 2, 3, 1) - s["r"].acc).abs().max()) < 1e-12
        dy = s["dy"].double().permute(0, 3, 1, 2)
        (dw,) = torch.autograd.grad(y, wt, dy)
        assert float((dw.permute(0, 2, 3, 1) - s["rw"].acc).abs().max()) < 1e-11
        assert torch.equal(SB.unpack_stem_ref(F.pad(dw.permute(0, 2, 3, 1), (0, 1, 0, 1, 0, 1)).float().contiguous()), dw.float())
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resize_pil.npz"))
    a = gold["in0"]
    hr, wr = resized_hw(a.shape[0], a.shape[1], 256)
    top, left = crop_origin(hr, wr, 224, 224)
    res = SB.resize_u8(torch.from_numpy(a)[None], hr, wr)
    assert np.array_equal(res[0].numpy(), gold["out0"])
    ref, bnd = SB.normalise_ref(SB.window(res, top, left, 224, 224), C.f32(C.IMAGENET_MEAN), C.f32(C.IMAGENET_STD), F32)
    want = torch.from_numpy(reference_transform(a)).permute(1, 2, 0)[None]
    assert _ratio(want, ref, bnd) <= 1.0          # (x / 255 - m) / std in fp32: another association of the same formula


def test_stem_restatements_stay_within_half_the_bound():
    worst = {}

    def note(k, v):
        worst[k] = max(worst.get(k, 0.0), v)
    for dtype in C.DTYPES:
        for shape in C.STEM_SHAPES:
            s = _stem(dtype, shape)
            assert fwd_faults(dtype, shape, None) == []
            y, st = stem_fwd_k(s["x4"], s["wp"], shape, dtype)
            bnd = B.bound(s["r"], dtype)
            note("forward y", _ratio(y, s["r"].acc, bnd))
            note("forward y, one rounding", _once(y, s["r"].acc, bnd, dtype))
            note("forward statistics", stats_ratio(st, s["r"]))
            for relu in (0, 1):
                out, _ = stem_fwd_k(s["x4"], s["wps"], shape, dtype, bias=s["bias"], relu=relu)
                ref, bnd = SB.affine_ref(s["r2"], s["bias"], relu, dtype)
                note("affine", _ratio(out, ref, bnd))
                note("affine, one rounding", _once(out, ref, bnd, dtype))
                if relu:
                    assert 0.2 < float((ref == 0).double().mean()) < 0.8
            bw = B.bound(s["rw"], F32)
            for rev in (False, True):
                dwp = stem_wgrad_k(s["x4"], s["dy"], shape, dtype, rev)
                note("weight gradient" + (", reversed" if rev else ""), _ratio(SB.packed_grad(dwp), s["rw"].acc, bw))
                assert not bool(_bits(dwp[..., 3]).any())
                pre = torch.randn(64, 8, 8, 4, generator=C._seed(7)) * float(s["rw"].acc.abs().mean())
                p = SB.packed_grad(pre).double()
                ref = p + s["rw"].acc
                note("weight gradient, accumulating", _ratio(SB.packed_grad(pre + dwp), ref, B.bound(s["rw"], F32, out=ref, epi=s["rw"].acc.abs() + p.abs())))
    print("RATIOS stem: %s" % {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= (1.0 if "one rounding" in k else 0.5) for k, v in worst.items()), worst


# ------------------------------------------------------------------ restatements: staging
def normalise_k(src, mean, std, dtype, fma, mutant=None):
    """((float) p * (1.f / 255.f) - m) * (1.f / std), the multiply-subtract separate or contracted"""
    m, i = C.f32(mean), 1.0 / C.f32(std)
    if mutant == "mean / std channels swapped":
        m, i = m.flip(0), i.flip(0)
    p, c = src.float(), torch.tensor(1.0, dtype=F32) / 255.0
    t = _fma(p, c, -m) if fma else p * c - m
    v = t * i
    return _trunc(v, dtype) if (mutant == "truncation instead of round-to-nearest-even" and dtype != F32) else v.to(dtype)


def stage_k(vals):
    b, h, w, _ = vals.shape
    x4 = torch.full((b, h + 2 * PAD, w + 2 * PAD, 4), SENT, dtype=vals.dtype)
    x4[:, PAD:PAD + h, PAD:PAD + w, :3] = vals
    x4[:, PAD:PAD + h, PAD:PAD + w, 3] = 0
    return x4


def resize_k(frames, hr, wr, mutant=None):
    """resize_h_u8_kernel + the vertical pass of resize_v_crop_norm_kernel on uint8 [B, Hs, Ws, 3] -> int64 [B, Hr, Wr, 3]"""
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import pil_bilinear_tables
    a = frames.numpy().astype(np.int64)
    b, hs, ws, _ = a.shape
    mid = a.astype(np.float64)
    if ws != wr:
        xb, xk = pil_bilinear_tables(ws, wr)
        mid = np.empty((b, hs, wr, 3))
        for x in range(wr):
            lo, n = xb[x]
            acc = (1 << 21) + np.tensordot(a[:, :, lo:lo + n], xk[x, :n].astype(np.int64), axes=(2, 0))
            mid[:, :, x] = acc / float(1 << 22) if mutant == "horizontal intermediate not rounded to 8 bits" else np.clip(acc >> 22, 0, 255)
    if hs == hr:
        return torch.from_numpy(np.floor(mid).astype(np.int64))
    if mutant == "vertical pass skipped":
        return torch.from_numpy(np.floor(mid[:, np.minimum(np.arange(hr), hs - 1)]).astype(np.int64))
    yb, yk = pil_bilinear_tables(hs, hr)
    out = np.empty((b, hr, wr, 3), np.int64)
    for y in range(hr):
        lo, n = yb[y]
        acc = (1 << 21) + np.tensordot(mid[:, lo:lo + n], yk[y, :n].astype(np.float64), axes=(1, 0))
        out[:, y] = np.clip(np.floor(acc / float(1 << 22)), 0, 255)
    return torch.from_numpy(out)


W0 = torch.randn(64, 3, 7, 7, generator=C._seed(3)) / 12.0


def model_proxy(x4):
    """what stands in for `a model output` on the CPU: conv1 -> ReLU -> global average of the staged image, fp32"""
    b, hp, wp, _ = x4.shape
    return F.relu(F.conv2d(SB.x4_image(x4, hp - 2 * PAD, wp - 2 * PAD).float(), W0, None, 2, 3)).mean((2, 3))


def old_staging_passes(x4, x4_good):
    """the old checks: fp32 only, allclose(rtol = 1e-4) on a model output; they never looked at channel 3 or at the border (a zero-filled
    buffer cannot tell a written border from an untouched one)"""
    if x4.dtype != F32:
        return True
    return bool(torch.allclose(model_proxy(x4), model_proxy(x4_good), rtol=1e-4))


def _frame_cases():
    """(label, dtype, source pixels [B, h, w, 3] as the kernel must read them, the same one row low, mean, std)"""
    for dtype in C.DTYPES:
        for geom in C.FRAME_GEOMS:
            b, hs, ws, h, w = geom
            fr = C.frames_case(geom)
            top, left = (hs - h) // 2, (ws - w) // 2
            low = SB.window(fr, min(top + 1, hs - h), left, h, w) if hs > h else None
            for name, mean, std in C.NORMS:
                yield "%s %s %s" % (_name(dtype), geom, name), dtype, SB.window(fr, top, left, h, w), low, mean, std


def _resize_cases():
    for dtype in C.DTYPES:
        for name, b, hs, ws, hr, wr, h, w, wins in C.RESIZE_CASES:
            yield name, dtype, C.resize_frames(b, hs, ws), hr, wr, h, w, wins


def test_staging_restatements_stay_within_half_the_bound():
    worst = {}

    def note(k, v):
        worst[k] = max(worst.get(k, 0.0), v)
    for label, dtype, src, _, mean, std in _frame_cases():
        ref, bnd = SB.normalise_ref(src, C.f32(mean), C.f32(std), dtype)
        for fma in (False, True):
            got = normalise_k(src, mean, std, dtype, fma)
            note("frames" + (", FMA" if fma else ""), _ratio(got, ref, bnd))
            note("frames, one rounding", _once(got, ref, bnd, dtype))
            assert staged_faults(stage_k(got), ref, bnd, dtype) == [], label
    for name, dtype, fr, hr, wr, h, w, wins in _resize_cases():
        res = resize_k(fr, hr, wr)
        assert torch.equal(res, SB.resize_u8(fr, hr, wr).long()), name + ": the kernel's statement is not Pillow's resize"
        for top, left in wins:
            src = SB.window(res, top, left, h, w)
            ref, bnd = SB.normalise_ref(src, C.f32(C.IMAGENET_MEAN), C.f32(C.IMAGENET_STD), dtype)
            for fma in (False, True):
                note("resized frames" + (", FMA" if fma else ""), _ratio(normalise_k(src, C.IMAGENET_MEAN, C.IMAGENET_STD, dtype, fma), ref, bnd))
    for dtype in C.DTYPES:
        for shape in C.IMAGE_SHAPES:
            img = C.image_case(shape)
            assert staged_faults(stage_image_k(img, dtype), None, None, dtype, exact=img.permute(0, 2, 3, 1).to(dtype)) == []
    for rows, cols, ld in C.COLSUM_CASES:
        x, old = C.colsum_case(rows, cols, ld)
        lanes = torch.zeros(8, cols)
        for r in range(rows):
            lanes[r % 8] += x[r, :cols]
        s = lanes[0].clone()
        for i in range(1, 8):
            s = s + lanes[i]
        note("colsum", _ratio(s, *SB.colsum_ref(x, cols)))
        note("colsum, accumulating", _ratio(old + s, *SB.colsum_ref(x, cols, old)))
    print("RATIOS staging: %s" % {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= (1.0 if "one rounding" in k else 0.5) for k, v in worst.items()), worst


# ------------------------------------------------------------------ power
def test_faults_are_rejected():
    rej, old = {f: 0 for f in FAULTS}, {f: 0 for f in FAULTS}

    def tally(f, bad, old_passes):
        if bad:
            rej[f] += 1
            old[f] += bool(old_passes)
    # the frame staging
    for label, dtype, src, low, mean, std in _frame_cases():
        ref, bnd = SB.normalise_ref(src, C.f32(mean), C.f32(std), dtype)
        good = stage_k(normalise_k(src, mean, std, dtype, False))
        if low is not None:
            x4 = stage_k(normalise_k(low, mean, std, dtype, False))
            tally(FAULTS[0], staged_faults(x4, ref, bnd, dtype), old_staging_passes(x4, good))
        for f in (FAULTS[1], FAULTS[4]):
            x4 = stage_k(normalise_k(src, mean, std, dtype, False, f))
            tally(f, staged_faults(x4, ref, bnd, dtype), old_staging_passes(x4, good))
    # rpe_stage_image_nhwc4: channel 3, the border, the rounding
    for dtype in C.DTYPES:
        for shape in C.IMAGE_SHAPES:
            img = C.image_case(shape)
            exact = img.permute(0, 2, 3, 1).to(dtype)
            for f in (FAULTS[2], FAULTS[3], FAULTS[4]):
                tally(f, staged_faults(stage_image_k(img, dtype, f), None, None, dtype, exact=exact), True)     # (no old check looks there)
    # the resize
    for name, dtype, fr, hr, wr, h, w, wins in _resize_cases():
        res = SB.resize_u8(fr, hr, wr).long()
        for f in (FAULTS[11], FAULTS[12]):
            mut = resize_k(fr, hr, wr, f)
            for top, left in wins[:1]:
                src = SB.window(res, top, left, h, w)
                ref, bnd = SB.normalise_ref(src, C.f32(C.IMAGENET_MEAN), C.f32(C.IMAGENET_STD), dtype)
                x4 = stage_k(normalise_k(SB.window(mut, top, left, h, w), C.IMAGENET_MEAN, C.IMAGENET_STD, dtype, False))
                tally(f, staged_faults(x4, ref, bnd, dtype), old_staging_passes(x4, stage_k(normalise_k(src, C.IMAGENET_MEAN, C.IMAGENET_STD, dtype, False))))
    # crop_origin with ties to the floor: the offsets, and the pixels behind them
    for hs, ws, h, w in C.ODD_CROPS:
        want, got = (int(round((hs - h) / 2.0)), int(round((ws - w) / 2.0))), ((hs - h) // 2, (ws - w) // 2)
        fr = C.resize_frames(2, hs, ws)
        ref, bnd = SB.normalise_ref(SB.window(fr, *want, h, w), C.f32(C.IMAGENET_MEAN), C.f32(C.IMAGENET_STD), F32)
        x4 = stage_k(normalise_k(SB.window(fr, *got, h, w), C.IMAGENET_MEAN, C.IMAGENET_STD, F32, False))
        tally(FAULTS[10], got != want and staged_faults(x4, ref, bnd, F32), True)     # (the old frame tests have even differences only)
    # the stem weight's and the trunk weights' packing
    for dtype in C.DTYPES:
        for shape in C.STEM_SHAPES[:1]:
            s = _stem(dtype, shape)
            late = (SB.pack_stem_ref(s["w"], None, dtype).float() * s["scale"].view(64, 1, 1, 1)).to(dtype)
            o = _stem(dtype, C.OLD_SHAPE)
            y_old = stem_fwd_k(o["x4"], (SB.pack_stem_ref(o["w"], None, dtype).float() * o["scale"].view(64, 1, 1, 1)).to(dtype), C.OLD_SHAPE, dtype)[0]
            tally(FAULTS[5], not _same_bits(late, s["wps"]), rel_err(y_old, o["r2"].acc) < OLD_TOL[dtype])
        for (co, rs, ci, sc, _, _), c in zip(C.PACK_TABLE, C.pack_case(C.PACK_TABLE)):
            if sc:
                wd = (c["src"] * c["scale"].view(-1, 1, 1)).permute(2, 1, 0).contiguous().to(dtype)
                tally(FAULTS[6], not _same_bits(wd, SB.pack_ref(c["src"], c["scale"], dtype)[1]), True)     # (no old check: the inference path never reads wd)
    # the stem forward
    for dtype in C.DTYPES:
        for f in (FAULTS[7], FAULTS[8], FAULTS[9]):
            o = _stem(dtype, C.OLD_SHAPE)
            y, st = stem_fwd_k(o["x4"], o["wp"], C.OLD_SHAPE, dtype, mutant=f)
            old_ok = rel_err(y, o["r"].acc) < OLD_TOL[dtype] and rel_err(st.sum(0)[0], o["r"].acc.sum((0, 1, 2))) < 1e-3 + OLD_TOL[dtype]
            for shape in C.STEM_SHAPES:
                tally(f, fwd_faults(dtype, shape, f), old_ok)
    for f in FAULTS:
        print("FAULT %-62s rejected on %2d cases, the old checks pass it on %2d of them" % (f, rej[f], old[f]))
    missed = [f for f in FAULTS if rej[f] == 0]
    assert not missed, "no case rejects %s" % missed


def test_truncation_helper():
    v = torch.tensor([1.0 + 2.0 ** -9, -(1.0 + 2.0 ** -9), 1.0 + 3 * 2.0 ** -9, 1.0, -2.5, 0.0])
    assert _trunc(v, torch.bfloat16).tolist() == [1.0, -1.0, 1.0, 1.0, -2.5, 0.0]
    x = torch.tensor([1.0 + 3 * 2.0 ** -12])          # nearest-even gives 1 + 2^-10, truncation 1
    assert float(x.to(torch.float16)) == 1.0 + 2.0 ** -10 and float(_trunc(x, torch.float16)) == 1.0
