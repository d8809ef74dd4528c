"""References and bars of the head-op tests: nn.Linear / nn.LSTM / F.relu on the CPU through torch.autograd.grad, in fp64 (the
reference) and in fp32 (the yardstick), from the same fp32 values; and the head graphs of the five model classes wired from copies of
a model's own nn modules as the class docstrings say.

An LSTM's outputs and a head graph's compound over S steps and several layers, so no single-launch bound applies to them.  Their bar
is relative to what fp32 costs on the same case: per tensor e = max|got - ref64| / max|ref64|, the yardstick y the same quantity for
torch's CPU fp32 run, and

    e <= m y + EPI u32

with the project's EPI = 4 as the floor (a lucky y near 0 cannot fail a correct kernel) and m fixed by measurement (M_BAR in
tests/test_gpu_headops.py).  Where the reference is exactly zero the result must be exactly zero.  No gradient flows into (h0, c0):
the ops truncate there."""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

import _bounds as B

F32, F64 = torch.float32, torch.float64
FLOOR = B.EPI * B.U32


def rel_err(got, ref):
    """max|got - ref| / max|ref|; against an all-zero reference 0 when got is all zero, inf otherwise; inf for a non-finite result"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    top = float(ref.abs().max()) if ref.numel() else 0.0
    if top == 0.0:
        return 0.0 if not bool((got != 0).any()) else float("inf")
    return float((got - ref).abs().max()) / top


def bar(m, y):
    return m * y + FLOOR


def yardstick(run32, run64):
    return {k: rel_err(run32[k], run64[k]) for k in run64}


def ratios(got, ref, yard, m):
    """-> {name: (e, bar, e / bar)} for every tensor of the reference (none skipped)"""
    out = {}
    for k in ref:
        e, b = rel_err(got[k], ref[k]), bar(m, yard[k])
        out[k] = (e, b, e / b)
    return out


def assert_bars(label, got, ref, yard, m):
    """every tensor of `ref` within its bar; prints each figure first (YARD lines: e, the yardstick y, e over the bar)"""
    res = ratios(got, ref, yard, m)
    for k, (e, b, r) in res.items():
        print("YARD %-44s %-10s e %.3e y %.3e ratio %.3f" % (label, k, e, yard[k], r))
    bad = {k: v for k, v in res.items() if not v[0] <= v[1]}
    assert not bad, "%s: %s" % (label, ", ".join("%s: e %.3g > bar %.3g (yardstick %.3g)" % (k, v[0], v[1], yard[k]) for k, v in bad.items()))
    return max(v[2] for v in res.values())


# ------------------------------------------------------------------ the two ops
def linear_run(d, case, dtype, which=1, addend=False, x=None, dy=None):
    """nn.Linear (+ addend, + F.relu) on pair `which` of linear_data -> y, dx, w, b (the gradients under the parameters' names)"""
    m, n, k, relu, bias = case
    lin = nn.Linear(k, n, bias=bool(bias)).to(dtype)
    with torch.no_grad():
        lin.weight.copy_(d["w"])
        if bias:
            lin.bias.copy_(d["b"])
    x = (d["x%d" % which] if x is None else x).to(dtype).requires_grad_()
    dy = (d["dy%d" % which] if dy is None else dy).to(dtype)
    y = lin(x)
    if addend:
        y = y + d["add"].to(dtype)
    if relu:
        y = F.relu(y)
    g = torch.autograd.grad(y, [x] + list(lin.parameters()), dy)
    out = dict(y=y.detach(), dx=g[0], w=g[1])
    if bias:
        out["b"] = g[2]
    return out


def make_lstm(d, dtype):
    i, h = d["w_ih"].shape[1], d["w_hh"].shape[1]
    lstm = nn.LSTM(i, h).to(dtype)
    with torch.no_grad():
        lstm.weight_ih_l0.copy_(d["w_ih"])
        lstm.weight_hh_l0.copy_(d["w_hh"])
        lstm.bias_ih_l0.copy_(d["b_ih"])
        lstm.bias_hh_l0.copy_(d["b_hh"])
    return lstm


def lstm_run(d, case, dtype):
    """nn.LSTM over (S, N, I) from (h0, c0) or zeros -> h_all [S*N, H], h_T, c_T, dx [S*N, I] and the four parameter gradients for
    the output gradient dh on every step's h"""
    s, n, i, h, given = case
    lstm = make_lstm(d, dtype)
    x = d["x"].to(dtype).view(s, n, i).clone().requires_grad_()
    hc = (d["h0"].to(dtype)[None], d["c0"].to(dtype)[None]) if given else None
    out, (ht, ct) = lstm(x, hc)
    g = torch.autograd.grad(out, [x, lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0], d["dh"].to(dtype).view(s, n, h))
    return dict(h_all=out.detach().reshape(s * n, h), h_T=ht[0].detach(), c_T=ct[0].detach(), dx=g[0].reshape(s * n, i), w_ih=g[1], w_hh=g[2],
                b_ih=g[3], b_hh=g[4])


# ------------------------------------------------------------------ the five head graphs
def graph_run(kind, mods, lead, data, dtype, given=(True, True), state=None):
    """One step of a family's head graph by autograd over copies of `mods` (name -> nn.Module, the model's own head modules):
      n:      pre = relu(fc(..relu(fc(feat)))), post = the same stack on cat(feat, pre - x0bar); ReLU on the 7-d outputs too
      no:     relu(fc(..relu(fc(cat(feat, x0bar))))), ReLU on the last layer too
      td:     pre = fc(lstm(feat)), post = fc(lstm(cat(feat, pre - x0bar)))
      tdo:    fc1(fc0(lstm(cat(feat, x0bar)))), no activation between
      tdo_v2: fc1(fc0(cat(lstm(feat), lstm(x0bar))))
    data: graph_data; given: which output gradients are handed over (the others are None to the model); state: tag -> (h0, c0) of a
    rollout step, None for the zero start.
    -> {"out0", ("out1"), "d_rows" (gradient of the rows the graph read, every column), "<module>.<parameter>" gradients (zero where
    the given outputs do not reach), "state.<tag>.h" / ".c" (the end state of every LSTM)}"""
    m = {k: copy.deepcopy(v).to(dtype) for k, v in mods.items()}
    feat, x0 = data["feat"].to(dtype), data["x0bar"].to(dtype)
    res = {}

    def lstm(tag, name, x):
        s, n = lead
        hc = None if state is None else (state[tag][0].to(dtype)[None], state[tag][1].to(dtype)[None])
        out, (h, c) = m[name](x.view(s, n, -1), hc)
        res["state.%s.h" % tag], res["state.%s.c" % tag] = h[0].detach(), c[0].detach()
        return out.reshape(s * n, -1)

    def stack(prefix, h):
        i = 0
        while prefix + str(i) in m:
            h = F.relu(m[prefix + str(i)](h))
            i += 1
        return h

    if kind == "n":
        leaf = feat.clone().requires_grad_()
        pre = stack("pre_fc", leaf)
        outs = [pre, stack("post_fc", torch.cat([leaf, pre - x0], 1))]
    elif kind == "no":
        leaf = torch.cat([feat, x0], 1).requires_grad_()
        outs = [stack("fc", leaf)]
    elif kind == "td":
        leaf = feat.clone().requires_grad_()
        pre = m["pre_measurement_fc"](lstm("pre", "pre_measurement_rnn", leaf))
        outs = [pre, m["post_measurement_fc"](lstm("post", "post_measurement_rnn", torch.cat([leaf, pre - x0], 1)))]
    elif kind == "tdo":
        leaf = torch.cat([feat, x0], 1).requires_grad_()
        outs = [m["fc1"](m["fc0"](lstm("rnn", "rnn", leaf)))]
    else:
        leaf = feat.clone().requires_grad_()
        h = torch.cat([lstm("img", "img_rnn", leaf), lstm("proprio", "proprio_rnn", x0)], 1)
        outs = [m["fc1"](m["fc0"](h))]
    for i, o in enumerate(outs):
        res["out%d" % i] = o.detach()
    names = [(k + "." + pn, p) for k, mod in m.items() for pn, p in mod.named_parameters()]
    pick = [(o, data["d_outs"][i].to(dtype)) for i, o in enumerate(outs) if given[i]]
    g = torch.autograd.grad([o for o, _ in pick], [leaf] + [p for _, p in names], [d for _, d in pick], allow_unused=True)
    res["d_rows"] = g[0] if g[0] is not None else torch.zeros_like(leaf)
    for (name, p), gp in zip(names, g[1:]):
        res[name] = gp if gp is not None else torch.zeros_like(p)
    return res
