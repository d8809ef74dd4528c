"""Self-tests of the head-op references and bars (tests/_headops_ref.py) on the cases of tests/_headops_cases.py, on the CPU.

- reference: the fp64 nn.LSTM runs equal oracle.pose_oracle.lstm_forward (values, and gradients through autograd) to 1e-12; every
  reference tensor of every case has max|ref| > 1e-3 apart from the listed exact zeros, so no relative check is vacuous;
- yardstick: torch's fp32 run of every case is finite and below 1e-5 of each tensor's largest element against fp64;
- soundness: a plain-torch fp32 restatement of LinearOp / LSTMOp (padded row buffers, the backward through time written out as
  headops.py launches it) and of the two-arm sequence graph passes every bar at m = 2;
- power: each fault of MUTANTS, put into that restatement, misses at least one case by at least 100 times its bar.  One of them shows
  only in the check it is named after: a finite value left in a padding column of dx changes no GEMM result, because the weights'
  padding columns are zero as well -- which is why the padding columns are asserted to be exactly zero on their own."""
import pytest
import torch
import torch.nn as nn

import _headops_cases as C
import _headops_ref as R
from oracle import pose_oracle as po

F32, F64 = torch.float32, torch.float64
M_CPU = 2


def pad4(n):
    return (n + 3) // 4 * 4


def rows(r, c, fill=0.0):
    return torch.full((r, pad4(c)), fill, dtype=F32)[:, :c]


def padded(v):
    ld = pad4(v.shape[1])
    assert v.stride(0) == ld
    return v.as_strided((v.shape[0], ld), (ld, 1), v.storage_offset())


def as_rows(t):
    out = rows(t.shape[0], t.shape[1])
    out.copy_(t)
    return out


# ------------------------------------------------------------------ fp32 restatements of headops.py
class SimLinear:
    def __init__(self, w, b, relu, gw, gb, mut=None):
        self.w, self.b, self.relu, self.gw, self.gb, self.mut = w, b, relu, gw, gb, mut

    def fwd(self, x, save=True, addend=None):
        v = x @ self.w.t()
        if self.b is not None:
            v = v + self.b
        if addend is not None:
            v = v + addend
        y = as_rows(torch.relu(v) if self.relu else v)
        if save:
            self.x, self.y = x, y
        return y

    def bwd(self, dy, need_dx=True, accumulate=False):
        n, k = self.w.shape
        if self.relu:
            dyp = padded(dy)
            src = dyp if self.mut == "relu_mask_from_dy" else padded(self.y)
            dy = torch.where(src > 0, dyp, torch.zeros_like(dyp))[:, :n]
        gw, gb = dy.t() @ self.x, dy.sum(0)
        if accumulate and self.mut != "accumulate_overwrites":
            self.gw.add_(gw)
            if self.b is not None:
                self.gb.add_(gb)
        else:
            self.gw.copy_(gw)
            if self.b is not None:
                self.gb.copy_(gb)
        if not need_dx:
            return None
        dx = rows(dy.shape[0], k, C.SENT if self.mut == "dirty_padding" else 0.0)
        dx.copy_(dy @ self.w)
        return dx


class SimLSTM:
    def __init__(self, p, g, mut=None):
        self.p, self.g, self.mut = p, g, mut
        self.in_lin = SimLinear(p["w_ih"], None, False, g["w_ih"], None)
        self.hidden = p["w_hh"].shape[1]

    def fwd(self, x, S, N, h0=None, c0=None, save=True):
        H, p = self.hidden, self.p
        xg = self.in_lin.fwd(x, save=save)
        gates, hs, cs = torch.empty(S, N, 4 * H), torch.empty(S, N, H), torch.empty(S, N, H)
        for t in range(S):
            h_prev = h0 if t == 0 else hs[t - 1]
            c_prev = c0 if t == 0 else cs[t - 1]
            z = xg[t * N:(t + 1) * N] if h_prev is None else h_prev @ p["w_hh"].t() + xg[t * N:(t + 1) * N]
            z = (z + p["b_ih"] + p["b_hh"]).view(N, 4, H)
            i, f, g, o = torch.sigmoid(z[:, 0]), torch.sigmoid(z[:, 1]), torch.tanh(z[:, 2]), torch.sigmoid(z[:, 3])
            cs[t] = i * g if c_prev is None else f * c_prev + i * g
            hs[t] = o * torch.tanh(cs[t])
            gates[t] = torch.stack([i, f, g, o], 1).view(N, 4 * H)
        if save:
            self.S, self.N, self.gates, self.hs, self.cs = S, N, gates, hs, cs
            self.h0, self.c0 = (None if h0 is None else h0.clone()), (None if c0 is None else c0.clone())
            if self.mut == "c_prev_is_c_T" and c0 is not None:
                self.c0 = cs[S - 1]          # the caller's tensor, overwritten in place with the end state before the backward
        return hs.view(S * N, H), (hs[S - 1], cs[S - 1])

    def bwd(self, dh_all, need_dx=True):
        S, N, H, p, mut = self.S, self.N, self.hidden, self.p, self.mut
        dgates = torch.empty(S, N, 4 * H)
        dc = torch.zeros(N, H)
        dh_all = dh_all.reshape(S, N, H)
        dh = dh_all[S - 1]
        for t in reversed(range(S)):
            c_prev = self.c0 if t == 0 else self.cs[t - 1]
            i, f, g, o = self.gates[t].view(N, 4, H).unbind(1)
            tc = torch.tanh(self.cs[t])
            dct = dc + dh * o * (1 - tc * tc)
            df = torch.zeros_like(dct) if c_prev is None else dct * c_prev * f * (1 - f)
            dgates[t] = torch.stack([dct * g * i * (1 - i), df, dct * i * (1 - g * g), dh * tc * o * (1 - o)], 1).view(N, 4 * H)
            dc = dct * f
            if t > 0:
                dh = dh_all[t - 1] if mut == "no_recurrent_dh" else dgates[t] @ p["w_hh"] + dh_all[t - 1]
        dg = dgates.view(S * N, 4 * H)
        g_hh = self.g["w_hh"]
        g_hh.zero_()
        if self.h0 is not None and mut != "no_h0_term":
            g_hh.add_(dgates[0].t() @ self.h0)
        if S > 1:
            hs = self.hs[1:] if mut == "w_hh_pairs_hs_t" else self.hs[:S - 1]
            g_hh.add_(dg[N:].t() @ hs.reshape((S - 1) * N, H))
        self.g["b_ih"].copy_(dg.sum(0))
        if mut != "b_hh_unset":
            self.g["b_hh"].copy_(self.g["b_ih"])
        return self.in_lin.bwd(dg, need_dx=need_dx)


MUTANTS = ["no_recurrent_dh", "w_hh_pairs_hs_t", "no_h0_term", "b_hh_unset", "c_prev_is_c_T", "relu_mask_from_dy", "accumulate_overwrites",
           "dirty_padding", "td_d_pre_dropped"]


def _sent_like(d, keys):
    return {k: torch.full_like(d[k], C.SENT) for k in keys if d[k] is not None}


def _pad_ok(v):
    """1 when the padding columns of the row buffer behind v are exactly zero, inf otherwise (as a ratio)"""
    p = padded(v)[:, v.shape[1]:]
    return 0.0 if not bool((p != 0).any()) else float("inf")


def linear_ratios(case, mut=None):
    """every check of one LinearOp case on the restatement -> {label: err / bar}"""
    m, n, k, relu, bias = case
    d = C.linear_data(case)
    ref = [R.linear_run(d, case, F64, w) for w in (1, 2)]
    f32 = [R.linear_run(d, case, F32, w) for w in (1, 2)]
    g = _sent_like(d, ("w", "b"))
    op = SimLinear(d["w"], d["b"], relu, g["w"], g.get("b"), mut)
    y = op.fwd(as_rows(d["x1"]))
    dx = op.bwd(as_rows(d["dy1"]))
    got = dict(y=y, dx=dx, w=g["w"].clone())
    if bias:
        got["b"] = g["b"].clone()
    out = {"step1 " + k_: v[2] for k_, v in R.ratios(got, ref[0], R.yardstick(f32[0], ref[0]), M_CPU).items()}
    out["pad y"], out["pad dx"] = _pad_ok(y), _pad_ok(dx)
    op.fwd(as_rows(d["x2"]))
    op.bwd(as_rows(d["dy2"]), accumulate=True)
    keys = ("w", "b") if bias else ("w",)
    ref2 = {k_: ref[0][k_] + ref[1][k_] for k_ in keys}
    yard2 = R.yardstick({k_: f32[0][k_] + f32[1][k_] for k_ in keys}, ref2)
    out.update({"accumulate " + k_: v[2] for k_, v in R.ratios({k_: g[k_] for k_ in keys}, ref2, yard2, M_CPU).items()})
    return out


def lstm_got(case, d, mut=None):
    s, n, i, h, given = case
    g = _sent_like(d, ("w_ih", "w_hh", "b_ih", "b_hh"))
    op = SimLSTM(d, g, mut)
    h_all, (ht, ct) = op.fwd(as_rows(d["x"]), s, n, d["h0"], d["c0"])
    ht, ct = ht.clone(), ct.clone()
    dx = op.bwd(as_rows(d["dh"]))
    return dict(h_all=h_all, h_T=ht, c_T=ct, dx=dx, **g)


def lstm_ratios(case, mut=None):
    d = C.lstm_data(case)
    ref = R.lstm_run(d, case, F64)
    return {k: v[2] for k, v in R.ratios(lstm_got(case, d, mut), ref, R.yardstick(R.lstm_run(d, case, F32), ref), M_CPU).items()}


# the two-arm sequence graph (models/time_sensitive.py: TemporallyDependentStateEstimator) at a small size
TD_F, TD_H, TD_LEAD = 21, 8, (3, 2)


def td_mods():
    torch.manual_seed(77)
    return {"pre_measurement_rnn": nn.LSTM(TD_F, TD_H), "pre_measurement_fc": nn.Linear(TD_H, 7),
            "post_measurement_rnn": nn.LSTM(TD_F + 7, TD_H), "post_measurement_fc": nn.Linear(TD_H, 7)}


def td_got(mods, data, given, mut=None):
    """_heads_fwd / _backward_impl of the two-arm sequence model over the restated ops"""
    S, N = TD_LEAD
    F_ = TD_F
    p = {k: {n_: t.detach().clone() for n_, t in m.named_parameters()} for k, m in mods.items()}
    g = {k: {n_: torch.full_like(t, C.SENT) for n_, t in v.items()} for k, v in p.items()}
    lp = lambda k: {a: p[k][b] for a, b in (("w_ih", "weight_ih_l0"), ("w_hh", "weight_hh_l0"), ("b_ih", "bias_ih_l0"), ("b_hh", "bias_hh_l0"))}
    lg = lambda k: {a: g[k][b] for a, b in (("w_ih", "weight_ih_l0"), ("w_hh", "weight_hh_l0"), ("b_ih", "bias_ih_l0"), ("b_hh", "bias_hh_l0"))}
    pre_rnn, post_rnn = SimLSTM(lp("pre_measurement_rnn"), lg("pre_measurement_rnn")), SimLSTM(lp("post_measurement_rnn"), lg("post_measurement_rnn"))
    pre_fc = SimLinear(p["pre_measurement_fc"]["weight"], p["pre_measurement_fc"]["bias"], False, g["pre_measurement_fc"]["weight"], g["pre_measurement_fc"]["bias"])
    post_fc = SimLinear(p["post_measurement_fc"]["weight"], p["post_measurement_fc"]["bias"], False, g["post_measurement_fc"]["weight"], g["post_measurement_fc"]["bias"])
    feat = as_rows(data["feat"])
    hp, hc1 = pre_rnn.fwd(feat, S, N)
    pre = pre_fc.fwd(as_rows(hp))
    post_in = rows(S * N, F_ + 7)
    post_in[:, :F_] = feat
    post_in[:, F_:] = pre - data["x0bar"]
    hq, hc2 = post_rnn.fwd(post_in, S, N)
    post = post_fc.fwd(as_rows(hq))
    d_pre, d_post = (data["d_outs"][i] if given[i] else None for i in (0, 1))
    d = post_fc.bwd(as_rows(d_post) if d_post is not None else rows(S * N, 7))
    d = post_rnn.bwd(d)
    d_rows = d[:, :F_].clone()
    d_pre_total = d[:, F_:F_ + 7].clone()
    if d_pre is not None and mut != "td_d_pre_dropped":
        d_pre_total = d_pre_total + d_pre
    d = pre_rnn.bwd(pre_fc.bwd(as_rows(d_pre_total)))
    d_rows.add_(d)
    got = {"out0": pre, "out1": post, "d_rows": d_rows, "state.pre.h": hc1[0], "state.pre.c": hc1[1], "state.post.h": hc2[0], "state.post.c": hc2[1]}
    for k, v in g.items():
        for n_, t in v.items():
            got[k + "." + n_] = t
    return got


def td_ratios(given, mut=None):
    mods = td_mods()
    data = C.graph_data("td", TD_LEAD, TD_F, {})
    ref = R.graph_run("td", mods, TD_LEAD, data, F64, given)
    yard = R.yardstick(R.graph_run("td", mods, TD_LEAD, data, F32, given), ref)
    return {k: v[2] for k, v in R.ratios(td_got(mods, data, given, mut), ref, yard, M_CPU).items()}


def all_ratios(mut=None):
    out = {}
    for case in C.LINEAR_CASES:
        out.update({"linear %s %s" % (C.case_id(case), k): v for k, v in linear_ratios(case, mut).items()})
    for case in C.LSTM_CASES:
        out.update({"lstm %s %s" % (C.case_id(case), k): v for k, v in lstm_ratios(case, mut).items()})
    for given in ((True, True), (True, False), (False, True)):
        out.update({"td %s %s" % (given, k): v for k, v in td_ratios(given, mut).items()})
    return out


# ------------------------------------------------------------------ the tests
@pytest.mark.parametrize("case", C.LSTM_CASES, ids=C.case_id)
def test_lstm_reference_equals_the_oracle(case):
    s, n, i, h, given = case
    d = C.lstm_data(case)
    ref = R.lstm_run(d, case, F64)
    p = [d[k].double().requires_grad_() for k in ("w_ih", "w_hh", "b_ih", "b_hh")]
    x = d["x"].double().view(s, n, i).requires_grad_()
    out, ht, ct = po.lstm_forward(x, *p, h0=d["h0"].double() if given else None, c0=d["c0"].double() if given else None)
    g = torch.autograd.grad(out, [x] + p, d["dh"].double().view(s, n, h))
    mine = dict(h_all=out.reshape(s * n, h), h_T=ht, c_T=ct, dx=g[0].reshape(s * n, i), w_ih=g[1], w_hh=g[2], b_ih=g[3], b_hh=g[4])
    for k, v in ref.items():
        assert float((mine[k].detach() - v).abs().max()) <= 1e-12 * max(1.0, float(v.abs().max())), k


def _all_refs():
    for case in C.LINEAR_CASES:
        d = C.linear_data(case)
        for w in (1, 2):
            yield "linear %s pair %d" % (C.case_id(case), w), R.linear_run(d, case, F64, w), R.linear_run(d, case, F32, w), ()
    for case in C.LSTM_CASES:
        d = C.lstm_data(case)
        yield "lstm %s" % C.case_id(case), R.lstm_run(d, case, F64), R.lstm_run(d, case, F32), C.LSTM_ZERO.get(case, ())
    mods, data = td_mods(), C.graph_data("td", TD_LEAD, TD_F, {})
    yield "td graph", R.graph_run("td", mods, TD_LEAD, data, F64), R.graph_run("td", mods, TD_LEAD, data, F32), ()


def test_no_reference_tensor_is_vacuous_and_every_yardstick_is_small():
    for label, ref, f32, zeros in _all_refs():
        yard = R.yardstick(f32, ref)
        for k, v in ref.items():
            if k in zeros:
                assert not bool((v != 0).any()), (label, k)
            else:
                assert float(v.abs().max()) > 1e-3, (label, k, float(v.abs().max()))
            assert yard[k] == yard[k] and yard[k] < 1e-5, (label, k, yard[k])


def test_the_restatement_passes_every_bar():
    res = all_ratios()
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    print("worst err/bar of the restatement at m = %d: %.3f (%s)" % (M_CPU, max(res.values()), max(res, key=res.get)))
    assert not bad, bad


@pytest.mark.parametrize("mut", MUTANTS)
def test_mutants_are_rejected(mut):
    res = all_ratios(mut)
    worst = max(res, key=res.get)
    print("%s: worst err/bar %.3g (%s)" % (mut, res[worst], worst))
    assert res[worst] >= 100.0, "%s passes: its worst err/bar is %.3g (%s)" % (mut, res[worst], worst)
