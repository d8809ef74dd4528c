"""LinearOp / LSTMOp of headops.py called on their own, and the head graphs of the five model classes with the trunk cut off, against
fp64 autograd on the CPU (tests/_headops_ref.py) on the cases of tests/_headops_cases.py.  The references, the bars and the faults they
reject are judged on the CPU by tests/test_headops_cpu.py.

(a) Op level: parameters on the device with sentinel-filled gradient views, inputs from headops.new_rows.
  - LinearOp: every output is one launch on known operands, so each is held per element with the bounds the kernels' own tests use
    (tests/_bounds.py, tests/_stem_bounds.py): y by linear_ref with epi = |acc| + |bias| + |addend|, dW by gemm_ref_tn (accumulating:
    the two accumulators and their Q added up, one fp32 add of them), db by colsum_ref, dx by gemm_ref on dy masked with the op's own
    y > 0, the mask itself bit for bit.  Besides: need_dx=False, a save=False forward in between, a halved weight (the padded copy
    cannot go stale), caller-owned strided out / addend, exactly zero padding columns.
  - LSTMOp: outputs compound over S steps: the yardstick bar of _headops_ref.py, e <= M_BAR y + EPI u32 per tensor.  Besides: the
    same op twice and two ops interleaved (bit for bit), need_dx=False, an initial state overwritten between forward and backward.
(b) The five head graphs: each family built once (module-scoped fixture), _features_bwd replaced by a recorder, _heads_fwd /
  _backward_impl driven with random rows; every output, the recorded row gradient (all columns), every head parameter's gradient and
  the LSTMs' end states against fp64 autograd over deep copies of the model's own nn modules, at the same bar; the two-output
  families with each output gradient None in turn; the sequence families again in rollout mode from a non-zero carried state.

M_BAR = 4, measured on the MI355X: the smallest of 2, 3, 4, 6, 8 at which the worst tensor sits at <= 0.5 of its bar (the device
sigmoid's __expf is allowed more than torch's exp: TR in tests/_bounds.py).  Worst e / bar over all 602 figures: m = 1: 1.61, m = 2:
0.83, m = 3: 0.56, m = 4: 0.42, m = 6: 0.29, m = 8: 0.25.  At m = 4, worst per tensor kind:
  LSTMOp:  h_all 0.31, h_T 0.31, c_T 0.25, dx 0.26, w_ih 0.29, w_hh 0.40, b_ih 0.29, b_hh 0.29
  graphs:  out0 0.30, out1 0.17, d_rows 0.26, end state h 0.34, c 0.35; LSTM weight_ih 0.41, weight_hh 0.32, bias_ih 0.42, bias_hh 0.42;
           Linear weight 0.40, bias 0.33   (the worst of all: the two-arm sequence graph at (S, N) = (2, 9), both gradients given)
  LinearOp, err / bound of the per-element bounds: y 0.17, dW 0.19 (accumulating 0.20), db 0.09 (0.09), dx 0.20, strided 0.16
Without the clones LSTMOp.fwd keeps of a given (h0, c0), the rollout step and the overwritten-state test fail, e.g.
  graph tdo (3, 2) rollout: d_rows: e 0.558, rnn.weight_ih_l0: e 0.939, rnn.weight_hh_l0: e 1.28, rnn.bias_ih_l0: e 1.09,
  rnn.bias_hh_l0: e 1.09 (bars of 2e-6 to 4e-6 at m = 2 then) -- the backward read the end state where step 0 needs the initial one."""
import copy

import pytest
import torch
import torch.nn.functional as F

import _bounds as B
import _headops_cases as C
import _headops_ref as R
import _stem_bounds as SB

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from rgb_proprioceptive_pose_estimator_amd import headops, ops
    from rgb_proprioceptive_pose_estimator_amd._lib import RPE_F32, lib

    from _helpers import CASES, build

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
M_BAR = 4


def dd(t):
    return t.detach().to(DEV, F64)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _param(t):
    p = torch.nn.Parameter(t.to(DEV).contiguous())
    p._rpe_grad = torch.full_like(p.data, C.SENT)
    return p


def _refill(ps):
    for p in ps:
        p._rpe_grad.fill_(C.SENT)


def _grads(ps):
    return [p._rpe_grad.clone() for p in ps]


def _rows(t):
    v = headops.new_rows(t.shape[0], t.shape[1], DEV)
    v.copy_(t.to(DEV))
    return v


def _padded(v):
    ld = ops.pad4(v.shape[1])
    assert v.stride(0) == ld
    return v.as_strided((v.shape[0], ld), (ld, 1), v.storage_offset())


def _pad_zero(v):
    return not bool((_padded(v)[:, v.shape[1]:] != 0).any())


def _within(got, r, label, out=None, epi=None):
    ref = r.acc if out is None else out
    return B.assert_within(got, ref, B.bound(r, F32, out=ref, epi=epi), label)


# ------------------------------------------------------------------ (a) LinearOp
@pytest.mark.parametrize("case", C.LINEAR_CASES, ids=C.case_id)
def test_linear_op(case):
    m, n, k, relu, bias = case
    tag = "LinearOp %s " % C.case_id(case)
    d = C.linear_data(case)
    w = _param(d["w"])
    b = _param(d["b"]) if bias else None
    ps = [w] + ([b] if bias else [])
    op = headops.LinearOp(w, b, relu=relu)
    if case == C.SPLIT_K_CASE:
        assert lib.rpe_linear_fwd_workspace_bytes(RPE_F32, m, n, ops.pad4(k)) > 0, "this shape is expected to split K"
    x1, x2, dy1, dy2 = (_rows(d[key]) for key in ("x1", "x2", "dy1", "dy2"))
    w64 = dd(d["w"])
    b64 = dd(d["b"]) if bias else torch.zeros(n, dtype=F64, device=DEV)

    def y_check(y, x, w64, label, add64=None):
        r = B.linear_ref(dd(x), w64)
        v, epi = r.acc + b64, r.acc.abs() + b64.abs()
        if add64 is not None:
            v, epi = v + add64, epi + add64.abs()
        _within(y, r, tag + label, out=F.relu(v) if relu else v, epi=epi)

    def masked(y, dy):
        """dy through the op's own ReLU mask; the mask kernel itself bit for bit"""
        if not relu:
            return dy
        yp, dyp = _padded(y), _padded(dy)
        want = torch.where(yp > 0, dyp, torch.zeros_like(dyp))
        assert _same_bits(ops.relu_bwd(yp, dyp), want), tag + "relu_bwd is not dy * (y > 0)"
        return want[:, :n]

    # forward, backward
    y1 = op.fwd(x1)
    y_check(y1, x1, w64, "y")
    assert tuple(y1.shape) == (m, n) and _pad_zero(y1), tag + "padding columns of y"
    dx1 = op.bwd(dy1)
    dym1 = masked(y1, dy1)
    r_w1 = B.gemm_ref_tn(dd(dym1), dd(x1))
    _within(w._rpe_grad, r_w1, tag + "dW")
    if bias:
        B.assert_within(b._rpe_grad, *SB.colsum_ref(dym1, n), tag + "db", layout="c")
    _within(dx1, B.gemm_ref(dd(dym1), w64.t().contiguous()), tag + "dx")
    assert tuple(dx1.shape) == (m, k) and _pad_zero(dx1), tag + "padding columns of dx"
    g1 = _grads(ps)

    # need_dx=False: None, the same gradient bits
    _refill(ps)
    assert op.bwd(dy1, need_dx=False) is None
    assert all(_same_bits(p._rpe_grad, g) for p, g in zip(ps, g1)), tag + "need_dx=False changed the gradients"

    # a forward that keeps nothing, between the saving forward and its backward
    _refill(ps)
    op.fwd(x2, save=False)
    dx1b = op.bwd(dy1)
    assert _same_bits(dx1b, dx1) and all(_same_bits(p._rpe_grad, g) for p, g in zip(ps, g1)), tag + "a save=False forward changed the backward"

    # accumulate: a second step on fresh inputs adds to the gradients of the first
    y2 = op.fwd(x2)
    y_check(y2, x2, w64, "y (second input)")
    assert op.bwd(dy2, need_dx=False, accumulate=True) is None
    dym2 = masked(y2, dy2)
    r_w2 = B.gemm_ref_tn(dd(dym2), dd(x2))
    r_sum = B.Ref(r_w1.acc + r_w2.acc, r_w1.Q + r_w2.Q, r_w1.K)       # two sums and one fp32 add of them
    _within(w._rpe_grad, r_sum, tag + "dW accumulate", epi=r_sum.acc.abs())
    if bias:
        B.assert_within(b._rpe_grad, *SB.colsum_ref(dym2, n, g1[1]), tag + "db accumulate", layout="c")

    # the next forward sees a changed weight (no stale padded copy)
    w.data.mul_(0.5)
    y_check(op.fwd(x1, save=False), x1, w64 * 0.5, "y after weight.mul_(0.5)")

    # caller-owned out and addend with row strides larger than the column count
    ld = ops.pad4(n) + 8
    big = torch.full((m, ld), C.SENT, dtype=F32, device=DEV)
    addb = torch.full((m, ld), C.SENT, dtype=F32, device=DEV)
    addb[:, :n] = d["add"].to(DEV)
    out = op.fwd(x1, save=False, out=big[:, :n], addend=addb[:, :n])
    assert out.data_ptr() == big.data_ptr() and out.stride(0) == ld
    y_check(big[:, :n], x1, w64 * 0.5, "y strided out + addend", add64=dd(d["add"]))
    assert bool((big[:, ops.pad4(n):] == C.SENT).all()), tag + "wrote past the row's columns"


# ------------------------------------------------------------------ (a) LSTMOp
LSTM_KEYS = ("w_ih", "w_hh", "b_ih", "b_hh")
_LSTM_REF = {}


def _lstm_ref(case, seed=0):
    """(fp64 reference, yardstick) of a case, computed once"""
    if (case, seed) not in _LSTM_REF:
        d = C.lstm_data(case, seed)
        ref = R.lstm_run(d, case, F64)
        _LSTM_REF[(case, seed)] = (ref, R.yardstick(R.lstm_run(d, case, F32), ref))
    return _LSTM_REF[(case, seed)]


def _lstm_fwd(op, d, case, clobber=False):
    s, n, i, h, given = case
    h0, c0 = (d["h0"].to(DEV), d["c0"].to(DEV)) if given else (None, None)
    h_all, (ht, ct) = op.fwd(_rows(d["x"]), s, n, h0, c0)
    got = dict(h_all=h_all.clone(), h_T=ht.clone(), c_T=ct.clone())
    if clobber:      # what rollout mode does with its carried state, directly after the forward
        h0.copy_(ht)
        c0.copy_(ct)
    return got


def _lstm_bwd(op, ps, d, got, need_dx=True):
    got = dict(got)
    got["dx"] = op.bwd(_rows(d["dh"]), need_dx=need_dx)
    got.update({k: p._rpe_grad.clone() for k, p in zip(LSTM_KEYS, ps)})
    return got


def _lstm_new(d):
    ps = [_param(d[k]) for k in LSTM_KEYS]
    return ps, headops.LSTMOp(*ps)


def _assert_same(a, b, label, skip=()):
    for k in a:
        if k not in skip:
            assert _same_bits(a[k], b[k]), "%s: %s differs" % (label, k)


@pytest.mark.parametrize("case", C.LSTM_CASES, ids=C.case_id)
def test_lstm_op(case):
    s, n, i, h, given = case
    tag = "LSTMOp %s" % C.case_id(case)
    d, (ref, yard) = C.lstm_data(case), _lstm_ref(case)
    ps, op = _lstm_new(d)
    got = _lstm_bwd(op, ps, d, _lstm_fwd(op, d, case))
    assert tuple(got["dx"].shape) == (s * n, i) and _pad_zero(got["dx"]), tag + ": padding columns of dx"
    R.assert_bars(tag, got, ref, yard, M_BAR)
    for k in C.LSTM_ZERO.get(case, ()):      # (the bar already demands it: rel_err is inf for a non-zero result against a zero reference)
        assert not bool((got[k] != 0).any()), "%s: %s must be exactly zero" % (tag, k)

    # the same op again: bit-equal outputs and gradients
    _refill(ps)
    _assert_same(got, _lstm_bwd(op, ps, d, _lstm_fwd(op, d, case)), tag + " run twice")

    # need_dx=False: None, the same gradient bits
    _refill(ps)
    again = _lstm_bwd(op, ps, d, _lstm_fwd(op, d, case), need_dx=False)
    assert again["dx"] is None
    _assert_same(got, again, tag + " need_dx=False", skip=("dx",))

    # two ops interleaved: each as on its own
    d_b, (ref_b, yard_b) = C.lstm_data(case, 1), _lstm_ref(case, 1)
    ps_b, op_b = _lstm_new(d_b)
    solo_b = _lstm_bwd(op_b, ps_b, d_b, _lstm_fwd(op_b, d_b, case))
    R.assert_bars(tag + " (second op)", solo_b, ref_b, yard_b, M_BAR)
    _refill(ps + ps_b)
    f_a = _lstm_fwd(op, d, case)
    f_b = _lstm_fwd(op_b, d_b, case)
    _assert_same(got, _lstm_bwd(op, ps, d, f_a), tag + " interleaved, first op")
    _assert_same(solo_b, _lstm_bwd(op_b, ps_b, d_b, f_b), tag + " interleaved, second op")


@pytest.mark.parametrize("case", [c for c in C.LSTM_CASES if c[4]], ids=C.case_id)
def test_lstm_saving_forward_owns_its_initial_state(case):
    """(h0, c0) overwritten in place with (h_T, c_T) between the forward and the backward, as rollout mode does with its carried
    state: the backward still starts from the state the forward read."""
    d, (ref, yard) = C.lstm_data(case), _lstm_ref(case)
    ps, op = _lstm_new(d)
    got = _lstm_bwd(op, ps, d, _lstm_fwd(op, d, case, clobber=True))
    R.assert_bars("LSTMOp %s, state overwritten" % C.case_id(case), got, ref, yard, M_BAR)


# ------------------------------------------------------------------ (b) the five head graphs
def _head_modules(kind, model):
    if kind == "n":
        mods = {"pre_fc%d" % i: getattr(model, "pre_fc%d" % i) for i in range(model.n_pre_hidden)}
        mods.update({"post_fc%d" % i: getattr(model, "post_fc%d" % i) for i in range(model.n_post_hidden)})
        return mods
    if kind == "no":
        return {"fc%d" % i: getattr(model, "fc%d" % i).module for i in range(model.n_fc)}
    if kind == "td":
        return {k: getattr(model, k) for k in ("pre_measurement_rnn", "pre_measurement_fc", "post_measurement_rnn", "post_measurement_fc")}
    if kind == "tdo":
        return {"rnn": model.rnn.module, "fc0": model.fc.module[0], "fc1": model.fc.module[1]}
    return {"img_rnn": model.img_rnn.module, "proprio_rnn": model.proprio_rnn.module, "fc0": model.fc.module[0], "fc1": model.fc.module[1]}


class _Graph:
    def __init__(self, kind):
        cfg = CASES[kind][0]
        torch.manual_seed(4321 + len(kind))
        model = build(kind, cfg, torch.float32)
        self.kind, self.model = kind, model
        self.live = _head_modules(kind, model)
        self.mods = copy.deepcopy(self.live)           # the reference's modules: CPU fp32 copies, taken before the arena holds the values
        model.cuda()
        model._materialize(next(model.parameters()).device)
        self.rec = []
        model._features_bwd = self.rec.append          # the trunk is cut off: the row gradient is recorded instead
        self.fdim = model.latent_dim + model.aux_latent_dim
        self.ld = {"n": self.fdim, "td": self.fdim}.get(kind) or model.input_dim
        self.rnn_ops, self.hidden = {}, {}
        if kind == "td":
            self.rnn_ops = {"pre": model._pre_rnn, "post": model._post_rnn}
        elif kind == "tdo":
            self.rnn_ops = {"rnn": model._rnn}
        elif kind == "tdo_v2":
            self.rnn_ops = {"img": model._img_rnn, "proprio": model._prop_rnn}
        self.hidden = {tag: op.hidden for tag, op in self.rnn_ops.items()}
        self.head_params = {id(p) for mod in self.live.values() for p in mod.parameters()}


@pytest.fixture(scope="module")
def graphs():
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = _Graph(kind)
        return made[kind]

    yield get
    made.clear()


def _graph_step(G, lead, data, given, state=None):
    """one _heads_fwd / _backward_impl of the model on `data` -> the tensors graph_run names"""
    model = G.model
    rows_n = data["feat"].shape[0]
    rows = headops.new_rows(rows_n, G.ld, DEV)
    rows[:, :G.fdim] = data["feat"].to(DEV)
    model._arena.grad.fill_(C.SENT)
    G.rec.clear()
    carried = {}
    try:
        if state is not None:
            model.rollout = True
            model._carried = {tag: (h.to(DEV).clone(), c.to(DEV).clone()) for tag, (h, c) in state.items()}
        outs = model._heads_fwd(rows, lead, data["x0bar"].to(DEV), save=True)
        end = {tag: (op.hs[-1].clone(), op.cs[-1].clone()) for tag, op in G.rnn_ops.items()}
        model._backward_impl([data["d_outs"][i].to(DEV).view(o.shape) if given[i] else None for i, o in enumerate(outs)])
        torch.cuda.synchronize()
        if state is not None:
            carried = dict(model._carried)
    finally:
        if state is not None:
            model.rollout = False
            model._carried = {}
    assert len(G.rec) == 1, "the backward hands the row gradient to the trunk exactly once"
    got = {"out%d" % i: o.reshape(rows_n, 7) for i, o in enumerate(outs)}
    got["d_rows"] = G.rec[0]
    assert G.rec[0].shape[0] == rows_n and _pad_zero(G.rec[0]), "padding columns of the row gradient"
    for name, mod in G.live.items():
        for pn, p in mod.named_parameters():
            got["%s.%s" % (name, pn)] = p._rpe_grad.clone()
    for tag, (h, c) in end.items():
        if state is not None:    # rollout: the carried state is that forward's end state
            assert _same_bits(carried[tag][0], h) and _same_bits(carried[tag][1], c), "carried state of %s is not the forward's (h_T, c_T)" % tag
            h, c = carried[tag]
        got["state.%s.h" % tag], got["state.%s.c" % tag] = h, c
    for name, p in model.named_parameters():      # trunk and aux parameters: the graph does not touch their gradients
        if id(p) not in G.head_params:
            assert bool((p._rpe_grad == C.SENT).all()), "the head graph wrote the gradient of %s" % name
    return got


GRAPH_PARAMS = [(kind, lead) for kind, leads in C.GRAPH_LEADS.items() for lead in leads]


def _graph_id(p):
    return "%s-%s" % (p[0], "x".join(str(v) for v in p[1]))


@pytest.mark.parametrize("kind,lead", GRAPH_PARAMS, ids=[_graph_id(p) for p in GRAPH_PARAMS])
def test_head_graph(graphs, kind, lead):
    G = graphs(kind)
    data = C.graph_data(kind, lead, G.fdim, G.hidden)
    variants = [(True, True), (True, False), (False, True)] if kind in C.TWO_OUTPUTS else [(True,)]
    for given in variants:
        ref = R.graph_run(kind, G.mods, lead, data, F64, given)
        yard = R.yardstick(R.graph_run(kind, G.mods, lead, data, F32, given), ref)
        got = _graph_step(G, lead, data, given)
        assert set(got) == set(ref)
        R.assert_bars("graph %s %s given=%s" % (kind, lead, "".join(str(int(g)) for g in given)), got, ref, yard, M_BAR)


SEQ_PARAMS = [p for p in GRAPH_PARAMS if p[0] in C.SEQUENCE]


@pytest.mark.parametrize("kind,lead", SEQ_PARAMS, ids=[_graph_id(p) for p in SEQ_PARAMS])
def test_head_graph_rollout_train_step(graphs, kind, lead):
    """The same step with model.rollout = True from a non-zero carried state: gradients as from the state the forward read, and the
    carried state afterwards that forward's (h_T, c_T)."""
    G = graphs(kind)
    data = C.graph_data(kind, lead, G.fdim, G.hidden)
    given = (True, True) if kind in C.TWO_OUTPUTS else (True,)
    ref = R.graph_run(kind, G.mods, lead, data, F64, given, state=data["state"])
    yard = R.yardstick(R.graph_run(kind, G.mods, lead, data, F32, given, state=data["state"]), ref)
    got = _graph_step(G, lead, data, given, state=data["state"])
    assert set(got) == set(ref)
    R.assert_bars("graph %s %s rollout" % (kind, lead), got, ref, yard, M_BAR)
