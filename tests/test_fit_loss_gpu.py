"""The loss options, the metrics and predict on the MI355X (csrc/nn_train_loss.hip ft_k_loss_opt, ft_k_metrics and
ft_k_metrics_reduce; include/corintho_hip.h, "loss and metrics").  At the defaults a fit is what it was, bit for bit; a
power-of-two pair of loss weights scales the gradient exactly; general values are held to the float64 restatement of
tests/fit_ref_loss.py by the rule of tests/test_fit_gpu.py (the device's error at most 4 x the float32 restatement's,
plus a small floor); the metrics are judged on the device's own logits, read back with predict, so the accuracies are
exact counts.

Shapes: both networks, a packed set of 48 samples (384 virtual rows), batches of 64 and one partial batch of 37."""
import ctypes as C

import numpy as np
import pytest

from corintho_ai_amd import NET_MLP12X100, NET_RESCNN4, LossOptions, expand_samples, fit, nets
from corintho_ai_amd import _lib
from corintho_ai_amd.fit import HISTORY_KEYS, METRIC_HISTORY_KEYS, METRIC_NAMES, Fitter, fit_samples, split_index
from tests import fit_ref, fit_ref_rescnn4
from tests import fit_ref_loss as L
from tests import fit_ref_weighted as RW
from tests import fit_ref_step as S
from tests.fit_ref_step import within as _within

pytestmark = pytest.mark.gpu

KINDS = {"mlp12x100": (NET_MLP12X100, nets.init_mlp12x100), "rescnn4": (NET_RESCNN4, nets.init_rescnn4)}
NETS = pytest.mark.parametrize("net", list(KINDS))
LR = 1e-3
ERR_ARG, ERR_STATE = -1, -4
BATCHES = (1, 17, 64)
EVERYTHING = LossOptions(value_weight=0.7, policy_weight=1.3, label_smoothing=0.1, value_loss="huber", huber_delta=0.5)
# the cases of test_general_values_against_float64: (name, loss, with sample weights)
GENERAL = [("weights", LossOptions(value_weight=0.7, policy_weight=1.3), False),
           ("smoothing", LossOptions(label_smoothing=0.1), False),
           ("huber", LossOptions(value_loss="huber", huber_delta=0.5), False),
           ("everything", EVERYTHING, True)]
FLOATS = ("mean_absolute_error", "policy_entropy", "target_entropy")


def packed():
    s, z, p = fit_ref.synthetic_samples(48, 23)
    return np.concatenate([s, p], axis=1).astype(np.float32), z


def expanded(_cdll=None):
    """the 384 virtual rows of packed() as arrays: (states, evals, probs)"""
    return expand_samples(*packed(), _cdll=_cdll)


def sample_weights():
    """one weight per packed sample, with zeros among them; sums of them are exact in float32"""
    return np.random.default_rng(31).choice(np.array([0.0, 0.25, 0.5, 1.0, 2.0], np.float32), 48)


def rows(n, seed=0):
    return np.random.default_rng(300 + seed).permutation(384)[:n].astype(np.int32)


def general_rng(name):
    return np.random.default_rng(400 + [g[0] for g in GENERAL].index(name))


def general_candidates(weighted, B):
    """the rows a case of test_general_values_against_float64 draws from: all of them, but a single weighted row is one
    of weight > 0 (the gradient of a batch whose only row has weight 0 is 0: nothing to judge)"""
    if not (weighted and B == 1):
        return None
    return np.flatnonzero(sample_weights()[np.arange(384) // 8] > 0)


def same(x, y):
    return np.asarray(x).tobytes() == np.asarray(y).tobytes()


class Ctx:
    """one fitter of `net` on the packed set, reused by the tests of this file: every use sets everything it relies on"""

    def __init__(self, net):
        self.net = net
        self.kind, init = KINDS[net]
        self.ref = S.BASE[net]
        self.w = init(5, bn_noise=True)
        self.zeros = np.zeros_like(self.w)
        self.data = expanded()
        self.f = Fitter(max_batch=64, net=self.kind)
        self.f.add_samples(*packed())

    def start(self, loss=None, metrics=False, top_k=5, weights=None, w=None):
        f = self.f
        f.set_options(None)
        f.set_adam(None)
        f.set_loss(loss)
        f.set_metrics(metrics, top_k)
        f.set_sample_weights(weights)
        f.set_weights(self.w if w is None else w)
        f.set_optimizer(self.zeros, self.zeros, 0)
        return f


_CTX = {}


@pytest.fixture(scope="module")
def ctxs():
    yield _CTX
    for c in _CTX.values():
        c.f.close()
    _CTX.clear()


@pytest.fixture
def ctx(ctxs, net):
    if net not in ctxs:
        ctxs[net] = Ctx(net)
    return ctxs[net]


def run_of(f, w):
    """gradients(), three steps (64, 64 and 37 rows) and a validation pass: everything they leave, as bytes"""
    f.set_weights(w)
    f.set_optimizer(np.zeros_like(w), np.zeros_like(w), 0)
    g, gl = f.gradients(rows(37, 1))
    losses, per = f.train(rows(165), 64, LR, batch_losses=True)
    m, v, it = f.get_optimizer()
    assert it == 3 and per.shape == (3, 3)
    ev = f.evaluate(268, 116, 64)
    return {"gradient": g.tobytes(), "gradient losses": gl, "weights": f.get_weights().tobytes(), "m": m.tobytes(),
            "v": v.tobytes(), "batch losses": per.tobytes(), "losses": losses, "evaluate": ev}


# ---------------------------------------------------------------------------------------------------- 1. defaults
@NETS
def test_defaults_change_nothing(net):
    """a fitter that never heard of the section, one set to other values and back, and one with metrics on: the same
    bytes from gradients(), three steps and evaluate"""
    kind, init = KINDS[net]
    w = init(5, bn_noise=True)
    outs = {}
    for how in ("never", "back", "metrics"):
        with Fitter(max_batch=64, net=kind) as f:
            f.add_samples(*packed())
            if how == "back":
                f.set_loss(LossOptions(value_weight=2.0, label_smoothing=0.1, value_loss="huber", huber_delta=0.5))
                f.set_weights(w)
                f.set_optimizer(np.zeros_like(w), np.zeros_like(w), 0)
                f.train(rows(101, 2), 64, LR)
                f.set_loss(None)
                assert f.get_loss() == LossOptions()
            if how == "metrics":
                f.set_metrics(True, 5)
            outs[how] = run_of(f, w)
            if how == "metrics":
                assert f.metrics()["rows"] == 116
            else:
                assert _lib.load().ca_fitter_metrics(f._h, C.byref(_lib.CaFitMetrics(struct_size=C.sizeof(_lib.CaFitMetrics)))) == ERR_STATE
    for k in outs["never"]:
        assert outs["never"][k] == outs["back"][k] == outs["metrics"][k], k
    assert outs["never"]["weights"] != w.tobytes()


# ---------------------------------------------------------------------------------------------------- 2. exact scaling
@NETS
def test_loss_weights_of_two_double_exactly(ctx):
    """(2, 0.5) against the defaults (1, 0.25): a power of two commutes with every float32 product and sum, so the
    gradient doubles bit for bit (the argument of test_fit_weights_gpu.py::test_weights_of_two_double_exactly)"""
    for B in BATCHES:
        r = rows(B, 10 + B)
        g1, l1 = ctx.start().gradients(r)
        g2, l2 = ctx.start(LossOptions(value_weight=2.0, policy_weight=0.5)).gradients(r)
        assert g1.any()
        assert same(g2, np.float32(2.0) * g1), B
        assert l2[1:] == l1[1:] and l2[0] == 2.0 * l1[0], B


# ---------------------------------------------------------------------------------------------------- 3. general values
@NETS
def test_general_values_against_float64(ctx):
    """loss weights (0.7, 1.3); label smoothing 0.1; Huber(0.5); and all of them with sample weights -- at B = 1, 17, 64.
    Every trainable tensor's gradient and the three losses by the rule of test_gradients_of_one_batch; a batch whose
    float64 restatement has a ReLU input within 2e-7 of its kink is drawn again (three times at the most) and then held
    to 5 % of the tensor's largest entry, and at most a quarter of the cases may be such.  With Huber a batch is also
    drawn again while a row lies within 1e-4 of |e| = delta, where the value gradient jumps; the draws (fit_ref_loss.
    draw_batch) never look at the device, and tests/test_fit_loss_cpu.py checks that they all succeed."""
    ref, w, data = ctx.ref, ctx.w, ctx.data
    sw = sample_weights()
    bad, cases, kinked = [], 0, 0
    for name, loss, weighted in GENERAL:
        rng = general_rng(name)
        f = ctx.start(loss, weights=sw if weighted else None)
        for B in BATCHES:
            r, relu_ok, huber_ok = S.draw_batch(ref, w, data[0], data[1], rng, B, loss, general_candidates(weighted, B))
            assert huber_ok, (name, B)
            assert not weighted or B == 1 or (sw[r // 8] == 0).any()  # a row of weight 0 is in the larger batches
            g, losses = f.gradients(r)
            s, z, p = (a[r] for a in data)
            swr = sw[r // 8] if weighted else None
            g64, l64, _ = S.loss_and_grad(ref, w, s, z, p, loss, swr)
            g32, l32, _ = S.loss_and_grad(ref, w, s, z, p, loss, swr, dtype=ref.torch.float32)
            assert not g[ref.stat_mask()].any(), "gradient at a moving statistic"
            kink = not relu_ok
            cases += 1
            kinked += kink
            tag = "%s %s B=%d" % (ctx.net, name, B)
            for tname, sl, scale in RW.tensors(ref):
                top = float(np.max(np.abs(g64[scale])))
                ok, ed, e3 = _within(g[sl], g32[sl], g64[sl], 2e-5 * top + 1e-12)
                if kink:
                    ok = ed <= 0.05 * top + 1e-12
                print("%s %-10s kink=%d dev %.3e f32 %.3e top %.3e%s" % (tag, tname, kink, ed, e3, top, "" if ok else "  FAIL"))
                if not ok:
                    bad.append((tag, tname, kink, ed, e3, top))
            ok, ed, e3 = _within(losses, l32, l64, 1e-6 * abs(l64[0]))
            print("%s losses dev %.3e f32 %.3e" % (tag, ed, e3))
            if not ok:
                bad.append((tag, "losses", ed, e3))
            assert g.any()
    assert not bad, "device error above 4 x float32's: %s" % bad[:12]
    assert cases == 12 and kinked <= cases // 4, (kinked, cases)


# ---------------------------------------------------------------------------------------------------- 4. predict
def outputs_within(got, ref, w, states, train, what):
    """the heads of predict against the float64 forward by the _within rule, floor 1e-6 of the output's scale"""
    o64 = S.predict(ref, w, states, train)
    o32 = S.predict(ref, w, states, train, ref.torch.float32)
    for name, d, a32, a64 in zip(("logits", "values"), got, o32, o64):
        ok, ed, e3 = _within(d, a32, a64, 1e-6 * max(1.0, float(np.max(np.abs(a64)))))
        print("%s %s dev %.3e f32 %.3e" % (what, name, ed, e3))
        assert ok, (what, name, ed, e3)


@NETS
def test_predict(ctx):
    f = ctx.start()
    rng = np.random.default_rng(6)
    m0 = rng.normal(0, 1e-3, ctx.w.size).astype(np.float32)
    v0 = rng.uniform(0, 1e-6, ctx.w.size).astype(np.float32)
    f.set_optimizer(m0, v0, 7)
    L_ = _lib.load()
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    with Fitter(max_batch=64, net=ctx.kind) as ex:
        ex.set_data(*ctx.data)
        ex.set_weights(ctx.w)
        for B in (1, 37, 64):
            r = rows(B, 40 + B)
            for train in (False, True):
                got = f.predict(r, train)
                assert got[0].shape == (B, 96) and got[1].shape == (B,)
                again, other = f.predict(r, train), ex.predict(r, train)
                assert same(got[0], again[0]) and same(got[1], again[1]), (B, train)
                assert same(got[0], other[0]) and same(got[1], other[1]), (B, train)  # packed equals expanded
                outputs_within(got, ctx.ref, ctx.w, ctx.data[0][r], train, "%s B=%d train=%d" % (ctx.net, B, train))
    # nothing of the fitter moved: the weights (the moving statistics among them), m, v and the step count
    m, v, it = f.get_optimizer()
    assert same(f.get_weights(), ctx.w) and same(m, m0) and same(v, v0) and it == 7
    # errors: more rows than max_batch, a row out of range, null pointers
    lo, va = np.zeros((65, 96), np.float32), np.zeros(65, np.float32)
    for r in (np.arange(65, dtype=np.int32), np.array([384], np.int32), np.array([-1], np.int32), np.zeros(0, np.int32)):
        assert L_.ca_fitter_predict(f._h, r.ctypes.data_as(i32p), r.size, 0, lo.ctypes.data_as(f32p), va.ctypes.data_as(f32p)) == ERR_ARG
    r = np.arange(4, dtype=np.int32)
    assert L_.ca_fitter_predict(f._h, None, 4, 0, lo.ctypes.data_as(f32p), va.ctypes.data_as(f32p)) == ERR_ARG
    assert L_.ca_fitter_predict(f._h, r.ctypes.data_as(i32p), 4, 0, None, va.ctypes.data_as(f32p)) == ERR_ARG
    assert L_.ca_fitter_predict(None, r.ctypes.data_as(i32p), 4, 0, lo.ctypes.data_as(f32p), va.ctypes.data_as(f32p)) == ERR_ARG
    assert not lo.any() and not va.any()


# ---------------------------------------------------------------------------------------------------- 5. metrics
def check_metrics(got, logits, values, z, t, top_k, w, n, what):
    """the device's metrics of a call against the restatement on the device's own logits: the accuracies exactly (counts
    below 2^24 over n) when unweighted, everything else by the _within rule with the floor 1e-6 max(1, |value|)"""
    m64 = L.metrics(logits, values, z, t, top_k, w)
    m32 = L.metrics(logits, values, z, t, top_k, w, np.float32)
    assert got["rows"] == n and got["top_k"] == top_k
    assert got["weight_sum"] == m64["weight_sum"], what
    for k in METRIC_NAMES:
        print("%s %-28s dev %.9g f64 %.9g f32 %.9g" % (what, k, got[k], m64[k], m32[k]))
        if w is None and k not in FLOATS:
            count = int(L.metric_rows(logits, values, z, t, top_k)[k].sum())
            assert got[k] == count / n, (what, k)
            continue
        ok, ed, e3 = _within(got[k], m32[k], m64[k], 1e-6 * max(1.0, abs(m64[k])))
        assert ok, (what, k, ed, e3)


@NETS
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_metrics_on_the_devices_own_logits(ctx, weighted):
    sw = sample_weights() if weighted else None
    assert sw is None or (sw == 0).any()
    s, z, t = ctx.data
    f = ctx.start(metrics=True, top_k=5, weights=sw)
    # evaluate: 300 rows in batches of 64, the last of 44; inference mode
    losses = f.evaluate(0, 300, 64)
    got = f.metrics()
    parts = [f.predict(np.arange(b, min(b + 64, 300), dtype=np.int32), False) for b in range(0, 300, 64)]
    assert parts[-1][0].shape[0] == 44
    lo, va = np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts])
    r = np.arange(300)
    check_metrics(got, lo, va, z[r], t[r], 5, None if sw is None else sw[r // 8], 300, "%s evaluate" % ctx.net)
    assert got["policy_entropy"] > 0 and got["target_entropy"] > 0 and got["mean_absolute_error"] > 0
    # train at learning rate 0: 165 rows as 64 + 64 + 37, each batch's own training-mode forward
    r = rows(165, 50)
    f.train(r, 64, 0.0)
    got = f.metrics()
    parts = [f.predict(r[b:b + 64], True) for b in range(0, 165, 64)]
    assert parts[-1][0].shape[0] == 37
    lo, va = np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts])
    check_metrics(got, lo, va, z[r], t[r], 5, None if sw is None else sw[r // 8], 165, "%s train" % ctx.net)
    # the losses are those of a fitter whose metrics are off
    assert ctx.start(weights=sw).evaluate(0, 300, 64) == losses


# ---------------------------------------------------------------------------------------------------- 6. ties
def head_bias_only(net, bias):
    """weights all zero but the policy head's bias: every row's logits are that bias"""
    w = np.zeros(KINDS[net][1](0).size, np.float32)
    if net == "mlp12x100":
        bp = fit_ref.layer_offsets()[1][3]
        w[bp:bp + 96] = bias
    else:
        w[fit_ref_rescnn4._slice(fit_ref_rescnn4.offsets(), "p_db")] = bias
    return w


@NETS
def test_ties_on_the_device(net):
    """the logits tie for the maximum (moves 1 and 2) and across rank 5 (moves 3 to 7 share the third-largest value);
    the targets include tied maxima, in the first 64 columns, in the last 32 and across the two"""
    bias = (-0.01 * np.arange(96)).astype(np.float32)
    bias[[1, 2]] = 3.0
    bias[3:8] = 2.0
    bias[0] = 1.0
    bias[[70, 90]] = 1.5
    hot = [0, 1, 2, 3, 5, 7, 8, 63, 64, 70, 90, 95]
    t = np.zeros((20, 96), np.float32)
    for i, c in enumerate(hot):
        t[i, c] = 1.0
    for i, pair in enumerate([(2, 4), (1, 2), (4, 7), (70, 90), (30, 70), (90, 95), (3, 64), (0, 1)]):
        t[len(hot) + i, list(pair)] = 0.5
    s, z, _ = fit_ref.synthetic_samples(20, 3)
    with Fitter(max_batch=8, net=KINDS[net][0]) as f:
        f.set_data(s, z, t)
        f.set_weights(head_bias_only(net, bias))
        lo, va = (np.concatenate(x) for x in zip(*[f.predict(np.arange(b, min(b + 8, 20), dtype=np.int32)) for b in (0, 8, 16)]))
        assert same(lo, np.tile(bias, (20, 1)))
        for k in (1, 5, 96):
            f.set_metrics(True, k)
            f.evaluate(0, 20, 8)  # batches of 8, 8 and 4: two workgroups, then one
            got = f.metrics()
            want = L.metric_rows(lo, va, z, t, k)
            for name in ("categorical_accuracy", "top_k_categorical_accuracy"):
                assert got[name] == int(want[name].sum()) / 20, (k, name)
        # by hand: the first maximum is move 1, so only the targets whose first maximum is 1 count
        assert int(want["categorical_accuracy"].sum()) == sum(1 for row in t if int(np.argmax(row)) == 1) == 2
        # in the top 5: nothing above 3.0, two above 2.0 -- the five-way tie at 2.0 is in, whichever of its moves
        top5 = L.metric_rows(lo, va, z, t, 5)["top_k_categorical_accuracy"]
        assert top5[:6].tolist() == [0.0, 1.0, 1.0, 1.0, 1.0, 1.0] and top5[9] == 0.0  # move 0 has 9 above, move 70 has 7


# ---------------------------------------------------------------------------------------------------- 7. a fit
@NETS
def test_fit_end_to_end(net):
    """fit_samples with every loss option and the metrics against the same fit on the float64 reference backend: the
    losses and the float metrics by the _within rule, the accuracies within 2 / rows, best_epoch equal; and twice the
    same bytes.  The learning rate is 1e-4: Adam's first steps are close to lr sign(g), so over the 15 steps of this fit
    the weights of any two arithmetics drift apart in proportion to it, and at 1e-3 the float32 restatement itself ends
    5 rows of 268 away from the float64 one in the top-k accuracy of the second epoch (the device 3); at 1e-4 the two
    restatements agree in every count, for both networks."""
    kind, init = KINDS[net]
    sp, oc = packed()
    w = init(6, bn_noise=True)
    kw = dict(batch_size=64, epochs=3, seed=3, loss=EVERYTHING, metrics=True, learning_rate=1e-4)
    a = fit_samples(w, sp, oc, net=kind, **kw)
    b = fit_samples(w, sp, oc, net=kind, **kw)
    assert same(a.weights, b.weights) and same(a.best_weights, b.best_weights) and a.history == b.history
    assert a.best_epoch == b.best_epoch and same(a.optimizer[0], b.optimizer[0]) and same(a.optimizer[1], b.optimizer[1])
    assert tuple(a.history) == HISTORY_KEYS + METRIC_HISTORY_KEYS and all(len(x) == 3 for x in a.history.values())
    data = expanded()
    ref = S.BASE[net]
    h64, h32 = (fit(w, *data, net=kind, _backend=S.RefBackend(net, dt), **kw) for dt in (ref.torch.float64, ref.torch.float32))
    assert a.best_epoch == h64.best_epoch and a.history["lr"] == h64.history["lr"]
    split_at = split_index(384, 0.3)
    for k in HISTORY_KEYS[:-1] + METRIC_HISTORY_KEYS:
        d, x32, x64 = (np.asarray(r.history[k]) for r in (a, h32, h64))
        print("%s %-40s dev %s f64 %s" % (net, k, d, x64))
        if "accuracy" in k:  # weights drift apart over the steps, so a row may change sides
            n = 384 - split_at if k.startswith("val_") else split_at
            assert np.all(np.abs(d - x64) <= 2.0 / n), k
            continue
        floor = 1e-6 * (abs(h64.history["val_loss" if k.startswith("val_") else "loss"][0]) if k in HISTORY_KEYS
                        else max(1.0, float(np.max(np.abs(x64)))))
        ok, ed, e3 = _within(d, x32, x64, floor)
        assert ok, (k, ed, e3)
    off = fit_samples(w, sp, oc, net=kind, batch_size=64, epochs=3, seed=3, learning_rate=1e-4)
    assert not same(off.weights, a.weights) and tuple(off.history) == HISTORY_KEYS


# ---------------------------------------------------------------------------------------------------- 8. ABI errors
def test_abi_errors_change_nothing():
    L_ = _lib.load()
    size = C.sizeof(_lib.CaFitLoss)
    with Fitter(max_batch=16) as f:
        good = LossOptions(value_weight=0.5, policy_weight=2.0, label_smoothing=0.25, value_loss="huber", huber_delta=0.75)
        f.set_loss(good)
        assert f.get_loss() == good
        ok = dict(struct_size=size, value_weight=1.0, policy_weight=1.0, label_smoothing=0.5, value_loss=0, huber_delta=1.0)
        bad = [dict(value_weight=-1.0), dict(value_weight=float("nan")), dict(value_weight=float("inf")),
               dict(policy_weight=-0.5), dict(policy_weight=float("inf")), dict(value_weight=0.0, policy_weight=0.0),
               dict(label_smoothing=1.0), dict(label_smoothing=-0.25), dict(label_smoothing=float("nan")),
               dict(value_loss=2), dict(value_loss=-1), dict(huber_delta=0.0), dict(huber_delta=-1.0),
               dict(huber_delta=float("inf")), dict(huber_delta=float("nan")), dict(struct_size=3)]
        for kw in bad:
            c = _lib.CaFitLoss(**dict(ok, **kw))
            assert L_.ca_fitter_set_loss(f._h, C.byref(c)) == ERR_ARG and L_.ca_last_error(), kw
            assert f.get_loss() == good
        assert L_.ca_fitter_set_loss(f._h, None) == ERR_ARG
        assert L_.ca_fitter_set_loss(None, C.byref(_lib.CaFitLoss(**ok))) == ERR_ARG
        assert L_.ca_fitter_get_loss(f._h, C.byref(_lib.CaFitLoss(struct_size=3))) == ERR_ARG
        # a shorter struct: what it does not have takes the defaults (not zeros), whatever the bytes behind it say
        c = _lib.CaFitLoss(struct_size=12, value_weight=3.0, policy_weight=0.0, label_smoothing=7.0, value_loss=9)
        assert L_.ca_fitter_set_loss(f._h, C.byref(c)) == 0
        assert f.get_loss() == LossOptions(value_weight=3.0, policy_weight=0.0)
        assert L_.ca_fitter_set_loss(f._h, C.byref(_lib.CaFitLoss(struct_size=4))) == 0
        assert f.get_loss() == LossOptions()
        c = _lib.CaFitLoss(struct_size=8, policy_weight=7.0)
        assert L_.ca_fitter_get_loss(f._h, C.byref(c)) == 0 and (c.struct_size, c.value_weight, c.policy_weight) == (8, 1.0, 7.0)
        # metrics: off on a new fitter, top_k in 1..96
        m = _lib.CaFitMetrics(struct_size=C.sizeof(_lib.CaFitMetrics))
        assert L_.ca_fitter_metrics(f._h, C.byref(m)) == ERR_STATE
        for k in (0, -1, 97):
            assert L_.ca_fitter_set_metrics(f._h, 1, k) == ERR_ARG
            assert L_.ca_fitter_metrics(f._h, C.byref(m)) == ERR_STATE
        assert L_.ca_fitter_set_metrics(None, 1, 5) == ERR_ARG
        f.set_metrics(True, 96)
        got = f.metrics()
        assert got["rows"] == 0 and got["top_k"] == 96 and got["weight_sum"] == 0.0
        assert L_.ca_fitter_metrics(f._h, None) == ERR_ARG
        f.set_metrics(False)
        assert L_.ca_fitter_metrics(f._h, C.byref(m)) == ERR_STATE
