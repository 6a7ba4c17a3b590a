"""The loss options and the metrics without a GPU (include/corintho_hip.h, "loss and metrics"): LossOptions, the
restatement of tests/fit_ref_loss.py by hand, how fit() and its relatives treat `loss` and `metrics` on that reference
backend, the draws of the GPU test's batches, and the run's settings and files."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import corintho_ai_amd
from corintho_ai_amd import LossOptions, RunParams, expand_samples, fit, fit_resident, fit_samples, fit_trainer, nets
from corintho_ai_amd import run as R
from corintho_ai_amd.fit import HISTORY_KEYS, METRIC_HISTORY_KEYS, METRIC_KEYS, METRIC_NAMES, MIN_DELTA
from tests import fit_ref
from tests import fit_ref_loss as L
from tests import fit_ref_step as S
from tests.emu import emulib
from tests.test_run_cpu import StubFitter, comparable, open_run, small

LOG96 = float(np.log(96.0))


def _tiny():
    return fit_ref.synthetic_samples(64, 5)


# ---------------------------------------------------------------------------------------------------- LossOptions
def test_loss_options_defaults_and_dict():
    d = LossOptions()
    assert (d.value_weight, d.policy_weight, d.label_smoothing, d.value_loss, d.huber_delta) == (1.0, 0.25, 0.0, "mse", 1.0)
    assert d.check() is d and d.is_default()
    assert d.as_dict() == dict(value_weight=1.0, policy_weight=0.25, label_smoothing=0.0, value_loss="mse", huber_delta=1.0)
    assert corintho_ai_amd.LossOptions is LossOptions
    for other in (LossOptions(value_weight=2.0), LossOptions(policy_weight=0.5), LossOptions(label_smoothing=0.1),
                  LossOptions(value_loss="huber"), LossOptions(policy_weight=0.0), LossOptions(value_weight=0.0)):
        assert other.check() is other and not other.is_default()
    assert LossOptions(huber_delta=0.5).is_default()  # not read with "mse"
    assert LossOptions(label_smoothing=1e-60).is_default()  # 0 in float32, as the device sees it
    assert LossOptions(policy_weight=1e-60).check().policy_weight == 1e-60  # 0 in float32, and value_weight is not
    assert LossOptions(1.0, 0.25, 0.0, "mse", 1.0) == d  # the order of ca_fit_loss


BAD = [LossOptions(value_weight=-1.0), LossOptions(policy_weight=-0.25), LossOptions(value_weight=float("nan")),
       LossOptions(policy_weight=float("inf")), LossOptions(value_weight=1e60),  # inf in float32
       LossOptions(value_weight=0.0, policy_weight=0.0), LossOptions(value_weight=0.0, policy_weight=1e-60),  # both 0 in float32
       LossOptions(label_smoothing=1.0), LossOptions(label_smoothing=-0.1), LossOptions(label_smoothing=1 - 1e-12),
       LossOptions(label_smoothing=float("nan")), LossOptions(huber_delta=0.0), LossOptions(value_loss="huber", huber_delta=0.0),
       LossOptions(huber_delta=-1.0), LossOptions(huber_delta=1e-60), LossOptions(huber_delta=float("inf")),
       LossOptions(value_loss="mae"), LossOptions(value_loss=1), LossOptions(value_weight="1"), LossOptions(value_weight=True),
       {"value_wieght": 2.0}, "huber"]
BAD_METRICS = [{"top_k": 0}, {"top_k": 97}, {"top_k": 2.5}, {"top_k": True}, {"k": 3}, "yes", 5]


def _refused_by_all_four(monkeypatch, **kw):
    F = sys.modules["corintho_ai_amd.fit"]  # (the package's attribute `fit` is the function)

    def no_fitter(*a, **k):
        raise AssertionError("a fitter was made")

    monkeypatch.setattr(F, "Fitter", no_fitter)
    s, z, p = _tiny()
    w = nets.init_mlp12x100(1)
    sp = np.concatenate([s, p], axis=1)
    with pytest.raises(ValueError):
        fit(w, s, z, p, **kw)
    with pytest.raises(ValueError):
        fit_samples(w, sp, z, **kw)
    with pytest.raises(ValueError):
        fit_trainer(w, [object()], **kw)
    with pytest.raises(ValueError):
        fit_resident(object(), w, **kw)


@pytest.mark.parametrize("bad", BAD, ids=[str(i) for i in range(len(BAD))])
def test_loss_errors_before_any_fitter(bad, monkeypatch):
    if isinstance(bad, LossOptions):
        with pytest.raises(ValueError):
            bad.check()
    _refused_by_all_four(monkeypatch, loss=bad)


@pytest.mark.parametrize("bad", BAD_METRICS, ids=[str(i) for i in range(len(BAD_METRICS))])
def test_metrics_errors_before_any_fitter(bad, monkeypatch):
    _refused_by_all_four(monkeypatch, metrics=bad)


# ---------------------------------------------------------------------------------------------------- the restatement
def _row(h, v, z, t):
    f = torch.float64
    return (torch.tensor([h], dtype=f), torch.tensor([v], dtype=f, requires_grad=True), torch.tensor([z], dtype=f),
            torch.tensor([t], dtype=f))


def test_loss_restatement_by_hand():
    """one row: logits 0 but for log 2 at move 0 (so the softmax is 2/97 and 1/97), the target on moves 0 and 1, v = 0"""
    h = [float(np.log(2.0))] + [0.0] * 95
    t = [0.5, 0.5] + [0.0] * 94
    log97, log2 = float(np.log(97.0)), float(np.log(2.0))
    # no smoothing: -(0.5 (log 2 - log 97) + 0.5 (-log 97))
    val, pol = (x.detach() for x in L.row_terms(*_row(h, 0.0, -0.25, t), LossOptions()))
    assert abs(float(pol) - (log97 - 0.5 * log2)) < 1e-14 and float(val) == 0.0625
    # smoothing 0.5: t'_0 = 0.25 + 1/192, and the t' sum to 1
    _, pol = (x.detach() for x in L.row_terms(*_row(h, 0.0, -0.25, t), LossOptions(label_smoothing=0.5)))
    assert abs(float(pol) - (log97 - (0.25 + 1.0 / 192.0) * log2)) < 1e-14
    # Huber(0.5) on both sides of delta and at it, and its gradient in v (tanh' = 1 at v = 0): clamp(e, -delta, delta)
    hub = LossOptions(value_loss="huber", huber_delta=0.5)
    for z, want, grad in ((-0.25, 0.03125, 0.25), (-0.5, 0.125, 0.5), (-1.0, 0.375, 0.5), (1.0, 0.375, -0.5), (0.25, 0.03125, -0.25)):
        args = _row(h, 0.0, z, t)
        val, _ = L.row_terms(*args, hub)
        assert float(val.detach()) == want, z
        val.sum().backward()
        assert float(args[1].grad) == grad, z
    # MSE's gradient is 2 e
    args = _row(h, 0.0, -1.0, t)
    L.row_terms(*args, LossOptions())[0].sum().backward()
    assert float(args[1].grad) == 2.0
    # the batch loss: the loss weights on the means, the sample weights inside them, the divisor B
    two = [torch.cat([a.detach(), b.detach()]) for a, b in zip(_row(h, 0.0, -1.0, t), _row(h, 0.0, -0.25, t))]
    tot, lv, lp = L.batch_losses(*two, LossOptions(value_weight=2.0, policy_weight=0.5, value_loss="huber", huber_delta=0.5),
                                 torch.tensor([2.0, 0.0], dtype=torch.float64))
    assert float(lv) == 0.375 and abs(float(lp) - (log97 - 0.5 * log2)) < 1e-14
    assert float(tot) == 2.0 * float(lv) + 0.5 * float(lp)
    tot, lv, lp = L.batch_losses(*two, LossOptions())
    assert float(lv) == (1.0 + 0.0625) / 2 and float(tot) == float(lv) + 0.25 * float(lp)


def test_metrics_restatement_by_hand():
    z96 = [0.0] * 91
    h = np.array([[1.0, 3.0, 3.0, 2.0, 2.0] + z96,   # the maximum is tied at 1 and 2: the first, 1
                  [1.0, 3.0, 3.0, 2.0, 2.0] + z96,
                  [0.0] * 96])
    t = np.array([[0.0, 0.0, 0.5, 0.0, 0.5] + z96,   # tied at 2 and 4: c = 2, h_c = 3, nothing above it
                  [0.0, 0.0, 0.0, 0.5, 0.5] + z96,   # c = 3, h_c = 2: two logits above, the tie at 4 is not
                  [1.0] + [0.0] * 95])                # one-hot: 0 log 0 = 0
    v, z = np.array([0.0, 0.0, 0.0]), np.array([-0.25, 1.0, 0.0])
    r = {k: L.metric_rows(h, v, z, t, k) for k in (1, 2, 3, 96)}
    assert r[1]["categorical_accuracy"].tolist() == [0.0, 0.0, 1.0]  # row 0: argmax h = 1, c = 2
    assert r[1]["top_k_categorical_accuracy"].tolist() == [1.0, 0.0, 1.0]  # row 0: a tie with the maximum is in the top 1
    assert r[2]["top_k_categorical_accuracy"].tolist() == [1.0, 0.0, 1.0]  # row 1: 2 above, not < 2
    assert r[3]["top_k_categorical_accuracy"].tolist() == [1.0, 1.0, 1.0]  # ... and < 3, whatever the tie at 4
    assert r[96]["top_k_categorical_accuracy"].tolist() == [1.0, 1.0, 1.0]
    assert r[1]["mean_absolute_error"].tolist() == [0.25, 1.0, 0.0]
    assert np.allclose(r[1]["target_entropy"], [np.log(2.0), np.log(2.0), 0.0], rtol=0, atol=1e-15)
    assert r[1]["target_entropy"][2] == 0.0
    assert abs(r[1]["policy_entropy"][2] - LOG96) < 1e-14  # uniform
    # row 2's all-equal logits: every move ties with the maximum; the first is taken, and it is the target's
    assert r[1]["categorical_accuracy"][2] == 1.0
    # the weighted mean: a weight of 0 takes its row out, weights that sum to 0 give 0
    m = L.metrics(h, v, z, t, 1, w=np.array([0.0, 2.0, 2.0]))
    assert m["categorical_accuracy"] == 0.5 and m["mean_absolute_error"] == 0.5 and m["weight_sum"] == 4.0 and m["rows"] == 3
    assert m["top_k"] == 1 and abs(m["target_entropy"] - 0.5 * np.log(2.0)) < 1e-15
    assert L.metrics(h, v, z, t, 1, w=np.zeros(3))["mean_absolute_error"] == 0.0
    m = L.metrics(h, v, z, t, 1)
    assert m["weight_sum"] == 3.0 and m["top_k_categorical_accuracy"] == 2.0 / 3.0
    m32 = L.metrics(h, v, z, t, 1, f=np.float32)
    assert m32["categorical_accuracy"] == float(np.float32(1.0) / np.float32(3.0))
    assert set(METRIC_NAMES) <= set(m)


# ---------------------------------------------------------------------------------------------------- fit() on the backend
def _plateau(vals, lr, anneal, patience):
    """ReduceLROnPlateau and ModelCheckpoint on a list of val_loss -> (the lr of every epoch, the best epoch)"""
    lrs, best, wait, lr = [], np.inf, 0, np.float32(lr)
    for x in vals:
        lrs.append(float(lr))
        if x < best - MIN_DELTA:
            best, wait = x, 0
        else:
            wait += 1
            if wait >= patience:
                lr, wait = np.float32(lr * np.float32(anneal)), 0
    return lrs, int(np.argmin(vals))


def test_defaults_give_todays_history():
    s, z, p = _tiny()
    w = nets.init_mlp12x100(1, bn_noise=True)
    plain = fit(w, s, z, p, batch_size=16, epochs=2, seed=1, _backend=S.RefBackend("mlp12x100"))
    be = S.RefBackend("mlp12x100")
    for loss in (None, LossOptions(), LossOptions().as_dict()):
        res = fit(w, s, z, p, batch_size=16, epochs=2, seed=1, loss=loss, metrics=False, _backend=be)
        assert tuple(res.history) == HISTORY_KEYS and res.history == plain.history
        assert res.weights.tobytes() == plain.weights.tobytes() and res.best_epoch == plain.best_epoch
    assert be.set_loss_calls == [LossOptions()] * 3 and be.set_metrics_calls == [(False, 5)] * 3
    # metrics on changes neither the losses nor the weights
    res = fit(w, s, z, p, batch_size=16, epochs=2, seed=1, metrics=True, _backend=be)
    assert tuple(res.history) == HISTORY_KEYS + METRIC_HISTORY_KEYS
    assert {k: res.history[k] for k in HISTORY_KEYS} == plain.history and res.weights.tobytes() == plain.weights.tobytes()


def test_fit_with_loss_and_metrics():
    s, z, p = _tiny()
    w = nets.init_mlp12x100(1, bn_noise=True)
    loss = LossOptions(value_weight=2.0, policy_weight=0.5, label_smoothing=0.1, value_loss="huber", huber_delta=0.5)
    be = S.RefBackend("mlp12x100")
    res = fit(w, s, z, p, batch_size=16, epochs=5, seed=1, patience=1, anneal_factor=0.5, loss=loss, metrics={"top_k": 3},
              _backend=be)
    h = res.history
    assert tuple(h) == HISTORY_KEYS + METRIC_HISTORY_KEYS and all(len(x) == 5 for x in h.values())
    assert be.set_loss_calls == [loss] and be.set_metrics_calls == [(True, 3)]
    for e in range(5):  # the totals are the weighted sums of the two means, in training and in validation
        assert abs(h["loss"][e] - (2.0 * h["value_loss"][e] + 0.5 * h["policy_loss"][e])) < 1e-12
        assert abs(h["val_loss"][e] - (2.0 * h["val_value_loss"][e] + 0.5 * h["val_policy_loss"][e])) < 1e-12
    # the checkpoint and the plateau rule follow that val_loss
    lrs, best = _plateau(h["val_loss"], 0.001, 0.5, 1)
    assert h["lr"] == lrs and res.best_epoch == best
    # the val_ metrics are the restatement's on the validation rows with the weights the epoch ended with
    assert all(0.0 <= x <= 1.0 for k in METRIC_HISTORY_KEYS if "accuracy" in k for x in h[k])
    assert all(a <= b for a, b in zip(h["val_policy_categorical_accuracy"], h["val_policy_top_k_categorical_accuracy"]))
    assert len(set(h["val_target_entropy"])) == 1 and h["val_target_entropy"][0] > 0  # the targets do not move
    lo, v = S.predict(fit_ref, be.w, s[44:], False)
    want = L.metrics(lo, v, z[44:], p[44:], 3)
    for k, name in zip(METRIC_KEYS, METRIC_NAMES):
        assert abs(h["val_" + k][-1] - want[name]) < 1e-12, k
    assert be.metrics()["rows"] == 20 and be.metrics()["top_k"] == 3
    # the same fit under the default loss is another fit, and the next call with the defaults sets the backend back
    off = fit(w, s, z, p, batch_size=16, epochs=5, seed=1, patience=1, _backend=be)
    assert be.set_loss_calls[-1] == LossOptions() and be.set_metrics_calls[-1] == (False, 5)
    assert tuple(off.history) == HISTORY_KEYS and off.weights.tobytes() != res.weights.tobytes()
    # the loss weights scale the gradient: (2, 0.5) from (1, 0.25) is twice the loss
    dbl = fit(w, s, z, p, batch_size=16, epochs=1, seed=1, loss=LossOptions(value_weight=2.0, policy_weight=0.5), _backend=be)
    one = fit(w, s, z, p, batch_size=16, epochs=1, seed=1, _backend=be)
    assert abs(dbl.history["loss"][0] - 2.0 * one.history["loss"][0]) < 1e-3 * one.history["loss"][0]
    assert dbl.history["loss"][0] != one.history["loss"][0]


def test_backend_without_loss_or_metrics():
    s, z, p = _tiny()
    w = nets.init_mlp12x100(1)
    be = S.BaseOnly(S.RefBackend("mlp12x100"))
    fit(w, s, z, p, batch_size=32, epochs=1, loss=LossOptions(), metrics=False, _backend=be)
    with pytest.raises(ValueError, match="set_loss"):
        fit(w, s, z, p, batch_size=32, epochs=1, loss=LossOptions(value_weight=2.0), _backend=be)
    with pytest.raises(ValueError, match="set_metrics"):
        fit(w, s, z, p, batch_size=32, epochs=1, metrics=True, _backend=be)


def test_sample_weights_enter_the_metrics():
    s, z, p = _tiny()
    w = nets.init_mlp12x100(1, bn_noise=True)
    sw = np.where(np.arange(64) % 3 == 0, 0.0, 1.5).astype(np.float32)
    be = S.RefBackend("mlp12x100")
    res = fit(w, s, z, p, batch_size=16, epochs=1, seed=1, sample_weight=sw, metrics=True, _backend=be)
    lo, v = S.predict(fit_ref, be.w, s[44:], False)
    want = L.metrics(lo, v, z[44:], p[44:], 5, w=sw[44:])
    assert be.metrics()["weight_sum"] == float(sw[44:].sum()) == want["weight_sum"]
    assert abs(res.history["val_value_mean_absolute_error"][0] - want["mean_absolute_error"]) < 1e-12


# ---------------------------------------------------------------------------------------------------- the GPU test's draws
@pytest.mark.parametrize("net", ["mlp12x100", "rescnn4"])
def test_the_synthetic_set_yields_batches_off_hubers_kink(net):
    """tests/test_fit_loss_gpu.py draws its batches with fit_ref_loss.draw_batch from these generators: every one is
    found off Huber's kink within the three redraws (the ReLU kink has its exception there)"""
    from tests import test_fit_loss_gpu as G

    ref = S.BASE[net]
    data = G.expanded(_cdll=emulib.load())
    w = G.KINDS[net][1](5, bn_noise=True)
    relu = []
    for name, loss, weighted in G.GENERAL:
        rng = G.general_rng(name)
        for B in G.BATCHES:
            rows, relu_ok, huber_ok = S.draw_batch(ref, w, data[0], data[1], rng, B, loss, G.general_candidates(weighted, B))
            assert huber_ok, (name, B)
            assert not weighted or (G.sample_weights()[rows // 8] == 0).any() == (B > 1)
            assert rows.size == B and len(set(rows.tolist())) == B
            relu.append(relu_ok)
    assert len(relu) - sum(relu) <= len(relu) // 4


# ---------------------------------------------------------------------------------------------------- the run
def test_run_params_toml_and_cli(tmp_path):
    d = RunParams(seed=1)
    assert d.loss_options() == LossOptions() and d.loss_options().is_default()
    assert (d.value_weight, d.policy_weight, d.label_smoothing, d.value_loss, d.huber_delta, d.metrics, d.top_k) == \
        (1.0, 0.25, 0.0, "mse", 1.0, False, 5)
    path = tmp_path / "a.toml"
    path.write_text("[hyperparameters]\nname = \"x\"\nvalue_weight = 0.7\npolicy_weight = 1.3\nlabel_smoothing = 0.1\n"
                    "value_loss = \"huber\"\nhuber_delta = 0.5\nmetrics = true\ntop_k = 3\n")
    p, _ = R.parse_args(["--config", str(path), "--seed", "1"])
    assert p.loss_options() == LossOptions(0.7, 1.3, 0.1, "huber", 0.5) and p.metrics is True and p.top_k == 3
    assert isinstance(p.top_k, int)
    p, _ = R.parse_args(["--config", str(path), "--seed", "1", "--value_weight", "2", "--top_k=7"])  # a flag beats the file
    assert (p.value_weight, p.policy_weight, p.top_k) == (2.0, 1.3, 7)
    p, _ = R.parse_args(["--seed", "1", "--metrics", "--value_loss", "huber", "--huber_delta", "0.25", "--label_smoothing", "0.05"])
    assert p.loss_options() == LossOptions(value_loss="huber", huber_delta=0.25, label_smoothing=0.05) and p.metrics
    q = R.parse_args(["--seed", "1"])[0]
    assert q.loss_options().is_default() and q.metrics is False
    for bad in (dict(value_weight=-1.0), dict(value_weight=0.0, policy_weight=0.0), dict(label_smoothing=1.0),
                dict(value_loss="mae"), dict(huber_delta=0.0), dict(top_k=0), dict(top_k=97)):
        with pytest.raises(ValueError):
            RunParams(seed=1, **bad)
    d = RunParams(seed=1, policy_weight=0.5, metrics=True).as_dict()
    assert d["policy_weight"] == 0.5 and d["metrics"] is True and d["value_loss"] == "mse"


class LossFitter(StubFitter):
    """test_run_cpu's float32 fitter with the loss options and the metrics of tests/fit_ref_loss.py's backend"""

    def __init__(self):
        super().__init__()
        self.inner = S.RefBackend("mlp12x100", torch.float32)
        self.inner.data = None

    def set_loss(self, loss=None):
        self.inner.set_loss(loss)

    def set_metrics(self, on=True, top_k=5):
        self.inner.set_metrics(on, top_k)

    def metrics(self):
        return self.inner.metrics()

    def _sync(self, to_inner):
        a, b = (self, self.inner) if to_inner else (self.inner, self)
        b.w, b.m, b.v, b.it, b.data = a.w, a.m, a.v, a.it, a.data

    def train(self, *a, **kw):
        if self.data is None:  # (as StubFitter.train)
            self.data = expand_samples(self.sp, self.oc, _cdll=emulib.load())
            self.datasets.append((self.sp.copy(), self.oc.copy()))
        self._sync(True)
        out = self.inner.train(*a, **kw)
        self._sync(False)
        return out

    def evaluate(self, *a):
        self._sync(True)
        return self.inner.evaluate(*a)


def _csv(run, gen=1):
    with open(os.path.join(run.root, "generations", "gen_%d" % gen, "training_logs", "train_loss.csv")) as f:
        return [line.rstrip("\n").split("\t") for line in f]


def test_generation_passes_loss_and_metrics(tmp_path):
    loss = LossOptions(value_weight=0.5, policy_weight=1.0, label_smoothing=0.1, value_loss="huber", huber_delta=0.5)
    fitter = LossFitter()
    run = open_run(small(tmp_path, name="a", value_weight=0.5, policy_weight=1.0, label_smoothing=0.1, value_loss="huber",
                         huber_delta=0.5, metrics=True, top_k=3), fitter)
    res = run.generation()
    assert fitter.inner.set_loss_calls == [loss] and fitter.inner.set_metrics_calls == [(True, 3)]
    rows = _csv(run)
    assert tuple(rows[0]) == ("epoch",) + R.LOSS_COLUMNS + METRIC_HISTORY_KEYS and len(rows) == 3
    for e, row in enumerate(rows[1:]):
        got = dict(zip(rows[0], row))
        assert int(got["epoch"]) == e
        for k in R.LOSS_COLUMNS + METRIC_HISTORY_KEYS:
            assert float(got[k]) == res.fit.history[k][e], k
    # losses.txt holds the smallest val_loss, not the last column
    with open(os.path.join(run.root, "metadata", "losses.txt")) as f:
        assert float(f.read().split()[0]) == min(res.fit.history["val_loss"])
    log = os.path.join(run.root, "generations", "gen_1", "training_logs")
    with open(os.path.join(log, "fit_options.json")) as f:
        d = json.load(f)
    assert d["loss"] == loss.as_dict() and "adam" not in d and "epochs" not in d and not any(d["options"].values())
    with open(os.path.join(run.root, "generations", "gen_1", "metadata.txt")) as f:
        meta = json.load(f)
    assert meta["value_loss"] == "huber" and meta["metrics"] is True and meta["top_k"] == 3 and meta["policy_weight"] == 1.0


def test_default_run_files_are_unchanged(tmp_path):
    """everything at its default: behind a fitter that has the new calls and behind one that knows nothing of them the
    run's files are the same bytes, the csv has the columns it had and there is no fit_options.json"""
    fitter = LossFitter()
    new = open_run(small(tmp_path, name="new"), fitter)
    new.generation()
    old = open_run(small(tmp_path, name="old"), StubFitter())
    old.generation()
    assert fitter.inner.set_loss_calls == [LossOptions()] and fitter.inner.set_metrics_calls == [(False, 5)]
    a, b = comparable(new.root), comparable(old.root)
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], dict):  # metadata.txt: the settings, but for the run's name
            assert {x: y for x, y in a[k].items() if x != "name"} == {x: y for x, y in b[k].items() if x != "name"}, k
        else:
            assert a[k] == b[k], k
    assert tuple(_csv(new)[0]) == ("epoch",) + R.LOSS_COLUMNS
    assert not os.path.exists(os.path.join(new.root, "generations", "gen_1", "training_logs", "fit_options.json"))
    # write_loss still takes the last column of a csv that has no header name for it
    csv, out = tmp_path / "x.csv", tmp_path / "losses.txt"
    csv.write_text("epoch\ta\tb\n0\t1.0\t0.5\n1\t2.0\t0.25\n")
    R.write_loss(str(csv), str(out))
    assert out.read_text() == "0.25\n"
