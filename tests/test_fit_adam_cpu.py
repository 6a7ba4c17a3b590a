"""Adam's arguments without a GPU (include/corintho_hip.h, "Adam's arguments"): AdamOptions, how fit() and its relatives
treat `adam` on the reference backend of tests/fit_ref_adam.py (epochs judged by the averaged weights, the checkpoint
holds them, the result is finalised), and the run's settings and files."""
import dataclasses
import json
import os
import sys

import numpy as np
import pytest

from corintho_ai_amd import AdamOptions, RunParams, fit, fit_resident, fit_samples, fit_trainer, nets
from corintho_ai_amd import run as R
from corintho_ai_amd.fit import HISTORY_KEYS, FitResult
from tests import fit_ref
from tests import fit_ref_adam as A
from tests import fit_ref_options as O
from tests import fit_ref_step as S
from tests.test_run_cpu import StubFitter, open_run, small


def _tiny():
    return fit_ref.synthetic_samples(64, 5)


# ---------------------------------------------------------------------------------------------------- AdamOptions
def test_adam_options_defaults_and_dict():
    d = AdamOptions()
    assert (d.beta_1, d.beta_2, d.epsilon, d.amsgrad, d.ema_momentum, d.ema_overwrite_frequency) == (0.9, 0.999, 1e-7, False, 0.0, 0)
    assert d.check() is d and d.is_default() and not d.averaged()
    assert d.as_dict() == dict(beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False, ema_momentum=0.0,
                               ema_overwrite_frequency=0)
    for other in (AdamOptions(beta_1=0.0), AdamOptions(beta_2=0.99), AdamOptions(epsilon=1e-8), AdamOptions(amsgrad=True),
                  AdamOptions(ema_momentum=0.5)):
        assert other.check() is other and not other.is_default()
    assert AdamOptions(ema_momentum=1e-60).is_default()  # 0 in float32: off, as the device sees it
    assert AdamOptions(ema_momentum=0.99, ema_overwrite_frequency=3).check().averaged()


BAD = [AdamOptions(beta_1=1.0), AdamOptions(beta_1=-0.1), AdamOptions(beta_2=1.0), AdamOptions(beta_2=float("nan")),
       AdamOptions(beta_1=1 - 1e-12),  # 1 in float32
       AdamOptions(epsilon=0.0), AdamOptions(epsilon=-1e-7), AdamOptions(epsilon=float("inf")), AdamOptions(epsilon=1e-60),
       AdamOptions(ema_momentum=1.0), AdamOptions(ema_momentum=-0.5), AdamOptions(ema_overwrite_frequency=-1),
       AdamOptions(ema_overwrite_frequency=2), AdamOptions(ema_momentum=0.5, ema_overwrite_frequency=1.5),
       AdamOptions(amsgrad=2), AdamOptions(beta_1="0.9"), {"beta_3": 0.5}, "amsgrad"]


@pytest.mark.parametrize("bad", BAD, ids=[str(i) for i in range(len(BAD))])
def test_argument_errors_before_any_fitter(bad, monkeypatch):
    if isinstance(bad, AdamOptions):
        with pytest.raises(ValueError):
            bad.check()
    F = sys.modules["corintho_ai_amd.fit"]  # (the package's attribute `fit` is the function)

    def no_fitter(*a, **kw):
        raise AssertionError("a fitter was made")

    monkeypatch.setattr(F, "Fitter", no_fitter)
    s, z, p = _tiny()
    w = nets.init_mlp12x100(1)
    sp = np.concatenate([s, p], axis=1)
    with pytest.raises(ValueError):
        fit(w, s, z, p, adam=bad)
    with pytest.raises(ValueError):
        fit_samples(w, sp, z, adam=bad)
    with pytest.raises(ValueError):
        fit_trainer(w, [object()], adam=bad)
    with pytest.raises(ValueError):
        fit_resident(object(), w, adam=bad)


# ---------------------------------------------------------------------------------------------------- the restatement
def test_restatement_by_hand():
    """one weight, numbers that float64 holds exactly enough to check by hand"""
    ad = AdamOptions(beta_1=0.5, beta_2=0.75, epsilon=0.5, amsgrad=True, ema_momentum=0.75, ema_overwrite_frequency=2)
    one = lambda x: np.array([x])  # noqa: E731
    u = A.adam_update(one(1.0), one(2.0), one(4.0), one(16.0), one(3.0), one(4.0), 1, 0.25, ad, np.float64)
    assert u["m"][0] == 2.0 + (4.0 - 2.0) * 0.5 and u["v"][0] == 4.0 + (16.0 - 4.0) * 0.25
    assert u["h"][0] == 16.0 and u["d"][0] == 16.0  # max(16, 7)
    lr_t = float(A.lr_t(0.25, 1, ad))
    assert abs(lr_t - 0.25 * np.sqrt(1 - 0.75 ** 2) / (1 - 0.5 ** 2)) < 1e-7
    assert u["w2"][0] == 1.0 - lr_t * 3.0 / 4.5
    assert u["a"][0] == 3.0 + (u["w2"][0] - 3.0) * 0.25
    assert u["w3"][0] == u["a"][0]  # the step brings the count to 2: overwritten
    assert A.adam_update(one(1.0), one(2.0), one(4.0), one(16.0), one(3.0), one(4.0), 2, 0.25, ad, np.float64)["w3"][0] != u["a"][0]
    # amsgrad from zero: max(0, v') = v'
    z = A.adam_update(one(1.0), one(0.0), one(0.0), one(0.0), None, one(4.0), 0, 0.25, AdamOptions(amsgrad=True), np.float64)
    assert z["h"][0] == z["v"][0] and z["a"] is None
    # the defaults are the base module's step
    w, m, v = (np.array([x, 0.0]) for x in (0.3, 0.01, 0.002))
    g = np.array([0.5, 0.0])
    mask = np.array([True, False])
    u = A.adam_update(w[mask], m[mask], v[mask], None, None, g[mask], 4, 1e-3, AdamOptions(), np.float64)
    f = np.float64
    lt = f(1e-3) * np.sqrt(f(1) - f(S.B2) ** f(5)) / (f(1) - f(S.B1) ** f(5))
    m1 = 0.01 + (0.5 - 0.01) * (1 - S.B1)
    v1 = 0.002 + (0.25 - 0.002) * (1 - S.B2)
    # the restatement holds the constants as the device does, in float32: 1 - float32(0.999) is off by 2^-25 / 0.001 =
    # 3e-5 of itself, which is the largest of the differences; 1e-4 of the step covers them
    step = lt * m1 / (np.sqrt(v1) + S.ADAM_EPS)
    assert abs(u["w3"][0] - (0.3 - step)) < 1e-4 * step


# ---------------------------------------------------------------------------------------------------- fit() and adam
def test_defaults_give_todays_result():
    s, z, p = _tiny()
    w = nets.init_mlp12x100(1, bn_noise=True)
    plain = fit(w, s, z, p, batch_size=16, epochs=2, seed=1, _backend=S.RefBackend("mlp12x100"))
    be = S.RefBackend("mlp12x100")
    for adam in (None, AdamOptions(), AdamOptions().as_dict()):
        res = fit(w, s, z, p, batch_size=16, epochs=2, seed=1, adam=adam, _backend=be)
        assert tuple(res.history) == HISTORY_KEYS and res.history == plain.history
        assert res.weights.tobytes() == plain.weights.tobytes() and res.best_weights.tobytes() == plain.best_weights.tobytes()
        assert res.best_epoch == plain.best_epoch and res.learning_rate == plain.learning_rate
        assert res.best_slots is None and res.slots is None
    assert be.set_adam_calls == [AdamOptions()] * 3 and be.swaps == 0 and be.applied == 0
    # the new fields stand last and have defaults: a FitResult made the old way is what it was
    names = [f.name for f in dataclasses.fields(FitResult)]
    assert names[-2:] == ["best_slots", "slots"] and names[:7] == ["best_weights", "best_optimizer", "best_epoch", "weights",
                                                                   "optimizer", "learning_rate", "history"]
    old = FitResult(w, (w, w, 0), 0, w, (w, w, 0), 0.5)
    assert old.best_slots is None and old.slots is None and old.history == {}


def test_backend_without_adam():
    s, z, p = _tiny()
    w = nets.init_mlp12x100(1)
    for be in (S.BaseOnly(S.RefBackend("mlp12x100")),
               S.BaseOnly(S.RefBackend("mlp12x100"), "set_options", "get_options", "train_stats")):
        assert not hasattr(be, "set_adam")
        fit(w, s, z, p, batch_size=32, epochs=1, _backend=be)
        fit(w, s, z, p, batch_size=32, epochs=1, adam=AdamOptions(), _backend=be)
        with pytest.raises(ValueError, match="set_adam"):
            fit(w, s, z, p, batch_size=32, epochs=1, adam=AdamOptions(beta_2=0.99), _backend=be)


def test_fit_judges_epochs_by_the_averaged_weights():
    s, z, p = _tiny()
    w = nets.init_mlp12x100(1, bn_noise=True)
    ad = AdamOptions(beta_2=0.99, amsgrad=True, ema_momentum=0.9)
    be = S.RefBackend("mlp12x100")
    seen = []  # (val_loss, evaluated weights, averaged weights, raw weights) of every evaluate
    evaluate = be.evaluate

    def spy(*a):
        out = evaluate(*a)
        seen.append((out[0], be.w.copy(), be.get_slot("average")))
        return out

    be.evaluate = spy
    res = fit(w, s, z, p, batch_size=16, epochs=3, seed=1, adam=ad, _backend=be)
    be.evaluate = evaluate
    assert be.set_adam_calls == [ad] and be.swaps == 6 and be.applied == 1
    assert tuple(res.history) == HISTORY_KEYS and len(seen) == 3
    # every epoch's val_loss is that of the averaged weights: the same epochs by hand, swapping ourselves
    hand = S.RefBackend("mlp12x100")
    hand.set_weights(w)
    hand.set_optimizer(np.zeros_like(w), np.zeros_like(w), 0)
    hand.set_data(s, z, p)
    hand.set_adam(ad)
    rng = np.random.default_rng(1)
    vals, avgs = [], []
    for epoch in range(3):
        hand.train(rng.permutation(44).astype(np.int32), 16, np.float32(0.001))
        raw, avg = hand.w.copy(), hand.a.copy()
        assert np.any(raw != avg)
        hand.w = avg
        vals.append(hand.evaluate(44, 20, 16)[0])
        hand.w = raw
        avgs.append(avg.astype(np.float32))
    assert res.history["val_loss"] == vals
    # (while it evaluates, the backend holds the average as its weights and the raw weights as its average)
    assert all(x[1].astype(np.float32).tobytes() == a.tobytes() for x, a in zip(seen, avgs))
    best = int(np.argmin(vals))
    assert res.best_epoch == best and res.best_weights.tobytes() == avgs[best].tobytes()
    assert set(res.best_slots) == {"vhat", "average"} and res.best_slots["average"].tobytes() == avgs[best].tobytes()
    assert res.best_slots["vhat"].any() and np.all(res.best_slots["vhat"] >= res.best_optimizer[1])
    # finalised: the weights are the average on the trainable weights (and on the moving statistics it always was)
    assert res.weights.tobytes() == avgs[-1].tobytes() == res.slots["average"].tobytes()
    assert be.get_weights().tobytes() == res.weights.tobytes()
    # the raw weights of a fit without averaging, otherwise alike, differ
    raw = fit(w, s, z, p, batch_size=16, epochs=3, seed=1, adam=AdamOptions(beta_2=0.99, amsgrad=True), _backend=be)
    assert raw.weights.tobytes() != res.weights.tobytes() and set(raw.slots) == {"vhat"} and be.swaps == 6
    assert raw.optimizer[0].tobytes() == res.optimizer[0].tobytes()  # without overwrite the iterates are the same
    # and the next call with the defaults sets the backend back
    off = fit(w, s, z, p, batch_size=16, epochs=3, seed=1, _backend=be)
    plain = fit(w, s, z, p, batch_size=16, epochs=3, seed=1, _backend=S.RefBackend("mlp12x100"))
    assert be.set_adam_calls[-1] == AdamOptions() and off.weights.tobytes() == plain.weights.tobytes()
    assert off.slots is None


def test_fit_resident_resumes_from_slots():
    s, z, p = _tiny()
    w = nets.init_mlp12x100(1, bn_noise=True)
    ad = AdamOptions(amsgrad=True, ema_momentum=0.5)
    be = S.RefBackend("mlp12x100")
    be.data_info = lambda: (64, 0)
    be.set_data(s, z, p)
    planted = {"vhat": np.full(w.size, 1e6, np.float32), "average": np.zeros(w.size, np.float32)}
    res = fit_resident(be, w, batch_size=16, epochs=1, seed=1, adam=ad, slots=planted)
    tr = ~fit_ref.stat_mask()
    assert np.all(res.slots["vhat"][tr] == np.float32(1e6))  # nothing the fit saw exceeds it
    fresh = fit_resident(be, w, batch_size=16, epochs=1, seed=1, adam=ad)
    assert np.all(fresh.slots["vhat"][tr] < 1.0) and fresh.weights.tobytes() != res.weights.tobytes()
    # three steps at momentum 0.5 from an average of zeros: the average is at most 7/8 of the way to the weights
    assert np.all(np.abs(res.weights[tr]) <= np.abs(w[tr]) * 0.875 + 0.01)


# ---------------------------------------------------------------------------------------------------- the run
def test_run_params_toml_and_cli(tmp_path):
    d = RunParams(seed=1)
    assert d.adam_options() == AdamOptions() and d.adam_options().is_default()
    assert (d.beta_1, d.beta_2, d.adam_epsilon, d.amsgrad, d.ema_momentum, d.ema_overwrite_frequency) == (0.9, 0.999, 1e-7, False, 0.0, 0)
    assert d.epsilon == 0.25  # the search's noise weight keeps its name
    path = tmp_path / "a.toml"
    path.write_text("[hyperparameters]\nname = \"x\"\nbeta_1 = 0.8\nbeta_2 = 0.99\nadam_epsilon = 1e-8\namsgrad = true\n"
                    "ema_momentum = 0.99\nema_overwrite_frequency = 100\n")
    p, _ = R.parse_args(["--config", str(path), "--seed", "1"])
    assert p.adam_options() == AdamOptions(beta_1=0.8, beta_2=0.99, epsilon=1e-8, amsgrad=True, ema_momentum=0.99,
                                           ema_overwrite_frequency=100)
    assert isinstance(p.ema_overwrite_frequency, int) and p.amsgrad is True
    p, _ = R.parse_args(["--config", str(path), "--seed", "1", "--beta_1", "0.5", "--ema_momentum=0.9"])  # a flag beats the file
    assert (p.beta_1, p.beta_2, p.ema_momentum) == (0.5, 0.99, 0.9)
    p, _ = R.parse_args(["--seed", "1", "--amsgrad", "--adam_epsilon", "1e-6"])
    assert p.adam_options() == AdamOptions(amsgrad=True, epsilon=1e-6)
    assert R.parse_args(["--seed", "1"])[0].adam_options().is_default()
    for bad in (dict(beta_1=1.0), dict(beta_2=-0.5), dict(adam_epsilon=0.0), dict(ema_momentum=1.0),
                dict(ema_overwrite_frequency=3), dict(ema_momentum=0.5, ema_overwrite_frequency=-1)):
        with pytest.raises(ValueError):
            RunParams(seed=1, **bad)
    assert RunParams(seed=1, ema_momentum=0.5).as_dict()["ema_momentum"] == 0.5


def test_model_npz_round_trip(tmp_path):
    w = nets.init_mlp12x100(2)
    m, v = w * 0.5, w * w
    plain, slotted = str(tmp_path / "plain.npz"), str(tmp_path / "slots.npz")
    R.save_model(plain, w, (m, v, 7), "mlp12x100")
    R.save_model(str(tmp_path / "none.npz"), w, (m, v, 7), "mlp12x100", None)
    R.save_model(str(tmp_path / "empty.npz"), w, (m, v, 7), "mlp12x100", {})
    with open(plain, "rb") as f:
        data = f.read()
    for name in ("none.npz", "empty.npz"):  # without slots the file is what it is today
        with open(str(tmp_path / name), "rb") as f:
            assert f.read() == data
    with np.load(plain) as z:
        assert set(z.files) == {"weights", "adam_m", "adam_v", "adam_iterations", "net"}
    assert R.load_model_slots(plain) == {}
    R.save_model(slotted, w, (m, v, 7), "mlp12x100", {"vhat": v * 2, "average": w + 1})
    with np.load(slotted) as z:
        assert set(z.files) == {"weights", "adam_m", "adam_v", "adam_iterations", "net", "adam_vhat", "adam_average"}
    got = R.load_model(slotted, "mlp12x100")  # the return value is what it was
    assert len(got) == 2 and got[0].tobytes() == w.tobytes() and got[1][2] == 7 and got[1][0].tobytes() == m.tobytes()
    slots = R.load_model_slots(slotted)
    assert set(slots) == {"vhat", "average"} and slots["vhat"].tobytes() == (v * 2).tobytes()
    assert slots["average"].tobytes() == (w + 1).tobytes()
    R.save_model(slotted, w, (m, v, 7), "mlp12x100", {"vhat": v})
    assert set(R.load_model_slots(slotted)) == {"vhat"}


class AdamFitter(StubFitter):
    """test_run_cpu's float32 fitter with the calls of Adam's arguments: it records them, keeps an average that moves
    once per train() call and a vhat that is the running maximum of v, and fits as before"""

    def __init__(self):
        super().__init__()
        self.set_to, self.slots_set, self.calls = [], [], []
        self.avg = self.vhat = None
        self.adam = AdamOptions()

    def set_adam(self, adam=None):
        self.adam = adam
        self.set_to.append(adam)

    def set_weights(self, w):
        super().set_weights(w)
        self.avg = None

    def set_optimizer(self, m, v, iterations):
        super().set_optimizer(m, v, iterations)
        self.vhat = np.zeros_like(self.v)

    def set_slot(self, which, values):
        self.slots_set.append((which, np.array(values, np.float32)))
        if which == "vhat":
            self.vhat = np.asarray(values, np.float32).copy()
        else:
            self.avg = np.asarray(values, np.float32).copy()

    def get_slot(self, which):
        return (self.vhat if which == "vhat" else self.avg).astype(np.float32)

    def train(self, *a, **kw):
        if self.adam.averaged() and self.avg is None:
            self.avg = self.w.copy()
        out = super().train(*a, **kw)
        if self.adam.averaged():
            self.avg = self.avg + (self.w - self.avg) * np.float32(1 - self.adam.ema_momentum)
        if self.adam.amsgrad:
            self.vhat = np.maximum(self.vhat, self.v)
        return out

    def swap_average(self):
        self.calls.append("swap")
        self.w, self.avg = self.avg, self.w

    def apply_average(self):
        self.calls.append("apply")
        self.w = self.avg.copy()


def test_generation_passes_adam_and_saves_the_slots(tmp_path):
    ad = AdamOptions(beta_2=0.99, amsgrad=True, ema_momentum=0.5)
    fitter = AdamFitter()
    run = open_run(small(tmp_path, name="a", beta_2=0.99, amsgrad=True, ema_momentum=0.5, test_threshold=-1), fitter)
    res = run.generation()
    assert fitter.set_to == [ad] and fitter.slots_set == []  # gen_0 has no slots to resume from
    assert fitter.calls == ["swap", "swap"] * 2 + ["apply"]
    gen = os.path.join(run.root, "generations")
    with np.load(os.path.join(gen, "gen_1", "model.npz")) as z:
        assert set(z.files) == {"weights", "adam_m", "adam_v", "adam_iterations", "net", "adam_vhat", "adam_average"}
        assert z["weights"].tobytes() == res.fit.best_weights.tobytes() == z["adam_average"].tobytes()
        assert z["adam_vhat"].tobytes() == res.fit.best_slots["vhat"].tobytes()
    w1, opt1 = R.load_model(os.path.join(gen, "gen_1", "model.npz"), "mlp12x100")
    assert w1.tobytes() == res.fit.best_weights.tobytes() and opt1[2] == res.fit.best_optimizer[2]
    with open(os.path.join(gen, "gen_1", "training_logs", "fit_options.json")) as f:
        d = json.load(f)
    assert d["adam"] == ad.as_dict() and "epochs" not in d and not any(d["options"].values())
    # the next generation resumes from the slots of the model it starts from
    run.generation()
    assert [k for k, _ in fitter.slots_set] == ["average", "vhat"] and fitter.set_to == [ad, ad]
    saved = R.load_model_slots(os.path.join(gen, "gen_1", "model.npz"))
    assert all(saved[k].tobytes() == a.tobytes() for k, a in fitter.slots_set)
    # a run with the defaults: the fitter is set back, model.npz and the logs are what they are today
    fitter = AdamFitter()
    run = open_run(small(tmp_path, name="b"), fitter)
    res = run.generation()
    assert fitter.set_to == [AdamOptions()] and fitter.calls == [] and res.fit.slots is None
    with np.load(os.path.join(run.root, "generations", "gen_1", "model.npz")) as z:
        assert set(z.files) == {"weights", "adam_m", "adam_v", "adam_iterations", "net"}
    assert not os.path.exists(os.path.join(run.root, "generations", "gen_1", "training_logs", "fit_options.json"))
    # and so is a generation behind a fitter that knows nothing of Adam's arguments
    plain = open_run(small(tmp_path, name="c"), StubFitter()).generation()
    assert plain.fit.weights.tobytes() == res.fit.weights.tobytes() and plain.fit.history == res.fit.history
