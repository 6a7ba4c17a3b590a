"""The fit options without a GPU (include/corintho_hip.h, "fit options"): the restatement the device is judged by
(tests/fit_ref_options.py) against torch autograd and hand-written cases, nets.tensor_table, how fit() and its
relatives treat `options`, and the run's settings."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from corintho_ai_amd import FitOptions, RunParams, fit, fit_resident, fit_samples, fit_trainer, nets
from corintho_ai_amd import run as R
from corintho_ai_amd.fit import HISTORY_KEYS, OPTION_HISTORY_KEYS
from tests import fit_ref, fit_ref_options as O
from tests import fit_ref_rescnn4
from tests import fit_ref_step as S
from tests.test_run_cpu import StubFitter, open_run, small

NETS = pytest.mark.parametrize("net", ["mlp12x100", "rescnn4"])
INIT = {"mlp12x100": nets.init_mlp12x100, "rescnn4": nets.init_rescnn4}


# ---------------------------------------------------------------------------------------------------- the tensor table
@NETS
def test_tensor_table_covers_the_weights(net):
    table = nets.tensor_table(net)
    at = 0
    for name, off, n, cls in table:
        assert off == at and n >= 1 and cls in nets.TENSOR_CLASSES, name
        at += n
    assert at == INIT[net](0).size
    names = [t[0] for t in table]
    assert len(set(names)) == len(names)
    trunk = [t[0] for t in table if t[3] == "trunk_kernel"]
    head = [t[0] for t in table if t[3] == "head_kernel"]
    if net == "mlp12x100":
        assert trunk == ["k%d" % l for l in range(12)] and head == ["kv", "kp"]
        assert not (O.class_mask(net, ("moving",)) ^ fit_ref.stat_mask()).any()
    else:
        assert trunk == ["stem_k"] + ["b%d_c%d_k" % (b, c) for b in range(4) for c in (1, 2)]
        assert head == ["p_k", "p_dk", "v_k", "v_d1k", "v_d2k"]
        assert names == [n for n, _ in nets._rescnn4_shapes()]
        assert not (O.class_mask(net, ("moving",)) ^ fit_ref_rescnn4.stat_mask()).any()
    for cls in ("bias", "gamma", "beta"):
        assert sum(1 for t in table if t[3] == cls) >= 11
    with pytest.raises(ValueError):
        nets.tensor_table("vgg")


# ---------------------------------------------------------------------------------------------------- the restatement
@NETS
@pytest.mark.parametrize("regularize", [0, 1])
def test_regulariser_gradient_is_autograd_of_R(net, regularize):
    """r of step 1 is the gradient of R of step 5, exact zeros included (sgn 0 = 0 on both sides)"""
    o = FitOptions(l1=0.03, l2=0.007, regularize=regularize)
    w = INIT[net](3, bn_noise=True).astype(np.float64)
    mask = O.regularized_mask(net, o)
    where = np.flatnonzero(mask)
    w[where[::7]] = 0.0
    w[where[3]] = -0.0
    wt = torch.tensor(w, requires_grad=True)
    m = torch.as_tensor(mask)
    l1, l2 = float(np.float32(o.l1)), float(np.float32(o.l2))
    Rt = l1 * wt[m].abs().sum() + l2 * (wt[m] ** 2).sum()
    Rt.backward()
    Rv = float(Rt.detach())
    r = O.reg_grad(net, w, o)
    assert np.array_equal(r[~mask], np.zeros((~mask).sum())) and not wt.grad.numpy()[~mask].any()
    assert np.max(np.abs(r - wt.grad.numpy())) <= 1e-15
    assert not r[where[::7]].any()
    assert abs(O.reg_loss(net, w, o) - Rv) <= 1e-12 * Rv
    # the head kernels are reached by regularize = 1 only
    heads = O.class_mask(net, ("head_kernel",))
    assert bool(r[heads].any()) == bool(regularize)
    assert not r[O.class_mask(net, ("bias", "gamma", "beta", "moving"))].any()


def _hand_gradient():
    """an mlp12x100 gradient with known norms: k3 has 10 000 entries of 0.1 (norm 10), b0 100 entries of -0.03 (norm 0.3),
    kv 100 entries of 0.2 (norm 2); a moving statistic holds a value that nothing may touch"""
    t = {name: sl for name, sl, _ in O.tensors("mlp12x100")}
    g = np.zeros(nets.MLP_NUM_WEIGHTS)
    g[t["k3"]] = 0.1
    g[t["b0"]] = -0.03
    g[t["kv"]] = 0.2
    g[t["mean5"]] = 123.0
    return g, t


def test_clip_scales_by_hand():
    g, t = _hand_gradient()
    total = np.sqrt(100.0 + 0.09 + 4.0)
    # per tensor, threshold 1: k3 to a tenth, kv to a half, b0 as it is
    out, info = O.clip("mlp12x100", g, FitOptions(clipnorm=1.0))
    assert info["scales"]["k3"] == np.float32(1.0 / 10.0) and info["scales"]["kv"] == np.float32(0.5)
    assert info["scales"]["b0"] == np.float32(1.0) and info["scales"]["gamma7"] == np.float32(1.0)
    assert abs(info["norms"]["k3"] - 10.0) < 1e-12 and abs(info["norm"] - total) < 1e-12 and info["clipped"]
    assert np.array_equal(out[t["b0"]], g[t["b0"]]) and np.allclose(out[t["k3"]], 0.1 * np.float32(0.1), rtol=1e-15)
    assert np.array_equal(out[t["mean5"]], g[t["mean5"]])
    # one norm over everything
    out, info = O.clip("mlp12x100", g, FitOptions(global_clipnorm=2.0))
    s = np.float32(2.0 / total)
    assert set(info["scales"].values()) == {s} and info["clipped"]
    assert np.allclose(out[t["b0"]], -0.03 * float(s), rtol=1e-15) and np.array_equal(out[t["mean5"]], g[t["mean5"]])
    # a threshold above the norm: the scale is 1.0f exactly and nothing changes
    out, info = O.clip("mlp12x100", g, FitOptions(global_clipnorm=2.0 * total))
    assert set(info["scales"].values()) == {np.float32(1.0)} and not info["clipped"] and np.array_equal(out, g)
    # by value
    out, info = O.clip("mlp12x100", g, FitOptions(clipvalue=0.05))
    assert np.array_equal(out[t["k3"]], np.full(10000, float(np.float32(0.05))))
    assert np.array_equal(out[t["kv"]], np.full(100, float(np.float32(0.05)))) and np.array_equal(out[t["b0"]], g[t["b0"]])
    assert info["clipped"] and np.array_equal(out[t["mean5"]], g[t["mean5"]])
    assert not O.clip("mlp12x100", g, FitOptions(clipvalue=0.5))[1]["clipped"]
    # no clip mode: nothing happens
    out, info = O.clip("mlp12x100", g, FitOptions(l2=1.0))
    assert np.array_equal(out, g) and not info["clipped"]


def test_decay_by_hand():
    w = nets.init_mlp12x100(2, bn_noise=True).astype(np.float64)
    o = FitOptions(weight_decay=0.25)
    w1 = O.decay("mlp12x100", w, 0.5, o)
    k = O.class_mask("mlp12x100", O.KERNELS)
    assert np.array_equal(w1[~k], w[~k]) and np.allclose(w1[k], w[k] * (1 - 0.125), rtol=1e-15)
    assert k.sum() == 7000 + 11 * 10000 + 100 + 9600
    assert np.array_equal(O.decay("mlp12x100", w, 0.5, FitOptions()), w)


# ---------------------------------------------------------------------------------------------------- fit() and options
def _tiny():
    return fit_ref.synthetic_samples(64, 5)


def test_fit_history_and_reset():
    s, z, p = _tiny()
    w = nets.init_mlp12x100(1, bn_noise=True)
    be = S.RefBackend("mlp12x100")
    o = FitOptions(l2=1e-3, weight_decay=1e-2, global_clipnorm=0.05)
    on = fit(w, s, z, p, batch_size=16, epochs=2, seed=1, options=o, _backend=be)
    assert be.set_options_calls == [o]
    assert set(on.history) == set(HISTORY_KEYS + OPTION_HISTORY_KEYS)
    assert all(len(on.history[k]) == 2 for k in on.history)
    assert on.history["clipped_steps"] == [3, 3] and min(on.history["grad_norm"]) > 0.05
    assert all(x > 0 for x in on.history["regularization_loss"])
    # R is in loss and in val_loss, and in neither of the two parts
    for e in range(2):
        assert on.history["loss"][e] > on.history["value_loss"][e] + 0.25 * on.history["policy_loss"][e] + 1e-6
        assert on.history["val_loss"][e] > on.history["val_value_loss"][e] + 0.25 * on.history["val_policy_loss"][e] + 1e-6
    # the next call asks for none: the backend is reset, the keys are the old ones, the result that of a plain backend
    off = fit(w, s, z, p, batch_size=16, epochs=2, seed=1, _backend=be)
    assert be.set_options_calls == [o, FitOptions()] and tuple(off.history) == HISTORY_KEYS
    plain = fit(w, s, z, p, batch_size=16, epochs=2, seed=1, _backend=S.RefBackend("mlp12x100"))
    assert off.weights.tobytes() == plain.weights.tobytes() and off.history == plain.history
    assert on.weights.tobytes() != plain.weights.tobytes()
    # all-zero options are no options
    zero = fit(w, s, z, p, batch_size=16, epochs=2, seed=1, options=FitOptions(), _backend=be)
    assert tuple(zero.history) == HISTORY_KEYS and zero.weights.tobytes() == plain.weights.tobytes()
    # a dict of the fields is taken too
    d = fit(w, s, z, p, batch_size=16, epochs=2, seed=1, options=o.as_dict(), _backend=be)
    assert d.weights.tobytes() == on.weights.tobytes() and d.history == on.history


def test_backend_without_options():
    s, z, p = _tiny()
    w = nets.init_mlp12x100(1)
    be = S.BaseOnly(S.RefBackend("mlp12x100"))
    assert not hasattr(be, "set_options")
    fit(w, s, z, p, batch_size=32, epochs=1, _backend=be)
    fit(w, s, z, p, batch_size=32, epochs=1, options=FitOptions(), _backend=be)
    with pytest.raises(ValueError, match="set_options"):
        fit(w, s, z, p, batch_size=32, epochs=1, options=FitOptions(l2=1.0), _backend=be)


BAD = [FitOptions(clipnorm=1.0, clipvalue=1.0), FitOptions(clipnorm=1.0, global_clipnorm=1.0), FitOptions(l2=-1e-3),
       FitOptions(weight_decay=float("nan")), FitOptions(l1=float("inf")), FitOptions(regularize=2), FitOptions(l2=1e300),
       {"l3": 1.0}, "l2"]


@pytest.mark.parametrize("bad", BAD, ids=[str(i) for i in range(len(BAD))])
def test_argument_errors_before_any_fitter(bad, monkeypatch):
    F = sys.modules["corintho_ai_amd.fit"]  # (the package's attribute `fit` is the function)

    def no_fitter(*a, **kw):
        raise AssertionError("a fitter was made")

    monkeypatch.setattr(F, "Fitter", no_fitter)
    s, z, p = _tiny()
    w = nets.init_mlp12x100(1)
    sp = np.concatenate([s, p], axis=1)
    with pytest.raises(ValueError):
        fit(w, s, z, p, options=bad)
    with pytest.raises(ValueError):
        fit_samples(w, sp, z, options=bad)
    with pytest.raises(ValueError):
        fit_trainer(w, [object()], options=bad)
    with pytest.raises(ValueError):
        fit_resident(object(), w, options=bad)


def test_options_dataclass():
    assert not FitOptions().any() and FitOptions(clipvalue=1e-3).any() and not FitOptions(regularize=1).any()
    assert not FitOptions(l2=1e-60).any()  # 0 in float32: off, as the device sees it
    assert FitOptions(l2=0.5, regularize=1).as_dict() == dict(l1=0.0, l2=0.5, weight_decay=0.0, clipvalue=0.0, clipnorm=0.0,
                                                             global_clipnorm=0.0, regularize=1)


# ---------------------------------------------------------------------------------------------------- the run
def test_run_params_toml_and_cli(tmp_path):
    d = RunParams(seed=1)
    assert (d.l1, d.l2, d.regularize, d.weight_decay, d.clipvalue, d.clipnorm, d.global_clipnorm) == (0, 0, 0, 0, 0, 0, 0)
    assert not d.fit_options().any()
    path = tmp_path / "o.toml"
    path.write_text("[hyperparameters]\nname = \"x\"\nl2 = 1e-4\nweight_decay = 0.01\nglobal_clipnorm = 2\nregularize = 1\n")
    p, _ = R.parse_args(["--config", str(path), "--seed", "1"])
    assert p.fit_options() == FitOptions(l2=1e-4, weight_decay=0.01, global_clipnorm=2.0, regularize=1)
    assert isinstance(p.global_clipnorm, float) and isinstance(p.regularize, int)
    p, _ = R.parse_args(["--config", str(path), "--seed", "1", "--l2", "0.5", "--l1=0.25"])  # a flag beats the file
    assert (p.l1, p.l2, p.weight_decay) == (0.25, 0.5, 0.01)
    p, _ = R.parse_args(["--seed", "1", "--clipvalue", "0.5", "--weight_decay", "1e-3"])
    assert p.fit_options() == FitOptions(clipvalue=0.5, weight_decay=1e-3)
    assert R.parse_args(["--seed", "1", "--clipnorm", "3"])[0].clipnorm == 3.0
    for bad in (dict(l2=-1.0), dict(clipnorm=1.0, clipvalue=2.0), dict(regularize=3), dict(weight_decay=float("nan"))):
        with pytest.raises(ValueError):
            RunParams(seed=1, **bad)
    assert RunParams(seed=1, l2=0.5).as_dict()["l2"] == 0.5


class OptionFitter(StubFitter):
    """test_run_cpu's float32 fitter with the option calls: it records what it is set to and fits as before"""

    def __init__(self):
        super().__init__()
        self.set_to = []

    def set_options(self, options=None):
        self.set_to.append(options)

    def train_stats(self):
        return {"steps": 1, "clipped_steps": 1, "regularization_loss": 0.125, "grad_norm": 2.5, "grad_norm_max": 3.0}


def test_generation_passes_the_options_and_logs_them(tmp_path):
    o = FitOptions(l2=1e-4, global_clipnorm=2.0)
    files = []
    for name in ("a", "b"):
        fitter = OptionFitter()
        run = open_run(small(tmp_path, name=name, l2=1e-4, global_clipnorm=2.0), fitter)
        res = run.generation()
        assert fitter.set_to == [o]
        assert res.fit.history["clipped_steps"] == [1, 1]
        with open(os.path.join(run.root, "generations", "gen_1", "training_logs", "fit_options.json"), "rb") as f:
            files.append(f.read())
        with np.load(os.path.join(run.root, "generations", "gen_1", "model.npz")) as z:
            assert set(z.files) == {"weights", "adam_m", "adam_v", "adam_iterations", "net"}
    assert files[0] == files[1]
    d = json.loads(files[0])
    assert d["options"] == o.as_dict()
    assert d["epochs"] == {"regularization_loss": [0.125, 0.125], "grad_norm": [2.5, 2.5], "clipped_steps": [1, 1]}
    # a run without options resets the fitter and writes no such file
    fitter = OptionFitter()
    run = open_run(small(tmp_path, name="c"), fitter)
    run.generation()
    assert fitter.set_to == [FitOptions()]
    assert not os.path.exists(os.path.join(run.root, "generations", "gen_1", "training_logs", "fit_options.json"))
