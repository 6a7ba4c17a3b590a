"""CPU checks of network training (corintho_ai_amd/fit.py): the float64 restatement of the Keras step (tests/fit_ref.py)
against finite differences and steps written out by hand, then fit()'s host logic -- the split, the epochs, the two
callbacks, the history, argument checks -- driven by the restatement or by a scripted backend."""
import numpy as np
import pytest
import torch

from corintho_ai_amd import nets
from corintho_ai_amd.fit import (HISTORY_KEYS, METRIC_HISTORY_KEYS, MIN_DELTA, OPTION_HISTORY_KEYS, AdamOptions, FitOptions,
                                 LossOptions, fit, split_index)
from tests import fit_ref as R
from tests import fit_ref_loss as L
from tests import fit_ref_step as S


def _data(n, seed=0):
    return R.synthetic_samples(n, seed)


def test_gradients_match_central_differences():
    """autograd of the float64 restatement against (L(w + h) - L(w - h)) / 2h at sampled coordinates of every kind of
    tensor, 12-layer net, batch 8"""
    w = nets.init_mlp12x100(3, bn_noise=True).astype(np.float64)
    s, z, p = _data(8, 1)
    g, _, _ = S.loss_and_grad(R, w, s, z, p)
    lay, (kv, bv, kp, bp) = R.layer_offsets()
    rng = np.random.default_rng(2)
    coords = []
    for li in (0, 5, 11):
        k, b, ga, be, _, _, fi = lay[li]
        coords += [k + int(rng.integers(fi * 100)), b + int(rng.integers(100)), ga + int(rng.integers(100)),
                   be + int(rng.integers(100))]
    coords += [kv + int(rng.integers(100)), bv, kp + int(rng.integers(9600)), bp + int(rng.integers(96))]

    def loss(wv):
        with torch.no_grad():
            logits, v, _ = R.forward(torch.as_tensor(wv), torch.as_tensor(s, dtype=torch.float64), True)
            _, lv, lp = L.batch_losses(logits, v, torch.as_tensor(z, dtype=torch.float64), torch.as_tensor(p, dtype=torch.float64), LossOptions())
            return float(lv + 0.25 * lp)

    h = 1e-6
    for c in coords:
        wp, wm = w.copy(), w.copy()
        wp[c] += h
        wm[c] -= h
        fd = (loss(wp) - loss(wm)) / (2 * h)
        assert abs(fd - g[c]) <= 1e-6 * max(1.0, abs(g[c])), (c, fd, g[c])


def test_moving_variance_is_the_biased_batch_variance():
    w = nets.init_mlp12x100(4, bn_noise=True).astype(np.float64)
    s, z, p = _data(16, 2)
    g, _, st = S.loss_and_grad(R, w, s, z, p)
    lay, _ = R.layer_offsets()
    k, b, _, _, mu, va, fi = lay[0]
    a = np.maximum(s.astype(np.float64) @ w[k:k + fi * 100].reshape(fi, 100) + w[b:b + 100], 0.0)
    assert np.allclose(st[0][1], a.var(0, ddof=0)) and not np.allclose(st[0][1], a.var(0, ddof=1))
    m, v = np.zeros_like(w), np.zeros_like(w)
    w2 = w.copy()
    S.adam_step(R, w2, m, v, g, 0, 1e-3, st)
    assert np.allclose(w2[va:va + 100], w[va:va + 100] - (w[va:va + 100] - a.var(0, ddof=0)) * 0.01)
    assert np.allclose(w2[mu:mu + 100], 0.99 * w[mu:mu + 100] + 0.01 * a.mean(0))
    assert not m[R.stat_mask()].any() and not v[R.stat_mask()].any()


def test_one_adam_update_by_hand():
    """TF ResourceApplyAdam with epsilon outside the root, at step 1 and step 3"""
    w = nets.init_mlp12x100(5).astype(np.float64)
    s, z, p = _data(8, 3)
    g, _, st = S.loss_and_grad(R, w, s, z, p)
    i = int(np.argmax(np.abs(g[:7000])))  # a layer-0 kernel entry with a gradient
    assert g[i] != 0.0
    m, v, w2 = np.zeros_like(w), np.zeros_like(w), w.copy()
    assert S.adam_step(R, w2, m, v, g, 0, 0.001, st) == 1
    lr_t = 0.001 * np.sqrt(1 - 0.999) / (1 - 0.9)
    mm, vv = 0.1 * g[i], 0.001 * g[i] ** 2
    assert np.isclose(m[i], mm) and np.isclose(v[i], vv)
    assert np.isclose(w2[i], w[i] - lr_t * mm / (np.sqrt(vv) + 1e-7))
    m[i], v[i], w3 = 0.5, 0.25, w2.copy()
    S.adam_step(R, w3, m, v, g, 2, 0.001, st)
    lr_t = 0.001 * np.sqrt(1 - 0.999 ** 3) / (1 - 0.9 ** 3)
    mm, vv = 0.5 + (g[i] - 0.5) * 0.1, 0.25 + (g[i] ** 2 - 0.25) * 0.001
    assert np.isclose(w3[i], w2[i] - lr_t * mm / (np.sqrt(vv) + 1e-7))


def test_cross_entropy_from_logits():
    rng = np.random.default_rng(6)
    logits = torch.tensor(rng.normal(0, 3, (5, 96)), requires_grad=True)
    t = torch.tensor(rng.dirichlet(np.ones(96), 5))
    v = torch.zeros(5, dtype=torch.float64)
    _, _, lp = L.batch_losses(logits, v, torch.zeros(5, dtype=torch.float64), t, LossOptions())
    sm = np.exp(logits.detach().numpy())
    sm /= sm.sum(1, keepdims=True)
    assert np.isclose(float(lp), np.mean(-(t.numpy() * np.log(sm)).sum(1)))
    lp.backward()
    want = (sm * t.numpy().sum(1, keepdims=True) - t.numpy()) / 5
    assert np.allclose(logits.grad.numpy(), want)


# ------------------------------------------------------------------ fit() host logic
class Scripted:
    """a backend whose losses are given: val_loss of epoch e is vals[e]; the weights record the epoch"""

    def __init__(self, vals):
        self.vals, self.epoch, self.rows, self.lrs = list(vals), 0, [], []

    def set_weights(self, w):
        self.w = np.asarray(w, np.float32).copy()

    def get_weights(self):
        return self.w.copy()

    def set_optimizer(self, m, v, it):
        self.it = it

    def get_optimizer(self):
        return np.zeros(1, np.float32), np.zeros(1, np.float32), self.it

    def set_data(self, s, e, p):
        self.n = s.shape[0]

    def train(self, rows, batch, lr):
        self.rows.append(np.asarray(rows).copy())
        self.lrs.append(float(lr))
        self.w[0] = self.epoch
        self.it += -(-len(rows) // batch)
        return (1.0, 0.5, 2.0)

    def evaluate(self, row0, n, batch):
        v = self.vals[self.epoch]
        self.epoch += 1
        return (v, v / 2, v * 2)

    def close(self):
        pass


def _fit_scripted(vals, n=100, **kw):
    s, z, p = _data(n)
    be = Scripted(vals)
    res = fit(nets.init_mlp12x100(0), s, z, p, epochs=len(vals), _backend=be, **kw)
    return res, be


def test_split_before_shuffling_and_every_training_row_once():
    res, be = _fit_scripted([1.0, 0.9, 0.8], n=103, batch_size=8, validation_split=0.3)
    split = split_index(103, 0.3)
    assert split == 72  # floor(103 * 0.7)
    for r in be.rows:
        assert sorted(r.tolist()) == list(range(split))
    assert not np.array_equal(be.rows[0], be.rows[1])  # a fresh permutation every epoch
    assert be.it == 3 * 9  # 72 rows at batch 8: nine steps an epoch


def test_partial_last_batch_with_the_restatement():
    """n_train % batch != 0: the restatement's steps cover every training row once, the last batch partial"""
    s, z, p = _data(30, 4)
    be = S.RefBackend("mlp12x100")
    res = fit(nets.init_mlp12x100(1), s, z, p, batch_size=8, epochs=2, _backend=be)
    assert split_index(30, 0.3) == 21
    for r in be.trained_rows:
        assert sorted(r.tolist()) == list(range(21))
    assert res.optimizer[2] == 2 * 3  # ceil(21 / 8) = 3 steps an epoch
    assert all(np.isfinite(res.history[k]).all() for k in HISTORY_KEYS)


def test_same_seed_same_permutation():
    _, a = _fit_scripted([1.0, 0.9], seed=7)
    _, b = _fit_scripted([1.0, 0.9], seed=7)
    _, c = _fit_scripted([1.0, 0.9], seed=8)
    assert all(np.array_equal(x, y) for x, y in zip(a.rows, b.rows))
    assert not np.array_equal(a.rows[0], c.rows[0])
    _, d = _fit_scripted([1.0, 0.9], shuffle=False)
    assert all(np.array_equal(x, np.arange(70)) for x in d.rows)


def test_reduce_lr_on_plateau():
    """min_delta 1e-4, patience 2, factor 0.5: an epoch within min_delta of the best is no improvement"""
    vals = [1.0, 1.0 - MIN_DELTA / 2, 0.99999, 0.5, 0.5, 0.6, 0.4999, 0.49985]
    res, be = _fit_scripted(vals, learning_rate=0.001, anneal_factor=0.5, patience=2)
    lr1 = np.float32(np.float32(0.001) * np.float32(0.5))
    lr2 = np.float32(lr1 * np.float32(0.5))
    # epoch: 0 best 1.0 | 1 wait 1 | 2 wait 2 -> lr/2 | 3 best 0.5 | 4 wait 1 | 5 wait 2 -> lr/4 | 6 wait 1 (0.4999 is not
    # below 0.5 - 1e-4) | 7 best 0.49985
    want = [np.float32(0.001)] * 3 + [lr1] * 3 + [lr2] * 2
    assert be.lrs == [float(x) for x in want]
    assert res.history["lr"] == [float(x) for x in want]
    assert res.learning_rate == float(lr2)


def test_best_epoch_by_strict_less():
    res, be = _fit_scripted([1.0, 0.8, 0.8, 0.9])
    assert res.best_epoch == 1 and res.best_weights[0] == 1.0
    assert res.weights[0] == 3.0


def test_history_fields():
    res, _ = _fit_scripted([1.0, 0.7, 0.9])
    assert tuple(res.history) == HISTORY_KEYS
    assert all(len(v) == 3 for v in res.history.values())
    assert res.history["val_loss"] == [1.0, 0.7, 0.9] and res.history["val_policy_loss"] == [2.0, 1.4, 1.8]
    assert res.history["loss"] == [1.0] * 3 and res.history["value_loss"] == [0.5] * 3


def test_fit_with_the_restatement_keeps_the_best_epoch():
    """the checkpoint's weights give the history's smallest val_loss, computed on the validation rows alone"""
    s, z, p = _data(200, 5)
    w = nets.init_mlp12x100(2)
    be = S.RefBackend("mlp12x100")
    res = fit(w, s, z, p, batch_size=32, epochs=3, learning_rate=0.003, _backend=be)
    best = S.evaluate(R, res.best_weights.astype(np.float64), s[140:], z[140:], p[140:])[0][0]
    assert np.isclose(min(res.history["val_loss"]), best, rtol=1e-5)
    assert res.best_epoch == int(np.argmin(res.history["val_loss"]))


def test_argument_validation():
    s, z, p = _data(20)
    w = nets.init_mlp12x100(0)
    be = Scripted([1.0])
    bad = [dict(weights=w[:-1]), dict(game_states=s[:, :69]), dict(eval_labels=z[:-1]), dict(prob_labels=p[:, :95]),
           dict(batch_size=0), dict(epochs=0), dict(validation_split=0.0), dict(validation_split=1.0),
           dict(learning_rate=0.0), dict(anneal_factor=1.0), dict(patience=-1)]
    for kw in bad:
        args = dict(weights=w, game_states=s, eval_labels=z, prob_labels=p)
        for k in list(kw):
            if k in args:
                args[k] = kw.pop(k)
        with pytest.raises(ValueError):
            fit(args["weights"], args["game_states"], args["eval_labels"], args["prob_labels"], _backend=be, **kw)
    with pytest.raises(ValueError):  # one row leaves no training rows
        fit(w, s[:1], z[:1], p[:1], _backend=be)


def test_every_family_at_once_and_each_switched_off_again():
    """a Huber loss with smoothing, the regulariser with a clip, AMSGrad with averaged weights, sample weights and
    metrics in one fit: the history has every family's keys, and the same fit without one family, on the backend that
    just had it, is to the byte the fit of a backend that was never given that family"""
    s, z, p = _data(64, 5)
    w = nets.init_mlp12x100(1, bn_noise=True)
    sw = np.where(np.arange(64) % 3 == 0, 0.0, 1.5).astype(np.float32)
    calls = {"loss": (LossOptions(value_loss="huber", huber_delta=0.5, label_smoothing=0.1), ("set_loss", "get_loss")),
             "options": (FitOptions(l2=1e-3, global_clipnorm=0.05), ("set_options", "get_options", "train_stats")),
             "adam": (AdamOptions(amsgrad=True, ema_momentum=0.9),
                      ("set_adam", "get_adam", "set_slot", "get_slot", "swap_average", "apply_average"))}
    others = ("set_sample_weights", "set_metrics", "metrics")
    kw = dict(batch_size=16, epochs=2, seed=1, sample_weight=sw, metrics=True)
    be = S.RefBackend("mlp12x100")
    full = fit(w, s, z, p, _backend=be, **kw, **{k: v[0] for k, v in calls.items()})
    assert tuple(full.history) == HISTORY_KEYS + OPTION_HISTORY_KEYS + METRIC_HISTORY_KEYS
    assert all(len(x) == 2 for x in full.history.values()) and set(full.slots) == {"vhat", "average"}
    plain = fit(w, s, z, p, batch_size=16, epochs=2, seed=1, _backend=S.RefBackend("mlp12x100"))
    assert full.weights.tobytes() != plain.weights.tobytes()
    assert [full.history[k] for k in HISTORY_KEYS[:-1]] != [plain.history[k] for k in HISTORY_KEYS[:-1]]

    def arrays(res):
        out = [res.weights, res.best_weights, *res.optimizer[:2], *res.best_optimizer[:2]]
        return [a.tobytes() for a in out + [d[k] for d in (res.slots, res.best_slots) for k in sorted(d or {})]]

    for off in calls:
        rest = {k: v[0] for k, v in calls.items() if k != off}
        again = fit(w, s, z, p, _backend=be, **kw, **rest)
        never = S.BaseOnly(S.RefBackend("mlp12x100"), *others, *(n for k, v in calls.items() if k != off for n in v[1]))
        assert not any(hasattr(never, n) for n in calls[off][1])
        want = fit(w, s, z, p, _backend=never, **kw, **rest)
        assert again.history == want.history and again.best_epoch == want.best_epoch, off
        assert arrays(again) == arrays(want) and again.optimizer[2] == want.optimizer[2] == 6, off
        assert again.weights.tobytes() != full.weights.tobytes(), off
