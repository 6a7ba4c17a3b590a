"""CPU checks of rescnn4 training (corintho_ai_amd.fit.fit(..., net=NET_RESCNN4)): the restatement of the step
(tests/fit_ref_rescnn4.py) against the project's float64 inference forward, against finite differences and against
updates written out by hand; then fit()'s host logic driven by the restatement on rescnn4 weights."""
import numpy as np
import pytest
import torch

from corintho_ai_amd import NET_RESCNN4, nets
from corintho_ai_amd.fit import HISTORY_KEYS, MIN_DELTA, fit, split_index
from corintho_ai_amd.fit import LossOptions
from tests import fit_ref_loss as L
from tests import fit_ref_rescnn4 as R
from tests import fit_ref_step as S
from tests import ref_nets

WEIGHTS = [("init", lambda: nets.init_rescnn4(0)), ("bn-noise", lambda: nets.init_rescnn4(7, bn_noise=True)),
           ("trained-like", lambda: nets.trained_like_rescnn4(1))]


@pytest.mark.parametrize("name,make", WEIGHTS, ids=[n for n, _ in WEIGHTS])
def test_inference_mode_is_the_projects_forward(name, make):
    w = make()
    s, z, p = R.synthetic_samples(48, 2)
    ev64, pr64 = ref_nets.rescnn4_forward_f64(w, s)
    _, (ev, pr) = S.evaluate(R, w, s, z, p)
    assert np.max(np.abs(ev - ev64)) <= 1e-6 and np.max(np.abs(pr - pr64)) <= 1e-6  # the oracle returns float32


def test_layout_and_masks():
    off = R.offsets()
    assert sum(int(np.prod(sh)) for _, sh in off.values()) == nets.RESCNN4_NUM_WEIGHTS
    mask = R.stat_mask()
    assert mask.sum() == 2 * (9 * 64 + 4 + 2)
    covered = np.zeros(nets.RESCNN4_NUM_WEIGHTS, int)
    for _, sl, _ in R.tensors():
        covered[sl] += 1
    assert np.array_equal(covered == 1, ~mask) and covered.max() == 1
    by_name = {n: (sl, sc) for n, sl, sc in R.tensors()}
    # a bias under a training-mode BatchNorm is scaled by that BatchNorm's beta; every other tensor by itself
    assert by_name["b2_c1_b"][1] == by_name["b2_c1_bn1"][0] and by_name["p_b"][1] == by_name["p_bn1"][0]
    assert by_name["v_d1b"][1] == by_name["v_d1b"][0] and by_name["p_db"][1] == by_name["p_db"][0]


def test_gradients_match_central_differences():
    """autograd of the float64 restatement against (L(w + h) - L(w - h)) / 2h at a handful of entries of every tensor;
    batch 6, weights with every BatchNorm term perturbed"""
    w = nets.init_rescnn4(3, bn_noise=True).astype(np.float64)
    s, z, p = R.synthetic_samples(6, 1)
    g, _, _ = S.loss_and_grad(R, w, s, z, p)
    rng = np.random.default_rng(2)
    st, zt, pt = (torch.as_tensor(a, dtype=torch.float64) for a in (s, z, p))

    def loss(wv):
        with torch.no_grad():
            logits, v, _ = R.forward(torch.as_tensor(wv), st, True)
            _, lv, lp = L.batch_losses(logits, v, zt, pt, LossOptions())
            return float(lv + 0.25 * lp)

    h = 1e-6
    top = float(np.max(np.abs(g)))
    for name, sl, _ in R.tensors():
        n = sl.stop - sl.start
        for c in sl.start + rng.choice(n, min(3, n), replace=False):
            wp, wm = w.copy(), w.copy()
            wp[c] += h
            wm[c] -= h
            fd = (loss(wp) - loss(wm)) / (2 * h)
            assert abs(fd - g[c]) <= 1e-6 * max(1.0, abs(g[c])), (name, c, fd, g[c])
    # the biases under a BatchNorm: zero up to rounding
    for name, sl, _ in R.tensors():
        if name.endswith("_b") and name[:-2] in R.BN_PREFIXES:
            assert np.max(np.abs(g[sl])) <= 1e-12 * max(top, 1.0), name
    assert not g[R.stat_mask()].any()


def test_moving_statistics_by_hand():
    """the stem's batch statistics are the mean and BIASED variance of conv + bias over all (row, pixel) pairs, and
    every moving statistic moves 1 % of the way toward its batch statistic"""
    w = nets.init_rescnn4(4, bn_noise=True).astype(np.float64)
    s, z, p = R.synthetic_samples(5, 2)
    g, _, st = S.loss_and_grad(R, w, s, z, p)
    assert len(st) == len(R.BN_PREFIXES) == 11
    W = nets.rescnn4_unpack(w.astype(np.float32))
    x = np.pad(nets.rescnn4_input_planes(s).astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    k = w[R._slice(R.offsets(), "stem_k")].reshape(3, 3, 10, 64)
    zc = np.zeros((5, 4, 4, 64))
    for ky in range(3):
        for kx in range(3):
            zc += x[:, ky:ky + 4, kx:kx + 4, :] @ k[ky, kx]
    zc = (zc + W["stem_b"].astype(np.float64)).reshape(80, 64)
    assert np.allclose(st[0][0], zc.mean(0)) and np.allclose(st[0][1], zc.var(0, ddof=0))
    assert not np.allclose(st[0][1], zc.var(0, ddof=1))
    m, v, w2 = np.zeros_like(w), np.zeros_like(w), w.copy()
    S.adam_step(R, w2, m, v, g, 0, 1e-3, st)
    off = R.offsets()
    for pre, (bm, bv) in zip(R.BN_PREFIXES, st):
        mu, va = R._slice(off, pre + "_bn2"), R._slice(off, pre + "_bn3")
        assert np.allclose(w2[mu], 0.99 * w[mu] + 0.01 * bm, rtol=1e-12, atol=1e-15)
        assert np.allclose(w2[va], w[va] - (w[va] - bv) * 0.01, rtol=1e-12, atol=1e-15)
    assert not m[R.stat_mask()].any() and not v[R.stat_mask()].any()


def test_one_adam_update_by_hand():
    """TF ResourceApplyAdam with epsilon outside the root, at step 1 and step 3, on a block kernel entry"""
    w = nets.init_rescnn4(5).astype(np.float64)
    s, z, p = R.synthetic_samples(8, 3)
    g, _, st = S.loss_and_grad(R, w, s, z, p)
    sl = R._slice(R.offsets(), "b1_c2_k")
    i = sl.start + int(np.argmax(np.abs(g[sl])))
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


def test_fit_rescnn4_with_the_restatement():
    """fit(..., net=NET_RESCNN4) on rescnn4 weights: history, the checkpoint, ReduceLROnPlateau, the size check"""
    s, z, p = R.synthetic_samples(60, 5)
    w = nets.init_rescnn4(2)
    be = S.RefBackend("rescnn4", torch.float64)
    # a learning rate too large for 60 rows: the validation loss rises after the first epoch, so ReduceLROnPlateau acts
    res = fit(w, s, z, p, batch_size=16, epochs=6, learning_rate=0.01, patience=2, anneal_factor=0.5, net=NET_RESCNN4,
              _backend=be)
    assert tuple(res.history) == HISTORY_KEYS and all(len(v) == 6 for v in res.history.values())
    assert all(np.isfinite(res.history[k]).all() for k in HISTORY_KEYS)
    vals = res.history["val_loss"]
    assert res.best_epoch == int(np.argmin(vals))
    # the callback by hand on the recorded val_loss: an epoch improves if it is more than min_delta below the best so
    # far; after `patience` epochs that do not, the rate is halved
    lr, best, wait, want = np.float32(0.01), np.inf, 0, []
    for x in vals:
        want.append(float(lr))
        if x < best - MIN_DELTA:
            best, wait = x, 0
        else:
            wait += 1
            if wait >= 2:
                lr, wait = np.float32(lr * np.float32(0.5)), 0
    assert be.lrs == want and res.history["lr"] == want and res.learning_rate == float(lr)
    assert want[-1] < want[0], (vals, want)  # it dropped
    flat = [e for e in range(1, 6) if want[e] < want[e - 1]]
    e = flat[0]  # the first drop follows two epochs without improvement
    assert all(vals[k] >= min(vals[:k]) - MIN_DELTA for k in (e - 2, e - 1)), (vals, want)
    split = split_index(60, 0.3)
    for r in be.trained_rows:
        assert sorted(r.tolist()) == list(range(split))
    assert res.optimizer[2] == 6 * -(-split // 16)
    assert res.best_weights.size == nets.RESCNN4_NUM_WEIGHTS
    best = S.evaluate(R, res.best_weights.astype(np.float64), s[split:], z[split:], p[split:])[0][0]
    assert np.isclose(min(vals), best, rtol=1e-5)
    # a real learning rate moves the weights and the moving statistics
    res2 = fit(w, s, z, p, batch_size=16, epochs=1, learning_rate=1e-3, net=NET_RESCNN4, _backend=S.RefBackend("rescnn4"))
    mask = R.stat_mask()
    assert np.any(res2.weights[mask] != w[mask]) and np.any(res2.weights[~mask] != w[~mask])
    with pytest.raises(ValueError, match="rescnn4"):
        fit(nets.init_mlp12x100(0), s, z, p, net=NET_RESCNN4, _backend=S.RefBackend("rescnn4"))
    with pytest.raises(ValueError, match="mlp12x100"):
        fit(w, s, z, p, _backend=S.RefBackend("rescnn4"))
    with pytest.raises(ValueError):
        fit(w, s, z, p, net=7, _backend=S.RefBackend("rescnn4"))
