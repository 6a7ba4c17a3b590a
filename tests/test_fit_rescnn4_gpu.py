"""rescnn4 training on the MI355X (csrc/nn_train_conv.hip and nn_train.hip through corintho_ai_amd.fit) against the
float64 restatement of the step (tests/fit_ref_rescnn4.py).  The rule of tests/test_fit_gpu.py: the device's error
against float64 is at most 4 x the float32 restatement's own error against float64, plus a small floor.  The Adam
steps, the bitwise repeat and the set/get round trip of this network are tests/test_fit_gpu.py's, parametrised."""
import ctypes as C

import numpy as np
import pytest

from corintho_ai_amd import NET_MLP12X100, NET_RESCNN4, NET_RESCNN4_H3, Trainer, _lib, nets, samples_io
from corintho_ai_amd.fit import Fitter, fit, split_index
from tests import fit_ref
from tests import fit_ref_rescnn4 as R
from tests import ref_nets
from tests import fit_ref_step as S
from tests.fit_ref_step import within as _within

pytestmark = pytest.mark.gpu

WEIGHTS = [("init", lambda: nets.init_rescnn4(0)), ("bn-noise", lambda: nets.init_rescnn4(7, bn_noise=True)),
           ("trained-like", lambda: nets.trained_like_rescnn4(1))]
KINK = 2e-7


def _check_gradient(f, w, data, rows, tag, kink, bad):
    """one batch's device gradient and losses against the two restatements; failures are appended to bad"""
    g, losses = f.gradients(rows)
    s, z, p = (a[rows] for a in data)
    g64, l64, _ = S.loss_and_grad(R, w, s, z, p)
    g32, l32, _ = S.loss_and_grad(R, w, s, z, p, dtype=R.torch.float32)
    assert not g[R.stat_mask()].any(), "gradient at a moving statistic"
    for name, sl, scale in R.tensors():
        top = float(np.max(np.abs(g64[scale])))
        ok, ed, e3 = _within(g[sl], g32[sl], g64[sl], 2e-5 * top + 1e-12)
        if kink:
            ok = ed <= 0.05 * top + 1e-12
        print("%s %-10s kink=%d dev %.3e f32 %.3e top %.3e%s" % (tag, name, kink, ed, e3, top, "" if ok else "  FAIL"))
        if not ok:
            bad.append((tag, name, kink, ed, e3, top))
    ok, ed, e3 = _within(losses, l32, l64, 1e-6 * abs(l64[0]))
    print("%s losses dev %.3e f32 %.3e" % (tag, ed, e3))
    if not ok:
        bad.append((tag, "losses", ed, e3))


def test_gradients_of_small_batches():
    """every trainable tensor within 4 x the float32 restatement's error plus 2e-5 of the tensor's largest entry (for a
    bias under a BatchNorm, whose gradient is 0, of that BatchNorm's beta gradient); a batch with a ReLU input within
    2e-7 (of its tensor's largest) of the kink is held to 5 % of the largest entry instead"""
    data = R.synthetic_samples(4096, 11)
    bad, cases, kinked = [], 0, 0
    rng = np.random.default_rng(3)
    with Fitter(max_batch=32, net=NET_RESCNN4) as f:
        f.set_data(*data)
        for wname, make in WEIGHTS:
            w = make()
            f.set_weights(w)
            for B in (1, 2, 5, 16, 17, 24):
                rows = rng.choice(4096, B, replace=False).astype(np.int32)
                margin = S.kink_margin(R, w, data[0][rows])
                kink = margin < KINK
                print("%s B=%d margin %.3e" % (wname, B, margin))
                cases += 1
                kinked += kink
                _check_gradient(f, w, data, rows, "%s B=%d" % (wname, B), kink, bad)
    assert not bad, "device error above 4 x float32's: %s" % bad[:12]
    assert cases == 18 and kinked <= cases // 4, (kinked, cases)


def test_gradients_at_scale_without_a_kink():
    """the row-split partials and the two-stage BatchNorm reductions, strictly: with 12 added to every beta each
    BatchNorm-fed ReLU is active, and no ReLU input of these batches lies within 2e-7 of its kink"""
    data = R.synthetic_samples(4096, 11)
    off = R.offsets()
    bad = []
    rng = np.random.default_rng(5)
    with Fitter(max_batch=2048, net=NET_RESCNN4) as f:
        f.set_data(*data)
        for seed in (7, 8):
            w = nets.init_rescnn4(seed, bn_noise=True)
            for pre in R.BN_PREFIXES:
                w[R._slice(off, pre + "_bn1")] += np.float32(12.0)
            f.set_weights(w)
            for B in (256, 2047, 2048):
                rows = rng.choice(4096, B, replace=False).astype(np.int32)
                margin = S.kink_margin(R, w, data[0][rows])
                print("seed %d B=%d margin %.3e" % (seed, B, margin))
                assert margin >= KINK, (seed, B, margin)
                _check_gradient(f, w, data, rows, "seed %d B=%d" % (seed, B), False, bad)
    assert not bad, "device error above 4 x float32's: %s" % bad[:12]


def test_whole_loop_small(tmp_path):
    """a generation of the headline network without TensorFlow: fused self-play -> samples_for_training -> fit ->
    the engine's network on the fitted weights -> arena of the new weights against the old"""
    w0 = nets.init_rescnn4(0)
    t = Trainer(256, "", 5, 100, 16, 1.0, 0.25, 0, 1, False, stagger=False)
    t.set_net(NET_RESCNN4_H3, w0)
    assert t.run()
    s, z, p = samples_io.samples_for_training(t, str(tmp_path / "gen_0"))
    res = fit(w0, s, z, p, batch_size=512, epochs=3, net=NET_RESCNN4)
    n = s.shape[0]
    split = split_index(n, 0.3)
    with Fitter(max_batch=512, net=NET_RESCNN4) as f:
        f.set_data(s, z, p)
        f.set_weights(w0)
        start = f.evaluate(split, n - split, 512)[0]
    vals = res.history["val_loss"]
    print("rows %d start %.6f val_loss %s" % (n, start, vals))
    assert min(vals) < start, (vals, start)
    assert res.best_epoch == int(np.argmin(vals))
    # the best epoch's val_loss is the restatement's on the checkpoint
    l64 = S.evaluate(R, res.best_weights, s[split:], z[split:], p[split:])[0]
    l32 = S.evaluate(R, res.best_weights, s[split:], z[split:], p[split:], dtype=R.torch.float32)[0]
    ok, ed, e3 = _within(vals[res.best_epoch], l32[0], l64[0], 1e-6 * abs(l64[0]))
    print("val_loss dev %.3e f32 %.3e" % (ed, e3))
    assert ok, ("val_loss of the best epoch", ed, e3)
    # the engine's network on the fitted weights: the project's 1e-4 output contract
    e = Trainer(64, "", 1, 50, 16, 1.0, 0.25, 0, 1, False)
    e.set_net(NET_RESCNN4_H3, res.best_weights)
    sub = s[split:split + 64 * 16]
    ev, pr = e.net_forward(sub)
    ev64, pr64 = ref_nets.rescnn4_forward_f64(res.best_weights, sub)
    assert np.max(np.abs(ev - ev64)) < 1e-4 and np.max(np.abs(pr - pr64)) < 1e-4
    # the first rescnn4 weights with real statistics: every BatchNorm's moving variances have left 1
    off = R.offsets()
    for pre in R.BN_PREFIXES:
        var = res.weights[R._slice(off, pre + "_bn3")]
        assert np.all(var > 0) and np.max(np.abs(var - 1.0)) > 1e-3, pre
    # arena: slot 0 the old (best) model, slot 1 the new one
    a = Trainer(64, "", 9, 50, 16, 1.0, 0.25, 0, 1, True, stagger=False)
    a.set_net(NET_RESCNN4_H3, w0, slot=0)
    a.set_net(NET_RESCNN4_H3, res.best_weights, slot=1)
    assert a.run()
    assert 0.0 <= a.score() <= 1.0


class _FitterOfCreate(Fitter):
    """a fitter made by ca_fitter_create, the entry point that has no net argument"""

    def __init__(self, max_batch, device=0):
        self.net, self.num_weights = NET_MLP12X100, nets.MLP_NUM_WEIGHTS
        self._L = _lib.load()
        self._h = C.c_void_p()
        self.max_batch = int(max_batch)
        _lib.check(self._L, self._L.ca_fitter_create(int(device), self.max_batch, C.byref(self._h)))


def test_mlp_fit_is_the_same_through_both_entry_points():
    s, z, p = fit_ref.synthetic_samples(3000, 13)
    w = nets.init_mlp12x100(6, bn_noise=True)
    a = fit(w, s, z, p, batch_size=512, epochs=2, seed=3, net=NET_MLP12X100)
    with _FitterOfCreate(512) as be:
        b = fit(w, s, z, p, batch_size=512, epochs=2, seed=3, _backend=be)
    assert a.weights.tobytes() == b.weights.tobytes() and a.best_weights.tobytes() == b.best_weights.tobytes()
    for x, y in zip(a.optimizer[:2], b.optimizer[:2]):
        assert x.tobytes() == y.tobytes()
    assert a.history == b.history and a.optimizer[2] == b.optimizer[2]
    L = _lib.load()
    h = C.c_void_p()
    assert L.ca_fitter_create_net(0, 7, 16, C.byref(h)) == -1 and not h  # CA_ERR_ARG: neither trainable network
    with pytest.raises(ValueError):
        Fitter(16, net=NET_RESCNN4_H3)
