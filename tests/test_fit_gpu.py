"""Network training on the MI355X (csrc/nn_train.hip and nn_train_mlp.hip through corintho_ai_amd.fit) against the
float64 restatement of the Keras step (tests/fit_ref.py); the tests that are the same for both networks run here for
rescnn4 too (tests/fit_ref_rescnn4.py).  The rule of tests/test_net_precision.py: the device's error against float64 is at most
4 x the float32 restatement's own error against float64, plus a small floor."""
import numpy as np
import pytest

from corintho_ai_amd import NET_MLP12X100, NET_RESCNN4, Trainer, nets, samples_io
from corintho_ai_amd.fit import Fitter, fit, net_info, split_index
from tests import fit_ref as R
from tests import fit_ref_rescnn4
from tests import fit_ref_step as S
from tests.fit_ref_step import within as _within

pytestmark = pytest.mark.gpu

WEIGHTS = [("init", lambda: nets.init_mlp12x100(0)), ("bn-noise", lambda: nets.init_mlp12x100(7, bn_noise=True)),
           ("trained-like", lambda: nets.trained_like_mlp12x100(1))]
# the tests both networks share: network kind, init function, reference module
NET_CASES = [(NET_MLP12X100, nets.init_mlp12x100, R), (NET_RESCNN4, nets.init_rescnn4, fit_ref_rescnn4)]
NETS = pytest.mark.parametrize("kind,init,ref", NET_CASES, ids=[net_info(c[0])[0] for c in NET_CASES])


def _tensors():
    """(name, slice) of every trainable tensor of the layout"""
    lay, (kv, bv, kp, bp) = R.layer_offsets()
    out = []
    for i, (k, b, g, be, _, _, fi) in enumerate(lay):
        out += [("k%d" % i, slice(k, k + fi * 100)), ("b%d" % i, slice(b, b + 100)), ("gamma%d" % i, slice(g, g + 100)),
                ("beta%d" % i, slice(be, be + 100))]
    return out + [("kv", slice(kv, kv + 100)), ("bv", slice(bv, bv + 1)), ("kp", slice(kp, kp + 9600)),
                  ("bp", slice(bp, bp + 96))]


@pytest.fixture(scope="module")
def selfplay():
    t = Trainer(64, "", 21, 50, 16, 1.0, 0.25, 0, 1, False, stagger=False)
    t.set_net(NET_MLP12X100, nets.init_mlp12x100(3))
    assert t.run()
    s, z, p = samples_io.get_samples(t)
    assert s.shape[0] >= 2048
    return s, z, p


def test_gradients_of_one_batch(selfplay):
    """every trainable tensor within 4 x the float32 restatement's error (plus 2e-5 of the tensor's largest entry); a
    batch with a pre-activation within 2e-7 (of its layer's largest) of a ReLU kink is held to 5 % of the tensor's largest entry instead"""
    synth = R.synthetic_samples(4096, 11)
    bad, cases, kinked = [], 0, 0
    with Fitter(max_batch=2048) as f:
        for src_name, data in (("selfplay", selfplay), ("synthetic", synth)):
            f.set_data(*data)
            rng = np.random.default_rng(3)
            for wname, make in WEIGHTS:
                w = make()
                f.set_weights(w)
                for B in (1, 127, 128, 129, 2048):
                    rows = rng.choice(data[0].shape[0], B, replace=False).astype(np.int32)
                    g, losses = f.gradients(rows)
                    s, z, p = (a[rows] for a in data)
                    g64, l64, _ = S.loss_and_grad(R, w, s, z, p)
                    g32, l32, _ = S.loss_and_grad(R, w, s, z, p, dtype=R.torch.float32)
                    assert not g[R.stat_mask()].any(), "gradient at a moving statistic"
                    kink = S.kink_margin(R, w, s) < 2e-7
                    cases += 1
                    kinked += kink
                    for name, sl in _tensors():
                        top = float(np.max(np.abs(g64[sl])))
                        ok, ed, e3 = _within(g[sl], g32[sl], g64[sl], 2e-5 * top + 1e-12)
                        if kink:
                            ok = ed <= 0.05 * top + 1e-12
                        if not ok:
                            bad.append((src_name, wname, B, name, kink, ed, e3, top))
                    ok, ed, e3 = _within(losses, l32, l64, 1e-6 * abs(l64[0]))
                    if not ok:
                        bad.append((src_name, wname, B, "losses", ed, e3))
    assert not bad, "device error above 4 x float32's: %s" % bad[:12]
    assert kinked <= cases // 4, (kinked, cases)


@NETS
def test_twenty_adam_steps(kind, init, ref):
    """batch losses, moving statistics and held-out inference outputs after 20 steps of 256 rows (raw weights are not
    compared: Adam's first steps are close to lr * sign(g) and amplify the smallest gradient differences)"""
    s, z, p = ref.synthetic_samples(5120 + 512, 12)
    w = init(5, bn_noise=True)
    rows = np.random.default_rng(4).permutation(5120).astype(np.int32)
    zeros = np.zeros_like(w)
    with Fitter(max_batch=256, net=kind) as f:
        f.set_data(s, z, p)
        f.set_weights(w)
        f.set_optimizer(zeros, zeros, 0)
        _, per = f.train(rows, 256, 1e-3, batch_losses=True)
        wd = f.get_weights()
        _, _, it = f.get_optimizer()
    assert it == 20
    refs = {}
    for dt in (ref.torch.float64, ref.torch.float32):
        be = S.RefBackend(ref.NET, dt)
        be.set_weights(w)
        be.set_optimizer(zeros, zeros, 0)
        be.set_data(s, z, p)
        _, pr = be.train(rows, 256, 1e-3, batch_losses=True)
        refs[dt] = (pr, be.w.astype(np.float64))
    (p64, w64), (p32, w32) = refs[ref.torch.float64], refs[ref.torch.float32]
    ok, ed, e3 = _within(per, p32, p64, 1e-6)
    print("batch losses dev %.3e f32 %.3e" % (ed, e3))
    assert ok, ("batch losses", ed, e3)
    mask = ref.stat_mask()
    ok, ed, e3 = _within(wd[mask], w32[mask], w64[mask], 1e-6)
    print("moving statistics dev %.3e f32 %.3e" % (ed, e3))
    assert ok, ("moving statistics", ed, e3)
    held = slice(5120, 5632)
    out64 = S.evaluate(ref, w64, s[held], z[held], p[held])[1]
    out32 = S.evaluate(ref, w32, s[held], z[held], p[held])[1]
    outd = S.evaluate(ref, wd.astype(np.float64), s[held], z[held], p[held])[1]
    for k, name in enumerate(("value", "policy")):
        ok, ed, e3 = _within(outd[k], out32[k], out64[k], 1e-6)
        print("%s dev %.3e f32 %.3e" % (name, ed, e3))
        assert ok, (name, ed, e3)


@NETS
def test_set_get_round_trip(kind, init, ref):
    name = net_info(kind)[0]
    w = getattr(nets, "trained_like_" + name)(2)
    rng = np.random.default_rng(1)
    m = rng.normal(0, 1e-3, w.size).astype(np.float32)
    v = rng.uniform(0, 1e-6, w.size).astype(np.float32)
    other = nets.init_rescnn4 if kind == NET_MLP12X100 else nets.init_mlp12x100
    with Fitter(max_batch=16, net=kind) as f:
        f.set_weights(w)
        f.set_optimizer(m, v, 1234)
        assert f.get_weights().tobytes() == w.tobytes()
        m2, v2, it = f.get_optimizer()
        assert m2.tobytes() == m.tobytes() and v2.tobytes() == v.tobytes() and it == 1234
        with pytest.raises(Exception):
            f.set_weights(other(0))  # the other network's size


@NETS
def test_two_fits_are_bitwise_identical(kind, init, ref):
    s, z, p = ref.synthetic_samples(3000, 13)
    w = init(6, bn_noise=True)
    a = fit(w, s, z, p, batch_size=512, epochs=2, seed=3, net=kind)
    b = fit(w, s, z, p, batch_size=512, epochs=2, seed=3, net=kind)
    assert a.weights.tobytes() == b.weights.tobytes() and a.best_weights.tobytes() == b.best_weights.tobytes()
    for x, y in zip(a.optimizer[:2], b.optimizer[:2]):
        assert x.tobytes() == y.tobytes()
    for x, y in zip(a.best_optimizer[:2], b.best_optimizer[:2]):
        assert x.tobytes() == y.tobytes()
    assert a.optimizer[2] == b.optimizer[2] == 2 * -(-split_index(3000, 0.3) // 512)
    assert a.history == b.history
    assert a.weights.tobytes() != w.tobytes()
    mask = ref.stat_mask()
    assert not a.optimizer[0][mask].any() and not a.optimizer[1][mask].any()


def _two_calls(fitters):
    """two train() calls of 40 rows at batch 17 (batches of 17, 17 and 6 rows: a full 16-row tile plus one row, and a
    partial tile) on every fitter in turn; per fitter the bytes of the weights, m, v and both calls' per-batch losses,
    and the iterations"""
    per = [[] for _ in fitters]
    for call in range(2):
        rows = np.random.default_rng(20 + call).permutation(64)[:40].astype(np.int32)
        for k, f in enumerate(fitters):
            per[k].append(f.train(rows, 17, 1e-3, batch_losses=True)[1])
    out = []
    for k, f in enumerate(fitters):
        m, v, it = f.get_optimizer()
        out.append(([a.tobytes() for a in [f.get_weights(), m, v] + per[k]], it))
    return out


def test_two_networks_side_by_side():
    """no state is shared between fitter objects: an MLP fitter and a rescnn4 fitter trained alternately in one process
    end, byte for byte, where each ends when trained alone in a fresh fitter with the same calls"""
    def start(kind, init, ref):
        f = Fitter(max_batch=17, net=kind)
        f.set_data(*ref.synthetic_samples(64, 14))
        w = init(8, bn_noise=True)
        f.set_weights(w)
        f.set_optimizer(np.zeros_like(w), np.zeros_like(w), 0)
        return f

    both = [start(*q) for q in NET_CASES]
    together = _two_calls(both)
    for f in both:
        f.close()
    for q, side in zip(NET_CASES, together):
        with start(*q) as f:
            (alone,) = _two_calls([f])
        assert side[1] == alone[1] == 6, (q[0], side[1], alone[1])
        for name, x, y in zip(("weights", "m", "v", "losses of call 0", "losses of call 1"), side[0], alone[0]):
            assert x == y, (q[0], name)
        assert side[0][0] != q[1](8, bn_noise=True).tobytes()


def test_whole_loop_small(tmp_path):
    """a TF-free generation: fused self-play -> samples_for_training -> fit -> arena of the new weights against the old"""
    w0 = nets.init_mlp12x100(0)
    t = Trainer(256, "", 5, 100, 16, 1.0, 0.25, 0, 1, False, stagger=False)
    t.set_net(NET_MLP12X100, w0)
    assert t.run()
    s, z, p = samples_io.samples_for_training(t, str(tmp_path / "gen_0"))
    res = fit(w0, s, z, p, batch_size=512, epochs=3)
    n = s.shape[0]
    split = split_index(n, 0.3)
    with Fitter(max_batch=512) as f:
        f.set_data(s, z, p)
        f.set_weights(w0)
        start = f.evaluate(split, n - split, 512)[0]
    vals = res.history["val_loss"]
    assert min(vals) < start, (vals, start)
    assert res.best_epoch == int(np.argmin(vals))
    # the engine's network on the fitted weights gives the fitter's val_loss
    e = Trainer(64, "", 1, 50, 16, 1.0, 0.25, 0, 1, False)
    e.set_net(NET_MLP12X100, res.best_weights)
    cap = 64 * 16  # rows one evaluation of this trainer takes
    parts = [e.net_forward(s[i:i + cap]) for i in range(split, n, cap)]
    ev, pr = np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts])
    lv = np.mean((ev.astype(np.float64) - z[split:]) ** 2)
    t_ = p[split:].astype(np.float64)
    lp = np.mean(-(np.where(t_ > 0, t_ * np.log(np.maximum(pr.astype(np.float64), 1e-300)), 0.0)).sum(1))
    assert abs((lv + 0.25 * lp) - vals[res.best_epoch]) <= 1e-5 * vals[res.best_epoch]
    # arena: slot 0 the old (best) model, slot 1 the new one
    a = Trainer(64, "", 9, 50, 16, 1.0, 0.25, 0, 1, True, stagger=False)
    a.set_net(NET_MLP12X100, w0, slot=0)
    a.set_net(NET_MLP12X100, res.best_weights, slot=1)
    assert a.run()
    assert 0.0 <= a.score() <= 1.0
