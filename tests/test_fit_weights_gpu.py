"""Per-sample weights in the fitter on the MI355X (csrc/nn_train_loss.hip ft_k_loss<true>,
csrc/nn_train_data.hip ft_k_assemble<true>; Keras's model.fit(sample_weight=...)), for both networks.  Weights of 1 and of 2 are compared by bytes (a multiply by 1 changes
no bit, a power of two scales exactly through the linear backward pass); general weights go against the float64
restatement of tests/fit_ref_weighted.py by the rule of tests/test_fit_gpu.py::test_gradients_of_one_batch: the
device's error is at most 4 x the float32 restatement's own error, plus 2e-5 of the tensor's largest entry."""
import numpy as np
import pytest

from corintho_ai_amd import NET_MLP12X100, NET_RESCNN4, expand_samples, nets
from corintho_ai_amd.fit import Fitter, fit, fit_samples, net_info
from tests import fit_ref, fit_ref_rescnn4
from tests import fit_ref_weighted as RW
from tests.fit_ref_step import within as _within

pytestmark = pytest.mark.gpu

NET_CASES = [(NET_MLP12X100, nets.init_mlp12x100, fit_ref), (NET_RESCNN4, nets.init_rescnn4, fit_ref_rescnn4)]
NETS = pytest.mark.parametrize("kind,init,ref", NET_CASES, ids=[net_info(c[0])[0] for c in NET_CASES])
KINK = 2e-7


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def synthetic40():
    """per network: 40 un-augmented samples (states | policies, outcomes) and their host expansion (320 rows)"""
    out = {}
    for kind, _, ref in NET_CASES:
        s, z, p = ref.synthetic_samples(40, 23)
        sp = np.concatenate([s, p], axis=1).astype(np.float32)
        out[kind] = (sp, z, expand_samples(sp, z))
    return out


def _general_weights(n, seed):
    """weights in [0, 3] with exact zeros among them"""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.0, 3.0, n).astype(np.float32)
    w[rng.choice(n, max(1, n // 8), replace=False)] = 0.0
    return w


def _open(kind, form, data, max_batch, weights=None):
    """a fitter that holds the 40 samples packed, or their 320 rows expanded; weights are per sample"""
    sp, oc, ex = data
    f = Fitter(max_batch=max_batch, net=kind)
    if form == "packed":
        f.add_samples(sp, oc)
        if weights is not None:
            f.set_sample_weights(weights)
    else:
        f.set_data(*ex)
        if weights is not None:
            f.set_sample_weights(np.repeat(weights, 8))
    return f


def _run(f, w):
    """gradients of three batches, then two epochs at batch 17 and a validation pass: everything a fit reads"""
    zeros = np.zeros_like(w)
    f.set_weights(w)
    f.set_optimizer(zeros, zeros, 0)
    rng = np.random.default_rng(9)
    grads = [f.gradients(rng.choice(320, B, replace=False).astype(np.int32)) for B in (1, 17, 129)]
    orders = [np.random.default_rng(s).permutation(224)[:200].astype(np.int32) for s in (1, 2)]
    per = [f.train(o, 17, 1e-3, batch_losses=True) for o in orders]
    val = f.evaluate(224, 96, 17)
    return grads, per, val, f.get_weights(), f.get_optimizer()


def _assert_runs_equal(a, b):
    for (ga, la), (gb, lb) in zip(a[0], b[0]):
        assert ga.any() and _same(ga, gb) and la == lb
    for (la, pa), (lb, pb) in zip(a[1], b[1]):
        assert la == lb and _same(pa, pb)
    assert a[2] == b[2]
    assert _same(a[3], b[3])
    assert _same(a[4][0], b[4][0]) and _same(a[4][1], b[4][1]) and a[4][2] == b[4][2] == 24


@NETS
@pytest.mark.parametrize("form", ["packed", "expanded"])
def test_weights_of_one_change_no_byte(kind, init, ref, form, synthetic40):
    """explicit weights of 1.0 (the weighted kernels) against no weights (the kernels of a set without weights)"""
    w = init(6, bn_noise=True)
    with _open(kind, form, synthetic40[kind], 129) as plain, \
            _open(kind, form, synthetic40[kind], 129, np.ones(40, np.float32)) as ones:
        assert _same(ones.get_sample_weights(), plain.get_sample_weights())
        a, b = _run(plain, w), _run(ones, w)
    _assert_runs_equal(a, b)
    assert not _same(a[3], w)


@NETS
@pytest.mark.parametrize("form", ["packed", "expanded"])
def test_weights_of_two_double_exactly(kind, init, ref, form, synthetic40):
    w = init(5, bn_noise=True)
    rng = np.random.default_rng(4)
    with _open(kind, form, synthetic40[kind], 129) as plain, \
            _open(kind, form, synthetic40[kind], 129, np.full(40, 2.0, np.float32)) as twos:
        for f in (plain, twos):
            f.set_weights(w)
        for B in (1, 17, 129):
            rows = rng.choice(320, B, replace=False).astype(np.int32)
            g1, l1 = plain.gradients(rows)
            g2, l2 = twos.gradients(rows)
            assert g1.any()
            assert _same(g2, np.float32(2.0) * g1), B
            assert l2 == tuple(2.0 * x for x in l1), B
        e1, e2 = plain.evaluate(3, 300, 17), twos.evaluate(3, 300, 17)
        assert e2 == tuple(2.0 * x for x in e1)


def _weights_of(kind):
    name = net_info(kind)[0]
    init = getattr(nets, "init_" + name)
    return [("init", init(0)), ("bn-noise", init(7, bn_noise=True)), ("trained-like", getattr(nets, "trained_like_" + name)(1))]


@NETS
def test_general_weights_against_float64(kind, init, ref):
    """weights in [0, 3] with an exact 0 in every batch of more than one row; B = 1, 17, 129.  Every trainable tensor's
    gradient and the three losses by the rule of test_gradients_of_one_batch; a batch with a ReLU input within 2e-7 of
    its kink is held to 5 % of the tensor's largest entry instead, and at most a quarter of the cases may be such.  At a
    kink the restatements themselves part ways (float32 and float64 take different sides, and a row of weight w carries
    w / mean(w) times an unweighted row's share: on one such draw the float32 restatement alone was 6 % off), so a
    batch whose float64 restatement sits at a kink is drawn again from the same generator, three times at the most,
    before the exception is used; the draw never looks at the device.  The row of weight 0 counts in the BatchNorm
    statistics: the float64 gradient of the batch without it is far away."""
    data = ref.synthetic_samples(1024, 11)
    sw = _general_weights(1024, 2)
    zero_rows = np.flatnonzero(sw == 0.0)
    bad, cases, kinked = [], 0, 0
    rng = np.random.default_rng(3)
    with Fitter(max_batch=129, net=kind) as f:
        f.set_data(*data)
        f.set_sample_weights(sw)
        for wname, w in _weights_of(kind):
            f.set_weights(w)
            for B in (1, 17, 129):
                for draw in range(4):  # (see the docstring: the margin is the float64 restatement's, not the device's)
                    rows = rng.choice(np.flatnonzero(sw > 0.0), B, replace=False).astype(np.int32)
                    if B > 1:
                        rows[B // 2] = zero_rows[cases % zero_rows.size]
                    if RW.kink_margin(ref, w, data[0][rows]) >= KINK:
                        break
                g, losses = f.gradients(rows)
                s, z, p = (a[rows] for a in data)
                g64, l64 = RW.loss_and_grad(ref, w, s, z, p, sw[rows])
                g32, l32 = RW.loss_and_grad(ref, w, s, z, p, sw[rows], dtype=ref.torch.float32)
                assert not g[ref.stat_mask()].any(), "gradient at a moving statistic"
                kink = RW.kink_margin(ref, w, s) < KINK
                cases += 1
                kinked += kink
                tag = "%s B=%d" % (wname, B)
                for name, sl, scale in RW.tensors(ref):
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
                if B == 17 and not kink:
                    live = np.delete(np.arange(B), B // 2)
                    gd, _ = RW.loss_and_grad(ref, w, s[live], z[live], p[live], sw[rows][live])
                    gd *= (B - 1) / B  # the divisor stays B
                    far = float(np.max(np.abs(gd - g64)))
                    near = float(np.max(np.abs(g.astype(np.float64) - g64)))
                    print("%s without the zero-weight row: %.3e away, the device %.3e" % (tag, far, near))
                    assert far > 100.0 * near, (tag, far, near)
    assert not bad, "device error above 4 x float32's: %s" % bad[:12]
    assert cases == 9 and kinked <= cases // 4, (kinked, cases)


@NETS
def test_evaluate_with_weights(kind, init, ref):
    """the validation pass (moving statistics) of 300 weighted rows in batches of 129 (the last one partial)"""
    data = ref.synthetic_samples(512, 12)
    sw = _general_weights(512, 5)
    w = getattr(nets, "trained_like_" + net_info(kind)[0])(2)
    with Fitter(max_batch=129, net=kind) as f:
        f.set_data(*data)
        f.set_sample_weights(sw)
        f.set_weights(w)
        got = f.evaluate(100, 300, 129)
    want = {}
    for dt in (ref.torch.float64, ref.torch.float32):
        tot = np.zeros(3)
        for b0 in range(100, 400, 129):
            b1 = min(b0 + 129, 400)
            tot += np.asarray(RW.evaluate(ref, w, data[0][b0:b1], data[1][b0:b1], data[2][b0:b1], sw[b0:b1], dt)) * (b1 - b0)
        want[dt] = tot / 300
    ok, ed, e3 = _within(got, want[ref.torch.float32], want[ref.torch.float64], 1e-6 * abs(want[ref.torch.float64][0]))
    print("weighted evaluate dev %.3e f32 %.3e" % (ed, e3))
    assert ok, (ed, e3)
    assert got[0] > 0.0


@NETS
def test_packed_weights_equal_expanded_weights_repeated(kind, init, ref, synthetic40):
    """a packed set with one weight per sample is the expanded set with each weight 8 times: the rows fetched, the
    gradients, two epochs and a validation pass, byte for byte; fit_samples and fit with sample_weight agree likewise"""
    sw = _general_weights(40, 8)
    w = init(6, bn_noise=True)
    with _open(kind, "packed", synthetic40[kind], 129, sw) as packed, \
            _open(kind, "expanded", synthetic40[kind], 129, sw) as expanded:
        assert _same(np.repeat(packed.get_sample_weights(), 8), expanded.get_sample_weights())
        rows = np.random.default_rng(5).integers(0, 320, 57).astype(np.int32)
        for x, y in zip(packed.fetch_rows(rows), expanded.fetch_rows(rows)):
            assert _same(x, y)
        a, b = _run(packed, w), _run(expanded, w)
    _assert_runs_equal(a, b)
    sp, oc, ex = synthetic40[kind]
    ra = fit_samples(w, sp, oc, sample_weight=sw, batch_size=17, epochs=2, seed=3, net=kind)
    rb = fit(w, *ex, sample_weight=np.repeat(sw, 8), batch_size=17, epochs=2, seed=3, net=kind)
    rc = fit_samples(w, sp, oc, batch_size=17, epochs=2, seed=3, net=kind)
    assert ra.history == rb.history and _same(ra.weights, rb.weights) and _same(ra.optimizer[1], rb.optimizer[1])
    assert ra.history != rc.history


def test_weights_move_with_their_samples_and_bad_ones_are_refused(synthetic40):
    sp, oc, ex = synthetic40[NET_MLP12X100]
    sw = _general_weights(40, 9)
    w = nets.init_mlp12x100(3, bn_noise=True)
    rows = np.arange(0, 200, 3, dtype=np.int32)
    with Fitter(max_batch=129) as f, Fitter(max_batch=129) as tail:
        with pytest.raises(Exception):
            f.set_sample_weights(np.ones(1, np.float32))  # no data
        f.add_samples(sp, oc)
        f.set_weights(w)
        plain = f.gradients(rows)
        f.set_sample_weights(sw)
        before = f.gradients(rows)
        assert not _same(before[0], plain[0])
        for wrong in (sw[:39], np.ones(320, np.float32), np.where(np.arange(40) == 7, -1.0, sw),
                      np.where(np.arange(40) == 7, np.nan, sw), np.where(np.arange(40) == 7, np.inf, sw)):
            with pytest.raises(Exception):
                f.set_sample_weights(wrong.astype(np.float32))
            assert _same(f.get_sample_weights(), sw) and f.data_info() == (320, 40)
        after = f.gradients(rows)
        assert _same(before[0], after[0]) and before[1] == after[1]
        with pytest.raises(Exception, match="clear_data first"):
            f.add_samples(sp[:3], oc[:3])  # a set that carries weights takes no more samples
        assert f.data_info() == (320, 40)
        # the 13 oldest samples leave: what stays keeps its weight
        f.drop_samples(13)
        assert f.data_info() == (216, 27) and _same(f.get_sample_weights(), sw[13:])
        tail.add_samples(sp[13:], oc[13:])
        tail.set_sample_weights(sw[13:])
        tail.set_weights(w)
        ga, gb = f.gradients(rows), tail.gradients(rows)
        assert _same(ga[0], gb[0]) and ga[1] == gb[1]
        # no weights again: the unweighted kernels, and samples may be added
        f.set_sample_weights(None)
        assert _same(f.get_sample_weights(), np.ones(27, np.float32))
        f.add_samples(sp[:13], oc[:13])
        assert f.data_info() == (320, 40)
        f.clear_data()
        f.add_samples(sp, oc)
        again = f.gradients(rows)
        assert _same(again[0], plain[0]) and again[1] == plain[1]
