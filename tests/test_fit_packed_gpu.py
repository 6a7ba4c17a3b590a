"""The fitter's packed data set on the MI355X (csrc/nn_train_data.hip ft_k_assemble, corintho_ai_amd.fit): un-augmented
samples on the device whose 8 n virtual rows -- row v is sample v // 8 under symmetry v % 8 -- must be, float for float,
the rows of the host expansion (`expand_samples`, the host routine ca_expand_samples).  Everything downstream of the
batch gather is the same code launched the same way, so every comparison between the two forms here is of bytes."""
import numpy as np
import pytest

from corintho_ai_amd import NET_MLP12X100, NET_RESCNN4, Trainer, _lib, expand_samples, nets, samples_io
from corintho_ai_amd.fit import Fitter, fit, fit_samples, fit_trainer, net_info
from tests import fit_ref, fit_ref_rescnn4

pytestmark = pytest.mark.gpu

NET_CASES = [(NET_MLP12X100, nets.init_mlp12x100, fit_ref), (NET_RESCNN4, nets.init_rescnn4, fit_ref_rescnn4)]
NETS = pytest.mark.parametrize("kind,init,ref", NET_CASES, ids=[net_info(c[0])[0] for c in NET_CASES])


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _same3(got, want):
    return all(_same(g, w) for g, w in zip(got, want))


def _distinct():
    """5 samples whose every cell is distinct and exact in float32: one wrong table entry shows"""
    sp = (256.0 * np.arange(5)[:, None] + np.arange(166)[None, :]).astype(np.float32)
    oc = (np.arange(5) - 2).astype(np.float32)
    return sp, oc


@pytest.fixture(scope="module")
def distinct():
    sp, oc = _distinct()
    return sp, oc, expand_samples(sp, oc)


def _row_lists():
    rng = np.random.default_rng(5)
    lists = [np.arange(40)] + [rng.integers(0, 40, k) for k in (1, 17, 40)] + [np.arange(32, 40)]
    return [r.astype(np.int32) for r in lists]


@pytest.fixture(scope="module")
def synthetic40():
    """per network: 40 un-augmented samples (states | policies, outcomes) and their host expansion"""
    out = {}
    for kind, _, ref in NET_CASES:
        s, z, p = ref.synthetic_samples(40, 23)
        sp = np.concatenate([s, p], axis=1).astype(np.float32)
        out[kind] = (sp, z, expand_samples(sp, z))
    return out


def test_gather_alone(distinct):
    sp, oc, want = distinct
    with Fitter(max_batch=16) as packed, Fitter(max_batch=16) as expanded:
        packed.clear_data()
        packed.add_samples(sp, oc)
        assert packed.data_info() == (40, 5)
        expanded.set_data(*want)
        assert expanded.data_info() == (40, 0)
        for rows in _row_lists():
            exp = tuple(a[rows] for a in want)
            assert _same3(packed.fetch_rows(rows), exp), rows
            assert _same3(expanded.fetch_rows(rows), exp), rows


@NETS
def test_gradients(kind, init, ref, synthetic40):
    sp, oc, ex = synthetic40[kind]
    w = init(5, bn_noise=True)
    rng = np.random.default_rng(9)
    with Fitter(max_batch=129, net=kind) as packed, Fitter(max_batch=129, net=kind) as expanded:
        packed.add_samples(sp, oc)
        expanded.set_data(*ex)
        for f in (packed, expanded):
            f.set_weights(w)
        for B in (1, 17, 129):
            rows = rng.choice(320, B, replace=False).astype(np.int32)
            gp, lp = packed.gradients(rows)
            ge, le = expanded.gradients(rows)
            assert gp.any()
            assert _same(gp, ge), B
            assert lp == le, B


@NETS
def test_two_epochs(kind, init, ref, synthetic40):
    sp, oc, ex = synthetic40[kind]
    w = init(6, bn_noise=True)
    zeros = np.zeros_like(w)
    orders = [np.random.default_rng(s).permutation(224)[:200].astype(np.int32) for s in (1, 2)]
    got = []
    for form in ("packed", "expanded"):
        with Fitter(max_batch=17, net=kind) as f:
            if form == "packed":
                f.add_samples(sp, oc)
            else:
                f.set_data(*ex)
            f.set_weights(w)
            f.set_optimizer(zeros, zeros, 0)
            per = [f.train(o, 17, 1e-3, batch_losses=True) for o in orders]
            val = f.evaluate(224, 96, 17)
            got.append((f.get_weights(), f.get_optimizer(), per, val))
    (wp, (mp, vp, ip), pp, valp), (we, (me, ve, ie), pe, vale) = got
    assert ip == ie == 2 * 12
    assert not _same(wp, w)
    assert _same(wp, we) and _same(mp, me) and _same(vp, ve)
    for (lp, bp), (le, be) in zip(pp, pe):
        assert lp == le
        assert bp.shape == (12, 3) and _same(bp, be)
    assert valp == vale


def _same_result(a, b):
    assert a.history == b.history
    assert a.best_epoch == b.best_epoch
    assert _same(a.best_weights, b.best_weights) and _same(a.weights, b.weights)
    for x, y in ((a.best_optimizer, b.best_optimizer), (a.optimizer, b.optimizer)):
        assert _same(x[0], y[0]) and _same(x[1], y[1]) and x[2] == y[2]
    assert a.learning_rate == b.learning_rate


@NETS
def test_fit_samples_against_fit(kind, init, ref):
    s, z, p = ref.synthetic_samples(375, 31)
    sp = np.concatenate([s, p], axis=1).astype(np.float32)
    w = init(2, bn_noise=True)
    a = fit_samples(w, sp, z, batch_size=512, epochs=2, seed=4, net=kind)
    b = fit(w, *expand_samples(sp, z), batch_size=512, epochs=2, seed=4, net=kind)
    assert len(a.history["loss"]) == 2
    _same_result(a, b)


def test_from_a_trainer():
    w = nets.init_mlp12x100(3)
    t = Trainer(64, "", 21, 50, 16, 1.0, 0.25, 0, 1, False, stagger=False)
    t.set_net(NET_MLP12X100, w)
    assert t.run()
    first = samples_io.get_samples(t)
    n1 = t.num_samples()
    assert n1 > 0
    with Fitter(max_batch=256) as f:
        assert f.add_trainer_samples(t) == n1
        assert f.data_info() == (8 * n1, n1)
        assert _same3(f.fetch_rows(np.arange(8 * n1)), first)
        by_trainer = fit_trainer(w, t, batch_size=512, epochs=1)
        t.reset(22)
        assert t.run()
        second = samples_io.get_samples(t)
        n2 = t.num_samples()
        assert not _same(first[0], second[0])
        assert f.add_trainer_samples(t) == n2
        assert f.data_info() == (8 * (n1 + n2), n1 + n2)
        both = tuple(np.concatenate([a, b]) for a, b in zip(first, second))
        assert _same3(f.fetch_rows(np.arange(8 * (n1 + n2))), both)
        f.drop_samples(n1)
        assert f.data_info() == (8 * n2, n2)
        assert _same3(f.fetch_rows(np.arange(8 * n2)), second)
    _same_result(by_trainer, fit(w, *first, batch_size=512, epochs=1))


def test_from_device_memory(distinct):
    import torch

    sp, oc, want = distinct
    d_sp, d_oc = torch.from_numpy(sp).cuda(), torch.from_numpy(oc).cuda()
    torch.cuda.synchronize()
    with Fitter(max_batch=64) as f:
        f.add_device_samples(d_sp.data_ptr(), d_oc.data_ptr(), 5)
        assert f.data_info() == (40, 5)
        assert _same3(f.fetch_rows(np.arange(40)), want)
        f.add_device_samples(d_sp.data_ptr(), d_oc.data_ptr(), 5)
        assert f.data_info() == (80, 10)
        assert _same3(f.fetch_rows(np.arange(40, 80)), want)
        assert _same3(f.fetch_rows(np.arange(40)), want)


def test_window_slides_in_place():
    """drop_samples by each of its roads: a sliver (through new buffers), pieces of the dropped length copied forward
    within the buffer, and one piece; what stays is what stayed, in order, and appending goes on behind it"""
    n = 200
    sp = (256.0 * np.arange(n)[:, None] + np.arange(166)[None, :]).astype(np.float32)
    oc = (np.arange(n) % 3 - 1).astype(np.float32)
    want = expand_samples(sp, oc)
    lo = 0
    with Fitter(max_batch=256) as f:
        f.add_samples(sp, oc)
        for drop in (1, 50, 100, 0):
            f.drop_samples(drop)
            lo += drop
            assert f.data_info() == (8 * (n - lo), n - lo)
            assert _same3(f.fetch_rows(np.arange(8 * (n - lo))), tuple(a[8 * lo:] for a in want)), drop
        f.add_samples(sp[:7], oc[:7])
        got = f.fetch_rows(np.arange(8 * (n - lo + 7)))
        assert _same3(got, tuple(np.concatenate([a[8 * lo:], a[:56]]) for a in want))
        f.drop_samples(n - lo + 7)
        assert f.data_info() == (0, 0)


def _refused(code, text, call):
    """`call` raises the engine's error `code`, and ca_last_error says `text`"""
    with pytest.raises(_lib.EngineError, match="error %d: .*%s" % (code, text)):
        call()
    assert text in _lib.load().ca_last_error().decode()


def test_errors(distinct):
    sp, oc, want = distinct
    rows = np.arange(8, dtype=np.int32)
    with Fitter(max_batch=16) as f:
        f.set_data(*want)
        _refused(-4, "expanded", lambda: f.add_samples(sp, oc))
        f.clear_data()
        assert f.data_info() == (0, 0)
        _refused(-4, "no data", lambda: f.train(rows, 8, 1e-3))
        f.add_samples(sp, oc)
        f.gradients(np.array([39], np.int32))
        _refused(-1, "out of range", lambda: f.gradients(np.array([40], np.int32)))
        _refused(-1, "out of range", lambda: f.train(np.array([0, 40], np.int32), 2, 1e-3))
        _refused(-1, "out of range", lambda: f.fetch_rows([40]))
        _refused(-1, "more than the set holds", lambda: f.drop_samples(6))
        arena = Trainer(4, "", 1, 8, 4, 1.0, 0.25, 0, 1, True)
        _refused(-4, "testing mode", lambda: f.add_trainer_samples(arena))
        arena.close()
        import ctypes as C

        assert _lib.load().ca_trainer_device(None, C.byref(C.c_int32())) == -1  # a null handle is an error, not a crash
        assert f.data_info() == (40, 5)  # a refused call changes nothing
        assert _same3(f.fetch_rows(np.arange(40)), want)
