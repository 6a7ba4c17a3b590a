"""Adam's arguments on the MI355X (csrc/nn_train_opt.hip ft_k_update_adam and ft_k_opt_update_adam, the
swap and apply kernels; include/corintho_hip.h, "Adam's arguments").  With every argument at its default a step is what
it was; off the defaults the slots are what the definition says, judged from the device's own gradients() and pre-step
state pushed through tests/fit_ref_adam.py: m', v', h' and a' are sums, differences, products and a maximum only, so the
float32 restatement gives their bits; w'' goes through a root and a quotient and is held to the float64 restatement
within 2^-24 |w| + 8 * 2^-24 |lr_t m' / (sqrt d + eps)|, eight float32 roundings on the step term.

Shapes: both networks, a packed set of 48 samples (384 virtual rows), batches of 64 and one partial batch of 37."""
import ctypes as C
import os

import numpy as np
import pytest

from corintho_ai_amd import NET_MLP12X100, NET_RESCNN4, AdamOptions, FitOptions, Run, nets, samples_io
from corintho_ai_amd import _lib
from corintho_ai_amd import run as R
from corintho_ai_amd.fit import Fitter, fit_resident, fit_samples, split_index
from tests import fit_ref
from tests import fit_ref_adam as A
from tests import fit_ref_options as O

pytestmark = pytest.mark.gpu

KINDS = {"mlp12x100": (NET_MLP12X100, nets.init_mlp12x100), "rescnn4": (NET_RESCNN4, nets.init_rescnn4)}
NETS = pytest.mark.parametrize("net", list(KINDS))
WITH_OPTIONS = pytest.mark.parametrize("options", [False, True], ids=["plain", "options"])
LR = 1e-3
ERR_ARG, ERR_STATE = -1, -4
OPTIONS = FitOptions(l2=1e-3, weight_decay=1e-2, global_clipnorm=0.05)
EVERYTHING = AdamOptions(beta_1=0.8, beta_2=0.99, epsilon=1e-5, amsgrad=True, ema_momentum=0.9, ema_overwrite_frequency=2)


def packed():
    s, z, p = fit_ref.synthetic_samples(48, 23)
    return np.concatenate([s, p], axis=1).astype(np.float32), z


def rows(n, seed=0):
    return np.random.default_rng(200 + seed).permutation(384)[:n].astype(np.int32)


class Ctx:
    """one fitter of `net` on the packed set, reused by the tests of this file: every use sets everything it relies on"""

    def __init__(self, net):
        self.net = net
        self.kind, init = KINDS[net]
        self.w = init(5, bn_noise=True)
        self.zeros = np.zeros_like(self.w)
        self.f = Fitter(max_batch=64, net=self.kind)
        self.f.add_samples(*packed())
        self.tr = O.trainable_mask(net)

    def start(self, adam=None, options=None, iterations=0, m=None, v=None):
        """the context's weights, an optimizer state (zeros unless given), no vhat, no average"""
        f = self.f
        f.set_options(options)
        f.set_adam(adam)
        f.set_weights(self.w)
        f.set_optimizer(self.zeros if m is None else m, self.zeros if v is None else v, iterations)
        return f


def state(f):
    """everything a step changes, read back: w, m, v, it, h and a (None while the average is invalid)"""
    m, v, it = f.get_optimizer()
    try:
        a = f.get_slot("average")
    except _lib.EngineError:
        a = None
    return dict(w=f.get_weights(), m=m, v=v, it=it, h=f.get_slot("vhat"), a=a)


def same(x, y, sl=slice(None)):
    return x[sl].tobytes() == y[sl].tobytes()


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


def restate(ctx, pre, g, adam, options, after_w=None, f=np.float32):
    """the step of the definition from the pre-step state `pre` and the device's data gradient g, on the trainable
    weights: steps 1 to 3 of the fit options (tests/fit_ref_options.py) in float32, as the device has them, then
    fit_ref_adam.adam_update in f"""
    w = pre["w"]
    if options is not None:
        g2 = O.clip(ctx.net, O.add_reg(ctx.net, g, w, options, np.float32), options, np.float32)[0]
        w1 = O.decay(ctx.net, w, LR, options, np.float32)
    else:
        g2, w1 = g, w
    tr = ctx.tr
    a = None if pre["a"] is None else pre["a"][tr]
    if adam.averaged() and a is None:
        a = w[tr]  # an invalid average starts as the pre-step weights
    return A.adam_update(w1[tr], pre["m"][tr], pre["v"][tr], pre["h"][tr], a, g2[tr], pre["it"], LR, adam, f,
                         None if after_w is None else after_w[tr])


def check_w(ctx, got_w, u64, what):
    """w'' against the float64 restatement within the bound of the module docstring; returns the largest share of it"""
    err = np.abs(got_w[ctx.tr].astype(np.float64) - u64["w2"])
    tol = 2.0 ** -24 * np.abs(u64["w2"]) + 8 * 2.0 ** -24 * np.abs(u64["step"])
    share = float(np.max(err / np.maximum(tol, 1e-300)))
    print("%s %s: w'' error / bound %.3f" % (ctx.net, what, share))
    assert np.all(err <= tol), (what, float(np.max(err - tol)))
    return share


# ---------------------------------------------------------------------------------------------------- 1. off is off
@NETS
@WITH_OPTIONS
def test_off_is_off(net, options):
    """a fitter that never saw set_adam, one set to the defaults and one set to other values and back: three steps (64,
    64 and 37 rows) give the same bytes"""
    kind, init = KINDS[net]
    w = init(5, bn_noise=True)
    o = OPTIONS if options else None
    outs = []
    for how in ("never", "default", "back"):
        with Fitter(max_batch=64, net=kind) as f:
            f.add_samples(*packed())
            f.set_options(o)
            if how == "default":
                f.set_adam(AdamOptions())
            if how == "back":
                f.set_adam(EVERYTHING)
                f.set_weights(w)
                f.set_optimizer(np.zeros_like(w), np.zeros_like(w), 0)
                f.train(rows(101, 1), 64, LR)
                f.set_adam(None)
                assert f.get_adam() == AdamOptions(beta_1=float(np.float32(0.9)), beta_2=float(np.float32(0.999)),
                                                   epsilon=float(np.float32(1e-7)))
            f.set_weights(w)
            f.set_optimizer(np.zeros_like(w), np.zeros_like(w), 0)
            losses, per = f.train(rows(165), 64, LR, batch_losses=True)
            m, v, it = f.get_optimizer()
            assert it == 3 and per.shape == (3, 3)
            if how != "back":  # neither slot was ever used
                assert not f.get_slot("vhat").any()
                assert _lib.load().ca_fitter_swap_average(f._h) == ERR_STATE
            outs.append([x.tobytes() for x in (f.get_weights(), m, v, per, np.asarray(losses))])
    for name, a, b, c in zip(("weights", "m", "v", "batch losses", "losses"), *outs):
        assert a == b == c, name
    assert outs[0][0] != w.tobytes()


# ---------------------------------------------------------------------------------------------------- 2. exact slots
def clipping_options(ctx, r):
    """l2, weight_decay and a global_clipnorm at half the norm of the regularised gradient of rows r: the step clips"""
    ctx.start()
    g0 = ctx.f.gradients(r)[0]
    gp = O.add_reg(ctx.net, g0, ctx.w, FitOptions(l2=1e-3), np.float32)
    return FitOptions(l2=1e-3, weight_decay=1e-2, global_clipnorm=0.5 * float(np.sqrt((gp[ctx.tr].astype(np.float64) ** 2).sum())))


def step_and_slots(ctx, f, ad, o, r):
    """gradients() on rows r, one step on them, and the four slots bit for bit against the float32 restatement fed with
    the device's own gradient and pre-step state (for a', with the device's own w'' as well) -> (pre, g, got)"""
    pre = state(f)
    g = f.gradients(r)[0]
    assert same(f.get_weights(), pre["w"])
    f.train(r, r.size, LR)
    got = state(f)
    tr = ctx.tr
    u = restate(ctx, pre, g, ad, o, after_w=got["w"])
    for k in ("m", "v", "h", "a"):
        if u[k] is not None:
            assert same(got[k][tr], u[k]), k
    for k in ("m", "v"):
        assert not got[k][~tr].any(), k
    if ad.averaged():
        assert same(got["a"], got["w"], ~tr)  # the average holds the moving statistics' new values
    return pre, g, got


@NETS
@WITH_OPTIONS
@pytest.mark.parametrize("B", [64, 37])
def test_exact_slots(ctx, options, B):
    """One step with non-default beta_1, beta_2 and epsilon, AMSGrad and the average.

    Twice.  From the state a first such step left, so that m, v, h and a are all in play: the four slots bit for bit.
    And from a zero m and v with a planted vhat and average: the slots again, and w'' against the float64 restatement.
    The bound's eight roundings are what a step from m = v = 0 can accumulate (m' = g'' c1 one, v' = g''^2 c2 two, of
    which the root keeps half, the root, the sum with epsilon, the product with lr_t and the quotient one each: six;
    1 - beta is exact for these betas), the case tests/test_fit_options_gpu.py has the bound from.  From a non-zero m the
    sum m + (g'' - m) c1 can cancel, and float32's own rounding of its terms is then not small against m': there the
    slots' bits are the check."""
    ad = AdamOptions(beta_1=0.8, beta_2=0.99, epsilon=1e-5, amsgrad=True, ema_momentum=0.9)
    r = rows(B, 3)
    o = clipping_options(ctx, r) if options else None
    what = "%s B=%d" % ("options" if options else "plain", B)
    f = ctx.start(ad, o)
    f.train(rows(B, 2), B, LR)
    assert f.get_optimizer()[2] == 1 and f.get_slot("vhat").any()
    pre, g, got = step_and_slots(ctx, f, ad, o, r)
    vhat = got["h"]  # of the size of v': planted below, the maximum takes both sides
    assert np.any(got["h"][ctx.tr] > got["v"][ctx.tr]) and np.any(got["h"][ctx.tr] == got["v"][ctx.tr])
    f = ctx.start(ad, o)
    f.set_slot("vhat", vhat * np.float32(0.5))
    f.set_slot("average", ctx.w * np.float32(1.5))
    pre, g, got = step_and_slots(ctx, f, ad, o, r)
    assert not pre["m"].any() and not pre["v"].any()
    assert np.any(got["h"][ctx.tr] > got["v"][ctx.tr]) and np.any(got["h"][ctx.tr] == got["v"][ctx.tr])
    check_w(ctx, got["w"], restate(ctx, pre, g, ad, o, f=np.float64), "exact slots " + what)
    if options:
        assert f.train_stats()["clipped_steps"] == 1


# ---------------------------------------------------------------------------------------------------- 3. AMSGrad
def state_after(ctx, adam, r, **kw):
    f = ctx.start(adam, **kw)
    f.train(r, r.size, LR)
    return state(f)


@NETS
def test_amsgrad(ctx):
    r = rows(64, 4)
    plain = state_after(ctx, None, r)
    # from a zero optimizer state max(0, v') = v': the bytes of the step without it
    f = ctx.start(AdamOptions(amsgrad=True))
    f.train(r, 64, LR)
    got = state(f)
    for k in ("w", "m", "v"):
        assert same(got[k], plain[k]), k
    assert same(got["h"], got["v"]) and got["a"] is None
    # a planted vhat of 1e6: it keeps its bytes, and the weight moves by lr_t m' / (1e3 + eps)
    ad = AdamOptions(amsgrad=True)
    planted = np.full(ctx.w.size, 1e6, np.float32)
    f = ctx.start(ad)
    f.set_slot("vhat", planted)
    pre, g, got = step_and_slots(ctx, f, ad, None, r)
    assert same(got["h"], planted) and same(got["m"], plain["m"]) and same(got["v"], plain["v"])
    check_w(ctx, got["w"], restate(ctx, pre, g, ad, None, f=np.float64), "planted vhat")
    moved = np.abs(got["w"][ctx.tr].astype(np.float64) - ctx.w[ctx.tr])
    assert np.max(moved) < 1e-6 < np.max(np.abs(plain["w"][ctx.tr].astype(np.float64) - ctx.w[ctx.tr]))
    # set_optimizer clears it
    f.set_optimizer(ctx.zeros, ctx.zeros, 0)
    assert not f.get_slot("vhat").any()


@NETS
@pytest.mark.parametrize("betas", [(0.0, 0.999), (0.9, 0.0), (0.0, 0.0)])
def test_zero_betas(ctx, betas):
    """beta_1 = 0 and beta_2 = 0 are legal values: the slots' bits from a non-zero optimizer state, and w'' from a zero
    one (test_exact_slots says why)"""
    ad = AdamOptions(beta_1=betas[0], beta_2=betas[1], amsgrad=True)
    first = state_after(ctx, None, rows(37, 5))
    r = rows(37, 6)
    f = ctx.start(ad, iterations=1, m=first["m"], v=first["v"])
    pre, g, got = step_and_slots(ctx, f, ad, None, r)
    assert pre["m"].any() and pre["it"] == 1
    if betas[0] == 0.0:  # 1 - 0^t = 1: lr_t has no first-moment correction
        assert float(A.lr_t(LR, 1, ad)) == float(np.float32(LR) * np.sqrt(np.float32(1) - np.power(np.float32(betas[1]), np.float32(2))))
    f = ctx.start(ad)
    pre, g, got = step_and_slots(ctx, f, ad, None, r)
    check_w(ctx, got["w"], restate(ctx, pre, g, ad, None, f=np.float64), "betas %s" % (betas,))


# ---------------------------------------------------------------------------------------------------- 4. average and overwrite
@NETS
def test_average_and_overwrite(ctx):
    L = _lib.load()
    ad = AdamOptions(ema_momentum=0.9, ema_overwrite_frequency=2)
    first = state_after(ctx, None, rows(64, 7))
    f = ctx.start(ad, iterations=7, m=first["m"], v=first["v"])
    tr = ctx.tr
    # no average yet: CA_ERR_STATE, and nothing changes
    a = np.zeros(ctx.w.size, np.float32)
    assert L.ca_fitter_get_slot(f._h, 1, a.ctypes.data_as(C.POINTER(C.c_float)), a.size) == ERR_STATE
    assert L.ca_fitter_swap_average(f._h) == ERR_STATE and L.ca_fitter_apply_average(f._h) == ERR_STATE
    assert same(f.get_weights(), ctx.w)
    for k, B in enumerate((64, 37, 64, 64, 37)):
        f.train(rows(B, 10 + k), B, LR)
        got = state(f)
        assert got["it"] == 8 + k
        assert same(got["a"], got["w"], ~tr)
        if got["it"] in (8, 10, 12):
            assert same(got["w"], got["a"]), got["it"]
        else:
            assert np.mean(got["w"][tr] != got["a"][tr]) > 0.5, got["it"]
    # swap twice is the identity; once exchanges the two
    before = state(f)
    f.swap_average()
    once = state(f)
    assert same(once["w"], before["a"]) and same(once["a"], before["w"])
    f.swap_average()
    twice = state(f)
    for k in ("w", "a", "m", "v"):
        assert same(twice[k], before[k]), k
    # apply: the trainable weights become the average, the rest stays
    planted = before["a"] + np.float32(1.0)
    f.set_slot("average", planted)
    f.apply_average()
    w = f.get_weights()
    assert same(w, planted, tr) and same(w, before["w"], ~tr)
    # an invalid average starts as the pre-step weights (a step that does not overwrite: 8 -> 9)
    f = ctx.start(ad, iterations=8, m=first["m"], v=first["v"])
    f.train(rows(37, 20), 37, LR)
    got = state(f)
    mom = np.float32(0.9)
    want = ctx.w[tr] + (got["w"][tr] - ctx.w[tr]) * (np.float32(1) - mom)
    assert same(got["a"][tr], want) and not same(got["a"], got["w"], tr)
    # set_weights makes it invalid again
    f.set_weights(ctx.w)
    assert L.ca_fitter_swap_average(f._h) == ERR_STATE


# ---------------------------------------------------------------------------------------------------- 5. one call, five calls
@NETS
def test_one_call_of_five_batches_is_five_single_calls(ctx):
    r = rows(4 * 64 + 37, 30)
    outs = []
    for pieces in ([r], [r[k:k + 64] for k in range(0, r.size, 64)]):
        f = ctx.start(EVERYTHING, OPTIONS, iterations=3)
        per = [f.train(x, 64, LR, batch_losses=True)[1] for x in pieces]
        st = state(f)
        assert st["it"] == 8
        outs.append([st[k].tobytes() for k in ("w", "m", "v", "h", "a")] + [np.concatenate(per).tobytes()])
    assert len(pieces) == 5 and pieces[-1].size == 37
    for name, x, y in zip(("w", "m", "v", "h", "a", "batch losses"), *outs):
        assert x == y, name
    # and it is none of the steps without Adam's arguments
    f = ctx.start(None, OPTIONS, iterations=3)
    f.train(r, 64, LR)
    assert f.get_weights().tobytes() != outs[0][0]


# ---------------------------------------------------------------------------------------------------- 6. reproducible
@NETS
def test_two_fits_are_bitwise_identical(net):
    kind, init = KINDS[net]
    sp, oc = packed()
    w = init(6, bn_noise=True)
    a = fit_samples(w, sp, oc, batch_size=64, epochs=3, seed=3, net=kind, options=OPTIONS, adam=EVERYTHING)
    b = fit_samples(w, sp, oc, batch_size=64, epochs=3, seed=3, net=kind, options=OPTIONS, adam=EVERYTHING)
    assert a.weights.tobytes() == b.weights.tobytes() and a.best_weights.tobytes() == b.best_weights.tobytes()
    for x, y in zip(a.optimizer[:2] + a.best_optimizer[:2], b.optimizer[:2] + b.best_optimizer[:2]):
        assert x.tobytes() == y.tobytes()
    assert a.history == b.history and a.best_epoch == b.best_epoch
    for sa, sb in ((a.slots, b.slots), (a.best_slots, b.best_slots)):
        assert set(sa) == set(sb) == {"vhat", "average"}
        assert all(sa[k].tobytes() == sb[k].tobytes() for k in sa)
    off = fit_samples(w, sp, oc, batch_size=64, epochs=3, seed=3, net=kind, options=OPTIONS)
    assert off.weights.tobytes() != a.weights.tobytes() and off.slots is None


# ---------------------------------------------------------------------------------------------------- 7. end to end
@NETS
def test_fit_resident_judges_and_returns_the_average(net):
    kind, init = KINDS[net]
    sp, oc = packed()
    w = init(7, bn_noise=True)
    with Fitter(max_batch=64, net=kind) as f:
        f.add_samples(sp, oc)
        res = fit_resident(f, w, batch_size=64, epochs=3, seed=5, adam=AdamOptions(ema_momentum=0.9))
        assert f.get_weights().tobytes() == res.weights.tobytes()
        assert res.slots["average"].tobytes() == res.weights.tobytes() and set(res.slots) == {"average"}
        raw = fit_resident(f, w, batch_size=64, epochs=3, seed=5)
        assert f.get_adam().ema_momentum == 0.0 and raw.slots is None
    split_at = split_index(384, 0.3)
    with Fitter(max_batch=64, net=kind) as fresh:
        fresh.add_samples(sp, oc)
        fresh.set_weights(res.best_weights)
        val = fresh.evaluate(split_at, 384 - split_at, 64)
    assert res.history["val_loss"][res.best_epoch] == val[0]
    assert res.history["val_loss"] != raw.history["val_loss"] and res.history["loss"] == raw.history["loss"]
    assert res.weights.tobytes() != raw.weights.tobytes()
    assert res.optimizer[0].tobytes() == raw.optimizer[0].tobytes()  # without overwrite the iterates are the same


# ---------------------------------------------------------------------------------------------------- 8. ABI errors
def test_abi_errors_change_nothing():
    L = _lib.load()
    size = C.sizeof(_lib.CaFitAdam)
    f32p = C.POINTER(C.c_float)
    with Fitter(max_batch=16) as f:
        good = AdamOptions(beta_1=0.5, beta_2=0.75, epsilon=0.125, amsgrad=True, ema_momentum=0.25, ema_overwrite_frequency=3)
        f.set_adam(good)
        assert f.get_adam() == good
        ok = dict(struct_size=size, beta_1=0.5, beta_2=0.5, epsilon=0.5, amsgrad=0, ema_momentum=0.5, ema_overwrite_frequency=0)
        bad = [dict(beta_1=1.0), dict(beta_1=-0.5), dict(beta_1=float("nan")), dict(beta_2=1.0), dict(beta_2=-1e-3),
               dict(beta_2=float("inf")), dict(epsilon=0.0), dict(epsilon=-1.0), dict(epsilon=float("inf")),
               dict(epsilon=float("nan")), dict(ema_momentum=1.0), dict(ema_momentum=-0.25), dict(ema_momentum=float("nan")),
               dict(ema_overwrite_frequency=-1), dict(ema_momentum=0.0, ema_overwrite_frequency=2), dict(struct_size=3)]
        for kw in bad:
            c = _lib.CaFitAdam(**dict(ok, **kw))
            assert L.ca_fitter_set_adam(f._h, C.byref(c)) == ERR_ARG and L.ca_last_error(), kw
            assert f.get_adam() == good
        assert L.ca_fitter_set_adam(f._h, None) == ERR_ARG
        assert L.ca_fitter_set_adam(None, C.byref(_lib.CaFitAdam(**ok))) == ERR_ARG
        assert L.ca_fitter_get_adam(None, C.byref(_lib.CaFitAdam(struct_size=size))) == ERR_ARG
        assert L.ca_fitter_get_adam(f._h, C.byref(_lib.CaFitAdam(struct_size=3))) == ERR_ARG
        assert f.get_adam() == good
        # a shorter struct: what it does not have takes the Adam defaults (not zeros), whatever the bytes behind it say
        c = _lib.CaFitAdam(struct_size=12, beta_1=0.0, beta_2=0.25, epsilon=float("nan"), amsgrad=1, ema_momentum=7.0)
        assert L.ca_fitter_set_adam(f._h, C.byref(c)) == 0
        assert f.get_adam() == AdamOptions(beta_1=0.0, beta_2=0.25, epsilon=float(np.float32(1e-7)))
        c = _lib.CaFitAdam(struct_size=4)
        assert L.ca_fitter_set_adam(f._h, C.byref(c)) == 0
        assert f.get_adam() == AdamOptions(beta_1=float(np.float32(0.9)), beta_2=float(np.float32(0.999)),
                                           epsilon=float(np.float32(1e-7)))
        # and only as many bytes are written back as the caller has
        c = _lib.CaFitAdam(struct_size=8, beta_2=7.0)
        assert L.ca_fitter_get_adam(f._h, C.byref(c)) == 0
        assert (c.struct_size, c.beta_1, c.beta_2) == (8, np.float32(0.9), 7.0)
        # the slots: a wrong count, a wrong slot, a null pointer
        n = f.num_weights
        x = np.ones(n + 1, np.float32)
        p = x.ctypes.data_as(f32p)
        f.set_weights(np.zeros(n, np.float32))
        f.set_slot("vhat", np.full(n, 2.0, np.float32))
        for which, count in ((0, n - 1), (0, n + 1), (1, n - 1), (2, n), (-1, n)):
            assert L.ca_fitter_set_slot(f._h, which, p, count) == ERR_ARG, (which, count)
            assert L.ca_fitter_get_slot(f._h, which, p, count) == ERR_ARG, (which, count)
        assert L.ca_fitter_set_slot(f._h, 0, None, n) == ERR_ARG and L.ca_fitter_get_slot(f._h, 0, None, n) == ERR_ARG
        assert L.ca_fitter_set_slot(None, 0, p, n) == ERR_ARG and L.ca_fitter_swap_average(None) == ERR_ARG
        assert L.ca_fitter_apply_average(None) == ERR_ARG
        assert np.all(x == 1.0) and np.all(f.get_slot("vhat") == 2.0)
        assert L.ca_fitter_get_slot(f._h, 1, p, n) == ERR_STATE  # the refused set_slot installed no average
        with pytest.raises(ValueError):
            f.get_slot("m")
        f.set_slot("average", np.full(n, 3.0, np.float32))
        assert np.all(f.get_slot("average") == 3.0)


# ---------------------------------------------------------------------------------------------------- 9. a generation
@NETS
def test_generation_with_adam_equals_the_pieces(net, tmp_path):
    """64 games x 50 searches through Run with averaging and AMSGrad in the TOML, and the same fit by hand"""
    toml = tmp_path / "a.toml"
    toml.write_text("[hyperparameters]\nname = \"run\"\ncwd = \"%s\"\nnet = \"%s\"\nnum_games = 64\nmax_searches = 50\n"
                    "searches_per_eval = 16\nnum_test_games = 32\nepochs = 2\nbatch_size = 256\nlearning_rate = 0.001\n"
                    "patience = 2\nc_puct = 3.0\nseed = 11\namsgrad = true\nema_momentum = 0.9\nbeta_2 = 0.99\n" % (tmp_path, net))
    p, _ = R.parse_args(["--config", str(toml)])
    ad = AdamOptions(beta_2=0.99, amsgrad=True, ema_momentum=0.9)
    assert p.adam_options() == ad
    with Run.open(p) as run:
        res = run.generation()
    gen = os.path.join(run.root, "generations")
    assert os.path.exists(os.path.join(gen, "gen_1", "training_logs", "fit_options.json"))
    w0, opt0 = R.load_model(os.path.join(gen, "gen_0", "model.npz"))
    assert R.load_model_slots(os.path.join(gen, "gen_0", "model.npz")) == {}
    sp, oc = samples_io.load_packed(os.path.join(run.root, "samples", "gen_1"))
    with Fitter(max_batch=256, net=KINDS[net][0]) as f:
        f.add_samples(sp, oc)
        hand = fit_resident(f, w0, learning_rate=0.001, batch_size=256, epochs=2, validation_split=R.VALIDATION_SPLIT,
                            anneal_factor=p.anneal_factor, patience=p.patience, seed=res.seeds["fit"], optimizer_state=opt0,
                            adam=ad)
        plain = fit_resident(f, w0, learning_rate=0.001, batch_size=256, epochs=2, validation_split=R.VALIDATION_SPLIT,
                             anneal_factor=p.anneal_factor, patience=p.patience, seed=res.seeds["fit"], optimizer_state=opt0)
    w1, (m1, v1, it1) = R.load_model(os.path.join(gen, "gen_1", "model.npz"))
    slots = R.load_model_slots(os.path.join(gen, "gen_1", "model.npz"))
    assert hand.history == res.fit.history
    assert hand.best_weights.tobytes() == w1.tobytes() == res.fit.best_weights.tobytes()
    assert hand.best_optimizer[0].tobytes() == m1.tobytes() and hand.best_optimizer[1].tobytes() == v1.tobytes()
    assert hand.best_optimizer[2] == it1
    assert set(slots) == {"vhat", "average"} and slots["average"].tobytes() == w1.tobytes()
    assert slots["vhat"].tobytes() == hand.best_slots["vhat"].tobytes()
    assert plain.best_weights.tobytes() != w1.tobytes() and plain.slots is None
