"""TEST INFRASTRUCTURE: the training step of both networks restated on the CPU, once, in float64 (the yardstick) or
float32 (its own error is the scale the device is judged by).  A network module (tests/fit_ref.py for mlp12x100,
tests/fit_ref_rescnn4.py for rescnn4; `ref` below) has forward(), stat_mask() and bn_slices(); everything else of a step is
here, written from tf.keras 2.x (corintho_ai_amd/fit.py; wrapper.py:256-282, main.pyx:249-260):

  * the loss is tests/fit_ref_loss.py's batch_losses: at LossOptions' defaults and without sample weights
    mean (tanh v - z)^2 + 0.25 * mean(-sum t log_softmax(logits)); gradients come from autograd;
  * Adam = TF ResourceApplyAdam: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), m += (g - m)(1 - b1), v += (g^2 - v)(1 - b2),
    w -= lr_t m / (sqrt(v) + 1e-7), on kernels, biases, gamma and beta only; the BatchNorms' moving statistics move by
    moving -= (moving - batch_stat) * 0.01;
  * around it, present or absent by the backend's state: the fit options (tests/fit_ref_options.py: regulariser, clip,
    decay), Adam's arguments (tests/fit_ref_adam.py: adam_update in place of the plain update) and the metrics
    (tests/fit_ref_loss.py).
RefBackend(net, dtype) drives corintho_ai_amd.fit.fit() and its relatives with it."""
import numpy as np
import torch

from corintho_ai_amd.fit import DEFAULT_TOP_K, METRIC_NAMES, AdamOptions, FitOptions, LossOptions
from tests import fit_ref, fit_ref_rescnn4
from tests import fit_ref_adam as A
from tests import fit_ref_loss as L
from tests import fit_ref_options as O

BASE = {"mlp12x100": fit_ref, "rescnn4": fit_ref_rescnn4}
B1, B2, ADAM_EPS, MOMENTUM = 0.9, 0.999, 1e-7, 0.99
RELU_KINK = 2e-7   # a ReLU input this close (relative) to 0 has no defined gradient
HUBER_KINK = 1e-4  # | |e| - delta | of every row of a batch judged against float64: Huber's gradient jumps at |e| = delta
NO_STATS = dict(steps=0, clipped_steps=0, regularization_loss=0.0, grad_norm=0.0, grad_norm_max=0.0)


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype)


def within(dev, f32, f64, floor):
    """the rule of the GPU tests: the device's error against float64 is at most 4 x the float32 restatement's, plus a
    floor -> (ok, the device's error, float32's)"""
    e_dev = float(np.max(np.abs(np.asarray(dev, np.float64) - f64)))
    e_32 = float(np.max(np.abs(np.asarray(f32, np.float64) - f64)))
    return e_dev <= 4.0 * e_32 + floor, e_dev, e_32


# ---------------------------------------------------------------------------------------------------- one batch
def loss_and_grad(ref, w, states, evals, probs, loss=None, sample_weight=None, dtype=torch.float64):
    """(flat gradient of the batch loss, (total, value, policy), the BatchNorms' batch statistics) of one batch in training
    mode; loss: a LossOptions, None: the defaults"""
    wt = _t(w, dtype).clone().requires_grad_(True)
    logits, v, aux = ref.forward(wt, _t(states, dtype), True)
    sw = None if sample_weight is None else _t(sample_weight, dtype)
    tot, lv, lp = L.batch_losses(logits, v, _t(evals, dtype), _t(probs, dtype), loss or LossOptions(), sw)
    tot.backward()
    g = wt.grad.detach().numpy().copy()
    g[ref.stat_mask()] = 0.0
    st = [(m.detach().numpy(), s.detach().numpy()) for m, s in aux["stats"]]
    return g, (float(tot.detach()), float(lv.detach()), float(lp.detach())), st


def predict(ref, w, states, train=False, dtype=torch.float64):
    """(logits [n, 96], pre-tanh values [n]) as numpy arrays of dtype"""
    with torch.no_grad():
        logits, v, _ = ref.forward(_t(w, dtype), _t(states, dtype), train)
    return logits.numpy(), v.numpy()


def evaluate(ref, w, states, evals, probs, loss=None, sample_weight=None, dtype=torch.float64):
    """inference mode (moving statistics): the (total, value, policy) losses of one batch and the outputs (tanh v, softmax)"""
    with torch.no_grad():
        logits, v, _ = ref.forward(_t(w, dtype), _t(states, dtype), False)
        sw = None if sample_weight is None else _t(sample_weight, dtype)
        ls = L.batch_losses(logits, v, _t(evals, dtype), _t(probs, dtype), loss or LossOptions(), sw)
        return tuple(float(x) for x in ls), (torch.tanh(v).numpy(), torch.softmax(logits, 1).numpy())


def kink_margin(ref, w, states):
    """smallest |ReLU input| / its tensor's largest, over the batch in float64 (training mode): where it is tiny a ReLU
    sits at its kink, the gradient is not defined there, and float32 rounding picks either side"""
    with torch.no_grad():
        _, _, aux = ref.forward(_t(w, torch.float64), _t(states, torch.float64), True)
    return min(float(t.abs().min() / t.abs().max()) for t in aux["relu_inputs"])


def value_errors(ref, w, states, evals, train=True):
    """e = tanh v - z of every row, in float64 (where Huber's kink |e| = delta is looked for)"""
    _, v = predict(ref, w, states, train)
    return np.tanh(v) - np.asarray(evals, np.float64)


def draw_batch(ref, w, states, evals, rng, B, loss, candidates=None):
    """B distinct rows of the set (of `candidates`, if given), drawn again from the same generator (three times at the
    most) while the float64 restatement has a ReLU input within RELU_KINK of its kink or, with Huber, a row within
    HUBER_KINK of |e| = delta.  Nothing here looks at the device.  -> (rows, the last draw's ReLU margin is fine, its Huber margin is fine)"""
    delta = L.constants(loss)[3]
    for _ in range(4):
        rows = rng.choice(np.asarray(states).shape[0] if candidates is None else candidates, B, replace=False).astype(np.int32)
        relu_ok = kink_margin(ref, w, states[rows]) >= RELU_KINK
        huber_ok = loss.value_loss != "huber" or bool(
            np.min(np.abs(np.abs(value_errors(ref, w, states[rows], evals[rows])) - delta)) >= HUBER_KINK)
        if relu_ok and huber_ok:
            break
    return rows, relu_ok, huber_ok


def move_statistics(ref, w, stats, np_dtype=np.float64):
    """the moving statistics of w, in place, toward the batch statistics of a step"""
    f = np_dtype
    for (mu, va), (bm, bv) in zip(ref.bn_slices(), stats):
        for sl, bs in ((mu, bm), (va, bv)):
            w[sl] = w[sl] - (w[sl] - bs.astype(f)) * f(1 - MOMENTUM)


def adam_step(ref, w, m, v, g, iterations, lr, stats, np_dtype=np.float64):
    """one Keras step in place of (w, m, v): Adam at its defaults on the trainable weights, the moving statistics
    toward `stats`"""
    t = iterations + 1
    f = np_dtype
    lr_t = f(lr) * np.sqrt(f(1) - f(B2) ** f(t)) / (f(1) - f(B1) ** f(t))
    mask = ~ref.stat_mask()
    gg = g.astype(f)
    m[mask] = m[mask] + (gg[mask] - m[mask]) * (f(1) - f(B1))
    v[mask] = v[mask] + (gg[mask] * gg[mask] - v[mask]) * (f(1) - f(B2))
    w[mask] = w[mask] - lr_t * m[mask] / (np.sqrt(v[mask]) + f(ADAM_EPS))
    move_statistics(ref, w, stats, f)
    return t


# ---------------------------------------------------------------------------------------------------- the backend
class RefBackend:
    """the Fitter protocol corintho_ai_amd.fit speaks, computed by this restatement (float64 by default): data and
    sample weights, the fit options and train_stats, Adam's arguments with the slots, the loss, the metrics and predict.
    With every family at its default, no sample weights and metrics off a step is loss_and_grad and adam_step."""

    def __init__(self, net, dtype=None):
        self.net, self.ref = net, BASE[net]
        self.dtype = dtype or torch.float64
        self.np_dtype = np.float64 if self.dtype == torch.float64 else np.float32
        self.data = self.sw = None
        self.options, self.adam, self.loss = FitOptions(), AdamOptions(), LossOptions()
        self.top_k = None  # None: metrics off
        self.h = self.a = None  # AMSGrad's third slot, the averaged weights
        self.stats, self.last = dict(NO_STATS), None
        # what the tests of fit's host logic read
        self.trained_rows, self.lrs = [], []  # the row order and the learning rate of every train() call
        self.set_options_calls, self.set_adam_calls, self.set_loss_calls, self.set_metrics_calls = [], [], [], []
        self.swaps, self.applied = 0, 0
        self.step_norms = []  # the norm of g' of every step trained with an option on

    # ---- weights, optimizer state and data
    def set_weights(self, w):
        self.w = np.asarray(w, self.np_dtype).copy()
        self.a = None

    def get_weights(self):
        return self.w.astype(np.float32)

    def set_optimizer(self, m, v, iterations):
        self.m = np.asarray(m, self.np_dtype).copy()
        self.v = np.asarray(v, self.np_dtype).copy()
        self.it = int(iterations)
        self.h = None

    def get_optimizer(self):
        return self.m.astype(np.float32), self.v.astype(np.float32), self.it

    def set_data(self, s, e, p):
        self.data = (np.asarray(s), np.asarray(e), np.asarray(p))
        self.sw = None

    def set_sample_weights(self, w):
        self.sw = None if w is None else np.asarray(w, np.float32).copy()

    # ---- the fit options
    def set_options(self, options=None):
        self.options = options or FitOptions()
        self.set_options_calls.append(self.options)

    def get_options(self):
        return self.options

    def train_stats(self):
        return dict(self.stats)

    # ---- Adam's arguments, the slots and the averaged weights
    def set_adam(self, adam=None):
        self.adam = adam or AdamOptions()
        self.set_adam_calls.append(self.adam)

    def get_adam(self):
        return self.adam

    def set_slot(self, which, values):
        x = np.asarray(values, self.np_dtype).copy()
        if which == "vhat":
            self.h = x
        else:
            self.a = x

    def get_slot(self, which):
        if which == "vhat":
            return (np.zeros_like(self.w) if self.h is None else self.h).astype(np.float32)
        if self.a is None:
            raise RuntimeError("no average")
        return self.a.astype(np.float32)

    def swap_average(self):
        if self.a is None:
            raise RuntimeError("no average")
        self.w, self.a = self.a, self.w
        self.swaps += 1

    def apply_average(self):
        if self.a is None:
            raise RuntimeError("no average")
        tr = ~self.ref.stat_mask()
        self.w[tr] = self.a[tr]
        self.applied += 1

    # ---- the loss, the metrics and predict
    def set_loss(self, loss=None):
        self.loss = loss or LossOptions()
        self.set_loss_calls.append(self.loss)

    def get_loss(self):
        return self.loss

    def set_metrics(self, on=True, top_k=DEFAULT_TOP_K):
        self.top_k = int(top_k) if on else None
        self.set_metrics_calls.append((bool(on), int(top_k)))
        self.last = None

    def metrics(self):
        if self.top_k is None:
            raise RuntimeError("metrics are off")
        return dict(self.last)

    def predict(self, rows, train=False):
        lo, v = predict(self.ref, self.w, self.data[0][np.asarray(rows)], train, self.dtype)
        return lo.astype(np.float32), v.astype(np.float32)

    def _collect(self, acc, r, train):
        """the rows' metric terms of one batch, from a forward of its own with the weights as they are, kept until the
        call's means are taken"""
        if self.top_k is None:
            return
        s, e, p = self.data
        lo, v = predict(self.ref, self.w, s[r], train, self.dtype)
        acc.append((L.metric_rows(lo, v, e[r], p[r], self.top_k, self.np_dtype), np.ones(len(r)) if self.sw is None else self.sw[r]))

    def _finish(self, acc, n):
        if self.top_k is None:
            return
        w = np.concatenate([a[1] for a in acc]).astype(np.float64)
        self.last = {k: L.weighted_mean(np.concatenate([a[0][k] for a in acc]), w) for k in METRIC_NAMES}
        self.last.update(rows=int(n), weight_sum=float(w.sum()), top_k=self.top_k)

    # ---- an epoch and an evaluation
    def train(self, rows, batch_size, lr, batch_losses=False):
        rows = np.asarray(rows)
        self.trained_rows.append(rows.copy())
        self.lrs.append(float(lr))
        ref, net, o, ad, f = self.ref, self.net, self.options, self.adam, self.np_dtype
        s, e, p = self.data
        tr = ~ref.stat_mask()
        tot, per, acc, regs, norms, clipped = np.zeros(3), [], [], [], [], 0
        for b0 in range(0, rows.size, batch_size):
            r = rows[b0:b0 + batch_size]
            self._collect(acc, r, True)
            g, ls, st = loss_and_grad(ref, self.w, s[r], e[r], p[r], self.loss, None if self.sw is None else self.sw[r], self.dtype)
            if o.any():  # steps 1, 2 and 5 of the fit options; step 3, the decay, is just before Adam's update
                R = O.reg_loss(net, self.w, o)
                g, info = O.clip(net, O.add_reg(net, g, self.w, o, f), o, f)
                ls = (ls[0] + R, ls[1], ls[2])
                regs.append(R)
                norms.append(info["norm"])
                clipped += bool(info["clipped"])
            if ad.is_default():
                if o.any():
                    self.w[:] = O.decay(net, self.w, lr, o, f)
                self.it = adam_step(ref, self.w, self.m, self.v, g, self.it, lr, st, f)
            else:
                if ad.amsgrad and self.h is None:
                    self.h = np.zeros_like(self.w)
                if ad.averaged() and self.a is None:
                    self.a = self.w.copy()
                u = A.adam_update(O.decay(net, self.w, lr, o, f)[tr], self.m[tr], self.v[tr], None if self.h is None else self.h[tr],
                                  None if self.a is None else self.a[tr], g[tr], self.it, lr, ad, f)
                move_statistics(ref, self.w, st, f)
                self.w[tr], self.m[tr], self.v[tr] = u["w3"], u["m"], u["v"]
                if ad.amsgrad:
                    self.h[tr] = u["h"]
                if ad.averaged():
                    self.a[tr] = u["a"]
                    self.a[~tr] = self.w[~tr]
                self.it += 1
            per.append(ls)
            tot += np.asarray(ls) * r.size
        self.step_norms += norms
        self.stats = dict(steps=len(per), clipped_steps=clipped, regularization_loss=float(np.mean(regs)),
                          grad_norm=float(np.mean(norms)), grad_norm_max=float(np.max(norms))) if o.any() else dict(NO_STATS)
        self._finish(acc, rows.size)
        out = tuple(tot / rows.size)
        return (out, np.asarray(per)) if batch_losses else out

    def evaluate(self, row0, n_rows, batch_size):
        s, e, p = self.data
        tot, acc = np.zeros(3), []
        for b0 in range(row0, row0 + n_rows, batch_size):
            r = np.arange(b0, min(b0 + batch_size, row0 + n_rows))
            self._collect(acc, r, False)
            ls, _ = evaluate(self.ref, self.w, s[r], e[r], p[r], self.loss, None if self.sw is None else self.sw[r], self.dtype)
            tot += np.asarray(ls) * r.size
        self._finish(acc, n_rows)
        tot, lv, lp = tot / n_rows
        return tot + (O.reg_loss(self.net, self.w, self.options) if self.options.any() else 0.0), lv, lp

    def close(self):
        pass


class BaseOnly:
    """a backend that knows no family: the seven calls fit() needs (and those of `more`), forwarded to a RefBackend"""

    def __init__(self, inner, *more):
        self.inner = inner
        for name in ("set_weights", "get_weights", "set_optimizer", "get_optimizer", "set_data", "train", "evaluate") + more:
            setattr(self, name, getattr(inner, name))
