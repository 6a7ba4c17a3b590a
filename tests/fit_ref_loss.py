"""TEST INFRASTRUCTURE: the loss options and the metrics (include/corintho_hip.h, "loss and metrics") restated on the
CPU, on top of forward() of tests/fit_ref.py (mlp12x100) and tests/fit_ref_rescnn4.py (rescnn4).  The loss in torch, in
float64 (the yardstick) or float32 (its own error is the scale the device is judged by); the five metrics in numpy from
given logits; RefBackend(net, dtype) is the base module's backend with set_loss / set_metrics / metrics / predict (and
sample weights), for fit.fit(..., loss=, metrics=).

    t'_j = t_j (1 - ls) + ls / 96;  policy term = -sum_j t'_j log_softmax_j(h);  e = tanh v - z
    value term = e^2 (mse), or 0.5 e^2 if |e| <= delta else delta (|e| - 0.5 delta) (huber)
    batch loss = value_weight * mean(w value term) + policy_weight * mean(w policy term)      (the divisor is B)
The loss weights, ls and delta enter as the float32 values the device holds."""
import numpy as np
import torch

from corintho_ai_amd import nets
from corintho_ai_amd.fit import DEFAULT_TOP_K, METRIC_NAMES, LossOptions
from tests import fit_ref, fit_ref_rescnn4

BASE = {"mlp12x100": fit_ref, "rescnn4": fit_ref_rescnn4}


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype)


def constants(loss):
    """(value_weight, policy_weight, label_smoothing, huber_delta) as the device holds them: float32 values, as floats"""
    return tuple(float(np.float32(getattr(loss, k))) for k in ("value_weight", "policy_weight", "label_smoothing", "huber_delta"))


def row_terms(logits, v, z, t, loss):
    """(value term [B], policy term [B]) of a batch, torch"""
    _, _, ls, delta = constants(loss)
    tp = t * (1.0 - ls) + ls / nets.NUM_MOVES
    pol = -(tp * torch.log_softmax(logits, dim=1)).sum(1)
    e = torch.tanh(v) - z
    if loss.value_loss == "huber":
        a = e.abs()
        val = torch.where(a <= delta, 0.5 * e * e, delta * (a - 0.5 * delta))
    else:
        val = e * e
    return val, pol


def batch_losses(logits, v, z, t, loss, w=None):
    """(total, value, policy) of a batch: the rows' (weighted) terms summed over the batch size, total with the loss weights"""
    vw, pw, _, _ = constants(loss)
    val, pol = row_terms(logits, v, z, t, loss)
    if w is not None:
        val, pol = w * val, w * pol
    lv, lp = val.sum() / logits.shape[0], pol.sum() / logits.shape[0]
    return vw * lv + pw * lp, lv, lp


def loss_and_grad(ref, w, states, evals, probs, loss, sample_weight=None, dtype=torch.float64):
    """ref: fit_ref or fit_ref_rescnn4.  (flat gradient of the weighted loss, (total, value, policy), batch statistics) of
    one batch in training mode"""
    wt = _t(w, dtype).clone().requires_grad_(True)
    logits, v, aux = ref.forward(wt, _t(states, dtype), True)
    sw = None if sample_weight is None else _t(sample_weight, dtype)
    tot, lv, lp = batch_losses(logits, v, _t(evals, dtype), _t(probs, dtype), loss, sw)
    tot.backward()
    g = wt.grad.detach().numpy().copy()
    g[ref.stat_mask()] = 0.0
    stats = aux["stats"] if isinstance(aux, dict) else aux
    st = [(m.detach().numpy(), s.detach().numpy()) for m, s in stats]
    return g, (float(tot.detach()), float(lv.detach()), float(lp.detach())), st


def predict(ref, w, states, train=False, dtype=torch.float64):
    """(logits [n, 96], pre-tanh values [n]) as numpy arrays of dtype"""
    with torch.no_grad():
        logits, v, _ = ref.forward(_t(w, dtype), _t(states, dtype), train)
    return logits.numpy(), v.numpy()


def evaluate(ref, w, states, evals, probs, loss, sample_weight=None, dtype=torch.float64):
    """inference mode (moving statistics): (total, value, policy) of one batch"""
    with torch.no_grad():
        logits, v, _ = ref.forward(_t(w, dtype), _t(states, dtype), False)
        sw = None if sample_weight is None else _t(sample_weight, dtype)
        return tuple(float(x) for x in batch_losses(logits, v, _t(evals, dtype), _t(probs, dtype), loss, sw))


def value_errors(ref, w, states, evals, train=True):
    """e = tanh v - z of every row, in float64 (where Huber's kink |e| = delta is looked for)"""
    _, v = predict(ref, w, states, train)
    return np.tanh(v) - np.asarray(evals, np.float64)


RELU_KINK = 2e-7   # tests/test_fit_weights_gpu.py KINK: a ReLU input this close (relative) to 0 has no defined gradient
HUBER_KINK = 1e-4  # | |e| - delta | of every row of a batch judged against float64: Huber's gradient jumps at |e| = delta


def draw_batch(ref, w, states, evals, rng, B, loss, candidates=None):
    """B distinct rows of the set (of `candidates`, if given), drawn again from the same generator (three times at the
    most) while the float64 restatement has a ReLU input within RELU_KINK of its kink or, with Huber, a row within
    HUBER_KINK of |e| = delta.  Nothing here looks at the device.  -> (rows, the last draw's ReLU margin is fine, its Huber margin is fine)"""
    from tests import fit_ref_weighted

    delta = constants(loss)[3]
    for _ in range(4):
        rows = rng.choice(np.asarray(states).shape[0] if candidates is None else candidates, B, replace=False).astype(np.int32)
        relu_ok = fit_ref_weighted.kink_margin(ref, w, states[rows]) >= RELU_KINK
        huber_ok = loss.value_loss != "huber" or bool(
            np.min(np.abs(np.abs(value_errors(ref, w, states[rows], evals[rows])) - delta)) >= HUBER_KINK)
        if relu_ok and huber_ok:
            break
    return rows, relu_ok, huber_ok


# ---------------------------------------------------------------------------------------------------- the metrics
def metric_rows(logits, v, z, t, top_k=DEFAULT_TOP_K, f=np.float64):
    """the five per-row metrics from given head outputs, in f: {name: [n]} (the accuracies are 0 or 1)"""
    h, v, z, t = (np.asarray(a).astype(f) for a in (logits, v, z, t))
    n = h.shape[0]
    c = np.argmax(t, axis=1)  # the first maximum, as numpy takes it
    hc = h[np.arange(n), c]
    m = h.max(axis=1, keepdims=True)
    lp = h - (m + np.log(np.exp(h - m).sum(axis=1, keepdims=True, dtype=f)))
    with np.errstate(divide="ignore", invalid="ignore"):
        tlt = np.where(t > 0, t * np.log(np.where(t > 0, t, 1)), f(0))
    return {"categorical_accuracy": (np.argmax(h, axis=1) == c).astype(f),
            "top_k_categorical_accuracy": ((h > hc[:, None]).sum(axis=1) < top_k).astype(f),
            "mean_absolute_error": np.abs(np.tanh(v) - z),
            "policy_entropy": -(np.exp(lp) * lp).sum(axis=1, dtype=f),
            "target_entropy": -tlt.sum(axis=1, dtype=f)}


def _sum(x, f):
    """the sum of x in f: float32 adds one term after the other in float32, as a plain float32 loop would"""
    x = np.asarray(x, f)
    return f(0) if x.size == 0 else np.cumsum(x, dtype=f)[-1]


def weighted_mean(x, w, f=np.float64):
    """sum w x / sum w in f (Keras's Mean with sample_weight); 0 if the weights sum to 0"""
    x, w = np.asarray(x, f), np.asarray(w, f)
    ws = _sum(w, f)
    return float(_sum(w * x, f) / ws) if ws > 0 else 0.0


def metrics(logits, v, z, t, top_k=DEFAULT_TOP_K, w=None, f=np.float64):
    """the call's metrics: METRIC_NAMES' weighted means, "rows", "weight_sum" and "top_k" (Fitter.metrics()'s dict)"""
    rows = metric_rows(logits, v, z, t, top_k, f)
    n = np.asarray(logits).shape[0]
    w = np.ones(n, f) if w is None else np.asarray(w).astype(f)
    out = {k: weighted_mean(rows[k], w, f) for k in METRIC_NAMES}
    out.update(rows=n, weight_sum=float(_sum(w, f)), top_k=int(top_k))
    return out


# ---------------------------------------------------------------------------------------------------- the backend
def RefBackend(net, dtype=None):
    """the base module's backend with the loss options, the metrics, predict and sample weights.  With the default loss,
    no sample weights and metrics off, train() and evaluate() are the base backend's own."""
    base = BASE[net]
    dtype = dtype or base.torch.float64

    class Backend(base.RefBackend):
        def __init__(self):
            super().__init__(dtype)
            self.loss = LossOptions()
            self.top_k = None  # None: metrics off
            self.sw = None
            self.last = None
            self.set_loss_calls, self.set_metrics_calls = [], []

        def set_data(self, s, e, p):
            super().set_data(s, e, p)
            self.sw = None

        def set_sample_weights(self, w):
            self.sw = None if w is None else np.asarray(w, np.float32).copy()

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
            lo, v = predict(base, self.w, self.data[0][np.asarray(rows)], train, self.dtype)
            return lo.astype(np.float32), v.astype(np.float32)

        def _plain(self):
            return self.loss.is_default() and self.sw is None and self.top_k is None

        def _collect(self, acc, lo, v, r):
            """the rows' metric terms of one batch, kept until the call's means are taken"""
            if self.top_k is None:
                return
            _, e, p = self.data
            rows = metric_rows(lo, v, e[r], p[r], self.top_k, self.np_dtype)
            acc.append((rows, np.ones(len(r)) if self.sw is None else self.sw[r]))

        def _finish(self, acc, n):
            if self.top_k is None:
                return
            w = np.concatenate([a[1] for a in acc]).astype(np.float64)
            out = {k: weighted_mean(np.concatenate([a[0][k] for a in acc]), w) for k in METRIC_NAMES}
            out.update(rows=int(n), weight_sum=float(w.sum()), top_k=self.top_k)
            self.last = out

        def train(self, rows, batch_size, lr, batch_losses=False):
            if self._plain():
                return super().train(rows, batch_size, lr, batch_losses)
            rows = np.asarray(rows)
            self.trained_rows.append(rows.copy())
            s, e, p = self.data
            tot, per, acc = np.zeros(3), [], []
            for b0 in range(0, rows.size, batch_size):
                r = rows[b0:b0 + batch_size]
                if self.top_k is not None:  # the step's own forward: batch statistics, the weights from before the step
                    self._collect(acc, *predict(base, self.w, s[r], True, self.dtype), r)
                g, ls, st = loss_and_grad(base, self.w, s[r], e[r], p[r], self.loss, None if self.sw is None else self.sw[r],
                                          self.dtype)
                self.it = base.adam_step(self.w, self.m, self.v, g, self.it, lr, st, self.np_dtype)
                per.append(ls)
                tot += np.asarray(ls) * r.size
            self._finish(acc, rows.size)
            out = tuple(tot / rows.size)
            return (out, np.asarray(per)) if batch_losses else out

        def evaluate(self, row0, n_rows, batch_size):
            if self._plain():
                return super().evaluate(row0, n_rows, batch_size)
            s, e, p = self.data
            tot, acc = np.zeros(3), []
            for b0 in range(row0, row0 + n_rows, batch_size):
                r = np.arange(b0, min(b0 + batch_size, row0 + n_rows))
                if self.top_k is not None:
                    self._collect(acc, *predict(base, self.w, s[r], False, self.dtype), r)
                ls = evaluate(base, self.w, s[r], e[r], p[r], self.loss, None if self.sw is None else self.sw[r], self.dtype)
                tot += np.asarray(ls) * r.size
            self._finish(acc, n_rows)
            return tuple(tot / n_rows)

    return Backend()
