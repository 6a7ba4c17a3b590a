"""TEST INFRASTRUCTURE: the loss with its options and the metrics (include/corintho_hip.h, "loss and metrics") restated on
the CPU as functions of the head outputs, for both networks.  The loss in torch, in float64 (the yardstick) or float32
(its own error is the scale the device is judged by); the five metrics in numpy from given logits.
tests/fit_ref_step.py builds the step and the backend on them.

    t'_j = t_j (1 - ls) + ls / 96;  policy term = -sum_j t'_j log_softmax_j(h);  e = tanh v - z
    value term = e^2 (mse), or 0.5 e^2 if |e| <= delta else delta (|e| - 0.5 delta) (huber)
    batch loss = value_weight * mean(w value term) + policy_weight * mean(w policy term)      (the divisor is B)
The loss weights, ls and delta enter as the float32 values the device holds.  Sample weights are Keras's
model.fit(sample_weight=w) under SUM_OVER_BATCH_SIZE: the divisor is B, not sum w, and BatchNorm's batch statistics stay
unweighted, so a row of weight 0 still counts in them."""
import numpy as np
import torch

from corintho_ai_amd import nets
from corintho_ai_amd.fit import DEFAULT_TOP_K, METRIC_NAMES


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
    """(total, value, policy) of a batch: the means over the batch of the rows' terms (times their sample weights w, if
    given), total with the loss weights.  At LossOptions' defaults: mean (tanh v - z)^2 + 0.25 mean cross-entropy"""
    vw, pw, _, _ = constants(loss)
    val, pol = row_terms(logits, v, z, t, loss)
    if w is not None:
        val, pol = w * val, w * pol
    lv, lp = val.mean(), pol.mean()
    return vw * lv + pw * lp, lv, lp


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
