"""TEST INFRASTRUCTURE: the training step with per-sample weights, restated in torch on the CPU on top of forward() of
tests/fit_ref.py (mlp12x100) and tests/fit_ref_rescnn4.py (rescnn4), in float64 (the yardstick) or float32 (its own
error is the scale the device is judged by).  Keras's model.fit(sample_weight=w) under SUM_OVER_BATCH_SIZE:

    value loss  = (1/B) sum_r w_r (tanh v_r - z_r)^2
    policy loss = (1/B) sum_r w_r (-sum_m t_r[m] log_softmax(logits_r)[m])

The divisor is B, not sum w, and forward() is untouched: BatchNorm's batch statistics stay unweighted, so a row of weight
0 still counts in them."""
import numpy as np
import torch

from tests import fit_ref, fit_ref_rescnn4


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype)


def weighted_losses(logits, v, z, t, w):
    """(value, policy) loss of a batch: sums of the rows' weighted terms over the batch size"""
    b = logits.shape[0]
    lv = (w * (torch.tanh(v) - z) ** 2).sum() / b
    lp = (w * -(t * torch.log_softmax(logits, dim=1)).sum(1)).sum() / b
    return lv, lp


def loss_and_grad(ref, w, states, evals, probs, sample_weight, dtype=torch.float64):
    """ref: fit_ref or fit_ref_rescnn4.  (flat gradient of value + 0.25 policy, (total, value, policy)) of one batch in
    training mode"""
    wt = _t(w, dtype).clone().requires_grad_(True)
    logits, v, _ = ref.forward(wt, _t(states, dtype), True)
    lv, lp = weighted_losses(logits, v, _t(evals, dtype), _t(probs, dtype), _t(sample_weight, dtype))
    loss = lv + 0.25 * lp
    loss.backward()
    g = wt.grad.detach().numpy().copy()
    g[ref.stat_mask()] = 0.0
    return g, (float(loss.detach()), float(lv.detach()), float(lp.detach()))


def evaluate(ref, w, states, evals, probs, sample_weight, dtype=torch.float64):
    """inference mode (moving statistics): the (total, value, policy) weighted losses of one batch"""
    with torch.no_grad():
        logits, v, _ = ref.forward(_t(w, dtype), _t(states, dtype), False)
        lv, lp = weighted_losses(logits, v, _t(evals, dtype), _t(probs, dtype), _t(sample_weight, dtype))
        return float(lv + 0.25 * lp), float(lv), float(lp)


def tensors(ref):
    """[(name, slice, slice of the tensor the gradient's scale is taken from)] of every trainable tensor of either network"""
    if ref is fit_ref_rescnn4:
        return ref.tensors()
    lay, (kv, bv, kp, bp) = fit_ref.layer_offsets()
    out = []
    for i, (k, b, g, be, _, _, fi) in enumerate(lay):
        out += [("k%d" % i, slice(k, k + fi * 100)), ("b%d" % i, slice(b, b + 100)), ("gamma%d" % i, slice(g, g + 100)),
                ("beta%d" % i, slice(be, be + 100))]
    out += [("kv", slice(kv, kv + 100)), ("bv", slice(bv, bv + 1)), ("kp", slice(kp, kp + 9600)), ("bp", slice(bp, bp + 96))]
    return [(name, sl, sl) for name, sl in out]


def kink_margin(ref, w, states):
    """smallest |ReLU input| / its tensor's largest over the batch, in float64 and training mode (the two networks' own
    margins: tests/test_fit_gpu.py::_kink_margin and fit_ref_rescnn4.kink_margin)"""
    if ref is fit_ref_rescnn4:
        return ref.kink_margin(w, states)
    from tests.test_fit_gpu import _kink_margin

    return _kink_margin(w, states)
