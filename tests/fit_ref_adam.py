"""TEST INFRASTRUCTURE: Adam's arguments (include/corintho_hip.h, "Adam's arguments": beta_1, beta_2, epsilon, AMSGrad's
third slot, the averaged weights and their overwrite) restated in numpy, in float32 (operation for operation what the
device does, so sums, differences, products and maxima agree bit for bit) or float64 (the yardstick).

    out = adam_update(w1, m, v, h, a, g2, iterations, lr, adam, f)      one step on trainable weights
tests/fit_ref_step.py's backend takes this update in place of the plain one when an argument is off its default."""
import numpy as np


def constants(adam, f=np.float32):
    """(beta_1, beta_2, epsilon, ema_momentum) as the device holds them (float32 values), in f"""
    return tuple(f(np.float32(x)) for x in (adam.beta_1, adam.beta_2, adam.epsilon, adam.ema_momentum))


def lr_t(lr, iterations, adam):
    """the host's float32 lr_t of the step that follows `iterations` steps"""
    f = np.float32
    b1, b2, _, _ = constants(adam)
    t = f(iterations + 1)
    return f(lr) * (np.sqrt(f(1) - np.power(b2, t)) / (f(1) - np.power(b1, t)))


def overwrites(iterations, adam):
    k = int(adam.ema_overwrite_frequency)
    return k > 0 and (iterations + 1) % k == 0


def adam_update(w1, m, v, h, a, g2, iterations, lr, adam, f=np.float32, w2=None):
    """The definition on arrays of trainable weights: w1 = w', g2 = g'', h and a may be None when amsgrad or the average
    is off.  lr_t is the host's float32 value whatever f is.  w2: take this as w'' for the average instead of the
    restatement's own (the device's, when a' is to be compared bit for bit).
    -> dict(m, v, h, d, step, w2, a, w3)"""
    b1, b2, eps, mom = constants(adam, f)
    one = f(1)
    w1, m, v, g2 = (np.asarray(x).astype(f) for x in (w1, m, v, g2))
    lt = f(lr_t(lr, iterations, adam))
    m1 = m + (g2 - m) * (one - b1)
    v1 = v + (g2 * g2 - v) * (one - b2)
    out = {"m": m1, "v": v1, "h": None, "a": None}
    d = v1
    if adam.amsgrad:
        d = np.maximum(np.asarray(h).astype(f), v1)
        out["h"] = d
    step = lt * m1 / (np.sqrt(d) + eps)
    out["d"], out["step"] = d, step
    out["w2"] = w1 - step
    w3 = out["w2"]
    if adam.averaged():
        base = out["w2"] if w2 is None else np.asarray(w2).astype(f)
        a0 = np.asarray(a).astype(f)
        out["a"] = a0 + (base - a0) * (one - mom)
        if overwrites(iterations, adam):
            w3 = out["a"]
    out["w3"] = w3
    return out
