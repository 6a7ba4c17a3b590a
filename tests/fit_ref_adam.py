"""TEST INFRASTRUCTURE: Adam's arguments (include/corintho_hip.h, "Adam's arguments": beta_1, beta_2, epsilon, AMSGrad's
third slot, the averaged weights and their overwrite) restated in numpy, in float32 (operation for operation what the
device does, so sums, differences, products and maxima agree bit for bit) or float64 (the yardstick).

    out = adam_update(w1, m, v, h, a, g2, iterations, lr, adam, f)      one step on trainable weights
RefBackend(net, dtype) is tests/fit_ref_options.py's backend with set_adam / get_adam / set_slot / get_slot /
swap_average / apply_average, for fit.fit(..., adam=...)."""
import numpy as np

from corintho_ai_amd.fit import AdamOptions
from tests import fit_ref_options as O


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


def RefBackend(net, dtype=None):
    """the backend of tests/fit_ref_options.py with Adam's arguments: a step with any of them off its default is
    steps 1 to 3 of the fit options, adam_update on the trainable weights and the base module's move of the moving
    statistics"""
    base = O.BASE[net]
    dtype = dtype or base.torch.float64

    class Backend(type(O.RefBackend(net, dtype))):
        def __init__(self):
            super().__init__()
            self.adam = AdamOptions()
            self.h = self.a = None
            self.set_adam_calls, self.swaps, self.applied = [], 0, 0

        def set_adam(self, adam=None):
            self.adam = adam or AdamOptions()
            self.set_adam_calls.append(self.adam)

        def get_adam(self):
            return self.adam

        def set_weights(self, w):
            super().set_weights(w)
            self.a = None

        def set_optimizer(self, m, v, iterations):
            super().set_optimizer(m, v, iterations)
            self.h = None

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
            tr = ~base.stat_mask()
            self.w[tr] = self.a[tr]
            self.applied += 1

        def train(self, rows, batch_size, lr, batch_losses=False):
            ad, o, f = self.adam, self.options, self.np_dtype
            if ad.is_default():
                return super().train(rows, batch_size, lr, batch_losses)
            rows = np.asarray(rows)
            self.trained_rows.append(rows.copy())
            s, e, p = self.data
            tr = ~base.stat_mask()
            tot, per = np.zeros(3), []
            for b0 in range(0, rows.size, batch_size):
                r = rows[b0:b0 + batch_size]
                g, ls, st = base.loss_and_grad(self.w, s[r], e[r], p[r], self.dtype)
                R = O.reg_loss(net, self.w, o) if o.any() else 0.0
                g2 = O.clip(net, O.add_reg(net, g, self.w, o, f), o, f)[0] if o.any() else np.asarray(g, f)
                w1 = O.decay(net, self.w, lr, o, f)
                if ad.amsgrad and self.h is None:
                    self.h = np.zeros_like(self.w)
                if ad.averaged() and self.a is None:
                    self.a = self.w.copy()
                # the moving statistics: the base module's step on copies, of which only they are kept
                moved = self.w.copy()
                base.adam_step(moved, self.m.copy(), self.v.copy(), g, self.it, lr, st, f)
                u = adam_update(w1[tr], self.m[tr], self.v[tr], None if self.h is None else self.h[tr],
                                None if self.a is None else self.a[tr], g2[tr], self.it, lr, ad, f)
                self.w[~tr] = moved[~tr]
                self.w[tr], self.m[tr], self.v[tr] = u["w3"], u["m"], u["v"]
                if ad.amsgrad:
                    self.h[tr] = u["h"]
                if ad.averaged():
                    self.a[tr] = u["a"]
                    self.a[~tr] = self.w[~tr]
                self.it += 1
                ls = (ls[0] + R, ls[1], ls[2])
                per.append(ls)
                tot += np.asarray(ls) * r.size
            out = tuple(tot / rows.size)
            return (out, np.asarray(per)) if batch_losses else out

    return Backend()
