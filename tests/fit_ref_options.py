"""TEST INFRASTRUCTURE: the fit options (include/corintho_hip.h, "fit options": the L1L2 regulariser, decoupled weight
decay, gradient clipping) restated in numpy, in float64 (the yardstick) or float32, as functions of the flat weights
and gradient.  Steps 1 to 3 and 5 of the definition are here; step 4 is Adam's update on what they leave, and
tests/fit_ref_step.py puts them around it.

    r, R = reg_grad(net, w, o), reg_loss(net, w, o)        step 1, step 5
    g2, info = clip(net, add_reg(net, g, w, o), o)         step 2 on g' = g + r
    w1 = decay(net, w, lr, o)                              step 3"""
import numpy as np

from corintho_ai_amd import nets

KERNELS = ("trunk_kernel", "head_kernel")


def tensors(net):
    """[(name, slice, class)] of nets.tensor_table(net)"""
    return [(name, slice(off, off + n), cls) for name, off, n, cls in nets.tensor_table(net)]


def class_mask(net, classes):
    """True at the weights of tensors whose class is one of `classes`"""
    size = nets.MLP_NUM_WEIGHTS if net == "mlp12x100" else nets.RESCNN4_NUM_WEIGHTS
    m = np.zeros(size, bool)
    for _, sl, cls in tensors(net):
        if cls in classes:
            m[sl] = True
    return m


def regularized_mask(net, o):
    return class_mask(net, KERNELS if o.regularize else ("trunk_kernel",))


def trainable_mask(net):
    return ~class_mask(net, ("moving",))


def reg_grad(net, w, o, f=np.float64):
    """step 1: r = l1 sgn(w) + (2 l2) w on the regularised tensors, 0 elsewhere (np.sign(+-0) = 0).  In float64
    whatever f is: the definition rounds g + r, not r (add_reg)"""
    w = np.asarray(w, f).astype(np.float64)
    r = np.zeros_like(w)
    m = regularized_mask(net, o)
    r[m] = float(np.float32(o.l1)) * np.sign(w[m]) + (2.0 * float(np.float32(o.l2))) * w[m]
    return r


def add_reg(net, g, w, o, f=np.float64):
    """g' = g + r, the sum taken in float64 and rounded once to f"""
    return (np.asarray(g, f).astype(np.float64) + reg_grad(net, w, o, f)).astype(f)


def reg_loss(net, w, o):
    """step 5: R = l1 sum |w| + l2 sum w^2 over the regularised tensors, in float64"""
    x = np.asarray(w, np.float64)[regularized_mask(net, o)]
    return float(np.float32(o.l1)) * float(np.abs(x).sum()) + float(np.float32(o.l2)) * float((x * x).sum())


def clip(net, gp, o, f=np.float64):
    """step 2 on g' = g + r: (g'', {"norm": the norm of g' over all trainable tensors, "norms": {tensor: its norm},
    "scales": {tensor: s_T}, "clipped": did anything change}).  Norms in float64; the scale is a float32."""
    gp = np.asarray(gp, f)
    out = gp.copy()
    tr = trainable_mask(net)
    norms = {name: float(np.sqrt((np.asarray(gp[sl], np.float64) ** 2).sum())) for name, sl, cls in tensors(net)
             if cls != "moving"}
    norm = float(np.sqrt((np.asarray(gp[tr], np.float64) ** 2).sum()))
    scales, clipped = {name: np.float32(1.0) for name in norms}, False
    cv, cn, cg = (float(np.float32(x)) for x in (o.clipvalue, o.clipnorm, o.global_clipnorm))
    if cv > 0:
        out[tr] = np.minimum(np.maximum(gp[tr], f(-cv)), f(cv))
        clipped = bool(np.any(np.abs(gp[tr]) > cv))
    elif cn > 0 or cg > 0:
        c = cn if cn > 0 else cg
        for name, sl, cls in tensors(net):
            if cls == "moving":
                continue
            n = norms[name] if cn > 0 else norm
            scales[name] = np.float32(c / max(n, c))
            out[sl] = gp[sl] * f(scales[name])
            clipped = clipped or n > c
    return out, {"norm": norm, "norms": norms, "scales": scales, "clipped": clipped}


def decay(net, w, lr, o, f=np.float64):
    """step 3: w' = w - (lr weight_decay) w on every kernel, trunk and head; w elsewhere"""
    w = np.asarray(w, f).copy()
    k = class_mask(net, KERNELS)
    if np.float32(o.weight_decay) > 0:
        w[k] = w[k] - (f(np.float32(lr)) * f(np.float32(o.weight_decay))) * w[k]
    return w
