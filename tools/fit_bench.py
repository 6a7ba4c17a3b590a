#!/usr/bin/env python3
"""Times the training step of mlp12x100 (csrc/nn_train_mlp.hip) or, with --net rescnn4, of the residual CNN
(csrc/nn_train_conv.hip), both driven by csrc/nn_train.hip, on one GPU: ms per step at `--batch` rows on a sample set
of `--rows` rows, rows/s and achieved FLOP/s against the fp32 matrix peak.  A step is 3 x 253.4 KFLOP per row (3 x 9.65 MFLOP for rescnn4) by the
algorithm (forward, and the two products of the backward pass).  Timing: a synchronised host clock around one
ca_fitter_train call of `--steps` steps (the call ends by reading its losses back).

--torch also times the same step written in torch-ROCm on the same GPU, in the same process, alternating with the HIP
path: autograd through the Keras BatchNorm (batch mean, biased variance), Adam as TF's ResourceApplyAdam (epsilon
outside the root) with torch._foreach ops, moving statistics at momentum 0.99.  For rescnn4 it is the same network
with torch's convolutions and the BatchNorm of the fit (batch mean and biased variance per channel over all rows and
pixels).  It is the yardstick the HIP step has to beat; torch is not part of the product path.

--packed also times the same step, on the same virtual rows in the same order, on a packed data set of rows / 8
un-augmented samples (include/corintho_hip.h, "the packed data set"), alternating with the expanded set in the same
process: what the batch-assembly launch costs.

--handoff measures something else and nothing of the above: the time from a finished fused self-play generation
(--games, --sims, mlp12x100 at random initial weights) to the data set being ready in a fitter, by the two roads in
turn, --reps times: samples_io.get_samples + Fitter.set_data (expand on the device, 8x rows to the host and back), and
Fitter.add_trainer_samples (packed device to device) into an emptied fitter and into one that has the capacity.

--l1, --l2, --regularize, --weight_decay, --clipvalue, --clipnorm, --global_clipnorm: the fit options
(include/corintho_hip.h, "fit options") of the HIP step and of the packed one; the result then carries the options and
the last call's train_stats.  All 0 (the default): the step without them, and no option entry point is called.

--adam default | on: Adam's arguments (include/corintho_hip.h, "Adam's arguments") of the HIP step and of the packed one.
`default` sets the fitter to the Adam defaults through set_adam, which must cost nothing: the step runs the kernels that
know of no arguments.  `on` switches AMSGrad and averaged weights (ema_momentum 0.99) on: the parametrised update kernel
with its third slot and the average.  Not given: no Adam entry point is called (an earlier build has none).

--loss default | on: the loss (include/corintho_hip.h, "loss and metrics") likewise.  `default` sets the reference's loss
through set_loss, which must cost nothing; `on` is loss weights (0.7, 1.3), label smoothing 0.1 and Huber(0.5): the
parametrised loss kernel in ft_k_loss's place.  --metrics switches the metrics on (top 5): two launches more per step.
--lib FILE times another build of the library (the parent commit's, built with `python -m corintho_ai_amd.build --out`).

--augmentation-ab PARENT.so measures something else again: the step on a packed set of rows / 8 samples three ways in
one process, in turn, --reps times -- this library with augmentation "reference", this library with "consistent"
(ft_k_assemble_consistent in ft_k_assemble's place), and the parent commit's library -- and reports each way's ms per
step, the spread (max - min) of the parent's own repetitions, and the consistent step's best minus the parent's best.
The two ways of this library are one fitter whose augmentation is set before every call, so their difference is the
kernel's; the parent's is a fitter of its own (other buffers), and "reference" against it shows what that alone makes.
--ab-two-fitters gives each way of this library a fitter of its own instead.

    python tools/fit_bench.py --torch [--net rescnn4] [--rows 1000000 --batch 2048 --steps 200 --reps 3] [--out file.json]
    python tools/fit_bench.py --packed [--net rescnn4]
    python tools/fit_bench.py --handoff [--games 4096 --sims 400]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from corintho_ai_amd import nets  # noqa: E402
from corintho_ai_amd import NET_MLP12X100, NET_RESCNN4  # noqa: E402
from corintho_ai_amd import _lib  # noqa: E402
from corintho_ai_amd.fit import OPTION_NAMES, AdamOptions, FitOptions, Fitter, LossOptions  # noqa: E402

FLOP_PER_ROW_STEP = {"mlp12x100": 3 * 2.0 * (70 * 100 + 11 * 100 * 100 + 100 * 97),
                     "rescnn4": 3 * nets.rescnn4_flop_per_row()}
PEAK_FP32_MATRIX = 157.3e12
PRODUCTION_STEPS = 12_000  # ~2.5 M training rows x 10 epochs at batch 2048


def samples(n, seed=0):
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 70), np.float32)
    s[:, :64] = rng.integers(0, 2, (n, 64))
    s[:, 64:] = rng.integers(0, 5, (n, 6)) * 0.25
    p = rng.random((n, 96), dtype=np.float32)
    p /= p.sum(1, keepdims=True)
    z = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), n)
    return s, z, p


class TorchStep:
    """the Keras step in torch-ROCm (autograd)"""

    def __init__(self, w, data, device):
        import torch

        self.torch = torch
        self.dev = device
        lay, p, fi = [], 0, 70
        for _ in range(12):
            lay.append((p, fi))
            p += fi * 100 + 500
            fi = 100
        self.lay, self.head = lay, p
        W = torch.tensor(w, device=device)
        self.params, self.stats = [], []
        for k, fi in lay:
            b = k + fi * 100
            self.params += [W[k:b].view(fi, 100).clone(), W[b:b + 100].clone(), W[b + 100:b + 200].clone(),
                            W[b + 200:b + 300].clone()]
            self.stats += [W[b + 300:b + 400].clone(), W[b + 400:b + 500].clone()]
        h = self.head
        self.params += [W[h:h + 100].view(100, 1).clone(), W[h + 100:h + 101].clone(),
                        W[h + 101:h + 9701].view(100, 96).clone(), W[h + 9701:h + 9797].clone()]
        for q in self.params:
            q.requires_grad_(True)
        self.m = [torch.zeros_like(q) for q in self.params]
        self.v = [torch.zeros_like(q) for q in self.params]
        self.it = 0
        self.s, self.z, self.p = (torch.tensor(a, device=device) for a in data)

    def step(self, rows, lr=1e-3):
        torch = self.torch
        x = self.s[rows]
        P = self.params
        batch_stats = []
        for i in range(12):
            k, b, g, be = P[4 * i:4 * i + 4]
            a = torch.relu(x @ k + b)
            mu = a.mean(0)
            var = ((a - mu) ** 2).mean(0)
            batch_stats += [mu.detach(), var.detach()]
            x = g * ((a - mu) * torch.rsqrt(var + 1e-3)) + be
        kv, bv, kp, bp = P[48:]
        v = (x @ kv).view(-1) + bv
        logits = x @ kp + bp
        loss = ((torch.tanh(v) - self.z[rows]) ** 2).mean() + 0.25 * (
            -(self.p[rows] * torch.log_softmax(logits, 1)).sum(1)).mean()
        grads = torch.autograd.grad(loss, P)
        self.batch_stats = batch_stats
        _adam(self, grads, lr)
        return loss


def _adam(ts, grads, lr):
    """TF ResourceApplyAdam on ts.params and the moving statistics toward ts.batch_stats, with torch._foreach ops"""
    torch = ts.torch
    with torch.no_grad():
        ts.it += 1
        t = np.float32(ts.it)
        lr_t = float(np.float32(lr) * np.sqrt(np.float32(1) - np.float32(0.999) ** t) / (np.float32(1) - np.float32(0.9) ** t))
        torch._foreach_lerp_(ts.m, grads, 1 - 0.9)
        torch._foreach_lerp_(ts.v, torch._foreach_mul(grads, grads), 1 - 0.999)
        den = torch._foreach_sqrt(ts.v)
        torch._foreach_add_(den, 1e-7)
        torch._foreach_addcdiv_(ts.params, ts.m, den, value=-lr_t)
        torch._foreach_lerp_(ts.stats, ts.batch_stats, 0.01)


class TorchStepCnn:
    """rescnn4's step in torch-ROCm (autograd): NCHW convolutions with OIHW kernels, the fit's BatchNorm"""

    def __init__(self, w, data, device):
        import torch

        self.torch = torch
        self.dev = device
        W = nets.rescnn4_unpack(w)
        self.P, self.S = {}, {}
        for name, a in W.items():
            t = torch.tensor(a, device=device)
            if a.ndim == 4:
                t = t.permute(3, 2, 0, 1).contiguous()  # HWIO -> OIHW
            elif name in ("p_k", "v_k"):
                t = t.t().contiguous().view(a.shape[1], a.shape[0], 1, 1)
            if name.endswith("_bn2") or name.endswith("_bn3"):
                self.S[name] = t
            else:
                self.P[name] = t.requires_grad_(True)
        self.params, self.stats = list(self.P.values()), list(self.S.values())
        self.m = [torch.zeros_like(q) for q in self.params]
        self.v = [torch.zeros_like(q) for q in self.params]
        self.it = 0
        self.s, self.z, self.p = (torch.tensor(a, device=device) for a in data)

    def step(self, rows, lr=1e-3):
        torch = self.torch
        F = torch.nn.functional
        P = self.P
        st = {}

        def cbr(x, pre, pad, res=None):
            z = F.conv2d(x, P[pre + "_k"], P[pre + "_b"], padding=pad)
            mu = z.mean((0, 2, 3))
            var = ((z - mu.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
            st[pre + "_bn2"], st[pre + "_bn3"] = mu.detach(), var.detach()
            y = P[pre + "_bn0"].view(1, -1, 1, 1) * ((z - mu.view(1, -1, 1, 1)) * torch.rsqrt(var.view(1, -1, 1, 1) + 1e-3)) \
                + P[pre + "_bn1"].view(1, -1, 1, 1)
            return torch.relu(y if res is None else y + res)

        s = self.s[rows]
        n = s.shape[0]
        x = torch.cat([s[:, :64].view(n, 16, 4), s[:, None, 64:70].expand(n, 16, 6)], 2).view(n, 4, 4, 10).permute(0, 3, 1, 2)
        h = cbr(x, "stem", 1)
        for b in range(4):
            h = cbr(cbr(h, "b%d_c1" % b, 1), "b%d_c2" % b, 1, res=h)
        pa = cbr(h, "p", 0).permute(0, 2, 3, 1).reshape(n, 64)
        logits = pa @ P["p_dk"] + P["p_db"]
        va = cbr(h, "v", 0).permute(0, 2, 3, 1).reshape(n, 32)
        v = (torch.relu(va @ P["v_d1k"] + P["v_d1b"]) @ P["v_d2k"]).view(-1) + P["v_d2b"]
        loss = ((torch.tanh(v) - self.z[rows]) ** 2).mean() + 0.25 * (
            -(self.p[rows] * torch.log_softmax(logits, 1)).sum(1)).mean()
        grads = torch.autograd.grad(loss, self.params)
        self.batch_stats = [st[k] for k in self.S]
        _adam(self, grads, lr)
        return loss


def handoff(a):
    """one generation, then the two roads to a ready data set in turn; -> the result record"""
    from corintho_ai_amd import Trainer, samples_io

    t = Trainer(a.games, "", 12345, a.sims, 16, 1.0, 0.25, 0, 1, False, device=a.device, stagger=False)
    t.set_net(NET_MLP12X100, nets.init_mlp12x100(0, bn_noise=True))
    t0 = time.perf_counter()
    if not t.run():
        raise SystemExit("fit_bench: the generation did not finish")
    generation_ms = (time.perf_counter() - t0) * 1e3
    n = t.num_samples()
    old, new, warm = [], [], []
    with Fitter(max_batch=a.batch, device=a.device) as fe, Fitter(max_batch=a.batch, device=a.device) as fp:
        for rep in range(a.reps + 1):  # the first round is the warm-up
            t0 = time.perf_counter()
            fe.set_data(*samples_io.get_samples(t))
            t1 = time.perf_counter()
            fp.clear_data()
            got = fp.add_trainer_samples(t)
            t2 = time.perf_counter()
            fp.drop_samples(got)  # the window slid: the capacity stays
            t3 = time.perf_counter()
            fp.add_trainer_samples(t)
            t4 = time.perf_counter()
            assert got == n and fe.data_info() == (8 * n, 0) and fp.data_info() == (8 * n, n)
            if rep:
                old.append((t1 - t0) * 1e3)
                new.append((t2 - t1) * 1e3)
                warm.append((t4 - t3) * 1e3)
    t.close()
    return {"handoff": {"games": a.games, "sims": a.sims, "samples": n, "rows": 8 * n, "generation_ms": generation_ms,
                        "expanded_bytes": 8 * n * 167 * 4, "packed_bytes": n * 167 * 4,
                        "get_samples_set_data_ms": min(old), "get_samples_set_data_ms_all": old,
                        "add_trainer_samples_ms": min(new), "add_trainer_samples_ms_all": new,
                        "add_trainer_samples_warm_ms": min(warm), "add_trainer_samples_warm_ms_all": warm,
                        "speedup": min(old) / min(new)}}


def augmentation_ab(a):
    """the packed step by this library under both augmentations and by the parent's library, alternating"""
    import ctypes as C

    from corintho_ai_amd.fit import net_info

    net = NET_RESCNN4 if a.net == "rescnn4" else NET_MLP12X100
    w = nets.init_rescnn4(0, bn_noise=True) if a.net == "rescnn4" else nets.init_mlp12x100(0, bn_noise=True)
    k = a.rows // 8
    s, z, p = samples(k)
    sp = np.concatenate([s, p], axis=1)
    parent = Fitter.__new__(Fitter)  # a Fitter served by the other build, which lacks the newer entry points
    parent.net, parent.num_weights, parent._L, parent._h, parent.max_batch, parent._data = (
        net, net_info(net)[1], _lib.declare(C.CDLL(os.path.abspath(a.augmentation_ab))), C.c_void_p(), a.batch, None)
    _lib.check(parent._L, parent._L.ca_fitter_create_net(a.device, int(net), a.batch, C.byref(parent._h)))
    mine = Fitter(max_batch=a.batch, device=a.device, net=net)
    other = Fitter(max_batch=a.batch, device=a.device, net=net) if a.ab_two_fitters else mine
    ways = [("reference", mine), ("consistent", other), ("parent library", parent)]
    fitters = [mine, parent] + ([other] if other is not mine else [])
    rng = np.random.default_rng(1)
    need = (a.steps + a.warmup) * a.batch
    order = np.concatenate([rng.permutation(8 * k) for _ in range(-(-need // (8 * k)))])[:need].astype(np.int32)
    for f in fitters:
        f.add_samples(sp, z)
        f.set_weights(w)
        f.set_optimizer(np.zeros_like(w), np.zeros_like(w), 0)
    for name, f in ways:
        if f is not parent:
            f.set_augmentation(name)
        f.train(order[:a.warmup * a.batch], a.batch, 1e-3)
    ms = {name: [] for name, _ in ways}
    for _ in range(a.reps):
        for name, f in ways:
            if f is not parent:
                f.set_augmentation(name)
            t0 = time.perf_counter()
            f.train(order[a.warmup * a.batch:], a.batch, 1e-3)
            ms[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
    for f in fitters:
        f.close()
    return {"two_fitters": bool(a.ab_two_fitters), "net": a.net, "batch": a.batch, "samples": k, "steps": a.steps, "reps": a.reps, "ms_per_step": ms,
            "best": {n: min(v) for n, v in ms.items()}, "median": {n: float(np.median(v)) for n, v in ms.items()},
            "parent_spread_ms": max(ms["parent library"]) - min(ms["parent library"]),
            "consistent_minus_parent_ms": min(ms["consistent"]) - min(ms["parent library"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", choices=("mlp12x100", "rescnn4"), default="mlp12x100")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch", action="store_true")
    ap.add_argument("--packed", action="store_true", help="also time the step on a packed set of rows / 8 samples")
    ap.add_argument("--handoff", action="store_true", help="time generation -> ready data set by both roads instead")
    ap.add_argument("--games", type=int, default=4096, help="--handoff: games of the generation")
    ap.add_argument("--sims", type=int, default=400, help="--handoff: searches per move")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="")
    for name in OPTION_NAMES:  # the fit options (fit.FitOptions); all 0: the step without them
        ap.add_argument("--" + name, type=float, default=0.0)
    ap.add_argument("--regularize", type=int, choices=(0, 1), default=0)
    ap.add_argument("--adam", choices=("default", "on"), default=None,
                    help="set Adam's arguments: the defaults, or AMSGrad and averaged weights on")
    ap.add_argument("--loss", choices=("default", "on"), default=None,
                    help="set the loss: the reference's, or loss weights, label smoothing and Huber on")
    ap.add_argument("--metrics", action="store_true", help="switch the metrics on")
    ap.add_argument("--lib", default="", help="another build of libcorintho_hip.so to time")
    ap.add_argument("--augmentation-ab", default="", metavar="PARENT.so",
                    help="time the packed step under both augmentations and by this build of the parent commit instead")
    ap.add_argument("--ab-two-fitters", action="store_true", help="--augmentation-ab: a fitter of its own for each way")
    a = ap.parse_args()
    if a.augmentation_ab:
        emit(augmentation_ab(a), a.out)
        return
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    loss = {None: None, "default": LossOptions(),
            "on": LossOptions(value_weight=0.7, policy_weight=1.3, label_smoothing=0.1, value_loss="huber", huber_delta=0.5)}[a.loss]
    adam = {None: None, "default": AdamOptions(), "on": AdamOptions(amsgrad=True, ema_momentum=0.99)}[a.adam]
    options = FitOptions(regularize=a.regularize, **{k: getattr(a, k) for k in OPTION_NAMES}).check()
    if a.handoff:
        emit(handoff(a), a.out)
        return
    if a.packed and a.rows % 8:
        raise SystemExit("fit_bench: --packed needs --rows to be a multiple of 8")
    data = samples(a.rows)
    cnn = a.net == "rescnn4"
    w = nets.init_rescnn4(0, bn_noise=True) if cnn else nets.init_mlp12x100(0, bn_noise=True)
    flop_per_row_step = FLOP_PER_ROW_STEP[a.net]
    rng = np.random.default_rng(1)
    need = (a.steps + a.warmup) * a.batch
    if max(a.steps, a.warmup) * a.batch > a.rows:
        raise SystemExit("fit_bench: one call trains at most --rows rows (an epoch): raise --rows or lower --steps")
    order = np.concatenate([rng.permutation(a.rows) for _ in range(-(-need // a.rows))])[:need].astype(np.int32)
    ts = None
    if a.torch:  # torch's runtime comes up first, before the engine library opens the device
        import torch

        ts = (TorchStepCnn if cnn else TorchStep)(w, data, "cuda:%d" % a.device)
        torder = torch.tensor(order.astype(np.int64), device=ts.dev)
    f = Fitter(max_batch=a.batch, device=a.device, net=NET_RESCNN4 if cnn else NET_MLP12X100)
    f.set_data(*data)
    f.set_weights(w)
    f.set_optimizer(np.zeros_like(w), np.zeros_like(w), 0)
    if options.any():  # (asked only then: an earlier build of the library has no options)
        f.set_options(options)
    if adam is not None:  # (likewise)
        f.set_adam(adam)
    if loss is not None:  # (likewise)
        f.set_loss(loss)
    if a.metrics:
        f.set_metrics(True)
    f.train(order[:a.warmup * a.batch], a.batch, 1e-3)
    if ts:
        for i in range(a.warmup):
            ts.step(torder[i * a.batch:(i + 1) * a.batch])
        torch.cuda.synchronize(ts.dev)
    fp = None
    if a.packed:  # the first rows / 8 rows as un-augmented samples: as many virtual rows as the expanded set has rows
        fp = Fitter(max_batch=a.batch, device=a.device, net=NET_RESCNN4 if cnn else NET_MLP12X100)
        k = a.rows // 8
        fp.add_samples(np.concatenate([data[0][:k], data[2][:k]], axis=1), data[1][:k])
        fp.set_weights(w)
        fp.set_optimizer(np.zeros_like(w), np.zeros_like(w), 0)
        if options.any():
            fp.set_options(options)
        if adam is not None:
            fp.set_adam(adam)
        if loss is not None:
            fp.set_loss(loss)
        if a.metrics:
            fp.set_metrics(True)
        fp.train(order[:a.warmup * a.batch], a.batch, 1e-3)
    hip, tor, pak = [], [], []
    timed = order[a.warmup * a.batch:]
    for _ in range(a.reps):
        t0 = time.perf_counter()
        f.train(timed, a.batch, 1e-3)
        hip.append((time.perf_counter() - t0) * 1e3 / a.steps)
        if fp:
            t0 = time.perf_counter()
            fp.train(timed, a.batch, 1e-3)
            pak.append((time.perf_counter() - t0) * 1e3 / a.steps)
        if ts:
            torch.cuda.synchronize(ts.dev)
            t0 = time.perf_counter()
            for i in range(a.steps):
                ts.step(torder[(a.warmup + i) * a.batch:(a.warmup + i + 1) * a.batch])
            torch.cuda.synchronize(ts.dev)
            tor.append((time.perf_counter() - t0) * 1e3 / a.steps)
    stats = f.train_stats() if options.any() else None
    metrics = f.metrics() if a.metrics else None
    f.close()
    if fp:
        fp.close()

    def rec(ms):
        best = min(ms)
        flops = flop_per_row_step * a.batch / (best * 1e-3)
        return {"ms_per_step": best, "ms_per_step_all": ms, "rows_per_s": a.batch / (best * 1e-3), "flop_per_s": flops,
                "share_of_fp32_matrix_peak": flops / PEAK_FP32_MATRIX,
                "production_fit_s": best * 1e-3 * PRODUCTION_STEPS}

    out = {"net": a.net, "batch": a.batch, "rows": a.rows, "steps": a.steps, "flop_per_row_step": flop_per_row_step,
           "hip": rec(hip)}
    if stats:
        out["options"] = options.as_dict()
        out["train_stats"] = stats
    if adam is not None:
        out["adam"] = adam.as_dict()
    if loss is not None:
        out["loss"] = loss.as_dict()
    if metrics:
        out["metrics"] = metrics
    if tor:
        out["torch"] = rec(tor)
        out["hip_speedup_over_torch"] = min(tor) / min(hip)
    if pak:
        out["packed"] = rec(pak)
        out["packed_over_expanded"] = min(pak) / min(hip)
    emit(out, a.out)


def emit(out, path):
    line = json.dumps(out)
    print(line)
    if path:
        with open(path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
