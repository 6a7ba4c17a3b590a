"""Network training on the device: the reference's Keras `model.fit` step (corintho_ai/python/main.pyx:221-272,
model and compile of wrapper.py:256-282) for mlp12x100, with the HIP kernels of csrc/nn_train_mlp.hip; and the same
recipe for rescnn4 (`net=NET_RESCNN4`, csrc/nn_train_conv.hip), whose BatchNorms take batch statistics per channel over
all (row, pixel) pairs.  The step driver, the loss and Adam are shared by both networks (csrc/nn_train.hip).

    res = fit(weights, game_states, eval_labels, prob_labels, epochs=10)
    trainer.set_net(NET_MLP12X100, res.best_weights)

The arrays are what samples_io.samples_for_training returns.  What Keras does and what is reproduced here:
  * the last `validation_split` of the rows validate, split before any shuffling (floor(n * (1 - split)) train);
  * every epoch the training rows go in a fresh permutation, in batches of `batch_size` (the last one partial).
    Keras's shuffle generator cannot be matched: the permutation is numpy's, seeded by `seed`;
  * Adam (TF ResourceApplyAdam, epsilon 1e-7) on MSE(value) + 0.25 x categorical cross-entropy(policy), BatchNorm
    in training mode with moving statistics at momentum 0.99 (the device kernels, DESIGN.md "Network training");
  * ModelCheckpoint(monitor="val_loss", save_best_only=True): the weights and optimizer state at the end of the first
    epoch whose val_loss is strictly below every earlier one;
  * ReduceLROnPlateau(factor=anneal_factor, patience=patience), min_delta 1e-4, no cooldown, no min_lr.

The samples need not leave the device, nor be held 8 times over.  A Fitter's data set can be PACKED: the un-augmented
rows of Trainer.export_samples (state_policy [n, 166], outcome [n]), whose 8 n virtual rows -- row v is sample v // 8
under symmetry v % 8, the row order of Trainer.writeSamples and expand_samples -- are produced batch by batch on the
device (DESIGN.md "Network training", "The packed data set"):

    fitter = Fitter(max_batch=2048)
    for generation in ...:
        trainer.run()
        fitter.add_trainer_samples(trainer)              # device to device, 668 bytes a sample
        res = fit_resident(fitter, weights, epochs=10)
        fitter.drop_samples(...)                         # slide the replay window

fit_samples(w, sp, oc, seed=s) equals fit(w, *expand_samples(sp, oc), seed=s) to the bit, and fit_trainer(w, t) equals
fit(w, *samples_io.get_samples(t)): the row order is the same, so the validation split and the permutations are, and a
step on virtual rows reads the floats the expanded arrays hold.

Samples may carry weights, Keras's model.fit(sample_weight=...): a batch's losses are (1/B) sum_r w_r loss_r, BatchNorm
statistics stay unweighted (fit(..., sample_weight=w), fit_samples(..., sample_weight=w), Fitter.set_sample_weights).
Fitter.merge_duplicates merges the duplicate positions of a packed set on the device into one weighted sample each
(DESIGN.md "Merging duplicate positions"; samples_io.merge_duplicates_host is its definition).  A set without weights
is fitted by the kernels that know of none.

Fit options (FitOptions; include/corintho_hip.h "fit options" is the definition): what the reference's model declares and
leaves at zero -- kernel_regularizer=L1L2() on its hidden Dense layers -- and what its Adam's constructor takes:
    res = fit_resident(fitter, weights, options=FitOptions(l2=1e-4, weight_decay=1e-4, global_clipnorm=1.0))
l1, l2: the regulariser, on the trunk kernels (regularize=0) or on all kernels (1); its R(w) is part of "loss" and
"val_loss", as Keras adds layer losses.  weight_decay: decoupled, on the kernels, times the learning rate.  clipvalue,
clipnorm (per tensor), global_clipnorm: at most one.  Everything runs in the device's step (csrc/nn_train_opt.hip); with
every option 0 a step is what it is without them, kernel for kernel and bit for bit.  fit_resident puts the fitter into
the state its call asks for: options=None switches a Fitter's options off.  With an option on, `history` gains
"regularization_loss", "grad_norm" (both means over the epoch's steps) and "clipped_steps", one entry per epoch.

Adam's arguments (AdamOptions; include/corintho_hip.h "Adam's arguments" is the definition): beta_1, beta_2, epsilon,
amsgrad (a third slot, "vhat") and averaged weights (Keras's use_ema, ema_momentum, ema_overwrite_frequency):
    res = fit_resident(fitter, weights, adam=AdamOptions(beta_2=0.99, amsgrad=True, ema_momentum=0.99))
adam=None means the defaults, and a fitter left with other values is set back.  With ema_momentum > 0 a fit is Keras 3's
SwapEMAWeights(swap_on_epoch=True) plus the finalisation its fit() does: every epoch is judged by the averaged weights
(swap, evaluate, swap back), so "val_loss", the best-epoch checkpoint and the plateau rule see those numbers and
best_weights are the averaged weights of the best epoch; at the end the average is applied, so `weights` and the fitter
hold it.  With every argument at its default a step is what it is without them, kernel for kernel and bit for bit.

The loss and the metrics (LossOptions; include/corintho_hip.h "loss and metrics" is the definition): the other half of
the reference's model.compile() -- loss_weights, CategoricalCrossentropy(label_smoothing=), Huber(delta) on the value head
and metrics=:
    res = fit_resident(fitter, weights, loss=LossOptions(value_weight=0.7, policy_weight=1.3, label_smoothing=0.1,
                                                         value_loss="huber", huber_delta=0.5), metrics={"top_k": 3})
"loss" and "val_loss" are value_weight x value + policy_weight x policy (+ R), and the checkpoint and the plateau rule see
them; "value_loss" and "policy_loss" stay the means of the two terms.  loss=None means the reference's loss, decided by
the call.  With metrics the history gains METRIC_HISTORY_KEYS, one entry per epoch: how often the network's best move is
the target's (and within its top k), the value head's mean absolute error, and the entropies of the policy and of its
target -- during the epoch from each step's own forward, as Keras logs them, and "val_" + each from the validation pass
(the averaged weights' with ema_momentum > 0).  They come from two launches on the head outputs a step already has;
with metrics off nothing is launched, and on or off the losses and the weights of a fit are the same bytes.
Fitter.predict(rows) reads the heads themselves.
"""
import ctypes as C
import inspect
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .nets import GAME_STATE_SIZE, MLP_NUM_WEIGHTS, NUM_MOVES, RESCNN4_NUM_WEIGHTS
from .trainer import NET_MLP12X100, NET_RESCNN4, Trainer

SAMPLE_FLOATS = GAME_STATE_SIZE + NUM_MOVES  # a packed row: state[70], policy[96]
MIN_DELTA = 1e-4  # keras.callbacks.ReduceLROnPlateau default
NETS = {NET_MLP12X100: ("mlp12x100", MLP_NUM_WEIGHTS), NET_RESCNN4: ("rescnn4", RESCNN4_NUM_WEIGHTS)}


def net_info(net):
    """(name, number of weights) of a trainable network kind"""
    if net not in NETS:
        raise ValueError("fit: net must be NET_MLP12X100 or NET_RESCNN4, got %r" % (net,))
    return NETS[net]


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None and a.shape != shape:
        a = a.reshape(shape)
    return a


def _ptr(a, t=C.c_float):
    return a.ctypes.data_as(C.POINTER(t))


def _packed(state_policy, outcome, who):
    """the two arrays of a packed sample set, checked"""
    sp = np.ascontiguousarray(state_policy, dtype=np.float32)
    if sp.ndim != 2 or sp.shape[1] != SAMPLE_FLOATS:
        raise ValueError("%s: state_policy must be [n, %d]" % (who, SAMPLE_FLOATS))
    oc = np.ascontiguousarray(outcome, dtype=np.float32).ravel()
    if oc.size != sp.shape[0]:
        raise ValueError("%s: outcome must be [n] for n = %d, got %d" % (who, sp.shape[0], oc.size))
    return sp, oc


OPTION_NAMES = ("l1", "l2", "weight_decay", "clipvalue", "clipnorm", "global_clipnorm")
OPTION_HISTORY_KEYS = ("regularization_loss", "grad_norm", "clipped_steps")


@dataclass(frozen=True)
class FitOptions:
    """ca_fit_options: every value 0 is off.  The device takes the values in float32."""
    l1: float = 0.0
    l2: float = 0.0
    regularize: int = 0          # 0: l1 and l2 on the trunk kernels, 1: on all kernels
    weight_decay: float = 0.0
    clipvalue: float = 0.0
    clipnorm: float = 0.0
    global_clipnorm: float = 0.0

    def check(self):
        """ValueError unless the options are ones the device takes; returns self"""
        for k in OPTION_NAMES:
            x = getattr(self, k)
            if not isinstance(x, (int, float, np.floating, np.integer)) or not np.isfinite(x) or x < 0:
                raise ValueError("fit options: %s must be finite and >= 0, got %r" % (k, x))
            with np.errstate(over="ignore"):
                narrow = np.float32(x)
            if not np.isfinite(narrow):
                raise ValueError("fit options: %s = %r is not finite in float32" % (k, x))
        if self.regularize not in (0, 1):
            raise ValueError("fit options: regularize must be 0 (trunk kernels) or 1 (all kernels), got %r" % (self.regularize,))
        if sum(1 for k in ("clipvalue", "clipnorm", "global_clipnorm") if np.float32(getattr(self, k)) > 0) > 1:
            raise ValueError("fit options: at most one of clipvalue, clipnorm and global_clipnorm may be set")
        return self

    def any(self):
        """is any option on (in float32, as the device sees them)"""
        return any(np.float32(getattr(self, k)) > 0 for k in OPTION_NAMES)

    def as_dict(self):
        d = {k: float(getattr(self, k)) for k in OPTION_NAMES}
        d["regularize"] = int(self.regularize)
        return d


ADAM_NAMES = ("beta_1", "beta_2", "epsilon", "amsgrad", "ema_momentum", "ema_overwrite_frequency")
SLOTS = {"vhat": 0, "average": 1}  # CA_SLOT_VHAT, CA_SLOT_AVERAGE


@dataclass(frozen=True)
class AdamOptions:
    """ca_fit_adam: the defaults are Keras Adam's.  The device takes the floats in float32."""
    beta_1: float = 0.9
    beta_2: float = 0.999
    epsilon: float = 1e-7
    amsgrad: bool = False
    ema_momentum: float = 0.0    # 0: no averaged weights
    ema_overwrite_frequency: int = 0

    def check(self):
        """ValueError unless the arguments are ones the device takes (judged in float32, as it does); returns self"""
        for k in ("beta_1", "beta_2", "epsilon", "ema_momentum"):
            x = getattr(self, k)
            if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.floating, np.integer)) or not np.isfinite(x):
                raise ValueError("adam: %s must be a finite number, got %r" % (k, x))
        with np.errstate(over="ignore", under="ignore"):
            b1, b2, eps, mom = (np.float32(getattr(self, k)) for k in ("beta_1", "beta_2", "epsilon", "ema_momentum"))
        for k, x in (("beta_1", b1), ("beta_2", b2), ("ema_momentum", mom)):
            if not 0 <= x < 1:
                raise ValueError("adam: %s must lie in [0, 1) in float32, got %r" % (k, getattr(self, k)))
        if not (np.isfinite(eps) and eps > 0):
            raise ValueError("adam: epsilon must be finite and > 0 in float32, got %r" % (self.epsilon,))
        if not isinstance(self.amsgrad, (bool, np.bool_)) and self.amsgrad not in (0, 1):
            raise ValueError("adam: amsgrad must be a bool, got %r" % (self.amsgrad,))
        k = self.ema_overwrite_frequency
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or k < 0 or k >= 2 ** 31:
            raise ValueError("adam: ema_overwrite_frequency must be an integer >= 0, got %r" % (k,))
        if k > 0 and not mom > 0:
            raise ValueError("adam: ema_overwrite_frequency needs ema_momentum > 0")
        return self

    def is_default(self):
        """is every argument at its default (in float32, as the device sees them)"""
        d = AdamOptions()
        return (all(np.float32(getattr(self, k)) == np.float32(getattr(d, k)) for k in ("beta_1", "beta_2", "epsilon"))
                and not self.amsgrad and not self.averaged())

    def averaged(self):
        return bool(np.float32(self.ema_momentum) > 0)

    def as_dict(self):
        return {"beta_1": float(self.beta_1), "beta_2": float(self.beta_2), "epsilon": float(self.epsilon),
                "amsgrad": bool(self.amsgrad), "ema_momentum": float(self.ema_momentum),
                "ema_overwrite_frequency": int(self.ema_overwrite_frequency)}


def _adam(adam):
    """None or an AdamOptions (or a mapping of its fields), checked; None stays None"""
    if adam is None:
        return None
    if isinstance(adam, dict):
        unknown = sorted(set(adam) - set(ADAM_NAMES))
        if unknown:
            raise ValueError("adam: unknown %s" % ", ".join(unknown))
        adam = AdamOptions(**adam)
    if not isinstance(adam, AdamOptions):
        raise ValueError("fit: adam must be an AdamOptions, a dict of its fields or None, got %r" % (adam,))
    return adam.check()


def _apply_adam(be, adam):
    """as _apply_options: a backend that has set_adam gets the call's arguments (None: the defaults); one that has none
    serves only a call that asks for the defaults.  Returns the AdamOptions if any is off its default, else None"""
    on = adam is not None and not adam.is_default()
    if inspect.getattr_static(be, "set_adam", None) is not None:
        be.set_adam(adam if adam is not None else AdamOptions())
    elif on:
        raise ValueError("fit: the backend %s has no set_adam" % type(be).__name__)
    return adam if on else None


LOSS_NAMES = ("value_weight", "policy_weight", "label_smoothing", "value_loss", "huber_delta")
VALUE_LOSSES = {"mse": 0, "huber": 1}  # CA_VALUE_LOSS_MSE, CA_VALUE_LOSS_HUBER
METRIC_NAMES = ("categorical_accuracy", "top_k_categorical_accuracy", "mean_absolute_error", "policy_entropy",
                "target_entropy")  # ca_fit_metrics' fields, and the keys of Fitter.metrics()
# what a fit's history calls them (Keras's names for a model whose outputs are "policy" and "value"), then their val_ forms
METRIC_KEYS = ("policy_categorical_accuracy", "policy_top_k_categorical_accuracy", "value_mean_absolute_error",
               "policy_entropy", "target_entropy")
METRIC_HISTORY_KEYS = METRIC_KEYS + tuple("val_" + k for k in METRIC_KEYS)
DEFAULT_TOP_K = 5


@dataclass(frozen=True)
class LossOptions:
    """ca_fit_loss: the defaults are the reference's compile(): MSE + 0.25 x cross-entropy.  The device takes the floats
    in float32."""
    value_weight: float = 1.0
    policy_weight: float = 0.25
    label_smoothing: float = 0.0
    value_loss: str = "mse"      # or "huber"
    huber_delta: float = 1.0     # read only with "huber"

    def check(self):
        """ValueError unless the values are ones the device takes (judged in float32, as it does); returns self"""
        for k in ("value_weight", "policy_weight", "label_smoothing", "huber_delta"):
            x = getattr(self, k)
            if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.floating, np.integer)) or not np.isfinite(x):
                raise ValueError("loss: %s must be a finite number, got %r" % (k, x))
        with np.errstate(over="ignore", under="ignore"):
            vw, pw, ls, delta = (np.float32(getattr(self, k)) for k in ("value_weight", "policy_weight", "label_smoothing",
                                                                        "huber_delta"))
        for k, x in (("value_weight", vw), ("policy_weight", pw)):
            if not (np.isfinite(x) and x >= 0):
                raise ValueError("loss: %s must be finite and >= 0 in float32, got %r" % (k, getattr(self, k)))
        if vw == 0 and pw == 0:
            raise ValueError("loss: value_weight and policy_weight may not both be 0 (in float32)")
        if not 0 <= ls < 1:
            raise ValueError("loss: label_smoothing must lie in [0, 1) in float32, got %r" % (self.label_smoothing,))
        if not isinstance(self.value_loss, str) or self.value_loss not in VALUE_LOSSES:
            raise ValueError('loss: value_loss must be "mse" or "huber", got %r' % (self.value_loss,))
        if not (np.isfinite(delta) and delta > 0):
            raise ValueError("loss: huber_delta must be finite and > 0 in float32, got %r" % (self.huber_delta,))
        return self

    def is_default(self):
        """is the loss the reference's (in float32, as the device sees it; huber_delta is not read with "mse")"""
        d = LossOptions()
        return (all(np.float32(getattr(self, k)) == np.float32(getattr(d, k)) for k in ("value_weight", "policy_weight",
                                                                                       "label_smoothing"))
                and self.value_loss == "mse")

    def as_dict(self):
        return {"value_weight": float(self.value_weight), "policy_weight": float(self.policy_weight),
                "label_smoothing": float(self.label_smoothing), "value_loss": str(self.value_loss),
                "huber_delta": float(self.huber_delta)}


def _loss(loss):
    """None or a LossOptions (or a mapping of its fields), checked; None stays None"""
    if loss is None:
        return None
    if isinstance(loss, dict):
        unknown = sorted(set(loss) - set(LOSS_NAMES))
        if unknown:
            raise ValueError("loss: unknown %s" % ", ".join(unknown))
        loss = LossOptions(**loss)
    if not isinstance(loss, LossOptions):
        raise ValueError("fit: loss must be a LossOptions, a dict of its fields or None, got %r" % (loss,))
    return loss.check()


def _top_k(metrics):
    """the metrics argument of a fit -- False or None, True, or {"top_k": k} -- as None (off) or k"""
    if metrics is None or metrics is False:
        return None
    if metrics is True:
        return DEFAULT_TOP_K
    if isinstance(metrics, dict):
        unknown = sorted(set(metrics) - {"top_k"})
        if unknown:
            raise ValueError("metrics: unknown %s" % ", ".join(unknown))
        k = metrics.get("top_k", DEFAULT_TOP_K)
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 1 <= k <= NUM_MOVES:
            raise ValueError("metrics: top_k must be an integer in 1..%d, got %r" % (NUM_MOVES, k))
        return int(k)
    raise ValueError('fit: metrics must be False, True or {"top_k": k}, got %r' % (metrics,))


def _apply_loss(be, loss, top_k):
    """as _apply_options: a backend that has set_loss / set_metrics gets what the call asks for (None: the default loss,
    metrics off); one that has neither serves only a call that asks for the defaults.  Returns whether metrics are on"""
    def has(name):
        return inspect.getattr_static(be, name, None) is not None

    if has("set_loss"):
        be.set_loss(loss if loss is not None else LossOptions())
    elif loss is not None and not loss.is_default():
        raise ValueError("fit: the backend %s has no set_loss" % type(be).__name__)
    if has("set_metrics"):
        be.set_metrics(top_k is not None, top_k if top_k is not None else DEFAULT_TOP_K)
    elif top_k is not None:
        raise ValueError("fit: the backend %s has no set_metrics" % type(be).__name__)
    return top_k is not None


def _options(options):
    """None or a FitOptions (or a mapping of its fields), checked; None stays None"""
    if options is None:
        return None
    if isinstance(options, dict):
        unknown = sorted(set(options) - set(OPTION_NAMES + ("regularize",)))
        if unknown:
            raise ValueError("fit options: unknown %s" % ", ".join(unknown))
        options = FitOptions(**options)
    if not isinstance(options, FitOptions):
        raise ValueError("fit: options must be a FitOptions, a dict of its fields or None, got %r" % (options,))
    return options.check()


def _apply_options(be, opts):
    """put the backend into the state the call asks for: a backend that has options gets them (None: all off); one that
    has none serves only a call that asks for none"""
    def has(name):  # (without asking a backend's __getattr__)
        return inspect.getattr_static(be, name, None) is not None

    if has("set_options"):
        be.set_options(opts if opts is not None else FitOptions())
    elif opts is not None and opts.any():
        raise ValueError("fit: the backend %s has no set_options" % type(be).__name__)
    return opts is not None and opts.any() and has("train_stats")


class Fitter:
    """One device's fitter of mlp12x100 or rescnn4 (include/corintho_hip.h, "network training").  Losses come back as
    (value_weight value + policy_weight policy, value, policy): value + 0.25 policy unless set_loss says otherwise."""

    def __init__(self, max_batch=2048, device=0, net=NET_MLP12X100):
        self.net = net
        self.num_weights = net_info(net)[1]
        self._L = _lib.load()
        self._h = C.c_void_p()
        self.max_batch = int(max_batch)
        self._data = None  # the host arrays of the last set_data, if the set is an expanded one
        _lib.check(self._L, self._L.ca_fitter_create_net(int(device), int(net), self.max_batch, C.byref(self._h)))

    def close(self):
        if self._h:
            self._L.ca_fitter_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        _lib.check(self._L, rc)

    def set_weights(self, weights):
        w = _f32(weights).ravel()
        self._check(self._L.ca_fitter_set_weights(self._h, _ptr(w), w.size))

    def get_weights(self):
        w = np.zeros(self.num_weights, np.float32)
        self._check(self._L.ca_fitter_get_weights(self._h, _ptr(w), w.size))
        return w

    def set_optimizer(self, m, v, iterations):
        m, v = _f32(m).ravel(), _f32(v).ravel()
        if m.size != v.size:
            raise ValueError("m and v differ in size")
        self._check(self._L.ca_fitter_set_optimizer(self._h, _ptr(m), _ptr(v), m.size, int(iterations)))

    def get_optimizer(self):
        """(m, v, iterations)"""
        m = np.zeros(self.num_weights, np.float32)
        v = np.zeros(self.num_weights, np.float32)
        it = C.c_int64()
        self._check(self._L.ca_fitter_get_optimizer(self._h, _ptr(m), _ptr(v), m.size, C.byref(it)))
        return m, v, int(it.value)

    def set_data(self, game_states, eval_labels, prob_labels):
        s = _f32(game_states)
        n = s.shape[0] if s.ndim else 0
        s = _f32(s, (n, GAME_STATE_SIZE))
        e = _f32(eval_labels, (n,))
        p = _f32(prob_labels, (n, NUM_MOVES))
        self._data = (s, e, p)  # the device copy is taken at once; kept only for the caller's inspection
        self._check(self._L.ca_fitter_set_data(self._h, _ptr(s), _ptr(e), _ptr(p), n))

    # ---- the packed data set (include/corintho_hip.h, "the packed data set") ----
    def clear_data(self):
        """empty the data set; the next add_* makes it packed"""
        self._data = None
        self._check(self._L.ca_fitter_clear_data(self._h))

    def add_samples(self, state_policy, outcome):
        """append un-augmented samples (Trainer.export_samples' arrays) from the host"""
        sp, oc = _packed(state_policy, outcome, "add_samples")
        self._check(self._L.ca_fitter_add_samples(self._h, _ptr(sp), _ptr(oc), sp.shape[0]))

    def add_device_samples(self, ptr_sp, ptr_oc, n):
        """append n packed rows from device memory of the fitter's device ([n, 166] and [n] float32 at these addresses,
        e.g. a tensor's data_ptr()); what produced them must have finished"""
        self._check(self._L.ca_fitter_add_device_samples(self._h, C.c_void_p(ptr_sp), C.c_void_p(ptr_oc), int(n)))

    def add_trainer_samples(self, trainer):
        """append the samples of a finished training-mode Trainer, device to device; returns how many"""
        n = C.c_int32()
        self._check(self._L.ca_fitter_add_trainer_samples(self._h, trainer._t, C.byref(n)))
        return n.value

    def drop_samples(self, n):
        """remove the n oldest samples; the others keep their order"""
        self._check(self._L.ca_fitter_drop_samples(self._h, int(n)))

    def data_info(self):
        """(addressable rows, packed samples): (8 n, n) of a packed set, (n, 0) of an expanded one"""
        rows, samples = C.c_int32(), C.c_int32()
        self._check(self._L.ca_fitter_data_info(self._h, C.byref(rows), C.byref(samples)))
        return rows.value, samples.value

    def fetch_rows(self, rows):
        """(states, evals, probs) of the batch a step on `rows` would read (diagnostic)"""
        r = np.ascontiguousarray(rows, dtype=np.int32).ravel()
        s = np.zeros((r.size, GAME_STATE_SIZE), np.float32)
        e = np.zeros(r.size, np.float32)
        p = np.zeros((r.size, NUM_MOVES), np.float32)
        self._check(self._L.ca_fitter_fetch_rows(self._h, _ptr(r, C.c_int32), r.size, _ptr(s), _ptr(e), _ptr(p)))
        return s, e, p

    # ---- sample weights and merging of duplicates (include/corintho_hip.h, "sample weights") ----
    def _units(self):
        """how many weights the set takes: its rows (expanded) or its samples (packed)"""
        rows, samples = self.data_info()
        return samples if samples else rows

    def set_sample_weights(self, weights):
        """Keras's sample_weight: one float32 weight per row of an expanded set, per un-augmented sample of a packed
        one (virtual row v has the weight of sample v // 8).  Every weight must be finite and >= 0.  None removes the
        weights: the set is fitted by the unweighted kernels again."""
        if weights is None:
            self._check(self._L.ca_fitter_set_sample_weights(self._h, None, 0))
            return
        w = np.ascontiguousarray(weights, dtype=np.float32).ravel()
        self._check(self._L.ca_fitter_set_sample_weights(self._h, _ptr(w), w.size))

    def get_sample_weights(self):
        """the weights, one per row or sample; ones for a set that carries none"""
        w = np.zeros(self._units(), np.float32)
        self._check(self._L.ca_fitter_get_sample_weights(self._h, _ptr(w), w.size))
        return w

    def merge_duplicates(self, normalize=True):
        """Merge the duplicate positions of a packed set on the device: samples whose 70 state floats have the same
        bits become one sample at the rank of the first of them, with the weighted mean of their policies and outcomes
        (float64 sums over the members in ascending index, rounded once) and the sum W of their weights as its weight
        (samples_io.merge_duplicates_host is the definition, and equals this bit for bit).  normalize: the weights are
        scaled to mean one.  A group whose weights are all 0 has W = 0 and no mean: it is dropped, members and all.
        The set carries weights afterwards, so add_* is refused until clear_data: merge once, after the last add.
        Returns (samples before, samples after)."""
        before, after = C.c_int32(), C.c_int32()
        self._check(self._L.ca_fitter_merge_duplicates(self._h, 1 if normalize else 0, C.byref(before), C.byref(after)))
        return before.value, after.value

    # ---- fit options (include/corintho_hip.h, "fit options") ----
    def set_options(self, options=None):
        """the regulariser, weight decay and clipping of every later step (FitOptions, or a dict of its fields); None:
        all off.  They stay until set again."""
        o = _options(options) or FitOptions()
        c = _lib.CaFitOptions(struct_size=C.sizeof(_lib.CaFitOptions), regularize=int(o.regularize),
                              **{k: float(np.float32(getattr(o, k))) for k in OPTION_NAMES})
        self._check(self._L.ca_fitter_set_options(self._h, C.byref(c)))

    def get_options(self):
        c = _lib.CaFitOptions(struct_size=C.sizeof(_lib.CaFitOptions))
        self._check(self._L.ca_fitter_get_options(self._h, C.byref(c)))
        return FitOptions(regularize=int(c.regularize), **{k: float(getattr(c, k)) for k in OPTION_NAMES})

    def train_stats(self):
        """of the last train(): {"steps", "clipped_steps", "regularization_loss", "grad_norm", "grad_norm_max"} -- the
        means over the steps of R(w) and of the norm of the regularised gradient before clipping, and that norm's
        maximum; zeros when no option is set"""
        c = _lib.CaFitStats(struct_size=C.sizeof(_lib.CaFitStats))
        self._check(self._L.ca_fitter_train_stats(self._h, C.byref(c)))
        return {"steps": int(c.steps), "clipped_steps": int(c.clipped_steps), "regularization_loss": float(c.regularization),
                "grad_norm": float(c.grad_norm), "grad_norm_max": float(c.grad_norm_max)}

    # ---- Adam's arguments, the third slot and the averaged weights (include/corintho_hip.h, "Adam's arguments") ----
    def set_adam(self, adam=None):
        """Adam's arguments of every later step (AdamOptions, or a dict of its fields); None: the defaults.  They stay
        until set again."""
        a = _adam(adam) or AdamOptions()
        c = _lib.CaFitAdam(struct_size=C.sizeof(_lib.CaFitAdam), beta_1=float(np.float32(a.beta_1)),
                           beta_2=float(np.float32(a.beta_2)), epsilon=float(np.float32(a.epsilon)),
                           amsgrad=int(bool(a.amsgrad)), ema_momentum=float(np.float32(a.ema_momentum)),
                           ema_overwrite_frequency=int(a.ema_overwrite_frequency))
        self._check(self._L.ca_fitter_set_adam(self._h, C.byref(c)))

    def get_adam(self):
        c = _lib.CaFitAdam(struct_size=C.sizeof(_lib.CaFitAdam))
        self._check(self._L.ca_fitter_get_adam(self._h, C.byref(c)))
        return AdamOptions(beta_1=float(c.beta_1), beta_2=float(c.beta_2), epsilon=float(c.epsilon), amsgrad=bool(c.amsgrad),
                           ema_momentum=float(c.ema_momentum), ema_overwrite_frequency=int(c.ema_overwrite_frequency))

    @staticmethod
    def _slot(which):
        if which not in SLOTS:
            raise ValueError('the slot must be "vhat" or "average", got %r' % (which,))
        return SLOTS[which]

    def set_slot(self, which, values):
        """install AMSGrad's third slot ("vhat") or the averaged weights ("average", which makes the average valid)"""
        a = _f32(values).ravel()
        self._check(self._L.ca_fitter_set_slot(self._h, self._slot(which), _ptr(a), a.size))

    def get_slot(self, which):
        """"vhat": zeros if no step has used it; "average": an EngineError (CA_ERR_STATE) while there is none"""
        a = np.zeros(self.num_weights, np.float32)
        self._check(self._L.ca_fitter_get_slot(self._h, self._slot(which), _ptr(a), a.size))
        return a

    def swap_average(self):
        """exchange the weights and the average (Keras's SwapEMAWeights)"""
        self._check(self._L.ca_fitter_swap_average(self._h))

    def apply_average(self):
        """the trainable weights become the average (Keras's finalize_variable_values)"""
        self._check(self._L.ca_fitter_apply_average(self._h))

    # ---- the loss, the metrics and predict (include/corintho_hip.h, "loss and metrics") ----
    def set_loss(self, loss=None):
        """the loss of every later step, evaluation and gradients() (LossOptions, or a dict of its fields); None: the
        reference's value MSE + 0.25 policy cross-entropy.  It stays until set again."""
        o = _loss(loss) or LossOptions()
        c = _lib.CaFitLoss(struct_size=C.sizeof(_lib.CaFitLoss), value_weight=float(np.float32(o.value_weight)),
                           policy_weight=float(np.float32(o.policy_weight)),
                           label_smoothing=float(np.float32(o.label_smoothing)), value_loss=VALUE_LOSSES[o.value_loss],
                           huber_delta=float(np.float32(o.huber_delta)))
        self._check(self._L.ca_fitter_set_loss(self._h, C.byref(c)))

    def get_loss(self):
        c = _lib.CaFitLoss(struct_size=C.sizeof(_lib.CaFitLoss))
        self._check(self._L.ca_fitter_get_loss(self._h, C.byref(c)))
        name = {v: k for k, v in VALUE_LOSSES.items()}[int(c.value_loss)]
        return LossOptions(value_weight=float(c.value_weight), policy_weight=float(c.policy_weight),
                           label_smoothing=float(c.label_smoothing), value_loss=name, huber_delta=float(c.huber_delta))

    def set_metrics(self, on=True, top_k=DEFAULT_TOP_K):
        """switch the metrics of train() and evaluate() on or off; top_k in 1..96"""
        self._check(self._L.ca_fitter_set_metrics(self._h, 1 if on else 0, int(top_k)))

    def metrics(self):
        """of the last train() or evaluate(): METRIC_NAMES' means weighted by the sample weights, and "rows",
        "weight_sum" and "top_k"; an EngineError (CA_ERR_STATE) while metrics are off"""
        c = _lib.CaFitMetrics(struct_size=C.sizeof(_lib.CaFitMetrics))
        self._check(self._L.ca_fitter_metrics(self._h, C.byref(c)))
        out = {k: float(getattr(c, k)) for k in METRIC_NAMES}
        out.update(rows=int(c.rows), weight_sum=float(c.weight_sum), top_k=int(c.top_k))
        return out

    def predict(self, rows, train=False):
        """Keras's predict: (logits [n, 96], values [n], pre-tanh) of at most max_batch rows.  train: the rows as one
        training batch, with batch statistics.  Nothing of the fitter changes."""
        r = np.ascontiguousarray(rows, dtype=np.int32).ravel()
        logits = np.zeros((r.size, NUM_MOVES), np.float32)
        values = np.zeros(r.size, np.float32)
        self._check(self._L.ca_fitter_predict(self._h, _ptr(r, C.c_int32), r.size, 1 if train else 0, _ptr(logits),
                                              _ptr(values)))
        return logits, values

    def tensor_table(self):
        """the device's table of the network's tensors: [(offset, floats, class)], class a name of nets.TENSOR_CLASSES;
        nets.tensor_table(name) is the same with the tensors' names"""
        from .nets import TENSOR_CLASSES
        n = C.c_int32()
        self._check(self._L.ca_fitter_tensor_table(self._h, None, 0, C.byref(n)))
        t = np.zeros((n.value, 3), np.int32)
        self._check(self._L.ca_fitter_tensor_table(self._h, _ptr(t, C.c_int32), n.value, C.byref(n)))
        return [(int(o), int(k), TENSOR_CLASSES[c]) for o, k, c in t]

    def train(self, rows, batch_size, learning_rate, batch_losses=False):
        """one epoch over `rows` in that order; returns the three mean losses (and the [batches, 3] per-batch ones)"""
        r = np.ascontiguousarray(rows, dtype=np.int32)
        out = np.zeros(3, np.float64)
        nb = -(-r.size // int(batch_size)) if batch_size > 0 else 0
        per = np.zeros((max(nb, 1), 3), np.float32) if batch_losses else None
        self._check(self._L.ca_fitter_train(self._h, _ptr(r, C.c_int32), r.size, int(batch_size),
                                            float(np.float32(learning_rate)), _ptr(out, C.c_double),
                                            _ptr(per) if per is not None else None))
        return (tuple(out), per) if batch_losses else tuple(out)

    def evaluate(self, row0, n_rows, batch_size):
        out = np.zeros(3, np.float64)
        self._check(self._L.ca_fitter_evaluate(self._h, int(row0), int(n_rows), int(batch_size), _ptr(out, C.c_double)))
        return tuple(out)

    def gradients(self, rows):
        """(gradient of the batch loss in the weight layout, the three losses); no update"""
        r = np.ascontiguousarray(rows, dtype=np.int32)
        g = np.zeros(self.num_weights, np.float32)
        out = np.zeros(3, np.float64)
        self._check(self._L.ca_fitter_gradients(self._h, _ptr(r, C.c_int32), r.size, _ptr(g), _ptr(out, C.c_double)))
        return g, tuple(out)


@dataclass
class FitResult:
    best_weights: np.ndarray      # ModelCheckpoint(save_best_only): the weights of the best epoch
    best_optimizer: tuple         # (m, v, iterations) of that epoch
    best_epoch: int
    weights: np.ndarray           # after the last epoch
    optimizer: tuple
    learning_rate: float          # after the last epoch's ReduceLROnPlateau
    history: dict = field(default_factory=dict)  # one entry per epoch in each list
    # the extra slots in use, by name ("vhat" with amsgrad, "average" with ema_momentum > 0): of the best epoch and after
    # the last one.  None when Adam's arguments ask for neither.
    best_slots: dict = None
    slots: dict = None


HISTORY_KEYS = ("loss", "value_loss", "policy_loss", "val_loss", "val_value_loss", "val_policy_loss", "lr")


def split_index(n, validation_split):
    """keras.engine.data_adapter.train_validation_split: rows [0, split_at) train"""
    return int(np.floor(n * (1.0 - validation_split)))


def epoch_order(rng, n_train, shuffle):
    return rng.permutation(n_train).astype(np.int32) if shuffle else np.arange(n_train, dtype=np.int32)


def _epochs(be, n, split_at, learning_rate, batch_size, epochs, shuffle, anneal_factor, patience, seed, stats=False,
            adam=None, metrics=False):
    """the epochs of model.fit on the n rows the backend holds, rows [0, split_at) training; the callbacks' logic.
    stats: an option is on, the backend's train_stats() of every epoch go to the history.
    adam: the call's AdamOptions if any is off its default.  With ema_momentum > 0 this is Keras 3's
    SwapEMAWeights(swap_on_epoch=True) plus the finalisation fit() does: an epoch is judged by the averaged weights (swap,
    evaluate, swap back), the checkpoint holds them, and at the end the average is applied to the weights.
    metrics: the backend's metrics() of every epoch's train() and evaluate() go to the history (METRIC_HISTORY_KEYS)."""
    averaged = adam is not None and adam.averaged()
    names = (("vhat",) if adam is not None and adam.amsgrad else ()) + (("average",) if averaged else ())

    def slots():
        return {k: be.get_slot(k) for k in names} if names else None

    rng = np.random.default_rng(seed)
    lr = np.float32(learning_rate)
    history = {k: [] for k in HISTORY_KEYS + (OPTION_HISTORY_KEYS if stats else ()) + (METRIC_HISTORY_KEYS if metrics else ())}
    ckpt_best, plateau_best, wait = np.inf, np.inf, 0
    best = None
    for epoch in range(epochs):
        order = epoch_order(rng, split_at, shuffle)
        loss = be.train(order, batch_size, lr)
        if metrics:
            mt = be.metrics()
            for k, name in zip(METRIC_KEYS, METRIC_NAMES):
                history[k].append(float(mt[name]))
        if stats:
            st = be.train_stats()
            for k in OPTION_HISTORY_KEYS:
                history[k].append(st[k])
        if averaged:
            be.swap_average()
        val = be.evaluate(split_at, n - split_at, batch_size)
        if metrics:
            mt = be.metrics()
            for k, name in zip(METRIC_KEYS, METRIC_NAMES):
                history["val_" + k].append(float(mt[name]))
        judged = be.get_weights() if averaged and val[0] < ckpt_best else None
        if averaged:
            be.swap_average()
        for k, x in zip(HISTORY_KEYS, tuple(loss) + tuple(val) + (lr,)):
            history[k].append(float(x))
        val_loss = val[0]
        if val_loss < ckpt_best:  # ModelCheckpoint(save_best_only=True): np.less
            ckpt_best = val_loss
            best = (judged if averaged else be.get_weights(), be.get_optimizer(), epoch, slots())
        if val_loss < plateau_best - MIN_DELTA:  # ReduceLROnPlateau, mode "min"
            plateau_best, wait = val_loss, 0
        else:
            wait += 1
            if wait >= patience:
                lr = np.float32(lr * np.float32(anneal_factor))
                wait = 0
    if best is None:  # every val_loss NaN: Keras saves nothing either; report the starting point
        raise FloatingPointError("fit: no epoch produced a finite val_loss")
    if averaged:
        be.apply_average()
    return FitResult(best_weights=best[0], best_optimizer=best[1], best_epoch=best[2], weights=be.get_weights(),
                     optimizer=be.get_optimizer(), learning_rate=float(lr), history=history, best_slots=best[3],
                     slots=slots())


def _check_fit_args(learning_rate, batch_size, epochs, validation_split, anneal_factor, patience):
    if int(batch_size) != batch_size or batch_size < 1:
        raise ValueError("fit: batch_size must be a positive integer")
    if int(epochs) != epochs or epochs < 1:
        raise ValueError("fit: epochs must be a positive integer")
    if not 0.0 < validation_split < 1.0:
        raise ValueError("fit: validation_split must lie in (0, 1)")
    if not learning_rate > 0.0 or not 0.0 < anneal_factor < 1.0 or int(patience) != patience or patience < 0:
        raise ValueError("fit: learning_rate > 0, anneal_factor in (0, 1) and patience >= 0 are required")


def fit_resident(fitter, weights, *, learning_rate=0.001, batch_size=2048, epochs=1, validation_split=0.3, shuffle=True,
                 anneal_factor=0.5, patience=3, seed=0, optimizer_state=None, options=None, adam=None, slots=None,
                 loss=None, metrics=False):
    """fit() on whatever data set `fitter` holds -- packed (add_samples, add_device_samples, add_trainer_samples) or
    expanded (set_data) -- without touching it: the rows are data_info()'s, the split, the permutations, the checkpoint
    and the plateau logic are fit()'s, and so is the FitResult.  On a packed set of n samples the rows are the 8 n
    virtual rows, so the result equals fit() on expand_samples of the same samples to the bit.  batch_size may not
    exceed the fitter's max_batch.  options: a FitOptions; None: no option, and a fitter that has options is set to all
    off -- the call decides, not what the fitter was left with.  adam: an AdamOptions; None: the defaults, decided by the
    call in the same way.  slots: {"vhat": ..., "average": ...} to resume from (a FitResult's slots), installed after the
    optimizer state; None starts vhat from zeros and the average from `weights`.  loss: a LossOptions; None: the
    reference's loss.  metrics: True or {"top_k": k}: the history gains METRIC_HISTORY_KEYS; False: off.  Both are decided
    by the call in the same way."""
    opts, adam, loss, top_k = _options(options), _adam(adam), _loss(loss), _top_k(metrics)
    w = _f32(weights).ravel()
    num_weights = getattr(fitter, "num_weights", w.size)
    if w.size != num_weights:
        raise ValueError("fit_resident: the fitter's network has %d floats, got %d" % (num_weights, w.size))
    _check_fit_args(learning_rate, batch_size, epochs, validation_split, anneal_factor, patience)
    n = int(fitter.data_info()[0])
    split_at = split_index(n, validation_split)
    if split_at < 1 or split_at >= n:
        raise ValueError("fit_resident: %d rows leave no training or no validation rows at validation_split=%g"
                         % (n, validation_split))
    fitter.set_weights(w)
    if optimizer_state is None:
        fitter.set_optimizer(np.zeros_like(w), np.zeros_like(w), 0)
    else:
        m, v, it = optimizer_state
        fitter.set_optimizer(m, v, it)
    for k in sorted(slots or {}):
        fitter.set_slot(k, slots[k])
    stats = _apply_options(fitter, opts)
    return _epochs(fitter, n, split_at, learning_rate, int(batch_size), int(epochs), shuffle, anneal_factor, patience,
                   seed, stats, _apply_adam(fitter, adam), _apply_loss(fitter, loss, top_k))


def fit_samples(weights, state_policy, outcome, *, batch_size=2048, device=0, net=NET_MLP12X100, sample_weight=None,
                merge_duplicates=False, _backend=None, **kw):
    """fit() from un-augmented samples (Trainer.export_samples, dist.SampleGather.rows): a packed data set, 668 bytes
    a sample on the device instead of 5 344.  fit_samples(w, sp, oc, seed=s) equals fit(w, *expand_samples(sp, oc),
    seed=s) to the bit: the 8 n virtual rows are in expand_samples' row order, so the validation split and every
    epoch's permutation are the same.  sample_weight: one weight per sample (Keras's sample_weight; the sample's 8
    virtual rows share it).  merge_duplicates: Fitter.merge_duplicates(normalize=True) on the set, weights and all,
    before the fit -- the same as fitting samples_io.merge_duplicates_host's three arrays.  Keywords as fit_resident's."""
    name, num_weights = net_info(net)
    if _f32(weights).size != num_weights:
        raise ValueError("fit_samples: %s weights have %d floats, got %d" % (name, num_weights, _f32(weights).size))
    sp, oc = _packed(state_policy, outcome, "fit_samples")
    sw = _sample_weight(sample_weight, sp.shape[0], "fit_samples")

    def add(be):
        be.add_samples(sp, oc)
        if sw is not None:
            be.set_sample_weights(sw)
        if merge_duplicates:
            be.merge_duplicates(normalize=True)

    return _fit_added(add, weights, batch_size, device, net, _backend, kw)


def _sample_weight(sample_weight, n, who):
    """the weights of n rows or samples, checked; None stays None"""
    if sample_weight is None:
        return None
    sw = np.ascontiguousarray(sample_weight, dtype=np.float32).ravel()
    if sw.size != n:
        raise ValueError("%s: sample_weight must be [n] for n = %d, got %d" % (who, n, sw.size))
    if not np.all(np.isfinite(sw)) or np.any(sw < 0):
        raise ValueError("%s: every sample weight must be finite and >= 0" % who)
    return sw


def fit_trainer(weights, trainers, *, batch_size=2048, device=0, net=NET_MLP12X100, _backend=None, **kw):
    """fit() from the samples of one finished Trainer, or of a sequence of them added in that order, taken device to
    device (Fitter.add_trainer_samples).  fit_trainer(w, t, seed=s) equals fit(w, *samples_io.get_samples(t), seed=s) to
    the bit.  Keywords as fit_resident's; the trainers must be on `device`."""
    ts = [trainers] if isinstance(trainers, Trainer) else list(trainers)
    if not ts:
        raise ValueError("fit_trainer: no trainer given")
    name, num_weights = net_info(net)
    if _f32(weights).size != num_weights:
        raise ValueError("fit_trainer: %s weights have %d floats, got %d" % (name, num_weights, _f32(weights).size))

    def add(be):
        for t in ts:
            be.add_trainer_samples(t)

    return _fit_added(add, weights, batch_size, device, net, _backend, kw)


def _fit_added(add, weights, batch_size, device, net, backend, kw):
    """a fitter of its own (unless a backend is given), emptied, filled by add(fitter), and fit_resident on it"""
    # the arguments are checked before a fitter is made, with the defaults of fit_resident's own signature
    args = inspect.signature(fit_resident).bind(None, weights, batch_size=batch_size, **kw)
    args.apply_defaults()
    a = args.arguments
    _check_fit_args(a["learning_rate"], a["batch_size"], a["epochs"], a["validation_split"], a["anneal_factor"],
                    a["patience"])
    _options(a["options"])
    _adam(a["adam"])
    _loss(a["loss"])
    _top_k(a["metrics"])
    own = backend is None
    be = Fitter(max_batch=int(batch_size), device=device, net=net) if own else backend
    try:
        be.clear_data()
        add(be)
        return fit_resident(be, weights, batch_size=batch_size, **kw)
    finally:
        if own:
            be.close()


def fit(weights, game_states, eval_labels, prob_labels, *, learning_rate=0.001, batch_size=2048, epochs=1,
        validation_split=0.3, shuffle=True, anneal_factor=0.5, patience=3, seed=0, optimizer_state=None, device=0,
        net=NET_MLP12X100, sample_weight=None, options=None, adam=None, loss=None, metrics=False, _backend=None):
    """main.pyx:249-260 `model.fit(...)` with its callbacks; see the module docstring.  Returns a FitResult.
    optimizer_state: (m, v, iterations) to resume from; None starts Adam from zeros, as a freshly compiled model.
    net: NET_MLP12X100 or NET_RESCNN4, the network `weights` belong to.
    sample_weight: one weight per row, Keras's model.fit(sample_weight=...): a batch's losses are (1/B) sum w_r loss_r,
    in training and in validation; None fits unweighted.
    options: a FitOptions (the module docstring); None: none.
    adam: an AdamOptions (the module docstring); None: Adam's defaults.
    loss: a LossOptions (the module docstring); None: the reference's loss.  metrics: True or {"top_k": k}; False: off."""
    opts, adam, loss, top_k = _options(options), _adam(adam), _loss(loss), _top_k(metrics)
    name, num_weights = net_info(net)
    w = _f32(weights).ravel()
    if w.size != num_weights:
        raise ValueError("fit: %s weights have %d floats, got %d" % (name, num_weights, w.size))
    states = _f32(game_states)
    n = states.shape[0] if states.ndim == 2 else -1
    if states.ndim != 2 or states.shape[1] != GAME_STATE_SIZE:
        raise ValueError("fit: game_states must be [n, %d]" % GAME_STATE_SIZE)
    evals = _f32(eval_labels).ravel()
    probs = _f32(prob_labels)
    if evals.size != n or probs.shape != (n, NUM_MOVES):
        raise ValueError("fit: eval_labels must be [n] and prob_labels [n, %d] for n = %d" % (NUM_MOVES, n))
    _check_fit_args(learning_rate, batch_size, epochs, validation_split, anneal_factor, patience)
    split_at = split_index(n, validation_split)
    if split_at < 1 or split_at >= n:
        raise ValueError("fit: %d rows leave no training or no validation rows at validation_split=%g"
                         % (n, validation_split))
    batch_size, epochs = int(batch_size), int(epochs)
    sw = _sample_weight(sample_weight, n, "fit")

    own = _backend is None
    be = Fitter(max_batch=batch_size, device=device, net=net) if own else _backend
    try:
        be.set_weights(w)
        if optimizer_state is None:
            be.set_optimizer(np.zeros_like(w), np.zeros_like(w), 0)
        else:
            m, v, it = optimizer_state
            be.set_optimizer(m, v, it)
        be.set_data(states, evals, probs)
        if sw is not None:
            be.set_sample_weights(sw)
        stats = _apply_options(be, opts)
        return _epochs(be, n, split_at, learning_rate, batch_size, epochs, shuffle, anneal_factor, patience, seed, stats,
                       _apply_adam(be, adam), _apply_loss(be, loss, top_k))
    finally:
        if own:
            be.close()
