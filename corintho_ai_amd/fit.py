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

The reference's move table does not belong to its space table for the two quarter-turns (DESIGN.md, quirk list): the
policies of virtual rows 8 i + 2 and 8 i + 6 are each other's.  Fitter.set_augmentation("consistent"), or
fit_samples(..., augmentation="consistent"), expands a packed set through the move table with those two rows exchanged;
the default stays the reference's, bit for bit.  Fitter.canonicalize() turns every sample of a packed set into the
smallest of its eight images (samples_io.canonicalize_host is its definition), and merge_duplicates(symmetries=True)
merges up to symmetry that way (DESIGN.md "Canonical orientation").  fit_resident leaves the fitter's augmentation alone,
as it leaves the data alone.

Fit options (FitOptions; include/corintho_hip.h "fit options" is the definition): what the reference's model declares and
leaves at zero -- kernel_regularizer=L1L2() on its hidden Dense layers -- and what its Adam's constructor takes:
    res = fit_resident(fitter, weights, options=FitOptions(l2=1e-4, weight_decay=1e-4, global_clipnorm=1.0))
The regulariser's R(w) is part of "loss" and "val_loss", as Keras adds layer losses; at most one clip mode may be set.
With an option on, `history` gains "regularization_loss", "grad_norm" (both means over the epoch's steps) and
"clipped_steps", one entry per epoch.

Adam's arguments (AdamOptions; include/corintho_hip.h "Adam's arguments" is the definition): beta_1, beta_2, epsilon,
amsgrad (a third slot, "vhat") and averaged weights (Keras's use_ema, ema_momentum, ema_overwrite_frequency):
    res = fit_resident(fitter, weights, adam=AdamOptions(beta_2=0.99, amsgrad=True, ema_momentum=0.99))
With ema_momentum > 0 a fit is Keras 3's SwapEMAWeights(swap_on_epoch=True) plus the finalisation its fit() does: every
epoch is judged by the averaged weights (swap, evaluate, swap back), so "val_loss", the best-epoch checkpoint and the
plateau rule see those numbers and best_weights are the averaged weights of the best epoch; at the end the average is
applied, so `weights` and the fitter hold it.

The loss and the metrics (LossOptions; include/corintho_hip.h "loss and metrics" is the definition): the other half of
the reference's model.compile() -- loss_weights, CategoricalCrossentropy(label_smoothing=), Huber(delta) on the value head
and metrics=:
    res = fit_resident(fitter, weights, loss=LossOptions(value_weight=0.7, policy_weight=1.3, label_smoothing=0.1,
                                                         value_loss="huber", huber_delta=0.5), metrics={"top_k": 3})
"loss" and "val_loss" are value_weight x value + policy_weight x policy (+ R), and the checkpoint and the plateau rule see
them; "value_loss" and "policy_loss" stay the means of the two terms.  With metrics the history gains
METRIC_HISTORY_KEYS, one entry per epoch: how often the network's best move is the target's (and within its top k), the
value head's mean absolute error, and the entropies of the policy and of its target -- during the epoch from each step's
own forward, as Keras logs them, and "val_" + each from the validation pass (the averaged weights' with
ema_momentum > 0).  On or off, the losses and the weights of a fit are the same bytes.  Fitter.predict(rows) reads the
heads themselves.

The three families work alike.  Each is a frozen dataclass whose fields are declared once (_opt); a call takes an
instance, a dict of its fields or None, and the call decides: None means the family's defaults, and a fitter left with
other values is set back.  With a family at its defaults a step is what it is without it, kernel for kernel and bit for
bit.  A backend other than Fitter that lacks a family's setter serves the calls that ask for that family's defaults.
"""
import ctypes as C
import inspect
from dataclasses import dataclass, field, fields, replace

import numpy as np

from . import _lib
from .nets import GAME_STATE_SIZE, MLP_NUM_WEIGHTS, NUM_MOVES, RESCNN4_NUM_WEIGHTS
from .samples_io import AUGMENTATIONS
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


# ---- the three option families: one description of a field, and everything else from it ----
_NUMBER = (int, float, np.floating, np.integer)
_BOOL = (bool, np.bool_)
# the kinds of float: what the float32 value must satisfy, and how the error says it
_FLOAT_KINDS = {"nonneg": (lambda x: np.isfinite(x) and x >= 0, "be finite and >= 0"),
                "unit": (lambda x: 0 <= x < 1, "lie in [0, 1)"),
                "positive": (lambda x: np.isfinite(x) and x > 0, "be finite and > 0")}


def _opt(default, kind, arg=None):
    """one field of a family: its default, its kind -- "nonneg", "unit" or "positive" (a float), "bool", "int" (arg: the
    bounds, both included) or "enum" (arg: {name: the C value}) -- and, as the field's own name, the name of the field
    of the C struct"""
    return field(default=default, metadata={"kind": kind, "arg": arg})


def _narrow(x):
    with np.errstate(over="ignore", under="ignore"):
        return np.float32(x)


class _Family:
    """What FitOptions, AdamOptions and LossOptions share.  A family names itself in errors (WHO), the keyword of fit()
    that takes it (ARG; the backend's setter is "set_" + ARG) and its C struct (STRUCT), and declares each field once with
    _opt(); a rule that spans fields is the family's own _rules()."""

    @classmethod
    def _table(cls):
        return [(f.name, f.metadata["kind"], f.metadata["arg"], f.default) for f in fields(cls)]

    def check(self):
        """ValueError unless the values are ones the device takes (judged in float32, as it does); returns self"""
        for name, kind, arg, _ in self._table():
            x, bad = getattr(self, name), None
            if kind in _FLOAT_KINDS:
                ok, text = _FLOAT_KINDS[kind]
                if isinstance(x, _BOOL) or not isinstance(x, _NUMBER) or not np.isfinite(x):
                    bad = "must be a finite number"
                elif not ok(_narrow(x)):
                    bad = "must %s in float32" % text
            elif kind == "bool":
                if not isinstance(x, _BOOL) and x not in (0, 1):
                    bad = "must be a bool"
            elif kind == "int":
                if isinstance(x, _BOOL) or not isinstance(x, (int, np.integer)) or not arg[0] <= x <= arg[1]:
                    bad = "must be an integer in %d..%d" % arg
            elif not isinstance(x, str) or x not in arg:
                bad = "must be %s" % " or ".join('"%s"' % c for c in arg)
            if bad:
                raise ValueError("%s: %s %s, got %r" % (self.WHO, name, bad, x))
        self._rules()
        return self

    def _rules(self):
        pass

    def _seen(self):
        """the values as the device sees them"""
        return tuple(_narrow(getattr(self, name)) if kind in _FLOAT_KINDS else getattr(self, name)
                     for name, kind, _, _ in self._table())

    def is_default(self):
        """is every value at its default (in float32, as the device sees them)"""
        return self._seen() == type(self)()._seen()

    def as_dict(self):
        as_type = {"bool": bool, "int": int, "enum": str}
        return {name: as_type.get(kind, float)(getattr(self, name)) for name, kind, _, _ in self._table()}

    @classmethod
    def parse(cls, x):
        """None or an instance (or a mapping of its fields), checked; None stays None"""
        if x is None:
            return None
        if isinstance(x, dict):
            unknown = sorted(set(x) - {f.name for f in fields(cls)})
            if unknown:
                raise ValueError("%s: unknown %s" % (cls.WHO, ", ".join(unknown)))
            x = cls(**x)
        if not isinstance(x, cls):
            raise ValueError("fit: %s must be %s %s, a dict of its fields or None, got %r"
                             % (cls.ARG, "an" if cls.__name__[0] in "AEIOU" else "a", cls.__name__, x))
        return x.check()

    def to_c(self):
        """the family's C struct, the floats rounded to float32"""
        as_c = {"bool": lambda x, _: int(bool(x)), "int": lambda x, _: int(x), "enum": lambda x, arg: arg[x]}
        return self.STRUCT(struct_size=C.sizeof(self.STRUCT),
                           **{name: as_c.get(kind, lambda x, _: float(_narrow(x)))(getattr(self, name), arg)
                              for name, kind, arg, _ in self._table()})

    @classmethod
    def from_c(cls, c):
        from_c = {"bool": lambda x, _: bool(x), "int": lambda x, _: int(x),
                  "enum": lambda x, arg: {v: k for k, v in arg.items()}[int(x)]}
        return cls(**{name: from_c.get(kind, lambda x, _: float(x))(getattr(c, name), arg)
                      for name, kind, arg, _ in cls._table()})


@dataclass(frozen=True)
class FitOptions(_Family):
    """ca_fit_options: every value 0 is off.  The device takes the values in float32."""
    WHO, ARG, STRUCT = "fit options", "options", _lib.CaFitOptions
    l1: float = _opt(0.0, "nonneg")
    l2: float = _opt(0.0, "nonneg")
    regularize: int = _opt(0, "int", (0, 1))  # 0: l1 and l2 on the trunk kernels, 1: on all kernels
    weight_decay: float = _opt(0.0, "nonneg")
    clipvalue: float = _opt(0.0, "nonneg")
    clipnorm: float = _opt(0.0, "nonneg")
    global_clipnorm: float = _opt(0.0, "nonneg")

    def _rules(self):
        if sum(1 for k in ("clipvalue", "clipnorm", "global_clipnorm") if _narrow(getattr(self, k)) > 0) > 1:
            raise ValueError("fit options: at most one of clipvalue, clipnorm and global_clipnorm may be set")

    def any(self):
        """is any option on (in float32, as the device sees them)"""
        return any(_narrow(getattr(self, k)) > 0 for k in OPTION_NAMES)

    def is_default(self):
        """is every option off (regularize is not read then)"""
        return not self.any()


OPTION_NAMES = tuple(name for name, kind, _, _ in FitOptions._table() if kind == "nonneg")
OPTION_HISTORY_KEYS = ("regularization_loss", "grad_norm", "clipped_steps")
SLOTS = {"vhat": 0, "average": 1}  # CA_SLOT_VHAT, CA_SLOT_AVERAGE


@dataclass(frozen=True)
class AdamOptions(_Family):
    """ca_fit_adam: the defaults are Keras Adam's.  The device takes the floats in float32."""
    WHO, ARG, STRUCT = "adam", "adam", _lib.CaFitAdam
    beta_1: float = _opt(0.9, "unit")
    beta_2: float = _opt(0.999, "unit")
    epsilon: float = _opt(1e-7, "positive")
    amsgrad: bool = _opt(False, "bool")
    ema_momentum: float = _opt(0.0, "unit")  # 0: no averaged weights
    ema_overwrite_frequency: int = _opt(0, "int", (0, 2 ** 31 - 1))

    def _rules(self):
        if self.ema_overwrite_frequency > 0 and not self.averaged():
            raise ValueError("adam: ema_overwrite_frequency needs ema_momentum > 0")

    def averaged(self):
        return bool(_narrow(self.ema_momentum) > 0)


ADAM_NAMES = tuple(f.name for f in fields(AdamOptions))
VALUE_LOSSES = {"mse": 0, "huber": 1}  # CA_VALUE_LOSS_MSE, CA_VALUE_LOSS_HUBER


@dataclass(frozen=True)
class LossOptions(_Family):
    """ca_fit_loss: the defaults are the reference's compile(): MSE + 0.25 x cross-entropy.  The device takes the floats
    in float32."""
    WHO, ARG, STRUCT = "loss", "loss", _lib.CaFitLoss
    value_weight: float = _opt(1.0, "nonneg")
    policy_weight: float = _opt(0.25, "nonneg")
    label_smoothing: float = _opt(0.0, "unit")
    value_loss: str = _opt("mse", "enum", VALUE_LOSSES)
    huber_delta: float = _opt(1.0, "positive")  # read only with "huber"

    def _rules(self):
        if _narrow(self.value_weight) == 0 and _narrow(self.policy_weight) == 0:
            raise ValueError("loss: value_weight and policy_weight may not both be 0 (in float32)")

    def is_default(self):
        """is the loss the reference's (in float32, as the device sees it; huber_delta is not read with "mse")"""
        return _Family.is_default(replace(self, huber_delta=1.0) if self.value_loss == "mse" else self)


LOSS_NAMES = tuple(f.name for f in fields(LossOptions))
METRIC_NAMES = ("categorical_accuracy", "top_k_categorical_accuracy", "mean_absolute_error", "policy_entropy",
                "target_entropy")  # ca_fit_metrics' fields, and the keys of Fitter.metrics()
# what a fit's history calls them (Keras's names for a model whose outputs are "policy" and "value"), then their val_ forms
METRIC_KEYS = ("policy_categorical_accuracy", "policy_top_k_categorical_accuracy", "value_mean_absolute_error",
               "policy_entropy", "target_entropy")
METRIC_HISTORY_KEYS = METRIC_KEYS + tuple("val_" + k for k in METRIC_KEYS)
DEFAULT_TOP_K = 5


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
        if isinstance(k, _BOOL) or not isinstance(k, (int, np.integer)) or not 1 <= k <= NUM_MOVES:
            raise ValueError("metrics: top_k must be an integer in 1..%d, got %r" % (NUM_MOVES, k))
        return int(k)
    raise ValueError('fit: metrics must be False, True or {"top_k": k}, got %r' % (metrics,))


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

    def _set(self, family, value, setter):
        """hand the device a family's struct: value is an instance, a dict of its fields, or None for the defaults"""
        self._check(setter(self._h, C.byref((family.parse(value) or family()).to_c())))

    def _get(self, struct, getter):
        c = struct(struct_size=C.sizeof(struct))
        self._check(getter(self._h, C.byref(c)))
        return c

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

    # ---- the augmentation of a packed set and its canonical orientation (include/corintho_hip.h) ----
    def set_augmentation(self, augmentation="reference"):
        """how virtual row 8 i + k of a packed set is expanded: "reference" -- the policy through the reference's move
        table, whose rows 2 and 6 belong to each other's rotation -- or "consistent" -- through the move table with those
        two rows exchanged (samples_io.symmetry_tables, samples_io.expand_host).  It belongs to the fitter and stays
        until set again; an expanded set (set_data) is never touched."""
        if augmentation not in AUGMENTATIONS:
            raise ValueError('the augmentation must be "reference" or "consistent", got %r' % (augmentation,))
        self._check(self._L.ca_fitter_set_augmentation(self._h, AUGMENTATIONS[augmentation]))

    def get_augmentation(self):
        a = C.c_int32()
        self._check(self._L.ca_fitter_get_augmentation(self._h, C.byref(a)))
        return {v: k for k, v in AUGMENTATIONS.items()}[a.value]

    def canonicalize(self):
        """Bring every sample of a packed set into its canonical orientation on the device: of the eight symmetric images
        of its board the one whose 64 words are smallest as unsigned patterns, the policy moved along through the
        consistent move table (samples_io.canonicalize_host is the definition, and equals this bit for bit).  Outcomes
        and weights stay, and the set takes more samples afterwards.  Returns how many samples changed."""
        moved = C.c_int32()
        self._check(self._L.ca_fitter_canonicalize(self._h, C.byref(moved)))
        return moved.value

    def merge_duplicates(self, normalize=True, symmetries=False):
        """Merge the duplicate positions of a packed set on the device: samples whose 70 state floats have the same
        bits become one sample at the rank of the first of them, with the weighted mean of their policies and outcomes
        (float64 sums over the members in ascending index, rounded once) and the sum W of their weights as its weight
        (samples_io.merge_duplicates_host is the definition, and equals this bit for bit).  normalize: the weights are
        scaled to mean one.  A group whose weights are all 0 has W = 0 and no mean: it is dropped, members and all.
        The set carries weights afterwards, so add_* is refused until clear_data: merge once, after the last add.
        Returns (samples before, samples after).
        symmetries: canonicalize() first, so that positions which are images of one another merge as well; the merge
        itself is the same.  Under set_augmentation("consistent") the merged set expands to the rows the unmerged one
        expands to, with mean targets; under "reference" the rows 2 and 6 of an image are other (wrong) rows than those
        of the sample, and the merge is not that equivalence ("Canonical orientation")."""
        if symmetries:
            self.canonicalize()
        before, after = C.c_int32(), C.c_int32()
        self._check(self._L.ca_fitter_merge_duplicates(self._h, 1 if normalize else 0, C.byref(before), C.byref(after)))
        return before.value, after.value

    # ---- fit options (include/corintho_hip.h, "fit options") ----
    def set_options(self, options=None):
        """the regulariser, weight decay and clipping of every later step (FitOptions, or a dict of its fields); None:
        all off.  They stay until set again."""
        self._set(FitOptions, options, self._L.ca_fitter_set_options)

    def get_options(self):
        return FitOptions.from_c(self._get(_lib.CaFitOptions, self._L.ca_fitter_get_options))

    def train_stats(self):
        """of the last train(): {"steps", "clipped_steps", "regularization_loss", "grad_norm", "grad_norm_max"} -- the
        means over the steps of R(w) and of the norm of the regularised gradient before clipping, and that norm's
        maximum; zeros when no option is set"""
        c = self._get(_lib.CaFitStats, self._L.ca_fitter_train_stats)
        return {"steps": int(c.steps), "clipped_steps": int(c.clipped_steps), "regularization_loss": float(c.regularization),
                "grad_norm": float(c.grad_norm), "grad_norm_max": float(c.grad_norm_max)}

    # ---- Adam's arguments, the third slot and the averaged weights (include/corintho_hip.h, "Adam's arguments") ----
    def set_adam(self, adam=None):
        """Adam's arguments of every later step (AdamOptions, or a dict of its fields); None: the defaults.  They stay
        until set again."""
        self._set(AdamOptions, adam, self._L.ca_fitter_set_adam)

    def get_adam(self):
        return AdamOptions.from_c(self._get(_lib.CaFitAdam, self._L.ca_fitter_get_adam))

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
        self._set(LossOptions, loss, self._L.ca_fitter_set_loss)

    def get_loss(self):
        return LossOptions.from_c(self._get(_lib.CaFitLoss, self._L.ca_fitter_get_loss))

    def set_metrics(self, on=True, top_k=DEFAULT_TOP_K):
        """switch the metrics of train() and evaluate() on or off; top_k in 1..96"""
        self._check(self._L.ca_fitter_set_metrics(self._h, 1 if on else 0, int(top_k)))

    def metrics(self):
        """of the last train() or evaluate(): METRIC_NAMES' means weighted by the sample weights, and "rows",
        "weight_sum" and "top_k"; an EngineError (CA_ERR_STATE) while metrics are off"""
        c = self._get(_lib.CaFitMetrics, self._L.ca_fitter_metrics)
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


def _epochs(be, n, split_at, call, stats=False, adam=None, metrics=False):
    """the epochs of model.fit on the n rows the backend holds, rows [0, split_at) training; the callbacks' logic.
    call: the _Call.  stats: an option is on, the backend's train_stats() of every epoch go to the history.
    adam: the call's AdamOptions if any is off its default.  With ema_momentum > 0 this is Keras 3's
    SwapEMAWeights(swap_on_epoch=True) plus the finalisation fit() does: an epoch is judged by the averaged weights (swap,
    evaluate, swap back), the checkpoint holds them, and at the end the average is applied to the weights.
    metrics: the backend's metrics() of every epoch's train() and evaluate() go to the history (METRIC_HISTORY_KEYS)."""
    averaged = adam is not None and adam.averaged()
    names = (("vhat",) if adam is not None and adam.amsgrad else ()) + (("average",) if averaged else ())

    def slots():
        return {k: be.get_slot(k) for k in names} if names else None

    batch_size, shuffle, anneal_factor, patience = call.batch_size, call.shuffle, call.anneal_factor, call.patience
    rng = np.random.default_rng(call.seed)
    lr = np.float32(call.learning_rate)
    history = {k: [] for k in HISTORY_KEYS + (OPTION_HISTORY_KEYS if stats else ()) + (METRIC_HISTORY_KEYS if metrics else ())}
    ckpt_best, plateau_best, wait = np.inf, np.inf, 0
    best = None
    for epoch in range(call.epochs):
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


@dataclass(frozen=True)
class _Call:
    """what one call of fit() or of a relative asks for, checked: made by _call() before any fitter is"""
    learning_rate: float
    batch_size: int
    epochs: int
    validation_split: float
    shuffle: bool
    anneal_factor: float
    patience: int
    seed: object
    optimizer_state: tuple  # (m, v, iterations), or None: Adam starts from zeros
    slots: dict             # {"vhat": ..., "average": ...} to resume from, or None
    options: FitOptions     # the three families, parsed; None: the defaults
    adam: AdamOptions
    loss: LossOptions
    top_k: int              # None: metrics off


def _call(*, learning_rate=0.001, batch_size=2048, epochs=1, validation_split=0.3, shuffle=True, anneal_factor=0.5,
          patience=3, seed=0, optimizer_state=None, options=None, adam=None, slots=None, loss=None, metrics=False):
    """the keywords fit() and its relatives share, with their defaults, as a _Call; ValueError on a bad one"""
    options, adam, loss = FitOptions.parse(options), AdamOptions.parse(adam), LossOptions.parse(loss)
    top_k = _top_k(metrics)
    if int(batch_size) != batch_size or batch_size < 1:
        raise ValueError("fit: batch_size must be a positive integer")
    if int(epochs) != epochs or epochs < 1:
        raise ValueError("fit: epochs must be a positive integer")
    if not 0.0 < validation_split < 1.0:
        raise ValueError("fit: validation_split must lie in (0, 1)")
    if not learning_rate > 0.0 or not 0.0 < anneal_factor < 1.0 or int(patience) != patience or patience < 0:
        raise ValueError("fit: learning_rate > 0, anneal_factor in (0, 1) and patience >= 0 are required")
    return _Call(learning_rate, int(batch_size), int(epochs), validation_split, shuffle, anneal_factor, patience, seed,
                 optimizer_state, slots, options, adam, loss, top_k)


def _weights(weights, net, who):
    """the flat float32 weights of a network of kind `net`, checked"""
    name, num_weights = net_info(net)
    w = _f32(weights).ravel()
    if w.size != num_weights:
        raise ValueError("%s: %s weights have %d floats, got %d" % (who, name, num_weights, w.size))
    return w


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


def _apply(be, call):
    """put the backend into the state the call asks for: a backend that has a family's setter gets the call's values
    (None: the defaults); one that has none serves only a call that asks for that family's defaults.  The same for the
    metrics.  Returns what _epochs takes: (do train_stats go to the history, the AdamOptions if any is off its default,
    are metrics on)"""
    def has(name):  # (without asking a backend's __getattr__)
        return inspect.getattr_static(be, name, None) is not None

    on = {}
    for family, asked in ((FitOptions, call.options), (AdamOptions, call.adam), (LossOptions, call.loss)):
        on[family] = asked is not None and not asked.is_default()
        if has("set_" + family.ARG):
            getattr(be, "set_" + family.ARG)(asked if asked is not None else family())
        elif on[family]:
            raise ValueError("fit: the backend %s has no set_%s" % (type(be).__name__, family.ARG))
    if has("set_metrics"):
        be.set_metrics(call.top_k is not None, call.top_k if call.top_k is not None else DEFAULT_TOP_K)
    elif call.top_k is not None:
        raise ValueError("fit: the backend %s has no set_metrics" % type(be).__name__)
    return on[FitOptions] and has("train_stats"), call.adam if on[AdamOptions] else None, call.top_k is not None


def _run(be, n, w, call, who):
    """the fit a call asks for, on a backend that holds its n rows: the split, the starting point, the families, the epochs"""
    split_at = split_index(n, call.validation_split)
    if split_at < 1 or split_at >= n:
        raise ValueError("%s: %d rows leave no training or no validation rows at validation_split=%g"
                         % (who, n, call.validation_split))
    be.set_weights(w)
    m, v, it = call.optimizer_state if call.optimizer_state is not None else (np.zeros_like(w), np.zeros_like(w), 0)
    be.set_optimizer(m, v, it)
    for k in sorted(call.slots or {}):
        be.set_slot(k, call.slots[k])
    return _epochs(be, n, split_at, call, *_apply(be, call))


def _run_filled(fill, w, call, device, net, backend, who):
    """_run on a fitter of its own (unless a backend is given) that fill(fitter) gives its data; fill returns the rows"""
    own = backend is None
    be = Fitter(max_batch=call.batch_size, device=device, net=net) if own else backend
    try:
        return _run(be, fill(be), w, call, who)
    finally:
        if own:
            be.close()


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
    call = _call(learning_rate=learning_rate, batch_size=batch_size, epochs=epochs, validation_split=validation_split,
                 shuffle=shuffle, anneal_factor=anneal_factor, patience=patience, seed=seed,
                 optimizer_state=optimizer_state, options=options, adam=adam, slots=slots, loss=loss, metrics=metrics)
    w = _f32(weights).ravel()
    num_weights = getattr(fitter, "num_weights", w.size)
    if w.size != num_weights:
        raise ValueError("fit_resident: the fitter's network has %d floats, got %d" % (num_weights, w.size))
    return _run(fitter, int(fitter.data_info()[0]), w, call, "fit_resident")


def _set_augmentation(be, augmentation):
    """a call's augmentation on the backend that is being filled: the call decides.  A backend without the setter
    serves the calls that ask for the reference's."""
    if inspect.getattr_static(be, "set_augmentation", None) is not None:
        be.set_augmentation(augmentation)
    elif augmentation != "reference":
        raise ValueError("fit: the backend %s has no set_augmentation" % type(be).__name__)


def _check_augmentation(augmentation, who):
    if augmentation not in AUGMENTATIONS:
        raise ValueError('%s: augmentation must be "reference" or "consistent", got %r' % (who, augmentation))


def fit_samples(weights, state_policy, outcome, *, device=0, net=NET_MLP12X100, sample_weight=None,
                merge_duplicates=False, merge_symmetries=False, augmentation="reference", _backend=None, **kw):
    """fit() from un-augmented samples (Trainer.export_samples, dist.SampleGather.rows): a packed data set, 668 bytes
    a sample on the device instead of 5 344.  fit_samples(w, sp, oc, seed=s) equals fit(w, *expand_samples(sp, oc),
    seed=s) to the bit: the 8 n virtual rows are in expand_samples' row order, so the validation split and every
    epoch's permutation are the same.  sample_weight: one weight per sample (Keras's sample_weight; the sample's 8
    virtual rows share it).  merge_duplicates: Fitter.merge_duplicates(normalize=True) on the set, weights and all,
    before the fit -- the same as fitting samples_io.merge_duplicates_host's three arrays; with merge_symmetries the
    merge is up to the eight symmetries (merge_duplicates(symmetries=True); it implies the merge).  augmentation: "reference" or "consistent",
    how the 8 n virtual rows are expanded (Fitter.set_augmentation): with "consistent" the fit equals fit(w,
    *samples_io.expand_host(sp, oc, "consistent"), seed=s) to the bit.  The call decides: a fitter left with another
    augmentation is set to this one.  Keywords as fit_resident's."""
    call = _call(**kw)
    _check_augmentation(augmentation, "fit_samples")
    w = _weights(weights, net, "fit_samples")
    sp, oc = _packed(state_policy, outcome, "fit_samples")
    sw = _sample_weight(sample_weight, sp.shape[0], "fit_samples")

    def fill(be):
        be.clear_data()
        _set_augmentation(be, augmentation)
        be.add_samples(sp, oc)
        if sw is not None:
            be.set_sample_weights(sw)
        if merge_symmetries:
            be.merge_duplicates(normalize=True, symmetries=True)
        elif merge_duplicates:
            be.merge_duplicates(normalize=True)
        return int(be.data_info()[0])

    return _run_filled(fill, w, call, device, net, _backend, "fit_resident")


def fit_trainer(weights, trainers, *, device=0, net=NET_MLP12X100, augmentation="reference", _backend=None, **kw):
    """fit() from the samples of one finished Trainer, or of a sequence of them added in that order, taken device to
    device (Fitter.add_trainer_samples).  fit_trainer(w, t, seed=s) equals fit(w, *samples_io.get_samples(t), seed=s) to
    the bit.  augmentation: as fit_samples'.  Keywords as fit_resident's; the trainers must be on `device`."""
    call = _call(**kw)
    _check_augmentation(augmentation, "fit_trainer")
    ts = [trainers] if isinstance(trainers, Trainer) else list(trainers)
    if not ts:
        raise ValueError("fit_trainer: no trainer given")
    w = _weights(weights, net, "fit_trainer")

    def fill(be):
        be.clear_data()
        _set_augmentation(be, augmentation)
        for t in ts:
            be.add_trainer_samples(t)
        return int(be.data_info()[0])

    return _run_filled(fill, w, call, device, net, _backend, "fit_resident")


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
    call = _call(learning_rate=learning_rate, batch_size=batch_size, epochs=epochs, validation_split=validation_split,
                 shuffle=shuffle, anneal_factor=anneal_factor, patience=patience, seed=seed,
                 optimizer_state=optimizer_state, options=options, adam=adam, loss=loss, metrics=metrics)
    w = _weights(weights, net, "fit")
    states = _f32(game_states)
    n = states.shape[0] if states.ndim == 2 else -1
    if states.ndim != 2 or states.shape[1] != GAME_STATE_SIZE:
        raise ValueError("fit: game_states must be [n, %d]" % GAME_STATE_SIZE)
    evals = _f32(eval_labels).ravel()
    probs = _f32(prob_labels)
    if evals.size != n or probs.shape != (n, NUM_MOVES):
        raise ValueError("fit: eval_labels must be [n] and prob_labels [n, %d] for n = %d" % (NUM_MOVES, n))
    sw = _sample_weight(sample_weight, n, "fit")

    def fill(be):
        be.set_data(states, evals, probs)
        if sw is not None:
            be.set_sample_weights(sw)
        return n

    return _run_filled(fill, w, call, device, net, _backend, "fit")
