"""A training run: the reference's run directory (corintho_ai/python/wrapper.py) and one generation of it
(`train_generation` and `update_rating`, corintho_ai/python/main.pyx:274-365) on the device engine.

    run = Run.open(RunParams(name="train", cwd="./logs", num_games=25000, max_searches=1600, searches_per_eval=16))
    res = run.generation()          # self-play -> samples -> fit -> arena -> rating -> metadata
    python -m corintho_ai_amd.run --config toml/train.toml --generations 5

One `generation()` is one call of the reference's `wrapper.py`: the run is set up from its metadata files
(setup_existing_run, wrapper.py:164-237), the generation is trained (main.pyx:285-365) and the metadata moves on
(update_run_data, write_learning_rate, wrapper.py:375-487).  Every step on the device is one the package already has:
Trainer.run() for self-play and arena, Fitter.add_trainer_samples for the hand-over, fit_resident for model.fit.

What is deliberately not the reference's:
  * a generation's model is generations/gen_k/model.npz (weights, adam_m, adam_v, adam_iterations, net), not a SavedModel;
  * the seeds of a generation come from numpy.random.default_rng([seed, generation]), not from the clock
    (main.pyx:293), so that an interrupted generation, played again, repeats itself;
  * the samples of a generation are samples/gen_k/samples.npz, un-augmented (samples_io.save_packed); the three
    expanded files are written as well with sample_format="reference";
  * the run is not zipped after every generation (wrapper.py:390-400) unless zip_logs is set;
  * metadata files are written through a temporary file and os.replace, current_generation.txt last; on opening a run
    metadata/losses.txt is cut to one line per finished generation (the reference appends the loss before the arena, so
    an interrupted generation would leave its line behind and count twice in write_learning_rate);
  * merge_duplicates (off by default): after the last samples of the fit's window are added, positions that occur more
    than once become one sample each, with the mean of their targets and a weight equal to their share
    (Fitter.merge_duplicates, normalised to mean one, so that a batch weighs what an unweighted one does; val_loss
    is lower all the same, because the merged targets are means: profiles/sample_merge.md).  samples.npz stays the un-merged export and fit_time.txt counts the generation's samples, as the reference does.
  * merge_symmetries (off by default; implies merge_duplicates): the merge is up to the eight symmetries -- every sample
    is first turned into the smallest of its eight images (Fitter.canonicalize; DESIGN.md "Canonical orientation").
  * augmentation ("reference" by default): "consistent" expands the fit's samples through the move table that belongs
    to the space table (the reference's rows 2 and 6 are each other's: DESIGN.md, quirk list).  It is written with the
    other settings into every generation's metadata.txt; generation_settings() reads one back, and a run directory
    from before the setting existed reads as "reference".
  * l1, l2, regularize, weight_decay, clipvalue, clipnorm, global_clipnorm (all off by default): the fit options of
    fit.FitOptions -- the regulariser the reference declares on its hidden layers and leaves at zero, and the arguments
    its Adam's constructor takes.  A generation that fits with any of them writes training_logs/fit_options.json: the
    options, and per epoch the regularisation loss, the mean gradient norm and the clipped steps.  val_loss, and with
    it metadata/losses.txt, then includes the regulariser's R(w), as Keras's does.  model.npz is what it was.
  * value_weight, policy_weight, label_smoothing, value_loss, huber_delta (the reference's loss by default): the loss of
    fit.LossOptions; off the defaults fit_options.json holds them under "loss", and val_loss is the weighted one.
    metrics, top_k (off by default): train_loss.csv carries fit.METRIC_HISTORY_KEYS' columns after the ones it has;
    write_loss takes val_loss by its column's name.
"""
import argparse
import dataclasses
import inspect
import json
import os
import shutil
import sys
import time
from dataclasses import dataclass, field
from datetime import datetime

import numpy as np

from . import _lib, nets, samples_io
from . import trainer as _trainer
from .fit import (METRIC_HISTORY_KEYS, OPTION_HISTORY_KEYS, AdamOptions, FitOptions, Fitter, LossOptions, fit_resident,
                  net_info)

NETS = {"mlp12x100": (_trainer.NET_MLP12X100, nets.init_mlp12x100), "rescnn4": (_trainer.NET_RESCNN4, nets.init_rescnn4)}
# the network kind self-play and arena evaluate with: (net, arith) -> Trainer.set_net's kind
PLAY_KINDS = {
    ("mlp12x100", "f32"): _trainer.NET_MLP12X100, ("mlp12x100", "x3"): _trainer.NET_MLP12X100_X3,
    ("mlp12x100", "x6"): _trainer.NET_MLP12X100_X6, ("mlp12x100", "h3"): _trainer.NET_MLP12X100_H3,
    ("rescnn4", "f32"): _trainer.NET_RESCNN4, ("rescnn4", "x3"): _trainer.NET_RESCNN4_X3,
    ("rescnn4", "x6"): _trainer.NET_RESCNN4_X6, ("rescnn4", "h3"): _trainer.NET_RESCNN4_H3,
}
VALIDATION_SPLIT = 0.3  # main.pyx:255
# a field of an option family that RunParams holds under another name: `epsilon` is the search's noise weight
FAMILY_FIELDS = {(AdamOptions, "epsilon"): "adam_epsilon"}
# train_loss.csv: Keras's CSVLogger writes "epoch" and then the sorted log keys, which puts val_loss last
# (main.pyx:244, read back by write_loss at main.pyx:65-66); the names here sort differently, so the order is spelled out
LOSS_COLUMNS = ("loss", "lr", "policy_loss", "value_loss", "val_policy_loss", "val_value_loss", "val_loss")


@dataclass
class RunParams:
    """The flags of wrapper.py:20-133 with their defaults, and the device options.  The clamps of wrapper.py:138-160
    are applied when the object is made; a field assigned afterwards is taken as it stands."""
    anneal_factor: float = 0.5
    batch_size: int = 2048
    c_puct: float = 1.0
    cwd: str = "."
    epochs: int = 1
    epsilon: float = 0.25
    learning_rate: float = 0.01
    max_searches: int = 1600
    name: str = ""
    num_games: int = 25000
    num_logged: int = 0
    num_old_gens: int = 20
    num_test_games: int = 400
    num_threads: int = 0  # accepted and ignored: the games are wavefronts of one device
    patience: int = 3
    searches_per_eval: int = 1
    test_threshold: float = 0.5
    # ---- no reference counterpart ----
    net: str = "mlp12x100"
    arith: str = "h3"
    device: int = 0
    seed: object = None          # None: from the clock, as main.pyx:293
    mix_old: bool = False        # False: train on this generation alone, as the reference does (main.pyx:212-214)
    sample_format: str = "packed"
    init_weights: object = None  # flat array or .npz for generation 0
    zip_logs: bool = False
    merge_duplicates: bool = False  # True: duplicate positions of the fit's window become one weighted sample each
    merge_symmetries: bool = False  # True: the same up to the eight symmetries (implies merge_duplicates)
    augmentation: str = "reference"  # or "consistent": the move table that belongs to the space table (fit.Fitter.set_augmentation)
    # the fit options (fit.FitOptions; include/corintho_hip.h "fit options"): 0 is off
    l1: float = 0.0
    l2: float = 0.0
    regularize: int = 0          # 0: l1 and l2 on the trunk kernels, 1: on all kernels
    weight_decay: float = 0.0
    clipvalue: float = 0.0
    clipnorm: float = 0.0
    global_clipnorm: float = 0.0
    # Adam's arguments (fit.AdamOptions; include/corintho_hip.h "Adam's arguments"); `epsilon` is the search's noise weight
    beta_1: float = 0.9
    beta_2: float = 0.999
    adam_epsilon: float = 1e-7
    amsgrad: bool = False
    ema_momentum: float = 0.0    # > 0: the fit judges and hands on averaged weights
    ema_overwrite_frequency: int = 0
    # the loss and the metrics (fit.LossOptions; include/corintho_hip.h "loss and metrics")
    value_weight: float = 1.0
    policy_weight: float = 0.25
    label_smoothing: float = 0.0
    value_loss: str = "mse"      # or "huber"
    huber_delta: float = 1.0
    metrics: bool = False        # True: train_loss.csv gains the metrics' columns
    top_k: int = 5

    def __post_init__(self):
        for f in dataclasses.fields(self):  # a TOML or command-line value may come as the other number type
            if f.type in (int, float):
                setattr(self, f.name, f.type(getattr(self, f.name)))
        # wrapper.py:138-160
        self.anneal_factor = max(0.0, min(1.0, self.anneal_factor))
        self.batch_size = max(1, self.batch_size)
        self.c_puct = max(0.0, self.c_puct)
        self.epochs = max(1, self.epochs)
        self.epsilon = min(1.0, max(0.0, self.epsilon))
        self.learning_rate = max(0.0, self.learning_rate)
        self.max_searches = max(2, self.max_searches)
        self.num_games = max(1, self.num_games)
        self.num_logged = max(0, self.num_logged)
        self.num_old_gens = max(0, self.num_old_gens)
        self.num_test_games = 2 * max(1, self.num_test_games // 2)  # even: first player bias
        self.patience = max(1, min(self.epochs, self.patience))
        self.searches_per_eval = min(self.max_searches - 1, max(1, self.searches_per_eval))
        self.test_threshold = min((self.num_test_games - 0.5) / self.num_test_games, max(0.5, self.test_threshold))
        if self.net not in NETS:
            raise ValueError("net must be one of %s, not %r" % (sorted(NETS), self.net))
        if (self.net, self.arith) not in PLAY_KINDS:
            raise ValueError('arith must be "h3", "f32", "x6" or "x3", not %r' % (self.arith,))
        if self.sample_format not in ("packed", "reference"):
            raise ValueError('sample_format must be "packed" or "reference", not %r' % (self.sample_format,))
        if self.seed is None:
            self.seed = int(time.time())
        self.seed = int(self.seed)
        if self.seed < 0:
            raise ValueError("seed must not be negative")
        self.mix_old, self.zip_logs = bool(self.mix_old), bool(self.zip_logs)
        self.merge_symmetries = bool(self.merge_symmetries)
        self.merge_duplicates = bool(self.merge_duplicates) or self.merge_symmetries
        if self.augmentation not in samples_io.AUGMENTATIONS:
            raise ValueError('augmentation must be "reference" or "consistent", not %r' % (self.augmentation,))
        self.amsgrad = bool(self.amsgrad)
        self.fit_options()  # ValueError: a negative value, two clip modes
        self.adam_options()  # ValueError: a beta outside [0, 1), ...
        self.loss_options()  # ValueError: a negative weight, both 0, an unknown value_loss, ...
        self.metrics = bool(self.metrics)
        if not 1 <= self.top_k <= nets.NUM_MOVES:
            raise ValueError("top_k must be in 1..%d, not %r" % (nets.NUM_MOVES, self.top_k))

    def _family(self, family):
        """one of fit's option families from the fields of the same names (FAMILY_FIELDS has the exceptions), checked"""
        return family(**{f.name: getattr(self, FAMILY_FIELDS.get((family, f.name), f.name))
                         for f in dataclasses.fields(family)}).check()

    def fit_options(self):
        """the fit options of the run as a fit.FitOptions, checked"""
        return self._family(FitOptions)

    def adam_options(self):
        """Adam's arguments of the run as a fit.AdamOptions, checked"""
        return self._family(AdamOptions)

    def loss_options(self):
        """the loss of the run as a fit.LossOptions, checked"""
        return self._family(LossOptions)

    def as_dict(self):
        d = {f.name: getattr(self, f.name) for f in dataclasses.fields(self)}
        if not isinstance(d["init_weights"], (str, type(None))):
            d["init_weights"] = "<array>"
        return d


@dataclass
class GenerationResult:
    generation: int
    improved: bool
    score: float
    rating: float
    fit: object            # fit.FitResult
    num_samples: int
    seeds: dict            # {"selfplay", "arena", "fit"}
    times: dict = field(default_factory=dict)  # seconds of "selfplay", "samples", "fit", "arena"
    merged: object = None  # merge_duplicates: (samples of the fit's window before, after); None: not asked for

    @property
    def val_loss(self):
        return min(self.fit.history["val_loss"])


# ---------------------------------------------------------------------------------------------------- files
def generation_settings(metadata_file):
    """the settings a generation was trained with, from its metadata.txt; a setting that did not exist when the file was
    written has its default (augmentation: "reference")"""
    with open(metadata_file, encoding="utf-8") as f:
        d = json.load(f)
    for f in dataclasses.fields(RunParams):
        if f.name not in d and f.default is not dataclasses.MISSING:
            d[f.name] = f.default
    return d


def _write_text(path, text):
    """a metadata file, whole or not at all"""
    tmp = path + ".tmp"
    with open(tmp, "w", encoding="utf-8") as f:
        f.write(text)
    os.replace(tmp, path)


def _read_text(path):
    with open(path, encoding="utf-8") as f:
        return f.read().strip()


def save_model(path, weights, optimizer, net, slots=None):
    """slots: {"vhat": ..., "average": ...} (a FitResult's best_slots), written as adam_vhat and adam_average; None or
    empty: the file is what it is without them"""
    m, v, it = optimizer
    arrays = {"weights": np.asarray(weights, np.float32), "adam_m": np.asarray(m, np.float32),
              "adam_v": np.asarray(v, np.float32), "adam_iterations": np.asarray(it, np.int64), "net": np.asarray(net)}
    for k in sorted(slots or {}):
        arrays["adam_" + k] = np.asarray(slots[k], np.float32)
    samples_io.write_npz(path, arrays)


def load_model(path, net=None):
    """(weights, (adam_m, adam_v, adam_iterations)) of a generation's model.npz"""
    with np.load(path) as z:
        if net is not None and str(z["net"]) != net:
            raise ValueError("%s holds a %s, the run is asked for a %s" % (path, z["net"], net))
        return z["weights"], (z["adam_m"], z["adam_v"], int(z["adam_iterations"]))


def load_model_slots(path):
    """the extra slots of a generation's model.npz: {"vhat": ..., "average": ...} with the ones it holds, {} if none"""
    with np.load(path) as z:
        return {k: z["adam_" + k] for k in ("vhat", "average") if "adam_" + k in z.files}


def format_time(t):
    """main.pyx:45-54"""
    if t < 1:
        return "%ss" % t
    if t < 60:
        return "%.2fs" % t
    if t < 3600:
        return "%dm%02ds" % (t // 60, round(t) % 60)
    return "%dh%02dm%02ds" % (t // 3600, (t % 3600) // 60, round(t) % 60)


def write_loss(loss_csv, loss_file):
    """main.pyx:56-68: the smallest val_loss of the csv -- its last column, unless the metrics' columns follow it --
    appended to the run's loss file"""
    best_loss = 999
    with open(loss_csv, encoding="utf-8") as f:
        lines = list(f)
    header = lines[0].rstrip("\n").split("\t") if lines else []
    col = header.index("val_loss") if "val_loss" in header else -1
    for line in lines[1:]:
        best_loss = min(best_loss, float(line.split("\t")[col]))
    with open(loss_file, "a+", encoding="utf-8") as f:
        f.write("%s\n" % best_loss)


def update_rating(new_rating_file, best_gen_rating, score):
    """main.pyx:274-283.  A score of 1 gives an infinite rating there too."""
    if score > 0:
        with np.errstate(divide="ignore"):
            new_rating = best_gen_rating - 400 * np.log10(1 / score - 1)
    else:
        new_rating = best_gen_rating - 400
    _write_text(new_rating_file, "%s\n" % new_rating)
    return float(new_rating)


def write_learning_rate(best_generation, current_generation, loss_file, learning_rate_file, fail_num_file,
                        learning_rate, patience, factor):
    """wrapper.py:432-487, quirks kept: the walk is over every line of the loss file, "the loss improved" means that
    its last line is strictly below every earlier one, and the factor is applied to `learning_rate`, the rate the
    generation started with."""
    if best_generation == current_generation:  # the generation passed
        _write_text(fail_num_file, "0")
        return
    min_loss, loss_fails = 999, 0
    with open(loss_file, encoding="utf-8") as f:
        for line in f:
            cur_loss = float(line.strip())
            if cur_loss < min_loss:
                min_loss, loss_fails = cur_loss, 0
            else:
                loss_fails += 1
    if loss_fails == 0:  # loss improved
        _write_text(fail_num_file, "0")
        return
    fail_num = int(_read_text(fail_num_file)) + 1
    if fail_num >= patience:
        _write_text(learning_rate_file, "%s" % (learning_rate * factor))
        _write_text(fail_num_file, "0")
    else:
        _write_text(fail_num_file, "%d" % fail_num)


def _write_play_time(log_folder, t, num_games, max_searches, time_taken, testing):
    """play_time.txt (main.pyx:101-119) from Trainer.stats(): an "evaluation" is one batched call of the network, the
    prediction and play times are the device's kernel times; then score_verbose.txt (main.pyx:121)"""
    st = t.stats()
    evals_done = max(1, int(st["nn_launches"]))
    play_time = st["mcts_ms"] / 1e3
    lines = ["%d games played" % num_games, "%d searches per turn" % max_searches,
             "Training complete in %s" % format_time(time_taken),
             "%s for neural network predictions" % format_time(st["nn_ms"] / 1e3), "%d evaluations" % evals_done,
             "%s per evaluation" % format_time(time_taken / evals_done), "%s for self play" % format_time(play_time)]
    if not testing:
        n = max(1, t.num_samples())
        lines += ["%s average mate length" % t.avg_mate_length(), "%d total turns" % n,
                  "%s average turns per game" % (n / num_games), "%s per turn" % format_time(play_time / n),
                  "%s per search" % format_time(play_time / (n * max_searches))]
    _write_text(os.path.join(log_folder, "play_time.txt"), "\n".join(lines) + "\n")
    t.writeScores(os.path.join(log_folder, "score_verbose.txt"))


# ---------------------------------------------------------------------------------------------------- one generation
def _play(trainer, what, generation, arith):
    try:
        done = trainer.run()
    except _lib.EngineError as e:
        _fp16_range(e, generation, arith)
        raise
    if not done:
        raise RuntimeError("generation %d: %s did not finish" % (generation, what))


def _fp16_range(e, generation, arith):
    if "fp16 range" in str(e):
        raise RuntimeError('generation %d: the network left the fp16 range of arith="%s"; run it with arith="x6" (%s)'
                           % (generation, arith, e)) from e


def _set_net(trainer, kind, weights, slot, generation, arith):
    try:
        trainer.set_net(kind, weights, slot=slot)
    except _lib.EngineError as e:
        _fp16_range(e, generation, arith)
        raise


def train_generation(params, state, *, _cdll=None, _fitter=None, _hook=None):
    """main.pyx:285-365 for the generation state["current_generation"] + 1.  `state` is what Run.setup_generation() gives
    (the keys wrapper.py adds to its params).  Returns a GenerationResult; the metadata is not touched, but for the loss
    appended to metadata/losses.txt (main.pyx:272).
    _cdll: the engine library the trainers use; _fitter: the fitter (fit.Fitter's interface); _hook(stage) is called
    after "selfplay", "fit" and "arena"."""
    p, generation = params, state["current_generation"] + 1
    hook = _hook or (lambda stage: None)
    if _fitter is None:
        with Fitter(max_batch=p.batch_size, device=p.device, net=NETS[p.net][0]) as own:
            return train_generation(params, state, _cdll=_cdll, _fitter=own, _hook=_hook)
    kind = PLAY_KINDS[(p.net, p.arith)]
    times = {}
    # main.pyx:293, 302, 332: one generator a generation, the trainer's seed first, the tester's second
    rng = np.random.default_rng([p.seed, generation])
    seeds = {"selfplay": int(rng.integers(65536)), "arena": int(rng.integers(65536)), "fit": int(rng.integers(2 ** 31))}
    best_weights, _ = load_model(state["best_gen_location"], p.net)  # main.pyx:296

    # self-play (main.pyx:299-317)
    t0 = time.perf_counter()
    trainer = _trainer.Trainer(p.num_games, state["train_log_folder"], seeds["selfplay"], p.max_searches,
                               p.searches_per_eval, p.c_puct, p.epsilon, p.num_logged, max(1, p.num_threads), False,
                               device=p.device, _cdll=_cdll)
    try:
        _set_net(trainer, kind, best_weights, 0, generation, p.arith)
        _play(trainer, "self-play", generation, p.arith)
        times["selfplay"] = time.perf_counter() - t0
        _write_play_time(state["train_log_folder"], trainer, p.num_games, p.max_searches, times["selfplay"], False)
        hook("selfplay")

        # samples (main.pyx:189-219): once to the host for the file, device to device for the fit
        t0 = time.perf_counter()
        state_policy, outcome = trainer.export_samples()
        num_samples = state_policy.shape[0]
        samples_io.save_packed(state["sample_folder"], state_policy, outcome)
        if p.sample_format == "reference":
            samples_io.save_samples(state["sample_folder"],
                                    *_trainer.expand_samples(state_policy, outcome, device=p.device, _cdll=_cdll))
        del state_policy, outcome
        _fitter.clear_data()
        if inspect.getattr_static(_fitter, "set_augmentation", None) is not None:  # the run decides, not what the fitter was left with
            _fitter.set_augmentation(p.augmentation)
        elif p.augmentation != "reference":
            raise ValueError("the fitter %s has no set_augmentation" % type(_fitter).__name__)
        if _fitter.add_trainer_samples(trainer) != num_samples:
            raise RuntimeError("generation %d: the fitter took another number of samples than the file" % generation)
    finally:
        trainer.close()  # main.pyx:324, before the tester is made: its trees are most of the device memory
    for folder in state["old_training_samples"]:  # read and checked like main.pyx:208-217, used only with mix_old
        old_sp, old_oc = samples_io.load_packed(folder)
        if p.mix_old:
            _fitter.add_samples(old_sp, old_oc)
    merged = None
    if p.merge_duplicates:  # after the last add: a set that carries weights takes no more samples
        more = {"symmetries": True} if p.merge_symmetries else {}  # (a fitter from before the keyword serves the plain merge)
        merged = tuple(int(x) for x in _fitter.merge_duplicates(normalize=True, **more))
        print("generation %d: merged %d samples into %d distinct positions" % (generation, merged[0], merged[1]), flush=True)
    times["samples"] = time.perf_counter() - t0

    # fit (main.pyx:221-272): the current generation's model, not the best one's, with its Adam state
    t0 = time.perf_counter()
    cur_weights, cur_optimizer = load_model(state["cur_gen_location"], p.net)
    options, adam, loss = p.fit_options(), p.adam_options(), p.loss_options()
    # the slots the model was saved with, as far as this generation's Adam uses them
    slots = {k: a for k, a in load_model_slots(state["cur_gen_location"]).items()
             if (k == "vhat" and adam.amsgrad) or (k == "average" and adam.averaged())}
    res = fit_resident(_fitter, cur_weights, learning_rate=state["learning_rate"], batch_size=p.batch_size,
                            epochs=p.epochs, validation_split=VALIDATION_SPLIT, anneal_factor=p.anneal_factor,
                            patience=p.patience, seed=seeds["fit"], optimizer_state=cur_optimizer,
                            options=options if options.any() else None, adam=None if adam.is_default() else adam,
                            slots=slots or None, loss=None if loss.is_default() else loss,
                            metrics={"top_k": p.top_k} if p.metrics else False)
    save_model(state["new_model_location"], res.best_weights, res.best_optimizer, p.net, res.best_slots)  # ModelCheckpoint
    times["fit"] = time.perf_counter() - t0
    log = state["train_log_folder"]
    columns = LOSS_COLUMNS + (METRIC_HISTORY_KEYS if p.metrics else ())
    rows = ["\t".join(("epoch",) + columns)]
    for e in range(len(res.history["val_loss"])):
        rows.append("\t".join([str(e)] + [repr(res.history[k][e]) for k in columns]))
    _write_text(os.path.join(log, "train_loss.csv"), "\n".join(rows) + "\n")
    if options.any() or not adam.is_default() or not loss.is_default():  # nothing in it is a time or a path: a generation played again writes the same bytes
        described = {"options": options.as_dict()}
        if options.any():
            described["epochs"] = {k: res.history[k] for k in OPTION_HISTORY_KEYS}
        if not adam.is_default():
            described["adam"] = adam.as_dict()
        if not loss.is_default():
            described["loss"] = loss.as_dict()
        _write_text(os.path.join(log, "fit_options.json"), json.dumps(described, indent=4, sort_keys=True) + "\n")
    n = max(1, num_samples)
    _write_text(os.path.join(log, "fit_time.txt"),  # main.pyx:261-270
                "Neural network fitting completed in %s\n%d samples\n%d batch size\n%d epochs\n%s per epoch\n%s per batch\n"
                % (format_time(times["fit"]), num_samples, p.batch_size, p.epochs, format_time(times["fit"] / p.epochs),
                   format_time(times["fit"] / (p.epochs * n / p.batch_size))))
    write_loss(os.path.join(log, "train_loss.csv"), state["loss_file"])
    hook("fit")

    # arena (main.pyx:327-351): slot 0 the best model, slot 1 the new one (get_predictions, main.pyx:70-83)
    t0 = time.perf_counter()
    tester = _trainer.Trainer(p.num_test_games, state["test_log_folder"], seeds["arena"], p.max_searches,
                              p.searches_per_eval, p.c_puct, p.epsilon, p.num_logged, max(1, p.num_threads), True,
                              device=p.device, _cdll=_cdll)
    try:
        _set_net(tester, kind, best_weights, 0, generation, p.arith)
        _set_net(tester, kind, res.best_weights, 1, generation, p.arith)
        _play(tester, "the arena", generation, p.arith)
        times["arena"] = time.perf_counter() - t0
        score = tester.score()
        _write_play_time(state["test_log_folder"], tester, p.num_test_games, p.max_searches, times["arena"], True)
    finally:
        tester.close()
    _write_text(os.path.join(state["test_log_folder"], "score.txt"), "New agent score %1f!\n" % score)
    rating = update_rating(state["new_rating_file"], state["best_gen_rating"], score)
    hook("arena")
    return GenerationResult(generation=generation, improved=bool(score > p.test_threshold), score=score, rating=rating,
                            fit=res, num_samples=num_samples, seeds=seeds, times=times, merged=merged)


# ---------------------------------------------------------------------------------------------------- the run
class Run:
    """A run directory <cwd>/<name> and the fitter that serves its generations.  Run.open(params) makes or resumes it."""

    def __init__(self, params, *, _cdll=None, _fitter=None):
        self.params = params
        self._cdll = _cdll
        self._fitter, self._own_fitter = _fitter, False
        self.root = os.path.join(params.cwd, params.name)

    @classmethod
    def open(cls, params, *, _cdll=None, _fitter=None):
        """wrapper.py:490-503: an existing <cwd>/<name> is continued, anything else is a new run"""
        if not os.path.isdir(params.cwd):
            os.makedirs(params.cwd)
        if not params.name:
            # wrapper.py:247-250 (whose second line, the time of day, is a statement of its own and never part of the name)
            params = dataclasses.replace(params, name=datetime.now().strftime("_run_%Y%m%d%H%M%S"))
        run = cls(params, _cdll=_cdll, _fitter=_fitter)
        if os.path.isdir(run.root):
            run._check_existing()
        else:
            run._setup_new_run()
        return run

    def close(self):
        if self._own_fitter and self._fitter is not None:
            self._fitter.close()
        self._fitter = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _meta(self, name):
        return os.path.join(self.root, "metadata", name)

    def _gen(self, k, *more):
        return os.path.join(self.root, "generations", "gen_%d" % k, *more)

    def _samples(self, k):
        return os.path.join(self.root, "samples", "gen_%d" % k)

    def _initial_weights(self):
        p = self.params
        w = p.init_weights
        if w is None:
            return NETS[p.net][1](int(np.random.default_rng([p.seed, 0]).integers(2 ** 31)))
        if isinstance(w, (str, os.PathLike)):
            with np.load(w) as z:
                w = z["weights"] if "weights" in z.files else z[z.files[0]]
        w = np.ascontiguousarray(w, dtype=np.float32).ravel()
        if w.size != net_info(NETS[p.net][0])[1]:
            raise ValueError("init_weights: a %s has %d floats, got %d" % (p.net, net_info(NETS[p.net][0])[1], w.size))
        return w

    def _setup_new_run(self):
        """wrapper.py:240-338.  gen_0 holds the initial weights, Adam at zero (a freshly compiled model) and rating 100."""
        p = self.params
        w = self._initial_weights()
        os.mkdir(self.root)
        os.mkdir(os.path.join(self.root, "generations"))
        os.mkdir(self._gen(0))
        save_model(self._gen(0, "model.npz"), w, (np.zeros_like(w), np.zeros_like(w), 0), p.net)
        os.mkdir(os.path.join(self.root, "samples"))
        _write_text(self._gen(0, "rating.txt"), "100")
        os.mkdir(os.path.join(self.root, "metadata"))
        _write_text(self._meta("current_generation.txt"), "0")
        _write_text(self._meta("best_generation.txt"), "0")
        _write_text(self._meta("learning_rate.txt"), "%s" % p.learning_rate)
        _write_text(self._meta("fails.txt"), "0")
        os.mkdir(self._gen(1))
        os.mkdir(self._samples(1))

    def _check_existing(self):
        st = self.state()
        load_model(self._gen(st["current_generation"], "model.npz"), self.params.net)
        load_model(self._gen(st["best_generation"], "model.npz"), self.params.net)

    def state(self):
        """the run's metadata"""
        losses = []
        if os.path.exists(self._meta("losses.txt")):
            with open(self._meta("losses.txt"), encoding="utf-8") as f:
                losses = [float(x) for x in f if x.strip()]
        return {"current_generation": int(_read_text(self._meta("current_generation.txt"))),
                "best_generation": int(_read_text(self._meta("best_generation.txt"))),
                "learning_rate": float(_read_text(self._meta("learning_rate.txt"))),
                "fails": int(_read_text(self._meta("fails.txt"))), "losses": losses}

    def setup_generation(self):
        """setup_existing_run and start_generation (wrapper.py:164-237, 341-372): the state of the coming generation,
        its folders made anew -- whatever an interrupted attempt left in them goes"""
        p, meta = self.params, self.state()
        cur, best = meta["current_generation"], meta["best_generation"]
        old = [self._samples(g) for g in range(max(1, cur - p.num_old_gens + 1), cur + 1)]
        new_gen_folder = self._gen(cur + 1)
        state = {
            "cur_gen_location": self._gen(cur, "model.npz"), "best_gen_location": self._gen(best, "model.npz"),
            "old_training_samples": [f for f in old if os.path.isdir(f)], "learning_rate": meta["learning_rate"],
            "best_gen_rating": float(_read_text(self._gen(best, "rating.txt"))),
            "new_rating_file": os.path.join(new_gen_folder, "rating.txt"), "current_generation": cur,
            "best_generation": best, "new_gen_samples": self._samples(cur + 1),
            "new_model_location": os.path.join(new_gen_folder, "model.npz"), "sample_folder": self._samples(cur + 1),
        }
        for folder in (new_gen_folder, state["sample_folder"]):
            if os.path.isdir(folder):
                shutil.rmtree(folder)
            os.mkdir(folder)
        if len(meta["losses"]) > cur:  # the line of an interrupted attempt (see the module docstring)
            with open(self._meta("losses.txt"), encoding="utf-8") as f:
                kept = [x for x in f if x.strip()][:cur]
            _write_text(self._meta("losses.txt"), "".join(kept))
        train_log_folder, test_log_folder = os.path.join(new_gen_folder, "training_logs"), os.path.join(new_gen_folder, "testing_logs")
        os.mkdir(train_log_folder)
        os.mkdir(test_log_folder)
        described = dict(p.as_dict(), **state)
        described["start_time"] = str(datetime.now().astimezone())
        _write_text(os.path.join(new_gen_folder, "metadata.txt"), json.dumps(described, ensure_ascii=False, indent=4))
        state.update(loss_file=self._meta("losses.txt"), train_log_folder=train_log_folder, test_log_folder=test_log_folder)
        return state

    def _update_run_data(self, state, improved):
        """wrapper.py:375-429.  current_generation.txt goes last: until it is written the generation is not finished
        and a reopened run plays it again."""
        p = self.params
        cur = state["current_generation"]
        if p.zip_logs:  # wrapper.py:390-400
            zips = os.path.join(p.cwd, "zips")
            if os.path.isdir(zips):
                shutil.rmtree(zips)
            os.mkdir(zips)
            shutil.make_archive(os.path.join(zips, "%s_%d" % (p.name, cur + 1)), "zip", self.root)
        best = cur + 1 if improved else state["best_generation"]
        write_learning_rate(best, cur + 1, self._meta("losses.txt"), self._meta("learning_rate.txt"),
                            self._meta("fails.txt"), state["learning_rate"], p.patience, p.anneal_factor)
        if improved:
            _write_text(self._meta("best_generation.txt"), "%d" % best)
        _write_text(self._meta("current_generation.txt"), "%d" % (cur + 1))

    def generation(self, *, _hook=None):
        """one call of wrapper.py's main(): set up, train_generation, post-processing.  -> GenerationResult"""
        p = self.params
        if self._fitter is None:
            self._fitter = Fitter(max_batch=p.batch_size, device=p.device, net=NETS[p.net][0])
            self._own_fitter = True
        state = self.setup_generation()
        res = train_generation(p, state, _cdll=self._cdll, _fitter=self._fitter, _hook=_hook)
        self._update_run_data(state, res.improved)
        return res


# ---------------------------------------------------------------------------------------------------- command line
def read_config(path):
    """the flat [hyperparameters] table of the reference's toml/train.toml and toml/test.toml (main.py:46-51)"""
    for name in ("tomllib", "tomli"):
        try:
            mod = __import__(name)
        except ImportError:
            continue
        with open(path, "rb") as f:
            return dict(mod.load(f)["hyperparameters"])
    table, section = {}, None
    with open(path, encoding="utf-8") as f:
        for number, raw in enumerate(f, 1):
            line = raw.strip()
            if not line or line.startswith("#"):
                continue
            if line.startswith("["):
                section = line.strip("[] \t")
                continue
            key, eq, value = (x.strip() for x in line.partition("="))
            if not eq or not key:
                raise ValueError("%s:%d: expected `key = value`" % (path, number))
            if section != "hyperparameters":
                continue
            if value[:1] in "\"'":
                end = value.find(value[0], 1)
                if end < 0:
                    raise ValueError("%s:%d: unterminated string" % (path, number))
                table[key] = value[1:end]
                continue
            value = value.split("#", 1)[0].strip()
            if value in ("true", "false"):
                table[key] = value == "true"
                continue
            try:
                table[key] = int(value.replace("_", ""))
            except ValueError:
                try:
                    table[key] = float(value.replace("_", ""))
                except ValueError:
                    raise ValueError("%s:%d: %r is no int, float, bool or quoted string" % (path, number, value)) from None
    return table


def _parser():
    ap = argparse.ArgumentParser(prog="python -m corintho_ai_amd.run",
                                 description="Train generations of a run on the MI355X engine (the reference's wrapper.py).")
    ap.add_argument("--config", help="TOML file whose [hyperparameters] table gives the flags' values (toml/train.toml)")
    ap.add_argument("--generations", type=int, default=1, help="generations to train (main.py -n). Default 1.")
    helps = {
        "anneal_factor": "Factor to reduce the learning rate upon plateau", "batch_size": "Batch size of the fit",
        "c_puct": "c_puct of the search", "cwd": "Folder in which all logging resides", "epochs": "Epochs of the fit",
        "epsilon": "Weight of the root's Dirichlet noise", "learning_rate": "Learning rate of a new run",
        "max_searches": "Searches per turn", "name": "Name of the run: the folder <cwd>/<name> is made, or continued "
        "if it exists; empty: a name from the time", "num_games": "Self-play games of a generation",
        "num_logged": "Games to log", "num_old_gens": "Earlier generations in the replay window",
        "num_test_games": "Arena games of a generation", "num_threads": "Accepted and ignored",
        "patience": "Epochs (fit) or failed generations (run) before the learning rate is reduced",
        "searches_per_eval": "Searches gathered before one network evaluation",
        "test_threshold": "Score (exclusive) above which the new generation becomes the best",
        "net": "mlp12x100 or rescnn4", "arith": "Arithmetic of self-play and arena: h3, f32, x6 or x3",
        "device": "HIP device ordinal", "seed": "Seed of the run; default: from the clock",
        "sample_format": "packed, or reference to write the three expanded files as well",
        "init_weights": ".npz with the weights of generation 0",
        "l1": "L1 factor of the fit's regulariser", "l2": "L2 factor of the fit's regulariser",
        "regularize": "What l1 and l2 act on: 0 the trunk kernels, 1 all kernels",
        "weight_decay": "Decoupled weight decay of the fit's Adam, on the kernels",
        "clipvalue": "Clip every gradient entry of the fit to [-c, c]",
        "clipnorm": "Clip every tensor's gradient of the fit to this norm",
        "global_clipnorm": "Clip the fit's whole gradient to this norm",
        "beta_1": "beta_1 of the fit's Adam", "beta_2": "beta_2 of the fit's Adam",
        "adam_epsilon": "epsilon of the fit's Adam",
        "ema_momentum": "Momentum of the fit's averaged weights (Keras use_ema); 0: none",
        "ema_overwrite_frequency": "Every this many steps the weights become the average; 0: never",
        "value_weight": "Weight of the value loss in the fit's loss", "policy_weight": "Weight of the policy loss in the fit's loss",
        "label_smoothing": "Label smoothing of the policy cross-entropy, in [0, 1)",
        "value_loss": "Value loss of the fit: mse or huber", "huber_delta": "delta of the Huber value loss",
        "top_k": "k of the top-k accuracy metric, 1..96",
    }
    for f in dataclasses.fields(RunParams):
        if f.name in ("mix_old", "zip_logs"):
            ap.add_argument("--" + f.name, action="store_true", default=False)
        elif f.name == "merge_duplicates":
            ap.add_argument("--merge-duplicates", "--merge_duplicates", dest="merge_duplicates", action="store_true",
                            default=False, help="Merge duplicate positions of the fit's samples into weighted ones")
        elif f.name == "merge_symmetries":
            ap.add_argument("--merge-symmetries", "--merge_symmetries", dest="merge_symmetries", action="store_true",
                            default=False, help="Merge positions that are images of one another under the eight "
                            "symmetries as well (implies --merge-duplicates)")
        elif f.name == "augmentation":
            ap.add_argument("--augmentation", choices=sorted(samples_io.AUGMENTATIONS), default="reference",
                            help="Move table of the fit's symmetry expansion: reference (the reference's pairing) or "
                            "consistent (rows 2 and 6 exchanged, so that policy and state turn alike). Default reference.")
        elif f.name == "amsgrad":
            ap.add_argument("--amsgrad", action="store_true", default=False, help="AMSGrad variant of the fit's Adam")
        elif f.name == "metrics":
            ap.add_argument("--metrics", action="store_true", default=False,
                            help="Log accuracy, top-k accuracy, value error and entropies per epoch in train_loss.csv")
        elif f.name in ("seed", "init_weights"):
            ap.add_argument("--" + f.name, type=int if f.name == "seed" else str, default=None, help=helps[f.name])
        else:
            ap.add_argument("--" + f.name, type=type(f.default), default=f.default,
                            help="%s. Default %r." % (helps[f.name], f.default))
    return ap


def parse_args(argv=None):
    """-> (RunParams, generations).  Values come from the flags, then from --config's table, then from the defaults."""
    argv = list(sys.argv[1:] if argv is None else argv)
    ap = _parser()
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--config")
    config = pre.parse_known_args(argv)[0].config
    if config:
        table = read_config(config)
        known = {f.name for f in dataclasses.fields(RunParams)}
        unknown = sorted(set(table) - known)
        if unknown:
            ap.error("%s: unknown hyperparameters %s" % (config, ", ".join(unknown)))
        ap.set_defaults(**table)
    args = vars(ap.parse_args(argv))
    generations = max(1, args.pop("generations"))
    args.pop("config")
    return RunParams(**args), generations


def main(argv=None):
    params, generations = parse_args(argv)
    with Run.open(params) as run:
        for _ in range(generations):
            r = run.generation()
            print("generation %d: %d samples, val_loss %.6f, score %.4f, rating %.1f, %s; self-play %.2fs, samples %.2fs, "
                  "fit %.2fs, arena %.2fs" % (r.generation, r.num_samples, r.val_loss, r.score, r.rating,
                                              "improved" if r.improved else "not improved", r.times["selfplay"],
                                              r.times["samples"], r.times["fit"], r.times["arena"]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
