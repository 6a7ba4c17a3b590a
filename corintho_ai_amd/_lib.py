"""Loader of libcorintho_hip.so (the HIP engine, C ABI in include/corintho_hip.h).

The product has no CPU fallback: if the library is missing or no gfx950 device
is visible, loading / creating a Trainer raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcorintho_hip.so")

f32p = C.POINTER(C.c_float)
i32p = C.POINTER(C.c_int32)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
# ca_net_fn: int fn(void *user, int32_t row0, int32_t cap_rows, const int32_t *d_rows, void *stream)
NET_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p)
CA_ERR_CALLBACK = -6


class CaConfig(C.Structure):
    """ca_config (include/corintho_hip.h)"""

    _fields_ = [
        ("num_games", C.c_int32),
        ("seed", C.c_int32),
        ("max_searches", C.c_int32),
        ("searches_per_eval", C.c_int32),
        ("c_puct", C.c_float),
        ("epsilon", C.c_float),
        ("num_logged", C.c_int32),
        ("num_threads", C.c_int32),
        ("testing", C.c_int32),
        ("device", C.c_int32),
        ("no_stagger", C.c_int32),
        ("arena_units", C.c_uint32),
        ("trace", C.c_int32),
        ("game_base", C.c_int32),
        ("total_games", C.c_int32),
        ("pools", C.c_int32),
        ("analyse", C.c_int32),
        ("resident", C.c_int32),
        ("eval_cache", C.c_int32),
        ("step_budget", C.c_int32),
    ]


class CaStats(C.Structure):
    _fields_ = [
        ("searches", C.c_int64),
        ("evals", C.c_int64),
        ("nodes", C.c_int64),
        ("plies", C.c_int64),
        ("iterations", C.c_int64),
        ("peak_arena_units", C.c_int64),
        ("mcts_ms", C.c_double),
        ("nn_ms", C.c_double),
        ("pack_ms", C.c_double),
        ("mcts_launches", C.c_int64),
        ("nn_launches", C.c_int64),
        ("nn_rows", C.c_int64),
        ("pools", C.c_int64),
        ("timed_launches", C.c_int64),
        ("nn_timed_rows", C.c_int64),
        ("mcts_timed_ms", C.c_double),
        ("nn_timed_ms", C.c_double),
        ("resident_slots", C.c_int64),
        ("nn_rows_evaluated", C.c_int64),
        ("steps_cut", C.c_int64),
        ("step_budget_last", C.c_int64),
        ("tourney_path", C.c_int64),
    ]


class CaFitOptions(C.Structure):
    """ca_fit_options (include/corintho_hip.h, "fit options"); struct_size is filled in by whoever passes it"""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("regularize", C.c_int32),
        ("l1", C.c_float),
        ("l2", C.c_float),
        ("weight_decay", C.c_float),
        ("clipvalue", C.c_float),
        ("clipnorm", C.c_float),
        ("global_clipnorm", C.c_float),
    ]


class CaFitAdam(C.Structure):
    """ca_fit_adam (include/corintho_hip.h, "Adam's arguments"); the defaults are not zeros: fit.AdamOptions has them"""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("beta_1", C.c_float),
        ("beta_2", C.c_float),
        ("epsilon", C.c_float),
        ("amsgrad", C.c_int32),
        ("ema_momentum", C.c_float),
        ("ema_overwrite_frequency", C.c_int32),
    ]


class CaFitLoss(C.Structure):
    """ca_fit_loss (include/corintho_hip.h, "loss and metrics"); the defaults are not zeros: fit.LossOptions has them"""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("value_weight", C.c_float),
        ("policy_weight", C.c_float),
        ("label_smoothing", C.c_float),
        ("value_loss", C.c_int32),
        ("huber_delta", C.c_float),
    ]


class CaFitMetrics(C.Structure):
    """ca_fit_metrics"""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("top_k", C.c_int32),
        ("rows", C.c_int64),
        ("weight_sum", C.c_double),
        ("categorical_accuracy", C.c_double),
        ("top_k_categorical_accuracy", C.c_double),
        ("mean_absolute_error", C.c_double),
        ("policy_entropy", C.c_double),
        ("target_entropy", C.c_double),
    ]


class CaFitStats(C.Structure):
    """ca_fit_stats"""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("reserved", C.c_uint32),
        ("steps", C.c_int64),
        ("clipped_steps", C.c_int64),
        ("regularization", C.c_double),
        ("grad_norm", C.c_double),
        ("grad_norm_max", C.c_double),
    ]


# every symbol include/corintho_hip.h declares
EXPORTS = [
    "ca_last_error", "ca_device_check", "ca_trainer_create", "ca_trainer_destroy", "ca_trainer_num_requests",
    "ca_trainer_num_samples", "ca_trainer_score", "ca_trainer_avg_mate_length", "ca_trainer_write_requests",
    "ca_trainer_write_samples", "ca_trainer_write_scores", "ca_trainer_do_iteration", "ca_trainer_set_net",
    "ca_trainer_run", "ca_trainer_set_host_cache", "ca_trainer_net_forward", "ca_trainer_net_bench", "ca_trainer_export_samples", "ca_trainer_pack_samples_device", "ca_trainer_pin_host", "ca_trainer_unpin_host", "ca_trainer_set_positions", "ca_trainer_analysis", "ca_trainer_finish", "ca_trainer_set_logging", "ca_trainer_reset", "ca_expand_samples", "ca_trainer_stats",
    "ca_trainer_game_info", "ca_trainer_trace", "ca_trainer_prof", "ca_rules_legal_moves", "ca_rules_do_move", "ca_rules_rows", "ca_rng_draw",
    "ca_fp_probe",
    "ca_tourney_create", "ca_tourney_destroy", "ca_tourney_set_log_folder", "ca_tourney_add_player", "ca_tourney_add_match", "ca_tourney_all_done",
    "ca_tourney_num_requests", "ca_tourney_write_requests", "ca_tourney_do_iteration", "ca_tourney_write_scores",
    "ca_tourney_set_net", "ca_tourney_run", "ca_tourney_set_exact_offsets", "ca_tourney_num_matches", "ca_tourney_match_info", "ca_tourney_match_score", "ca_tourney_trace", "ca_tourney_stats",
    "ca_fitter_create", "ca_fitter_create_net", "ca_fitter_destroy", "ca_fitter_set_weights", "ca_fitter_get_weights", "ca_fitter_set_optimizer",
    "ca_fitter_get_optimizer", "ca_fitter_set_data", "ca_fitter_train", "ca_fitter_evaluate", "ca_fitter_gradients",
    "ca_trainer_device", "ca_fitter_clear_data", "ca_fitter_add_samples", "ca_fitter_add_device_samples",
    "ca_fitter_add_trainer_samples", "ca_fitter_drop_samples", "ca_fitter_data_info", "ca_fitter_fetch_rows",
    "ca_trainer_request_rows", "ca_trainer_set_net_fn", "ca_tourney_set_net_fn", "ca_net_create", "ca_net_forward_device",
    "ca_net_destroy",
    "ca_tourney_set_grouped", "ca_tourney_set_seed", "ca_net_group_create", "ca_net_group_forward", "ca_net_group_info", "ca_net_group_tables",
    "ca_net_group_bench", "ca_net_group_destroy",
    "ca_fitter_set_sample_weights", "ca_fitter_get_sample_weights", "ca_fitter_merge_duplicates",
    "ca_net_forward_device_io",
    "ca_fitter_set_options", "ca_fitter_get_options", "ca_fitter_train_stats", "ca_fitter_tensor_table",
    "ca_fitter_set_adam", "ca_fitter_get_adam", "ca_fitter_set_slot", "ca_fitter_get_slot", "ca_fitter_swap_average",
    "ca_fitter_apply_average",
    "ca_fitter_set_loss", "ca_fitter_get_loss", "ca_fitter_set_metrics", "ca_fitter_metrics", "ca_fitter_predict",
    "ca_fitter_set_augmentation", "ca_fitter_get_augmentation", "ca_fitter_canonicalize",
]
# the caller-supplied network: an earlier build of the library has none of these
NET_FN_EXPORTS = ["ca_trainer_request_rows", "ca_trainer_set_net_fn", "ca_tourney_set_net_fn", "ca_net_create", "ca_net_forward_device",
                  "ca_net_destroy"]
# grouped multi-model inference and the rating driver's tournament entries: likewise
GROUP_EXPORTS = ["ca_tourney_set_grouped", "ca_tourney_set_seed", "ca_net_group_create", "ca_net_group_forward", "ca_net_group_info",
                 "ca_net_group_tables", "ca_net_group_bench", "ca_net_group_destroy"]
# sample weights and the merging of duplicate positions: likewise
WEIGHT_EXPORTS = ["ca_fitter_set_sample_weights", "ca_fitter_get_sample_weights", "ca_fitter_merge_duplicates"]
# a network launch with a fused run's indirection: likewise
NET_IO_EXPORTS = ["ca_net_forward_device_io"]
# the fit options (regulariser, weight decay, clipping): likewise
OPTION_EXPORTS = ["ca_fitter_set_options", "ca_fitter_get_options", "ca_fitter_train_stats", "ca_fitter_tensor_table"]
# Adam's arguments, the third slot and the averaged weights: likewise
ADAM_EXPORTS = ["ca_fitter_set_adam", "ca_fitter_get_adam", "ca_fitter_set_slot", "ca_fitter_get_slot", "ca_fitter_swap_average",
                "ca_fitter_apply_average"]
# the loss options, the metrics and predict: likewise
LOSS_EXPORTS = ["ca_fitter_set_loss", "ca_fitter_get_loss", "ca_fitter_set_metrics", "ca_fitter_metrics", "ca_fitter_predict"]
# the augmentation choice of a packed set and the canonical orientation: likewise
AUG_EXPORTS = ["ca_fitter_set_augmentation", "ca_fitter_get_augmentation", "ca_fitter_canonicalize"]
assert set(NET_FN_EXPORTS + GROUP_EXPORTS + WEIGHT_EXPORTS + NET_IO_EXPORTS + OPTION_EXPORTS + ADAM_EXPORTS
           + LOSS_EXPORTS + AUG_EXPORTS) <= set(EXPORTS)


def declare(L):
    vp = C.c_void_p
    L.ca_last_error.restype = C.c_char_p
    L.ca_device_check.argtypes = [C.c_int]
    L.ca_trainer_create.argtypes = [C.POINTER(CaConfig), C.POINTER(vp)]
    L.ca_trainer_destroy.argtypes = [vp]
    L.ca_trainer_destroy.restype = None
    L.ca_trainer_num_requests.argtypes = [vp, C.c_int, i32p]
    L.ca_trainer_num_samples.argtypes = [vp, i32p]
    L.ca_trainer_score.argtypes = [vp, f32p]
    L.ca_trainer_avg_mate_length.argtypes = [vp, f32p]
    L.ca_trainer_write_requests.argtypes = [vp, f32p, C.c_int]
    L.ca_trainer_write_samples.argtypes = [vp, f32p, f32p, f32p]
    L.ca_trainer_write_scores.argtypes = [vp, C.c_char_p]
    L.ca_trainer_do_iteration.argtypes = [vp, f32p, f32p, C.c_int, i32p]
    L.ca_trainer_set_net.argtypes = [vp, C.c_int, C.c_int, f32p, C.c_size_t]
    L.ca_trainer_run.argtypes = [vp, C.c_int64, i32p]
    L.ca_trainer_set_host_cache.argtypes = [vp, C.c_int32]
    L.ca_trainer_net_forward.argtypes = [vp, C.c_int, f32p, C.c_int32, f32p, f32p]
    L.ca_trainer_net_bench.argtypes = [vp, C.c_int, f32p, C.c_int32, C.c_int32, f32p]
    L.ca_trainer_export_samples.argtypes = [vp, f32p, f32p]
    L.ca_trainer_pack_samples_device.argtypes = [vp, C.c_void_p, C.c_void_p, C.c_int32, i32p]
    L.ca_trainer_pin_host.argtypes = [vp, C.c_void_p, C.c_size_t, i32p]
    L.ca_trainer_unpin_host.argtypes = [vp, C.c_void_p]
    L.ca_trainer_set_positions.argtypes = [vp, i32p, i32p, i32p, i32p]
    L.ca_trainer_analysis.argtypes = [vp, i32p]
    L.ca_trainer_finish.argtypes = [vp]
    L.ca_trainer_set_logging.argtypes = [vp, C.c_char_p, C.c_int32]
    L.ca_trainer_reset.argtypes = [vp, C.c_int32]
    L.ca_trainer_device.argtypes = [vp, i32p]
    L.ca_expand_samples.argtypes = [C.c_int, f32p, f32p, C.c_int32, f32p, f32p, f32p]
    L.ca_trainer_stats.argtypes = [vp, C.POINTER(CaStats)]
    L.ca_trainer_game_info.argtypes = [vp, C.c_int, i32p]
    L.ca_trainer_trace.argtypes = [vp, C.c_int, i32p, C.c_int32, i32p]
    L.ca_trainer_prof.argtypes = [vp, C.POINTER(C.c_ulonglong)]
    L.ca_rules_legal_moves.argtypes = [C.c_int, u64p, u32p, C.c_int32, u32p, i32p]
    L.ca_rules_do_move.argtypes = [C.c_int, u64p, u32p, i32p, C.c_int32, f32p]
    L.ca_rules_rows.argtypes = [C.c_int, u64p, u32p, i32p, C.c_int32, u32p]
    L.ca_rng_draw.argtypes = [C.c_int, C.c_uint32, C.c_int32, C.c_int32, u32p]
    L.ca_fp_probe.argtypes = [C.c_int, f32p, C.c_int32, f32p]
    L.ca_tourney_create.argtypes = [C.c_int, C.c_uint32, C.c_int, C.POINTER(vp)]
    L.ca_tourney_set_log_folder.argtypes = [vp, C.c_char_p]
    L.ca_tourney_destroy.argtypes = [vp]
    L.ca_tourney_destroy.restype = None
    L.ca_tourney_add_player.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int32]
    L.ca_tourney_add_match.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32]
    L.ca_tourney_all_done.argtypes = [vp, i32p]
    L.ca_tourney_num_requests.argtypes = [vp, C.c_int32, i32p]
    L.ca_tourney_write_requests.argtypes = [vp, f32p, C.c_int32]
    L.ca_tourney_do_iteration.argtypes = [vp, f32p, f32p, C.c_int32, C.c_int32]
    L.ca_tourney_write_scores.argtypes = [vp, C.c_char_p]
    L.ca_tourney_set_net.argtypes = [vp, C.c_int32, C.c_int32, f32p, C.c_size_t]
    L.ca_tourney_run.argtypes = [vp, C.c_int64, i32p]
    L.ca_tourney_set_exact_offsets.argtypes = [vp, C.c_int32]
    L.ca_tourney_num_matches.argtypes = [vp, i32p]
    L.ca_tourney_match_info.argtypes = [vp, C.c_int32, i32p]
    L.ca_tourney_match_score.argtypes = [vp, C.c_int32, f32p]
    L.ca_tourney_trace.argtypes = [vp, C.c_int32, i32p, C.c_int32, i32p]
    L.ca_tourney_stats.argtypes = [vp, C.POINTER(CaStats)]
    net_fn = hasattr(L, "ca_trainer_set_net_fn")  # an earlier build of the library (tools/ab.py compares against them) has none
    if net_fn:
        L.ca_trainer_request_rows.argtypes = [vp, i32p]
        L.ca_trainer_set_net_fn.argtypes = [vp, C.c_int, NET_FN, vp, vp, vp, vp, C.c_int32, C.c_double]
        L.ca_tourney_set_net_fn.argtypes = [vp, C.c_int32, NET_FN, vp, vp, vp, vp, C.c_int32, C.c_double]
        L.ca_net_create.argtypes = [C.c_int, C.c_int, f32p, C.c_size_t, C.c_int32, C.POINTER(vp)]
        L.ca_net_forward_device.argtypes = [vp, vp, C.c_int32, vp, vp, vp, vp]
        L.ca_net_destroy.argtypes = [vp]
        L.ca_net_destroy.restype = None
    if hasattr(L, "ca_net_forward_device_io"):  # (as above)
        L.ca_net_forward_device_io.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, vp, vp, vp, C.c_int32, vp, C.c_int32, C.c_int32, vp]
    group = hasattr(L, "ca_net_group_create")  # (as above: an earlier build has none)
    if group:
        L.ca_tourney_set_grouped.argtypes = [vp, C.c_int32]
        L.ca_tourney_set_seed.argtypes = [vp, C.c_uint32]
        L.ca_net_group_create.argtypes = [C.c_int, C.c_int, C.POINTER(f32p), C.c_int32, C.c_size_t, C.c_int32, C.POINTER(vp)]
        L.ca_net_group_forward.argtypes = [vp, f32p, i32p, C.c_int32, f32p, f32p]
        L.ca_net_group_info.argtypes = [vp, i32p]
        L.ca_net_group_bench.argtypes = [vp, f32p, i32p, C.c_int32, C.c_int32, f32p]
        L.ca_net_group_tables.argtypes = [vp, i32p, i32p, i32p, i32p, i32p]
        L.ca_net_group_destroy.argtypes = [vp]
        L.ca_net_group_destroy.restype = None
    f64p = C.POINTER(C.c_double)
    fitter = hasattr(L, "ca_fitter_create")  # the emulation build of the engine (tests/emu) has no training kernels
    if fitter:
        _declare_fitter(L, vp, f64p)
    for name in EXPORTS:
        if name.startswith("ca_fitter_") and not fitter:
            continue
        if name in NET_FN_EXPORTS and not net_fn:
            continue
        if name in GROUP_EXPORTS and not group:
            continue
        if (name in WEIGHT_EXPORTS + NET_IO_EXPORTS + OPTION_EXPORTS + ADAM_EXPORTS + LOSS_EXPORTS + AUG_EXPORTS
                and not hasattr(L, name)):
            continue
        fn = getattr(L, name)
        if name not in ("ca_last_error", "ca_trainer_destroy", "ca_tourney_destroy", "ca_fitter_destroy", "ca_net_destroy",
                        "ca_net_group_destroy"):
            fn.restype = C.c_int
    return L


def _declare_fitter(L, vp, f64p):
    L.ca_fitter_create.argtypes = [C.c_int, C.c_int32, C.POINTER(vp)]
    L.ca_fitter_create_net.argtypes = [C.c_int, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.ca_fitter_destroy.argtypes = [vp]
    L.ca_fitter_destroy.restype = None
    L.ca_fitter_set_weights.argtypes = [vp, f32p, C.c_size_t]
    L.ca_fitter_get_weights.argtypes = [vp, f32p, C.c_size_t]
    L.ca_fitter_set_optimizer.argtypes = [vp, f32p, f32p, C.c_size_t, C.c_int64]
    L.ca_fitter_get_optimizer.argtypes = [vp, f32p, f32p, C.c_size_t, C.POINTER(C.c_int64)]
    L.ca_fitter_set_data.argtypes = [vp, f32p, f32p, f32p, C.c_int32]
    L.ca_fitter_train.argtypes = [vp, i32p, C.c_int32, C.c_int32, C.c_float, f64p, f32p]
    L.ca_fitter_evaluate.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, f64p]
    L.ca_fitter_gradients.argtypes = [vp, i32p, C.c_int32, f32p, f64p]
    L.ca_fitter_clear_data.argtypes = [vp]
    L.ca_fitter_add_samples.argtypes = [vp, f32p, f32p, C.c_int32]
    L.ca_fitter_add_device_samples.argtypes = [vp, C.c_void_p, C.c_void_p, C.c_int32]
    L.ca_fitter_add_trainer_samples.argtypes = [vp, vp, i32p]
    L.ca_fitter_drop_samples.argtypes = [vp, C.c_int32]
    L.ca_fitter_data_info.argtypes = [vp, i32p, i32p]
    L.ca_fitter_fetch_rows.argtypes = [vp, i32p, C.c_int32, f32p, f32p, f32p]
    if hasattr(L, "ca_fitter_merge_duplicates"):  # (an earlier build has none of these)
        L.ca_fitter_set_sample_weights.argtypes = [vp, f32p, C.c_int32]
        L.ca_fitter_get_sample_weights.argtypes = [vp, f32p, C.c_int32]
        L.ca_fitter_merge_duplicates.argtypes = [vp, C.c_int, i32p, i32p]
    if hasattr(L, "ca_fitter_set_options"):  # (likewise)
        L.ca_fitter_set_options.argtypes = [vp, C.POINTER(CaFitOptions)]
        L.ca_fitter_get_options.argtypes = [vp, C.POINTER(CaFitOptions)]
        L.ca_fitter_train_stats.argtypes = [vp, C.POINTER(CaFitStats)]
        L.ca_fitter_tensor_table.argtypes = [vp, i32p, C.c_int32, i32p]
    if hasattr(L, "ca_fitter_set_adam"):  # (likewise)
        L.ca_fitter_set_adam.argtypes = [vp, C.POINTER(CaFitAdam)]
        L.ca_fitter_get_adam.argtypes = [vp, C.POINTER(CaFitAdam)]
        L.ca_fitter_set_slot.argtypes = [vp, C.c_int32, f32p, C.c_size_t]
        L.ca_fitter_get_slot.argtypes = [vp, C.c_int32, f32p, C.c_size_t]
        L.ca_fitter_swap_average.argtypes = [vp]
        L.ca_fitter_apply_average.argtypes = [vp]
    if hasattr(L, "ca_fitter_set_loss"):  # (likewise)
        L.ca_fitter_set_loss.argtypes = [vp, C.POINTER(CaFitLoss)]
        L.ca_fitter_get_loss.argtypes = [vp, C.POINTER(CaFitLoss)]
        L.ca_fitter_set_metrics.argtypes = [vp, C.c_int32, C.c_int32]
        L.ca_fitter_metrics.argtypes = [vp, C.POINTER(CaFitMetrics)]
        L.ca_fitter_predict.argtypes = [vp, i32p, C.c_int32, C.c_int32, f32p, f32p]
    if hasattr(L, "ca_fitter_canonicalize"):  # (likewise)
        L.ca_fitter_set_augmentation.argtypes = [vp, C.c_int32]
        L.ca_fitter_get_augmentation.argtypes = [vp, i32p]
        L.ca_fitter_canonicalize.argtypes = [vp, i32p]


_lib = None


def load():
    """The HIP engine.  Raises ImportError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "corintho_ai_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % LIB_PATH
            )
        _lib = declare(C.CDLL(LIB_PATH))
    return _lib


class EngineError(RuntimeError):
    pass


def check(L, rc):
    if rc != 0:
        msg = L.ca_last_error()
        raise EngineError("corintho_hip error %d: %s" % (rc, msg.decode() if msg else "?"))


class NetCallback:
    """A Python function fn(row0, cap_rows, d_rows_ptr, stream_ptr) as a ca_net_fn.  Whatever fn raises is kept in
    `error` and reported to the library as a failure (return 1); the object must live as long as the slot it serves."""

    def __init__(self, fn):
        self.fn = fn
        self.error = None

        def call(_user, row0, cap_rows, d_rows, stream):
            try:
                fn(row0, cap_rows, d_rows or 0, stream or 0)
                return 0
            except BaseException as e:  # noqa: B902 -- nothing may unwind through the C frames above
                self.error = e
                return 1

        self.c = NET_FN(call)


def check_callbacks(L, rc, callbacks):
    """check() for a call that may have run caller-supplied network functions: CA_ERR_CALLBACK re-raises what the
    function raised, chained to the library's error"""
    if rc == CA_ERR_CALLBACK:
        for cb in callbacks:
            if cb.error is not None:
                err, cb.error = cb.error, None
                msg = L.ca_last_error()
                raise err from EngineError("corintho_hip error %d: %s" % (rc, msg.decode() if msg else "?"))
    check(L, rc)
