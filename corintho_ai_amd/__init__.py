"""corintho_ai_amd -- MI355X-native self-play engine for Corintho (hot path of
maxjiang216/corintho-ai behind the reference's Trainer interface)."""
from .trainer import (NET_MLP12X100, NET_MLP12X100_H3, NET_MLP12X100_X3, NET_MLP12X100_X6, NET_RESCNN4,  # noqa: F401
                      NET_RESCNN4_H3, NET_RESCNN4_X3, NET_RESCNN4_X6, Trainer, expand_samples)
from .tourney import Tourney  # noqa: F401
from .net import Net, NetGroup  # noqa: F401
from .fit import (AdamOptions, FitOptions, FitResult, Fitter, LossOptions, fit, fit_resident, fit_samples,  # noqa: F401,E402
                  fit_trainer)


def __getattr__(name):
    # Run, RunParams, train_generation: imported on first use, so that `python -m corintho_ai_amd.run` does not find its
    # module imported before it runs
    if name in ("Run", "RunParams", "train_generation"):
        from . import run

        return getattr(run, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
