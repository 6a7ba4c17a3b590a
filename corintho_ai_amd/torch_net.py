"""A torch-ROCm module as the network of fused mode (Trainer.set_net_fn): the whole generation stays on the device and
the module is called inside run(), on the run's streams, on device tensors.

    net = TorchNet(model, trainer)     # owns the three device tensors and registers itself as slot 0
    trainer.run()

`model(states [n][70] float32)` returns what the reference's Keras model returns (main.pyx:70-83): the value, [n] or
[n, 1], and the probabilities, [n, 96], both float32.  It is called with torch.inference_mode() under
torch.cuda.stream(ExternalStream(the pool's HIP stream)) on ALL the rows a launch can hold; the rows beyond the
launch's count are zero and their answers ignored.  With the evaluation cache on, the model must give a row the same
outputs in whatever batch it stands.  Keep the TorchNet alive as long as the trainer uses it.

torch is imported here only: `import corintho_ai_amd` does not import it.

ONE HIP RUNTIME.  A torch-ROCm wheel carries its own copy of the HIP runtime, and a stream handle or a device pointer
means something only to the copy that made it.  Import torch (or this module) BEFORE the first Trainer, Tourney, Fitter
or Net is created: the engine's library, loaded at that moment, then binds to the runtime torch has brought (same
SONAME) and the process holds one.  The other way round the process gets two, and torch finds no device.
"""
import torch

from .trainer import GAME_STATE_SIZE, NUM_MOVES


class TorchNet:
    def __init__(self, model, trainer, slot=0, flop_per_row=0.0):
        self.model = model
        self.rows = trainer.request_rows()
        self.device = torch.device("cuda", trainer.device)
        try:
            self.states = torch.zeros((self.rows, GAME_STATE_SIZE), dtype=torch.float32, device=self.device)
        except RuntimeError as e:
            raise RuntimeError("TorchNet: torch cannot use device %s (%s) -- if torch was imported after the engine was loaded, the "
                               "process holds two HIP runtimes: import torch before the first Trainer is created" % (self.device, e)) from e
        self.evals = torch.zeros(self.rows, dtype=torch.float32, device=self.device)
        self.probs = torch.zeros((self.rows, NUM_MOVES), dtype=torch.float32, device=self.device)
        torch.cuda.synchronize(self.device)  # the zeros are there before any stream of the engine touches the tensors
        self._streams = {}
        self.calls = 0
        self.rows_asked = 0  # the sum of cap_rows: the rows the model has evaluated
        trainer.set_net_fn(self._fn, self.states.data_ptr(), self.evals.data_ptr(), self.probs.data_ptr(), self.rows,
                           slot=slot, flop_per_row=flop_per_row)

    def _fn(self, row0, cap_rows, d_rows_ptr, stream_ptr):
        stream = self._streams.get(stream_ptr)
        if stream is None:
            stream = self._streams[stream_ptr] = torch.cuda.ExternalStream(stream_ptr, device=self.device)
        self.calls += 1
        self.rows_asked += cap_rows
        with torch.cuda.stream(stream), torch.inference_mode():
            value, probabilities = self.model(self.states[row0:row0 + cap_rows])
            self.evals[row0:row0 + cap_rows].copy_(value.reshape(-1))
            self.probs[row0:row0 + cap_rows].copy_(probabilities)
