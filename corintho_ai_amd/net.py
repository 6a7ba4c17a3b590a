"""One of the library's own networks on device memory, without a trainer (ca_net_*): what a caller-supplied network
function (Trainer.set_net_fn) calls to run the library's kernels on the rows it is handed.

    net = Net(NET_RESCNN4_H3, weights, max_rows)
    net.forward_device(ptr_states, rows_cap, ptr_rows, ptr_evals, ptr_probs, stream)

All pointers are device addresses as integers: states [rows_cap][70], a device int32 row count, evals [rows_cap],
probs [rows_cap][96].  stream: a HIP stream handle; 0 = the net's own stream, synchronised before the call returns.
"""
import ctypes as C

import numpy as np

from . import _lib


class Net:
    def __init__(self, kind, weights, max_rows, device=0, _cdll=None):
        self._L = _cdll if _cdll is not None else _lib.load()
        self._n = C.c_void_p()
        w = np.ascontiguousarray(weights, dtype=np.float32)
        self.max_rows = int(max_rows)
        _lib.check(self._L, self._L.ca_net_create(device, kind, w.ctypes.data_as(_lib.f32p), w.size, self.max_rows, C.byref(self._n)))

    def forward_device(self, ptr_states, rows_cap, ptr_rows, ptr_evals, ptr_probs, stream=0):
        _lib.check(self._L, self._L.ca_net_forward_device(self._n, C.c_void_p(ptr_states), int(rows_cap), C.c_void_p(ptr_rows),
                                                          C.c_void_p(ptr_evals), C.c_void_p(ptr_probs), C.c_void_p(stream or None)))

    def close(self):
        if getattr(self, "_n", None) and self._n.value:
            self._L.ca_net_destroy(self._n)
            self._n = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
