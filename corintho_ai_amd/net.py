"""One of the library's own networks on device memory, without a trainer (ca_net_*): what a caller-supplied network
function (Trainer.set_net_fn) calls to run the library's kernels on the rows it is handed.

    net = Net(NET_RESCNN4_H3, weights, max_rows)
    net.forward_device(ptr_states, rows_cap, ptr_rows, ptr_evals, ptr_probs, stream)

All pointers are device addresses as integers: states [rows_cap][70], a device int32 row count, evals [rows_cap],
probs [rows_cap][96].  stream: a HIP stream handle; 0 = the net's own stream, synchronised before the call returns.

The keyword arguments of forward_device shape the launch as a fused run does (ca_net_forward_device_io): in_idx / out_idx
are device int32 lists (0: rows in place) -- row r is read from states row in_idx[r], of state_rows rows, and written to
element out_idx[r] of evals (eval_stride floats per element) and probs (probs_stride); alone=False tells the kernels that
other streams keep the GPU busy.  The library cannot check the indices.
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

    def forward_device(self, ptr_states, rows_cap, ptr_rows, ptr_evals, ptr_probs, stream=0, *, in_idx=0, out_idx=0, eval_stride=1,
                       probs_stride=96, alone=True, state_rows=None):
        if not in_idx and not out_idx and (eval_stride, probs_stride) == (1, 96) and alone and state_rows is None:
            _lib.check(self._L, self._L.ca_net_forward_device(self._n, C.c_void_p(ptr_states), int(rows_cap), C.c_void_p(ptr_rows),
                                                              C.c_void_p(ptr_evals), C.c_void_p(ptr_probs), C.c_void_p(stream or None)))
            return
        _lib.check(self._L, self._L.ca_net_forward_device_io(
            self._n, C.c_void_p(ptr_states), int(rows_cap if state_rows is None else state_rows), int(rows_cap), C.c_void_p(ptr_rows),
            C.c_void_p(in_idx or None), C.c_void_p(out_idx or None), C.c_void_p(ptr_evals), int(eval_stride), C.c_void_p(ptr_probs),
            int(probs_stride), int(bool(alone)), C.c_void_p(stream or None)))

    def close(self):
        if getattr(self, "_n", None) and self._n.value:
            self._L.ca_net_destroy(self._n)
            self._n = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NetGroup:
    """Many models of one kind on one set of rows, in one launch (ca_net_group_*).

        g = NetGroup(NET_MLP12X100_H3, [weights_0, weights_1, ...], max_rows=4096)
        evals, probs = g.forward(states, model_of_row)    # states [n][70], model_of_row [n] in 0 .. len(weights) - 1

    Row r is evaluated by model model_of_row[r], to the same bits as by that model alone.  The split-precision kinds of
    mlp12x100 run one kernel whose workgroups each take the weights of their own model (`grouped_kernel`); every other
    kind runs one launch per model on the same index lists."""

    def __init__(self, kind, weights, max_rows=4096, device=0, _cdll=None):
        self._L = _cdll if _cdll is not None else _lib.load()
        self._g = C.c_void_p()
        ws = [np.ascontiguousarray(w, dtype=np.float32).ravel() for w in weights]
        if not ws or any(w.size != ws[0].size for w in ws):
            raise ValueError("NetGroup: one or more weight sets, all of one size")
        ptrs = (_lib.f32p * len(ws))(*[w.ctypes.data_as(_lib.f32p) for w in ws])
        _lib.check(self._L, self._L.ca_net_group_create(device, kind, ptrs, len(ws), ws[0].size, int(max_rows), C.byref(self._g)))
        info = (C.c_int32 * 6)()
        _lib.check(self._L, self._L.ca_net_group_info(self._g, info))
        self.models, self.max_rows, grouped, self.tile, self._idx_len, self._wg_cap = list(info)
        self.grouped_kernel = bool(grouped)

    def forward(self, states, model_of_row):
        s = np.ascontiguousarray(states, dtype=np.float32)
        m = np.ascontiguousarray(model_of_row, dtype=np.int32)
        n = s.shape[0]
        if s.ndim != 2 or s.shape[1] != 70 or m.shape != (n,):
            raise ValueError("NetGroup.forward: states [n][70] and model_of_row [n]")
        evals, probs = np.zeros(n, np.float32), np.zeros((n, 96), np.float32)
        _lib.check(self._L, self._L.ca_net_group_forward(self._g, s.ctypes.data_as(_lib.f32p), m.ctypes.data_as(_lib.i32p), n,
                                                         evals.ctypes.data_as(_lib.f32p), probs.ctypes.data_as(_lib.f32p)))
        return evals, probs

    def bench(self, states, model_of_row, reps=20):
        """diagnostic: kernel-only milliseconds per call of (the grouping kernel, the network launch) on these rows"""
        s = np.ascontiguousarray(states, dtype=np.float32)
        m = np.ascontiguousarray(model_of_row, dtype=np.int32)
        out = (C.c_float * 2)()
        _lib.check(self._L, self._L.ca_net_group_bench(self._g, s.ctypes.data_as(_lib.f32p), m.ctypes.data_as(_lib.i32p), s.shape[0],
                                                       int(reps), out))
        return out[0], out[1]

    def tables(self):
        """diagnostic: what the grouping kernel left for the last forward -- dict(idx, wg [n_wg][3] = (model, first index,
        rows), seg_start [models], seg_count [models]); model m's rows are idx[seg_start[m] : seg_start[m] + seg_count[m]]"""
        idx = np.zeros(self._idx_len, np.int32)
        wg = np.zeros((self._wg_cap, 4), np.int32)
        n_wg = C.c_int32()
        start, count = np.zeros(self.models, np.int32), np.zeros(self.models, np.int32)
        _lib.check(self._L, self._L.ca_net_group_tables(self._g, idx.ctypes.data_as(_lib.i32p), wg.ctypes.data_as(_lib.i32p), C.byref(n_wg),
                                                        start.ctypes.data_as(_lib.i32p), count.ctypes.data_as(_lib.i32p)))
        return {"idx": idx, "wg": wg[:n_wg.value, :3].copy(), "seg_start": start, "seg_count": count}

    def close(self):
        if getattr(self, "_g", None) and self._g.value:
            self._L.ca_net_group_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
