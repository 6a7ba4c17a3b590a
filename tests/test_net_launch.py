"""Every network kernel path under the launch conditions of the fused run (csrc/pools.h Pools::launch), which no other test
of the kernels' bits reproduces: a capacity above the device's row count, rows read through in_idx, and -- the evaluation
cache's launch -- outputs written through out_idx into one array of 100 floats per element (value at float 0, priors at
floats 4..99).  Launches go through ca_net_forward_device_io (Net.forward_device with its keyword arguments).

Per kind and weight set there is one baseline E, P: the plain launch of all N rows (count = capacity = N, no indices).
test_baseline_* anchors it -- bitwise to Trainer.net_forward, and on 512 of its rows to the float64 restatement of the
network (tests/ref_nets.py) within the bounds of tests/test_net_precision.py; for the bf16x3 throughput kernel
co_k_rescnn_forward_x3 (more than 4096 rows) that is the only float64 check there is.  Every other test asserts bits of
E, P and the sentinel -7.0 in every float no row of the launch owns.

Boundaries (from the code): the MLP kernels' workgroup takes 128 rows (nn_mlp.hip, nn_mlp_split.hip); rescnn4 fp32 16
(nn_rescnn.hip RC_POS_PER_WG); rescnn4 x6 8 on the thin path up to 2048 rows, 16 above; x3 16 up to 4096 rows, 32 above;
f16x3 thin up to 2048, 16 up to 4096, above that the pixel-major kernel, and for a launch that is `alone` the batch is
split at whole passes of PASS = 32 x CU count rows (nn_rescnn_split.h rcp_small_begin).  The host computes the grids of
all of these from the CAPACITY (nn_rescnn.hip ResCnnSplitNet::forward), the device picks the path from the COUNT.

Every index handed to a kernel names memory inside this module's buffers: entries at or beyond the count name one fixed
trap row / trap element, which the assertions then find untouched.

The emulation build has the fp32 MLP only (tests/emu/nn_emu.cpp): its leg checks the entry point and the assertions
themselves (a network that ignores out_idx, drops eval_stride or writes to its workgroup's end fails cases C, C and A).
"""
import numpy as np
import pytest
import torch  # noqa: F401 -- before the engine is loaded: one HIP runtime per process (tests/test_ext_net.py)

from corintho_ai_amd import (NET_MLP12X100, NET_MLP12X100_H3, NET_MLP12X100_X3, NET_MLP12X100_X6, NET_RESCNN4, NET_RESCNN4_H3,
                             NET_RESCNN4_X3, NET_RESCNN4_X6, _lib, nets)
from corintho_ai_amd.net import Net
from tests import ref_nets
from tests.engines import cdll, make_trainer
from tests.test_ext_net import Buffers
from tests.test_net_precision import _states

SENTINEL = -7.0
VAL = 100  # floats per element of the evaluation cache's value array (engine_defs.h CO_CACHE_VAL_FLOATS)
MLP_KINDS = (NET_MLP12X100, NET_MLP12X100_X3, NET_MLP12X100_X6, NET_MLP12X100_H3)
NAMES = {NET_MLP12X100: "mlp12x100", NET_RESCNN4: "rescnn4", NET_RESCNN4_X3: "rescnn4-x3", NET_MLP12X100_X3: "mlp12x100-x3",
         NET_RESCNN4_X6: "rescnn4-x6", NET_MLP12X100_X6: "mlp12x100-x6", NET_RESCNN4_H3: "rescnn4-f16x3", NET_MLP12X100_H3: "mlp12x100-f16x3"}
WEIGHTS = {"mlp": {"bn-noise": lambda: nets.init_mlp12x100(7, bn_noise=True), "trained-like": lambda: nets.trained_like_mlp12x100(0)},
           "cnn": {"bn-noise": lambda: nets.init_rescnn4(3, bn_noise=True), "trained-like": lambda: nets.trained_like_rescnn4(0)}}
WSETS = ("bn-noise", "trained-like")


def _rows(x, PASS):
    """a row number: an int, or (passes, rows) = passes * PASS + rows"""
    return x if isinstance(x, int) else x[0] * PASS + x[1]


# per kind: rows of the baseline, capacities of case A (every branch of the host's grid arithmetic), path and tile boundaries,
# and the launches of cases B and C as (count, capacity, alone): one count per path, none a multiple of its path's tile
def _shape(kind):
    if kind in MLP_KINDS:
        return dict(n=640, caps=[1, 128, 129, 300], bounds=[128, 256], io=[(200, 300, 1)])
    if kind == NET_RESCNN4:
        return dict(n=560, caps=[1, 16, 17, 100], bounds=[16, 32, 96], io=[(50, 100, 1)])
    if kind == NET_RESCNN4_X6:
        return dict(n=4200, caps=[2048, 2049, 4100], bounds=[8, 16, 2040, 2048, 2064, 4096], io=[(1003, 2500, 1), (3000, 4100, 1)])
    if kind == NET_RESCNN4_X3:
        return dict(n=8300, caps=[4096, 4097, 8200], bounds=[16, 32, 4080, 4096, 4128, 8192], io=[(3000, 4500, 1), (5000, 8200, 1)])
    assert kind == NET_RESCNN4_H3
    return dict(n=(2, 4096), caps=[2048, 4096, 4097, (1, 4096), (2, 100)],
                bounds=[8, 16, 2040, 2048, 2064, 4096, 4128, (1, 0), (1, 8), (1, 16), (1, 2048), (1, 2064), (1, 4096), (2, 0)],
                # thin / 16-row / pixel-major unsplit (not alone) / split batches: a thin and a 16-row remainder behind one
                # pass, both kernels at work in ONE launch / more than 4096 rows behind a pass: the pixel-major kernel alone
                io=[(1500, 5000, 1), (3000, 5000, 0), (5000, 6000, 0), ((1, 1500), (1, 4000), 1), ((1, 3000), (1, 4090), 1),
                    ((1, 5000), (1, 6000), 1)])


def _label(x):
    return str(x) if isinstance(x, int) else "%dPASS+%d" % x


def _cases(per_kind):
    """(engine, kind, wset, *extra) for every kind on the device and the fp32 MLP on the emulation build too"""
    out = []
    for kind in (1, 2, 3, 4, 5, 6, 8, 9):
        for engine in (["emu"] if kind == NET_MLP12X100 else []) + ["hip"]:
            for wset in WSETS:
                for extra, label in per_kind(kind):
                    out.append(pytest.param(engine, kind, wset, *extra, id="-".join([engine, NAMES[kind], wset] + label),
                                            marks=[pytest.mark.gpu] if engine == "hip" else []))
    return out


def _bits(a):
    return a.view(np.int32) if isinstance(a, np.ndarray) else a.view(torch.int32)


def same(a, b):
    return bool((_bits(a) == _bits(b)).all())


def untouched(a):
    return bool((a == SENTINEL).all())


class World:
    """one kind with one weight set: the Net, N input rows, the baseline and the buffers every case launches into"""

    def __init__(self, engine, kind, wset, trainer):
        self.engine, self.kind = engine, kind
        self.PASS = 32 * torch.cuda.get_device_properties(0).multi_processor_count if engine == "hip" else 8192
        self.shape = _shape(kind)
        self.n = n = _rows(self.shape["n"], self.PASS)
        self.weights = WEIGHTS["mlp" if kind in MLP_KINDS else "cnn"][wset]()
        self.net = Net(kind, self.weights, n, _cdll=cdll(engine))
        self.states = _states(n, 100 + kind, reserves=8)
        self.b = Buffers(engine, n)
        self.b.fill(states=self.states)
        self.val = self.dev(np.zeros((n + 50, VAL), np.float32))
        self.in_idx = self.dev(np.zeros(n, np.int32))
        self.out_idx = self.dev(np.zeros(n, np.int32))
        self.reset()
        self.launch(n, n)
        self.E, self.P = self.dev(self.b.host("evals")), self.dev(self.b.host("probs"))
        # the same rows through the trainer's own launch, in chunks it accepts
        trainer.set_net(kind, self.weights)
        chunk = trainer.request_rows()
        self.trainer_E = np.concatenate([trainer.net_forward(self.states[i:i + chunk])[0] for i in range(0, n, chunk)])
        self.trainer_P = np.concatenate([trainer.net_forward(self.states[i:i + chunk])[1] for i in range(0, n, chunk)])

    def dev(self, a):
        return a.copy() if self.engine == "emu" else torch.from_numpy(a).cuda()

    def index(self, a, idx):
        """rows idx (a host array) of a"""
        return a[idx] if self.engine == "emu" else a[torch.from_numpy(idx.astype(np.int64)).cuda()]

    def reset(self):
        self.b.evals[...] = SENTINEL
        self.b.probs[...] = SENTINEL
        self.val[...] = SENTINEL

    def launch(self, cap, count, alone=1, in_idx=None, out_idx=None, cache=False):
        """cap rows of capacity, count on the device; cache: into val as the evaluation cache's launch does"""
        ptr = (lambda a: a.ctypes.data) if self.engine == "emu" else (lambda a: a.data_ptr())
        for dst, src in ((self.in_idx, in_idx), (self.out_idx, out_idx)):
            if src is not None:
                dst[:len(src)] = self.dev(np.asarray(src, np.int32))
        self.b.count[0] = count
        if self.engine == "hip":
            torch.cuda.synchronize()  # (the launch is on the net's own stream, synchronised before the call returns)
        ev, pr, stride = (ptr(self.val), ptr(self.val) + 16, (VAL, VAL)) if cache else (self.b.ptrs[1], self.b.ptrs[2], (1, 96))
        self.net.forward_device(self.b.ptrs[0], cap, self.b.count_ptr, ev, pr, in_idx=0 if in_idx is None else ptr(self.in_idx),
                                out_idx=0 if out_idx is None else ptr(self.out_idx), eval_stride=stride[0], probs_stride=stride[1],
                                alone=alone, state_rows=self.n)


@pytest.fixture(scope="module")
def world():
    made, trainers = {}, {}

    def get(engine, kind, wset):
        if engine not in trainers:
            trainers[engine] = make_trainer(engine, 512 if engine == "hip" else 64, "", 1, 50, 16, 1.0, 0.25, 0, 1, False)
        if (engine, kind, wset) not in made:
            made[engine, kind, wset] = World(engine, kind, wset, trainers[engine])
        return made[engine, kind, wset]

    yield get
    for w in made.values():
        w.net.close()
    for t in trainers.values():
        t.close()


@pytest.mark.parametrize("engine,kind,wset", _cases(lambda kind: [((), [])]))
def test_baseline_is_the_trainers_and_float64(world, engine, kind, wset):
    """the baseline of every other test here: (1) bitwise Trainer.net_forward's on the same rows; (2) on 512 rows spread over
    the batch, its last 40 among them, within the project's bounds of the float64 restatement -- 1e-5 for the fp32, bf16x6
    and f16x3 kinds, 1e-4 for bf16x3 -- and priors that sum to 1 within 1e-5"""
    w = world(engine, kind, wset)
    E, P = (w.E, w.P) if engine == "emu" else (w.E.cpu().numpy(), w.P.cpu().numpy())
    assert E.tobytes() == w.trainer_E.tobytes() and P.tobytes() == w.trainer_P.tobytes()
    n = w.n
    pick = np.unique(np.concatenate([np.linspace(0, n - 41, 472).astype(np.int64), np.arange(n - 40, n)]))
    assert len(pick) == 512 and pick[-1] == n - 1
    f64 = ref_nets.mlp12x100_forward_f64 if kind in MLP_KINDS else ref_nets.rescnn4_forward_f64
    ev, pr = f64(w.weights, w.states[pick])
    err_e = float(np.max(np.abs(E[pick].astype(np.float64) - np.asarray(ev, np.float64))))
    err_p = float(np.max(np.abs(P[pick].astype(np.float64) - np.asarray(pr, np.float64))))
    err_s = float(np.max(np.abs(P[pick].astype(np.float64).sum(axis=1) - 1.0)))
    print("%s %s %-12s N %5d  max |err| vs float64 on 512 rows: value %.3e  priors %.3e  |sum of priors - 1| %.3e"
          % (engine, NAMES[kind], wset, n, err_e, err_p, err_s))
    bound = 1e-4 if kind in (NET_RESCNN4_X3, NET_MLP12X100_X3) else 1e-5
    assert err_e < bound and err_p < bound, (err_e, err_p, bound)
    assert err_s < 1e-5, err_s


def _caps(kind):
    alones = (1, 0) if kind == NET_RESCNN4_H3 else (1,)
    return [((cap, alone), ["cap" + _label(cap)] + (["alone%d" % alone] if len(alones) > 1 else []))
            for cap in _shape(kind)["caps"] for alone in alones]


@pytest.mark.parametrize("engine,kind,wset,cap,alone", _cases(_caps))
def test_count_below_capacity(world, engine, kind, wset, cap, alone):
    """A. a grid sized for `cap` rows, a device count of 0, 1, cap and every path and tile boundary b <= cap as b - 1, b,
    b + 1: the rows below the count are the baseline's bits, every float from the count on keeps the sentinel"""
    w = world(engine, kind, wset)
    cap = _rows(cap, w.PASS)
    counts = {0, 1, cap}
    for b in w.shape["bounds"]:
        counts.update(c for c in (_rows(b, w.PASS) + d for d in (-1, 0, 1)) if 0 <= c <= cap)
    for count in sorted(counts):
        w.reset()
        w.launch(cap, count, alone)
        where = "capacity %d, count %d, alone %d" % (cap, count, alone)
        assert same(w.b.evals[:count], w.E[:count]) and same(w.b.probs[:count], w.P[:count]), "rows below the count: " + where
        assert untouched(w.b.evals[count:]) and untouched(w.b.probs[count:]), "rows beyond the count were written: " + where


def _io(kind):
    return [(c, ["count" + _label(c[0]), "cap" + _label(c[1]), "alone%d" % c[2]]) for c in _shape(kind)["io"]]


def _indices(w, count, cap, seed):
    """cap entries each: a selection without repeats from the N input rows and from val's elements; the entries from the
    count on name ONE row and ONE element outside the selections"""
    rng = np.random.default_rng(seed)
    rows, elems = rng.permutation(w.n), rng.permutation(w.n + 50)
    in_idx, out_idx = rows[:cap].copy(), elems[:cap].copy()
    trap_row, trap_elem = int(rows[cap]), int(elems[cap])
    in_idx[count:], out_idx[count:] = trap_row, trap_elem
    return in_idx, out_idx, trap_elem


@pytest.mark.parametrize("engine,kind,wset,count,cap,alone", _cases(_io))
def test_rows_through_in_idx(world, engine, kind, wset, count, cap, alone):
    """B. the fused launch without a cache: output row r < count is the baseline of input row in_idx[r], bit for bit;
    nothing from the count on is written (the entries there name the trap row)"""
    w = world(engine, kind, wset)
    count, cap = _rows(count, w.PASS), _rows(cap, w.PASS)
    assert count < cap < w.n
    in_idx, _, _ = _indices(w, count, cap, 17)
    w.reset()
    w.launch(cap, count, alone, in_idx=in_idx)
    assert same(w.b.evals[:count], w.index(w.E, in_idx[:count])), "values"
    assert same(w.b.probs[:count], w.index(w.P, in_idx[:count])), "priors"
    assert untouched(w.b.evals[count:]) and untouched(w.b.probs[count:]), "rows beyond the count were written"


@pytest.mark.parametrize("engine,kind,wset,count,cap,alone", _cases(_io))
def test_the_cache_launch(world, engine, kind, wset, count, cap, alone):
    """C. in_idx and out_idx, both strides 100, d_evals = val, d_probs = val + 4: element out_idx[r] holds the value of input
    row in_idx[r] at float 0 and its priors at floats 4..99; floats 1..3, every element not named and the trap element keep
    the sentinel.  (rescnn4 f16x3, count above PASS, alone: the pixel-major kernel and the small-batch kernel both write
    through out_idx in this one launch.)"""
    w = world(engine, kind, wset)
    count, cap = _rows(count, w.PASS), _rows(cap, w.PASS)
    in_idx, out_idx, trap_elem = _indices(w, count, cap, 23)
    w.reset()
    w.launch(cap, count, alone, in_idx=in_idx, out_idx=out_idx, cache=True)
    got = w.index(w.val, out_idx[:count])
    assert same(got[:, 0], w.index(w.E, in_idx[:count])), "values at float 0"
    assert same(got[:, 4:], w.index(w.P, in_idx[:count])), "priors at floats 4..99"
    assert untouched(got[:, 1:4]), "floats 1..3 of a written element"
    assert untouched(w.val[trap_elem]), "the trap element was written"
    rest = np.setdiff1d(np.arange(w.n + 50), out_idx[:count])
    assert untouched(w.index(w.val, rest)), "an element no row names was written"
    assert untouched(w.b.evals) and untouched(w.b.probs)


@pytest.mark.parametrize("engine", [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)])
def test_arguments_the_entry_refuses(world, engine):
    """CA_ERR_ARG, and nothing launched: rows beyond max_rows, strides below 1 / 96, a null buffer, fewer state rows than
    the launch reads in place"""
    w = world(engine, NET_MLP12X100 if engine == "emu" else NET_MLP12X100_H3, "bn-noise")
    s, e, p = w.b.ptrs
    w.reset()
    for kw, args in ((dict(state_rows=w.n + 1), (s, 10, w.b.count_ptr, e, p)), (dict(state_rows=w.n), (s, w.n + 1, w.b.count_ptr, e, p)),
                     (dict(state_rows=w.n, eval_stride=0), (s, 10, w.b.count_ptr, e, p)),
                     (dict(state_rows=w.n, probs_stride=95), (s, 10, w.b.count_ptr, e, p)),
                     (dict(state_rows=9), (s, 10, w.b.count_ptr, e, p)), (dict(state_rows=w.n), (0, 10, w.b.count_ptr, e, p)),
                     (dict(state_rows=w.n), (s, 10, 0, e, p)), (dict(state_rows=w.n), (s, 10, w.b.count_ptr, 0, p)),
                     (dict(state_rows=w.n), (s, 10, w.b.count_ptr, e, 0))):
        with pytest.raises(_lib.EngineError, match="error -1"):
            w.net.forward_device(*args, **kw)
    assert untouched(w.b.evals) and untouched(w.b.probs)
