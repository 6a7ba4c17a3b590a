"""rescnn4's gradients above 2048 rows, where two launch plans of csrc/nn_train_conv.hip change, against the float64
restatement (tests/fit_ref_rescnn4.py) by the rule of tests/test_fit_rescnn4_gpu.py; and one batch of that size through
mlp12x100, whose kernels have no such threshold.

With B positions a BatchNorm reduces R = 16 B rows, and (FC_BN_CHUNKS = 256, FC_WG_CHUNKS = 128)

    fc_bn_rpc(R)    = 128 ceil(R / (128 * 256))        rows per BatchNorm chunk, ceil(R / rpc) chunks
    fc_conv3_wgrad  ppc = ceil(B / 128); ppc < 16 ? 16 : 4 ceil(ppc / 4)    positions per chunk, ceil(B / ppc) chunks,
                    each walked four positions (pb += 4) at a time

so up to B = 2048 a BatchNorm chunk has 128 rows and a weight-gradient chunk 16 positions.  Above it:

    B     ceil(B/128)  ppc  chunks                       R       rpc  BatchNorm chunks
    2049  17           20   103, the last of 9 (4+4+1)   32 784  256  129, the last of 16 rows
    2560  20           20   128, all full                40 960  256  160, all full
    4097  33           36   114, the last of 29 (7x4+1)  65 552  384  171, the last of 272 rows

A row group of fc_k_bn_part / fc_k_bnb_part (256 / C groups; C = 64, 4, 2) walks rpc C / 256 rows of a full chunk:
32, 2 and 1 at rpc = 128, twice that at 256, three times at 384.  A change of those constants or formulas asks for new
sizes here."""
import numpy as np
import pytest

from corintho_ai_amd import NET_RESCNN4, nets
from corintho_ai_amd.fit import Fitter
from tests import fit_ref
from tests import fit_ref_step as S
from tests.fit_ref_step import within as _within
from tests.test_fit_gpu import _tensors
from tests.test_fit_rescnn4_gpu import KINK, R, _check_gradient

pytestmark = pytest.mark.gpu

BATCHES = (2049, 2560, 4097)
# One number seeds the weights (nets.init_rescnn4) and the draw of the three batches' rows, in the order of BATCHES.
# Tried from 7 upwards for the first whose three batches keep every ReLU input of the float64 restatement at least
# KINK from its kink: 7 holds at once (margins 4.018e-06, 1.054e-04, 1.204e-05), so no other was tried.
SEED = 7


def _plan(B):
    """(positions per weight-gradient chunk, its chunks, the last one's positions, BatchNorm rows per chunk, its
    chunks, the last one's rows) as fc_conv3_wgrad and fc_bn_rpc lay them out"""
    ppc = -(-B // 128)
    ppc = 16 if ppc < 16 else -(-ppc // 4) * 4
    wg = -(-B // ppc)
    rows = 16 * B
    rpc = 128 * -(-rows // (128 * 256))
    bn = -(-rows // rpc)
    return ppc, wg, B - (wg - 1) * ppc, rpc, bn, rows - (bn - 1) * rpc


def test_the_sizes_are_the_ones_the_launch_plans_turn_at():
    assert _plan(2048) == (16, 128, 16, 128, 256, 128)
    assert _plan(2049) == (20, 103, 9, 256, 129, 16)
    assert _plan(2560) == (20, 128, 20, 256, 160, 256)
    assert _plan(4097) == (36, 114, 29, 384, 171, 272)


@pytest.fixture(scope="module")
def large():
    data = R.synthetic_samples(8192, 11)
    off = R.offsets()
    w = nets.init_rescnn4(SEED, bn_noise=True)
    for pre in R.BN_PREFIXES:
        w[R._slice(off, pre + "_bn1")] += np.float32(12.0)
    rng = np.random.default_rng(SEED)
    rows = {B: rng.choice(8192, B, replace=False).astype(np.int32) for B in BATCHES}
    with Fitter(max_batch=4112, net=NET_RESCNN4) as f:
        f.set_data(*data)
        f.set_weights(w)
        yield f, w, data, rows


@pytest.mark.parametrize("B", BATCHES)
def test_gradients_above_2048_rows_without_a_kink(large, B):
    """strictly, as test_gradients_at_scale_without_a_kink: with 12 added to every beta each BatchNorm-fed ReLU is
    active, and no ReLU input of these batches lies within 2e-7 of its kink"""
    f, w, data, rows = large
    margin = S.kink_margin(R, w, data[0][rows[B]])
    print("seed %d B=%d margin %.3e plan %s" % (SEED, B, margin, _plan(B)))
    assert margin >= KINK, (SEED, B, margin)
    bad = []
    _check_gradient(f, w, data, rows[B], "seed %d B=%d" % (SEED, B), False, bad)
    assert not bad, "device error above 4 x float32's: %s" % bad[:12]


def test_gradients_of_4097_rows_repeat_bit_for_bit(large):
    f, _, _, rows = large
    g1, l1 = f.gradients(rows[4097])
    g2, l2 = f.gradients(rows[4097])
    assert g1.tobytes() == g2.tobytes() and np.asarray(l1).tobytes() == np.asarray(l2).tobytes()
    assert np.any(g1) and np.all(np.isfinite(g1))


def test_mlp_gradients_of_4097_rows():
    """the rule of tests/test_fit_gpu.py's test_gradients_of_one_batch at a batch twice its largest.  This network's
    ReLUs stand in front of their BatchNorms, and 4097 rows have 4.9 M pre-activations: one of them lies within 2e-7
    of its kink whatever the draw (the row seeds 3 to 19 all give margins of 1.4e-9 to 1.4e-7), so the rule's kink
    clause bounds the tensors here and only the losses are held to float32's own error."""
    data = fit_ref.synthetic_samples(8192, 11)
    w = nets.init_mlp12x100(7, bn_noise=True)
    rows = np.random.default_rng(3).choice(8192, 4097, replace=False).astype(np.int32)
    with Fitter(max_batch=4097) as f:
        f.set_data(*data)
        f.set_weights(w)
        g, losses = f.gradients(rows)
    s, z, p = (a[rows] for a in data)
    g64, l64, _ = S.loss_and_grad(fit_ref, w, s, z, p)
    g32, l32, _ = S.loss_and_grad(fit_ref, w, s, z, p, dtype=fit_ref.torch.float32)
    assert not g[fit_ref.stat_mask()].any(), "gradient at a moving statistic"
    kink = S.kink_margin(fit_ref, w, s) < 2e-7
    bad = []
    for name, sl in _tensors():
        top = float(np.max(np.abs(g64[sl])))
        ok, ed, e3 = _within(g[sl], g32[sl], g64[sl], 2e-5 * top + 1e-12)
        if kink:
            ok = ed <= 0.05 * top + 1e-12
        print("%-8s kink=%d dev %.3e f32 %.3e top %.3e%s" % (name, kink, ed, e3, top, "" if ok else "  FAIL"))
        if not ok:
            bad.append((name, kink, ed, e3, top))
    ok, ed, e3 = _within(losses, l32, l64, 1e-6 * abs(l64[0]))
    print("losses dev %.3e f32 %.3e" % (ed, e3))
    if not ok:
        bad.append(("losses", ed, e3))
    assert not bad, "device error above 4 x float32's: %s" % bad[:12]
