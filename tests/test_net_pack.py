"""The flat weight layouts (csrc/nn_layout.h) and the weight fragments the host packs for the split-precision kernels
(csrc/nn_split.h: one packer of one K step in the A-operand order of v_mfma_f32_32x32x16, and the networks' buffers built
from it), through tests/cxx/net_pack_driver.cpp: a program of its own, built with g++ -DCO_EMU and AddressSanitizer +
UBSan and run directly.  The fragment order is restated here from its definition:

    lane 32 h + i holds output o = 32 tile + i;  k-slot (h, j) <-> k = 32 T + 8 (2 a + j / 4) + 4 h + j % 4,  step = 2 T + a;
    word j / 2, half j & 1;  [tile][term][lane][4 words]."""
import os
import subprocess

import numpy as np
import pytest

from corintho_ai_amd import nets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("net_pack") / "net_pack_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DCO_EMU", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "cxx", "net_pack_driver.cpp")])
    return exe


def _run(exe, args, data=b""):
    return subprocess.run([exe] + [str(a) for a in args], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def _words(exe, args, floats):
    r = _run(exe, args, np.ascontiguousarray(floats, np.float32).tobytes())
    assert r.returncode == 0, r.stderr.decode()
    return np.frombuffer(r.stdout, np.uint32)


def _terms(v, nt, f16):
    """v (float32 array) -> [nt] uint16 arrays: the value rounded to nearest even, then the same of the float32 remainder"""
    out = []
    v = v.astype(np.float32)
    for _ in range(nt):
        if f16:
            h = v.astype(np.float16)
            out.append(h.view(np.uint16))
            back = h.astype(np.float32)
        else:  # bfloat16 = the upper half of the float32, rounded to nearest even (finite values far from overflow here)
            u = v.view(np.uint32).astype(np.uint64)
            t = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
            out.append(t)
            back = (t.astype(np.uint32) << 16).view(np.float32)
        v = v - back
    return out


def _slot_k(st, h, j):
    return 32 * (st >> 1) + 8 * (2 * (st & 1) + j // 4) + 4 * h + j % 4


# ---------------------------------------------------------------- layouts
def _mlp_shapes():
    sh = []
    for l in range(12):
        sh += [("kernel%d" % l, (70 if l == 0 else 100, 100))] + [("%s%d" % (n, l), (100,)) for n in ("bias", "gamma", "beta", "mean", "var")]
    return sh + [("kv", (100, 1)), ("bv", (1,)), ("kp", (100, 96)), ("bp", (96,))]


def test_layout_offsets_are_the_running_sums_of_the_shapes(driver):
    r = _run(driver, ["layouts"])
    assert r.returncode == 0, r.stderr.decode()
    got = {"mlp": [], "rescnn": []}
    for line in r.stdout.decode().split("\n"):
        if line:
            net, name, off = line.split()
            got[net].append((name, int(off)))
    for net, shapes, total in (("mlp", _mlp_shapes(), nets.MLP_NUM_WEIGHTS), ("rescnn", nets._rescnn4_shapes(), nets.RESCNN4_NUM_WEIGHTS)):
        sums = np.concatenate([[0], np.cumsum([int(np.prod(s)) for _, s in shapes])])
        assert len(got[net]) == len(shapes) + 1, net
        for (name, off), (want_name, _), want in zip(got[net], shapes + [("nw", ())], sums):
            assert off == want, "%s: %s (%s) at %d, the shapes put it at %d" % (net, name, want_name, off, want)
        assert got[net][-1] == ("nw", total)


# ---------------------------------------------------------------- one K step
@pytest.mark.parametrize("tiles,nt,f16", [(t, nt, f) for t in (1, 2, 4) for nt, f in ((2, False), (3, False), (2, True))])
def test_one_step_is_the_fragment_order(driver, tiles, nt, f16):
    # all-distinct weights with full significands, inside fp16's range: W[k][o] = (128 k + o + 1) * 0.0123456789
    W = (np.arange(1, 128 * 128 + 1, dtype=np.float32) * np.float32(0.0123456789)).reshape(128, 128)
    assert np.unique(W).size == W.size
    for st in (0, 1, 4, 7):
        got = _words(driver, ["step", tiles, nt, int(f16), st], W).reshape(tiles, nt, 64, 4)
        want = np.zeros((tiles, nt, 64, 4), np.uint32)
        for to in range(tiles):
            for h in range(2):
                for j in range(8):
                    t = _terms(W[_slot_k(st, h, j), 32 * to:32 * to + 32], nt, f16)
                    for i in range(nt):
                        want[to, i, 32 * h:32 * h + 32, j // 2] |= t[i].astype(np.uint32) << (16 * (j & 1))
        assert (got != 0xDEADBEEF).all(), "every word of the step is written"
        assert np.array_equal(got, want), "step %d" % st


# ---------------------------------------------------------------- the whole rescnn4 trunk
def _decode_trunk(words, nt):
    """fragments -> K[conv][tap][ci 0..63][co] per term, float64 (bf16 terms)"""
    out, off = [], 0
    for cv in range(9):
        cs = 1 if cv == 0 else 4
        n = 9 * cs * 2 * nt * 256
        f = words[off:off + n].reshape(9, cs, 2, nt, 2, 32, 4)  # tap, step, tile, term, h, i, word
        off += n
        K = np.zeros((nt, 9, 64, 64))
        for st in range(cs):
            for h in range(2):
                for j in range(8):
                    half = (f[:, st, :, :, h, :, j // 2] >> (16 * (j & 1))) & 0xFFFF  # tap, tile, term, i
                    val = (half.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
                    K[:, :, _slot_k(st, h, j), :] = val.transpose(2, 0, 1, 3).reshape(nt, 9, 64)
        out.append(K)
    assert off == words.size
    return out


@pytest.mark.parametrize("nt", [2, 3])
def test_trunk_fragments_decode_to_the_weights(driver, nt):
    w = nets.init_rescnn4(0, bn_noise=True)
    K = _decode_trunk(_words(driver, ["trunk", nt, 0], w), nt)
    ref = nets.rescnn4_unpack(w)
    names = ["stem_k"] + ["b%d_c%d_k" % (b, c) for b in range(4) for c in (1, 2)]
    worst = 0.0
    for cv, name in enumerate(names):
        k = ref[name].astype(np.float64)  # [3][3][cin][64]
        cin = k.shape[2]
        k = k.reshape(9, cin, 64)
        assert (K[cv][:, :, cin:, :] == 0).all(), "channels beyond cin are zero in every term"
        total = K[cv].sum(axis=0)[:, :cin, :]  # exact in float64
        if nt == 3:  # three bf16 terms are the float32 value
            assert np.array_equal(total, k), name
        else:  # two bf16 terms keep 16 significand bits
            err = np.abs(total - k)
            assert (err <= np.abs(k) * 2.0 ** -16).all(), name
            worst = max(worst, float((err / np.maximum(np.abs(k), 1e-30)).max()))
    if nt == 2:
        print("bf16x3 trunk: largest relative remainder %.3g (bound %.3g)" % (worst, 2.0 ** -16))


def test_f16_packer_refuses_a_weight_beyond_fp16(driver):
    w = nets.init_rescnn4(0, bn_noise=True)
    assert _run(driver, ["trunk", 2, 1], w.tobytes()).returncode == 0
    w[1234] = 65520.0  # rounds to fp16's infinity
    r = _run(driver, ["trunk", 2, 1], w.tobytes())
    assert r.returncode == 3
    assert r.stderr.decode().strip() == ("rescnn4h3: a convolution weight is 65520.000000, beyond the fp16 range of the f16x3 kernels: "
                                         "use rescnn4x6")
    m = nets.init_mlp12x100(0)
    m[7] = 65520.0  # layer 0's kernel: no BatchNorm is folded into it
    r = _run(driver, ["mlp", 2, 1], m.tobytes())
    assert r.returncode == 3
    assert r.stderr.decode().strip() == ("mlp12x100h3: a weight of layer 0 is 65520.000000 after the BatchNorm fold, beyond the fp16 range "
                                         "of the f16x3 kernels: use mlp12x100x6")
