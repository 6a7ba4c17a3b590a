// nn_layout.h -- the flat float32 weight layouts of the two networks, by name: where every kernel, bias and BatchNorm
// constant lies in the array that set_net, the fitters and the checkpoints pass around (nn.h states both layouts in
// words and asserts their totals against these).  Whoever reads weights reads them through these offsets: the inference
// constructors, the fitters, the emulation build's network.  Plain C++17 without an include: any host compiler takes it.
#pragma once

/* mlp12x100 (Keras get_weights() order of wrapper.py:256-271): layer l has kernel[in_dim(l)][100], then bias, gamma,
 * beta, moving mean, moving variance, 100 floats each; then the value head's kernel[100][1] and bias, the policy head's
 * kernel[100][96] and bias */
struct MlpLayout {
  static constexpr int IN = 70, W = 100, LAYERS = 12, MOVES = 96;
  constexpr int in_dim(int l) const { return l == 0 ? IN : W; }
  constexpr int kernel(int l) const { return l == 0 ? 0 : (IN + 5) * W + (l - 1) * (W + 5) * W; }
  constexpr int bias(int l) const { return kernel(l) + in_dim(l) * W; }
  constexpr int gamma(int l) const { return bias(l) + W; }
  constexpr int beta(int l) const { return bias(l) + 2 * W; }
  constexpr int mean(int l) const { return bias(l) + 3 * W; }
  constexpr int var(int l) const { return bias(l) + 4 * W; }
  int kv = kernel(LAYERS), bv = kv + W, kp = bv + 1, bp = kp + W * MOVES, nw = bp + MOVES;
  /* algorithmic flop per row: the twelve layers and the two heads */
  constexpr double flop_per_row() const { return 2.0 * (IN * W + (LAYERS - 1) * W * W + W + W * MOVES); }
};

/* rescnn4 (nets._rescnn4_shapes): convolution l = 0 (stem) .. 8 has its kernel[3][3][cin(l)][64] at kernel(l), the
 * heads' 1x1 convolutions theirs at p_k ([64][4]) and v_k ([64][2]); each is followed by its BatchNorm's (j = l, 9 policy,
 * 10 value) bias, gamma, beta, moving mean and moving variance, channels(j) floats each.  Then the head's dense kernels
 * and biases: policy [64][96]; value [32][64] and [64][1]. */
struct ResCnnLayout {
  static constexpr int CIN = 10, C = 64, CONVS = 9, NBN = 11, MOVES = 96;
  static constexpr int cin(int l) { return l == 0 ? CIN : C; }
  static constexpr int channels(int j) { return j < CONVS ? C : j == 9 ? 4 : 2; }
  constexpr int kernel(int l) const { return l == 0 ? 0 : (9 * CIN + 5) * C + (l - 1) * (9 * C + 5) * C; }
  int p_k = kernel(CONVS), p_dk = p_k + (C + 5) * 4, p_db = p_dk + 64 * MOVES;
  int v_k = p_db + MOVES, v_d1k = v_k + (C + 5) * 2, v_d1b = v_d1k + 32 * 64, v_d2k = v_d1b + 64, v_d2b = v_d2k + 64, nw = v_d2b + 1;
  constexpr int bias(int j) const { return j < CONVS ? kernel(j) + 9 * cin(j) * C : (j == 9 ? p_k : v_k) + C * channels(j); }
  constexpr int gamma(int j) const { return bias(j) + channels(j); }
  constexpr int beta(int j) const { return bias(j) + 2 * channels(j); }
  constexpr int mean(int j) const { return bias(j) + 3 * channels(j); }
  constexpr int var(int j) const { return bias(j) + 4 * channels(j); }
  /* algorithmic flop per row: the 3x3 convolutions on 16 pixels (zero padding counted), the 1x1 heads, the dense layers */
  constexpr double flop_per_row() const {
    return 2.0 * 16 * 9 * (CIN * C + (CONVS - 1) * C * C) + 2.0 * 16 * C * 6 + 2.0 * 64 * MOVES + 2.0 * 32 * 64 + 2.0 * 64;
  }
};
