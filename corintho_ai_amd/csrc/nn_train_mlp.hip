// nn_train_mlp.hip -- mlp12x100's training step ("Network training"): the reference's Keras model
// (wrapper.py:256-282) forward and backward, in float32 on the fp32 matrix pipe through ft_k_gemm (nn_train.hip).
//
//   gather      X0 = states[rows] (rows of the epoch's permutation)                           1 launch
//   forward     per layer: Z = X W + b, ReLU -> A_l (ft_k_gemm);  BatchNorm with batch statistics
//               (mean, biased variance) -> Y_l (ft_k_bn_fwd)                                       24 launches
//   heads       logits = Y_11 Kp + bp, v = Y_11 Kv + bv (two ft_k_gemm)                          2 launches
//   backward    head kernel gradients and dY_11 (four ft_k_gemm); per layer: BatchNorm and ReLU
//               backward with dgamma, dbeta, dbias (ft_k_bn_bwd), dW = X^T dZ (ft_k_gemm, split over
//               the rows), dX = dZ W^T (ft_k_gemm)                                                39 launches
// The weights live in the Keras get_weights() layout (nn.h) and the kernels read them there with bounds checks, so
// there is no padded copy to keep in step.
#include "nn_train.h"

#define FT_IN_LD 80 /* gathered input row stride: 70 padded to 5 tiles */

static constexpr MlpLayout ML; /* the flat layout (nn_layout.h) */
static_assert(ML.IN == CA_GAME_STATE_SIZE && ML.MOVES == CA_NUM_MOVES, "MlpLayout is not the engine's state and move count");

/* X0[r][k] = states[rows[r]][k], k < 70 */
__global__ __launch_bounds__(256) void ft_k_gather(const float *__restrict__ states, const int32_t *__restrict__ rows,
                                                   int B, float *__restrict__ x0) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * CA_GAME_STATE_SIZE) return;
  const int r = e / CA_GAME_STATE_SIZE, k = e % CA_GAME_STATE_SIZE;
  x0[(long)r * FT_IN_LD + k] = states[(long)rows[r] * CA_GAME_STATE_SIZE + k];
}

/* BatchNormalization forward of one layer, A_l -> Y_l.  Block = 16 features x 64 row groups, so one block owns its
 * features over all B rows.  train: batch mean and biased variance (saved to stat[0 / 1][f]); else the moving ones. */
__global__ __launch_bounds__(1024) void ft_k_bn_fwd(const float *__restrict__ A, float *__restrict__ Y, int B,
                                                   const float *__restrict__ w, int off_gamma, int train,
                                                   float *__restrict__ stat) {
  __shared__ float red[(FT_BN_RG + 1) * 16];
  const int f = blockIdx.x * 16 + (threadIdx.x & 15), rg = threadIdx.x >> 4;
  const bool fv = f < CO_MLP_WIDTH;
  const float *a = A + f;
  float mu, var;
  if (train) {
    float s = 0.0f;
    if (fv)
      for (int r = rg; r < B; r += FT_BN_RG) s += a[(long)r * FT_PADW];
    mu = ft_colsum(red, s) / (float)B;
    float s2 = 0.0f;
    if (fv)
      for (int r = rg; r < B; r += FT_BN_RG) {
        const float d = a[(long)r * FT_PADW] - mu;
        s2 += d * d;
      }
    var = ft_colsum(red, s2) / (float)B;
    if (fv && rg == 0) {
      stat[f] = mu;
      stat[FT_PADW + f] = var;
    }
  } else {
    mu = fv ? w[off_gamma + 200 + f] : 0.0f;
    var = fv ? w[off_gamma + 300 + f] : 1.0f;
  }
  if (!fv) return;
  const float rstd = 1.0f / sqrtf(var + (float)CO_BN_EPS);
  const float ga = w[off_gamma + f], be = w[off_gamma + 100 + f];
  for (int r = rg; r < B; r += FT_BN_RG) Y[(long)r * FT_PADW + f] = ga * ((a[(long)r * FT_PADW] - mu) * rstd) + be;
}

/* BatchNormalization (batch statistics) and ReLU backward of one layer: dY -> dZ, and the layer's dgamma, dbeta and
 * dbias, written whole (one block owns its features over all rows) to the gradient partial of split 0. */
__global__ __launch_bounds__(1024) void ft_k_bn_bwd(const float *__restrict__ dY, const float *__restrict__ A,
                                                   float *__restrict__ dZ, int B, const float *__restrict__ w,
                                                   int off_bias, const float *__restrict__ stat, float *__restrict__ g) {
  __shared__ float red[(FT_BN_RG + 1) * 16];
  const int f = blockIdx.x * 16 + (threadIdx.x & 15), rg = threadIdx.x >> 4;
  const bool fv = f < CO_MLP_WIDTH;
  const float mu = fv ? stat[f] : 0.0f;
  const float rstd = 1.0f / sqrtf((fv ? stat[FT_PADW + f] : 1.0f) + (float)CO_BN_EPS);
  float sdy = 0.0f, sdyx = 0.0f;
  if (fv)
    for (int r = rg; r < B; r += FT_BN_RG) {
      const float dy = dY[(long)r * FT_PADW + f];
      sdy += dy;
      sdyx += dy * ((A[(long)r * FT_PADW + f] - mu) * rstd);
    }
  const float dbeta = ft_colsum(red, sdy);
  const float dgamma = ft_colsum(red, sdyx);
  const float ga = fv ? w[off_bias + 100 + f] : 0.0f;
  const float scale = ga * rstd, inv_b = 1.0f / (float)B;
  const float mdy = dbeta * inv_b, mdyx = dgamma * inv_b;
  float sdz = 0.0f;
  if (fv)
    for (int r = rg; r < B; r += FT_BN_RG) {
      const long e = (long)r * FT_PADW + f;
      const float a = A[e];
      const float xh = (a - mu) * rstd;
      const float dz = a > 0.0f ? scale * (dY[e] - mdy - xh * mdyx) : 0.0f;
      dZ[e] = dz;
      sdz += dz;
    }
  const float dbias = ft_colsum(red, sdz);
  if (fv && rg == 0) {
    g[off_bias + f] = dbias;
    g[off_bias + 100 + f] = dgamma;
    g[off_bias + 200 + f] = dbeta;
  }
}

/* ------------------------------------------------------------------ host */
#define FT_STAT_LD (2 * FT_PADW) /* a layer's slot in stat: the batch mean, then the batch variance, FT_PADW apart */

struct FtMlp : FtNet {
  size_t rows_ld; /* floats of one layer's activations: max_batch rounded up to whole tiles x FT_PADW */
  DevBuf<float> x0, act, y, dy, dz;

  FtMlp(int max_batch, rt_stream_t s) : rows_ld((size_t)((max_batch + 15) / 16 * 16) * FT_PADW) {
    x0.alloc(rows_ld / FT_PADW * FT_IN_LD, s);
    act.alloc(CO_MLP_LAYERS * rows_ld, s);
    y.alloc(CO_MLP_LAYERS * rows_ld, s);
    dy.alloc(rows_ld, s);
    dz.alloc(rows_ld, s);
  }
  const char *name() const override { return "mlp12x100"; }
  int num_weights() const override { return ML.nw; }
  size_t stat_floats() const override { return (size_t)CO_MLP_LAYERS * FT_STAT_LD; }
  int policy_bias() const override { return ML.bp; }
  int value_bias() const override { return ML.bv; }
  void update_table(std::vector<int32_t> &sidx) const override {
    sidx.assign(ML.nw, FT_SPLIT0); /* every kernel is a product over the B rows; FT_SPLIT1 counts the same */
    for (int l = 0; l < CO_MLP_LAYERS; ++l)
      for (int f = 0; f < CO_MLP_WIDTH; ++f) {
        sidx[ML.mean(l) + f] = l * FT_STAT_LD + f;
        sidx[ML.var(l) + f] = l * FT_STAT_LD + FT_PADW + f;
      }
  }
  void tensor_table(std::vector<FtTensor> &t) const override {
    t.clear();
    for (int l = 0; l < CO_MLP_LAYERS; ++l) {
      t.push_back({ML.kernel(l), ML.in_dim(l) * CO_MLP_WIDTH, CA_TENSOR_TRUNK_KERNEL});
      t.push_back({ML.bias(l), CO_MLP_WIDTH, CA_TENSOR_BIAS});
      t.push_back({ML.gamma(l), CO_MLP_WIDTH, CA_TENSOR_GAMMA});
      t.push_back({ML.beta(l), CO_MLP_WIDTH, CA_TENSOR_BETA});
      t.push_back({ML.mean(l), CO_MLP_WIDTH, CA_TENSOR_MOVING});
      t.push_back({ML.var(l), CO_MLP_WIDTH, CA_TENSOR_MOVING});
    }
    t.push_back({ML.kv, CO_MLP_WIDTH, CA_TENSOR_HEAD_KERNEL});
    t.push_back({ML.bv, 1, CA_TENSOR_BIAS});
    t.push_back({ML.kp, CO_MLP_WIDTH * CA_NUM_MOVES, CA_TENSOR_HEAD_KERNEL});
    t.push_back({ML.bp, CA_NUM_MOVES, CA_TENSOR_BIAS});
  }

  float *A(int l) { return act.p + l * rows_ld; } /* layer l after its ReLU */
  float *Y(int l) { return y.p + l * rows_ld; }   /* and after its BatchNorm */
  const float *X(int l) { return l == 0 ? x0.p : Y(l - 1); }
  static long x_ld(int l) { return l == 0 ? FT_IN_LD : FT_PADW; }

  void forward(const FtShared &sh, const int32_t *rows, int B, bool train) override {
    RT_LAUNCH(ft_k_gather, (B * CA_GAME_STATE_SIZE + 255) / 256, 256, sh.s, sh.states, rows, B, x0.p);
    for (int l = 0; l < CO_MLP_LAYERS; ++l) {
      FtGemm a = mk(X(l), x_ld(l), 1, sh.w + ML.kernel(l), 100, 1, A(l), FT_PADW, 1, B, CO_MLP_WIDTH, ML.in_dim(l));
      a.bias = sh.w + ML.bias(l);
      a.relu = 1;
      ft_gemm(sh.s, a);
      RT_LAUNCH(ft_k_bn_fwd, FT_PADW / 16, 1024, sh.s, (const float *)A(l), Y(l), B, (const float *)sh.w, ML.gamma(l),
                train ? 1 : 0, sh.stat + l * FT_STAT_LD);
    }
    FtGemm p = mk(Y(11), FT_PADW, 1, sh.w + ML.kp, CA_NUM_MOVES, 1, sh.h, FT_PADW, 1, B, CA_NUM_MOVES, CO_MLP_WIDTH);
    p.bias = sh.w + ML.bp;
    ft_gemm(sh.s, p);
    FtGemm vh = mk(Y(11), FT_PADW, 1, sh.w + ML.kv, 1, 1, sh.h + 96, FT_PADW, 1, B, 1, CO_MLP_WIDTH);
    vh.bias = sh.w + ML.bv;
    ft_gemm(sh.s, vh);
  }

  FtSplits backward(const FtShared &sh, int B) override {
    const int kch = ft_split_chunk(B);
    /* heads: dKp = Y11^T Hd[:, :96], dKv = Y11^T Hd[:, 96] (row-split partials) */
    FtGemm a = mk(Y(11), 1, FT_PADW, sh.hd, FT_PADW, 1, sh.g + ML.kp, CA_NUM_MOVES, 1, CO_MLP_WIDTH, CA_NUM_MOVES, B);
    a.kchunk = kch, a.c_split = ML.nw;
    ft_gemm(sh.s, a);
    a = mk(Y(11), 1, FT_PADW, sh.hd + 96, FT_PADW, 1, sh.g + ML.kv, 1, 1, CO_MLP_WIDTH, 1, B);
    a.kchunk = kch, a.c_split = ML.nw;
    ft_gemm(sh.s, a);
    /* dY11 = Hd[:, :96] Kp^T + Hd[:, 96] Kv^T */
    ft_gemm(sh.s, mk(sh.hd, FT_PADW, 1, sh.w + ML.kp, 1, CA_NUM_MOVES, dy.p, FT_PADW, 1, B, CO_MLP_WIDTH, CA_NUM_MOVES));
    a = mk(sh.hd + 96, FT_PADW, 1, sh.w + ML.kv, 1, 1, dy.p, FT_PADW, 1, B, CO_MLP_WIDTH, 1);
    a.accumulate = 1;
    ft_gemm(sh.s, a);
    for (int l = CO_MLP_LAYERS - 1; l >= 0; --l) {
      RT_LAUNCH(ft_k_bn_bwd, FT_PADW / 16, 1024, sh.s, (const float *)dy.p, (const float *)A(l), dz.p, B,
                (const float *)sh.w, ML.bias(l), (const float *)(sh.stat + l * FT_STAT_LD), sh.g);
      a = mk(X(l), 1, x_ld(l), dz.p, FT_PADW, 1, sh.g + ML.kernel(l), CO_MLP_WIDTH, 1, ML.in_dim(l), CO_MLP_WIDTH, B);
      a.kchunk = kch, a.c_split = ML.nw;
      ft_gemm(sh.s, a);
      if (l > 0)
        ft_gemm(sh.s, mk(dz.p, FT_PADW, 1, sh.w + ML.kernel(l), 1, CO_MLP_WIDTH, dy.p, FT_PADW, 1, B, CO_MLP_WIDTH, CO_MLP_WIDTH));
    }
    const int nsplit = (B + kch - 1) / kch;
    return {nsplit, nsplit};
  }
};

FtNet *ft_mlp_create(int max_batch, rt_stream_t s) { return new FtMlp(max_batch, s); }
