// nn_train.hip -- network training: the reference's Keras fit step (main.pyx:221-272) in float32 on the fp32 matrix
// pipe (v_mfma_f32_16x16x4_f32).  This file is what every network shares: the strided GEMM, the loss, the end of a step
// (Adam and the moving statistics), the fitter's state and step driver, and the C ABI.  A network is an FtNet
// (nn_train.h): mlp12x100, the reference's model (wrapper.py:256-282), in nn_train_mlp.hip and rescnn4, the network of
// nets.py, in nn_train_conv.hip.
//
// One training step of a batch of B rows ("Network training"):
//   forward     FtNet::forward: the batch's rows -> the heads' outputs H (96 logits and the value per row)
//   loss        per row: (tanh v - z)^2, -sum t log_softmax, and their gradients (ft_k_loss);
//               column sums of the head gradients and of the loss terms (ft_k_head_reduce)     2 launches
//               (off the default loss ft_k_loss_opt in ft_k_loss's place; with metrics on two launches more, which
//               read H and touch nothing a step uses: nn_train_loss.hip)
//   backward    FtNet::backward: the weight gradient as partials, and how many of them a weight has
//   update      sum of the split partials in a fixed order, Adam (TF ResourceApplyAdam) on kernels, biases,
//               gamma and beta, moving statistics from the batch statistics (ft_k_update)      1 launch
// Every cross-workgroup sum is written as partials and combined in a fixed order by a later launch: no float atomics,
// no grid-wide barriers, so a step is bitwise reproducible.
//
// The data set has two forms.  Expanded: the three arrays of Trainer::writeSamples, 8 symmetry copies of every sample,
// which the networks' input kernels and ft_k_loss read through the batch's row indices.  Packed: the un-augmented rows of
// co_k_pack_samples, whose 8n virtual rows (row v = sample v / 8 under symmetry v % 8) exist only batch by batch: one
// launch (ft_k_assemble) writes the batch's rows as the expanded arrays would hold them and the same kernels, launched
// the same way, read that batch through an identity index -- so a step is the same to the bit in either form.
#include <math.h>

#include <memory>

#include "nn_train.h"
#include "tables.inc"

#define FT_SAMPLE_FLOATS (CA_GAME_STATE_SIZE + CA_NUM_MOVES) /* a packed row: state[70], policy[96] */

typedef float f32x4 __attribute__((ext_vector_type(4)));

/* the strided product that FtGemm (nn_train.h) describes */
__global__ __launch_bounds__(256) void ft_k_gemm(FtGemm g) {
  const int lane = threadIdx.x & 63;
  const int tm = (g.M + 15) >> 4, tn = (g.N + 15) >> 4, ns = (g.K + g.kchunk - 1) / g.kchunk;
  const int id = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (id >= tm * tn * ns) return; /* whole waves leave; the kernel has no barrier */
  const int s = id / (tm * tn), t = id % (tm * tn);
  const int m0 = (t / tn) * 16, n0 = (t % tn) * 16;
  const int k0 = s * g.kchunk, k1 = min(g.K, k0 + g.kchunk);
  const int i = lane & 15, q = lane >> 4;
  const bool am = m0 + i < g.M, bn = n0 + i < g.N;
  const float *Ap = g.A + (long)(m0 + i) * g.sam;
  const float *Bp = g.B + (long)(n0 + i) * g.sbn;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k = k0; k < k1; k += 16) { /* four k steps: their loads in flight together, then four products in order */
    float a[4], b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kk = k + 4 * j + q;
      a[j] = (am && kk < k1) ? Ap[(long)kk * g.sak] : 0.0f;
      b[j] = (bn && kk < k1) ? Bp[(long)kk * g.sbk] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc, 0, 0, 0);
  }
  /* acc[r] = C[m0 + 4q + r][n0 + i] */
  const int n = n0 + i;
  if (n >= g.N) return;
  const float bv = g.bias ? g.bias[n] : 0.0f;
  float *Cp = g.C + (long)s * g.c_split + (long)n * g.scn;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = m0 + 4 * q + r;
    if (m < g.M) {
      float v = acc[r];
      if (g.bias) v = v + bv;
      if (g.relu) v = v > 0.0f ? v : 0.0f;
      if (g.accumulate) v = Cp[(long)m * g.scm] + v;
      Cp[(long)m * g.scm] = v;
    }
  }
}

/* Per row of the heads' outputs H[r] (96 logits, value at 96): the loss terms and the gradients of the batch loss
 * value_mse + 0.25 * policy_cce (means over the B rows) with respect to the logits and to v:
 *   Hd[r][0..95] = 0.25 (softmax * sum t - t) / B,  Hd[r][96] = 2 (tanh v - z)(1 - tanh^2 v) / B,
 *   Hd[r][97] = (tanh v - z)^2,  Hd[r][98] = -sum_j t_j log_softmax_j  (from the logits, as Keras does)
 * 1 - tanh^2 v is one fused multiply-add, rounded once.  As 1 - (t * t) it is biased where tanh saturates: with t = 1 - a
 * the product 1 - 2a + a^2 rounds to 1 - 2a whenever a^2 is under half an ulp of one (a < 1.7e-4, |v| > 4.7), so every
 * such row's factor 2a - a^2 comes out a / 2 of itself too large, all rows the same way (measured 1e-5 to 3e-5 of the
 * value head's whole gradient on a saturated head).
 * WEIGHTED: every one of these 99 terms times the row's sample weight wts[rows[r]] (Keras's sample_weight under
 * SUM_OVER_BATCH_SIZE: the divisor stays B); the unweighted instantiation never reads that last operand and has no such
 * multiply. */
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void ft_k_loss(const float *__restrict__ H, const int32_t *__restrict__ rows, int B,
                                                const float *__restrict__ evals, const float *__restrict__ probs,
                                                float *__restrict__ Hd, const float *__restrict__ wts) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= B) return;
  const float *h = H + (long)r * FT_PADW;
  const float *t = probs + (long)rows[r] * CA_NUM_MOVES;
  float *d = Hd + (long)r * FT_PADW;
  float m = -INFINITY;
  for (int j = 0; j < CA_NUM_MOVES; ++j) m = h[j] > m ? h[j] : m;
  float se = 0.0f;
  for (int j = 0; j < CA_NUM_MOVES; ++j) se += expf(h[j] - m);
  const float lse = m + logf(se);
  float st = 0.0f, ce = 0.0f;
  for (int j = 0; j < CA_NUM_MOVES; ++j) {
    st += t[j];
    ce += t[j] * (lse - h[j]);
  }
  const float inv_b = 1.0f / (float)B;
  if (!WEIGHTED) {
    for (int j = 0; j < CA_NUM_MOVES; ++j) d[j] = 0.25f * (expf(h[j] - lse) * st - t[j]) * inv_b;
    const float tv = tanhf(h[96]);
    const float err = tv - evals[rows[r]];
    d[96] = 2.0f * err * fmaf(-tv, tv, 1.0f) * inv_b;
    d[97] = err * err;
    d[98] = ce;
  } else { /* today's terms, each rounded as above, then times w: a weight of 1 changes no bit, one of 2 doubles exactly */
    const float w = wts[rows[r]];
    for (int j = 0; j < CA_NUM_MOVES; ++j) d[j] = 0.25f * (expf(h[j] - lse) * st - t[j]) * inv_b * w;
    const float tv = tanhf(h[96]);
    const float err = tv - evals[rows[r]];
    d[96] = 2.0f * err * fmaf(-tv, tv, 1.0f) * inv_b * w;
    d[97] = err * err * w;
    d[98] = ce * w;
  }
}

/* the engine's symmetry tables (kernels.h CO_SPACE_SYM, CO_MOVE_SYM), from the same initialisers of tables.inc */
__constant__ int32_t FT_SPACE_SYM[CA_NUM_SYMMETRIES][16] = CO_SPACE_SYM_INIT;
__constant__ int32_t FT_MOVE_SYM[CA_NUM_SYMMETRIES][CA_NUM_MOVES] = CO_MOVE_SYM_INIT;

/* where a batch's rows are fetched from: a packed set (sp != null) or an expanded one */
struct FtSource {
  const float *sp, *oc;               /* state_policy[n][166], outcome[n] */
  const float *states, *evals, *probs; /* [n][70], [n], [n][96] */
};

/* The batch of rows[0..B) written compactly: bs[r] = the state, be[r] = the value label and bp[r] = the policy of row
 * rows[r].  Of a packed set that is virtual row v = rows[r]: sample v / 8 under symmetry k = v % 8, the gathers of
 * co_k_write_samples (state cell j < 64 from SS[k][j / 4] * 4 + j % 4, cells 64..69 as they are, policy entry m from
 * MS[k][m]).  One thread per float of the batch's 166-float rows, so a wave writes consecutive floats and reads within
 * one or two 664-byte samples.  WEIGHTED: bw[r] = the row's sample weight as well, next to be[r], from wt (one weight
 * per packed sample or per expanded row).  The two operands stand last, so that the unweighted instantiation, which
 * reads neither, is instruction for instruction the kernel it was before weights existed. */
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void ft_k_assemble(FtSource d, const int32_t *__restrict__ rows, int B,
                                                    float *__restrict__ bs, float *__restrict__ be,
                                                    float *__restrict__ bp, const float *__restrict__ wt,
                                                    float *__restrict__ bw) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * FT_SAMPLE_FLOATS) return;
  const int r = e / FT_SAMPLE_FLOATS, c = e % FT_SAMPLE_FLOATS;
  const int v = rows[r];
  if (d.sp) {
    const int i = v >> 3, k = v & 7;
    const float *src = d.sp + (long)i * FT_SAMPLE_FLOATS;
    if (c < CA_GAME_STATE_SIZE) {
      bs[(long)r * CA_GAME_STATE_SIZE + c] = src[c < 64 ? FT_SPACE_SYM[k][c >> 2] * 4 + (c & 3) : c];
    } else {
      const int m = c - CA_GAME_STATE_SIZE;
      bp[(long)r * CA_NUM_MOVES + m] = src[CA_GAME_STATE_SIZE + FT_MOVE_SYM[k][m]];
    }
    if (c == 0) be[r] = d.oc[i];
    if (WEIGHTED && c == 0) bw[r] = wt[i];
  } else {
    if (c < CA_GAME_STATE_SIZE) {
      bs[(long)r * CA_GAME_STATE_SIZE + c] = d.states[(long)v * CA_GAME_STATE_SIZE + c];
    } else {
      const int m = c - CA_GAME_STATE_SIZE;
      bp[(long)r * CA_NUM_MOVES + m] = d.probs[(long)v * CA_NUM_MOVES + m];
    }
    if (c == 0) be[r] = d.evals[v];
    if (WEIGHTED && c == 0) bw[r] = wt[v];
  }
}

/* Column sums of Hd over the B rows (fixed order): the head biases' gradients (when g is given; the policy bias at
 * off_bp, the value bias at off_bv) and the batch's value and policy loss sums (loss[0], loss[1]). */
__global__ __launch_bounds__(1024) void ft_k_head_reduce(const float *__restrict__ Hd, int B, float *__restrict__ g,
                                                        int off_bp, int off_bv, float *__restrict__ loss) {
  __shared__ float red[(FT_BN_RG + 1) * 16];
  const int f = blockIdx.x * 16 + (threadIdx.x & 15), rg = threadIdx.x >> 4;
  float s = 0.0f;
  if (f < 99)
    for (int r = rg; r < B; r += FT_BN_RG) s += Hd[(long)r * FT_PADW + f];
  s = ft_colsum(red, s);
  if (rg != 0 || f >= 99) return;
  if (f < 96) {
    if (g) g[off_bp + f] = s;
  } else if (f == 96) {
    if (g) g[off_bv] = s;
  } else {
    loss[f - 97] = s;
  }
}

/* ReLU backward of a dense layer's output A[B][ld] in place on dA, and the column sums of the result (the layer's bias
 * gradient) to gbias[0..ncol), in the fixed order of ft_colsum */
__global__ __launch_bounds__(1024) void ft_k_relu_bwd(float *__restrict__ dA, const float *__restrict__ A, int B, int ld,
                                                     int ncol, float *__restrict__ gbias) {
  __shared__ float red[(FT_BN_RG + 1) * 16];
  const int f = blockIdx.x * 16 + (threadIdx.x & 15), rg = threadIdx.x >> 4;
  float s = 0.0f;
  if (f < ncol)
    for (int r = rg; r < B; r += FT_BN_RG) {
      const long e = (long)r * ld + f;
      const float d = A[e] > 0.0f ? dA[e] : 0.0f;
      dA[e] = d;
      s += d;
    }
  s = ft_colsum(red, s);
  if (rg == 0 && f < ncol) gbias[f] = s;
}

/* The end of a step, one thread per weight of the nw: its gradient is the sum of its partials in order.  sidx[i] < 0:
 * a trainable weight with ns0 (FT_SPLIT0), ns1 (FT_SPLIT1) or one (FT_WHOLE) partial, Adam (TF ResourceApplyAdam,
 * epsilon outside the root; ft_adam, nn_train.h); sidx[i] >= 0: a moving statistic, moved toward the batch statistic
 * stat[sidx[i]] with momentum 0.99.  apply = 0: write the summed gradient to gout only.  PARAM: with Adam's arguments A,
 * and a moving statistic's new value goes to the average as well. */
template <bool PARAM>
__device__ __forceinline__ void ft_update_weight(float *__restrict__ w, float *__restrict__ m, float *__restrict__ v,
                                                 const float *__restrict__ g, int nw, int ns0, int ns1,
                                                 const int32_t *__restrict__ sidx, const float *__restrict__ stat,
                                                 float lr_t, int apply, float *__restrict__ gout, const FtAdamArgs &A) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nw) return;
  const int si = sidx[i];
  const int nsplit = si == FT_SPLIT0 ? ns0 : si == FT_SPLIT1 ? ns1 : 1;
  if (!apply) {
    float s = 0.0f;
    if (si < 0)
      for (int k = 0; k < nsplit; ++k) s += g[(long)k * nw + i];
    gout[i] = s;
    return;
  }
  if (si >= 0) {
    const float mv = w[i];
    const float nv = mv - (mv - stat[si]) * 0.01f;
    w[i] = nv;
    if (PARAM && A.a) A.a[i] = nv;
    return;
  }
  float s = 0.0f;
  for (int k = 0; k < nsplit; ++k) s += g[(long)k * nw + i];
  ft_adam<PARAM>(w, m, v, i, w[i], s, lr_t, A);
}

/* the Adam defaults: the kernel of a step before Adam had arguments, instruction for instruction */
__global__ __launch_bounds__(256) void ft_k_update(float *__restrict__ w, float *__restrict__ m, float *__restrict__ v,
                                                  const float *__restrict__ g, int nw, int ns0, int ns1,
                                                  const int32_t *__restrict__ sidx, const float *__restrict__ stat,
                                                  float lr_t, int apply, float *__restrict__ gout) {
  ft_update_weight<false>(w, m, v, g, nw, ns0, ns1, sidx, stat, lr_t, apply, gout, FtAdamArgs{});
}

__global__ __launch_bounds__(256) void ft_k_update_adam(float *__restrict__ w, float *__restrict__ m, float *__restrict__ v,
                                                       const float *__restrict__ g, int nw, int ns0, int ns1,
                                                       const int32_t *__restrict__ sidx, const float *__restrict__ stat,
                                                       float lr_t, FtAdamArgs A) {
  ft_update_weight<true>(w, m, v, g, nw, ns0, ns1, sidx, stat, lr_t, 1, (float *)nullptr, A);
}

/* w <-> a, every entry of the weight vector (ca_fitter_swap_average) */
__global__ __launch_bounds__(256) void ft_k_average_swap(float *__restrict__ w, float *__restrict__ a, int nw) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nw) return;
  const float t = w[i];
  w[i] = a[i];
  a[i] = t;
}

/* w := a on the trainable weights (ca_fitter_apply_average) */
__global__ __launch_bounds__(256) void ft_k_average_apply(float *__restrict__ w, const float *__restrict__ a,
                                                         const int32_t *__restrict__ sidx, int nw) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nw) return;
  if (sidx[i] < 0) w[i] = a[i];
}

/* ------------------------------------------------------------------ host */
void ft_gemm(rt_stream_t s, const FtGemm &a) {
  const int tiles = ((a.M + 15) / 16) * ((a.N + 15) / 16) * ((a.K + a.kchunk - 1) / a.kchunk);
  if (tiles == 0) return;
  RT_LAUNCH(ft_k_gemm, (tiles + 3) / 4, 256, s, a);
}

void ft_relu_bwd(rt_stream_t s, float *dA, const float *A, int B, int ld, int ncol, float *gbias) {
  RT_LAUNCH(ft_k_relu_bwd, (ncol + 15) / 16, 1024, s, dA, A, B, ld, ncol, gbias);
}

FtNet *ft_net_create(int kind, int max_batch, rt_stream_t s) {
  return kind == CA_NET_RESCNN4 ? ft_rescnn_create(max_batch, s) : ft_mlp_create(max_batch, s);
}

struct ca_fitter {
  int device = 0;
  int nw = 0; /* floats of the weight vector */
  int max_batch = 0;
  int64_t iterations = 0;
  int32_t n = 0, idx_cap = 0; /* addressable rows (8 * ns of a packed set); rows idx holds */
  bool expanded = false;      /* the form: set by ca_fitter_set_data, until ca_fitter_clear_data */
  int32_t ns = 0, cap = 0;    /* packed samples, and how many sp and oc have room for */
  rt_stream_t s = nullptr;
  std::unique_ptr<FtNet> net;
  int dev() const { return device; }
  DevBuf<float> w, m, v, g, gsum, stat, h, hd, loss;
  DevBuf<float> states, evals, probs; /* the expanded set */
  DevBuf<float> sp, oc;               /* the packed set: state_policy[cap][166], outcome[cap] */
  DevBuf<float> wt;                   /* sample weights, when `weighted`: [n] of an expanded set, [cap] beside sp and oc */
  bool weighted = false;              /* ca_fitter_set_sample_weights, ca_fitter_merge_duplicates; until clear_data */
  DevBuf<float> bstates, bevals, bprobs, bwts; /* one batch of a packed set as ft_k_assemble wrote it: max_batch rows */
  DevBuf<int32_t> sidx, idx, ident, bidx; /* ident[r] = r, the rows of an assembled batch; bidx: ca_fitter_fetch_rows */
  std::vector<float> hloss;
  FtOpt opt;                                       /* the fit options (nn_train_opt.hip); all 0: never touched by a step */
  ca_fit_stats last = {sizeof(ca_fit_stats), 0, 0, 0, 0.0, 0.0, 0.0}; /* of the last ca_fitter_train */
  ca_fit_adam adam = CA_FIT_ADAM_INIT; /* Adam's arguments; at their defaults a step never looks at what follows */
  DevBuf<float> vhat, avg;             /* the third slot and the average: no memory before their first use */
  bool avg_valid = false;              /* until ca_fitter_set_weights */
  ca_fit_loss lossopt = CA_FIT_LOSS_INIT; /* the loss; at its defaults a step launches ft_k_loss and no other loss kernel */
  bool metrics_on = false;                /* ca_fitter_set_metrics; off: nothing below has memory */
  int32_t top_k = 5;
  DevBuf<float> mrow, metric; /* the metric terms of a batch's rows [max_batch][8]; the batches' sums [slots][8] */
  std::vector<float> hmetric;
  ca_fit_metrics lastm = {sizeof(ca_fit_metrics), 5, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; /* of the last train or evaluate */

  void init(int dev, int kind, int mb) {
    device = dev;
    max_batch = mb;
    rt_set_device(dev);
    rt_stream_create(&s);
    net.reset(ft_net_create(kind, mb, s));
    nw = net->num_weights();
    const size_t rows = (size_t)((mb + 15) / 16 * 16);
    w.alloc(nw, s);
    m.alloc(nw, s);
    v.alloc(nw, s);
    g.alloc((size_t)FT_NSPLIT * nw, s);
    gsum.alloc(nw, s);
    stat.alloc(net->stat_floats(), s);
    h.alloc(rows * FT_PADW, s);
    hd.alloc(rows * FT_PADW, s);
    std::vector<int32_t> si;
    net->update_table(si);
    sidx.alloc(nw, s);
    rt_h2d(sidx.p, si.data(), nw * sizeof(int32_t), s);
    rt_sync(s);
  }
  ~ca_fitter() { rt_stream_destroy(s); }

  /* what the kernels of a step read a batch through: row indices into three arrays */
  struct Batch {
    const int32_t *rows;
    const float *states, *evals, *probs;
    const float *wts; /* null: an unweighted set */
  };
  FtSource source() const { return FtSource{expanded ? nullptr : sp.p, oc.p, states.p, evals.p, probs.p}; }
  void assemble(const int32_t *rows, int B) {
    const int grid = (B * FT_SAMPLE_FLOATS + 255) / 256;
    if (weighted)
      RT_LAUNCH(ft_k_assemble<true>, grid, 256, s, source(), rows, B, bstates.p, bevals.p, bprobs.p, (const float *)wt.p,
                bwts.p);
    else
      RT_LAUNCH(ft_k_assemble<false>, grid, 256, s, source(), rows, B, bstates.p, bevals.p, bprobs.p,
                (const float *)nullptr, (float *)nullptr);
  }
  /* the batch of rows[0..B) (a device pointer): the expanded set itself, or a packed set's rows assembled */
  Batch batch(const int32_t *rows, int B) {
    if (expanded) return Batch{rows, states.p, evals.p, probs.p, weighted ? wt.p : nullptr};
    assemble(rows, B);
    return Batch{ident.p, bstates.p, bevals.p, bprobs.p, weighted ? bwts.p : nullptr};
  }
  FtShared shared(const Batch &b) const { return FtShared{s, w.p, g.p, stat.p, h.p, hd.p, b.states}; }

  /* is the loss the reference's value_mse + 0.25 policy_cce?  Then a step runs the kernels that know of no other. */
  bool loss_default() const {
    return lossopt.value_weight == 1.0f && lossopt.policy_weight == 0.25f && lossopt.label_smoothing == 0.0f &&
           lossopt.value_loss == CA_VALUE_LOSS_MSE;
  }
  /* the batch's metric sums to metric.p[FT_METRIC_W * slot], from the H the loss kernel reads */
  void metric_terms(const Batch &b, int B, int slot) {
    ft_metrics(s, h.p, b.rows, B, b.evals, b.probs, b.wts, top_k, mrow.p, metric.p + (size_t)FT_METRIC_W * slot);
  }
  /* loss terms of the batch (and the logit / value gradients in Hd); loss sums to loss.p[2 * slot] */
  void loss_terms(const Batch &b, int B, bool grads, int slot) {
    if (!loss_default())
      ft_loss_opt(s, h.p, b.rows, B, b.evals, b.probs, hd.p, b.wts,
                  FtLossArgs{lossopt.value_weight, lossopt.policy_weight, lossopt.label_smoothing, lossopt.huber_delta,
                             lossopt.value_loss == CA_VALUE_LOSS_HUBER});
    else if (b.wts)
      RT_LAUNCH(ft_k_loss<true>, (B + 255) / 256, 256, s, (const float *)h.p, b.rows, B, b.evals, b.probs, hd.p, b.wts);
    else
      RT_LAUNCH(ft_k_loss<false>, (B + 255) / 256, 256, s, (const float *)h.p, b.rows, B, b.evals, b.probs, hd.p,
                (const float *)nullptr);
    RT_LAUNCH(ft_k_head_reduce, FT_PADW / 16, 1024, s, (const float *)hd.p, B, grads ? g.p : (float *)nullptr,
              net->policy_bias(), net->value_bias(), loss.p + 2 * slot);
  }

  /* forward, loss (sums to slot) and backward of one batch: leaves the gradient partials and returns their counts.
   * metrics: the batch's metric sums to slot as well */
  FtSplits gradient(const int32_t *rows, int B, int slot, bool metrics = false) {
    const Batch b = batch(rows, B);
    const FtShared sh = shared(b);
    net->forward(sh, b.rows, B, true);
    loss_terms(b, B, true, slot);
    if (metrics) metric_terms(b, B, slot);
    return net->backward(sh, B);
  }

  /* the end of a step on the partials gradient() left: Adam and the moving statistics, or (apply = false) the
   * summed gradient to gsum only */
  void update(FtSplits ns, float lr_t, bool apply) {
    RT_LAUNCH(ft_k_update, (nw + 255) / 256, 256, s, w.p, m.p, v.p, (const float *)g.p, nw, ns.rows, ns.pixels,
              (const int32_t *)sidx.p, (const float *)stat.p, lr_t, apply ? 1 : 0, gsum.p);
  }

  /* the end of a step with options on: the summed gradient to gsum as ca_fitter_gradients has it, then steps 1 to 4 */
  void update_with_options(FtSplits ns, float lr, float lr_t, int slot, const FtAdamArgs *A) {
    update(ns, 0.0f, false);
    opt.step(s, w.p, m.p, v.p, gsum.p, sidx.p, stat.p, lr, lr_t, slot, A);
  }
  /* the end of a step with Adam's arguments off their defaults: ft_k_update's work, parametrised */
  void update_adam(FtSplits ns, float lr_t, const FtAdamArgs &A) {
    RT_LAUNCH(ft_k_update_adam, (nw + 255) / 256, 256, s, w.p, m.p, v.p, (const float *)g.p, nw, ns.rows, ns.pixels,
              (const int32_t *)sidx.p, (const float *)stat.p, lr_t, A);
  }
  /* is every one of Adam's arguments at its default?  Then a step runs the kernels that know of none. */
  bool adam_default() const {
    return adam.beta_1 == 0.9f && adam.beta_2 == 0.999f && adam.epsilon == 1e-7f && !adam.amsgrad &&
           !(adam.ema_momentum > 0.0f);
  }
  /* Adam's arguments of the step that brings the step count to `step`.  The third slot and the average get their memory
   * at their first use (zeroed, on the stream); an invalid average starts as the weights before the step. */
  FtAdamArgs adam_args(int64_t step) {
    FtAdamArgs A = {adam.beta_1, adam.beta_2, adam.epsilon, adam.ema_momentum, nullptr, nullptr, 0};
    if (adam.amsgrad) {
      if (!vhat.p) vhat.alloc(nw, s);
      A.h = vhat.p;
    }
    if (adam.ema_momentum > 0.0f) {
      if (!avg.p) avg.alloc(nw, s);
      if (!avg_valid) rt_d2d(avg.p, w.p, (size_t)nw * sizeof(float), s);
      avg_valid = true;
      A.a = avg.p;
      A.overwrite = adam.ema_overwrite_frequency > 0 && step % adam.ema_overwrite_frequency == 0;
    }
    return A;
  }
  void need_average(const char *who) {
    if (!avg_valid) throw CaError(CA_ERR_STATE, std::string(who) + ": the fitter has no average (no step with ema_momentum > 0, no ca_fitter_set_slot)");
  }
  /* the piece table of the options' kernels, made when options are first switched on.  Those kernels take a weight for
   * a moving statistic by its tensor's class and ft_k_update by its code: the two tables must agree. */
  void plan_options() {
    if (opt.pieces.p) return;
    std::vector<FtTensor> tt;
    std::vector<int32_t> si;
    net->tensor_table(tt);
    net->update_table(si);
    for (const FtTensor &t : tt)
      for (int32_t i = t.off; i < t.off + t.count && i >= 0 && i < nw; ++i)
        if ((si[i] >= 0) != (t.cls == CA_TENSOR_MOVING))
          throw CaError(CA_ERR_INTERNAL, "ca_fitter: tensor_table and update_table disagree about the moving statistics");
    opt.plan(tt, nw, s);
  }

  void need_data() {
    if (n <= 0) throw CaError(CA_ERR_STATE, "ca_fitter: no data (ca_fitter_set_data, ca_fitter_add_samples)");
  }
  /* room in idx for the nr rows of a call: an expanded set has it from ca_fitter_set_data, a packed one takes what its
   * largest call asked for, not a share of its capacity */
  void need_idx(int32_t nr) {
    if (idx_cap >= nr) return;
    idx.alloc((size_t)nr, s);
    idx_cap = nr;
  }
  /* the buffers of an assembled batch */
  void need_stage() {
    if (bidx.p) return;
    std::vector<int32_t> id((size_t)max_batch);
    for (int32_t i = 0; i < max_batch; ++i) id[i] = i;
    bstates.alloc((size_t)max_batch * CA_GAME_STATE_SIZE, s);
    bevals.alloc((size_t)max_batch, s);
    bprobs.alloc((size_t)max_batch * CA_NUM_MOVES, s);
    bwts.alloc((size_t)max_batch, s);
    ident.alloc((size_t)max_batch, s);
    rt_h2d(ident.p, id.data(), id.size() * sizeof(int32_t), s);
    rt_sync(s); /* id is a local */
    bidx.alloc((size_t)max_batch, s);
  }
  void clear_data() {
    n = 0, ns = 0, cap = 0, idx_cap = 0, expanded = false, weighted = false;
    states.release(), evals.release(), probs.release(), sp.release(), oc.release(), idx.release(), wt.release();
  }
  /* the packed rows [first, first + count) to the front of the buffers they are in (a slide of the window), device to
   * device without a second buffer: in pieces of `first` rows from the front, each of which ends before its source
   * begins, queued in order on one stream.  Only a drop of less than 1/64 of what stays goes through new buffers. */
  void slide_samples(int32_t first, int32_t count) {
    if ((int64_t)first * 64 < count) {
      move_samples(first, count, cap);
      return;
    }
    for (int32_t d = 0; d < count; d += first) {
      const size_t k = (size_t)(count - d < first ? count - d : first);
      rt_d2d(sp.p + (size_t)d * FT_SAMPLE_FLOATS, sp.p + ((size_t)d + first) * FT_SAMPLE_FLOATS,
             k * FT_SAMPLE_FLOATS * sizeof(float), s);
      rt_d2d(oc.p + d, oc.p + d + first, k * sizeof(float), s);
      if (weighted) rt_d2d(wt.p + d, wt.p + d + first, k * sizeof(float), s);
    }
    rt_sync(s);
  }
  /* the packed rows [first, first + count) to the front of new buffers with room for new_cap samples, device to device */
  void move_samples(int32_t first, int32_t count, int32_t new_cap) {
    DevBuf<float> nsp, noc, nwt;
    nsp.alloc((size_t)new_cap * FT_SAMPLE_FLOATS, s);
    noc.alloc((size_t)new_cap, s);
    if (weighted) {
      nwt.alloc((size_t)new_cap, s);
      rt_d2d(nwt.p, wt.p + first, (size_t)count * sizeof(float), s);
    }
    rt_d2d(nsp.p, sp.p + (size_t)first * FT_SAMPLE_FLOATS, (size_t)count * FT_SAMPLE_FLOATS * sizeof(float), s);
    rt_d2d(noc.p, oc.p + first, (size_t)count * sizeof(float), s);
    rt_sync(s); /* before the old buffers are freed */
    std::swap(sp, nsp);
    std::swap(oc, noc);
    if (weighted) std::swap(wt, nwt);
    cap = new_cap;
  }
  /* room for `add` more packed samples behind the ns there are; capacity grows geometrically */
  void reserve(int32_t add) {
    if (expanded) throw CaError(CA_ERR_STATE, "ca_fitter: the data set is expanded (ca_fitter_clear_data first)");
    if (weighted) throw CaError(CA_ERR_STATE, "ca_fitter: the data set carries sample weights (ca_fitter_clear_data first)");
    if (add < 0) throw CaError(CA_ERR_ARG, "ca_fitter: negative sample count");
    const int64_t need = (int64_t)ns + add, most = INT32_MAX / CA_NUM_SYMMETRIES;
    if (need > most) throw CaError(CA_ERR_ARG, "ca_fitter: more than INT32_MAX virtual rows");
    need_stage();
    if (need <= cap) return;
    int64_t nc = 2 * (int64_t)cap > need ? 2 * (int64_t)cap : need;
    nc = nc < 1024 ? 1024 : nc > most ? most : nc;
    move_samples(0, ns, (int32_t)nc);
  }
  void added(int32_t add) {
    ns += add;
    n = ns * CA_NUM_SYMMETRIES;
  }
  void check_n(size_t n_floats) {
    if (n_floats != (size_t)nw)
      throw CaError(CA_ERR_ARG, std::string("ca_fitter: ") + net->name() + " has " + std::to_string(nw) + " floats");
  }
  void check_rows(const int32_t *rows, int32_t nr) {
    if (nr < 0 || nr > n) throw CaError(CA_ERR_ARG, "ca_fitter: more rows than the data set holds");
    check_range(rows, nr);
  }
  void check_range(const int32_t *rows, int32_t nr) {
    for (int32_t i = 0; i < nr; ++i)
      if (rows[i] < 0 || rows[i] >= n) throw CaError(CA_ERR_ARG, "ca_fitter: row index out of range");
  }
  void check_batch(int32_t batch) {
    if (batch < 1 || batch > max_batch) throw CaError(CA_ERR_ARG, "ca_fitter: batch must be in [1, max_batch]");
  }
  void ensure_loss(int slots) {
    if ((int)hloss.size() < 2 * slots) {
      loss.alloc((size_t)2 * slots, s);
      hloss.assign((size_t)2 * slots, 0.0f);
    }
  }
  /* the metrics' buffers, for a call of `slots` batches */
  void ensure_metrics(int slots) {
    if (!mrow.p) mrow.alloc((size_t)max_batch * FT_METRIC_W, s);
    if (hmetric.size() < (size_t)FT_METRIC_W * slots) {
      metric.alloc((size_t)FT_METRIC_W * slots, s);
      hmetric.assign((size_t)FT_METRIC_W * slots, 0.0f);
    }
  }
  /* the call's metrics from its nb batches' sums, which losses() fetched: the batches added in float64 */
  void metrics_of(int nb, int32_t nr) {
    double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < nb; ++b)
      for (int k = 0; k < 6; ++k) sum[k] += (double)hmetric[(size_t)FT_METRIC_W * b + k];
    const double ws = sum[5];
    auto mean = [&](int k) { return ws > 0.0 ? sum[k] / ws : 0.0; };
    lastm = ca_fit_metrics{sizeof(ca_fit_metrics), top_k, nr, ws, mean(0), mean(1), mean(2), mean(3), mean(4)};
  }
  /* per-batch sums -> out[3] = {value_weight value + policy_weight policy, value, policy}, means weighted by batch size;
   * per[3 * b] */
  void losses(int nb, int32_t nr, int32_t batch, double *out, float *per) { losses(nb, nr, batch, out, per, 0, false); }
  /* reg: with the regulariser's R added to the totals, 1: R of every batch (ca_fitter_train), 2: one R for all
   * (ca_fitter_evaluate); the options' buffer, and with `metrics` the batches' metric sums, come back in the same
   * synchronisation */
  void losses(int nb, int32_t nr, int32_t batch, double *out, float *per, int reg, bool metrics) {
    rt_d2h(hloss.data(), loss.p, (size_t)2 * nb * sizeof(float), s);
    if (reg) opt.fetch(reg == 1 ? nb : 1, s);
    if (metrics) rt_d2h(hmetric.data(), metric.p, (size_t)FT_METRIC_W * nb * sizeof(float), s);
    rt_sync(s);
    if (metrics) metrics_of(nb, nr);
    const float vw = lossopt.value_weight, pw = lossopt.policy_weight; /* 1.0f * lv has the bits of lv */
    double sv = 0.0, sp = 0.0, sr = 0.0;
    for (int b = 0; b < nb; ++b) {
      const int rb = b * batch + batch <= nr ? batch : nr - b * batch;
      const float lv = hloss[2 * b] / (float)rb, lp = hloss[2 * b + 1] / (float)rb;
      if (per) {
        per[3 * b] = reg ? vw * lv + pw * lp + (float)opt.R(reg == 1 ? b : 0) : vw * lv + pw * lp;
        per[3 * b + 1] = lv;
        per[3 * b + 2] = lp;
      }
      sv += (double)lv * rb;
      sp += (double)lp * rb;
      if (reg) sr += opt.R(reg == 1 ? b : 0) * rb;
    }
    if (out) {
      out[1] = nr ? sv / nr : 0.0;
      out[2] = nr ? sp / nr : 0.0;
      out[0] = (double)vw * out[1] + (double)pw * out[2];
      if (reg) out[0] += nr ? sr / nr : 0.0;
    }
  }
};

extern "C" int ca_fitter_create(int device, int32_t max_batch, ca_fitter **out) {
  return ca_fitter_create_net(device, CA_NET_MLP12X100, max_batch, out);
}

extern "C" int ca_fitter_create_net(int device, int32_t net, int32_t max_batch, ca_fitter **out) {
  if (!out || max_batch < 1 || max_batch > (1 << 20)) {
    co_set_last_error("ca_fitter_create: null argument or max_batch outside [1, 2^20]");
    return CA_ERR_ARG;
  }
  if (net != CA_NET_MLP12X100 && net != CA_NET_RESCNN4) {
    co_set_last_error("ca_fitter_create_net: net must be CA_NET_MLP12X100 or CA_NET_RESCNN4");
    return CA_ERR_ARG;
  }
  *out = nullptr;
  int rc = ca_device_check(device);
  if (rc != CA_OK) return rc;
  return co_guard([&] {
    auto f = std::make_unique<ca_fitter>();
    f->init(device, net, max_batch);
    *out = f.release();
  });
}

extern "C" void ca_fitter_destroy(ca_fitter *f) {
  if (!f) return;
  try {
    rt_set_device(f->device);
    rt_sync(f->s);
  } catch (const std::exception &) {
  }
  delete f;
}

extern "C" int ca_fitter_set_weights(ca_fitter *f, const float *weights, size_t n_floats) {
  return co_guard(f, [&] {
    f->check_n(n_floats);
    if (!weights) throw CaError(CA_ERR_ARG, "null weights");
    rt_h2d(f->w.p, weights, f->nw * sizeof(float), f->s);
    rt_sync(f->s);
    f->avg_valid = false;
  });
}

extern "C" int ca_fitter_get_weights(ca_fitter *f, float *weights, size_t n_floats) {
  return co_guard(f, [&] {
    f->check_n(n_floats);
    if (!weights) throw CaError(CA_ERR_ARG, "null weights");
    rt_d2h(weights, f->w.p, f->nw * sizeof(float), f->s);
    rt_sync(f->s);
  });
}

extern "C" int ca_fitter_set_optimizer(ca_fitter *f, const float *m, const float *v, size_t n_floats, int64_t iterations) {
  return co_guard(f, [&] {
    f->check_n(n_floats);
    if (!m || !v || iterations < 0) throw CaError(CA_ERR_ARG, "null slots or negative iterations");
    rt_h2d(f->m.p, m, f->nw * sizeof(float), f->s);
    rt_h2d(f->v.p, v, f->nw * sizeof(float), f->s);
    if (f->vhat.p) rt_memset(f->vhat.p, 0, f->nw * sizeof(float), f->s);
    rt_sync(f->s);
    f->iterations = iterations;
  });
}

extern "C" int ca_fitter_get_optimizer(ca_fitter *f, float *m, float *v, size_t n_floats, int64_t *iterations) {
  return co_guard(f, [&] {
    f->check_n(n_floats);
    if (!m || !v || !iterations) throw CaError(CA_ERR_ARG, "null output");
    rt_d2h(m, f->m.p, f->nw * sizeof(float), f->s);
    rt_d2h(v, f->v.p, f->nw * sizeof(float), f->s);
    rt_sync(f->s);
    *iterations = f->iterations;
  });
}

extern "C" int ca_fitter_set_data(ca_fitter *f, const float *states, const float *evals, const float *probs, int32_t n) {
  return co_guard(f, [&] {
    if (n < 1 || !states || !evals || !probs) throw CaError(CA_ERR_ARG, "ca_fitter_set_data: empty or null");
    f->clear_data(); /* no data while the buffers are being replaced: a failure below leaves the fitter without, not with half */
    f->expanded = true;
    f->states.alloc((size_t)n * CA_GAME_STATE_SIZE, f->s);
    f->evals.alloc((size_t)n, f->s);
    f->probs.alloc((size_t)n * CA_NUM_MOVES, f->s);
    f->idx.alloc((size_t)n, f->s);
    f->idx_cap = n;
    rt_h2d(f->states.p, states, (size_t)n * CA_GAME_STATE_SIZE * sizeof(float), f->s);
    rt_h2d(f->evals.p, evals, (size_t)n * sizeof(float), f->s);
    rt_h2d(f->probs.p, probs, (size_t)n * CA_NUM_MOVES * sizeof(float), f->s);
    rt_sync(f->s);
    f->n = n;
  });
}

extern "C" int ca_fitter_train(ca_fitter *f, const int32_t *rows, int32_t n_rows, int32_t batch, float learning_rate,
                               double *out_losses, float *batch_losses) {
  return co_guard(f, [&] {
    f->need_data();
    f->check_batch(batch);
    if (!rows || n_rows < 1) throw CaError(CA_ERR_ARG, "ca_fitter_train: no rows");
    f->check_rows(rows, n_rows);
    f->need_idx(n_rows);
    const int nb = (n_rows + batch - 1) / batch;
    f->ensure_loss(nb);
    if (f->metrics_on) f->ensure_metrics(nb);
    rt_h2d(f->idx.p, rows, (size_t)n_rows * sizeof(int32_t), f->s);
    const bool options = f->opt.on(), adam_on = !f->adam_default();
    if (options) f->opt.begin(nb, f->s);
    f->last = ca_fit_stats{sizeof(ca_fit_stats), 0, 0, 0, 0.0, 0.0, 0.0};
    for (int b = 0; b < nb; ++b) {
      const int B = b * batch + batch <= n_rows ? batch : n_rows - b * batch;
      const FtSplits ns = f->gradient(f->idx.p + (size_t)b * batch, B, b, f->metrics_on);
      /* Keras Adam: local_step = iterations + 1, lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t), in float32 */
      const float t = (float)(f->iterations + 1);
      const float lr_t = learning_rate * (sqrtf(1.0f - powf(f->adam.beta_2, t)) / (1.0f - powf(f->adam.beta_1, t)));
      if (adam_on) {
        const FtAdamArgs A = f->adam_args(f->iterations + 1);
        if (options)
          f->update_with_options(ns, learning_rate, lr_t, b, &A);
        else
          f->update_adam(ns, lr_t, A);
      } else if (options)
        f->update_with_options(ns, learning_rate, lr_t, b, nullptr);
      else
        f->update(ns, lr_t, true);
      f->iterations += 1;
    }
    f->losses(nb, n_rows, batch, out_losses, batch_losses, options ? 1 : 0, f->metrics_on);
    if (options) { /* the statistics came back with the losses */
      const double *st = f->opt.hout.data();
      f->last.steps = nb;
      f->last.clipped_steps = (int64_t)st[3];
      f->last.regularization = st[0] / nb;
      f->last.grad_norm = st[1] / nb;
      f->last.grad_norm_max = st[2];
    }
  });
}

extern "C" int ca_fitter_evaluate(ca_fitter *f, int32_t row0, int32_t n_rows, int32_t batch, double *out_losses) {
  return co_guard(f, [&] {
    f->need_data();
    f->check_batch(batch);
    if (n_rows < 1 || row0 < 0 || (int64_t)row0 + n_rows > f->n)
      throw CaError(CA_ERR_ARG, "ca_fitter_evaluate: rows out of range");
    f->need_idx(n_rows);
    std::vector<int32_t> rows(n_rows);
    for (int32_t i = 0; i < n_rows; ++i) rows[i] = row0 + i;
    const int nb = (n_rows + batch - 1) / batch;
    f->ensure_loss(nb);
    if (f->metrics_on) f->ensure_metrics(nb);
    rt_h2d(f->idx.p, rows.data(), (size_t)n_rows * sizeof(int32_t), f->s);
    const bool reg = f->opt.on() && f->opt.regularized(); /* the weights do not move: one R for the call */
    if (reg) {
      f->opt.begin(1, f->s);
      f->opt.regularization(f->s, f->w.p, 0);
    }
    for (int b = 0; b < nb; ++b) {
      const int B = b * batch + batch <= n_rows ? batch : n_rows - b * batch;
      const ca_fitter::Batch bt = f->batch(f->idx.p + (size_t)b * batch, B);
      f->net->forward(f->shared(bt), bt.rows, B, false);
      f->loss_terms(bt, B, false, b);
      if (f->metrics_on) f->metric_terms(bt, B, b);
    }
    f->losses(nb, n_rows, batch, out_losses, nullptr, reg ? 2 : 0, f->metrics_on);
  });
}

extern "C" int ca_fitter_gradients(ca_fitter *f, const int32_t *rows, int32_t n_rows, float *grads, double *out_losses) {
  return co_guard(f, [&] {
    f->need_data();
    f->check_batch(n_rows);
    if (!rows || !grads) throw CaError(CA_ERR_ARG, "null argument");
    f->check_rows(rows, n_rows);
    f->need_idx(n_rows);
    f->ensure_loss(1);
    rt_h2d(f->idx.p, rows, (size_t)n_rows * sizeof(int32_t), f->s);
    f->update(f->gradient(f->idx.p, n_rows, 0), 0.0f, false);
    rt_d2h(grads, f->gsum.p, f->nw * sizeof(float), f->s);
    f->losses(1, n_rows, n_rows, out_losses, nullptr);
  });
}

extern "C" int ca_fitter_clear_data(ca_fitter *f) {
  return co_guard(f, [&] {
    rt_sync(f->s);
    f->clear_data();
  });
}

extern "C" int ca_fitter_add_samples(ca_fitter *f, const float *state_policy, const float *outcome, int32_t n) {
  return co_guard(f, [&] {
    if (!state_policy || !outcome || n < 0) throw CaError(CA_ERR_ARG, "ca_fitter_add_samples: null or negative");
    f->reserve(n);
    rt_h2d(f->sp.p + (size_t)f->ns * FT_SAMPLE_FLOATS, state_policy, (size_t)n * FT_SAMPLE_FLOATS * sizeof(float), f->s);
    rt_h2d(f->oc.p + f->ns, outcome, (size_t)n * sizeof(float), f->s);
    rt_sync(f->s);
    f->added(n);
  });
}

/* is p memory of the fitter's device? */
static void ft_check_device_ptr(const ca_fitter *f, const void *p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    throw CaError(CA_ERR_ARG, "ca_fitter_add_device_samples: not a device pointer");
  }
  if (a.type != hipMemoryTypeDevice || a.device != f->device)
    throw CaError(CA_ERR_ARG, "ca_fitter_add_device_samples: not memory of the fitter's device");
}

extern "C" int ca_fitter_add_device_samples(ca_fitter *f, const void *d_state_policy, const void *d_outcome, int32_t n) {
  return co_guard(f, [&] {
    if (!d_state_policy || !d_outcome || n < 0) throw CaError(CA_ERR_ARG, "ca_fitter_add_device_samples: null or negative");
    ft_check_device_ptr(f, d_state_policy);
    ft_check_device_ptr(f, d_outcome);
    f->reserve(n);
    rt_d2d(f->sp.p + (size_t)f->ns * FT_SAMPLE_FLOATS, d_state_policy, (size_t)n * FT_SAMPLE_FLOATS * sizeof(float), f->s);
    rt_d2d(f->oc.p + f->ns, d_outcome, (size_t)n * sizeof(float), f->s);
    rt_sync(f->s);
    f->added(n);
  });
}

extern "C" int ca_fitter_add_trainer_samples(ca_fitter *f, ca_trainer *t, int32_t *n_added) {
  return co_guard(f, [&] {
    if (!t || !n_added) throw CaError(CA_ERR_ARG, "ca_fitter_add_trainer_samples: null argument");
    /* the trainer's own entry points have left their message in ca_last_error */
    auto ok = [](int rc) {
      if (rc != CA_OK) throw CaError(rc, ca_last_error());
    };
    int32_t dev = -1, count = 0, got = 0;
    ok(ca_trainer_device(t, &dev));
    if (dev != f->device) throw CaError(CA_ERR_ARG, "ca_fitter_add_trainer_samples: the trainer is on another device");
    ok(ca_trainer_num_samples(t, &count));
    f->reserve(count);
    rt_sync(f->s); /* the buffers' clears and moves are on the fitter's stream, the pack on the trainer's */
    ok(ca_trainer_pack_samples_device(t, f->sp.p + (size_t)f->ns * FT_SAMPLE_FLOATS, f->oc.p + f->ns, f->cap - f->ns, &got));
    f->added(got);
    *n_added = got;
  });
}

extern "C" int ca_fitter_drop_samples(ca_fitter *f, int32_t n_oldest) {
  return co_guard(f, [&] {
    if (f->expanded) throw CaError(CA_ERR_STATE, "ca_fitter_drop_samples: the data set is expanded");
    if (n_oldest < 0 || n_oldest > f->ns) throw CaError(CA_ERR_ARG, "ca_fitter_drop_samples: more than the set holds");
    if (n_oldest == 0) return;
    rt_sync(f->s);
    if (n_oldest < f->ns) f->slide_samples(n_oldest, f->ns - n_oldest);
    f->ns -= n_oldest;
    f->added(0);
  });
}

extern "C" int ca_fitter_data_info(ca_fitter *f, int32_t *rows, int32_t *samples) {
  return co_guard(f, [&] {
    if (!rows || !samples) throw CaError(CA_ERR_ARG, "ca_fitter_data_info: null output");
    *rows = f->n;
    *samples = f->expanded ? 0 : f->ns;
  });
}

extern "C" int ca_fitter_fetch_rows(ca_fitter *f, const int32_t *rows, int32_t n_rows, float *states, float *evals,
                                    float *probs) {
  return co_guard(f, [&] {
    f->need_data();
    if (!rows || !states || !evals || !probs || n_rows < 0) throw CaError(CA_ERR_ARG, "ca_fitter_fetch_rows: null or negative");
    f->check_range(rows, n_rows);
    f->need_stage();
    for (int32_t r0 = 0; r0 < n_rows; r0 += f->max_batch) {
      const int B = n_rows - r0 < f->max_batch ? n_rows - r0 : f->max_batch;
      rt_h2d(f->bidx.p, rows + r0, (size_t)B * sizeof(int32_t), f->s);
      f->assemble(f->bidx.p, B);
      rt_d2h(states + (size_t)r0 * CA_GAME_STATE_SIZE, f->bstates.p, (size_t)B * CA_GAME_STATE_SIZE * sizeof(float), f->s);
      rt_d2h(evals + r0, f->bevals.p, (size_t)B * sizeof(float), f->s);
      rt_d2h(probs + (size_t)r0 * CA_NUM_MOVES, f->bprobs.p, (size_t)B * CA_NUM_MOVES * sizeof(float), f->s);
      rt_sync(f->s);
    }
  });
}

/* ------------------------------------------------------------------ sample weights, merging of duplicates */
extern "C" int ca_fitter_set_sample_weights(ca_fitter *f, const float *weights, int32_t n) {
  return co_guard(f, [&] {
    f->need_data();
    if (!weights) { /* back to the unweighted set */
      rt_sync(f->s);
      f->weighted = false;
      f->wt.release();
      return;
    }
    const int32_t units = f->expanded ? f->n : f->ns;
    if (n != units)
      throw CaError(CA_ERR_ARG, "ca_fitter_set_sample_weights: " + std::to_string(units) + " weights are needed, got " +
                                    std::to_string(n));
    for (int32_t i = 0; i < n; ++i)
      if (!(weights[i] >= 0.0f) || weights[i] == INFINITY) /* (a NaN fails the first comparison) */
        throw CaError(CA_ERR_ARG, "ca_fitter_set_sample_weights: every weight must be finite and >= 0");
    if (!f->weighted) f->wt.alloc((size_t)(f->expanded ? f->n : f->cap), f->s);
    rt_h2d(f->wt.p, weights, (size_t)n * sizeof(float), f->s);
    rt_sync(f->s);
    f->weighted = true;
  });
}

extern "C" int ca_fitter_get_sample_weights(ca_fitter *f, float *out, int32_t n) {
  return co_guard(f, [&] {
    f->need_data();
    const int32_t units = f->expanded ? f->n : f->ns;
    if (!out || n != units)
      throw CaError(CA_ERR_ARG, "ca_fitter_get_sample_weights: null output, or not the " + std::to_string(units) +
                                    " weights of the set");
    if (!f->weighted) { /* an unweighted set counts every row once */
      for (int32_t i = 0; i < n; ++i) out[i] = 1.0f;
      return;
    }
    rt_d2h(out, f->wt.p, (size_t)n * sizeof(float), f->s);
    rt_sync(f->s);
  });
}

extern "C" int ca_fitter_merge_duplicates(ca_fitter *f, int normalize, int32_t *before, int32_t *after) {
  return co_guard(f, [&] {
    if (!before || !after) throw CaError(CA_ERR_ARG, "ca_fitter_merge_duplicates: null output");
    if (f->expanded) throw CaError(CA_ERR_STATE, "ca_fitter_merge_duplicates: the data set is expanded");
    if (f->ns <= 0) throw CaError(CA_ERR_STATE, "ca_fitter_merge_duplicates: no samples (ca_fitter_add_samples)");
    rt_sync(f->s);
    FtMerged m = ft_merge_duplicates(f->s, f->sp.p, f->oc.p, f->weighted ? f->wt.p : nullptr, f->ns, normalize != 0);
    /* the merged samples are in buffers of their own: swapped in as move_samples does; nothing waits on the old ones */
    *before = f->ns;
    *after = m.count;
    std::swap(f->sp, m.sp);
    std::swap(f->oc, m.oc);
    std::swap(f->wt, m.wt);
    f->weighted = true;
    f->cap = m.cap;
    f->ns = m.count;
    f->added(0);
  });
}

/* ------------------------------------------------------------------ fit options */
extern "C" int ca_fitter_set_options(ca_fitter *f, const ca_fit_options *options) {
  return co_guard(f, [&] {
    if (!options || options->struct_size < sizeof(uint32_t)) throw CaError(CA_ERR_ARG, "ca_fitter_set_options: null, or a struct_size below 4");
    ca_fit_options o = {}; /* the defaults: everything off */
    const size_t n = options->struct_size < sizeof(o) ? options->struct_size : sizeof(o);
    memcpy(&o, options, n);
    o.struct_size = sizeof(o);
    const float vals[6] = {o.l1, o.l2, o.weight_decay, o.clipvalue, o.clipnorm, o.global_clipnorm};
    for (float x : vals)
      if (!(x >= 0.0f) || x == INFINITY) /* (a NaN fails the first comparison) */
        throw CaError(CA_ERR_ARG, "ca_fitter_set_options: every value must be finite and >= 0");
    if (o.regularize < 0 || o.regularize > 1) throw CaError(CA_ERR_ARG, "ca_fitter_set_options: regularize must be 0 or 1");
    if ((o.clipvalue > 0.0f) + (o.clipnorm > 0.0f) + (o.global_clipnorm > 0.0f) > 1)
      throw CaError(CA_ERR_ARG, "ca_fitter_set_options: at most one of clipvalue, clipnorm and global_clipnorm");
    FtOpt probe;
    probe.o = o;
    if (probe.on()) f->plan_options();
    f->opt.o = o;
  });
}

extern "C" int ca_fitter_get_options(ca_fitter *f, ca_fit_options *out) {
  return co_guard(f, [&] {
    if (!out || out->struct_size < sizeof(uint32_t)) throw CaError(CA_ERR_ARG, "ca_fitter_get_options: null, or a struct_size below 4");
    ca_fit_options o = f->opt.o;
    o.struct_size = (uint32_t)(out->struct_size < sizeof(o) ? out->struct_size : sizeof(o));
    memcpy(out, &o, o.struct_size);
  });
}

extern "C" int ca_fitter_train_stats(ca_fitter *f, ca_fit_stats *out) {
  return co_guard(f, [&] {
    if (!out || out->struct_size < sizeof(uint32_t)) throw CaError(CA_ERR_ARG, "ca_fitter_train_stats: null, or a struct_size below 4");
    ca_fit_stats st = f->last;
    st.struct_size = (uint32_t)(out->struct_size < sizeof(st) ? out->struct_size : sizeof(st));
    memcpy(out, &st, st.struct_size);
  });
}

/* ------------------------------------------------------------------ Adam's arguments, the third slot, the average */
extern "C" int ca_fitter_set_adam(ca_fitter *f, const ca_fit_adam *adam) {
  return co_guard(f, [&] {
    if (!adam || adam->struct_size < sizeof(uint32_t)) throw CaError(CA_ERR_ARG, "ca_fitter_set_adam: null, or a struct_size below 4");
    ca_fit_adam a = CA_FIT_ADAM_INIT; /* the defaults for what the caller's struct does not have */
    const size_t n = adam->struct_size < sizeof(a) ? adam->struct_size : sizeof(a);
    memcpy(&a, adam, n);
    a.struct_size = sizeof(a);
    /* (a NaN fails every comparison) */
    if (!(a.beta_1 >= 0.0f && a.beta_1 < 1.0f) || !(a.beta_2 >= 0.0f && a.beta_2 < 1.0f))
      throw CaError(CA_ERR_ARG, "ca_fitter_set_adam: beta_1 and beta_2 must lie in [0, 1)");
    if (!(a.epsilon > 0.0f) || a.epsilon == INFINITY) throw CaError(CA_ERR_ARG, "ca_fitter_set_adam: epsilon must be finite and > 0");
    if (!(a.ema_momentum >= 0.0f && a.ema_momentum < 1.0f)) throw CaError(CA_ERR_ARG, "ca_fitter_set_adam: ema_momentum must lie in [0, 1)");
    if (a.ema_overwrite_frequency < 0 || (a.ema_overwrite_frequency > 0 && !(a.ema_momentum > 0.0f)))
      throw CaError(CA_ERR_ARG, "ca_fitter_set_adam: ema_overwrite_frequency must be >= 0, and > 0 only with ema_momentum > 0");
    a.amsgrad = a.amsgrad != 0;
    f->adam = a;
  });
}

extern "C" int ca_fitter_get_adam(ca_fitter *f, ca_fit_adam *out) {
  return co_guard(f, [&] {
    if (!out || out->struct_size < sizeof(uint32_t)) throw CaError(CA_ERR_ARG, "ca_fitter_get_adam: null, or a struct_size below 4");
    ca_fit_adam a = f->adam;
    a.struct_size = (uint32_t)(out->struct_size < sizeof(a) ? out->struct_size : sizeof(a));
    memcpy(out, &a, a.struct_size);
  });
}

static void ft_check_slot(ca_fitter *f, int32_t which, const void *values, size_t n_floats) {
  if (which != CA_SLOT_VHAT && which != CA_SLOT_AVERAGE) throw CaError(CA_ERR_ARG, "ca_fitter: the slot must be CA_SLOT_VHAT or CA_SLOT_AVERAGE");
  if (!values) throw CaError(CA_ERR_ARG, "ca_fitter: null slot values");
  f->check_n(n_floats);
}

extern "C" int ca_fitter_set_slot(ca_fitter *f, int32_t which, const float *values, size_t n_floats) {
  return co_guard(f, [&] {
    ft_check_slot(f, which, values, n_floats);
    DevBuf<float> &b = which == CA_SLOT_VHAT ? f->vhat : f->avg;
    if (!b.p) b.alloc(f->nw, f->s);
    rt_h2d(b.p, values, f->nw * sizeof(float), f->s);
    rt_sync(f->s);
    if (which == CA_SLOT_AVERAGE) f->avg_valid = true;
  });
}

extern "C" int ca_fitter_get_slot(ca_fitter *f, int32_t which, float *values, size_t n_floats) {
  return co_guard(f, [&] {
    ft_check_slot(f, which, values, n_floats);
    if (which == CA_SLOT_AVERAGE) f->need_average("ca_fitter_get_slot");
    const DevBuf<float> &b = which == CA_SLOT_VHAT ? f->vhat : f->avg;
    if (!b.p) { /* a third slot that no step has used yet */
      for (int i = 0; i < f->nw; ++i) values[i] = 0.0f;
      return;
    }
    rt_d2h(values, b.p, f->nw * sizeof(float), f->s);
    rt_sync(f->s);
  });
}

extern "C" int ca_fitter_swap_average(ca_fitter *f) {
  return co_guard(f, [&] {
    f->need_average("ca_fitter_swap_average");
    RT_LAUNCH(ft_k_average_swap, (f->nw + 255) / 256, 256, f->s, f->w.p, f->avg.p, f->nw);
  });
}

extern "C" int ca_fitter_apply_average(ca_fitter *f) {
  return co_guard(f, [&] {
    f->need_average("ca_fitter_apply_average");
    RT_LAUNCH(ft_k_average_apply, (f->nw + 255) / 256, 256, f->s, f->w.p, (const float *)f->avg.p, (const int32_t *)f->sidx.p,
              f->nw);
  });
}

/* ------------------------------------------------------------------ loss, metrics, predict */
extern "C" int ca_fitter_set_loss(ca_fitter *f, const ca_fit_loss *loss) {
  return co_guard(f, [&] {
    if (!loss || loss->struct_size < sizeof(uint32_t)) throw CaError(CA_ERR_ARG, "ca_fitter_set_loss: null, or a struct_size below 4");
    ca_fit_loss l = CA_FIT_LOSS_INIT; /* the defaults for what the caller's struct does not have */
    const size_t n = loss->struct_size < sizeof(l) ? loss->struct_size : sizeof(l);
    memcpy(&l, loss, n);
    l.struct_size = sizeof(l);
    /* (a NaN fails every comparison) */
    if (!(l.value_weight >= 0.0f) || l.value_weight == INFINITY || !(l.policy_weight >= 0.0f) || l.policy_weight == INFINITY)
      throw CaError(CA_ERR_ARG, "ca_fitter_set_loss: value_weight and policy_weight must be finite and >= 0");
    if (l.value_weight == 0.0f && l.policy_weight == 0.0f)
      throw CaError(CA_ERR_ARG, "ca_fitter_set_loss: value_weight and policy_weight may not both be 0");
    if (!(l.label_smoothing >= 0.0f && l.label_smoothing < 1.0f))
      throw CaError(CA_ERR_ARG, "ca_fitter_set_loss: label_smoothing must lie in [0, 1)");
    if (l.value_loss != CA_VALUE_LOSS_MSE && l.value_loss != CA_VALUE_LOSS_HUBER)
      throw CaError(CA_ERR_ARG, "ca_fitter_set_loss: value_loss must be CA_VALUE_LOSS_MSE or CA_VALUE_LOSS_HUBER");
    if (!(l.huber_delta > 0.0f) || l.huber_delta == INFINITY)
      throw CaError(CA_ERR_ARG, "ca_fitter_set_loss: huber_delta must be finite and > 0");
    f->lossopt = l;
  });
}

extern "C" int ca_fitter_get_loss(ca_fitter *f, ca_fit_loss *out) {
  return co_guard(f, [&] {
    if (!out || out->struct_size < sizeof(uint32_t)) throw CaError(CA_ERR_ARG, "ca_fitter_get_loss: null, or a struct_size below 4");
    ca_fit_loss l = f->lossopt;
    l.struct_size = (uint32_t)(out->struct_size < sizeof(l) ? out->struct_size : sizeof(l));
    memcpy(out, &l, l.struct_size);
  });
}

extern "C" int ca_fitter_set_metrics(ca_fitter *f, int32_t on, int32_t top_k) {
  return co_guard(f, [&] {
    if (on && (top_k < 1 || top_k > CA_NUM_MOVES)) throw CaError(CA_ERR_ARG, "ca_fitter_set_metrics: top_k must be in 1..96");
    if (on) f->top_k = top_k;
    f->metrics_on = on != 0;
    f->lastm = ca_fit_metrics{sizeof(ca_fit_metrics), f->top_k, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  });
}

extern "C" int ca_fitter_metrics(ca_fitter *f, ca_fit_metrics *out) {
  return co_guard(f, [&] {
    if (!out || out->struct_size < sizeof(uint32_t)) throw CaError(CA_ERR_ARG, "ca_fitter_metrics: null, or a struct_size below 4");
    if (!f->metrics_on) throw CaError(CA_ERR_STATE, "ca_fitter_metrics: metrics are off (ca_fitter_set_metrics)");
    ca_fit_metrics m = f->lastm;
    m.struct_size = (uint32_t)(out->struct_size < sizeof(m) ? out->struct_size : sizeof(m));
    memcpy(out, &m, m.struct_size);
  });
}

extern "C" int ca_fitter_predict(ca_fitter *f, const int32_t *rows, int32_t n_rows, int32_t train, float *logits,
                                 float *values) {
  return co_guard(f, [&] {
    f->need_data();
    if (!rows || !logits || !values) throw CaError(CA_ERR_ARG, "ca_fitter_predict: null argument");
    f->check_batch(n_rows);
    f->check_rows(rows, n_rows);
    f->need_idx(n_rows);
    rt_h2d(f->idx.p, rows, (size_t)n_rows * sizeof(int32_t), f->s);
    const ca_fitter::Batch bt = f->batch(f->idx.p, n_rows);
    f->net->forward(f->shared(bt), bt.rows, n_rows, train != 0);
    std::vector<float> hh((size_t)n_rows * FT_PADW);
    rt_d2h(hh.data(), f->h.p, hh.size() * sizeof(float), f->s);
    rt_sync(f->s);
    for (int32_t r = 0; r < n_rows; ++r) {
      memcpy(logits + (size_t)r * CA_NUM_MOVES, hh.data() + (size_t)r * FT_PADW, CA_NUM_MOVES * sizeof(float));
      values[r] = hh[(size_t)r * FT_PADW + CA_NUM_MOVES];
    }
  });
}

extern "C" int ca_fitter_tensor_table(ca_fitter *f, int32_t *out, int32_t cap, int32_t *count) {
  return co_guard(f, [&] {
    if (!count || cap < 0 || (cap > 0 && !out)) throw CaError(CA_ERR_ARG, "ca_fitter_tensor_table: null output or negative cap");
    std::vector<FtTensor> tt;
    f->net->tensor_table(tt);
    *count = (int32_t)tt.size();
    for (int32_t k = 0; k < cap && k < *count; ++k) out[3 * k] = tt[k].off, out[3 * k + 1] = tt[k].count, out[3 * k + 2] = tt[k].cls;
  });
}
