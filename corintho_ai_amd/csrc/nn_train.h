// nn_train.h -- what the training sources share ("Network training"): the fitter's step driver
// (nn_train.hip) sees a network as an FtNet, one class per network next to its kernels (FtMlp in nn_train_mlp.hip,
// FtResCnn in nn_train_conv.hip), and both networks are built from the strided GEMM and the column kernels declared
// here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "host.h"

#define FT_PADW 112  /* row stride of the heads' outputs H and their gradients Hd (and of the MLP's activations): 7 tiles of 16 */
#define FT_NSPLIT 16 /* at most this many row chunks per weight gradient (partials of ft_k_gemm) */
#define FT_BN_RG 64  /* row groups of the column kernels: 16 features x 64 = 1024 threads */
/* ft_k_update's code of a trainable weight: how many gradient partials it has (FtSplits::rows, ::pixels, or one).  A code
 * >= 0 is a moving statistic and indexes the batch statistic it follows. */
#define FT_SPLIT0 -1
#define FT_SPLIT1 -2
#define FT_WHOLE -3

/* C[m][n] (+)= sum_k A[m][k] B[k][n] over one chunk of k, every operand addressed through strides (so a transpose is
 * free).  One wave per 16x16 output tile and chunk; chunk s writes C + s * c_split.  Loads outside [0,M) x [k0,k1) and
 * [k0,k1) x [0,N) are zero and only the M x N block is written. */
struct FtGemm {
  const float *A;
  long sam, sak;
  const float *B;
  long sbk, sbn;
  float *C;
  long scm, scn, c_split;
  int M, N, K, kchunk;
  const float *bias; /* per column n, or null */
  int relu, accumulate;
};
void ft_gemm(rt_stream_t s, const FtGemm &a);
/* the whole of k in one chunk, no bias, no ReLU, C overwritten */
inline FtGemm mk(const float *A, long sam, long sak, const float *B, long sbk, long sbn, float *C, long scm, long scn, int M,
                 int N, int K) {
  FtGemm a;
  a.A = A, a.sam = sam, a.sak = sak, a.B = B, a.sbk = sbk, a.sbn = sbn, a.C = C, a.scm = scm, a.scn = scn;
  a.c_split = 0, a.M = M, a.N = N, a.K = K, a.kchunk = K > 0 ? K : 1, a.bias = nullptr, a.relu = 0, a.accumulate = 0;
  return a;
}
/* rows of one of at most FT_NSPLIT chunks of K, a multiple of 16 */
inline int ft_split_chunk(int K) { return ((K + FT_NSPLIT - 1) / FT_NSPLIT + 15) / 16 * 16; }

/* ReLU backward of a dense layer's output A[B][ld] in place on dA, and the column sums of the result (the layer's bias
 * gradient) to gbias[0..ncol): ft_k_relu_bwd */
void ft_relu_bwd(rt_stream_t s, float *dA, const float *A, int B, int ld, int ncol, float *gbias);

/* Fixed-order sum of the 64 row-group partials of each of the block's 16 features: red[rg][f] -> returned to every
 * thread of feature f.  Leaves red free for the next use. */
__device__ __forceinline__ float ft_colsum(float *red, float v) {
  const int f = threadIdx.x & 15, rg = threadIdx.x >> 4;
  __syncthreads();
  red[rg * 16 + f] = v;
  __syncthreads();
  if (rg == 0) {
    float s = 0.0f;
    for (int j = 0; j < FT_BN_RG; ++j) s += red[j * 16 + f];
    red[FT_BN_RG * 16 + f] = s;
  }
  __syncthreads();
  return red[FT_BN_RG * 16 + f];
}

/* what a network's step reads and writes but does not own */
struct FtShared {
  rt_stream_t s;
  float *w;     /* the weights, in the network's flat layout */
  float *g;     /* gradient partials [FT_NSPLIT][num_weights] */
  float *stat;  /* batch statistics [stat_floats], where update_table's codes point */
  float *h;     /* the heads' outputs [B][FT_PADW]: 96 logits, the value at 96 */
  float *hd;    /* their gradients, from ft_k_loss */
  const float *states; /* the game states [n][70] that forward's rows index: the expanded data set's, or the batch that
                          ft_k_assemble wrote from a packed one (nn_train.hip) */
};

/* how many partials in g backward left for a weight whose gradient is a sum over the B rows (FT_SPLIT0) and over the
 * B * 16 (row, pixel) pairs (FT_SPLIT1) */
struct FtSplits {
  int rows, pixels;
};

/* a contiguous range of the flat weight vector and its class (CA_TENSOR_* of corintho_hip.h, "fit options") */
struct FtTensor {
  int32_t off, count, cls;
};

struct FtNet {
  virtual ~FtNet() {}
  virtual const char *name() const = 0;
  virtual int num_weights() const = 0;
  virtual size_t stat_floats() const = 0;
  /* where ft_k_head_reduce writes the gradients of the heads' last biases */
  virtual int policy_bias() const = 0;
  virtual int value_bias() const = 0;
  /* ft_k_update's code of every weight: sidx has num_weights entries */
  virtual void update_table(std::vector<int32_t> &sidx) const = 0;
  /* the network's tensors in the order of the weight vector: together they cover it without a gap */
  virtual void tensor_table(std::vector<FtTensor> &tensors) const = 0;
  /* forward of rows[0..B) (a device pointer) of the data set; train = batch statistics (left in stat), else the moving
   * ones.  Leaves h. */
  virtual void forward(const FtShared &sh, const int32_t *rows, int B, bool train) = 0;
  /* from hd and what forward kept: the weight gradient of the batch as partials in g (the heads' last biases excepted) */
  virtual FtSplits backward(const FtShared &sh, int B) = 0;
};
/* Adam's arguments as the update kernels take them (the definition: corintho_hip.h, "Adam's arguments") */
struct FtAdamArgs {
  float beta_1, beta_2, epsilon, ema_momentum;
  float *h;      /* the third slot ("vhat"); null: amsgrad is off */
  float *a;      /* the average; null: ema_momentum is 0 */
  int overwrite; /* this step brings the step count to a multiple of ema_overwrite_frequency: w := a' */
};

/* Adam on trainable weight i: gradient s (g''), wv the weight the step starts from (w').  Both update kernels, with and
 * without fit options, end in this one expression.  PARAM = false: the Adam defaults as literals and neither the third
 * slot nor the average; A is not looked at, and the code is what the kernels held before Adam had arguments. */
template <bool PARAM>
__device__ __forceinline__ void ft_adam(float *__restrict__ w, float *__restrict__ m, float *__restrict__ v, int i,
                                        float wv, float s, float lr_t, const FtAdamArgs &A) {
  const float b1 = PARAM ? A.beta_1 : 0.9f, b2 = PARAM ? A.beta_2 : 0.999f, eps = PARAM ? A.epsilon : 1e-7f;
  const float mt = m[i] + (s - m[i]) * (1.0f - b1);
  const float vt = v[i] + (s * s - v[i]) * (1.0f - b2);
  m[i] = mt;
  v[i] = vt;
  float d = vt;
  if (PARAM && A.h) {
    const float hv = A.h[i];
    d = hv > vt ? hv : vt;
    A.h[i] = d;
  }
  float wn = wv - lr_t * mt / (sqrtf(d) + eps);
  if (PARAM && A.a) {
    const float av = A.a[i];
    const float an = av + (wn - av) * (1.0f - A.ema_momentum);
    A.a[i] = an;
    if (A.overwrite) wn = an;
  }
  w[i] = wn;
}

/* Merging of a packed set's duplicate positions on the device (nn_samples.hip; the definition: ca_fitter_merge_duplicates
 * in corintho_hip.h).  sp[n][166], oc[n] and wt[n] (null: every weight 1) are read only; the merged samples come back in
 * buffers of their own with room for `cap` samples, of which `count` are filled.  Everything is queued on s, which is
 * synchronised on return. */
struct FtMerged {
  DevBuf<float> sp, oc, wt;
  int32_t count = 0, cap = 0;
};
FtMerged ft_merge_duplicates(rt_stream_t s, const float *sp, const float *oc, const float *wt, int32_t n, bool normalize);

/* The step with fit options (nn_train_opt.hip; the definition: corintho_hip.h, "fit options").  The weight vector is cut
 * into PIECES of at most 256 floats of one tensor; a workgroup owns a piece.  A step is three launches on the summed
 * gradient ft_k_update(apply = 0) left in gsum: the regulariser gradient added and per-piece float64 partials of
 * sum g'^2, R and the count of |g'| > clipvalue (ft_k_opt_partials); the partials combined by a tree of fixed shape
 * into the tensors' scales, the step's R and the call's statistics (ft_k_opt_combine); the clamp or scale, the decay,
 * Adam and the moving statistics (ft_k_opt_update; with Adam's arguments off their defaults ft_k_opt_update_adam). */
struct FtOptStats { /* accumulated on the device over the steps of one ca_fitter_train */
  double reg_sum, norm_sum, norm_max, clipped;
};
struct FtOpt {
  ca_fit_options o = {};
  int nt = 0, npieces = 0;
  DevBuf<int32_t> pieces, tfirst; /* [npieces][4] = {offset, floats, tensor, class}; [nt + 1]: a tensor's first piece */
  DevBuf<double> part;            /* [npieces][3] */
  DevBuf<float> scale;            /* [nt] */
  DevBuf<double> out;             /* the statistics (4 doubles), then R of every batch of the call */
  size_t slots = 0;
  std::vector<double> hout;

  bool regularized() const { return o.l1 > 0.0f || o.l2 > 0.0f; }
  bool on() const { return regularized() || o.weight_decay > 0.0f || o.clipvalue > 0.0f || o.clipnorm > 0.0f || o.global_clipnorm > 0.0f; }
  /* the piece table of a network's tensors; once */
  void plan(const std::vector<FtTensor> &tensors, int nw, rt_stream_t s);
  /* room for the R of `n` batches; clears the statistics */
  void begin(int n, rt_stream_t s);
  /* R(w) to slot `slot`; nothing else is read or written */
  void regularization(rt_stream_t s, const float *w, int slot);
  /* steps 1 to 4 on gsum; R to slot, the statistics accumulated.  adam: null, the Adam defaults (ft_k_opt_update), or
   * the arguments of ft_k_opt_update_adam */
  void step(rt_stream_t s, float *w, float *m, float *v, float *gsum, const int32_t *sidx, const float *stat, float lr,
            float lr_t, int slot, const FtAdamArgs *adam);
  /* queues the copy of the statistics and the first n R to hout; valid after the stream is synchronised */
  void fetch(int n, rt_stream_t s);
  double R(int slot) const { return hout[4 + slot]; }
};

/* The loss off its defaults and the metrics (nn_train_loss.hip; the definition: corintho_hip.h, "loss and metrics").
 * Both read a batch as ft_k_loss does: H[B][FT_PADW], the labels through rows[r], wts null on an unweighted set. */
struct FtLossArgs {
  float value_weight, policy_weight, label_smoothing, huber_delta;
  int huber;
};
#define FT_METRIC_W 8 /* floats of a row's and of a batch's metric terms: the five sums of w x, the sum of w, two spare */
/* ft_k_loss's work with the arguments L: Hd[B][FT_PADW], for ft_k_head_reduce as ft_k_loss leaves it */
void ft_loss_opt(rt_stream_t s, const float *H, const int32_t *rows, int B, const float *evals, const float *probs,
                 float *Hd, const float *wts, const FtLossArgs &L);
/* the rows' metric terms to mrow[B][FT_METRIC_W], and their column sums in a fixed order to out[FT_METRIC_W] */
void ft_metrics(rt_stream_t s, const float *H, const int32_t *rows, int B, const float *evals, const float *probs,
                const float *wts, int top_k, float *mrow, float *out);

/* kind: CA_NET_MLP12X100 or CA_NET_RESCNN4; the network's own buffers are sized for max_batch rows and cleared on s */
FtNet *ft_net_create(int kind, int max_batch, rt_stream_t s);
FtNet *ft_mlp_create(int max_batch, rt_stream_t s);
FtNet *ft_rescnn_create(int max_batch, rt_stream_t s);
