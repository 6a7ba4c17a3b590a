// nn_train.h -- what the training sources share ("Network training"): the fitter's step driver
// (nn_train.hip) sees a network as an FtNet, one class per network next to its kernels (FtMlp in nn_train_mlp.hip,
// FtResCnn in nn_train_conv.hip), and both networks are built from the strided GEMM and the column kernels declared
// here.  The fitter itself is made of three parts that own their state, each declared here and defined next to its
// kernels: the data set (FtData, nn_train_data.hip), the loss and what a call reports (FtLoss, nn_train_loss.hip), the
// end of a step (FtStepEnd with the fit options' FtOpt, nn_train_opt.hip).  Also here: the readers and writers of the C
// ABI's size-prefixed structs.
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
                          ft_k_assemble wrote from a packed one (nn_train_data.hip) */
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

/* ---- What the C ABI's entry points share.  Finite and >= 0 (a NaN fails the first comparison): */
inline bool ft_finite_nonneg(float x) { return x >= 0.0f && x != INFINITY; }

/* A caller's size-prefixed struct (corintho_hip.h): one built against an earlier header is shorter than today's.
 * ft_struct_in: its struct_size bytes, at most sizeof(T), over the defaults v.  ft_struct_out: as many bytes of v as the
 * caller has room for, and that count as its size. */
template <class T>
void ft_struct_check(const T *p, const char *who) {
  if (!p || p->struct_size < sizeof(uint32_t)) throw CaError(CA_ERR_ARG, std::string(who) + ": null, or a struct_size below 4");
}
template <class T>
T ft_struct_in(const T *in, T v, const char *who) {
  ft_struct_check(in, who);
  memcpy(&v, in, in->struct_size < sizeof(T) ? in->struct_size : sizeof(T));
  v.struct_size = sizeof(T);
  return v;
}
template <class T>
void ft_struct_out(T *out, T v, const char *who) {
  ft_struct_check(out, who);
  v.struct_size = (uint32_t)(out->struct_size < sizeof(T) ? out->struct_size : sizeof(T));
  memcpy(out, &v, v.struct_size);
}

/* ---- The data set (nn_train_data.hip).  What the kernels of a step read a batch through: row indices into three arrays */
struct FtBatch {
  const int32_t *rows;
  const float *states, *evals, *probs;
  const float *wts; /* null: an unweighted set */
};
/* the batches of a call on n_rows rows (a device pointer): `batch` rows each, the last one what is left */
struct FtBatches {
  const int32_t *rows;
  int32_t n_rows, batch;
  int nb;
  bool metrics; /* the call reports metrics as well */
  int size(int b) const { return b * batch + batch <= n_rows ? batch : n_rows - b * batch; }
  const int32_t *at(int b) const { return rows + (size_t)b * batch; }
};

/* Merging of a packed set's duplicate positions on the device (nn_samples.hip; the definition: ca_fitter_merge_duplicates
 * in corintho_hip.h).  sp[n][166], oc[n] and wt[n] (null: every weight 1) are read only; the merged samples come back in
 * buffers of their own with room for `cap` samples, of which `count` are filled.  Everything is queued on s, which is
 * synchronised on return. */
struct FtMerged {
  DevBuf<float> sp, oc, wt;
  int32_t count = 0, cap = 0;
};
FtMerged ft_merge_duplicates(rt_stream_t s, const float *sp, const float *oc, const float *wt, int32_t n, bool normalize);
/* The n samples of sp[n][166] brought into their canonical orientation in place (nn_samples.hip; the definition:
 * ca_fitter_canonicalize in corintho_hip.h).  Returns how many changed their orientation; s is synchronised on return. */
int32_t ft_canonicalize(rt_stream_t s, float *sp, int32_t n);

#define FT_SAMPLE_FLOATS (CA_GAME_STATE_SIZE + CA_NUM_MOVES) /* a packed row: state[70], policy[96] */
typedef void (*FtCopy)(void *, const void *, size_t, rt_stream_t); /* rt_h2d or rt_d2d */

/* The data set in either form, its sample weights, the rows of a call and the staging buffers of an assembled batch.
 * Nothing outside writes its counts or its form. */
struct FtData {
  void init(int32_t mb, rt_stream_t stream) { max_batch = mb, s = stream; }
  int32_t rows() const { return n; }                    /* addressable rows: 8 per sample of a packed set */
  int32_t samples() const { return expanded ? 0 : ns; } /* packed samples */
  void need_data() const;
  void check_batch(int32_t batch) const;
  void check_rows(const int32_t *rows, int32_t nr) const; /* nr <= n, every index in range */
  void need_idx(int32_t nr);                              /* room on the device for the nr rows of a call ... */
  const int32_t *upload(const int32_t *rows, int32_t nr); /* ... and the rows queued to it */
  /* the batch of rows[0..B) (a device pointer): the expanded set itself, or a packed set's rows assembled */
  FtBatch batch(const int32_t *rows, int B);
  void clear();
  void set_expanded(const float *st, const float *ev, const float *pr, int32_t count); /* ca_fitter_set_data */
  /* room for `add` more packed samples behind the ns there are (capacity grows geometrically); where they go, how many
   * fit, and that `add` of them have arrived */
  void reserve(int32_t add);
  float *sp_end() { return sp.p + (size_t)ns * FT_SAMPLE_FLOATS; }
  float *oc_end() { return oc.p + ns; }
  int32_t room() const { return cap - ns; }
  void added(int32_t add) { ns += add, n = ns * CA_NUM_SYMMETRIES; }
  void add(const float *state_policy, const float *outcome, int32_t count, FtCopy copy); /* all four, and the copy */
  void drop(int32_t n_oldest);                                  /* ca_fitter_drop_samples */
  void merge(bool normalize, int32_t *before, int32_t *after);  /* ca_fitter_merge_duplicates */
  void canonicalize(int32_t *moved);                            /* ca_fitter_canonicalize */
  void set_augmentation(int32_t a);                             /* ca_fitter_set_augmentation: CA_AUG_* */
  int32_t augmentation() const { return aug; }
  void set_weights(const float *weights, int32_t count);        /* ca_fitter_set_sample_weights */
  void get_weights(float *out, int32_t count);
  void fetch_rows(const int32_t *rows, int32_t n_rows, float *st, float *ev, float *pr);

 private:
  rt_stream_t s = nullptr;
  int32_t max_batch = 0;
  int32_t n = 0, idx_cap = 0; /* addressable rows (8 * ns of a packed set); rows idx holds */
  bool expanded = false;      /* the form: set by set_expanded, until clear */
  int32_t ns = 0, cap = 0;    /* packed samples, and how many sp and oc have room for */
  bool weighted = false;      /* set_weights, merge; until clear */
  int32_t aug = CA_AUG_REFERENCE; /* which move table a packed set's virtual rows go through; the fitter's, not the set's */
  DevBuf<float> states, evals, probs;          /* the expanded set */
  DevBuf<float> sp, oc;                        /* the packed set: state_policy[cap][166], outcome[cap] */
  DevBuf<float> wt;                            /* when `weighted`: [n] of an expanded set, [cap] beside sp and oc */
  DevBuf<float> bstates, bevals, bprobs, bwts; /* one batch as ft_k_assemble wrote it: max_batch rows */
  DevBuf<int32_t> idx, ident, bidx;            /* ident[r] = r, the rows of an assembled batch; bidx: fetch_rows */
  int32_t units() const { return expanded ? n : ns; } /* what a sample weight belongs to */
  void check_range(const int32_t *rows, int32_t nr) const;
  void need_stage();
  void assemble(const int32_t *rows, int B);
  void move_samples(int32_t first, int32_t count, int32_t new_cap);
  void slide_samples(int32_t first, int32_t count);
};

/* ---- The step with fit options (nn_train_opt.hip; the definition: corintho_hip.h, "fit options").  The weight vector is
 * cut into PIECES of at most 256 floats of one tensor; a workgroup owns a piece.  A step is three launches on the summed
 * gradient ft_k_update(apply = 0) left in gsum: the regulariser gradient added and per-piece float64 partials of
 * sum g'^2, R and the count of |g'| > clipvalue (ft_k_opt_partials); the partials combined by a tree of fixed shape
 * into the tensors' scales, the step's R and the call's statistics (ft_k_opt_combine); the clamp or scale, the decay,
 * Adam and the moving statistics (ft_k_opt_update; with Adam's arguments off their defaults ft_k_opt_update_adam). */
struct FtOptStats { /* accumulated on the device over the steps of one ca_fitter_train */
  double reg_sum, norm_sum, norm_max, clipped;
};
inline bool ft_regularized(const ca_fit_options &o) { return o.l1 > 0.0f || o.l2 > 0.0f; }
inline bool ft_options_on(const ca_fit_options &o) {
  return ft_regularized(o) || o.weight_decay > 0.0f || o.clipvalue > 0.0f || o.clipnorm > 0.0f || o.global_clipnorm > 0.0f;
}
struct FtOpt {
  ca_fit_options o = {};
  int nt = 0, npieces = 0;
  DevBuf<int32_t> pieces, tfirst; /* [npieces][4] = {offset, floats, tensor, class}; [nt + 1]: a tensor's first piece */
  DevBuf<double> part;            /* [npieces][3] */
  DevBuf<float> scale;            /* [nt] */
  DevBuf<double> out;             /* the statistics (4 doubles), then R of every batch of the call */
  size_t slots = 0;
  std::vector<double> hout;

  /* the piece table of a network's tensors; once */
  void plan(const std::vector<FtTensor> &tensors, int nw, rt_stream_t s);
  /* room for the R of `n` batches; clears the statistics */
  void begin(int n, rt_stream_t s);
  /* R(w) to slot `slot`; nothing else is read or written */
  void regularization(rt_stream_t s, const float *w, int slot);
  /* step 1 on gsum and the tensors' scales; R to slot, the statistics accumulated */
  void reduce(rt_stream_t s, const float *w, float *gsum, int slot);
  /* queues the copy of the statistics and the first n R to hout; valid after the stream is synchronised */
  void fetch(int n, rt_stream_t s);
  double R(int slot) const { return hout[4 + slot]; }
};
/* which regulariser terms a call's losses carry: none, R of every batch (ca_fitter_train: the weights move), or one R
 * for the call (ca_fitter_evaluate) */
enum class FtReg { none, per_batch, once };

/* ---- The loss and what a call reports (nn_train_loss.hip; the definition: corintho_hip.h, "loss and metrics").  Every
 * loss kernel reads a batch alike: H[B][FT_PADW], the labels through rows[r], wts null on an unweighted set. */
struct FtLossArgs {
  float value_weight, policy_weight, label_smoothing, huber_delta;
  int huber;
};
#define FT_METRIC_W 8 /* floats of a row's and of a batch's metric terms: the five sums of w x, the sum of w, two spare */
struct FtLoss {
  ca_fit_loss args = CA_FIT_LOSS_INIT; /* at its defaults a step launches ft_k_loss and no other loss kernel */
  bool metrics_on = false;             /* set_metrics; off: the metrics' buffers have no memory */
  ca_fit_metrics lastm = {sizeof(ca_fit_metrics), 5, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; /* of the last train or evaluate */

  void set_metrics(bool on, int32_t k);
  /* the loss buffers, and with `metrics` the metrics', of a call of `slots` batches of at most max_batch rows */
  void ensure(int slots, bool metrics, int32_t max_batch, rt_stream_t s);
  /* loss terms of the batch in sh.h (and the logit / value gradients in sh.hd; grads: the head biases' to sh.g as well);
   * the loss sums to slot.  The one place that chooses among ft_k_loss, ft_k_loss<weighted> and ft_k_loss_opt */
  void terms(const FtShared &sh, const FtNet &net, const FtBatch &b, int B, bool grads, int slot);
  /* the batch's metric sums to slot, from the H the loss kernel reads */
  void metric_terms(const FtShared &sh, const FtBatch &b, int B, int slot);
  /* per-batch sums -> out[3] = {value_weight value + policy_weight policy, value, policy}, means weighted by batch size;
   * per[3 * b]; reg: with the regulariser's R, which opt holds, added to the totals.  The options' buffer and the
   * batches' metric sums come back in the same synchronisation */
  void losses(rt_stream_t s, const FtBatches &bs, double *out, float *per, FtReg reg, FtOpt &opt);

 private:
  int32_t top_k = 5;
  DevBuf<float> loss, mrow, metric; /* [slots][2]; a batch's rows' metric terms [max_batch][8]; the batches' sums [slots][8] */
  std::vector<float> hloss, hmetric;
  bool is_default() const;
  void metrics_of(int nb, int32_t nr);
};

/* ---- The end of a step (nn_train_opt.hip).  Adam's arguments as the update kernels take them (the definition:
 * corintho_hip.h, "Adam's arguments") */
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

/* the fitter's buffers that the end of a step works on */
struct FtWeights {
  float *w, *m, *v, *g, *gsum; /* [nw] each, g [FT_NSPLIT][nw] */
  const int32_t *sidx;         /* FtNet::update_table on the device */
  const float *stat;
  int nw;
};
/* Adam's arguments with the third slot and the average, the fit options and the statistics of a call's steps */
struct FtStepEnd {
  ca_fit_adam adam = CA_FIT_ADAM_INIT; /* at their defaults a step never looks at the third slot or the average */
  FtOpt opt;                           /* the fit options; all 0: never touched by a step */
  ca_fit_stats last = {sizeof(ca_fit_stats), 0, 0, 0, 0.0, 0.0, 0.0}; /* of the last ca_fitter_train */

  void init(const FtWeights &weights, rt_stream_t stream) { W = weights, s = stream; }
  /* the piece table of the options' kernels, made when options are first switched on */
  void plan_options(const FtNet &net);
  /* a ca_fitter_train of nb steps: before the first, and once the losses and the options' statistics are on the host */
  FtReg begin(int nb);
  void finish(int nb);
  /* The end of step number `step` on the partials that backward left, ns of them: Adam at learning rate lr and the
   * moving statistics; the options' R to slot.  The one place that chooses among the four update kernels. */
  void step(FtSplits ns, float lr, int64_t step, int slot);
  void sum_gradient(FtSplits ns); /* the summed gradient to gsum, nothing else: ca_fitter_gradients */
  FtReg begin_evaluate();         /* with a regulariser: one R for the call, since the weights do not move */
  void weights_replaced() { avg_valid = false; } /* ca_fitter_set_weights */
  void slots_replaced();                         /* ca_fitter_set_optimizer: the third slot starts again from 0 */
  void set_slot(int32_t which, const float *values);
  void get_slot(int32_t which, float *values);
  void swap_average(); /* w <-> the average */
  void apply_average(); /* w := the average on the trainable weights */

 private:
  FtWeights W = {};
  rt_stream_t s = nullptr;
  DevBuf<float> vhat, avg; /* the third slot and the average: no memory before their first use */
  bool avg_valid = false;  /* until ca_fitter_set_weights */
  bool adam_default() const;
  FtAdamArgs adam_args(int64_t step);
  void need_average(const char *who) const;
};

/* kind: CA_NET_MLP12X100 or CA_NET_RESCNN4; the network's own buffers are sized for max_batch rows and cleared on s */
FtNet *ft_net_create(int kind, int max_batch, rt_stream_t s);
FtNet *ft_mlp_create(int max_batch, rt_stream_t s);
FtNet *ft_rescnn_create(int max_batch, rt_stream_t s);
