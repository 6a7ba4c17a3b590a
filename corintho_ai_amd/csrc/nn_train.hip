// nn_train.hip -- network training: the reference's Keras fit step (main.pyx:221-272) in float32 on the fp32 matrix
// pipe (v_mfma_f32_16x16x4_f32).  This file holds what every network shares (the strided GEMM ft_k_gemm and the column
// kernel ft_k_relu_bwd), the fitter as a composition of its parts, and the C ABI.  A network is an FtNet (nn_train.h):
// mlp12x100, the reference's model (wrapper.py:256-282), in nn_train_mlp.hip and rescnn4, the network of nets.py, in
// nn_train_conv.hip.  The parts: the data set in nn_train_data.hip, the loss and what a call reports in
// nn_train_loss.hip, the end of a step in nn_train_opt.hip.
//
// One training step of a batch of B rows ("Network training"):
//   batch       FtData::batch: the rows of an expanded set as they are; of a packed set assembled (ft_k_assemble)
//   forward     FtNet::forward: the batch's rows -> the heads' outputs H (96 logits and the value per row)
//   loss        FtLoss::terms: per row (tanh v - z)^2, -sum t log_softmax, and their gradients (ft_k_loss; off the
//               default loss ft_k_loss_opt in its place); column sums of the head gradients and of the loss terms
//               (ft_k_head_reduce)                                                             2 launches
//               (with metrics on FtLoss::metric_terms, two launches more, which read H and touch nothing a step uses)
//   backward    FtNet::backward: the weight gradient as partials, and how many of them a weight has
//   update      FtStepEnd::step: sum of the split partials in a fixed order, Adam (TF ResourceApplyAdam) on kernels,
//               biases, gamma and beta, moving statistics from the batch statistics (ft_k_update)  1 launch
//               (off Adam's defaults ft_k_update_adam; with fit options four launches)
// Every cross-workgroup sum is written as partials and combined in a fixed order by a later launch: no float atomics,
// no grid-wide barriers, so a step is bitwise reproducible.
#include <math.h>

#include <memory>

#include "nn_train.h"

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

/* The fitter: the network, the stream, the weights with Adam's two slots, the gradient and the heads' buffers -- and the
 * three parts, each of which owns the rest of its state (nn_train.h). */
struct ca_fitter {
  int device = 0;
  int nw = 0; /* floats of the weight vector */
  int max_batch = 0;
  int64_t iterations = 0;
  rt_stream_t s = nullptr;
  std::unique_ptr<FtNet> net;
  int dev() const { return device; }
  DevBuf<float> w, m, v, g, gsum, stat, h, hd;
  DevBuf<int32_t> sidx;
  FtData data;   /* the data set and the rows of a call */
  FtLoss loss;   /* the loss, the metrics, what a call reports */
  FtStepEnd end; /* Adam's arguments, the fit options, the update */

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
    data.init(mb, s);
    end.init(FtWeights{w.p, m.p, v.p, g.p, gsum.p, sidx.p, stat.p, nw}, s);
  }
  ~ca_fitter() { rt_stream_destroy(s); }

  FtShared shared(const FtBatch &b) const { return FtShared{s, w.p, g.p, stat.p, h.p, hd.p, b.states}; }
  void check_n(size_t n_floats) {
    if (n_floats != (size_t)nw)
      throw CaError(CA_ERR_ARG, std::string("ca_fitter: ") + net->name() + " has " + std::to_string(nw) + " floats");
  }

  /* What ca_fitter_train, _evaluate, _gradients and _predict begin with.  The data set and the batch size are checked;
   * rows_of() makes the entry point's own checks and returns the call's rows on the host; those are checked and queued
   * to the device; a call that reports losses gets room for its batches' sums, one that may report metrics (and has
   * them switched on) for theirs.  -> the call's batches */
  enum Report { REPORT_NONE, REPORT_LOSS, REPORT_ALL };
  template <class R>
  FtBatches begin(int32_t n_rows, int32_t batch, Report report, R &&rows_of) {
    data.need_data();
    data.check_batch(batch);
    const int32_t *rows = rows_of();
    data.check_rows(rows, n_rows);
    data.need_idx(n_rows);
    const int nb = (n_rows + batch - 1) / batch;
    const bool metrics = report == REPORT_ALL && loss.metrics_on;
    if (report != REPORT_NONE) loss.ensure(nb, metrics, max_batch, s);
    return FtBatches{data.upload(rows, n_rows), n_rows, batch, nb, metrics};
  }
  /* forward and loss of batch b, the loss sums (and the call's metric sums) to slot b.  train: a training step's, on
   * batch statistics and with the head biases' gradients; else on the moving statistics */
  FtShared forward(const FtBatches &bs, int b, bool train) {
    const int B = bs.size(b);
    const FtBatch bt = data.batch(bs.at(b), B);
    const FtShared sh = shared(bt);
    net->forward(sh, bt.rows, B, train);
    loss.terms(sh, *net, bt, B, train, b);
    if (bs.metrics) loss.metric_terms(sh, bt, B, b);
    return sh;
  }
  /* ... and backward: leaves the gradient partials and returns their counts */
  FtSplits gradient(const FtBatches &bs, int b) { return net->backward(forward(bs, b, true), bs.size(b)); }
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
    f->end.weights_replaced();
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
    f->end.slots_replaced();
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
    f->data.set_expanded(states, evals, probs, n);
  });
}

extern "C" int ca_fitter_train(ca_fitter *f, const int32_t *rows, int32_t n_rows, int32_t batch, float learning_rate,
                               double *out_losses, float *batch_losses) {
  return co_guard(f, [&] {
    const FtBatches bs = f->begin(n_rows, batch, ca_fitter::REPORT_ALL, [&] {
      if (!rows || n_rows < 1) throw CaError(CA_ERR_ARG, "ca_fitter_train: no rows");
      return rows;
    });
    const FtReg reg = f->end.begin(bs.nb);
    for (int b = 0; b < bs.nb; ++b) {
      f->end.step(f->gradient(bs, b), learning_rate, f->iterations + 1, b);
      f->iterations += 1;
    }
    f->loss.losses(f->s, bs, out_losses, batch_losses, reg, f->end.opt);
    f->end.finish(bs.nb);
  });
}

extern "C" int ca_fitter_evaluate(ca_fitter *f, int32_t row0, int32_t n_rows, int32_t batch, double *out_losses) {
  return co_guard(f, [&] {
    std::vector<int32_t> rows;
    const FtBatches bs = f->begin(n_rows, batch, ca_fitter::REPORT_ALL, [&] {
      if (n_rows < 1 || row0 < 0 || (int64_t)row0 + n_rows > f->data.rows())
        throw CaError(CA_ERR_ARG, "ca_fitter_evaluate: rows out of range");
      rows.resize(n_rows);
      for (int32_t i = 0; i < n_rows; ++i) rows[i] = row0 + i;
      return rows.data();
    });
    const FtReg reg = f->end.begin_evaluate();
    for (int b = 0; b < bs.nb; ++b) f->forward(bs, b, false);
    f->loss.losses(f->s, bs, out_losses, nullptr, reg, f->end.opt);
  });
}

extern "C" int ca_fitter_gradients(ca_fitter *f, const int32_t *rows, int32_t n_rows, float *grads, double *out_losses) {
  return co_guard(f, [&] {
    const FtBatches bs = f->begin(n_rows, n_rows, ca_fitter::REPORT_LOSS, [&] {
      if (!rows || !grads) throw CaError(CA_ERR_ARG, "null argument");
      return rows;
    });
    f->end.sum_gradient(f->gradient(bs, 0));
    rt_d2h(grads, f->gsum.p, f->nw * sizeof(float), f->s);
    f->loss.losses(f->s, bs, out_losses, nullptr, FtReg::none, f->end.opt);
  });
}

extern "C" int ca_fitter_clear_data(ca_fitter *f) {
  return co_guard(f, [&] {
    rt_sync(f->s);
    f->data.clear();
  });
}

extern "C" int ca_fitter_add_samples(ca_fitter *f, const float *state_policy, const float *outcome, int32_t n) {
  return co_guard(f, [&] {
    if (!state_policy || !outcome || n < 0) throw CaError(CA_ERR_ARG, "ca_fitter_add_samples: null or negative");
    f->data.add(state_policy, outcome, n, rt_h2d);
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
    f->data.add((const float *)d_state_policy, (const float *)d_outcome, n, rt_d2d);
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
    f->data.reserve(count);
    rt_sync(f->s); /* the buffers' clears and moves are on the fitter's stream, the pack on the trainer's */
    ok(ca_trainer_pack_samples_device(t, f->data.sp_end(), f->data.oc_end(), f->data.room(), &got));
    f->data.added(got);
    *n_added = got;
  });
}

extern "C" int ca_fitter_drop_samples(ca_fitter *f, int32_t n_oldest) {
  return co_guard(f, [&] { f->data.drop(n_oldest); });
}

extern "C" int ca_fitter_data_info(ca_fitter *f, int32_t *rows, int32_t *samples) {
  return co_guard(f, [&] {
    if (!rows || !samples) throw CaError(CA_ERR_ARG, "ca_fitter_data_info: null output");
    *rows = f->data.rows();
    *samples = f->data.samples();
  });
}

extern "C" int ca_fitter_fetch_rows(ca_fitter *f, const int32_t *rows, int32_t n_rows, float *states, float *evals,
                                    float *probs) {
  return co_guard(f, [&] { f->data.fetch_rows(rows, n_rows, states, evals, probs); });
}

/* ------------------------------------------------------------------ sample weights, merging of duplicates */
extern "C" int ca_fitter_set_sample_weights(ca_fitter *f, const float *weights, int32_t n) {
  return co_guard(f, [&] { f->data.set_weights(weights, n); });
}

extern "C" int ca_fitter_get_sample_weights(ca_fitter *f, float *out, int32_t n) {
  return co_guard(f, [&] { f->data.get_weights(out, n); });
}

extern "C" int ca_fitter_merge_duplicates(ca_fitter *f, int normalize, int32_t *before, int32_t *after) {
  return co_guard(f, [&] {
    if (!before || !after) throw CaError(CA_ERR_ARG, "ca_fitter_merge_duplicates: null output");
    f->data.merge(normalize != 0, before, after);
  });
}

/* ------------------------------------------------------------------ augmentation choice, canonical orientation */
extern "C" int ca_fitter_set_augmentation(ca_fitter *f, int32_t augmentation) {
  return co_guard(f, [&] { f->data.set_augmentation(augmentation); });
}

extern "C" int ca_fitter_get_augmentation(ca_fitter *f, int32_t *augmentation) {
  return co_guard(f, [&] {
    if (!augmentation) throw CaError(CA_ERR_ARG, "ca_fitter_get_augmentation: null output");
    *augmentation = f->data.augmentation();
  });
}

extern "C" int ca_fitter_canonicalize(ca_fitter *f, int32_t *moved) {
  return co_guard(f, [&] {
    if (!moved) throw CaError(CA_ERR_ARG, "ca_fitter_canonicalize: null output");
    f->data.canonicalize(moved);
  });
}

/* ------------------------------------------------------------------ fit options */
extern "C" int ca_fitter_set_options(ca_fitter *f, const ca_fit_options *options) {
  return co_guard(f, [&] {
    const ca_fit_options o = ft_struct_in(options, ca_fit_options{}, "ca_fitter_set_options"); /* the defaults: everything off */
    const float vals[6] = {o.l1, o.l2, o.weight_decay, o.clipvalue, o.clipnorm, o.global_clipnorm};
    for (float x : vals)
      if (!ft_finite_nonneg(x)) throw CaError(CA_ERR_ARG, "ca_fitter_set_options: every value must be finite and >= 0");
    if (o.regularize < 0 || o.regularize > 1) throw CaError(CA_ERR_ARG, "ca_fitter_set_options: regularize must be 0 or 1");
    if ((o.clipvalue > 0.0f) + (o.clipnorm > 0.0f) + (o.global_clipnorm > 0.0f) > 1)
      throw CaError(CA_ERR_ARG, "ca_fitter_set_options: at most one of clipvalue, clipnorm and global_clipnorm");
    if (ft_options_on(o)) f->end.plan_options(*f->net);
    f->end.opt.o = o;
  });
}

extern "C" int ca_fitter_get_options(ca_fitter *f, ca_fit_options *out) {
  return co_guard(f, [&] { ft_struct_out(out, f->end.opt.o, "ca_fitter_get_options"); });
}

extern "C" int ca_fitter_train_stats(ca_fitter *f, ca_fit_stats *out) {
  return co_guard(f, [&] { ft_struct_out(out, f->end.last, "ca_fitter_train_stats"); });
}

/* ------------------------------------------------------------------ Adam's arguments, the third slot, the average */
extern "C" int ca_fitter_set_adam(ca_fitter *f, const ca_fit_adam *adam) {
  return co_guard(f, [&] {
    const ca_fit_adam defaults = CA_FIT_ADAM_INIT; /* for what the caller's struct does not have */
    ca_fit_adam a = ft_struct_in(adam, defaults, "ca_fitter_set_adam");
    /* (a NaN fails every comparison) */
    if (!(a.beta_1 >= 0.0f && a.beta_1 < 1.0f) || !(a.beta_2 >= 0.0f && a.beta_2 < 1.0f))
      throw CaError(CA_ERR_ARG, "ca_fitter_set_adam: beta_1 and beta_2 must lie in [0, 1)");
    if (!(a.epsilon > 0.0f) || a.epsilon == INFINITY) throw CaError(CA_ERR_ARG, "ca_fitter_set_adam: epsilon must be finite and > 0");
    if (!(a.ema_momentum >= 0.0f && a.ema_momentum < 1.0f)) throw CaError(CA_ERR_ARG, "ca_fitter_set_adam: ema_momentum must lie in [0, 1)");
    if (a.ema_overwrite_frequency < 0 || (a.ema_overwrite_frequency > 0 && !(a.ema_momentum > 0.0f)))
      throw CaError(CA_ERR_ARG, "ca_fitter_set_adam: ema_overwrite_frequency must be >= 0, and > 0 only with ema_momentum > 0");
    a.amsgrad = a.amsgrad != 0;
    f->end.adam = a;
  });
}

extern "C" int ca_fitter_get_adam(ca_fitter *f, ca_fit_adam *out) {
  return co_guard(f, [&] { ft_struct_out(out, f->end.adam, "ca_fitter_get_adam"); });
}

static void ft_check_slot(ca_fitter *f, int32_t which, const void *values, size_t n_floats) {
  if (which != CA_SLOT_VHAT && which != CA_SLOT_AVERAGE) throw CaError(CA_ERR_ARG, "ca_fitter: the slot must be CA_SLOT_VHAT or CA_SLOT_AVERAGE");
  if (!values) throw CaError(CA_ERR_ARG, "ca_fitter: null slot values");
  f->check_n(n_floats);
}

extern "C" int ca_fitter_set_slot(ca_fitter *f, int32_t which, const float *values, size_t n_floats) {
  return co_guard(f, [&] {
    ft_check_slot(f, which, values, n_floats);
    f->end.set_slot(which, values);
  });
}

extern "C" int ca_fitter_get_slot(ca_fitter *f, int32_t which, float *values, size_t n_floats) {
  return co_guard(f, [&] {
    ft_check_slot(f, which, values, n_floats);
    f->end.get_slot(which, values);
  });
}

extern "C" int ca_fitter_swap_average(ca_fitter *f) {
  return co_guard(f, [&] { f->end.swap_average(); });
}

extern "C" int ca_fitter_apply_average(ca_fitter *f) {
  return co_guard(f, [&] { f->end.apply_average(); });
}

/* ------------------------------------------------------------------ loss, metrics, predict */
extern "C" int ca_fitter_set_loss(ca_fitter *f, const ca_fit_loss *loss) {
  return co_guard(f, [&] {
    const ca_fit_loss defaults = CA_FIT_LOSS_INIT; /* for what the caller's struct does not have */
    const ca_fit_loss l = ft_struct_in(loss, defaults, "ca_fitter_set_loss");
    if (!ft_finite_nonneg(l.value_weight) || !ft_finite_nonneg(l.policy_weight))
      throw CaError(CA_ERR_ARG, "ca_fitter_set_loss: value_weight and policy_weight must be finite and >= 0");
    if (l.value_weight == 0.0f && l.policy_weight == 0.0f)
      throw CaError(CA_ERR_ARG, "ca_fitter_set_loss: value_weight and policy_weight may not both be 0");
    if (!(l.label_smoothing >= 0.0f && l.label_smoothing < 1.0f)) /* (a NaN fails every comparison) */
      throw CaError(CA_ERR_ARG, "ca_fitter_set_loss: label_smoothing must lie in [0, 1)");
    if (l.value_loss != CA_VALUE_LOSS_MSE && l.value_loss != CA_VALUE_LOSS_HUBER)
      throw CaError(CA_ERR_ARG, "ca_fitter_set_loss: value_loss must be CA_VALUE_LOSS_MSE or CA_VALUE_LOSS_HUBER");
    if (!(l.huber_delta > 0.0f) || l.huber_delta == INFINITY)
      throw CaError(CA_ERR_ARG, "ca_fitter_set_loss: huber_delta must be finite and > 0");
    f->loss.args = l;
  });
}

extern "C" int ca_fitter_get_loss(ca_fitter *f, ca_fit_loss *out) {
  return co_guard(f, [&] { ft_struct_out(out, f->loss.args, "ca_fitter_get_loss"); });
}

extern "C" int ca_fitter_set_metrics(ca_fitter *f, int32_t on, int32_t top_k) {
  return co_guard(f, [&] {
    if (on && (top_k < 1 || top_k > CA_NUM_MOVES)) throw CaError(CA_ERR_ARG, "ca_fitter_set_metrics: top_k must be in 1..96");
    f->loss.set_metrics(on != 0, top_k);
  });
}

extern "C" int ca_fitter_metrics(ca_fitter *f, ca_fit_metrics *out) {
  return co_guard(f, [&] {
    ft_struct_check(out, "ca_fitter_metrics");
    if (!f->loss.metrics_on) throw CaError(CA_ERR_STATE, "ca_fitter_metrics: metrics are off (ca_fitter_set_metrics)");
    ft_struct_out(out, f->loss.lastm, "ca_fitter_metrics");
  });
}

extern "C" int ca_fitter_predict(ca_fitter *f, const int32_t *rows, int32_t n_rows, int32_t train, float *logits,
                                 float *values) {
  return co_guard(f, [&] {
    f->data.need_data(); /* here as well: this call has always looked at its pointers before its batch size */
    if (!rows || !logits || !values) throw CaError(CA_ERR_ARG, "ca_fitter_predict: null argument");
    const FtBatches bs = f->begin(n_rows, n_rows, ca_fitter::REPORT_NONE, [&] { return rows; });
    const FtBatch bt = f->data.batch(bs.rows, n_rows);
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
