// nn_train_opt.hip -- the end of a training step (FtStepEnd, nn_train.h): the update kernels, Adam's arguments with the
// third slot and the averaged weights (ft_k_average_swap, ft_k_average_apply), and the fit options (FtOpt): the L1L2
// regulariser, decoupled weight decay and gradient clipping (the definitions: corintho_hip.h, "Adam's arguments" and
// "fit options"; DESIGN.md, "Network training").  FtStepEnd::step is the one function that chooses among the four
// update kernels: ft_k_update at every default (one launch sums the split partials in a fixed order, applies Adam as TF
// ResourceApplyAdam does and moves the moving statistics), ft_k_update_adam with Adam's arguments off theirs, and with
// fit options on ft_k_opt_update or ft_k_opt_update_adam behind the options' two reducing launches.  A fitter whose
// options are all 0 never touches FtOpt.
//
// The weight vector is cut into pieces of at most FT_PIECE floats that lie within one tensor; workgroup p owns piece p
// in the two kernels that walk the weights.  Every sum is float64 and has a fixed shape: 256 values of a piece by a
// butterfly within each wave and the four waves' sums in order (ft_block_sum3); a tensor's pieces strided over the 64
// lanes of one wave, each lane's in ascending order, then the butterfly; the tensors the same way.  No float atomics:
// a launch writes what the next one reads.
#include "nn_train.h"

#define FT_PIECE 256
#define FT_OPT_MAXT 128      /* tensors the combine kernel has room for (mlp12x100 76, rescnn4 72) */
#define FT_OPT_MODE_NONE 0
#define FT_OPT_MODE_VALUE 1
#define FT_OPT_MODE_NORM 2
#define FT_OPT_MODE_GLOBAL 3

/* the sum over the wave's 64 lanes, in every lane: a butterfly, so the order of the additions is fixed */
__device__ __forceinline__ double ft_wave_sum(double x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
  return x;
}

/* three sums over the 256 threads of a block, valid in thread 0 */
__device__ __forceinline__ void ft_block_sum3(double (*red)[3], double &a, double &b, double &c) {
  a = ft_wave_sum(a), b = ft_wave_sum(b), c = ft_wave_sum(c);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[wv][0] = a, red[wv][1] = b, red[wv][2] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    a = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
    b = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    c = ((red[0][2] + red[1][2]) + red[2][2]) + red[3][2];
  }
}

/* Step 1 and the partials of piece blockIdx.x: g' = g + r in place in gsum (unless r_only), and
 * part[piece] = {sum g'^2 (trainable tensors), this piece's share of R, how many |g'| > clipvalue}.  reg_mask: bit c set
 * when tensors of class c are regularised.  r_only: R alone, gsum is neither read nor written. */
__global__ __launch_bounds__(FT_PIECE) void ft_k_opt_partials(const int4 *__restrict__ pieces, const float *__restrict__ w,
                                                             float *__restrict__ gsum, float l1, float l2, float two_l2,
                                                             int reg_mask, float clipvalue, int r_only,
                                                             double *__restrict__ part) {
  __shared__ double red[4][3];
  const int4 pc = pieces[blockIdx.x]; /* {offset, floats, tensor, class} */
  const int j = threadIdx.x;
  double sq = 0.0, rr = 0.0, nc = 0.0;
  if (j < pc.y) {
    const int i = pc.x + j;
    const bool reg = (reg_mask >> pc.w) & 1;
    double r = 0.0; /* in float64, so that g' is g + r rounded once: nothing is lost where the two cancel */
    if (reg) {
      const float wv = w[i];
      const double sg = wv > 0.0f ? 1.0 : wv < 0.0f ? -1.0 : 0.0;
      r = (double)l1 * sg + (double)two_l2 * (double)wv;
      rr = (double)l1 * fabs((double)wv) + (double)l2 * ((double)wv * (double)wv);
    }
    if (!r_only && pc.w != CA_TENSOR_MOVING) {
      float g = gsum[i];
      if (reg) {
        g = (float)((double)g + r);
        gsum[i] = g;
      }
      sq = (double)g * (double)g;
      nc = (clipvalue > 0.0f && fabsf(g) > clipvalue) ? 1.0 : 0.0;
    }
  }
  ft_block_sum3(red, sq, rr, nc);
  if (j == 0) {
    double *o = part + (size_t)blockIdx.x * 3;
    o[0] = sq, o[1] = rr, o[2] = nc;
  }
}

/* The partials combined, one block of 16 waves.  Wave k sums tensors k, k + 16, ...: the tensor's pieces (tfirst[t] to
 * tfirst[t + 1]) strided over its lanes.  Then wave 0 sums the tensors, and writes: scale[t] of every tensor, R to
 * *r_out, and (stats given) the call's statistics.  One block's launches follow each other on the stream, so the
 * statistics need no atomics. */
__global__ __launch_bounds__(1024) void ft_k_opt_combine(const double *__restrict__ part, const int32_t *__restrict__ tfirst,
                                                        int nt, int mode, float clip, float *__restrict__ scale,
                                                        double *__restrict__ r_out, FtOptStats *__restrict__ stats) {
  __shared__ double tsq[FT_OPT_MAXT], tr[FT_OPT_MAXT], tn[FT_OPT_MAXT];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int t = wv; t < nt; t += 16) {
    const int c0 = tfirst[t], c1 = tfirst[t + 1];
    double a = 0.0, b = 0.0, c = 0.0;
    for (int p = c0 + lane; p < c1; p += 64) {
      const double *q = part + (size_t)p * 3;
      a += q[0], b += q[1], c += q[2];
    }
    a = ft_wave_sum(a), b = ft_wave_sum(b), c = ft_wave_sum(c);
    if (lane == 0) tsq[t] = a, tr[t] = b, tn[t] = c;
  }
  __syncthreads();
  if (wv != 0) return;
  double a = 0.0, b = 0.0, c = 0.0, over = 0.0;
  const double cl = (double)clip;
  for (int t = lane; t < nt; t += 64) {
    a += tsq[t], b += tr[t], c += tn[t];
    if (mode == FT_OPT_MODE_NORM && sqrt(tsq[t]) > cl) over += 1.0;
  }
  a = ft_wave_sum(a), b = ft_wave_sum(b), c = ft_wave_sum(c), over = ft_wave_sum(over);
  const double norm = sqrt(a);
  for (int t = lane; t < nt; t += 64) {
    float s = 1.0f;
    if (mode == FT_OPT_MODE_NORM || mode == FT_OPT_MODE_GLOBAL) {
      const double n = mode == FT_OPT_MODE_NORM ? sqrt(tsq[t]) : norm;
      s = (float)(cl / (!(n <= cl) ? n : cl)); /* c / max(n, c); a NaN norm stays one */
    }
    scale[t] = s;
  }
  if (lane != 0) return;
  *r_out = b;
  if (stats) {
    const bool clipped = mode == FT_OPT_MODE_VALUE ? c > 0.0 : mode == FT_OPT_MODE_NORM ? over > 0.0
                       : mode == FT_OPT_MODE_GLOBAL ? norm > cl : false;
    stats->reg_sum += b;
    stats->norm_sum += norm;
    stats->norm_max = norm > stats->norm_max ? norm : stats->norm_max;
    stats->clipped += clipped ? 1.0 : 0.0;
  }
}

/* Steps 2 to 4 of piece blockIdx.x on g' in gsum: the clamp or the tensor's scale, the decay of the kernels
 * (decay = lr * weight_decay), Adam as ft_k_update has it (ft_adam, nn_train.h); a moving statistic moves as there.
 * PARAM: with Adam's arguments A, and a moving statistic's new value goes to the average as well. */
template <bool PARAM>
__device__ __forceinline__ void ft_opt_update_piece(const int4 *__restrict__ pieces, float *__restrict__ w,
                                                    float *__restrict__ m, float *__restrict__ v,
                                                    const float *__restrict__ gsum, const int32_t *__restrict__ sidx,
                                                    const float *__restrict__ stat, const float *__restrict__ scale,
                                                    float clipvalue, float decay, float lr_t, const FtAdamArgs &A) {
  const int4 pc = pieces[blockIdx.x];
  if ((int)threadIdx.x >= pc.y) return;
  const int i = pc.x + threadIdx.x;
  if (pc.w == CA_TENSOR_MOVING) {
    const float mv = w[i];
    const float nv = mv - (mv - stat[sidx[i]]) * 0.01f;
    w[i] = nv;
    if (PARAM && A.a) A.a[i] = nv;
    return;
  }
  float s = gsum[i];
  if (clipvalue > 0.0f)
    s = s > clipvalue ? clipvalue : s < -clipvalue ? -clipvalue : s;
  else
    s = s * scale[pc.z];
  float wv = w[i];
  if (decay > 0.0f && pc.w <= CA_TENSOR_HEAD_KERNEL) wv = wv - decay * wv;
  ft_adam<PARAM>(w, m, v, i, wv, s, lr_t, A);
}

/* the Adam defaults: the kernel of a step with fit options before Adam had arguments, instruction for instruction */
__global__ __launch_bounds__(FT_PIECE) void ft_k_opt_update(const int4 *__restrict__ pieces, float *__restrict__ w,
                                                           float *__restrict__ m, float *__restrict__ v,
                                                           const float *__restrict__ gsum, const int32_t *__restrict__ sidx,
                                                           const float *__restrict__ stat, const float *__restrict__ scale,
                                                           float clipvalue, float decay, float lr_t) {
  ft_opt_update_piece<false>(pieces, w, m, v, gsum, sidx, stat, scale, clipvalue, decay, lr_t, FtAdamArgs{});
}

__global__ __launch_bounds__(FT_PIECE) void ft_k_opt_update_adam(const int4 *__restrict__ pieces, float *__restrict__ w,
                                                                float *__restrict__ m, float *__restrict__ v,
                                                                const float *__restrict__ gsum,
                                                                const int32_t *__restrict__ sidx,
                                                                const float *__restrict__ stat,
                                                                const float *__restrict__ scale, float clipvalue,
                                                                float decay, float lr_t, FtAdamArgs A) {
  ft_opt_update_piece<true>(pieces, w, m, v, gsum, sidx, stat, scale, clipvalue, decay, lr_t, A);
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
void FtOpt::plan(const std::vector<FtTensor> &tensors, int nw, rt_stream_t s) {
  if (pieces.p) return;
  if ((int)tensors.size() > FT_OPT_MAXT) throw CaError(CA_ERR_INTERNAL, "fit options: more tensors than FT_OPT_MAXT");
  std::vector<int32_t> pc, first;
  int32_t at = 0;
  for (size_t t = 0; t < tensors.size(); ++t) {
    const FtTensor &T = tensors[t];
    /* the kernels index w, m, v and gsum by these offsets: the table must cover [0, nw) in order and nothing else */
    if (T.off != at || T.count < 1 || T.cls < CA_TENSOR_TRUNK_KERNEL || T.cls > CA_TENSOR_MOVING)
      throw CaError(CA_ERR_INTERNAL, "fit options: the tensor table does not cover the weight vector in order");
    first.push_back((int32_t)(pc.size() / 4));
    for (int32_t o = 0; o < T.count; o += FT_PIECE) {
      const int32_t k = T.count - o < FT_PIECE ? T.count - o : FT_PIECE;
      pc.insert(pc.end(), {T.off + o, k, (int32_t)t, T.cls});
    }
    at += T.count;
  }
  if (at != nw) throw CaError(CA_ERR_INTERNAL, "fit options: the tensor table does not cover the weight vector");
  first.push_back((int32_t)(pc.size() / 4));
  nt = (int)tensors.size();
  npieces = (int)(pc.size() / 4);
  pieces.upload(pc.data(), pc.size(), s);
  tfirst.upload(first.data(), first.size(), s);
  part.alloc((size_t)npieces * 3, s);
  scale.alloc((size_t)nt, s);
  rt_sync(s); /* pc and first are locals */
}

void FtOpt::begin(int n, rt_stream_t s) {
  if (slots < (size_t)n || !out.p) {
    out.alloc(4 + (size_t)n, s);
    slots = (size_t)n;
    hout.assign(4 + (size_t)n, 0.0);
  } else {
    rt_memset(out.p, 0, 4 * sizeof(double), s);
  }
}

static int ft_opt_reg_mask(const ca_fit_options &o) {
  if (!(o.l1 > 0.0f || o.l2 > 0.0f)) return 0;
  return o.regularize ? (1 << CA_TENSOR_TRUNK_KERNEL) | (1 << CA_TENSOR_HEAD_KERNEL) : 1 << CA_TENSOR_TRUNK_KERNEL;
}

void FtOpt::regularization(rt_stream_t s, const float *w, int slot) {
  RT_LAUNCH(ft_k_opt_partials, npieces, FT_PIECE, s, (const int4 *)pieces.p, w, (float *)nullptr, o.l1, o.l2, 2.0f * o.l2,
            ft_opt_reg_mask(o), 0.0f, 1, part.p);
  RT_LAUNCH(ft_k_opt_combine, 1, 1024, s, (const double *)part.p, (const int32_t *)tfirst.p, nt, FT_OPT_MODE_NONE, 0.0f,
            scale.p, out.p + 4 + slot, (FtOptStats *)nullptr);
}

void FtOpt::reduce(rt_stream_t s, const float *w, float *gsum, int slot) {
  const int mode = o.clipvalue > 0.0f ? FT_OPT_MODE_VALUE : o.clipnorm > 0.0f ? FT_OPT_MODE_NORM
                 : o.global_clipnorm > 0.0f ? FT_OPT_MODE_GLOBAL : FT_OPT_MODE_NONE;
  const float clip = mode == FT_OPT_MODE_VALUE ? o.clipvalue : mode == FT_OPT_MODE_NORM ? o.clipnorm : o.global_clipnorm;
  RT_LAUNCH(ft_k_opt_partials, npieces, FT_PIECE, s, (const int4 *)pieces.p, w, gsum, o.l1, o.l2, 2.0f * o.l2,
            ft_opt_reg_mask(o), o.clipvalue, 0, part.p);
  RT_LAUNCH(ft_k_opt_combine, 1, 1024, s, (const double *)part.p, (const int32_t *)tfirst.p, nt, mode, clip, scale.p,
            out.p + 4 + slot, (FtOptStats *)out.p);
}

void FtOpt::fetch(int n, rt_stream_t s) { rt_d2h(hout.data(), out.p, (4 + (size_t)n) * sizeof(double), s); }

/* ------------------------------------------------------------------ the end of a step */
/* is every one of Adam's arguments at its default?  Then a step runs the kernels that know of none. */
bool FtStepEnd::adam_default() const {
  return adam.beta_1 == 0.9f && adam.beta_2 == 0.999f && adam.epsilon == 1e-7f && !adam.amsgrad && !(adam.ema_momentum > 0.0f);
}

/* Adam's arguments of the step that brings the step count to `step`.  The third slot and the average get their memory
 * at their first use (zeroed, on the stream); an invalid average starts as the weights before the step. */
FtAdamArgs FtStepEnd::adam_args(int64_t step) {
  FtAdamArgs A = {adam.beta_1, adam.beta_2, adam.epsilon, adam.ema_momentum, nullptr, nullptr, 0};
  if (adam.amsgrad) {
    if (!vhat.p) vhat.alloc(W.nw, s);
    A.h = vhat.p;
  }
  if (adam.ema_momentum > 0.0f) {
    if (!avg.p) avg.alloc(W.nw, s);
    if (!avg_valid) rt_d2d(avg.p, W.w, (size_t)W.nw * sizeof(float), s);
    avg_valid = true;
    A.a = avg.p;
    A.overwrite = adam.ema_overwrite_frequency > 0 && step % adam.ema_overwrite_frequency == 0;
  }
  return A;
}

void FtStepEnd::sum_gradient(FtSplits ns) {
  RT_LAUNCH(ft_k_update, (W.nw + 255) / 256, 256, s, W.w, W.m, W.v, (const float *)W.g, W.nw, ns.rows, ns.pixels, W.sidx,
            W.stat, 0.0f, 0, W.gsum);
}

void FtStepEnd::step(FtSplits ns, float lr, int64_t step, int slot) {
  /* Keras Adam: local_step = iterations + 1, lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t), in float32 */
  const float t = (float)step;
  const float lr_t = lr * (sqrtf(1.0f - powf(adam.beta_2, t)) / (1.0f - powf(adam.beta_1, t)));
  const bool adam_on = !adam_default();
  const FtAdamArgs A = adam_on ? adam_args(step) : FtAdamArgs{};
  if (!ft_options_on(opt.o)) { /* one launch: the partials summed, Adam, the moving statistics */
    if (adam_on)
      RT_LAUNCH(ft_k_update_adam, (W.nw + 255) / 256, 256, s, W.w, W.m, W.v, (const float *)W.g, W.nw, ns.rows, ns.pixels,
                W.sidx, W.stat, lr_t, A);
    else
      RT_LAUNCH(ft_k_update, (W.nw + 255) / 256, 256, s, W.w, W.m, W.v, (const float *)W.g, W.nw, ns.rows, ns.pixels,
                W.sidx, W.stat, lr_t, 1, W.gsum);
    return;
  }
  /* with options: the summed gradient to gsum as ca_fitter_gradients has it, then steps 1 to 4 */
  sum_gradient(ns);
  opt.reduce(s, W.w, W.gsum, slot);
  const float clipvalue = opt.o.clipvalue, decay = lr * opt.o.weight_decay;
  if (adam_on)
    RT_LAUNCH(ft_k_opt_update_adam, opt.npieces, FT_PIECE, s, (const int4 *)opt.pieces.p, W.w, W.m, W.v,
              (const float *)W.gsum, W.sidx, W.stat, (const float *)opt.scale.p, clipvalue, decay, lr_t, A);
  else
    RT_LAUNCH(ft_k_opt_update, opt.npieces, FT_PIECE, s, (const int4 *)opt.pieces.p, W.w, W.m, W.v, (const float *)W.gsum,
              W.sidx, W.stat, (const float *)opt.scale.p, clipvalue, decay, lr_t);
}

FtReg FtStepEnd::begin(int nb) {
  last = ca_fit_stats{sizeof(ca_fit_stats), 0, 0, 0, 0.0, 0.0, 0.0};
  if (!ft_options_on(opt.o)) return FtReg::none;
  opt.begin(nb, s);
  return FtReg::per_batch;
}

void FtStepEnd::finish(int nb) {
  if (!ft_options_on(opt.o)) return;
  const double *st = opt.hout.data(); /* the statistics came back with the losses */
  last.steps = nb;
  last.clipped_steps = (int64_t)st[3];
  last.regularization = st[0] / nb;
  last.grad_norm = st[1] / nb;
  last.grad_norm_max = st[2];
}

FtReg FtStepEnd::begin_evaluate() {
  if (!ft_regularized(opt.o)) return FtReg::none;
  opt.begin(1, s);
  opt.regularization(s, W.w, 0);
  return FtReg::once;
}

/* Those kernels take a weight for a moving statistic by its tensor's class and ft_k_update by its code: the two tables
 * must agree. */
void FtStepEnd::plan_options(const FtNet &net) {
  if (opt.pieces.p) return;
  std::vector<FtTensor> tt;
  std::vector<int32_t> si;
  net.tensor_table(tt);
  net.update_table(si);
  for (const FtTensor &t : tt)
    for (int32_t i = t.off; i < t.off + t.count && i >= 0 && i < W.nw; ++i)
      if ((si[i] >= 0) != (t.cls == CA_TENSOR_MOVING))
        throw CaError(CA_ERR_INTERNAL, "ca_fitter: tensor_table and update_table disagree about the moving statistics");
  opt.plan(tt, W.nw, s);
}

void FtStepEnd::slots_replaced() {
  if (vhat.p) rt_memset(vhat.p, 0, W.nw * sizeof(float), s);
}

void FtStepEnd::need_average(const char *who) const {
  if (!avg_valid) throw CaError(CA_ERR_STATE, std::string(who) + ": the fitter has no average (no step with ema_momentum > 0, no ca_fitter_set_slot)");
}

void FtStepEnd::set_slot(int32_t which, const float *values) {
  DevBuf<float> &b = which == CA_SLOT_VHAT ? vhat : avg;
  if (!b.p) b.alloc(W.nw, s);
  rt_h2d(b.p, values, W.nw * sizeof(float), s);
  rt_sync(s);
  if (which == CA_SLOT_AVERAGE) avg_valid = true;
}

void FtStepEnd::get_slot(int32_t which, float *values) {
  if (which == CA_SLOT_AVERAGE) need_average("ca_fitter_get_slot");
  const DevBuf<float> &b = which == CA_SLOT_VHAT ? vhat : avg;
  if (!b.p) { /* a third slot that no step has used yet */
    for (int i = 0; i < W.nw; ++i) values[i] = 0.0f;
    return;
  }
  rt_d2h(values, b.p, W.nw * sizeof(float), s);
  rt_sync(s);
}

void FtStepEnd::swap_average() {
  need_average("ca_fitter_swap_average");
  RT_LAUNCH(ft_k_average_swap, (W.nw + 255) / 256, 256, s, W.w, avg.p, W.nw);
}

void FtStepEnd::apply_average() {
  need_average("ca_fitter_apply_average");
  RT_LAUNCH(ft_k_average_apply, (W.nw + 255) / 256, 256, s, W.w, (const float *)avg.p, W.sidx, W.nw);
}
