// nn_train_loss.hip -- every loss kernel of a fit, the metrics, and what a call reports (FtLoss, nn_train.h; the
// definition: corintho_hip.h, "loss and metrics").  ft_k_loss is the reference's value_mse + 0.25 policy_cce;
// ft_k_loss_opt is its row loop with the loss weights, label smoothing and the Huber value loss as arguments, and a fit
// at the defaults never launches it; ft_k_head_reduce sums either one's rows.  FtLoss::terms is the one function that
// chooses among them.  ft_k_metrics reads the same head outputs H, one wavefront per row, and ft_k_metrics_reduce sums
// the rows' terms in the fixed order of ft_colsum: no atomics, so a call's metrics are bitwise reproducible.  The host
// part owns the loss arguments, the per-batch loss and metric sums on the device and the host, and turns them into
// the losses and the ca_fit_metrics a call returns.
#include <math.h>

#include "nn_train.h"

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

/* ft_k_loss with L: the smoothed target t' = t (1 - ls) + ls / 96 in place of t, the policy gradient times
 * policy_weight where ft_k_loss has 0.25f, the value gradient times value_weight, and with L.huber Keras's Huber(delta)
 * for the squared error.  Hd[r][97] and [98] are the row's two terms, not times the loss weights.  At the defaults
 * (1, 0.25, 0, MSE) every float is the one ft_k_loss writes. */
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void ft_k_loss_opt(const float *__restrict__ H, const int32_t *__restrict__ rows, int B,
                                                    const float *__restrict__ evals, const float *__restrict__ probs,
                                                    float *__restrict__ Hd, const float *__restrict__ wts, FtLossArgs L) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= B) return;
  const float *h = H + (long)r * FT_PADW;
  const float *t = probs + (long)rows[r] * CA_NUM_MOVES;
  float *d = Hd + (long)r * FT_PADW;
  const float keep = 1.0f - L.label_smoothing, uniform = L.label_smoothing / (float)CA_NUM_MOVES;
  float m = -INFINITY;
  for (int j = 0; j < CA_NUM_MOVES; ++j) m = h[j] > m ? h[j] : m;
  float se = 0.0f;
  for (int j = 0; j < CA_NUM_MOVES; ++j) se += expf(h[j] - m);
  const float lse = m + logf(se);
  float st = 0.0f, ce = 0.0f;
  for (int j = 0; j < CA_NUM_MOVES; ++j) {
    const float tj = t[j] * keep + uniform;
    st += tj;
    ce += tj * (lse - h[j]);
  }
  const float inv_b = 1.0f / (float)B;
  const float w = WEIGHTED ? wts[rows[r]] : 1.0f;
  for (int j = 0; j < CA_NUM_MOVES; ++j) {
    const float tj = t[j] * keep + uniform;
    const float x = L.policy_weight * (expf(h[j] - lse) * st - tj) * inv_b;
    d[j] = WEIGHTED ? x * w : x;
  }
  const float tv = tanhf(h[96]);
  const float err = tv - evals[rows[r]];
  float gv, lv;
  if (L.huber) {
    const float dl = L.huber_delta, a = fabsf(err);
    const float c = err > dl ? dl : err < -dl ? -dl : err;
    gv = L.value_weight * c * fmaf(-tv, tv, 1.0f) * inv_b;
    lv = a <= dl ? 0.5f * err * err : dl * (a - 0.5f * dl);
  } else {
    gv = L.value_weight * 2.0f * err * fmaf(-tv, tv, 1.0f) * inv_b;
    lv = err * err;
  }
  d[96] = WEIGHTED ? gv * w : gv;
  d[97] = WEIGHTED ? lv * w : lv;
  d[98] = WEIGHTED ? ce * w : ce;
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

/* the sum of v over the 64 lanes, to every lane: a butterfly of fixed shape (both lanes of a pair add the same two
 * floats, so all lanes end with the same bits) */
__device__ __forceinline__ float ft_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

/* the largest v over the 64 lanes and its index i, to every lane.  Pairs are ordered by larger value, then lower index:
 * a total order, so the result is the first maximum whatever the shape of the reduction. */
__device__ __forceinline__ void ft_wave_argmax(float &v, int &i) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(v, off);
    const int oi = __shfl_xor(i, off);
    if (ov > v || (ov == v && oi < i)) v = ov, i = oi;
  }
}

/* One wavefront per row r < B, four rows per workgroup: lane l holds columns l and l + 64 (the latter for l < 32) of the
 * logits H[r] and of the target probs[rows[r]].  mrow[r] = {accuracy, top-k accuracy, |tanh v - z|, policy entropy,
 * target entropy} of the row, each times the row's sample weight w when WEIGHTED, then w (1 when not), then two zeros. */
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void ft_k_metrics(const float *__restrict__ H, const int32_t *__restrict__ rows, int B,
                                                   const float *__restrict__ evals, const float *__restrict__ probs,
                                                   const float *__restrict__ wts, int top_k, float *__restrict__ mrow) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B) return; /* whole waves leave; the kernel has no barrier */
  const int row = rows[r];
  const float *h = H + (long)r * FT_PADW;
  const float *t = probs + (long)row * CA_NUM_MOVES;
  const bool two = lane + 64 < CA_NUM_MOVES;
  const float h0 = h[lane], h1 = two ? h[lane + 64] : -INFINITY;
  const float t0 = t[lane], t1 = two ? t[lane + 64] : -INFINITY;
  /* the two first maxima */
  float hm = h0, tm = t0;
  int hi = lane, c = lane;
  if (h1 > h0) hm = h1, hi = lane + 64;
  if (t1 > t0) tm = t1, c = lane + 64;
  ft_wave_argmax(hm, hi);
  ft_wave_argmax(tm, c);
  /* how many logits are above the target's: h_c from the lane that holds it, one ballot per half */
  const float hc = __shfl(c >= 64 ? h1 : h0, c & 63);
  const int above = __popcll(__ballot(h0 > hc)) + __popcll(__ballot(two && h1 > hc));
  /* log-sum-exp from the maximum, then the entropy of the softmax and of the target */
  const float se = ft_wave_sum(expf(h0 - hm) + (two ? expf(h1 - hm) : 0.0f));
  const float lse = hm + logf(se);
  const float l0 = h0 - lse, l1 = h1 - lse;
  const float pe = ft_wave_sum(-(expf(l0) * l0) + (two ? -(expf(l1) * l1) : 0.0f));
  const float te = ft_wave_sum((t0 > 0.0f ? -(t0 * logf(t0)) : 0.0f) + (two && t1 > 0.0f ? -(t1 * logf(t1)) : 0.0f));
  if (lane != 0) return;
  const float mae = fabsf(tanhf(h[96]) - evals[row]);
  const float acc = hi == c ? 1.0f : 0.0f, topk = above < top_k ? 1.0f : 0.0f;
  float *o = mrow + (long)r * FT_METRIC_W;
  if (WEIGHTED) {
    const float w = wts[row];
    o[0] = acc * w, o[1] = topk * w, o[2] = mae * w, o[3] = pe * w, o[4] = te * w, o[5] = w;
  } else {
    o[0] = acc, o[1] = topk, o[2] = mae, o[3] = pe, o[4] = te, o[5] = 1.0f;
  }
  o[6] = 0.0f, o[7] = 0.0f;
}

/* column sums of mrow over the B rows, in the fixed order of ft_k_head_reduce: one workgroup */
__global__ __launch_bounds__(1024) void ft_k_metrics_reduce(const float *__restrict__ mrow, int B, float *__restrict__ out) {
  __shared__ float red[(FT_BN_RG + 1) * 16];
  const int f = threadIdx.x & 15, rg = threadIdx.x >> 4;
  float s = 0.0f;
  if (f < FT_METRIC_W)
    for (int r = rg; r < B; r += FT_BN_RG) s += mrow[(long)r * FT_METRIC_W + f];
  s = ft_colsum(red, s);
  if (rg == 0 && f < FT_METRIC_W) out[f] = s;
}

/* ------------------------------------------------------------------ host */
/* is the loss the reference's value_mse + 0.25 policy_cce?  Then a step runs the kernels that know of no other. */
bool FtLoss::is_default() const {
  return args.value_weight == 1.0f && args.policy_weight == 0.25f && args.label_smoothing == 0.0f &&
         args.value_loss == CA_VALUE_LOSS_MSE;
}

void FtLoss::terms(const FtShared &sh, const FtNet &net, const FtBatch &b, int B, bool grads, int slot) {
  const float *H = sh.h;
  const int grid = (B + 255) / 256;
  if (!is_default()) {
    const FtLossArgs L = {args.value_weight, args.policy_weight, args.label_smoothing, args.huber_delta,
                          args.value_loss == CA_VALUE_LOSS_HUBER};
    if (b.wts)
      RT_LAUNCH(ft_k_loss_opt<true>, grid, 256, sh.s, H, b.rows, B, b.evals, b.probs, sh.hd, b.wts, L);
    else
      RT_LAUNCH(ft_k_loss_opt<false>, grid, 256, sh.s, H, b.rows, B, b.evals, b.probs, sh.hd, (const float *)nullptr, L);
  } else if (b.wts)
    RT_LAUNCH(ft_k_loss<true>, grid, 256, sh.s, H, b.rows, B, b.evals, b.probs, sh.hd, b.wts);
  else
    RT_LAUNCH(ft_k_loss<false>, grid, 256, sh.s, H, b.rows, B, b.evals, b.probs, sh.hd, (const float *)nullptr);
  RT_LAUNCH(ft_k_head_reduce, FT_PADW / 16, 1024, sh.s, (const float *)sh.hd, B, grads ? sh.g : (float *)nullptr,
            net.policy_bias(), net.value_bias(), loss.p + 2 * slot);
}

void FtLoss::metric_terms(const FtShared &sh, const FtBatch &b, int B, int slot) {
  const float *H = sh.h;
  if (b.wts)
    RT_LAUNCH(ft_k_metrics<true>, (B + 3) / 4, 256, sh.s, H, b.rows, B, b.evals, b.probs, b.wts, top_k, mrow.p);
  else
    RT_LAUNCH(ft_k_metrics<false>, (B + 3) / 4, 256, sh.s, H, b.rows, B, b.evals, b.probs, (const float *)nullptr, top_k,
              mrow.p);
  RT_LAUNCH(ft_k_metrics_reduce, 1, 1024, sh.s, (const float *)mrow.p, B, metric.p + (size_t)FT_METRIC_W * slot);
}

void FtLoss::set_metrics(bool on, int32_t k) {
  if (on) top_k = k;
  metrics_on = on;
  lastm = ca_fit_metrics{sizeof(ca_fit_metrics), top_k, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
}

void FtLoss::ensure(int slots, bool metrics, int32_t max_batch, rt_stream_t s) {
  if ((int)hloss.size() < 2 * slots) {
    loss.alloc((size_t)2 * slots, s);
    hloss.assign((size_t)2 * slots, 0.0f);
  }
  if (!metrics) return;
  if (!mrow.p) mrow.alloc((size_t)max_batch * FT_METRIC_W, s);
  if (hmetric.size() < (size_t)FT_METRIC_W * slots) {
    metric.alloc((size_t)FT_METRIC_W * slots, s);
    hmetric.assign((size_t)FT_METRIC_W * slots, 0.0f);
  }
}

/* the call's metrics from its nb batches' sums, which losses() fetched: the batches added in float64 */
void FtLoss::metrics_of(int nb, int32_t nr) {
  double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = 0; b < nb; ++b)
    for (int k = 0; k < 6; ++k) sum[k] += (double)hmetric[(size_t)FT_METRIC_W * b + k];
  const double ws = sum[5];
  auto mean = [&](int k) { return ws > 0.0 ? sum[k] / ws : 0.0; };
  lastm = ca_fit_metrics{sizeof(ca_fit_metrics), top_k, nr, ws, mean(0), mean(1), mean(2), mean(3), mean(4)};
}

void FtLoss::losses(rt_stream_t s, const FtBatches &bs, double *out, float *per, FtReg reg, FtOpt &opt) {
  const int nb = bs.nb;
  const int32_t nr = bs.n_rows;
  const bool with_r = reg != FtReg::none, each = reg == FtReg::per_batch;
  rt_d2h(hloss.data(), loss.p, (size_t)2 * nb * sizeof(float), s);
  if (with_r) opt.fetch(each ? nb : 1, s);
  if (bs.metrics) rt_d2h(hmetric.data(), metric.p, (size_t)FT_METRIC_W * nb * sizeof(float), s);
  rt_sync(s);
  if (bs.metrics) metrics_of(nb, nr);
  const float vw = args.value_weight, pw = args.policy_weight; /* 1.0f * lv has the bits of lv */
  double sv = 0.0, sp = 0.0, sr = 0.0;
  for (int b = 0; b < nb; ++b) {
    const int rb = bs.size(b);
    const float lv = hloss[2 * b] / (float)rb, lp = hloss[2 * b + 1] / (float)rb;
    if (per) {
      per[3 * b] = with_r ? vw * lv + pw * lp + (float)opt.R(each ? b : 0) : vw * lv + pw * lp;
      per[3 * b + 1] = lv;
      per[3 * b + 2] = lp;
    }
    sv += (double)lv * rb;
    sp += (double)lp * rb;
    if (with_r) sr += opt.R(each ? b : 0) * rb;
  }
  if (out) {
    out[1] = nr ? sv / nr : 0.0;
    out[2] = nr ? sp / nr : 0.0;
    out[0] = (double)vw * out[1] + (double)pw * out[2];
    if (with_r) out[0] += nr ? sr / nr : 0.0;
  }
}
