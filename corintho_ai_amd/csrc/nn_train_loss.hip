// nn_train_loss.hip -- the loss off its defaults and the metrics of a fit (the definition: corintho_hip.h, "loss and
// metrics").  ft_k_loss_opt is ft_k_loss's row loop (nn_train.hip) with the loss weights, label smoothing and the Huber
// value loss as arguments; a fit at the defaults never launches it.  ft_k_metrics reads the same head outputs H, one
// wavefront per row, and ft_k_metrics_reduce sums the rows' terms in the fixed order of ft_colsum: no atomics, so a
// call's metrics are bitwise reproducible.
#include <math.h>

#include "nn_train.h"

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
void ft_loss_opt(rt_stream_t s, const float *H, const int32_t *rows, int B, const float *evals, const float *probs,
                 float *Hd, const float *wts, const FtLossArgs &L) {
  if (wts)
    RT_LAUNCH(ft_k_loss_opt<true>, (B + 255) / 256, 256, s, H, rows, B, evals, probs, Hd, wts, L);
  else
    RT_LAUNCH(ft_k_loss_opt<false>, (B + 255) / 256, 256, s, H, rows, B, evals, probs, Hd, (const float *)nullptr, L);
}

void ft_metrics(rt_stream_t s, const float *H, const int32_t *rows, int B, const float *evals, const float *probs,
                const float *wts, int top_k, float *mrow, float *out) {
  if (wts)
    RT_LAUNCH(ft_k_metrics<true>, (B + 3) / 4, 256, s, H, rows, B, evals, probs, wts, top_k, mrow);
  else
    RT_LAUNCH(ft_k_metrics<false>, (B + 3) / 4, 256, s, H, rows, B, evals, probs, (const float *)nullptr, top_k, mrow);
  RT_LAUNCH(ft_k_metrics_reduce, 1, 1024, s, (const float *)mrow, B, out);
}
