// nn_train_conv.hip -- rescnn4's training step ("Network training", rescnn4): its convolutional kernels,
// float32 on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32), and below them the network as the fitter sees it
// (FtResCnn, an FtNet of nn_train.h): layout, buffers, forward and backward.  The heads' 1x1 convolutions and dense
// layers go through ft_k_gemm (nn_train.hip).
//
// Activations are NHWC [B * 16][C], row = position * 16 + pixel, so a 16-row MFMA tile is one 4x4 board and a 3x3 tap
// is a permutation of the tile's rows with the off-board rows zero: no im2col buffer exists.
//   fc_k_conv3       implicit GEMM, forward and (on the mirrored, transposed kernels of fc_k_wtrans) backward-data
//   fc_k_wgrad       dW = X_shifted^T dZ per row chunk; fc_k_wgrad_sum adds the chunks in order
//   fc_k_bn_part / _final / _apply      BatchNorm forward with batch statistics, residual add, ReLU
//   fc_k_bnb_part / _final / _apply     its backward: ReLU mask, residual pass-through, dgamma, dbeta, dZ
// Every cross-workgroup sum is per-chunk partials combined in chunk order by a later launch: no float atomics, no
// grid-wide barrier, so a step is bitwise reproducible.
#include <math.h>

#include "nn_train.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define FC_C 64           /* trunk channels */
#define FC_IN_LD 16       /* input planes: 10 channels padded with zeros to one k tile row of 16 */
#define FC_BN_CHUNKS 256  /* at most this many row chunks in a BatchNorm reduction */
#define FC_WG_CHUNKS 128  /* at most this many row chunks in a 3x3 weight gradient */
#define FC_WG_FLOATS (9 * FC_C * FC_C)
#define FC_BN_PART (FC_BN_CHUNKS * 3 * 64)         /* BatchNorm chunk partials: float32 forward, float64 backward */
#define FC_BN_SCRATCH (2 * (FC_BN_PART + 2 * 64)) /* floats of those and of the two per-channel constants behind them */
#define FC_POS 4   /* positions of a convolution workgroup, one per wave */
#define FC_XLD 66  /* LDS row stride of a board tile: lanes (row i, k q) of a 32-lane half on 32 banks (2 i + q) */
#define FC_WLD 80  /* LDS row stride of [k][n] operands: lanes (k q, n i) of a half on banks 16 q + i */

__global__ __launch_bounds__(256) void fc_k_planes(const float *__restrict__ states, const int32_t *__restrict__ rows, int B,
                                                   float *__restrict__ x0) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)B * 16 * FC_IN_LD) return;
  const int c = (int)(e % FC_IN_LD), p = (int)(e / FC_IN_LD % 16);
  const long r = e / (16 * FC_IN_LD);
  const float *s = states + (long)rows[r] * CA_GAME_STATE_SIZE;
  x0[e] = c < 4 ? s[p * 4 + c] : c < 10 ? s[64 + c - 4] : 0.0f;
}

__global__ __launch_bounds__(256) void fc_k_wtrans(const float *__restrict__ w, int first, int stride, int n,
                                                   float *__restrict__ wt) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n * FC_WG_FLOATS) return;
  const int l = e / FC_WG_FLOATS, t = e / (FC_C * FC_C) % 9, co = e / FC_C % FC_C, ci = e % FC_C;
  wt[e] = w[(long)first + (long)l * stride + ((8 - t) * FC_C + ci) * FC_C + co];
}

/* One workgroup = FC_POS positions x 64 output channels, a wave per position with four 16x16 accumulators.  The
 * boards' input rows are staged once, each tap's [CIN][64] weights in turn.  CIN = 16: the stem (weights of ci >= cin
 * read as zero). */
template <int CIN>
__global__ __launch_bounds__(256) void fc_k_conv3(const float *__restrict__ X, const float *__restrict__ W, int cin,
                                                  const float *__restrict__ bias, float *__restrict__ out, int B,
                                                  int accumulate) {
  __shared__ float xs[FC_POS * 16 * FC_XLD];
  __shared__ float ws[CIN * FC_WLD];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
  const long row0 = (long)blockIdx.x * FC_POS * 16, nrow = (long)B * 16;
  for (int e = threadIdx.x; e < FC_POS * 16 * CIN; e += 256) {
    const int r = e / CIN, c = e % CIN;
    xs[r * FC_XLD + c] = row0 + r < nrow ? X[(row0 + r) * CIN + c] : 0.0f;
  }
  f32x4 acc[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int py = i >> 2, px = i & 3;
  for (int tap = 0; tap < 9; ++tap) {
    __syncthreads(); /* the previous tap's reads are done */
    const float *Wt = W + (long)tap * cin * FC_C;
    for (int e = threadIdx.x; e < CIN * FC_C; e += 256) {
      const int k = e >> 6, n = e & 63;
      ws[k * FC_WLD + n] = k < cin ? Wt[e] : 0.0f;
    }
    __syncthreads();
    const int sy = py + tap / 3 - 1, sx = px + tap % 3 - 1;
    const bool on = sy >= 0 && sy < 4 && sx >= 0 && sx < 4;
    const float *xr = xs + (wave * 16 + (on ? sy * 4 + sx : 0)) * FC_XLD + q;
    const float *wr = ws + q * FC_WLD + i;
#pragma unroll 4
    for (int k = 0; k < CIN / 4; ++k) {
      const float a = on ? xr[4 * k] : 0.0f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wr[4 * k * FC_WLD + nt * 16], acc[nt], 0, 0, 0);
    }
  }
  /* acc[nt][r] = out[row 4q + r of the wave's board][channel 16 nt + i] */
  const long pos = (long)blockIdx.x * FC_POS + wave;
  if (pos >= B) return;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int co = nt * 16 + i;
    const float bv = bias ? bias[co] : 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float *o = out + (pos * 16 + 4 * q + r) * FC_C + co;
      float v = acc[nt][r] + bv;
      if (accumulate) v = *o + v;
      *o = v;
    }
  }
}

/* One workgroup = one row chunk (ppc positions) x one kernel row (three taps); a wave per (tap, 16 input channels) with
 * four accumulators, 3 * CIN / 16 waves.  Four boards of X and dZ are staged at a time; a k step is one board row (four
 * pixels), skipped where the tap's shift takes the whole row off the board.  part[chunk][tap][ci][co]. */
template <int CIN>
__global__ __launch_bounds__(3 * CIN * 4) void fc_k_wgrad(const float *__restrict__ X, const float *__restrict__ dZ, int B,
                                                          int ppc, int cin, float *__restrict__ part) {
  __shared__ float xs[64 * FC_WLD];
  __shared__ float gs[64 * FC_WLD];
  constexpr int MT = CIN / 16, NT = 3 * MT * 64;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
  const int dy = (int)blockIdx.y - 1, dx = wave / MT - 1, mt = wave % MT;
  const int p0 = blockIdx.x * ppc, p1 = min(B, p0 + ppc);
  f32x4 acc[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int sx = q + dx;
  const bool onx = sx >= 0 && sx < 4;
  for (int pb = p0; pb < p1; pb += 4) {
    __syncthreads();
    const long r0 = (long)pb * 16, rend = (long)p1 * 16;
    for (int e = threadIdx.x; e < 64 * CIN; e += NT) {
      const int r = e / CIN, c = e % CIN;
      xs[r * FC_WLD + c] = r0 + r < rend ? X[(r0 + r) * CIN + c] : 0.0f;
    }
    for (int e = threadIdx.x; e < 64 * FC_C; e += NT) {
      const int r = e >> 6, c = e & 63;
      gs[r * FC_WLD + c] = r0 + r < rend ? dZ[(r0 + r) * FC_C + c] : 0.0f;
    }
    __syncthreads();
#pragma unroll 2
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int y = 0; y < 4; ++y) {
        const int sy = y + dy;
        if (sy < 0 || sy >= 4) continue; /* wave-uniform */
        const float a = onx ? xs[(j * 16 + sy * 4 + sx) * FC_WLD + mt * 16 + i] : 0.0f;
        const float *gr = gs + (j * 16 + y * 4 + q) * FC_WLD + i;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, gr[nt * 16], acc[nt], 0, 0, 0);
      }
  }
  /* acc[nt][r] = dW[tap][ci = 16 mt + 4q + r][co = 16 nt + i] of this chunk */
  const int tap = (dy + 1) * 3 + dx + 1;
  float *o = part + ((long)blockIdx.x * 9 + tap) * cin * FC_C;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ci = mt * 16 + 4 * q + r;
      if (ci < cin) o[ci * FC_C + nt * 16 + i] = acc[nt][r];
    }
}

__global__ __launch_bounds__(256) void fc_k_wgrad_sum(const float *__restrict__ part, int nchunk, int n, float *__restrict__ dW) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  float s = 0.0f;
  for (int j = 0; j < nchunk; ++j) s += part[(long)j * n + e];
  dW[e] = s;
}

/* ---------------------------------------------------------------- BatchNorm over channels
 * 256 threads = (256 / C) row groups x C channels, so thread t always meets channel t % C and rows are read whole. */

/* sum over the block's row groups in a fixed order, returned to every thread of the channel; red holds 256 + 64 of T
 * (float forward, double backward) */
template <typename T>
__device__ __forceinline__ T fc_groupsum(T *red, T v, int C) {
  const int c = threadIdx.x % C;
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  if ((int)threadIdx.x < C) {
    T s = 0;
    for (int j = 0; j < 256; j += C) s += red[j + c];
    red[256 + c] = s;
  }
  __syncthreads();
  return red[256 + c];
}

/* chunk j = rows [j rpc, min(R, (j + 1) rpc)): part[j][0][c] = its mean, part[j][1][c] = sum (z - that mean)^2 */
__global__ __launch_bounds__(256) void fc_k_bn_part(const float *__restrict__ Z, int R, int C, int rpc, float *__restrict__ part) {
  __shared__ float red[256 + 64];
  const int c = threadIdx.x % C, rg = threadIdx.x / C, nrg = 256 / C;
  const int r0 = blockIdx.x * rpc, r1 = min(R, r0 + rpc);
  float s = 0.0f;
  for (int r = r0 + rg; r < r1; r += nrg) s += Z[(long)r * C + c];
  const float mean = fc_groupsum(red, s, C) / (float)(r1 - r0);
  float s2 = 0.0f;
  for (int r = r0 + rg; r < r1; r += nrg) {
    const float d = Z[(long)r * C + c] - mean;
    s2 += d * d;
  }
  s2 = fc_groupsum(red, s2, C);
  if (rg == 0) {
    part[(blockIdx.x * 2) * 64 + c] = mean;
    part[(blockIdx.x * 2 + 1) * 64 + c] = s2;
  }
}

/* the chunks combined in order: mean = sum n_j mean_j / R, variance = sum (M2_j + n_j (mean_j - mean)^2) / R (biased).
 * The sums over the chunks are float64, each statistic rounded once: a float32 running sum of up to 256 terms n_j mean_j
 * leaves the mean some 3e-7 of itself off, the same for every row, and xhat = (z - mean) rstd carries that times
 * |mean| / sigma into every row alike -- an error that does not average out over the batch (it reached the policy head's
 * gradient and the policy loss where a channel's mean is tens of its sigma; the backward sums are float64 for the same
 * reason, below).  Every chunk but the last has rpc rows, so the sums run over the chunks' means, their M2 and their
 * squared distances from the mean as they are, and the row counts come in once at the end. */
__global__ __launch_bounds__(64) void fc_k_bn_final(const float *__restrict__ part, int nch, int R, int rpc, int C,
                                                    float *__restrict__ stat) {
  const int c = threadIdx.x;
  if (c >= C) return;
  const int full = nch - 1, nlast = R - full * rpc; /* chunks of rpc rows, and the rows of the last one */
  const double mlast = (double)part[(full * 2) * 64 + c], slast = (double)part[(full * 2 + 1) * 64 + c];
  double sm = 0.0;
  for (int j = 0; j < full; ++j) sm += (double)part[(j * 2) * 64 + c];
  const double mu = (sm * (double)rpc + mlast * (double)nlast) / (double)R;
  double s2 = 0.0, q = 0.0;
  for (int j = 0; j < full; ++j) {
    const double d = (double)part[(j * 2) * 64 + c] - mu;
    s2 += (double)part[(j * 2 + 1) * 64 + c];
    q += d * d;
  }
  const double dl = mlast - mu;
  const double m2 = s2 + slast + (double)rpc * q + (double)nlast * (dl * dl);
  stat[c] = (float)mu;
  stat[64 + c] = (float)(m2 / (double)R);
}

/* out = relu(gamma (z - mu) rsqrt(var + eps) + beta (+ res)); 4096 elements per block */
__global__ __launch_bounds__(256) void fc_k_bn_apply(const float *__restrict__ Z, const float *__restrict__ res,
                                                     float *__restrict__ out, long n, int C, const float *__restrict__ bn,
                                                     const float *__restrict__ mean, const float *__restrict__ var) {
  const int c = threadIdx.x % C;
  const float mu = mean[c], rstd = 1.0f / sqrtf(var[c] + (float)CO_BN_EPS), ga = bn[c], be = bn[C + c];
  const long e0 = (long)blockIdx.x * 4096 + threadIdx.x;
#pragma unroll 4
  for (int k = 0; k < 16; ++k) {
    const long e = e0 + k * 256;
    if (e >= n) return;
    float y = ga * ((Z[e] - mu) * rstd) + be;
    if (res) y = y + res[e];
    out[e] = y > 0.0f ? y : 0.0f;
  }
}

/* The backward reductions and the per-channel constants made from them are float64.  In exact arithmetic dZ sums to 0
 * over the rows of a channel; a constant rounded to float32 and subtracted from every one of B * 16 rows leaves a sum
 * of that many half ulps instead, which the next layer's weight gradient multiplies by the mean of its input and every
 * beta along the residual path inherits.  With float64 sums of the float32 terms (sum xhat among them: it is 0 only as
 * far as the float32 mean is exact) and one rounding of each dZ, what is left is the rounding of dZ itself. */

/* chunk partials of sum dY, sum dY xhat and sum xhat, dY = dOut where out > 0 (written back when keep) */
__global__ __launch_bounds__(256) void fc_k_bnb_part(float *__restrict__ dOut, const float *__restrict__ out,
                                                     const float *__restrict__ Z, int R, int C, int rpc,
                                                     const float *__restrict__ stat, int keep, double *__restrict__ part) {
  __shared__ double red[256 + 64];
  const int c = threadIdx.x % C, rg = threadIdx.x / C, nrg = 256 / C;
  const int r0 = blockIdx.x * rpc, r1 = min(R, r0 + rpc);
  const float mu = stat[c], rstd = 1.0f / sqrtf(stat[64 + c] + (float)CO_BN_EPS);
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int r = r0 + rg; r < r1; r += nrg) {
    const long e = (long)r * C + c;
    const float dy = out[e] > 0.0f ? dOut[e] : 0.0f, xh = (Z[e] - mu) * rstd;
    if (keep) dOut[e] = dy;
    s1 += (double)dy;
    s2 += (double)dy * (double)xh;
    s3 += (double)xh;
  }
  s1 = fc_groupsum(red, s1, C);
  s2 = fc_groupsum(red, s2, C);
  s3 = fc_groupsum(red, s3, C);
  if (rg == 0) {
    part[(blockIdx.x * 3) * 64 + c] = s1;
    part[(blockIdx.x * 3 + 1) * 64 + c] = s2;
    part[(blockIdx.x * 3 + 2) * 64 + c] = s3;
  }
}

/* g[0..C) = dbias, g[C..2C) = dgamma, g[2C..3C) = dbeta.  The bias feeds a BatchNorm with batch statistics, which
 * removes any constant per channel: its gradient is identically zero and is written as such.  dgamma = sum dY (xhat -
 * mean xhat); fin[c] = dgamma / R, fin[64 + c] = mean dY - mean xhat dgamma / R: the two constants of fc_k_bnb_apply. */
__global__ __launch_bounds__(64) void fc_k_bnb_final(const double *__restrict__ part, int nch, int C, int R,
                                                     float *__restrict__ g, double *__restrict__ fin) {
  const int c = threadIdx.x;
  if (c >= C) return;
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int j = 0; j < nch; ++j) {
    s1 += part[(j * 3) * 64 + c];
    s2 += part[(j * 3 + 1) * 64 + c];
    s3 += part[(j * 3 + 2) * 64 + c];
  }
  /* xhat is centred on the float32 mean; what its own mean s3 / R still holds is taken out of dgamma too */
  const double dg = s2 - (s3 / R) * s1;
  g[c] = 0.0f;
  g[C + c] = (float)dg;
  g[2 * C + c] = (float)s1;
  fin[c] = dg / R;
  fin[64 + c] = s1 / R - (s3 / R) * (dg / R);
}

/* dZ = gamma rstd (dY - xhat mean(dY xhat) - (mean dY - mean xhat mean(dY xhat))), rounded once */
__global__ __launch_bounds__(256) void fc_k_bnb_apply(const float *__restrict__ dOut, const float *__restrict__ out,
                                                      const float *__restrict__ Z, float *__restrict__ dZ, long n, int C,
                                                      const float *__restrict__ bn, const float *__restrict__ stat,
                                                      const double *__restrict__ fin) {
  const int c = threadIdx.x % C;
  const float mu = stat[c], rstd = 1.0f / sqrtf(stat[64 + c] + (float)CO_BN_EPS);
  const double scale = (double)bn[c] * (double)rstd, mdyx = fin[c], mdy = fin[64 + c];
  const long e0 = (long)blockIdx.x * 4096 + threadIdx.x;
#pragma unroll 4
  for (int k = 0; k < 16; ++k) {
    const long e = e0 + k * 256;
    if (e >= n) return;
    const float dy = out[e] > 0.0f ? dOut[e] : 0.0f, xh = (Z[e] - mu) * rstd;
    dZ[e] = (float)(scale * ((double)dy - (double)xh * mdyx - mdy));
  }
}

/* ------------------------------------------------------------------ launchers */
static inline int fc_bn_rpc(int R) { return 128 * ((R + 128 * FC_BN_CHUNKS - 1) / (128 * FC_BN_CHUNKS)); }

/* x0[B * 16][16] = rescnn4's input planes of states[rows[r]] (nets.rescnn4_input_planes), channels 10..15 zero */
static void fc_planes(rt_stream_t s, const float *states, const int32_t *rows, int B, float *x0) {
  RT_LAUNCH(fc_k_planes, (unsigned)(((long)B * 16 * FC_IN_LD + 255) / 256), 256, s, states, rows, B, x0);
}

/* wt[l][tap][co][ci] = w[first + l * stride][8 - tap][ci][co] for the n 64 -> 64 kernels: the operand of backward-data */
static void fc_wtrans(rt_stream_t s, const float *w, int first, int stride, int n, float *wt) {
  RT_LAUNCH(fc_k_wtrans, (n * FC_WG_FLOATS + 255) / 256, 256, s, w, first, stride, n, wt);
}

/* out[row][co] (+)= bias[co] + sum over taps and ci of X[row shifted by the tap][ci] W[tap][ci][co]; cin = 10 reads X
 * with row stride FC_IN_LD, cin = 64 with FC_C.  bias may be null. */
static void fc_conv3(rt_stream_t s, const float *X, int cin, const float *W, const float *bias, float *out, int B,
                     int accumulate) {
  const int grid = (B + FC_POS - 1) / FC_POS;
  if (cin == FC_C)
    RT_LAUNCH(fc_k_conv3<FC_C>, grid, 256, s, X, W, cin, bias, out, B, accumulate);
  else
    RT_LAUNCH(fc_k_conv3<FC_IN_LD>, grid, 256, s, X, W, cin, bias, out, B, accumulate);
}

/* dW[tap][ci][co] = sum over rows of X[row shifted by the tap][ci] dZ[row][co]: per-chunk partials into part
 * ([FC_WG_CHUNKS][9 * cin * 64]), then their sum in chunk order into dW */
static void fc_conv3_wgrad(rt_stream_t s, const float *X, int cin, const float *dZ, int B, float *part, float *dW) {
  int ppc = (B + FC_WG_CHUNKS - 1) / FC_WG_CHUNKS;
  ppc = ppc < 16 ? 16 : (ppc + 3) / 4 * 4;
  const int nchunk = (B + ppc - 1) / ppc, n = 9 * cin * FC_C;
  if (cin == FC_C)
    RT_LAUNCH(fc_k_wgrad<FC_C>, dim3(nchunk, 3), 3 * FC_C * 4, s, X, dZ, B, ppc, cin, part);
  else
    RT_LAUNCH(fc_k_wgrad<FC_IN_LD>, dim3(nchunk, 3), 3 * FC_IN_LD * 4, s, X, dZ, B, ppc, cin, part);
  RT_LAUNCH(fc_k_wgrad_sum, (n + 255) / 256, 256, s, (const float *)part, nchunk, n, dW);
}

/* BatchNorm over the R rows of Z[R][C] (C in {64, 4, 2}), then + res (or null), then ReLU -> out.  bn = gamma, beta,
 * moving mean, moving variance, C floats each.  train: batch statistics, two stage (per-chunk mean and centred sum of
 * squares in part (FC_BN_SCRATCH floats), combined in chunk order), left in stat[0..C) and stat[64..64 + C); else the
 * moving ones. */
static void fc_bn_fwd(rt_stream_t s, const float *Z, const float *res, float *out, int R, int C, const float *bn, int train,
                      float *part, float *stat) {
  const long n = (long)R * C;
  const float *mean = bn + 2 * C, *var = bn + 3 * C;
  if (train) {
    const int rpc = fc_bn_rpc(R), nch = (R + rpc - 1) / rpc;
    RT_LAUNCH(fc_k_bn_part, nch, 256, s, Z, R, C, rpc, part);
    RT_LAUNCH(fc_k_bn_final, 1, 64, s, (const float *)part, nch, R, rpc, C, stat);
    mean = stat, var = stat + 64;
  }
  RT_LAUNCH(fc_k_bn_apply, (unsigned)((n + 4095) / 4096), 256, s, Z, res, out, n, C, bn, mean, var);
}

/* backward of the same: dOut is the gradient at `out`; dY = dOut where out > 0 (written back to dOut when keep: the
 * residual branch's share); dZ, and dbias (identically 0), dgamma, dbeta to g[0..3C) */
static void fc_bn_bwd(rt_stream_t s, float *dOut, const float *out, const float *Z, float *dZ, int R, int C, const float *bn,
                      const float *stat, int keep, float *part, float *g) {
  const long n = (long)R * C;
  const int rpc = fc_bn_rpc(R), nch = (R + rpc - 1) / rpc;
  RT_LAUNCH(fc_k_bnb_part, nch, 256, s, dOut, out, Z, R, C, rpc, stat, keep, (double *)part);
  double *dpart = (double *)part, *fin = dpart + FC_BN_PART; /* the backward partials are float64 */
  RT_LAUNCH(fc_k_bnb_final, 1, 64, s, (const double *)dpart, nch, C, R, g, fin);
  RT_LAUNCH(fc_k_bnb_apply, (unsigned)((n + 4095) / 4096), 256, s, (const float *)dOut, out, Z, dZ, n, C, bn, stat,
            (const double *)fin);
}

/* ------------------------------------------------------------------ the network */
#define FC_NBN ResCnnLayout::NBN /* BatchNorms of rescnn4: nine convolutions, the policy and the value head's 1x1 */
#define FC_STAT_LD 128  /* a BatchNorm's slot in stat: the batch mean at 0, the batch variance at 64 (fc_k_bn_final) */

/* hands out consecutive pieces of one allocation; with base null it only adds up their sizes */
struct FcCarver {
  float *base;
  size_t used = 0;
  float *take(size_t n) {
    float *p = base ? base + used : nullptr;
    used += n;
    return p;
  }
};

struct FtResCnn : FtNet {
  static constexpr ResCnnLayout L{}; /* the flat layout (nn_layout.h) */
  const size_t rows; /* max_batch rounded up to whole 16-row tiles */
  DevBuf<float> x0, act, wt, wpart, bnpart;
  /* pieces of act: activations are [rows * 16][C]; the heads' [rows * 16][4] and [rows * 16][2] are [rows][64] and
   * [rows][32] once flattened (pixel * C + channel) */
  float *Z[9], *X[5], *T[4];  /* convolution l's output before its BatchNorm; the stem's (0) and block b - 1's output;
                                 block b's first activation */
  float *G, *GB, *DZ;         /* the trunk's three gradient buffers */
  float *zp, *pa, *dpa, *dzp; /* policy head: the 1x1 convolution's output, its activation, and their gradients */
  float *zv, *va, *dva, *dzv; /* value head: the same */
  float *d1, *dd1;            /* the value head's dense layer of 64 and its gradient */

  void carve(FcCarver &c) {
    const size_t plane = rows * 16 * FC_C;
    for (float *&p : Z) p = c.take(plane);
    for (float *&p : X) p = c.take(plane);
    for (float *&p : T) p = c.take(plane);
    G = c.take(plane), GB = c.take(plane), DZ = c.take(plane);
    zp = c.take(rows * 16 * 4), pa = c.take(rows * 64), dpa = c.take(rows * 64), dzp = c.take(rows * 16 * 4);
    zv = c.take(rows * 16 * 2), va = c.take(rows * 32), dva = c.take(rows * 32), dzv = c.take(rows * 16 * 2);
    d1 = c.take(rows * 64), dd1 = c.take(rows * 64);
  }

  FtResCnn(int max_batch, rt_stream_t s) : rows((size_t)((max_batch + 15) / 16 * 16)) {
    FcCarver count{nullptr}, c{nullptr};
    carve(count);
    act.alloc(count.used, s);
    c.base = act.p;
    carve(c);
    x0.alloc(rows * 16 * FC_IN_LD, s);
    wt.alloc((size_t)8 * FC_WG_FLOATS, s);
    wpart.alloc((size_t)FC_WG_CHUNKS * FC_WG_FLOATS, s);
    bnpart.alloc((size_t)FC_BN_SCRATCH, s);
  }
  const char *name() const override { return "rescnn4"; }
  int num_weights() const override { return L.nw; }
  size_t stat_floats() const override { return (size_t)FC_NBN * FC_STAT_LD; }
  int policy_bias() const override { return L.p_db; }
  int value_bias() const override { return L.v_d2b; }
  void update_table(std::vector<int32_t> &sidx) const override {
    sidx.assign(L.nw, FT_WHOLE);
    for (int e = 0; e < 64 * CA_NUM_MOVES; ++e) sidx[L.p_dk + e] = FT_SPLIT0; /* products over the B rows */
    for (int e = 0; e < 32 * 64; ++e) sidx[L.v_d1k + e] = FT_SPLIT0;
    for (int e = 0; e < 64; ++e) sidx[L.v_d2k + e] = FT_SPLIT0;
    for (int e = 0; e < FC_C * 4; ++e) sidx[L.p_k + e] = FT_SPLIT1; /* products over the B * 16 (position, pixel) rows */
    for (int e = 0; e < FC_C * 2; ++e) sidx[L.v_k + e] = FT_SPLIT1;
    for (int j = 0; j < FC_NBN; ++j)
      for (int c = 0; c < L.channels(j); ++c) {
        sidx[L.mean(j) + c] = j * FC_STAT_LD + c;
        sidx[L.var(j) + c] = j * FC_STAT_LD + 64 + c;
      }
  }
  void tensor_table(std::vector<FtTensor> &t) const override {
    t.clear();
    /* BatchNorm j's five arrays behind its convolution's kernel */
    auto bn = [&](int j) {
      const int c = L.channels(j);
      t.push_back({L.bias(j), c, CA_TENSOR_BIAS});
      t.push_back({L.gamma(j), c, CA_TENSOR_GAMMA});
      t.push_back({L.beta(j), c, CA_TENSOR_BETA});
      t.push_back({L.mean(j), c, CA_TENSOR_MOVING});
      t.push_back({L.var(j), c, CA_TENSOR_MOVING});
    };
    for (int l = 0; l < L.CONVS; ++l) {
      t.push_back({L.kernel(l), 9 * L.cin(l) * FC_C, CA_TENSOR_TRUNK_KERNEL});
      bn(l);
    }
    t.push_back({L.p_k, FC_C * 4, CA_TENSOR_HEAD_KERNEL});
    bn(9);
    t.push_back({L.p_dk, 64 * CA_NUM_MOVES, CA_TENSOR_HEAD_KERNEL});
    t.push_back({L.p_db, CA_NUM_MOVES, CA_TENSOR_BIAS});
    t.push_back({L.v_k, FC_C * 2, CA_TENSOR_HEAD_KERNEL});
    bn(10);
    t.push_back({L.v_d1k, 32 * 64, CA_TENSOR_HEAD_KERNEL});
    t.push_back({L.v_d1b, 64, CA_TENSOR_BIAS});
    t.push_back({L.v_d2k, 64, CA_TENSOR_HEAD_KERNEL});
    t.push_back({L.v_d2b, 1, CA_TENSOR_BIAS});
  }

  void bn_fwd(const FtShared &sh, int j, const float *Zj, const float *res, float *out, int R, bool train) {
    fc_bn_fwd(sh.s, Zj, res, out, R, L.channels(j), sh.w + L.gamma(j), train ? 1 : 0, bnpart.p, sh.stat + j * FC_STAT_LD);
  }
  void bn_bwd(const FtShared &sh, int j, float *dOut, const float *out, const float *Zj, float *dZ, int R, bool keep) {
    fc_bn_bwd(sh.s, dOut, out, Zj, dZ, R, L.channels(j), sh.w + L.gamma(j), sh.stat + j * FC_STAT_LD, keep ? 1 : 0,
              bnpart.p, sh.g + L.bias(j));
  }

  void forward(const FtShared &sh, const int32_t *rws, int B, bool train) override {
    const int R = B * 16;
    rt_stream_t s = sh.s;
    float *w = sh.w;
    fc_planes(s, sh.states, rws, B, x0.p);
    fc_conv3(s, x0.p, 10, w + L.kernel(0), w + L.bias(0), Z[0], B, 0);
    bn_fwd(sh, 0, Z[0], nullptr, X[0], R, train);
    for (int b = 0; b < 4; ++b) {
      const int l1 = 1 + 2 * b, l2 = 2 + 2 * b;
      fc_conv3(s, X[b], FC_C, w + L.kernel(l1), w + L.bias(l1), Z[l1], B, 0);
      bn_fwd(sh, l1, Z[l1], nullptr, T[b], R, train);
      fc_conv3(s, T[b], FC_C, w + L.kernel(l2), w + L.bias(l2), Z[l2], B, 0);
      bn_fwd(sh, l2, Z[l2], X[b], X[b + 1], R, train);
    }
    /* policy: 1x1 convolution to 4 channels, BatchNorm, ReLU, flatten, dense to the 96 logits */
    FtGemm a = mk(X[4], FC_C, 1, w + L.p_k, 4, 1, zp, 4, 1, R, 4, FC_C);
    a.bias = w + L.bias(9);
    ft_gemm(s, a);
    bn_fwd(sh, 9, zp, nullptr, pa, R, train);
    a = mk(pa, 64, 1, w + L.p_dk, CA_NUM_MOVES, 1, sh.h, FT_PADW, 1, B, CA_NUM_MOVES, 64);
    a.bias = w + L.p_db;
    ft_gemm(s, a);
    /* value: 1x1 convolution to 2 channels, BatchNorm, ReLU, flatten, dense 32 -> 64, ReLU, dense 64 -> 1 */
    a = mk(X[4], FC_C, 1, w + L.v_k, 2, 1, zv, 2, 1, R, 2, FC_C);
    a.bias = w + L.bias(10);
    ft_gemm(s, a);
    bn_fwd(sh, 10, zv, nullptr, va, R, train);
    a = mk(va, 32, 1, w + L.v_d1k, 64, 1, d1, 64, 1, B, 64, 32);
    a.bias = w + L.v_d1b, a.relu = 1;
    ft_gemm(s, a);
    a = mk(d1, 64, 1, w + L.v_d2k, 1, 1, sh.h + 96, FT_PADW, 1, B, 1, 64);
    a.bias = w + L.v_d2b;
    ft_gemm(s, a);
  }

  FtSplits backward(const FtShared &sh, int B) override {
    const int R = B * 16, kb = ft_split_chunk(B), kr = ft_split_chunk(R), nw = L.nw;
    rt_stream_t s = sh.s;
    float *w = sh.w, *g = sh.g, *hd = sh.hd;
    /* policy head: dense kernel, its input's gradient, BatchNorm and ReLU, the 1x1 kernel, G = the trunk output's share */
    FtGemm a = mk(pa, 1, 64, hd, FT_PADW, 1, g + L.p_dk, CA_NUM_MOVES, 1, 64, CA_NUM_MOVES, B);
    a.kchunk = kb, a.c_split = nw;
    ft_gemm(s, a);
    ft_gemm(s, mk(hd, FT_PADW, 1, w + L.p_dk, 1, CA_NUM_MOVES, dpa, 64, 1, B, 64, CA_NUM_MOVES));
    bn_bwd(sh, 9, dpa, pa, zp, dzp, R, false);
    a = mk(X[4], 1, FC_C, dzp, 4, 1, g + L.p_k, 4, 1, FC_C, 4, R);
    a.kchunk = kr, a.c_split = nw;
    ft_gemm(s, a);
    ft_gemm(s, mk(dzp, 4, 1, w + L.p_k, 1, 4, G, FC_C, 1, R, FC_C, 4));
    /* value head, added to G */
    a = mk(d1, 1, 64, hd + 96, FT_PADW, 1, g + L.v_d2k, 1, 1, 64, 1, B);
    a.kchunk = kb, a.c_split = nw;
    ft_gemm(s, a);
    ft_gemm(s, mk(hd + 96, FT_PADW, 1, w + L.v_d2k, 1, 1, dd1, 64, 1, B, 64, 1));
    ft_relu_bwd(s, dd1, d1, B, 64, 64, g + L.v_d1b);
    a = mk(va, 1, 32, dd1, 64, 1, g + L.v_d1k, 64, 1, 32, 64, B);
    a.kchunk = kb, a.c_split = nw;
    ft_gemm(s, a);
    ft_gemm(s, mk(dd1, 64, 1, w + L.v_d1k, 1, 64, dva, 32, 1, B, 32, 64));
    bn_bwd(sh, 10, dva, va, zv, dzv, R, false);
    a = mk(X[4], 1, FC_C, dzv, 2, 1, g + L.v_k, 2, 1, FC_C, 2, R);
    a.kchunk = kr, a.c_split = nw;
    ft_gemm(s, a);
    a = mk(dzv, 2, 1, w + L.v_k, 1, 2, G, FC_C, 1, R, FC_C, 2);
    a.accumulate = 1;
    ft_gemm(s, a);
    /* trunk: G is the gradient at block b's output.  Its ReLU-masked copy (kept in G) is both the second BatchNorm's
     * input gradient and the residual branch's share of the block input's gradient, to which backward-data of the
     * first convolution is added */
    fc_wtrans(s, w, L.kernel(1), L.kernel(2) - L.kernel(1), 8, wt.p);
    for (int b = 3; b >= 0; --b) {
      const int l1 = 1 + 2 * b, l2 = 2 + 2 * b;
      bn_bwd(sh, l2, G, X[b + 1], Z[l2], DZ, R, true);
      fc_conv3_wgrad(s, T[b], FC_C, DZ, B, wpart.p, g + L.kernel(l2));
      fc_conv3(s, DZ, FC_C, wt.p + (size_t)(l2 - 1) * FC_WG_FLOATS, nullptr, GB, B, 0);
      bn_bwd(sh, l1, GB, T[b], Z[l1], DZ, R, false);
      fc_conv3_wgrad(s, X[b], FC_C, DZ, B, wpart.p, g + L.kernel(l1));
      fc_conv3(s, DZ, FC_C, wt.p + (size_t)(l1 - 1) * FC_WG_FLOATS, nullptr, G, B, 1);
    }
    bn_bwd(sh, 0, G, X[0], Z[0], DZ, R, false);
    fc_conv3_wgrad(s, x0.p, 10, DZ, B, wpart.p, g + L.kernel(0));
    return {(B + kb - 1) / kb, (R + kr - 1) / kr};
  }
};

FtNet *ft_rescnn_create(int max_batch, rt_stream_t s) { return new FtResCnn(max_batch, s); }
