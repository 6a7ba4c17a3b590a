// nn_train.hip -- network training: the reference's Keras fit step (main.pyx:221-272, model and compile of
// wrapper.py:256-282) for mlp12x100, in float32 on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32).
//
// One training step of a batch of B rows ("Network training"):
//   gather      X0 = states[rows] (rows of the epoch's permutation)                           1 launch
//   forward     per layer: Z = X W + b, ReLU -> A_l (ft_k_gemm);  BatchNorm with batch statistics
//               (mean, biased variance) -> Y_l (ft_k_bn_fwd)                                       24 launches
//   heads       logits = Y_11 Kp + bp, v = Y_11 Kv + bv (two ft_k_gemm)                          2 launches
//   loss        per row: (tanh v - z)^2, -sum t log_softmax, and their gradients (ft_k_loss);
//               column sums of the head gradients and of the loss terms (ft_k_head_reduce)     2 launches
//   backward    head kernel gradients and dY_11 (four ft_k_gemm); per layer: BatchNorm and ReLU
//               backward with dgamma, dbeta, dbias (ft_k_bn_bwd), dW = X^T dZ (ft_k_gemm, split over
//               the rows), dX = dZ W^T (ft_k_gemm)                                                39 launches
//   update      sum of the split partials in a fixed order, Adam (TF ResourceApplyAdam) on kernels, biases,
//               gamma and beta, moving statistics from the batch statistics (ft_k_update)      1 launch
// Every cross-workgroup sum is written as partials and combined in a fixed order by a later launch: no float atomics,
// no grid-wide barriers, so a step is bitwise reproducible.  The weights live in the Keras get_weights() layout
// (nn.h) and the kernels read them there with bounds checks, so there is no padded copy to keep in step.
//
// rescnn4 (ca_fitter_create_net with CA_NET_RESCNN4) is trained by the same recipe on the network of nets.py: the
// convolutions and the BatchNorm over channels are the kernels of nn_train_conv.hip, the 1x1 convolutions and dense
// layers of the heads go through ft_k_gemm, and the data, loss, Adam and guard code below is shared by both networks.
#include <hip/hip_runtime.h>
#include <math.h>

#include <string>
#include <vector>

#include "../../include/corintho_hip.h"
#include "nn.h"
#include "nn_train_conv.h"

#define FT_PADW 112    /* activation row stride: 100 features padded to 7 tiles of 16 */
#define FT_IN_LD 80    /* gathered input row stride: 70 padded to 5 tiles */
#define FT_NSPLIT 16   /* at most this many row chunks per weight gradient (partials of ft_k_gemm) */
#define FT_BN_RG 64    /* row groups of the column kernels: 16 features x 64 = 1024 threads */
#define FT_NW CO_MLP_NUM_WEIGHTS
#define FT_HEAD (7500 + 11 * 10500) /* offset of the value head kernel */
#define FT_KV FT_HEAD
#define FT_BV (FT_HEAD + 100)
#define FT_KP (FT_HEAD + 101)
#define FT_BP (FT_HEAD + 101 + 9600)

typedef float f32x4 __attribute__((ext_vector_type(4)));

void co_set_last_error(const std::string &m);

static inline int ft_in_dim(int l) { return l == 0 ? CA_GAME_STATE_SIZE : CO_MLP_WIDTH; }
/* flat offset of layer l's kernel; bias, gamma, beta, moving mean, moving variance follow, 100 floats each */
static inline int ft_base(int l) { return l == 0 ? 0 : 7500 + (l - 1) * 10500; }
static inline int ft_off(int l, int part /* 0 bias .. 4 variance */) { return ft_base(l) + ft_in_dim(l) * 100 + 100 * part; }

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

/* X0[r][k] = states[rows[r]][k], k < 70 */
__global__ __launch_bounds__(256) void ft_k_gather(const float *__restrict__ states, const int32_t *__restrict__ rows,
                                                   int B, float *__restrict__ x0) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * CA_GAME_STATE_SIZE) return;
  const int r = e / CA_GAME_STATE_SIZE, k = e % CA_GAME_STATE_SIZE;
  x0[(long)r * FT_IN_LD + k] = states[(long)rows[r] * CA_GAME_STATE_SIZE + k];
}

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

/* Per row of the heads' outputs H[r] (96 logits, value at 96): the loss terms and the gradients of the batch loss
 * value_mse + 0.25 * policy_cce (means over the B rows) with respect to the logits and to v:
 *   Hd[r][0..95] = 0.25 (softmax * sum t - t) / B,  Hd[r][96] = 2 (tanh v - z)(1 - tanh^2 v) / B,
 *   Hd[r][97] = (tanh v - z)^2,  Hd[r][98] = -sum_j t_j log_softmax_j  (from the logits, as Keras does) */
__global__ __launch_bounds__(256) void ft_k_loss(const float *__restrict__ H, const int32_t *__restrict__ rows, int B,
                                                const float *__restrict__ evals, const float *__restrict__ probs,
                                                float *__restrict__ Hd) {
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
  for (int j = 0; j < CA_NUM_MOVES; ++j) d[j] = 0.25f * (expf(h[j] - lse) * st - t[j]) * inv_b;
  const float tv = tanhf(h[96]);
  const float err = tv - evals[rows[r]];
  d[96] = 2.0f * err * (1.0f - tv * tv) * inv_b;
  d[97] = err * err;
  d[98] = ce;
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
 * epsilon outside the root); sidx[i] >= 0: a moving statistic, moved toward the batch statistic stat[sidx[i]] with
 * momentum 0.99.  apply = 0: write the summed gradient to gout only. */
#define FT_SPLIT0 -1
#define FT_SPLIT1 -2
#define FT_WHOLE -3
__global__ __launch_bounds__(256) void ft_k_update(float *__restrict__ w, float *__restrict__ m, float *__restrict__ v,
                                                  const float *__restrict__ g, int nw, int ns0, int ns1,
                                                  const int32_t *__restrict__ sidx, const float *__restrict__ stat,
                                                  float lr_t, int apply, float *__restrict__ gout) {
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
    w[i] = mv - (mv - stat[si]) * 0.01f;
    return;
  }
  float s = 0.0f;
  for (int k = 0; k < nsplit; ++k) s += g[(long)k * nw + i];
  const float mt = m[i] + (s - m[i]) * (1.0f - 0.9f);
  const float vt = v[i] + (s * s - v[i]) * (1.0f - 0.999f);
  m[i] = mt;
  v[i] = vt;
  w[i] = w[i] - lr_t * mt / (sqrtf(vt) + 1e-7f);
}

/* ------------------------------------------------------------------ host */
namespace {

template <typename T>
struct FtBuf {
  T *p = nullptr;
  FtBuf() = default;
  FtBuf(const FtBuf &) = delete;
  FtBuf &operator=(const FtBuf &) = delete;
  ~FtBuf() { rt_free(p); }
  void alloc(size_t n, rt_stream_t s) {
    rt_free(p);
    p = nullptr;
    rt_malloc((void **)&p, n * sizeof(T), s);
  }
};

struct FtError : std::runtime_error {
  int code;
  FtError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

}  // namespace

/* rescnn4's flat layout (nets._rescnn4_shapes): convolution l = 0 (stem) .. 8 has its kernel at conv_k[l] and bias,
 * gamma, beta, moving mean, moving variance (64 each) from conv_b[l]; the heads' 1x1 convolutions likewise with 4 and 2
 * channels from p_b and v_b */
struct FcLayout {
  int conv_k[9], conv_b[9];
  int p_k, p_b, p_dk, p_db, v_k, v_b, v_d1k, v_d1b, v_d2k, v_d2b, nw;
  FcLayout() {
    int p = 0;
    for (int l = 0; l < 9; ++l) {
      conv_k[l] = p;
      p += 9 * (l == 0 ? 10 : FC_C) * FC_C;
      conv_b[l] = p;
      p += 5 * FC_C;
    }
    p_k = p, p_b = p_k + FC_C * 4, p_dk = p_b + 5 * 4, p_db = p_dk + 64 * CA_NUM_MOVES;
    v_k = p_db + CA_NUM_MOVES, v_b = v_k + FC_C * 2, v_d1k = v_b + 5 * 2, v_d1b = v_d1k + 32 * 64;
    v_d2k = v_d1b + 64, v_d2b = v_d2k + 64, nw = v_d2b + 1;
  }
};
#define FC_NBN 11 /* BatchNorms of rescnn4: nine convolutions, the policy and the value head's 1x1 */

struct ca_fitter {
  int device = 0;
  int net = CA_NET_MLP12X100;
  int nw = FT_NW; /* floats of the weight vector */
  FcLayout L;
  int max_batch = 0;
  int64_t iterations = 0;
  int32_t n = 0, idx_cap = 0;
  rt_stream_t s = nullptr;
  FtBuf<float> w, m, v, g, gsum, stat, x0, act, y, h, hd, dy, dz, loss;
  FtBuf<float> states, evals, probs;
  FtBuf<int32_t> sidx, idx;
  /* rescnn4: the trunk's activations (nine Z, five X, four T), its three gradient buffers (G, GB, DZ), the heads' small
   * buffers, the mirrored transposed kernels and the partials of the two-stage reductions */
  FtBuf<float> cact, cgrad, chead, wt, wpart, bnpart;
  std::vector<float> hloss;

  void init(int dev, int kind, int mb) {
    device = dev;
    net = kind;
    max_batch = mb;
    nw = kind == CA_NET_RESCNN4 ? L.nw : FT_NW;
    rt_set_device(dev);
    rt_stream_create(&s);
    const size_t rows = (size_t)((mb + 15) / 16 * 16);
    w.alloc(nw, s);
    m.alloc(nw, s);
    v.alloc(nw, s);
    g.alloc((size_t)FT_NSPLIT * nw, s);
    gsum.alloc(nw, s);
    h.alloc(rows * FT_PADW, s);
    hd.alloc(rows * FT_PADW, s);
    /* stat index of every weight: < 0 trainable (the number of its gradient partials, ft_k_update), else the batch
     * statistic its moving average follows */
    std::vector<int32_t> si(nw, FT_SPLIT0);
    if (kind == CA_NET_RESCNN4) {
      stat.alloc((size_t)FC_NBN * 128, s);
      x0.alloc(rows * 16 * FC_IN_LD, s);
      cact.alloc((size_t)18 * rows * 16 * FC_C, s);
      cgrad.alloc((size_t)3 * rows * 16 * FC_C, s);
      chead.alloc(rows * (size_t)(2 * 64 + 4 * 64 + 4 * 32), s);
      wt.alloc((size_t)8 * FC_WG_FLOATS, s);
      wpart.alloc((size_t)FC_WG_CHUNKS * FC_WG_FLOATS, s);
      bnpart.alloc((size_t)FC_BN_SCRATCH, s);
      si.assign(nw, FT_WHOLE);
      for (int e = 0; e < 64 * CA_NUM_MOVES; ++e) si[L.p_dk + e] = FT_SPLIT0; /* products over the B rows */
      for (int e = 0; e < 32 * 64; ++e) si[L.v_d1k + e] = FT_SPLIT0;
      for (int e = 0; e < 64; ++e) si[L.v_d2k + e] = FT_SPLIT0;
      for (int e = 0; e < FC_C * 4; ++e) si[L.p_k + e] = FT_SPLIT1; /* products over the B * 16 (position, pixel) rows */
      for (int e = 0; e < FC_C * 2; ++e) si[L.v_k + e] = FT_SPLIT1;
      for (int j = 0; j < FC_NBN; ++j) {
        const int C = bn_c(j), mean = bn_w(j) + 2 * C;
        for (int c = 0; c < C; ++c) {
          si[mean + c] = j * 128 + c;
          si[mean + C + c] = j * 128 + 64 + c;
        }
      }
    } else {
      stat.alloc((size_t)2 * CO_MLP_LAYERS * FT_PADW, s);
      x0.alloc(rows * FT_IN_LD, s);
      act.alloc((size_t)CO_MLP_LAYERS * rows * FT_PADW, s);
      y.alloc((size_t)CO_MLP_LAYERS * rows * FT_PADW, s);
      dy.alloc(rows * FT_PADW, s);
      dz.alloc(rows * FT_PADW, s);
      for (int l = 0; l < CO_MLP_LAYERS; ++l)
        for (int f = 0; f < CO_MLP_WIDTH; ++f) {
          si[ft_off(l, 3) + f] = 2 * l * FT_PADW + f;
          si[ft_off(l, 4) + f] = (2 * l + 1) * FT_PADW + f;
        }
    }
    sidx.alloc(nw, s);
    rt_h2d(sidx.p, si.data(), nw * sizeof(int32_t), s);
    rt_sync(s);
  }
  ~ca_fitter() { rt_stream_destroy(s); }

  /* rescnn4's BatchNorm j: channels, and the offset of its gamma (beta, moving mean, moving variance follow) */
  int bn_c(int j) const { return j < 9 ? FC_C : j == 9 ? 4 : 2; }
  int bn_w(int j) const { return (j < 9 ? L.conv_b[j] : j == 9 ? L.p_b : L.v_b) + bn_c(j); }
  size_t crows() const { return (size_t)((max_batch + 15) / 16 * 16) * 16; }
  float *cZ(int l) { return cact.p + (size_t)l * crows() * FC_C; }        /* convolution l's output, before its BatchNorm */
  float *cX(int b) { return cact.p + (size_t)(9 + b) * crows() * FC_C; }  /* the stem's (0) and block b - 1's output */
  float *cT(int b) { return cact.p + (size_t)(14 + b) * crows() * FC_C; } /* block b's first activation */
  float *cG(int k) { return cgrad.p + (size_t)k * crows() * FC_C; }
  /* the heads: [B * 16][4] and [B * 16][2] are [B][64] and [B][32] once flattened (pixel * C + channel) */
  float *hb(int k) { return chead.p + (size_t)k * crows() * 2; }
  float *h_zp() { return hb(0); }
  float *h_pa() { return hb(2); }
  float *h_dpa() { return hb(4); }
  float *h_dzp() { return hb(6); }
  float *h_zv() { return hb(8); }
  float *h_va() { return hb(9); }
  float *h_dva() { return hb(10); }
  float *h_dzv() { return hb(11); }
  float *h_d1() { return hb(12); }
  float *h_dd1() { return hb(14); }

  size_t rows_ld() const { return (size_t)((max_batch + 15) / 16 * 16) * FT_PADW; }
  float *A(int l) { return act.p + l * rows_ld(); }
  float *Y(int l) { return y.p + l * rows_ld(); }
  float *st(int l) { return stat.p + 2 * l * FT_PADW; }

  void gemm(const FtGemm &a) {
    const int tiles = ((a.M + 15) / 16) * ((a.N + 15) / 16) * ((a.K + a.kchunk - 1) / a.kchunk);
    if (tiles == 0) return;
    hipLaunchKernelGGL(ft_k_gemm, dim3((tiles + 3) / 4), dim3(256), 0, s, a);
    RT_CHECK(hipGetLastError());
  }
  static FtGemm mk(const float *A, long sam, long sak, const float *B, long sbk, long sbn, float *C, long scm, long scn,
                   int M, int N, int K) {
    FtGemm a;
    a.A = A, a.sam = sam, a.sak = sak, a.B = B, a.sbk = sbk, a.sbn = sbn, a.C = C, a.scm = scm, a.scn = scn;
    a.c_split = 0, a.M = M, a.N = N, a.K = K, a.kchunk = K > 0 ? K : 1, a.bias = nullptr, a.relu = 0, a.accumulate = 0;
    return a;
  }

  /* forward of rows idx[0..B) (a device pointer); train = batch statistics.  Leaves H = heads' outputs. */
  void forward(const int32_t *rows, int B, bool train) {
    if (net == CA_NET_RESCNN4)
      cnn_forward(rows, B, train);
    else
      mlp_forward(rows, B, train);
  }
  /* the weight gradient of one batch as partials in g; leaves their counts in ns0, ns1 (ft_k_update) */
  void backward(int B) {
    if (net == CA_NET_RESCNN4)
      cnn_backward(B);
    else
      ns0 = ns1 = mlp_backward(B);
  }
  int ns0 = 1, ns1 = 1;
  static int split_chunk(int K) { /* rows of one of at most FT_NSPLIT chunks of K, a multiple of 16 */
    const int kch = (K + FT_NSPLIT - 1) / FT_NSPLIT;
    return (kch + 15) / 16 * 16;
  }

  void bn_fwd(int j, const float *Z, const float *res, float *out, int R, bool train) {
    fc_bn_fwd(s, Z, res, out, R, bn_c(j), w.p + bn_w(j), train ? 1 : 0, bnpart.p, stat.p + j * 128);
  }
  void bn_bwd(int j, float *dOut, const float *out, const float *Z, float *dZ, int R, bool keep) {
    fc_bn_bwd(s, dOut, out, Z, dZ, R, bn_c(j), w.p + bn_w(j), stat.p + j * 128, keep ? 1 : 0, bnpart.p,
              g.p + bn_w(j) - bn_c(j));
  }

  void cnn_forward(const int32_t *rows, int B, bool train) {
    const int R = B * 16;
    fc_planes(s, states.p, rows, B, x0.p);
    fc_conv3(s, x0.p, 10, w.p + L.conv_k[0], w.p + L.conv_b[0], cZ(0), B, 0);
    bn_fwd(0, cZ(0), nullptr, cX(0), R, train);
    for (int b = 0; b < 4; ++b) {
      const int l1 = 1 + 2 * b, l2 = 2 + 2 * b;
      fc_conv3(s, cX(b), FC_C, w.p + L.conv_k[l1], w.p + L.conv_b[l1], cZ(l1), B, 0);
      bn_fwd(l1, cZ(l1), nullptr, cT(b), R, train);
      fc_conv3(s, cT(b), FC_C, w.p + L.conv_k[l2], w.p + L.conv_b[l2], cZ(l2), B, 0);
      bn_fwd(l2, cZ(l2), cX(b), cX(b + 1), R, train);
    }
    /* policy: 1x1 convolution to 4 channels, BatchNorm, ReLU, flatten, dense to the 96 logits */
    FtGemm a = mk(cX(4), FC_C, 1, w.p + L.p_k, 4, 1, h_zp(), 4, 1, R, 4, FC_C);
    a.bias = w.p + L.p_b;
    gemm(a);
    bn_fwd(9, h_zp(), nullptr, h_pa(), R, train);
    a = mk(h_pa(), 64, 1, w.p + L.p_dk, CA_NUM_MOVES, 1, h.p, FT_PADW, 1, B, CA_NUM_MOVES, 64);
    a.bias = w.p + L.p_db;
    gemm(a);
    /* value: 1x1 convolution to 2 channels, BatchNorm, ReLU, flatten, dense 32 -> 64, ReLU, dense 64 -> 1 */
    a = mk(cX(4), FC_C, 1, w.p + L.v_k, 2, 1, h_zv(), 2, 1, R, 2, FC_C);
    a.bias = w.p + L.v_b;
    gemm(a);
    bn_fwd(10, h_zv(), nullptr, h_va(), R, train);
    a = mk(h_va(), 32, 1, w.p + L.v_d1k, 64, 1, h_d1(), 64, 1, B, 64, 32);
    a.bias = w.p + L.v_d1b, a.relu = 1;
    gemm(a);
    a = mk(h_d1(), 64, 1, w.p + L.v_d2k, 1, 1, h.p + 96, FT_PADW, 1, B, 1, 64);
    a.bias = w.p + L.v_d2b;
    gemm(a);
  }

  void cnn_backward(int B) {
    const int R = B * 16, kb = split_chunk(B), kr = split_chunk(R);
    ns0 = (B + kb - 1) / kb, ns1 = (R + kr - 1) / kr;
    float *G = cG(0), *GB = cG(1), *DZ = cG(2);
    /* policy head: dense kernel, its input's gradient, BatchNorm and ReLU, the 1x1 kernel, G = the trunk output's share */
    FtGemm a = mk(h_pa(), 1, 64, hd.p, FT_PADW, 1, g.p + L.p_dk, CA_NUM_MOVES, 1, 64, CA_NUM_MOVES, B);
    a.kchunk = kb, a.c_split = nw;
    gemm(a);
    gemm(mk(hd.p, FT_PADW, 1, w.p + L.p_dk, 1, CA_NUM_MOVES, h_dpa(), 64, 1, B, 64, CA_NUM_MOVES));
    bn_bwd(9, h_dpa(), h_pa(), h_zp(), h_dzp(), R, false);
    a = mk(cX(4), 1, FC_C, h_dzp(), 4, 1, g.p + L.p_k, 4, 1, FC_C, 4, R);
    a.kchunk = kr, a.c_split = nw;
    gemm(a);
    gemm(mk(h_dzp(), 4, 1, w.p + L.p_k, 1, 4, G, FC_C, 1, R, FC_C, 4));
    /* value head, added to G */
    a = mk(h_d1(), 1, 64, hd.p + 96, FT_PADW, 1, g.p + L.v_d2k, 1, 1, 64, 1, B);
    a.kchunk = kb, a.c_split = nw;
    gemm(a);
    gemm(mk(hd.p + 96, FT_PADW, 1, w.p + L.v_d2k, 1, 1, h_dd1(), 64, 1, B, 64, 1));
    hipLaunchKernelGGL(ft_k_relu_bwd, dim3(4), dim3(1024), 0, s, h_dd1(), (const float *)h_d1(), B, 64, 64, g.p + L.v_d1b);
    RT_CHECK(hipGetLastError());
    a = mk(h_va(), 1, 32, h_dd1(), 64, 1, g.p + L.v_d1k, 64, 1, 32, 64, B);
    a.kchunk = kb, a.c_split = nw;
    gemm(a);
    gemm(mk(h_dd1(), 64, 1, w.p + L.v_d1k, 1, 64, h_dva(), 32, 1, B, 32, 64));
    bn_bwd(10, h_dva(), h_va(), h_zv(), h_dzv(), R, false);
    a = mk(cX(4), 1, FC_C, h_dzv(), 2, 1, g.p + L.v_k, 2, 1, FC_C, 2, R);
    a.kchunk = kr, a.c_split = nw;
    gemm(a);
    a = mk(h_dzv(), 2, 1, w.p + L.v_k, 1, 2, G, FC_C, 1, R, FC_C, 2);
    a.accumulate = 1;
    gemm(a);
    /* trunk: G is the gradient at block b's output.  Its ReLU-masked copy (kept in G) is both the second BatchNorm's
     * input gradient and the residual branch's share of the block input's gradient, to which backward-data of the
     * first convolution is added */
    fc_wtrans(s, w.p, L.conv_k[1], L.conv_k[2] - L.conv_k[1], 8, wt.p);
    for (int b = 3; b >= 0; --b) {
      const int l1 = 1 + 2 * b, l2 = 2 + 2 * b;
      bn_bwd(l2, G, cX(b + 1), cZ(l2), DZ, R, true);
      fc_conv3_wgrad(s, cT(b), FC_C, DZ, B, wpart.p, g.p + L.conv_k[l2]);
      fc_conv3(s, DZ, FC_C, wt.p + (size_t)(l2 - 1) * FC_WG_FLOATS, nullptr, GB, B, 0);
      bn_bwd(l1, GB, cT(b), cZ(l1), DZ, R, false);
      fc_conv3_wgrad(s, cX(b), FC_C, DZ, B, wpart.p, g.p + L.conv_k[l1]);
      fc_conv3(s, DZ, FC_C, wt.p + (size_t)(l1 - 1) * FC_WG_FLOATS, nullptr, G, B, 1);
    }
    bn_bwd(0, G, cX(0), cZ(0), DZ, R, false);
    fc_conv3_wgrad(s, x0.p, 10, DZ, B, wpart.p, g.p + L.conv_k[0]);
  }

  void mlp_forward(const int32_t *rows, int B, bool train) {
    hipLaunchKernelGGL(ft_k_gather, dim3((B * CA_GAME_STATE_SIZE + 255) / 256), dim3(256), 0, s, (const float *)states.p,
                       rows, B, x0.p);
    RT_CHECK(hipGetLastError());
    for (int l = 0; l < CO_MLP_LAYERS; ++l) {
      const float *X = l == 0 ? x0.p : Y(l - 1);
      const long ld = l == 0 ? FT_IN_LD : FT_PADW;
      FtGemm a = mk(X, ld, 1, w.p + ft_base(l), 100, 1, A(l), FT_PADW, 1, B, CO_MLP_WIDTH, ft_in_dim(l));
      a.bias = w.p + ft_off(l, 0);
      a.relu = 1;
      gemm(a);
      hipLaunchKernelGGL(ft_k_bn_fwd, dim3(FT_PADW / 16), dim3(1024), 0, s, (const float *)A(l), Y(l), B,
                         (const float *)w.p, ft_off(l, 1), train ? 1 : 0, st(l));
      RT_CHECK(hipGetLastError());
    }
    FtGemm p = mk(Y(11), FT_PADW, 1, w.p + FT_KP, CA_NUM_MOVES, 1, h.p, FT_PADW, 1, B, CA_NUM_MOVES, CO_MLP_WIDTH);
    p.bias = w.p + FT_BP;
    gemm(p);
    FtGemm vh = mk(Y(11), FT_PADW, 1, w.p + FT_KV, 1, 1, h.p + 96, FT_PADW, 1, B, 1, CO_MLP_WIDTH);
    vh.bias = w.p + FT_BV;
    gemm(vh);
  }

  /* loss terms of the batch (and the logit / value gradients in Hd); loss sums to loss.p[2 * slot] */
  void loss_terms(const int32_t *rows, int B, bool grads, int slot) {
    hipLaunchKernelGGL(ft_k_loss, dim3((B + 255) / 256), dim3(256), 0, s, (const float *)h.p, rows, B,
                       (const float *)evals.p, (const float *)probs.p, hd.p);
    RT_CHECK(hipGetLastError());
    const bool cnn = net == CA_NET_RESCNN4;
    hipLaunchKernelGGL(ft_k_head_reduce, dim3(FT_PADW / 16), dim3(1024), 0, s, (const float *)hd.p, B,
                       grads ? g.p : (float *)nullptr, cnn ? L.p_db : FT_BP, cnn ? L.v_d2b : FT_BV, loss.p + 2 * slot);
    RT_CHECK(hipGetLastError());
  }

  /* the weight gradient of one batch as FT_NSPLIT-bounded partials in g; returns the number of partials */
  int mlp_backward(int B) {
    const int kch = split_chunk(B);
    const int nsplit = (B + kch - 1) / kch;
    /* heads: dKp = Y11^T Hd[:, :96], dKv = Y11^T Hd[:, 96] (row-split partials) */
    FtGemm a = mk(Y(11), 1, FT_PADW, hd.p, FT_PADW, 1, g.p + FT_KP, CA_NUM_MOVES, 1, CO_MLP_WIDTH, CA_NUM_MOVES, B);
    a.kchunk = kch, a.c_split = FT_NW;
    gemm(a);
    a = mk(Y(11), 1, FT_PADW, hd.p + 96, FT_PADW, 1, g.p + FT_KV, 1, 1, CO_MLP_WIDTH, 1, B);
    a.kchunk = kch, a.c_split = FT_NW;
    gemm(a);
    /* dY11 = Hd[:, :96] Kp^T + Hd[:, 96] Kv^T */
    gemm(mk(hd.p, FT_PADW, 1, w.p + FT_KP, 1, CA_NUM_MOVES, dy.p, FT_PADW, 1, B, CO_MLP_WIDTH, CA_NUM_MOVES));
    a = mk(hd.p + 96, FT_PADW, 1, w.p + FT_KV, 1, 1, dy.p, FT_PADW, 1, B, CO_MLP_WIDTH, 1);
    a.accumulate = 1;
    gemm(a);
    for (int l = CO_MLP_LAYERS - 1; l >= 0; --l) {
      hipLaunchKernelGGL(ft_k_bn_bwd, dim3(FT_PADW / 16), dim3(1024), 0, s, (const float *)dy.p, (const float *)A(l), dz.p,
                         B, (const float *)w.p, ft_off(l, 0), (const float *)st(l), g.p);
      RT_CHECK(hipGetLastError());
      const float *X = l == 0 ? x0.p : Y(l - 1);
      const long ld = l == 0 ? FT_IN_LD : FT_PADW;
      a = mk(X, 1, ld, dz.p, FT_PADW, 1, g.p + ft_base(l), CO_MLP_WIDTH, 1, ft_in_dim(l), CO_MLP_WIDTH, B);
      a.kchunk = kch, a.c_split = FT_NW;
      gemm(a);
      if (l > 0) gemm(mk(dz.p, FT_PADW, 1, w.p + ft_base(l), 1, CO_MLP_WIDTH, dy.p, FT_PADW, 1, B, CO_MLP_WIDTH, CO_MLP_WIDTH));
    }
    return nsplit;
  }

  void update(float lr_t, bool apply) {
    hipLaunchKernelGGL(ft_k_update, dim3((nw + 255) / 256), dim3(256), 0, s, w.p, m.p, v.p, (const float *)g.p, nw, ns0, ns1,
                       (const int32_t *)sidx.p, (const float *)stat.p, lr_t, apply ? 1 : 0, gsum.p);
    RT_CHECK(hipGetLastError());
  }

  void need_data() {
    if (n <= 0) throw FtError(CA_ERR_STATE, "ca_fitter: no data (ca_fitter_set_data)");
  }
  void check_rows(const int32_t *rows, int32_t nr) {
    if (nr < 0 || nr > idx_cap) throw FtError(CA_ERR_ARG, "ca_fitter: more rows than the data set holds");
    for (int32_t i = 0; i < nr; ++i)
      if (rows[i] < 0 || rows[i] >= n) throw FtError(CA_ERR_ARG, "ca_fitter: row index out of range");
  }
  void check_batch(int32_t batch) {
    if (batch < 1 || batch > max_batch) throw FtError(CA_ERR_ARG, "ca_fitter: batch must be in [1, max_batch]");
  }
  void ensure_loss(int slots) {
    if ((int)hloss.size() < 2 * slots) {
      loss.alloc((size_t)2 * slots, s);
      hloss.assign((size_t)2 * slots, 0.0f);
    }
  }
  /* per-batch sums -> out[3] = {value + 0.25 policy, value, policy}, means weighted by batch size; per[3 * b] */
  void losses(int nb, int32_t nr, int32_t batch, double *out, float *per) {
    rt_d2h(hloss.data(), loss.p, (size_t)2 * nb * sizeof(float), s);
    rt_sync(s);
    double sv = 0.0, sp = 0.0;
    for (int b = 0; b < nb; ++b) {
      const int rb = b * batch + batch <= nr ? batch : nr - b * batch;
      const float lv = hloss[2 * b] / (float)rb, lp = hloss[2 * b + 1] / (float)rb;
      if (per) {
        per[3 * b] = lv + 0.25f * lp;
        per[3 * b + 1] = lv;
        per[3 * b + 2] = lp;
      }
      sv += (double)lv * rb;
      sp += (double)lp * rb;
    }
    if (out) {
      out[1] = nr ? sv / nr : 0.0;
      out[2] = nr ? sp / nr : 0.0;
      out[0] = out[1] + 0.25 * out[2];
    }
  }
};

#define FT_GUARD(...)                     \
  try {                                   \
    if (!f) throw FtError(CA_ERR_ARG, "ca_fitter: null handle"); \
    rt_set_device(f->device);             \
    __VA_ARGS__;                          \
    return CA_OK;                         \
  } catch (const FtError &e) {            \
    co_set_last_error(e.what());          \
    return e.code;                        \
  } catch (const std::exception &e) {     \
    co_set_last_error(e.what());          \
    return CA_ERR_DEVICE;                 \
  }

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
  ca_fitter *f = nullptr;
  try {
    f = new ca_fitter();
    f->init(device, net, max_batch);
  } catch (const std::exception &e) {
    co_set_last_error(e.what());
    delete f;
    return CA_ERR_DEVICE;
  }
  *out = f;
  return CA_OK;
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

static void ft_check_n(const ca_fitter *f, size_t n_floats) {
  if (n_floats != (size_t)f->nw)
    throw FtError(CA_ERR_ARG, std::string("ca_fitter: ") + (f->net == CA_NET_RESCNN4 ? "rescnn4" : "mlp12x100") + " has " +
                                  std::to_string(f->nw) + " floats");
}

extern "C" int ca_fitter_set_weights(ca_fitter *f, const float *weights, size_t n_floats) {
  FT_GUARD(ft_check_n(f, n_floats); if (!weights) throw FtError(CA_ERR_ARG, "null weights");
           rt_h2d(f->w.p, weights, f->nw * sizeof(float), f->s); rt_sync(f->s))
}

extern "C" int ca_fitter_get_weights(ca_fitter *f, float *weights, size_t n_floats) {
  FT_GUARD(ft_check_n(f, n_floats); if (!weights) throw FtError(CA_ERR_ARG, "null weights");
           rt_d2h(weights, f->w.p, f->nw * sizeof(float), f->s); rt_sync(f->s))
}

extern "C" int ca_fitter_set_optimizer(ca_fitter *f, const float *m, const float *v, size_t n_floats, int64_t iterations) {
  FT_GUARD(ft_check_n(f, n_floats); if (!m || !v || iterations < 0) throw FtError(CA_ERR_ARG, "null slots or negative iterations");
           rt_h2d(f->m.p, m, f->nw * sizeof(float), f->s); rt_h2d(f->v.p, v, f->nw * sizeof(float), f->s); rt_sync(f->s);
           f->iterations = iterations)
}

extern "C" int ca_fitter_get_optimizer(ca_fitter *f, float *m, float *v, size_t n_floats, int64_t *iterations) {
  FT_GUARD(ft_check_n(f, n_floats); if (!m || !v || !iterations) throw FtError(CA_ERR_ARG, "null output");
           rt_d2h(m, f->m.p, f->nw * sizeof(float), f->s); rt_d2h(v, f->v.p, f->nw * sizeof(float), f->s); rt_sync(f->s);
           *iterations = f->iterations)
}

extern "C" int ca_fitter_set_data(ca_fitter *f, const float *states, const float *evals, const float *probs, int32_t n) {
  FT_GUARD(if (n < 1 || !states || !evals || !probs) throw FtError(CA_ERR_ARG, "ca_fitter_set_data: empty or null");
           f->n = 0; f->states.alloc((size_t)n * CA_GAME_STATE_SIZE, f->s); f->evals.alloc((size_t)n, f->s);
           f->probs.alloc((size_t)n * CA_NUM_MOVES, f->s); f->idx.alloc((size_t)n, f->s); f->idx_cap = n;
           rt_h2d(f->states.p, states, (size_t)n * CA_GAME_STATE_SIZE * sizeof(float), f->s);
           rt_h2d(f->evals.p, evals, (size_t)n * sizeof(float), f->s);
           rt_h2d(f->probs.p, probs, (size_t)n * CA_NUM_MOVES * sizeof(float), f->s); rt_sync(f->s); f->n = n)
}

extern "C" int ca_fitter_train(ca_fitter *f, const int32_t *rows, int32_t n_rows, int32_t batch, float learning_rate,
                               double *out_losses, float *batch_losses) {
  FT_GUARD(
      f->need_data(); f->check_batch(batch); if (!rows || n_rows < 1) throw FtError(CA_ERR_ARG, "ca_fitter_train: no rows");
      f->check_rows(rows, n_rows); const int nb = (n_rows + batch - 1) / batch; f->ensure_loss(nb);
      rt_h2d(f->idx.p, rows, (size_t)n_rows * sizeof(int32_t), f->s);
      for (int b = 0; b < nb; ++b) {
        const int B = b * batch + batch <= n_rows ? batch : n_rows - b * batch;
        const int32_t *r = f->idx.p + (size_t)b * batch;
        f->forward(r, B, true);
        f->loss_terms(r, B, true, b);
        f->backward(B);
        /* Keras Adam: local_step = iterations + 1, lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t), in float32 */
        const float t = (float)(f->iterations + 1);
        const float lr_t = learning_rate * (sqrtf(1.0f - powf(0.999f, t)) / (1.0f - powf(0.9f, t)));
        f->update(lr_t, true);
        f->iterations += 1;
      } f->losses(nb, n_rows, batch, out_losses, batch_losses))
}

extern "C" int ca_fitter_evaluate(ca_fitter *f, int32_t row0, int32_t n_rows, int32_t batch, double *out_losses) {
  FT_GUARD(f->need_data(); f->check_batch(batch);
           if (n_rows < 1 || row0 < 0 || (int64_t)row0 + n_rows > f->n) throw FtError(CA_ERR_ARG, "ca_fitter_evaluate: rows out of range");
           std::vector<int32_t> rows(n_rows); for (int32_t i = 0; i < n_rows; ++i) rows[i] = row0 + i;
           const int nb = (n_rows + batch - 1) / batch; f->ensure_loss(nb);
           rt_h2d(f->idx.p, rows.data(), (size_t)n_rows * sizeof(int32_t), f->s);
           for (int b = 0; b < nb; ++b) {
             const int B = b * batch + batch <= n_rows ? batch : n_rows - b * batch;
             const int32_t *r = f->idx.p + (size_t)b * batch;
             f->forward(r, B, false);
             f->loss_terms(r, B, false, b);
           } f->losses(nb, n_rows, batch, out_losses, nullptr))
}

extern "C" int ca_fitter_gradients(ca_fitter *f, const int32_t *rows, int32_t n_rows, float *grads, double *out_losses) {
  FT_GUARD(f->need_data(); f->check_batch(n_rows); if (!rows || !grads) throw FtError(CA_ERR_ARG, "null argument");
           f->check_rows(rows, n_rows); f->ensure_loss(1);
           rt_h2d(f->idx.p, rows, (size_t)n_rows * sizeof(int32_t), f->s); f->forward(f->idx.p, n_rows, true);
           f->loss_terms(f->idx.p, n_rows, true, 0); f->backward(n_rows); f->update(0.0f, false);
           rt_d2h(grads, f->gsum.p, f->nw * sizeof(float), f->s); f->losses(1, n_rows, n_rows, out_losses, nullptr))
}
