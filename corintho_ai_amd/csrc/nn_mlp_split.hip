// nn_mlp_split.hip -- K5x3 / K5x6: the reference's policy/value network (12 x [Dense(100) -> ReLU ->
// BatchNorm] -> {Dense(1) tanh, Dense(96) softmax}, wrapper.py:256-271) as ONE fused gfx950
// kernel at split precision on v_mfma_f32_32x32x16_bf16.
//
// Same network, same flat weights and the same function as K5 (nn_mlp.hip, fp32 MFMA); what
// changes is the arithmetic of the thirteen matrix products.  Both operands are written as a sum
// of NT bf16 terms (the value rounded to bf16, then the successive remainders, each exact in
// float32) and the product is expanded into the terms w_i x_j with i + j <= NT - 1, accumulated in
// fp32 by the MFMA:
//   NT = 2 (CO_NET_MLP12X100_X3, "bf16x3"): 16 significand bits, 3 MFMAs, <= 1e-4 from float32;
//   NT = 3 (CO_NET_MLP12X100_X6, "bf16x6"): the three terms ARE the float32 value, 6 MFMAs, the
//          dropped terms are <= 2^-24 of a product: float32-equivalent (tests/test_net_precision.py
//          holds its error against a float64 restatement to that of K5's fp32 MFMA chain).
// The dense layers of this network are too small for fp32 MFMA to pay: K5 spends as long on them
// as the whole tree search takes.
//
// Mapping (the one of the residual CNN's split kernels, nn_rescnn_split.h).  Transposed evaluation:
// out^T[feature][row] = W^T[feature][k] act^T[k][row]; a wave owns 32 batch rows = one MFMA
// column tile and all 128 (padded) output features = four 32-row tiles, 64 accumulator
// registers.  The accumulator layout (lane = (h, row), register 4g + i of tile T = feature
// 32T + 8g + 4h + i) is the B-operand layout of the next layer when its K steps are taken in the
// order  step s = 2T + a, k-slot (h, j) <-> feature 32T + 8(2a + j/4) + 4h + j%4,  so activations
// stay in registers through all 13 layers; the weights are pre-permuted (and pre-split into
// bf16 terms) on the host into that fragment order and stream through LDS by LDS-DMA.
// BatchNorm of layer l is folded into the weights and bias of layer l + 1 on the host (in
// float64, as the TFLite converter does for the reference's own checkpoints), the bias is the
// initial value of the accumulators, so a layer's epilogue is ReLU + the split.  tanh and the
// 96-way softmax are fused into the last layer.  Fixed k order, no batch-dependent tiling: a
// row's result does not depend on its batch.
//
// Weight stream: a layer is two CHUNKS of four K steps (K = 112 = 7 steps, the eighth is padding
// that is staged but never multiplied; the input layer has K = 80 = 5 steps), every chunk the same
// size (4 steps + a 4 KiB bias piece = 13 LDS-DMA instructions per wave), through a ring of three
// LDS slots: while chunk c computes, chunk c + 1 has landed or is landing and chunk c + 2 is
// requested -- the wait at the top of a chunk is `vmcnt(13)` (everything but the youngest chunk),
// not a drain.  (Round 1 staged whole layers through two slots and drained at every layer; the
// kernel waited for the stream about half of its time.)
//
// Geometry: 256 threads = 4 waves x 32 rows = 128 rows per workgroup, one workgroup per CU.
// The input layer's operands are exact in bf16 (0/1 and k/4): only their first term exists.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <vector>

#include "engine_defs.h"
#include "host.h"
#include "lds_dma.h"
#include "nn_split.h"

/* (the chunks' geometry, M3_NLAYERS .. M3_TOTAL_WORDS: nn_split.h) */
#define M3_CHUNK_PIECES_PER_WAVE(NT) (M3_CHUNK_WORDS(NT) / 256 / 4)  /* 9 / 13 */
#define M3_LDS_BYTES(NT) (3 * M3_CHUNK_WORDS(NT) * 4)
#define M3_ROWS_PER_WG 128

/* one wave copies 1 KiB per instruction: lane i supplies bytes [16 i, 16 i + 16) */
template <int NT>
__device__ __forceinline__ void m3_stage(const uint32_t *w, uint32_t lds_slot_addr, int c, int wave, int lane) {
  const uint32_t *src = w + (size_t)c * M3_CHUNK_WORDS(NT) + lane * 4;
#pragma unroll
  for (int i = 0; i < M3_CHUNK_PIECES_PER_WAVE(NT); ++i) {
    const int p = wave + 4 * i;
    co_lds_dma_1k(src + p * 256, lds_slot_addr + (uint32_t)p * 1024u);
  }
}

/* K steps S0 .. S0 + NS - 1 of a layer from one chunk: acc += W x.  XT = number of terms the B
 * operand has (1 for the input layer).  Products w_i x_j, i + j <= NT - 1, j < XT, largest
 * first.  Weight fragments of step s + 1 are requested from LDS before the MFMAs of step s issue. */
template <int NT, int S0, int NS, int XT, bool F16 = false>
__device__ __forceinline__ void m3_steps(f32x16 (&acc)[4], const uint32_t (&b)[NT][8][4], const uint32_t *wl, int lane) {
  u32x4 a[2][NT][4];
#pragma unroll
  for (int to = 0; to < 4; ++to)
#pragma unroll
    for (int t = 0; t < NT; ++t) a[0][t][to] = *reinterpret_cast<const u32x4 *>(wl + (((0 * 4 + to) * NT + t) * 64 + lane) * 4);
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int cur = s & 1, nxt = cur ^ 1;
    if (s + 1 < NS) {
#pragma unroll
      for (int to = 0; to < 4; ++to)
#pragma unroll
        for (int t = 0; t < NT; ++t)
          a[nxt][t][to] = *reinterpret_cast<const u32x4 *>(wl + ((((s + 1) * 4 + to) * NT + t) * 64 + lane) * 4);
    }
    u32x4 B[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int m = 0; m < 4; ++m) B[t][m] = b[t][S0 + s][m];
    }
#pragma unroll
    for (int sum = 0; sum < NT; ++sum)
#pragma unroll
      for (int i = 0; i <= sum; ++i)
        if (sum - i < XT) {
#pragma unroll
          for (int to = 0; to < 4; ++to) {
            co_mfma_32x32x16<F16>(acc[to], a[cur][i][to], B[sum - i]);
          }
        }
  }
}

/* accumulators := bias (feature 32T + 8g + 4h + i in register 4g + i of tile T) */
__device__ __forceinline__ void m3_init_bias(f32x16 (&acc)[4], const float *bias, int h) {
#pragma unroll
  for (int T = 0; T < 4; ++T)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 b4 = *reinterpret_cast<const float4 *>(bias + 32 * T + 8 * g + 4 * h);
      acc[T][4 * g + 0] = b4.x;
      acc[T][4 * g + 1] = b4.y;
      acc[T][4 * g + 2] = b4.z;
      acc[T][4 * g + 3] = b4.w;
    }
}

/* top of chunk c: everything this wave requested except the youngest chunk has landed; after the
 * barrier that holds for every wave, and everyone has left the slot of chunk c - 1, which
 * receives chunk c + 2 */
#define M3_CHUNK_HEAD(NT, c)                                                                         \
  {                                                                                                  \
    if ((c) + 1 < M3_NCHUNKS) {                                                                      \
      if (NT == 2) CO_WAIT_VMCNT(9);                                                                 \
      else CO_WAIT_VMCNT(13);                                                                        \
    } else {                                                                                         \
      CO_WAIT_VMCNT(0);                                                                              \
    }                                                                                                \
    co_wg_barrier();                                                                                 \
    if ((c) + 2 < M3_NCHUNKS)                                                                        \
      m3_stage<NT>(wfrag, lds_base + (uint32_t)(((c) + 2) % 3) * (M3_CHUNK_WORDS(NT) * 4u), (c) + 2, wave, lane); \
  }

/* rows row0 .. min(row0 + 128, rows) - 1 of the launch, by one workgroup, with the weights at wfrag */
template <int NT, bool F16>
__device__ __forceinline__ void m3_forward(const float *__restrict__ in, const int rows, const int row0, const uint32_t *__restrict__ wfrag,
                                           float *__restrict__ eval, float *__restrict__ probs, const CoNetIO &io, uint32_t *range_flag) {
  static_assert(M3_CHUNK_PIECES_PER_WAVE(2) == 9 && M3_CHUNK_PIECES_PER_WAVE(3) == 13, "vmcnt immediates of M3_CHUNK_HEAD");
  extern __shared__ __attribute__((aligned(16))) uint32_t m3_lds[]; /* ring of three chunk slots */
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, h = lane >> 5, n = lane & 31;
  const uint32_t lds_base = co_lds_addr(m3_lds);

  /* inputs as the B operand of layer 0: step s = 2T + a, slot j <-> input 32T + 16a + 8(j/4) + 4h + j%4;
   * every input is 0, 1 or k/4: exact in bf16, so only the first term exists */
  const int row = row0 + wave * 32 + n;
  uint32_t b[NT][8][4];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
      for (int m = 0; m < 4; ++m) b[t][s][m] = 0u;
  if (row < rows) {
    const float *x = in + (size_t)(io.in_idx ? io.in_idx[row] : row) * CO_STATE_STRIDE;
#pragma unroll
    for (int s = 0; s < M3_STEPS_L0; ++s) {
      const float4 v0 = *reinterpret_cast<const float4 *>(x + 16 * s + 4 * h);
      const float4 v1 = *reinterpret_cast<const float4 *>(x + 16 * s + 8 + 4 * h);
      uint32_t t[NT];
      co_split_pair<NT, F16>(v0.x, v0.y, t);
      b[0][s][0] = t[0];
      co_split_pair<NT, F16>(v0.z, v0.w, t);
      b[0][s][1] = t[0];
      co_split_pair<NT, F16>(v1.x, v1.y, t);
      b[0][s][2] = t[0];
      co_split_pair<NT, F16>(v1.z, v1.w, t);
      b[0][s][3] = t[0];
    }
  }
  /* the first two chunks are requested behind the input loads: vmcnt retires in issue order, so
   * loads issued behind a transfer would wait for it */
  m3_stage<NT>(wfrag, lds_base, 0, wave, lane);
  m3_stage<NT>(wfrag, lds_base + M3_CHUNK_WORDS(NT) * 4u, 1, wave, lane);
  f32x16 acc[4];
  uint32_t amax = 0u; /* F16: the running maximum of the packed first terms (nn_split.h co_pk_max_f16) */
  for (int l = 0; l < M3_NLAYERS; ++l) {
    const int c0 = 2 * l;
    {
      M3_CHUNK_HEAD(NT, c0)
      const uint32_t *wl = m3_lds + (c0 % 3) * M3_CHUNK_WORDS(NT);
      m3_init_bias(acc, reinterpret_cast<const float *>(wl + 4 * M3_STEP_WORDS(NT)), h);
      if (l == 0) m3_steps<NT, 0, 4, 1, F16>(acc, b, wl, lane);
      else m3_steps<NT, 0, 4, NT, F16>(acc, b, wl, lane);
    }
    {
      M3_CHUNK_HEAD(NT, c0 + 1)
      const uint32_t *wl = m3_lds + ((c0 + 1) % 3) * M3_CHUNK_WORDS(NT);
      if (l == 0) m3_steps<NT, 4, M3_STEPS_L0 - 4, 1, F16>(acc, b, wl, lane);
      else m3_steps<NT, 4, M3_STEPS - 4, NT, F16>(acc, b, wl, lane);
    }
    if (l + 1 < M3_NLAYERS) {
      /* ReLU, then the term operands of the next layer: step 2T + a, word m = registers
       * (8a + 2m, 8a + 2m + 1) of tile T (BatchNorm lives in the next layer's weights) */
#pragma unroll
      for (int T = 0; T < 4; ++T)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            float v0 = acc[T][8 * a + 2 * m], v1 = acc[T][8 * a + 2 * m + 1];
            v0 = v0 > 0.0f ? v0 : 0.0f;
            v1 = v1 > 0.0f ? v1 : 0.0f;
            uint32_t t[NT];
            co_split_pair<NT, F16>(v0, v1, t);
            if constexpr (F16) amax = co_pk_max_f16(amax, t[0]);
#pragma unroll
            for (int i = 0; i < NT; ++i) b[i][2 * T + a][m] = t[i];
          }
    }
  }
  if constexpr (F16) co_raise_unless_f16_finite(amax, range_flag);
  /* heads: features 0..95 = policy logits (tiles 0..2), feature 96 = value (tile 3, g 0, h 0, i 0) */
  float mx = -INFINITY;
#pragma unroll
  for (int T = 0; T < 3; ++T)
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = acc[T][r] > mx ? acc[T][r] : mx;
  float o = __shfl_xor(mx, 32, 64);
  mx = o > mx ? o : mx;
  float sum = 0.0f;
#pragma unroll
  for (int T = 0; T < 3; ++T)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc[T][r] = __builtin_amdgcn_exp2f((acc[T][r] - mx) * 1.44269504088896340736f);
      sum += acc[T][r];
    }
  sum += __shfl_xor(sum, 32, 64);
  const float inv = 1.0f / sum;
  if (row < rows) {
    const size_t orow = (size_t)(io.out_idx ? io.out_idx[row] : row);
#pragma unroll
    for (int T = 0; T < 3; ++T)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float4 p = make_float4(acc[T][4 * g] * inv, acc[T][4 * g + 1] * inv, acc[T][4 * g + 2] * inv, acc[T][4 * g + 3] * inv);
        *reinterpret_cast<float4 *>(probs + orow * (size_t)io.probs_stride + 32 * T + 8 * g + 4 * h) = p;
      }
    if (h == 0) eval[orow * (size_t)io.eval_stride] = tanhf(acc[3][0]);
  }
}

template <int NT, bool F16 = false>
__global__ __launch_bounds__(256, 1) void co_k_mlp_forward_split_t(const float *__restrict__ in, const int32_t *__restrict__ d_rows,
                                                                   const uint32_t *__restrict__ wfrag, float *__restrict__ eval,
                                                                   float *__restrict__ probs, CoNetIO io, uint32_t *range_flag) {
  const int rows = *d_rows;
  const int row0 = blockIdx.x * M3_ROWS_PER_WG;
  if (row0 >= rows) return;
  m3_forward<NT, F16>(in, rows, row0, wfrag, eval, probs, io, range_flag);
}

/* The grouped instance (nn.h CoNetGroup): workgroup b takes entry b of the workgroup table -- a model and up to 128
 * positions of the index list, all that model's -- reads the weights at wbase + model * M3_TOTAL_WORDS and its rows, and
 * writes its results, through the index list.  One table read per workgroup; everything behind it is m3_forward. */
template <int NT, bool F16 = false>
__global__ __launch_bounds__(256, 1) void co_k_mlp_forward_split_grouped_t(const float *__restrict__ in, const CoGroupWG *__restrict__ wg,
                                                                           const int32_t *__restrict__ n_wg, const int32_t *__restrict__ idx,
                                                                           const uint32_t *__restrict__ wbase, float *__restrict__ eval,
                                                                           float *__restrict__ probs, uint32_t *range_flag) {
  if ((int)blockIdx.x >= *n_wg) return;
  const CoGroupWG e = wg[blockIdx.x];
  const int first = __builtin_amdgcn_readfirstlane(e.first), count = __builtin_amdgcn_readfirstlane(e.count);
  const int model = __builtin_amdgcn_readfirstlane(e.model);
  CoNetIO io;
  io.in_idx = io.out_idx = idx;
  m3_forward<NT, F16>(in, first + count, first, wbase + (size_t)model * M3_TOTAL_WORDS(NT), eval, probs, io, range_flag);
}
#define co_k_mlp_forward_x3 co_k_mlp_forward_split_t<2>
#define co_k_mlp_forward_x6 co_k_mlp_forward_split_t<3>
/* "f16x3": two fp16 terms per operand (22 significand bits), three MFMA products -- see nn_rescnn_split.h */
#define co_k_mlp_forward_h3 co_k_mlp_forward_split_t<2, true>

/* ------------------------------------------------------------------ host */
struct MlpSplitNet : CoNet {
  DevBuf<uint32_t> d_w;
  RangeFlag range; /* f16: the kernels' out-of-range flag */
  size_t cap;
  int nt;
  bool f16;
  MlpSplitNet(const float *w, size_t max_rows, rt_stream_t s, int nterms, bool fp16 = false) : cap(max_rows), nt(nterms), f16(fp16) {
    const std::vector<uint32_t> buf = co_pack_mlp_split(w, nt, f16);
    d_w.upload(buf.data(), buf.size(), s);
    if (f16) range.alloc(s);
    rt_sync(s);
    rt_max_dynamic_lds(kernel(), M3_LDS_BYTES(nt));
  }
  /* (the three instances have one signature) */
  decltype(&co_k_mlp_forward_x3) kernel() const { return f16 ? co_k_mlp_forward_h3 : nt == 2 ? co_k_mlp_forward_x3 : co_k_mlp_forward_x6; }
  bool range_exceeded(rt_stream_t s) override { return range.read(s); }
  size_t max_rows() const override { return cap; }
  int kind() const override { return co_net_kind_of(CO_FAMILY_MLP12X100, nt, f16); }
  double flop_per_row() const override { return MlpLayout().flop_per_row(); }
  void forward(const float *d_in, int32_t rows_cap, const int32_t *d_rows, float *d_eval, float *d_probs,
               rt_stream_t s, const CoNetIO &io = CoNetIO()) override {
    int grid = (rows_cap + M3_ROWS_PER_WG - 1) / M3_ROWS_PER_WG;
    if (grid < 1) return;
    RT_LAUNCH_LDS(kernel(), grid, 256, M3_LDS_BYTES(nt), s, d_in, d_rows, (const uint32_t *)d_w.p, d_eval, d_probs, io, range.ptr());
  }
};

/* M weight sets in one buffer at a stride of M3_TOTAL_WORDS, the range flag shared by the launch */
struct MlpSplitNetGroup : CoNetGroup {
  DevBuf<uint32_t> d_w;
  RangeFlag range;
  size_t cap;
  int nt, m;
  bool f16;
  MlpSplitNetGroup(const float *const *w, int models, size_t max_rows, rt_stream_t s, int nterms, bool fp16)
      : cap(max_rows), nt(nterms), m(models), f16(fp16) {
    std::vector<uint32_t> buf;
    buf.reserve((size_t)models * M3_TOTAL_WORDS(nt));
    for (int i = 0; i < models; ++i) {
      try {
        const std::vector<uint32_t> one = co_pack_mlp_split(w[i], nt, f16);
        buf.insert(buf.end(), one.begin(), one.end());
      } catch (const std::invalid_argument &e) {
        throw std::invalid_argument("model " + std::to_string(i) + " of the group: " + e.what());
      }
    }
    d_w.upload(buf.data(), buf.size(), s);
    if (f16) range.alloc(s);
    rt_sync(s);
    rt_max_dynamic_lds(kernel(), M3_LDS_BYTES(nt));
  }
  decltype(&co_k_mlp_forward_split_grouped_t<2>) kernel() const {
    return f16 ? co_k_mlp_forward_split_grouped_t<2, true> : nt == 2 ? co_k_mlp_forward_split_grouped_t<2> : co_k_mlp_forward_split_grouped_t<3>;
  }
  int kind() const override { return co_net_kind_of(CO_FAMILY_MLP12X100, nt, f16); }
  int models() const override { return m; }
  size_t max_rows() const override { return cap; }
  bool grouped_kernel() const override { return true; }
  bool range_exceeded(rt_stream_t s) override { return range.read(s); }
  void forward(const float *d_in, int32_t rows_cap, const CoGroupPlan &plan, float *d_eval, float *d_probs, rt_stream_t s) override {
    static_assert(CO_GROUP_TILE == M3_ROWS_PER_WG, "the workgroup table is cut for this kernel's rows per workgroup");
    /* the worst case of rows_cap rows: every model ends in a partial workgroup (never more than the table holds) */
    int grid = rows_cap / M3_ROWS_PER_WG + m;
    if (grid > plan.wg_cap) grid = plan.wg_cap;
    if (grid < 1 || plan.seg_stride) return;
    RT_LAUNCH_LDS(kernel(), grid, 256, M3_LDS_BYTES(nt), s, d_in, plan.wg, plan.n_wg, plan.idx, (const uint32_t *)d_w.p, d_eval, d_probs,
                  range.ptr());
  }
};

CoNetGroup *co_mlp_split_group_create(const float *const *weights, int models, size_t n_floats, size_t max_rows, rt_stream_t s, int nterms,
                                      bool f16) {
  if (n_floats != (size_t)CO_MLP_NUM_WEIGHTS || (nterms != 2 && nterms != 3) || (f16 && nterms != 2)) return nullptr;
  return new MlpSplitNetGroup(weights, models, max_rows, s, nterms, f16);
}

CoNet *co_mlp_split_create(const float *weights, size_t n_floats, size_t max_rows, rt_stream_t s, int nterms, bool f16) {
  if (n_floats != (size_t)CO_MLP_NUM_WEIGHTS || (nterms != 2 && nterms != 3) || (f16 && nterms != 2)) return nullptr;
  return new MlpSplitNet(weights, max_rows, s, nterms, f16);
}
