// nn_rescnn.hip -- K6: the north-star policy/value network, a 4-block residual
// CNN over the 4x4 board (specification: corintho_ai_amd/nets.py "rescnn4"), as
// ONE fused gfx950 kernel on fp32 MFMA.
//
// Mapping.  A 4x4 board has exactly 16 pixels -- one N-tile of
// v_mfma_f32_16x16x4_f32.  A 3x3 convolution is evaluated transposed, as for the
// MLP (nn_mlp.hip): out^T[co][pixel] += W[tap][ci][co] * in[ci][pixel + tap], so
//   A operand = a 16(co) x 4(ci) weight fragment,
//   B operand = the activation tile of ONE position shifted by the tap.
// The activation tile of a position lives in registers in accumulator layout
// (pixel on the lane, lane & 15; channel 16t + 4q + r in register r of tile t,
// q = lane >> 4), which IS the B layout when the K steps run in the order
// (tap, t, r) with k-slot q.  The spatial shift of a tap is a DPP row shift inside
// each 16-lane row (source pixel p + 4dy + dx, zero outside the row) plus a lane
// mask for the x wrap-around: "im2col" costs two VALU ops per B operand and no
// memory traffic at all.  Activations, the residual skip and the accumulators
// never leave registers through stem + 8 convolutions; bias + BatchNorm + ReLU +
// residual add run on the accumulators; the heads (1x1 convs, dense layers, tanh,
// 96-way softmax) are fused behind them.  Only weights move: one tap of one
// convolution (16 KB) at a time through a double-buffered LDS window filled by
// LDS-DMA (global_load_lds) while the previous tap computes.
//
// fp32 end to end, fixed k order, one position per MFMA column: a row's result
// does not depend on its batch (SURVEY 8e invariant).
// Work: 9.65 MFLOP per position, no padding waste in the 64->64 convolutions.
// Geometry: 256 threads = 4 waves, 4 positions per wave (every weight fragment
// feeds 16 MFMAs), 16 positions per workgroup.
//
// This file: the fp32 kernel, the dense heads all rescnn4 kernels share (rc_dense_*), the host
// classes and the factories.  The split-precision kernels are nn_rescnn_split.h and
// nn_rescnn_pix.h, included below: one translation unit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "engine_defs.h"
#include <memory>

#include "host.h"
#include "lds_dma.h"
#include "nn_split.h"

#define RC_NB 4
#define RC_POS_PER_WG 16
#define RC_STEM_CHUNK 1024   /* floats: 4 steps x 4 out tiles x 64 lanes */
#define RC_CONV_CHUNK 4096   /* floats: 16 steps x 4 out tiles x 64 lanes */
#define RC_NUM_CONVS 9       /* stem + 8 */
#define RC_NUM_CHUNKS 81
#define RC_TRUNK_FLOATS (9 * RC_STEM_CHUNK + 72 * RC_CONV_CHUNK)

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct RcParams {
  const float *in;        /* [rows][80] */
  const int32_t *d_rows;
  const float *wtrunk;    /* RC_TRUNK_FLOATS, fragment order */
  const float *epi;       /* [9][3][64]: bias, bn scale, bn shift */
  const float *whead;     /* [16][64]   1x1 convs: rows 0..3 policy, 4..5 value */
  const float *head_epi;  /* [3][16] */
  const float *wpol;      /* [16][6][64] */
  const float *bpol;      /* [96] */
  const float *wv1;       /* [8][4][64] */
  const float *bv1;       /* [64] */
  const float *wv2;       /* [16][64] */
  const float *bv2;       /* [1] */
  float *eval;
  float *probs;
  CoNetIO io;             /* row indirection (evaluation cache), see nn.h */
};

/* input row / output element of launch row `pos` */
__device__ __forceinline__ size_t rc_in_row(const RcParams &P, int pos) { return (size_t)(P.io.in_idx ? P.io.in_idx[pos] : pos); }
__device__ __forceinline__ size_t rc_out_row(const RcParams &P, int pos) { return (size_t)(P.io.out_idx ? P.io.out_idx[pos] : pos); }

__device__ __forceinline__ const float *rc_chunk_ptr(const float *wtrunk, int ch) {
  return ch < 9 ? wtrunk + ch * RC_STEM_CHUNK : wtrunk + 9 * RC_STEM_CHUNK + (ch - 9) * RC_CONV_CHUNK;
}

/* LDS-DMA: each wave-instruction moves 1 KiB (lane i: bytes [16 i, 16 i + 16)) */
__device__ __forceinline__ void rc_stage(const float *wtrunk, float *lds_buf, int ch, int wave, int lane) {
  const float *src = rc_chunk_ptr(wtrunk, ch);
  const int pieces = ch < 9 ? RC_STEM_CHUNK / 256 : RC_CONV_CHUNK / 256;
  for (int p = wave; p < pieces; p += 4) {
    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1))) *)(src + p * 256 + lane * 4),
                                     (void __attribute__((address_space(3))) *)(lds_buf + p * 256), 16, 0, 0);
  }
}

/* the tap's view of an activation register: pixel p reads pixel p + S (S = 4 dy + dx),
 * zero outside the board */
template <int S>
__device__ __forceinline__ float rc_row_shift(float v) {
  if (S == 0) return v;
  constexpr int ctrl = S > 0 ? (0x100 + S) : (0x110 - S); /* row_shl:S reads lane+S, row_shr:S reads lane-S */
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), ctrl, 0xF, 0xF, true));
}

template <int TAP>
__device__ __forceinline__ float rc_tap(float v, bool okL, bool okR) {
  constexpr int dy = TAP / 3 - 1, dx = TAP % 3 - 1;
  float s = rc_row_shift<4 * dy + dx>(v);
  if (dx == -1) s = okL ? s : 0.0f;
  if (dx == 1) s = okR ? s : 0.0f;
  return s;
}

template <int CT, int TAP>
__device__ __forceinline__ void rc_conv_tap(f32x4 (&acc)[RC_NB][4], const float (&in)[RC_NB][4][4], const float *w, int lane,
                                            bool okL, bool okR) {
#pragma unroll
  for (int t = 0; t < CT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float *wp = w + ((t * 4 + r) * 4) * 64 + lane;
      float a[4];
#pragma unroll
      for (int to = 0; to < 4; ++to) a[to] = wp[to * 64];
#pragma unroll
      for (int nb = 0; nb < RC_NB; ++nb) {
        const float b = rc_tap<TAP>(in[nb][t][r], okL, okR);
#pragma unroll
        for (int to = 0; to < 4; ++to) acc[nb][to] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[to], b, acc[nb][to], 0, 0, 0);
      }
    }
  }
}

/* one 3x3 convolution = 9 weight chunks; chunk `ch` is consumed from LDS buffer ch & 1
 * while chunk ch + 1 streams into the other */
template <int CT>
__device__ __forceinline__ void rc_conv3x3(f32x4 (&acc)[RC_NB][4], const float (&in)[RC_NB][4][4], int &ch,
                                           const float *wtrunk, float *lds_w, int wave, int lane, bool okL, bool okR) {
#pragma unroll
  for (int nb = 0; nb < RC_NB; ++nb)
#pragma unroll
    for (int to = 0; to < 4; ++to) acc[nb][to] = (f32x4){0.f, 0.f, 0.f, 0.f};
#define RC_TAP(T)                                                                         \
  {                                                                                       \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                      \
    __syncthreads();                                                                      \
    if (ch + 1 < RC_NUM_CHUNKS) rc_stage(wtrunk, lds_w + ((ch + 1) & 1) * RC_CONV_CHUNK, ch + 1, wave, lane); \
    rc_conv_tap<CT, T>(acc, in, lds_w + (ch & 1) * RC_CONV_CHUNK, lane, okL, okR);        \
    ++ch;                                                                                 \
  }
  RC_TAP(0) RC_TAP(1) RC_TAP(2) RC_TAP(3) RC_TAP(4) RC_TAP(5) RC_TAP(6) RC_TAP(7) RC_TAP(8)
#undef RC_TAP
}

/* conv bias -> BatchNorm affine (-> + skip) -> ReLU, channel 16 to + 4 q + r */
template <bool ADD_SKIP, bool RELU>
__device__ __forceinline__ void rc_epilogue(float (&out)[RC_NB][4][4], const f32x4 (&acc)[RC_NB][4],
                                            const float (&skip)[RC_NB][4][4], const float *epi, int q) {
#pragma unroll
  for (int to = 0; to < 4; ++to) {
    const float4 b4 = *reinterpret_cast<const float4 *>(epi + 16 * to + 4 * q);
    const float4 a4 = *reinterpret_cast<const float4 *>(epi + 64 + 16 * to + 4 * q);
    const float4 c4 = *reinterpret_cast<const float4 *>(epi + 128 + 16 * to + 4 * q);
    const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
    const float aa[4] = {a4.x, a4.y, a4.z, a4.w};
    const float cc[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
    for (int nb = 0; nb < RC_NB; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[nb][to][r] + bb[r];
        v = aa[r] * v + cc[r];
        if (ADD_SKIP) v = skip[nb][to][r] + v;
        if (RELU) v = v > 0.0f ? v : 0.0f;
        out[nb][to][r] = v;
      }
  }
}

/* ---- heads, shared by both precisions: x = the trunk output of this wave's RC_NB
 * positions (fp32, accumulator layout); feat_w = RC_NB x 96 floats of LDS owned by the wave */
__device__ __forceinline__ void rc_dense_policy(const RcParams &P, const float *wpol, const float *feat16, int rows,
                                                int pos_base, int lane, int ncols = 16);
__device__ __forceinline__ void rc_dense_value(const RcParams &P, const float *wv1, const float *wv2, const float *feat16,
                                               int rows, int pos_base, int lane, int ncols = 16);

__device__ __forceinline__ void rc_heads(const RcParams &P, const float (&x)[RC_NB][4][4], float *feat_wg, int wave,
                                         int rows, int row0, int lane, int q, int c) {
  float *feat_w = feat_wg + wave * RC_NB * 96;
  /* ---- heads.  1x1 convolutions: out rows 0..3 policy planes, 4..5 value planes */
  f32x4 h1[RC_NB];
#pragma unroll
  for (int nb = 0; nb < RC_NB; ++nb) h1[nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float a = P.whead[(t * 4 + r) * 64 + lane];
#pragma unroll
      for (int nb = 0; nb < RC_NB; ++nb) h1[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x[nb][t][r], h1[nb], 0, 0, 0);
    }
  {
    const float4 b4 = *reinterpret_cast<const float4 *>(P.head_epi + 4 * q);
    const float4 a4 = *reinterpret_cast<const float4 *>(P.head_epi + 16 + 4 * q);
    const float4 c4 = *reinterpret_cast<const float4 *>(P.head_epi + 32 + 4 * q);
    const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
    const float aa[4] = {a4.x, a4.y, a4.z, a4.w};
    const float cc[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
    for (int nb = 0; nb < RC_NB; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = h1[nb][r] + bb[r];
        v = aa[r] * v + cc[r];
        v = v > 0.0f ? v : 0.0f;
        /* flatten: policy index pixel*4 + ch, value index 64 + pixel*2 + ch */
        if (q == 0) feat_w[nb * 96 + c * 4 + r] = v;
        if (q == 1 && r < 2) feat_w[nb * 96 + 64 + c * 2 + r] = v;
      }
  }
  __syncthreads();
  /* the workgroup's 16 positions = one column tile: wave 0 policy, wave 1 value */
  if (wave == 0) rc_dense_policy(P, P.wpol, feat_wg, rows, row0, lane);
  if (wave == 1) rc_dense_value(P, P.wv1, P.wv2, feat_wg, rows, row0, lane);
}

/* Dense heads on 16 positions at once (one full MFMA column tile): `feat` = 16 x 96 floats of
 * LDS (flattened head features of consecutive positions pos_base .. pos_base + 15), column c =
 * position.  One wave runs the policy head (Dense 64 -> 96, softmax) of a tile, another its
 * value head (Dense 32 -> 64, ReLU, Dense 64 -> 1, tanh), so the dense weights are read once
 * per 16 positions and no MFMA column is idle. */
__device__ __forceinline__ void rc_dense_policy(const RcParams &P, const float *wpol, const float *feat16, int rows,
                                                int pos_base, int lane, int ncols) {
  const int q = lane >> 4, c = lane & 15;
  const float *feat = feat16 + c * 96;
  f32x4 pl[6];
#pragma unroll
  for (int to = 0; to < 6; ++to) pl[to] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const float b = feat[4 * s + q];
#pragma unroll
    for (int to = 0; to < 6; ++to)
      pl[to] = __builtin_amdgcn_mfma_f32_16x16x4f32(wpol[(s * 6 + to) * 64 + lane], b, pl[to], 0, 0, 0);
  }
  /* softmax over the 96 logits of column c: registers (to, r) in the lane, q across lanes */
  float lg[6][4];
  float m = -INFINITY;
#pragma unroll
  for (int to = 0; to < 6; ++to) {
    const float4 b4 = *reinterpret_cast<const float4 *>(P.bpol + 16 * to + 4 * q);
    const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      lg[to][r] = pl[to][r] + bb[r];
      m = lg[to][r] > m ? lg[to][r] : m;
    }
  }
  float o = __shfl_xor(m, 16, 64);
  m = o > m ? o : m;
  o = __shfl_xor(m, 32, 64);
  m = o > m ? o : m;
  float sum = 0.0f;
#pragma unroll
  for (int to = 0; to < 6; ++to)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      /* exp(x) = 2^(x log2 e) on the hardware exponential (1 ulp; x <= 0 here) */
      lg[to][r] = __builtin_amdgcn_exp2f((lg[to][r] - m) * 1.44269504088896340736f);
      sum += lg[to][r];
    }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  const float inv = 1.0f / sum;
  const int pos = pos_base + c;
  if (pos < rows && c < ncols) { /* a workgroup of the thin kernel owns the first ncols = 8 columns of the tile only */
    const size_t orow = rc_out_row(P, pos);
#pragma unroll
    for (int to = 0; to < 6; ++to) {
      float4 p = make_float4(lg[to][0] * inv, lg[to][1] * inv, lg[to][2] * inv, lg[to][3] * inv);
      *reinterpret_cast<float4 *>(P.probs + orow * (size_t)P.io.probs_stride + 16 * to + 4 * q) = p;
    }
  }
}

__device__ __forceinline__ void rc_dense_value(const RcParams &P, const float *wv1, const float *wv2, const float *feat16,
                                               int rows, int pos_base, int lane, int ncols) {
  const int q = lane >> 4, c = lane & 15;
  const float *feat = feat16 + c * 96;
  f32x4 v1[4];
#pragma unroll
  for (int to = 0; to < 4; ++to) v1[to] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const float b = feat[64 + 4 * s + q];
#pragma unroll
    for (int to = 0; to < 4; ++to)
      v1[to] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv1[(s * 4 + to) * 64 + lane], b, v1[to], 0, 0, 0);
  }
  f32x4 v2 = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const float4 b4 = *reinterpret_cast<const float4 *>(P.bv1 + 16 * t + 4 * q);
    const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float hv = v1[t][r] + bb[r];
      hv = hv > 0.0f ? hv : 0.0f;
      v2 = __builtin_amdgcn_mfma_f32_16x16x4f32(wv2[(t * 4 + r) * 64 + lane], hv, v2, 0, 0, 0);
    }
  }
  const int pos = pos_base + c;
  if (q == 0 && pos < rows && c < ncols) P.eval[rc_out_row(P, pos) * (size_t)P.io.eval_stride] = tanhf(v2[0] + P.bv2[0]);
}

#define CO_RC_F32_BLOCKS 2
__global__ __launch_bounds__(256, CO_RC_F32_BLOCKS) void co_k_rescnn_forward(RcParams P) {
  __shared__ __attribute__((aligned(16))) float lds_w[2 * RC_CONV_CHUNK];
  __shared__ float lds_feat[4][RC_NB][96];
  const int rows = *P.d_rows;
  const int row0 = blockIdx.x * RC_POS_PER_WG;
  if (row0 >= rows) return;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, q = lane >> 4, c = lane & 15;
  const bool okL = (c & 3) != 0, okR = (c & 3) != 3;
  rc_stage(P.wtrunk, lds_w, 0, wave, lane);

  /* input planes: lane (q, pixel c) holds channels 4q..4q+3 -- q 0: the cell's four
   * board bits, q 1: reserves 0..3, q 2: reserves 4..5 (+ zero padding), q 3: zeros */
  float x[RC_NB][4][4];
#pragma unroll
  for (int nb = 0; nb < RC_NB; ++nb) {
    const int pos = row0 + wave * RC_NB + nb;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (pos < rows) v = *reinterpret_cast<const float4 *>(P.in + rc_in_row(P, pos) * CO_STATE_STRIDE + (q == 0 ? 4 * c : 60 + 4 * q));
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) x[nb][t][r] = 0.0f;
    x[nb][0][0] = v.x;
    x[nb][0][1] = v.y;
    x[nb][0][2] = v.z;
    x[nb][0][3] = v.w;
  }

  f32x4 acc[RC_NB][4];
  float y[RC_NB][4][4];
  int ch = 0;
  /* stem */
  rc_conv3x3<1>(acc, x, ch, P.wtrunk, lds_w, wave, lane, okL, okR);
  rc_epilogue<false, true>(x, acc, x, P.epi, q);
  /* residual tower */
  for (int b = 0; b < 4; ++b) {
    rc_conv3x3<4>(acc, x, ch, P.wtrunk, lds_w, wave, lane, okL, okR);
    rc_epilogue<false, true>(y, acc, x, P.epi + (size_t)(1 + 2 * b) * 192, q);
    rc_conv3x3<4>(acc, y, ch, P.wtrunk, lds_w, wave, lane, okL, okR);
    rc_epilogue<true, true>(x, acc, x, P.epi + (size_t)(2 + 2 * b) * 192, q);
  }

  rc_heads(P, x, &lds_feat[0][0][0], wave, rows, row0, lane, q, c);
}

#include "nn_rescnn_split.h"
#include "nn_rescnn_pix.h"

/* ------------------------------------------------------------------ host */
struct ResCnnNet : CoNet {
  std::vector<DevBuf<float>> bufs;
  RcParams P;
  size_t cap;

  float *upload(const std::vector<float> &h, rt_stream_t s) {
    bufs.emplace_back();
    bufs.back().upload(h.data(), h.size(), s);
    return bufs.back().p;
  }

  ResCnnNet(const float *w, size_t max_rows, rt_stream_t s) : cap(max_rows) {
    constexpr ResCnnLayout RL;
    std::vector<float> trunk(RC_TRUNK_FLOATS, 0.0f), epi((size_t)RC_NUM_CONVS * 192, 0.0f);
    size_t off = 0;
    for (int cv = 0; cv < RC_NUM_CONVS; ++cv) {
      const int cin = RL.cin(cv), ct = cv == 0 ? 1 : 4;
      const size_t chunk = cv == 0 ? RC_STEM_CHUNK : RC_CONV_CHUNK;
      const float *K = w + RL.kernel(cv); /* [3][3][cin][64] */
      for (int tap = 0; tap < 9; ++tap)
        for (int t = 0; t < ct; ++t)
          for (int r = 0; r < 4; ++r)
            for (int to = 0; to < 4; ++to)
              for (int q = 0; q < 4; ++q)
                for (int i = 0; i < 16; ++i) {
                  int ci = 16 * t + 4 * q + r, co = 16 * to + i;
                  float v = ci < cin ? K[((size_t)tap * cin + ci) * 64 + co] : 0.0f;
                  trunk[off + (size_t)tap * chunk + ((size_t)(t * 4 + r) * 4 + to) * 64 + 16 * q + i] = v;
                }
      off += 9 * chunk;
      for (int i = 0; i < 64; ++i) epi[(size_t)cv * 192 + i] = w[RL.bias(cv) + i];
      bn_fold(w, RL, cv, 64, &epi[(size_t)cv * 192 + 64], &epi[(size_t)cv * 192 + 128]);
    }
    /* the heads: 1x1 convolutions (BatchNorms 9 and 10), then the dense layers */
    const float *pk = w + RL.p_k, *pb = w + RL.bias(9), *pdk = w + RL.p_dk, *pdb = w + RL.p_db;
    const float *vk = w + RL.v_k, *vb = w + RL.bias(10);
    const float *vd1k = w + RL.v_d1k, *vd1b = w + RL.v_d1b, *vd2k = w + RL.v_d2k, *vd2b = w + RL.v_d2b;
    std::vector<float> whead(16 * 64, 0.0f), hepi(48, 0.0f), wpol(16 * 6 * 64, 0.0f), bpol(pdb, pdb + 96);
    std::vector<float> wv1(8 * 4 * 64, 0.0f), bv1(vd1b, vd1b + 64), wv2(16 * 64, 0.0f), bv2(vd2b, vd2b + 1);
    for (int t = 0; t < 4; ++t)
      for (int r = 0; r < 4; ++r)
        for (int q = 0; q < 4; ++q)
          for (int i = 0; i < 16; ++i) {
            int k = 16 * t + 4 * q + r;
            float v = i < 4 ? pk[k * 4 + i] : i < 6 ? vk[k * 2 + (i - 4)] : 0.0f;
            whead[(size_t)(t * 4 + r) * 64 + 16 * q + i] = v;
            wv2[(size_t)(t * 4 + r) * 64 + 16 * q + i] = i == 0 ? vd2k[k] : 0.0f;
          }
    for (int i = 0; i < 4; ++i) hepi[i] = pb[i];
    for (int i = 0; i < 2; ++i) hepi[4 + i] = vb[i];
    bn_fold(w, RL, 9, 4, &hepi[16], &hepi[32]);
    bn_fold(w, RL, 10, 2, &hepi[16 + 4], &hepi[32 + 4]);
    for (int s2 = 0; s2 < 16; ++s2)
      for (int to = 0; to < 6; ++to)
        for (int q = 0; q < 4; ++q)
          for (int i = 0; i < 16; ++i) wpol[((size_t)s2 * 6 + to) * 64 + 16 * q + i] = pdk[(size_t)(4 * s2 + q) * 96 + 16 * to + i];
    for (int s2 = 0; s2 < 8; ++s2)
      for (int to = 0; to < 4; ++to)
        for (int q = 0; q < 4; ++q)
          for (int i = 0; i < 16; ++i) wv1[((size_t)s2 * 4 + to) * 64 + 16 * q + i] = vd1k[(size_t)(4 * s2 + q) * 64 + 16 * to + i];
    memset(&P, 0, sizeof P);
    P.wtrunk = upload(trunk, s);
    P.epi = upload(epi, s);
    P.whead = upload(whead, s);
    P.head_epi = upload(hepi, s);
    P.wpol = upload(wpol, s);
    P.bpol = upload(bpol, s);
    P.wv1 = upload(wv1, s);
    P.bv1 = upload(bv1, s);
    P.wv2 = upload(wv2, s);
    P.bv2 = upload(bv2, s);
    rt_sync(s);
  }
  size_t max_rows() const override { return cap; }
  int kind() const override { return co_net_kind_of(CO_FAMILY_RESCNN4, 0, false); }
  double flop_per_row() const override { return ResCnnLayout().flop_per_row(); }
  void forward(const float *d_in, int32_t rows_cap, const int32_t *d_rows, float *d_eval, float *d_probs,
               rt_stream_t s, const CoNetIO &io = CoNetIO()) override {
    int grid = (rows_cap + RC_POS_PER_WG - 1) / RC_POS_PER_WG;
    if (grid < 1) return;
    RT_LAUNCH(co_k_rescnn_forward, grid, 256, s, launch_params(d_in, d_rows, d_eval, d_probs, io));
  }
  /* P with one launch's rows and outputs */
  RcParams launch_params(const float *d_in, const int32_t *d_rows, float *d_eval, float *d_probs, const CoNetIO &io) const {
    RcParams p = P;
    p.io = io, p.in = d_in, p.d_rows = d_rows, p.eval = d_eval, p.probs = d_probs;
    return p;
  }
};

/* the split-precision kernels: NT = 2 (bf16x3) or 3 (bf16x6, float32-equivalent) */
struct ResCnnSplitNet : ResCnnNet {
  int nt;
  bool f16;          /* fp16 terms; batches beyond RC3_SMALL_ROWS on the pixel-major kernel (K6p) */
  int num_cus = 256; /* (a pass of that kernel = one workgroup per CU) */
  DevBuf<uint32_t> d_trunk3, d_whead3, d_epi3;
  RangeFlag range; /* f16: the kernels' out-of-range flag */
  ResCnnSplitNet(const float *w, size_t max_rows, rt_stream_t s, int nterms, bool fp16 = false)
      : ResCnnNet(w, max_rows, s), nt(nterms), f16(fp16) {
    const std::vector<uint32_t> tr = co_pack_rescnn_trunk(w, nt, f16), wh3 = co_pack_rescnn_head(w, nt, f16);
    const size_t frag1 = wh3.size(), head_words = RCS_HEAD_WORDS(nt);
    d_trunk3.upload(tr.data(), tr.size(), s);
    d_whead3.alloc(head_words, s);
    rt_h2d(d_whead3.p, wh3.data(), wh3.size() * 4, s);
    rt_d2d(d_whead3.p + frag1, P.wpol, 6144 * 4, s); /* the dense weights in the base class's MFMA order */
    rt_d2d(d_whead3.p + frag1 + 6144, P.wv1, 2048 * 4, s);
    rt_d2d(d_whead3.p + frag1 + 6144 + 2048, P.wv2, 1024 * 4, s);
    if (f16) range.alloc(s);
    d_epi3.alloc(RC3_EPI_WORDS, s); /* zero-filled: the padding is staged too */
    rt_d2d(d_epi3.p, P.epi, (size_t)RC_NUM_CONVS * 192 * 4, s);
    if (nt == 2) {
      rt_max_dynamic_lds(co_k_rescnn_forward_x3, RCS_LDS_WORDS(2, 2) * 4);
      rt_max_dynamic_lds(co_k_rescnn_forward_x3_small, RCS_LDS_WORDS(2, 1) * 4);
      rt_max_dynamic_lds(co_k_rescnn_forward_h3p, RCP_LDS_WORDS * 4);
      rt_max_dynamic_lds(co_k_rescnn_forward_h3_small, RCS_LDS_WORDS(2, 1) * 4);
      int dev = 0;
      hipDeviceProp_t prop;
      if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        num_cus = prop.multiProcessorCount;
    } else {
      rt_max_dynamic_lds(co_k_rescnn_forward_x6, RCS_LDS_WORDS(3, 1) * 4);
    }
    rt_sync(s);
  }
  bool range_exceeded(rt_stream_t s) override { return range.read(s); }
  int kind() const override { return co_net_kind_of(CO_FAMILY_RESCNN4, nt, f16); }
  void forward(const float *d_in, int32_t rows_cap, const int32_t *d_rows, float *d_eval, float *d_probs,
               rt_stream_t s, const CoNetIO &io = CoNetIO()) override {
    if (rows_cap < 1) return;
    Rc3Params q;
    q.base = launch_params(d_in, d_rows, d_eval, d_probs, io);
    q.wtrunk = d_trunk3.p;
    q.whead3 = d_whead3.p;
    q.epi3 = d_epi3.p;
    q.range_flag = range.ptr();
    q.pass_rows = f16 && io.alone ? 32 * num_cus : 0;
    if (nt == 2) {
      /* both kernels are queued; the row count on the device decides which one works (the other's
       * workgroups return at once).  Batches that can exceed RC3_SMALL_ROWS need the throughput kernel. */
      const int small_rows = rows_cap < RC3_SMALL_ROWS ? rows_cap : RC3_SMALL_ROWS;
      /* enough workgroups for either path of the f16 kernel: 16 positions each, or 8 on its thin path (<= RC6_THIN_ROWS rows) */
      const int thin_rows = rows_cap < RC6_THIN_ROWS ? rows_cap : RC6_THIN_ROWS;
      const int small_grid = f16 && (thin_rows + 7) / 8 > (small_rows + 15) / 16 ? (thin_rows + 7) / 8 : (small_rows + 15) / 16;
      RT_LAUNCH_LDS(f16 ? co_k_rescnn_forward_h3_small : co_k_rescnn_forward_x3_small, small_grid, 512, RCS_LDS_WORDS(2, 1) * 4, s, q);
      if (rows_cap > RC3_SMALL_ROWS) {
        if (f16)
          RT_LAUNCH_LDS(co_k_rescnn_forward_h3p, (rows_cap + 31) / 32, 512, RCP_LDS_WORDS * 4, s, q);
        else
          RT_LAUNCH_LDS(co_k_rescnn_forward_x3, (rows_cap + 31) / 32, 512, RCS_LDS_WORDS(2, 2) * 4, s, q);
      }
    } else {
      /* enough workgroups for either path: 16 positions each in the throughput path, 8 in the thin one (<= 2048 rows) */
      const int thin_rows = rows_cap < RC6_THIN_ROWS ? rows_cap : RC6_THIN_ROWS;
      const int grid = (rows_cap + 15) / 16 > (thin_rows + 7) / 8 ? (rows_cap + 15) / 16 : (thin_rows + 7) / 8;
      RT_LAUNCH_LDS(co_k_rescnn_forward_x6, grid, 512, RCS_LDS_WORDS(3, 1) * 4, s, q);
    }
  }
};

/* M models of rescnn4 at f16x3 for the grouped small-batch kernel: each model's buffers are made as for the model alone
 * (ResCnnSplitNet) and copied, device to device, into one buffer at a fixed stride */
struct ResCnnH3NetGroup : CoNetGroup {
  DevBuf<uint32_t> d_w;
  RangeFlag range;
  size_t cap;
  int m;
  uint32_t stride = 0, off_epi = 0, off_head = 0, off_small = 0;
  ResCnnH3NetGroup(const float *const *w, int models, size_t max_rows, rt_stream_t s) : cap(max_rows), m(models) {
    for (int i = 0; i < models; ++i) {
      std::unique_ptr<ResCnnSplitNet> one;
      try {
        one.reset(new ResCnnSplitNet(w[i], max_rows, s, 2, true));
      } catch (const std::invalid_argument &e) {
        throw std::invalid_argument("model " + std::to_string(i) + " of the group: " + e.what());
      }
      if (i == 0) {
        off_epi = (uint32_t)one->d_trunk3.n;
        off_head = off_epi + RC3_EPI_WORDS;
        off_small = off_head + RCS_HEAD_WORDS(2);
        stride = off_small + RCG_SMALL_WORDS;
        d_w.alloc((size_t)models * stride, s);
      }
      uint32_t *dst = d_w.p + (size_t)i * stride;
      rt_d2d(dst, one->d_trunk3.p, (size_t)off_epi * 4, s);
      rt_d2d(dst + off_epi, one->d_epi3.p, (size_t)RC3_EPI_WORDS * 4, s);
      rt_d2d(dst + off_head, one->d_whead3.p, (size_t)RCS_HEAD_WORDS(2) * 4, s);
      rt_d2d(dst + off_small, one->P.head_epi, 48 * 4, s);
      rt_d2d(dst + off_small + 48, one->P.bpol, 96 * 4, s);
      rt_d2d(dst + off_small + 144, one->P.bv1, 64 * 4, s);
      rt_d2d(dst + off_small + 208, one->P.bv2, 4, s);
      rt_sync(s); /* (the model's own buffers go with `one`) */
    }
    range.alloc(s);
    rt_sync(s);
    rt_max_dynamic_lds(co_k_rescnn_forward_h3_grouped, RCS_LDS_WORDS(2, 1) * 4);
  }
  int kind() const override { return co_net_kind_of(CO_FAMILY_RESCNN4, 2, true); }
  int models() const override { return m; }
  size_t max_rows() const override { return cap; }
  bool grouped_kernel() const override { return true; }
  int tile() const override { return RCG_POS_PER_WG; }
  bool range_exceeded(rt_stream_t s) override { return range.read(s); }
  void forward(const float *d_in, int32_t rows_cap, const CoGroupPlan &plan, float *d_eval, float *d_probs, rt_stream_t s) override {
    int grid = rows_cap / RCG_POS_PER_WG + m; /* the worst case: every model ends in a partial workgroup */
    if (grid > plan.wg_cap) grid = plan.wg_cap;
    if (grid < 1 || plan.seg_stride) return;
    RcGroupParams g;
    g.in = d_in, g.wg = plan.wg, g.n_wg = plan.n_wg, g.idx = plan.idx, g.wbase = d_w.p;
    g.stride = stride, g.off_epi = off_epi, g.off_head = off_head, g.off_small = off_small;
    g.eval = d_eval, g.probs = d_probs, g.range_flag = range.ptr();
    RT_LAUNCH_LDS(co_k_rescnn_forward_h3_grouped, grid, 512, RCS_LDS_WORDS(2, 1) * 4, s, g);
  }
};

CoNetGroup *co_rescnn_h3_group_create(const float *const *weights, int models, size_t n_floats, size_t max_rows, rt_stream_t s) {
  if (n_floats != (size_t)CO_RESCNN4_NUM_WEIGHTS) return nullptr;
  return new ResCnnH3NetGroup(weights, models, max_rows, s);
}

CoNet *co_rescnn_create(const float *weights, size_t n_floats, size_t max_rows, rt_stream_t s) {
  if (n_floats != (size_t)CO_RESCNN4_NUM_WEIGHTS) return nullptr;
  return new ResCnnNet(weights, max_rows, s);
}

CoNet *co_rescnn_split_create(const float *weights, size_t n_floats, size_t max_rows, rt_stream_t s, int nterms, bool f16) {
  if (n_floats != (size_t)CO_RESCNN4_NUM_WEIGHTS || (nterms != 2 && nterms != 3) || (f16 && nterms != 2)) return nullptr;
  return new ResCnnSplitNet(weights, max_rows, s, nterms, f16);
}
