// nn_split.h -- what the split-precision kernels of both networks (nn_mlp_split.hip, nn_rescnn_split.h, nn_rescnn_pix.h)
// share: on the device the split of an fp32 pair into 16-bit terms, the MFMA on packed terms and the fp16 range guard; on
// the host the same split, the A-operand fragment order of v_mfma_f32_32x32x16 and the packers that put a network's
// weights into it.  The host part compiles under a plain host compiler with -DCO_EMU (tests/cxx/net_pack_driver.cpp).
#pragma once
#include <vector>

#include "host.h"

/* ---- geometry of the fragment buffers, shared by the packers and the kernels (NT = terms per operand)
 * mlp12x100: 13 layers (12 hidden + the heads) of 128 padded output features = four 32-wide tiles; a layer is two chunks
 * of four K steps plus a 4 KiB bias piece (nn_mlp_split.hip "weight stream") */
#define M3_NLAYERS 13
#define M3_NCHUNKS (2 * M3_NLAYERS)
#define M3_STEPS 7      /* hidden layers and heads: K = 112 */
#define M3_STEPS_L0 5   /* input layer: K = 80 */
#define M3_STEP_WORDS(NT) (4 * (NT) * 64 * 4) /* 4 output tiles x NT terms x 64 lanes x 4 words */
#define M3_BIAS_WORDS 1024                     /* 128 biases in a 4 KiB piece: one LDS-DMA per wave */
#define M3_CHUNK_WORDS(NT) (4 * M3_STEP_WORDS(NT) + M3_BIAS_WORDS) /* NT 2: 36 KB, NT 3: 52 KB */
#define M3_TOTAL_WORDS(NT) (M3_NCHUNKS * M3_CHUNK_WORDS(NT))
/* rescnn4: 64 output channels = two tiles; one chunk per tap of a convolution */
#define RCS_STEM_CHUNK(NT) (512 * (NT))  /* u32: 1 k-step x 2 out tiles x NT terms x 64 lanes x 4 */
#define RCS_CONV_CHUNK(NT) (2048 * (NT)) /* u32: 4 k-steps ... = 8 KB per term */
#define RCS_TRUNK_WORDS(NT) (9 * RCS_STEM_CHUNK(NT) + 72 * RCS_CONV_CHUNK(NT))
#define RCS_FRAG1_WORDS(NT) (4 * (NT) * 256) /* the heads' 1x1 convolutions: 4 k-steps x 1 tile */

#ifndef CO_EMU
/* ------------------------------------------------------------------ device */
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

/* (a, b) -> NT packed 16-bit pairs: the values rounded to bf16 (F16: to fp16), then the successive remainders
 * (each remainder is exact in float32, so with three bf16 terms they add up to the float32 value; two fp16
 * terms keep 2 x 11 = 22 significand bits) */
template <int NT, bool F16 = false>
__device__ __forceinline__ void co_split_pair(float a, float b, uint32_t (&t)[NT]) {
  if constexpr (F16 && NT == 2) {
    /* three instructions instead of five: the pair's first terms, then each second term as ONE mixed-precision fma,
     * f16(a - float(t0.lo)) -- the difference is exact in float32 (see above), so the one rounding is the conversion's,
     * as in the loop below: the same bits.  (An epilogue of the f16x3 kernels is vector-issue-bound: 336 -> 272
     * instructions per wave in the pixel-major kernel; round 5.) */
    const f32x2 v2 = {a, b};
    const uint32_t t0 = __builtin_bit_cast(uint32_t, __builtin_convertvector(v2, f16x2));
    uint32_t t1;
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %0, %1, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
        : "=&v"(t1)
        : "v"(t0), "v"(a), "v"(b));
    t[0] = t0;
    t[1] = t1;
    return;
  }
  f32x2 v = {a, b};
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    if constexpr (F16) {
      f16x2 hb = __builtin_convertvector(v, f16x2);
      t[i] = __builtin_bit_cast(uint32_t, hb);
      if (i + 1 < NT) {
        f32x2 hf = __builtin_convertvector(hb, f32x2);
        v = (f32x2){v.x - hf.x, v.y - hf.y};
      }
    } else {
      bf16x2 hb = __builtin_convertvector(v, bf16x2);
      t[i] = __builtin_bit_cast(uint32_t, hb);
      if (i + 1 < NT) {
        f32x2 hf = __builtin_convertvector(hb, f32x2);
        v = (f32x2){v.x - hf.x, v.y - hf.y};
      }
    }
  }
}

/* acc += a b: one v_mfma_f32_32x32x16 on packed 16-bit operands, bf16 terms or fp16 terms */
template <bool F16>
__device__ __forceinline__ void co_mfma_32x32x16(f32x16 &acc, const u32x4 &a, const u32x4 &b) {
  if constexpr (F16)
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
  else
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}

/* The range guard of the f16x3 kinds (nn.h range_exceeded) follows the FIRST terms as they are split: the running maximum
 * of the packed fp16 pairs, one v_pk_max_f16 per pair of activations (on the float32 values it was two v_max_f32 per pair
 * in a vector-issue-bound epilogue).  What is split is an input plane or the output of a ReLU, never negative; an
 * activation beyond fp16's range has the first term +inf -- exactly the event the guard reports (a NaN can only follow an
 * infinity, which is reported when it appears). */
__device__ __forceinline__ uint32_t co_pk_max_f16(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_pk_max_f16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ bool co_pk_f16_finite(uint32_t pk) { return (pk & 0x7FFFu) < 0x7C00u && ((pk >> 16) & 0x7FFFu) < 0x7C00u; }
/* the end of a kernel: raise the network's flag if the running maximum left the range (never in range: no lane enters) */
__device__ __forceinline__ void co_raise_unless_f16_finite(uint32_t amax, uint32_t *range_flag) {
  if (!co_pk_f16_finite(amax)) atomicOr(range_flag, 1u);
}
#endif

/* ------------------------------------------------------------------ host */
/* ---- 16-bit operand terms, as the host packs them */
inline uint16_t bf16_rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint32_t a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40); /* NaN: the rounding add could carry a full mantissa into a finite number */
  if (a >= 0x7f7f8000u && a < 0x7f800000u) return (uint16_t)(u >> 16); /* ... or a finite one to infinity: the largest bf16, the next term takes the rest */
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline float bf16_to_f(uint16_t h) {
  uint32_t u = (uint32_t)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
/* float -> IEEE binary16, round to nearest even, subnormals kept (what v_cvt_f16_f32 gives); in integer arithmetic, so
 * that a host compiler without a 16-bit float type gives the same bits */
inline uint16_t f16_rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint32_t sign = (u >> 16) & 0x8000u;
  u &= 0x7fffffffu;
  if (u > 0x7f800000u) return (uint16_t)(sign | 0x7e00u | ((u >> 13) & 0x1ffu)); /* NaN */
  if (u >= 0x47800000u) return (uint16_t)(sign | 0x7c00u);                        /* 2^16 and beyond, infinity */
  uint32_t r, rem, half;
  if (u < 0x38800000u) { /* below 2^-14: a multiple of fp16's subnormal quantum 2^-24 */
    if (u <= 0x33000000u) return (uint16_t)sign; /* up to 2^-25, the tie included: zero */
    const int shift = 126 - (int)(u >> 23);      /* 14 .. 24 */
    const uint32_t m = (u & 0x7fffffu) | 0x800000u;
    r = m >> shift;
    rem = m & ((1u << shift) - 1u);
    half = 1u << (shift - 1);
  } else {
    r = (u - 0x38000000u) >> 13; /* exponent rebiased; a carry out of the mantissa below is the next exponent (65520: infinity) */
    rem = u & 0x1fffu;
    half = 0x1000u;
  }
  if (rem > half || (rem == half && (r & 1u))) ++r;
  return (uint16_t)(sign | r);
}
inline float f16_to_f(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
  float f;
  if (e == 0) { /* zero or subnormal: m quanta of 2^-24, exact */
    f = (float)m * 5.9604644775390625e-8f;
    return sign ? -f : f;
  }
  const uint32_t u = sign | (e == 31 ? 0x7f800000u : (e + 112u) << 23) | (m << 13);
  memcpy(&f, &u, 4);
  return f;
}
/* v -> nt 16-bit terms: bf16(v) (f16: fp16(v)), the same of the remainder, ... (the device's co_split_pair).  An f16
 * caller checks the range first (co_f16_weight). */
inline void split_terms(float v, int nt, bool f16, uint16_t *out) {
  for (int i = 0; i < nt; ++i) {
    out[i] = f16 ? f16_rne(v) : bf16_rne(v);
    v = v - (f16 ? f16_to_f(out[i]) : bf16_to_f(out[i]));
  }
}

/* A weight beyond fp16's largest finite value would become an infinite term (nn.h range_exceeded): an f16x3 network is
 * refused at its creation, in the words its constructor puts around the value. */
struct F16RangeText {
  std::string before, after;
};
inline void co_f16_weight(float v, const F16RangeText &m) {
  if (!(fabsf(v) <= CO_F16_MAX)) throw std::invalid_argument(m.before + std::to_string(v) + m.after);
}

/* ---- The A-operand fragment order of v_mfma_f32_32x32x16, once.  ONE K step `st` (16 values of k) of `tiles` 32-wide
 * output tiles, term-major inside a tile: dst[((tile * nt + term) * 64 + lane) * 4 + word], every word written.  Lane
 * 32 h + i holds output o = 32 tile + i; its k-slot (h, j), j = 0..7, is
 *     k = 32 T + 8 (2 a + j / 4) + 4 h + j % 4,   st = 2 T + a,
 * in half j & 1 of word j / 2 -- the order in which the accumulator registers of one layer are the B operand of the next
 * (nn_mlp_split.hip, nn_rescnn_split.h).  weight(k, o) -> float gives the value; f16: checked against `range`. */
template <class Fn>
inline void co_pack_step(uint32_t *dst, int tiles, int st, int nt, bool f16, const F16RangeText &range, Fn &&weight) {
  const int T = st >> 1, a = st & 1;
  for (int to = 0; to < tiles; ++to)
    for (int h = 0; h < 2; ++h)
      for (int i = 0; i < 32; ++i)
        for (int m = 0; m < 4; ++m) {
          uint16_t term[2][3];
          for (int half = 0; half < 2; ++half) {
            const int j = 2 * m + half;
            const float v = weight(32 * T + 8 * (2 * a + (j >> 2)) + 4 * h + (j & 3), 32 * to + i);
            if (f16) co_f16_weight(v, range);
            split_terms(v, nt, f16, term[half]);
          }
          for (int t = 0; t < nt; ++t)
            dst[(((size_t)to * nt + t) * 64 + 32 * h + i) * 4 + m] = (uint32_t)term[0][t] | (uint32_t)term[1][t] << 16;
        }
}

/* ---- the networks' fragment buffers from their flat weights (nn_layout.h)
 * mlp12x100: float64 copies of the 13 dense layers with BatchNorm l folded into layer l + 1 (as the TFLite converter does
 * for the reference's own checkpoints), the heads as one layer (features 0..95 policy, 96 value); chunk 2l holds steps
 * 0..3 of layer l and its 128 biases, chunk 2l + 1 steps 4.. */
inline std::vector<uint32_t> co_pack_mlp_split(const float *w, int nt, bool f16) {
  constexpr MlpLayout ML;
  constexpr int W = ML.W;
  std::vector<double> K[M3_NLAYERS], B[M3_NLAYERS];
  std::vector<double> a_prev, c_prev;
  auto fold = [&](int l, int kern, int bias, int nin, int nout, int out_base) {
    /* K[l][k * 128 + out_base + o], B[l][out_base + o] */
    for (int o = 0; o < nout; ++o) {
      double b = w[bias + o];
      for (int k = 0; k < nin; ++k) {
        double wv = w[kern + (size_t)k * nout + o];
        if (!a_prev.empty()) {
          b += c_prev[k] * wv;
          wv *= a_prev[k];
        }
        K[l][(size_t)k * 128 + out_base + o] = wv;
      }
      B[l][out_base + o] = b;
    }
  };
  for (int l = 0; l < M3_NLAYERS; ++l) {
    K[l].assign((size_t)128 * 128, 0.0);
    B[l].assign(128, 0.0);
    if (l == ML.LAYERS) {
      fold(l, ML.kp, ML.bp, W, ML.MOVES, 0);
      fold(l, ML.kv, ML.bv, W, 1, ML.MOVES);
      break;
    }
    fold(l, ML.kernel(l), ML.bias(l), ML.in_dim(l), W, 0);
    /* the float32 constants K5 applies (BatchNormalization inference, eps 1e-3) */
    float a[W], c[W];
    bn_fold(w, ML, l, W, a, c);
    a_prev.assign(a, a + W);
    c_prev.assign(c, c + W);
  }
  const size_t step_words = M3_STEP_WORDS(nt), chunk_words = M3_CHUNK_WORDS(nt);
  std::vector<uint32_t> buf(M3_TOTAL_WORDS(nt), 0u);
  for (int l = 0; l < M3_NLAYERS; ++l) {
    const F16RangeText range{"mlp12x100h3: a weight of layer " + std::to_string(l) + " is ",
                             " after the BatchNorm fold, beyond the fp16 range of the f16x3 kernels: use mlp12x100x6"};
    const int ns = l == 0 ? M3_STEPS_L0 : M3_STEPS, kin = ML.in_dim(l);
    for (int st = 0; st < ns; ++st)
      co_pack_step(&buf[((size_t)2 * l + (st >> 2)) * chunk_words + (size_t)(st & 3) * step_words], 4, st, nt, f16, range,
                   [&](int k, int o) { return k < kin ? (float)K[l][(size_t)k * 128 + o] : 0.0f; });
    for (int o = 0; o < 128; ++o) {
      float b = (float)B[l][o];
      memcpy(&buf[(size_t)2 * l * chunk_words + 4 * step_words + o], &b, 4);
    }
  }
  return buf;
}

inline const F16RangeText &co_rescnn_f16_range() {
  static const F16RangeText t{"rescnn4h3: a convolution weight is ", ", beyond the fp16 range of the f16x3 kernels: use rescnn4x6"};
  return t;
}

/* rescnn4's nine 3x3 convolutions: per convolution nine tap chunks of its K steps (stem: 1, channels >= 10 zero; else 4) */
inline std::vector<uint32_t> co_pack_rescnn_trunk(const float *w, int nt, bool f16) {
  constexpr ResCnnLayout RL;
  std::vector<uint32_t> tr(RCS_TRUNK_WORDS(nt), 0u);
  size_t off = 0;
  for (int cv = 0; cv < RL.CONVS; ++cv) {
    const int cin = RL.cin(cv), cs = cv == 0 ? 1 : 4;
    const size_t chunk = cv == 0 ? RCS_STEM_CHUNK(nt) : RCS_CONV_CHUNK(nt);
    const float *K = w + RL.kernel(cv); /* [3][3][cin][64] */
    for (int tap = 0; tap < 9; ++tap)
      for (int st = 0; st < cs; ++st)
        co_pack_step(&tr[off + tap * chunk + (size_t)st * 2 * nt * 256], 2, st, nt, f16, co_rescnn_f16_range(),
                     [&](int ci, int co) { return ci < cin ? K[((size_t)tap * cin + ci) * 64 + co] : 0.0f; });
    off += 9 * chunk;
  }
  return tr;
}

/* rescnn4's 1x1 head convolutions as one more K loop of one tile: output row 0..3 policy planes, 4..5 value planes, the
 * rest zero */
inline std::vector<uint32_t> co_pack_rescnn_head(const float *w, int nt, bool f16) {
  constexpr ResCnnLayout RL;
  const float *pk = w + RL.p_k, *vk = w + RL.v_k;
  std::vector<uint32_t> wh(RCS_FRAG1_WORDS(nt), 0u);
  for (int st = 0; st < 4; ++st)
    co_pack_step(&wh[(size_t)st * nt * 256], 1, st, nt, f16, co_rescnn_f16_range(),
                 [&](int k, int o) { return o < 4 ? pk[k * 4 + o] : o < 6 ? vk[k * 2 + (o - 4)] : 0.0f; });
  return wh;
}
