// nn_rescnn_split.h -- part of nn_rescnn.hip's translation unit (included there, behind the fp32 kernel and the heads the
// families share): the split-precision kernels of rescnn4 on (position, pixel) columns.
#pragma once
/* ======================================================================
 * Split-precision variants (CO_NET_RESCNN4_X3: NT = 2 terms, CO_NET_RESCNN4_X6: NT = 3 terms):
 * same network, same weights, same register-resident structure, but every 3x3 convolution runs
 * on the bf16 matrix pipe with both operands written as a sum of NT bf16 values,
 *   x = x0 + x1 (+ x2),  x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1),
 * and the product expanded into the terms w_i x_j with i + j <= NT - 1 (fp32 accumulation in the
 * MFMA):
 *   NT = 2 ("bf16x3"): 16 significand bits kept, 3 MFMAs; dropped terms ~2^-16 |x w|.  Within
 *           2e-5 of the float32 restatement -- narrower than the reference's float32 arithmetic.
 *   NT = 3 ("bf16x6"): x0 + x1 + x2 IS the float32 value (3 x 8 = 24 significand bits, the
 *           remainders are exact), 6 MFMAs; the dropped terms w1 x2, w2 x1, w2 x2 are <= 2^-24
 *           |x w| each -- the size of ONE float32 rounding of the product, and there are fewer
 *           accumulator roundings than in the fp32 MFMA chain (one per 16 products instead of one
 *           per product).  Measured against a float64 restatement the error is that of K6 (fp32
 *           MFMA) or smaller (tests/test_net_precision.py): float32-equivalent arithmetic at 16/6 =
 *           2.7x the fp32 matrix rate.
 *
 * v_mfma_f32_32x32x16_bf16 (an MFMA of this shape occupies the SIMD's issue port for 8 of
 * its 32 cycles; the 16x16x32 shape for 8 of 16, which left too little room for the DPP
 * shifts).  Its 32 columns are TWO positions (lane & 31 = position*16 + pixel), its 32 rows
 * half of the 64 output channels.  A lane (h = lane >> 5) owns 16 channels of each row tile
 * T: channel 32T + 4h + 8g + i in accumulator register 4g + i.  One K step = 16 input
 * channels = the lane's registers 8a..8a+7 of tile T (k-slot (h, j) <-> channel
 * 32T + 4h + 8(2a + j/4) + j%4), packed two bf16 per VGPR: again the output layout of one
 * layer is the operand layout of the next, and the tap shift is the same DPP row shift
 * (a row of 16 lanes = one position), now on packed pairs.
 * Bias, BatchNorm, residual adds and the heads stay in fp32.
 * Geometry: 512 threads = 8 waves (two per SIMD), NP position pairs per wave. */
/* NP = position pairs per wave.  NT = 2: 2 in the throughput kernel (32 positions per workgroup), 1 in
 * the small-batch kernel (16 per workgroup: half the MFMA work behind the same weight stream, so a
 * batch that fits one round of workgroups comes back sooner -- the thinning tail of a generation
 * runs hundreds of such iterations, each as long as its slowest kernel).  NT = 3: 1 (three packed
 * operand sets + three weight fragment sets leave no registers for a second pair at two waves per
 * SIMD; the MFMA work per weight byte is that of NT = 2, NP = 2 again). */
#define RC3_SMALL_ROWS 4096 /* NT = 2: batches up to this size take the small-batch kernel: <= 256 workgroups */
#define RC6_THIN_ROWS 2048  /* NT = 3: batches up to this size take the four-wave kernel: <= 256 workgroups of 8 positions */
/* (the fragment buffers' geometry, RCS_STEM_CHUNK .. RCS_FRAG1_WORDS: nn_split.h) */
#define RC3_EPI_WORDS 1792 /* 9 convolutions x (bias, BN scale, BN shift)[64], padded to whole 256-word pieces */
/* head weights: 1x1 fragments (4 steps x NT terms x 64 lanes x 4 words), then the fp32 dense weights in
 * MFMA order: policy dense (6144), value dense 1 (2048), value dense 2 (1024) */
#define RCS_DENSE_WORDS (6144 + 2048 + 1024)
#define RCS_HEAD_WORDS(NT) (RCS_FRAG1_WORDS(NT) + RCS_DENSE_WORDS)
/* weights stream through LDS in groups of three taps (one kernel row): 27 groups, group
 * gi < 3 belongs to the stem */
#define RC3_NUM_GROUPS 27
#define RCS_GROUP_WORDS(NT) (3 * RCS_CONV_CHUNK(NT)) /* 48 KB / 72 KB */
#define RCS_FEAT_WORDS(NP) (8 * 2 * (NP) * 96)
/* LDS: [2 weight groups][NT = 2: head features][epilogue constants][NT = 2: head weights].  With three
 * terms the head weights do not fit beside two 72 KB groups: they are staged into the idle group
 * buffer while the last group computes, and the head features go where the last group was once every
 * wave has left it.  151 KB: what is left of the CU's 160 KB (and of its registers, see the kernel's
 * attributes) is room for wavefronts of the search kernel beside this one. */
#define RCS_LDS_WORDS(NT, NP) \
  (2 * RCS_GROUP_WORDS(NT) + ((NT) == 2 ? RCS_FEAT_WORDS(NP) : 0) + RC3_EPI_WORDS + ((NT) == 2 ? RCS_HEAD_WORDS(NT) : 0))

struct Rc3Params {
  RcParams base;          /* dense heads + epilogue parameters, in/out pointers */
  const uint32_t *wtrunk; /* RCS_TRUNK_WORDS, bf16 term fragments */
  const uint32_t *whead3; /* RCS_HEAD_WORDS: [4 steps][NT terms][64 lanes][4 words] 1x1 head convs in fragment order,
                           * then the fp32 dense weights wpol, wv1, wv2 as in RcParams */
  const uint32_t *epi3;   /* RC3_EPI_WORDS: RcParams::epi, padded */
  uint32_t *range_flag;   /* f16x3: raised when an activation beyond fp16's range was split (nn.h range_exceeded) */
  int32_t pass_rows;      /* f16x3 with the pixel-major kernel: rows of one pass of that kernel over the chip (32 per CU);
                           * 0 = batches are not split between the kernels (rcp_small_begin) */
};

/* Which rows of a batch does the small-batch kernel take?  Without the pixel-major kernel: all of a batch of up to
 * RC3_SMALL_ROWS rows, none of a larger one.  With it the batch is SPLIT on the device: the pixel-major kernel runs one
 * workgroup of 32 rows per CU and a pass costs its full time however few of its workgroups have rows, so it takes the
 * whole passes of the batch, plus a remainder of more than RC3_SMALL_ROWS rows; a smaller remainder -- half of all
 * batches -- goes to the small-batch kernel (16 rows per workgroup; 8 on its thin path), which is through in a third to two
 * thirds of a pass.  A row's result does not depend on the kernel that evaluates it.  -> the small kernel's first row
 * (Only for a launch that has the GPU to itself, CoNetIO::alone: measured in round 4, 10 000 / 12 288 / 20 000 rows alone
 * 0.185 / 0.217 / 0.345 ms against 0.27 / 0.26 / 0.40 unsplit -- but beside the other pool's kernels, where CUs and not
 * latency are scarce, the pixel-major kernel's 32 rows per 160 us of a CU beat the small kernel's 16 per 110: a
 * two-pool generation 438.7 ms split against 434.0 unsplit.) */
__device__ __forceinline__ int rcp_small_begin(const Rc3Params &Q, int rows) {
  /* (a batch the host queues no throughput kernel for -- rows_cap <= RC3_SMALL_ROWS -- is the small kernel's whole,
   * whatever a pass is: on a device or partition of <= 128 CUs a pass is <= RC3_SMALL_ROWS rows, and `full` below would
   * hand rows to a kernel that was never launched) */
  if (rows <= RC3_SMALL_ROWS) return 0;
  if (Q.pass_rows <= 0) return rows;
  const int full = rows / Q.pass_rows * Q.pass_rows;
  return rows - full > RC3_SMALL_ROWS ? rows : full;
}

template <int NT>
__device__ __forceinline__ const uint32_t *rcs_group_ptr(const uint32_t *wtrunk, int gi) {
  return gi < 3 ? wtrunk + gi * 3 * RCS_STEM_CHUNK(NT) : wtrunk + 9 * RCS_STEM_CHUNK(NT) + (gi - 3) * 3 * RCS_CONV_CHUNK(NT);
}

/* LDS-DMA of `words` (a multiple of 256) by the eight waves of the workgroup (lds_dma.h: the waits
 * are the kernel's own) */
__device__ __forceinline__ void rcs_stage_words(const uint32_t *src, uint32_t lds_addr, int words, int wave, int lane,
                                                int nw = 8) {
  const int pieces = words / 256;
  for (int p = wave; p < pieces; p += nw) co_lds_dma_1k(src + p * 256 + lane * 4, lds_addr + (uint32_t)p * 1024u);
}

template <int NT>
__device__ __forceinline__ void rcs_stage(const uint32_t *wtrunk, uint32_t lds_addr, int gi, int wave, int lane, int nw = 8) {
  rcs_stage_words(rcs_group_ptr<NT>(wtrunk, gi), lds_addr, gi < 3 ? 3 * RCS_STEM_CHUNK(NT) : 3 * RCS_CONV_CHUNK(NT), wave, lane, nw);
}

template <int S>
__device__ __forceinline__ uint32_t rc3_row_shift(uint32_t v) {
  if (S == 0) return v;
  constexpr int ctrl = S > 0 ? (0x100 + S) : (0x110 - S);
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, ctrl, 0xF, 0xF, true);
}

/* The four packed words of one B operand shifted to tap (dy, dx).  For dx != 0 the shift and
 * the zeroing of the lanes whose source pixel lies in the neighbouring board row are ONE
 * instruction, v_cndmask_b32 with a DPP source: D = vcc ? 0 : row_shift(v) with vcc = the wrap
 * lanes (x = 0 for dx = -1, x = 3 for dx = +1; a constant lane pattern).  As two instructions
 * (v_mov_b32_dpp + v_cndmask_b32_e64) the B-operand preparation took 2.7 vector issues per MFMA
 * and, with two waves per SIMD, left the issue port nearly full.  The trailing s_nop 1 covers
 * the VALU-write -> MFMA-read wait states that the compiler cannot see into the asm for. */
#define RC3_CNDMASK_DPP4(CTRL)                                                                          \
  asm("s_mov_b64 vcc, %[m]\n\t"                                                                         \
      "v_cndmask_b32_dpp %[o0], %[i0], %[z], vcc " CTRL " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"   \
      "v_cndmask_b32_dpp %[o1], %[i1], %[z], vcc " CTRL " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"   \
      "v_cndmask_b32_dpp %[o2], %[i2], %[z], vcc " CTRL " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"   \
      "v_cndmask_b32_dpp %[o3], %[i3], %[z], vcc " CTRL " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"   \
      "s_nop 1"                                                                                         \
      : [o0] "=&v"(o0), [o1] "=&v"(o1), [o2] "=&v"(o2), [o3] "=&v"(o3)                                  \
      : [i0] "v"(in[0]), [i1] "v"(in[1]), [i2] "v"(in[2]), [i3] "v"(in[3]), [z] "v"(zero), [m] "s"(wrap) \
      : "vcc")

template <int TAP>
__device__ __forceinline__ u32x4 rc3_tap4(const uint32_t (&in)[4], uint32_t zero) {
  constexpr int dy = TAP / 3 - 1, dx = TAP % 3 - 1;
  u32x4 out;
  if constexpr (dx == 0) {
#pragma unroll
    for (int m = 0; m < 4; ++m) out[m] = rc3_row_shift<4 * dy>(in[m]);
  } else {
    const unsigned long long wrap = dx < 0 ? 0x1111111111111111ull : 0x8888888888888888ull;
    uint32_t o0, o1, o2, o3;
    if constexpr (4 * dy + dx == -5) RC3_CNDMASK_DPP4("row_shr:5");
    if constexpr (4 * dy + dx == -3) RC3_CNDMASK_DPP4("row_shr:3");
    if constexpr (4 * dy + dx == -1) RC3_CNDMASK_DPP4("row_shr:1");
    if constexpr (4 * dy + dx == 1) RC3_CNDMASK_DPP4("row_shl:1");
    if constexpr (4 * dy + dx == 3) RC3_CNDMASK_DPP4("row_shl:3");
    if constexpr (4 * dy + dx == 5) RC3_CNDMASK_DPP4("row_shl:5");
    out[0] = o0;
    out[1] = o1;
    out[2] = o2;
    out[3] = o3;
  }
  return out;
}

/* tap as a value: after full unrolling every call site has a constant tap and folds to one case */
__device__ __forceinline__ u32x4 rc3_tap4_sel(const uint32_t (&in)[4], int tap, uint32_t zero) {
  switch (tap) {
    case 0: return rc3_tap4<0>(in, zero);
    case 1: return rc3_tap4<1>(in, zero);
    case 2: return rc3_tap4<2>(in, zero);
    case 3: return rc3_tap4<3>(in, zero);
    case 4: return rc3_tap4<4>(in, zero);
    case 5: return rc3_tap4<5>(in, zero);
    case 6: return rc3_tap4<6>(in, zero);
    case 7: return rc3_tap4<7>(in, zero);
    default: return rc3_tap4<8>(in, zero);
  }
}

/* One staged group = taps 3G .. 3G + 2, CS K steps each.  p[t][np][s][m]: term t, K step s = 2T + a,
 * word m = channels (reg 8a + 2m, 8a + 2m + 1) of tile T.  The weight fragments of step i + 1
 * (also across the tap boundary) are requested from LDS before the MFMAs of step i issue (two
 * register sets), so the LDS latency is paid once per group.  Products w_i x_j, i + j <= NT - 1,
 * largest first. */
template <int CS, int G, int NP, int NT, bool F16 = false>
__device__ __forceinline__ void rcs_conv_group(f32x16 (&acc)[NP][2], const uint32_t (&p)[NT][NP][4][4], const uint32_t *wg,
                                               int lane) {
  /* terms the B operand has: the stem's inputs (board bits 0 / 1, reserves k / 4) are exact in bf16 */
  constexpr int XT = CS == 1 ? 1 : NT;
  constexpr int tw = CS == 1 ? RCS_STEM_CHUNK(NT) : RCS_CONV_CHUNK(NT);
  constexpr int N = 3 * CS;
  uint32_t zero;
  asm("v_mov_b32 %0, 0" : "=v"(zero)); /* a zero the compiler keeps in a VGPR (second cndmask source) */
  u32x4 a[2][NT][2];
#pragma unroll
  for (int to = 0; to < 2; ++to)
#pragma unroll
    for (int t = 0; t < NT; ++t) a[0][t][to] = *reinterpret_cast<const u32x4 *>(wg + (((0 * 2 + to) * NT + t) * 64 + lane) * 4);
#pragma unroll
  for (int idx = 0; idx < N; ++idx) {
    const int cur = idx & 1, nxt = cur ^ 1;
    const int tg = idx / CS, s = idx % CS;
    if (idx + 1 < N) {
      const int tg1 = (idx + 1) / CS, s1 = (idx + 1) % CS;
      const uint32_t *w1 = wg + tg1 * tw;
#pragma unroll
      for (int to = 0; to < 2; ++to)
#pragma unroll
        for (int t = 0; t < NT; ++t)
          a[nxt][t][to] = *reinterpret_cast<const u32x4 *>(w1 + (((s1 * 2 + to) * NT + t) * 64 + lane) * 4);
    }
#pragma unroll
    for (int np = 0; np < NP; ++np) {
      u32x4 B[XT];
#pragma unroll
      for (int t = 0; t < XT; ++t) B[t] = rc3_tap4_sel(p[t][np][s], 3 * G + tg, zero);
#pragma unroll
      for (int sum = 0; sum < NT; ++sum)
#pragma unroll
        for (int i = 0; i <= sum; ++i)
          if (sum - i < XT) {
#pragma unroll
            for (int to = 0; to < 2; ++to)
              co_mfma_32x32x16<F16>(acc[np][to], a[cur][i][to], B[sum - i]);
          }
    }
  }
}

template <int CS, int NP, int NT, int NW, bool F16 = false>
__device__ __forceinline__ void rcs_conv3x3(f32x16 (&acc)[NP][2], const uint32_t (&p)[NT][NP][4][4], int &ch,
                                            const Rc3Params &Q, uint32_t *lds_w, uint32_t lds_w_addr, int wave, int lane) {
#pragma unroll
  for (int np = 0; np < NP; ++np)
#pragma unroll
    for (int to = 0; to < 2; ++to)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[np][to][i] = 0.0f;
#define RC3_GROUP(G)                                                                                              \
  {                                                                                                               \
    CO_WAIT_VMCNT(0); /* group ch has landed (requested one group ago) */                                         \
    co_wg_barrier();  /* ... for every wave, and everyone has left the other buffer */                            \
    if (ch + 1 < RC3_NUM_GROUPS)                                                                                  \
      rcs_stage<NT>(Q.wtrunk, lds_w_addr + (uint32_t)((ch + 1) & 1) * (RCS_GROUP_WORDS(NT) * 4u), ch + 1, wave, lane, NW); \
    else if (NT != 2) /* the head weights ride in the buffer the last group leaves idle */                        \
      rcs_stage_words(Q.whead3, lds_w_addr + (uint32_t)((ch + 1) & 1) * (RCS_GROUP_WORDS(NT) * 4u), RCS_HEAD_WORDS(NT), wave, lane, NW); \
    rcs_conv_group<CS, G, NP, NT, F16>(acc, p, lds_w + (ch & 1) * RCS_GROUP_WORDS(NT), lane);                          \
    ++ch;                                                                                                         \
  }
  RC3_GROUP(0) RC3_GROUP(1) RC3_GROUP(2)
#undef RC3_GROUP
}

/* fp32 tile values -> the packed operands of the next convolution */
template <int NP, int NT, bool F16 = false>
__device__ __forceinline__ void rcs_pack(uint32_t (&p)[NT][NP][4][4], const float (&v)[NP][2][16], uint32_t &amax) {
#pragma unroll
  for (int np = 0; np < NP; ++np)
#pragma unroll
    for (int T = 0; T < 2; ++T)
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          uint32_t t[NT];
          /* (what is packed is an input plane or the output of a ReLU: never negative) */
          co_split_pair<NT, F16>(v[np][T][8 * a + 2 * m], v[np][T][8 * a + 2 * m + 1], t);
          if constexpr (F16) amax = co_pk_max_f16(amax, t[0]);
#pragma unroll
          for (int i = 0; i < NT; ++i) p[i][np][2 * T + a][m] = t[i];
        }
}

/* conv bias -> BatchNorm affine (-> + skip) -> ReLU; register 4g + i of tile T is channel
 * 32T + 8g + 4h + i */
template <bool ADD_SKIP, int NP>
__device__ __forceinline__ void rc3_epilogue(float (&out)[NP][2][16], const f32x16 (&acc)[NP][2],
                                             const float (&skip)[NP][2][16], const float *epi, int h) {
#pragma unroll
  for (int T = 0; T < 2; ++T)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int chn = 32 * T + 8 * g + 4 * h;
      const float4 b4 = *reinterpret_cast<const float4 *>(epi + chn);
      const float4 a4 = *reinterpret_cast<const float4 *>(epi + 64 + chn);
      const float4 c4 = *reinterpret_cast<const float4 *>(epi + 128 + chn);
      const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
      const float aa[4] = {a4.x, a4.y, a4.z, a4.w};
      const float cc[4] = {c4.x, c4.y, c4.z, c4.w};
      float cb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) cb[i] = __builtin_fmaf(aa[i], bb[i], cc[i]);
#pragma unroll
      for (int np = 0; np < NP; ++np)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          /* a (acc + bias) + c as one fma on the folded shift cb = a bias + c */
          float v = __builtin_fmaf(aa[i], acc[np][T][4 * g + i], cb[i]);
          if (ADD_SKIP) v = skip[np][T][4 * g + i] + v;
          v = v > 0.0f ? v : 0.0f;
          out[np][T][4 * g + i] = v;
        }
    }
}

#ifdef CO_PROF
/* diagnostic builds: cycles of wave 0 of every workgroup by phase (tools/prof_nn.py) */
__device__ unsigned long long rc3_prof[12]; /* 0..5 phases, 6 whole pass, 7 passes, 8 whole pass in 100 MHz ticks; K6p only: 9 waited for the
                                             * weight DMA, 10 waited at the tap barrier, 11 multiplied (inside phases 1 and 3) */
#define RC3_STAMP(slot)                                                              \
  {                                                                                  \
    unsigned long long now_ = __builtin_readcyclecounter();                          \
    if (tid == 0) atomicAdd(&rc3_prof[slot], now_ - stamp_);                         \
    stamp_ = now_;                                                                   \
  }
extern "C" int ca_net_prof(unsigned long long out[12]) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(rc3_prof), sizeof(rc3_prof)) == hipSuccess ? 0 : 1;
}
/* K6p: the core-clock stamps of workgroup 0's eight waves at the nine tap barriers of ONE trunk convolution (the fifth
 * convolution of the kernel): [wave][tap][arrived, left], [wave][18] = the convolution's end (tools/prof_nn.py with NN_TRACE=1) */
__device__ unsigned rc3_trace[8 * 20];
extern "C" int ca_net_trace(unsigned out[160]) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(rc3_trace), sizeof(rc3_trace)) == hipSuccess ? 0 : 1;
}
#else
#define RC3_STAMP(slot)
#endif

/* NW = waves per workgroup: 8 (two per SIMD), or 4 in the thin-batch kernel of NT = 3 (below) */
/* GROUPED (the grouped instance below): the workgroup's positions are rbase .. g_end - 1 of the launch, not the ones its
 * index gives it */
template <int NP, int NT, int NW = 8, bool F16 = false, bool GROUPED = false>
__device__ __forceinline__ void rcs_forward(const Rc3Params &Q, const int rbase = 0, const int g_end = 0) {
  const RcParams &P = Q.base;
  extern __shared__ __attribute__((aligned(16))) uint32_t lds_dyn[];
  uint32_t *lds_w = lds_dyn;
  /* NT = 3: the features reuse the buffer of the last group (RC3_NUM_GROUPS - 1 = 26 -> buffer 0), free behind
   * the barrier in front of the heads */
  float *lds_feat = reinterpret_cast<float *>(NT == 2 ? lds_dyn + 2 * RCS_GROUP_WORDS(NT) : lds_dyn);
  const int rows = GROUPED ? g_end : *P.d_rows; /* this launch works on rows rbase .. rows - 1 */
  if (!GROUPED && NT == 2 && (rows - rbase <= RC3_SMALL_ROWS) != (NP == 1)) return; /* the other kernel takes this batch */
  const int row0 = GROUPED ? rbase : rbase + (int)blockIdx.x * (2 * NP * NW);
  if (row0 >= rows) return;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, h = lane >> 5, p2 = (lane >> 4) & 1, c = lane & 15;
#ifdef CO_PROF
  unsigned long long stamp_ = __builtin_readcyclecounter();
  const unsigned long long start_ = stamp_, real_ = __builtin_amdgcn_s_memrealtime();
#endif
  const uint32_t lds_w_addr = co_lds_addr(lds_dyn);
  constexpr int epi_off = 2 * RCS_GROUP_WORDS(NT) + (NT == 2 ? RCS_FEAT_WORDS(NP) : 0);
  uint32_t *lds_epi_w = lds_dyn + epi_off;
  const uint32_t lds_epi_addr = lds_w_addr + epi_off * 4u;
  const uint32_t *lds_head = NT == 2 ? lds_epi_w + RC3_EPI_WORDS : lds_w + (RC3_NUM_GROUPS & 1) * RCS_GROUP_WORDS(NT);

  /* input planes: register 4g + i of tile 0 = channel 8g + 4h + i:
   * g 0: h 0 the cell's board bits, h 1 reserves 0..3; g 1: h 0 reserves 4..5 (+ padding), h 1 zeros */
  float x[NP][2][16];
#pragma unroll
  for (int np = 0; np < NP; ++np) {
    const int pos = row0 + wave * (2 * NP) + np * 2 + p2;
#pragma unroll
    for (int T = 0; T < 2; ++T)
#pragma unroll
      for (int i = 0; i < 16; ++i) x[np][T][i] = 0.0f;
    if (pos < rows) {
      const float *row = P.in + rc_in_row(P, pos) * CO_STATE_STRIDE;
      const float4 v0 = *reinterpret_cast<const float4 *>(row + (h == 0 ? 4 * c : 64));
      const float4 v1 = *reinterpret_cast<const float4 *>(row + (h == 0 ? 68 : 72));
      x[np][0][0] = v0.x; x[np][0][1] = v0.y; x[np][0][2] = v0.z; x[np][0][3] = v0.w;
      x[np][0][4] = v1.x; x[np][0][5] = v1.y; x[np][0][6] = v1.z; x[np][0][7] = v1.w;
    }
  }
  uint32_t pk[NT][NP][4][4];
  uint32_t amax = 0u; /* (packed fp16 pair: co_pk_max_f16) */
  rcs_pack<NP, NT, F16>(pk, x, amax);
  /* weight stream, requested behind the input loads (vmcnt retires in issue order): group 0, the
   * epilogue constants and, with two terms, the head weights (the wait before the first MFMA
   * covers them) */
  rcs_stage<NT>(Q.wtrunk, lds_w_addr, 0, wave, lane, NW);
  rcs_stage_words(Q.epi3, lds_epi_addr, RC3_EPI_WORDS, wave, lane, NW);
  if (NT == 2) rcs_stage_words(Q.whead3, lds_epi_addr + RC3_EPI_WORDS * 4u, RCS_HEAD_WORDS(NT), wave, lane, NW);
  RC3_STAMP(0)
  f32x16 acc[NP][2];
  float y[NP][2][16];
  int ch = 0;
  rcs_conv3x3<1, NP, NT, NW, F16>(acc, pk, ch, Q, lds_w, lds_w_addr, wave, lane);
  RC3_STAMP(1)
  const float *lds_epi = reinterpret_cast<const float *>(lds_epi_w);
  rc3_epilogue<false, NP>(x, acc, x, lds_epi, h);
  rcs_pack<NP, NT, F16>(pk, x, amax);
  RC3_STAMP(2)
  for (int b = 0; b < 4; ++b) {
    rcs_conv3x3<4, NP, NT, NW, F16>(acc, pk, ch, Q, lds_w, lds_w_addr, wave, lane);
    RC3_STAMP(3)
    rc3_epilogue<false, NP>(y, acc, x, lds_epi + (1 + 2 * b) * 192, h);
    rcs_pack<NP, NT, F16>(pk, y, amax);
    RC3_STAMP(2)
    rcs_conv3x3<4, NP, NT, NW, F16>(acc, pk, ch, Q, lds_w, lds_w_addr, wave, lane);
    RC3_STAMP(3)
    rc3_epilogue<true, NP>(x, acc, x, lds_epi + (2 + 2 * b) * 192, h);
    rcs_pack<NP, NT, F16>(pk, x, amax);
    RC3_STAMP(2)
  }
  if constexpr (F16) co_raise_unless_f16_finite(amax, Q.range_flag);
  if (NT != 2) {
    /* the head weights were requested behind the last group */
    CO_WAIT_VMCNT(0);
    co_wg_barrier();
  }
  /* heads: the two 1x1 convolutions as one more split-precision step on the operands packed
   * after the last block (no tap shift); output rows 0..3 policy planes (h 0), 4..5 value (h 1) */
  float *feat_w = lds_feat + wave * (2 * NP) * 96; /* this wave's positions, workgroup order */
  u32x4 hw[NT][4];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int t = 0; t < NT; ++t) hw[t][s] = *reinterpret_cast<const u32x4 *>(lds_head + ((s * NT + t) * 64 + lane) * 4);
#pragma unroll
  for (int np = 0; np < NP; ++np) {
    f32x16 h1;
#pragma unroll
    for (int i = 0; i < 16; ++i) h1[i] = 0.0f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      u32x4 B[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int m = 0; m < 4; ++m) B[t][m] = pk[t][np][s][m];
      }
#pragma unroll
      for (int sum = 0; sum < NT; ++sum)
#pragma unroll
        for (int i = 0; i <= sum; ++i) co_mfma_32x32x16<F16>(h1, hw[i][s], B[sum - i]);
    }
    const float4 b4 = *reinterpret_cast<const float4 *>(P.head_epi + 4 * h);
    const float4 a4 = *reinterpret_cast<const float4 *>(P.head_epi + 16 + 4 * h);
    const float4 c4 = *reinterpret_cast<const float4 *>(P.head_epi + 32 + 4 * h);
    const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
    const float aa[4] = {a4.x, a4.y, a4.z, a4.w};
    const float cc[4] = {c4.x, c4.y, c4.z, c4.w};
    const int pw = np * 2 + p2; /* position of this lane within the wave */
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = h1[r] + bb[r];
      v = aa[r] * v + cc[r];
      v = v > 0.0f ? v : 0.0f;
      if (h == 0) feat_w[pw * 96 + c * 4 + r] = v;
      if (h == 1 && r < 2) feat_w[pw * 96 + 64 + c * 2 + r] = v;
    }
  }
  RC3_STAMP(4)
  __syncthreads();
  /* 16 NP positions = NP column tiles: waves 0 (, 1) run their policy heads, waves 2 (, 3) their
   * value heads */
  const float *lds_dense = reinterpret_cast<const float *>(lds_head + RCS_FRAG1_WORDS(NT));
  constexpr int wgpos = 2 * NP * NW, ntiles = (wgpos + 15) / 16;
  constexpr int ncols = wgpos < 16 ? wgpos : 16; /* the thin kernel's workgroup is half a column tile */
  if (wave < ntiles)
    rc_dense_policy(P, lds_dense, lds_feat + wave * 16 * 96, rows, row0 + wave * 16, lane, ncols);
  else if (wave >= 2 && wave < 2 + ntiles)
    rc_dense_value(P, lds_dense + 6144, lds_dense + 6144 + 2048, lds_feat + (wave - 2) * 16 * 96, rows,
                   row0 + (wave - 2) * 16, lane, ncols);
  RC3_STAMP(5)
#ifdef CO_PROF
  if (tid == 0) {
    atomicAdd(&rc3_prof[6], __builtin_readcyclecounter() - start_);
    atomicAdd(&rc3_prof[7], 1ull);
    atomicAdd(&rc3_prof[8], __builtin_amdgcn_s_memrealtime() - real_);
  }
#endif
}

/* NT = 2  <2>: throughput kernel, batches of more than RC3_SMALL_ROWS rows, 32 positions per workgroup;
 *         <1>: small-batch kernel, up to RC3_SMALL_ROWS rows, 16 positions per workgroup, one round
 * NT = 3  <1> only */
__global__ __launch_bounds__(512, 2) void co_k_rescnn_forward_x3(Rc3Params Q) { rcs_forward<2, 2>(Q); }
__global__ __launch_bounds__(512, 2) void co_k_rescnn_forward_x3_small(Rc3Params Q) { rcs_forward<1, 2>(Q); }
/* "f16x3": the two-term kernels with fp16 terms instead of bf16 ones -- x = fp16(x) + fp16(x - fp16(x)) keeps 22
 * significand bits per operand (bf16x3: 16), the three products w0 x0 + w0 x1 + w1 x0 drop terms of 2^-22 |w x|:
 * float32-class arithmetic at the MFMA cost of bf16x3.  fp16's exponent range is narrower (normal from 6.1e-5,
 * subnormal quantum 6e-8): remainders of small values lose relative, not absolute, accuracy -- measured against
 * float64 in tests/test_net_precision.py. */
/* (the kernels themselves: behind co_k_rescnn_forward_x6) */
/* (Capping this kernel at 168 registers so that a wave of the search kernel fits beside two of its waves on a SIMD was
 * measured: the network kernel alone 5 % slower, the generation 4 % slower -- the kernel trace shows 81 % of the search
 * kernel's time overlapping the other pool's network launches already, tools/overlap.py.) */
/* Thin batches (up to RC6_THIN_ROWS rows = 256 workgroups): four waves, one per SIMD, 8 positions per workgroup.  A batch
 * that does not fill the chip is as slow as ONE workgroup's pass over the 27 weight groups; with the MFMA pipe of a SIMD
 * to itself a wave finishes its 3456 MFMAs in half the time (the DPP operand shifts fit in their shadow).  The tail of a
 * generation, the arena and the analysis mode run such batches every iteration.  Same launch, same workgroups: the row
 * count on the device picks the path, and waves 4..7 of a thin workgroup leave at once (a second kernel that merely
 * returns would still queue 256 workgroups of 151 KB LDS behind the other pool's network launch). */
__global__ __launch_bounds__(512, 2) void co_k_rescnn_forward_x6(Rc3Params Q) {
  if (*Q.base.d_rows <= RC6_THIN_ROWS) {
    if (threadIdx.x >= 256) return;
    rcs_forward<1, 3, 4>(Q);
  } else {
    rcs_forward<1, 3, 8>(Q);
  }
}

/* The f16x3 kernels (see above rcs_forward): throughput kernel, 32 positions per workgroup; _small: batches up to
 * RC3_SMALL_ROWS rows, 16 positions per workgroup, and up to RC6_THIN_ROWS rows on the four-wave thin path (one wave per
 * SIMD, 8 positions per workgroup, waves 4..7 leave at once; see co_k_rescnn_forward_x6). */
__global__ __launch_bounds__(512, 2) void co_k_rescnn_forward_h3_small(Rc3Params Q) {
  const int rows = *Q.base.d_rows, rbase = rcp_small_begin(Q, rows);
  if (rows - rbase <= 0) return; /* the whole batch is the throughput kernel's */
  if (rows - rbase <= RC6_THIN_ROWS) {
    if (threadIdx.x >= 256) return;
    rcs_forward<1, 2, 4, true>(Q, rbase);
  } else {
    rcs_forward<1, 2, 8, true>(Q, rbase);
  }
}


/* The grouped instance of the f16x3 small-batch kernel (nn.h CoNetGroup; 16 positions per workgroup at any batch size --
 * the paths are bit-identical, a throughput choice can come later): workgroup b takes entry b of the workgroup table -- a
 * model and up to 16 positions of the index list, all that model's -- and finds everything of its model in ONE buffer at a
 * fixed stride: [trunk fragments | epilogue constants | head weights | head_epi 48, bpol 96, bv1 64, bv2 1 floats]. */
#define RCG_POS_PER_WG 16
#define RCG_SMALL_WORDS 256 /* the four small float arrays, padded */
struct RcGroupParams {
  const float *in;
  const CoGroupWG *wg;
  const int32_t *n_wg, *idx;
  const uint32_t *wbase;
  uint32_t stride, off_epi, off_head, off_small; /* words */
  float *eval, *probs;
  uint32_t *range_flag;
};
__global__ __launch_bounds__(512, 2) void co_k_rescnn_forward_h3_grouped(RcGroupParams G) {
  if ((int)blockIdx.x >= *G.n_wg) return;
  const CoGroupWG e = G.wg[blockIdx.x];
  const int first = __builtin_amdgcn_readfirstlane(e.first), count = __builtin_amdgcn_readfirstlane(e.count);
  const uint32_t *w = G.wbase + (size_t)__builtin_amdgcn_readfirstlane(e.model) * G.stride;
  const float *small = reinterpret_cast<const float *>(w + G.off_small);
  Rc3Params Q;
  Q.base.in = G.in, Q.base.d_rows = nullptr;
  Q.base.wtrunk = nullptr, Q.base.epi = nullptr, Q.base.whead = nullptr, Q.base.wpol = nullptr, Q.base.wv1 = nullptr, Q.base.wv2 = nullptr;
  Q.base.head_epi = small, Q.base.bpol = small + 48, Q.base.bv1 = small + 144, Q.base.bv2 = small + 208;
  Q.base.eval = G.eval, Q.base.probs = G.probs;
  Q.base.io = CoNetIO();
  Q.base.io.in_idx = Q.base.io.out_idx = G.idx;
  Q.wtrunk = w, Q.epi3 = w + G.off_epi, Q.whead3 = w + G.off_head;
  Q.range_flag = G.range_flag, Q.pass_rows = 0;
  rcs_forward<1, 2, 8, true, true>(Q, first, first + count);
}
