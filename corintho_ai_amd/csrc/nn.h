// nn.h -- policy/value network interface of the fused mode.
//
// A net evaluates the compact, game-major batch of leaf states produced by K4
// (rows of CO_STATE_STRIDE floats, 70 used) and writes one value and 96 prior
// probabilities per row, in the order the search reads them back
// (main.pyx:70-83 get_predictions: evals[:n] = res[0].flatten(); probs[:n] = res[1]).
// The row count lives on the device (req_offset[G]); kernels are launched for
// `rows_cap` rows and workgroups beyond the count exit, so the play loop never
// waits for the host.  Results of a row depend on that row only (fixed
// reduction order, no batch-dependent tiling): SURVEY 8e invariant.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "nn_layout.h"
#include "rt.h"

#define CO_NET_NUM_MOVES 96
#define CO_NET_MLP12X100 1
#define CO_NET_RESCNN4 2
#define CO_NET_RESCNN4_X3 3 /* same network and weights, convolutions at bf16x3 split precision */
#define CO_NET_MLP12X100_X3 4 /* mlp12x100, same weights, dense layers at bf16x3 split precision */
/* float32-equivalent arithmetic on the bf16 matrix pipe: both operands as three bf16 terms (their sum is the
 * float32 value), six MFMA products -- everything down to 2^-24 of a product is kept (nn_rescnn_split.h) */
#define CO_NET_RESCNN4_X6 5
#define CO_NET_MLP12X100_X6 6
/* two fp16 terms per operand (22 significand bits), three MFMA products: float32-class arithmetic at the cost of bf16x3 */
#define CO_NET_RESCNN4_H3 8
#define CO_NET_MLP12X100_H3 9
/* (7 was round 2's Winograd experiment, git 22960a5:tools/exp/archive, removed from the tree in round 6) */
/* what a kind is: the network, the terms per operand of its matrix products (0: fp32 MFMA) and whether they are fp16 */
enum CoNetFamily { CO_FAMILY_MLP12X100, CO_FAMILY_RESCNN4 };
struct CoNetKind {
  int kind, family, terms;
  bool f16;
};
inline constexpr CoNetKind CO_NET_KINDS[] = {
    {CO_NET_MLP12X100, CO_FAMILY_MLP12X100, 0, false},    {CO_NET_RESCNN4, CO_FAMILY_RESCNN4, 0, false},
    {CO_NET_MLP12X100_X3, CO_FAMILY_MLP12X100, 2, false}, {CO_NET_RESCNN4_X3, CO_FAMILY_RESCNN4, 2, false},
    {CO_NET_MLP12X100_X6, CO_FAMILY_MLP12X100, 3, false}, {CO_NET_RESCNN4_X6, CO_FAMILY_RESCNN4, 3, false},
    {CO_NET_MLP12X100_H3, CO_FAMILY_MLP12X100, 2, true},  {CO_NET_RESCNN4_H3, CO_FAMILY_RESCNN4, 2, true},
};
inline const CoNetKind *co_net_kind(int kind) {
  for (const CoNetKind &k : CO_NET_KINDS)
    if (k.kind == kind) return &k;
  return nullptr;
}
inline int co_net_kind_of(int family, int terms, bool f16) {
  for (const CoNetKind &k : CO_NET_KINDS)
    if (k.family == family && k.terms == terms && k.f16 == f16) return k.kind;
  return 0;
}

/* mlp12x100 flat weight layout (float32), matching Keras get_weights() order of
 * wrapper.py:256-271:
 *   for l in 0..11: kernel[in_l][100], bias[100], gamma[100], beta[100], moving_mean[100], moving_var[100]
 *   value head: kernel[100][1], bias[1];  policy head: kernel[100][96], bias[96]
 * in_0 = 70, in_l = 100.  BatchNormalization epsilon = 1e-3 (Keras default). */
#define CO_MLP_LAYERS 12
#define CO_MLP_WIDTH 100
#define CO_MLP_NUM_WEIGHTS (70 * 100 + 500 + 11 * (100 * 100 + 500) + 100 + 1 + 100 * 96 + 96)
#define CO_BN_EPS 1e-3
/* rescnn4 flat weight layout (float32; specification: nets.py "rescnn4"), in order:
 *   stem: kernel[3,3,10,64] (HWIO), bias[64], gamma, beta, mean, var [64 each]
 *   blocks b = 0..3: conv1 (kernel[3,3,64,64], bias, gamma, beta, mean, var), conv2 (same)
 *   policy: kernel[64,4], bias[4], gamma, beta, mean, var [4 each], dense kernel[64,96], bias[96]
 *   value:  kernel[64,2], bias[2], gamma, beta, mean, var [2 each], dense1 kernel[32,64], bias[64],
 *           dense2 kernel[64,1], bias[1] */
#define CO_RESCNN4_NUM_WEIGHTS \
  ((9 * 10 + 5) * 64 + 8 * (9 * 64 + 5) * 64 + (64 + 5) * 4 + 64 * 96 + 96 + (64 + 5) * 2 + 32 * 64 + 64 + 64 + 1)
/* both layouts by name: nn_layout.h */
static_assert(MlpLayout().nw == CO_MLP_NUM_WEIGHTS && MlpLayout::LAYERS == CO_MLP_LAYERS && MlpLayout::W == CO_MLP_WIDTH,
              "MlpLayout is not the mlp12x100 layout above");
static_assert(ResCnnLayout().nw == CO_RESCNN4_NUM_WEIGHTS && CO_RESCNN4_NUM_WEIGHTS == 312383, "ResCnnLayout is not the rescnn4 layout above");

/* Optional indirection of a network launch (the evaluation cache of fused training): row r of the launch is read
 * from input row in_idx[r] and its outputs go to element out_idx[r] of arrays with the given strides (floats per
 * element).  All null / {1, 96}: rows in place, the reference layout. */
struct CoNetIO {
  const int32_t *in_idx = nullptr;
  const int32_t *out_idx = nullptr;
  int32_t eval_stride = 1;
  int32_t probs_stride = CO_NET_NUM_MOVES;
  /* Does this launch have the GPU to itself?  False when other streams keep it busy too (fused training in several pools:
   * the other pools' search and network kernels): a kernel family may then choose for throughput per CU rather than for
   * the latency of this launch (nn_rescnn_split.h rcp_small_begin). */
  int32_t alone = 1;
  /* First row of the launch in the buffers of a caller-supplied network (net_host.h ExternalNet): each pool of a fused run
   * works in its own slice of them.  Every other network ignores it. */
  int32_t row_base = 0;
};

struct CoNet {
  virtual ~CoNet() {}
  virtual size_t max_rows() const = 0;
  virtual int kind() const = 0;
  /* d_rows: device int32 holding the number of valid rows (<= rows_cap) */
  virtual void forward(const float *d_in, int32_t rows_cap, const int32_t *d_rows, float *d_eval, float *d_probs,
                       rt_stream_t s, const CoNetIO &io = CoNetIO()) = 0;
  /* algorithmic flop per row, for the roofline */
  virtual double flop_per_row() const = 0;
  /* The f16x3 kinds hold every operand as two fp16 terms: a folded weight or an activation beyond fp16's largest
   * finite value (CO_F16_MAX) would convert to infinity and the evaluation to NaN without a word.  Weights are checked
   * when the net is created (std::invalid_argument); the kernels track the largest activation they split and raise a
   * flag on the device, which this call reads (a 4-byte copy and a wait on `s`): true = some evaluation since the
   * net was created left the range, its outputs are not to be trusted -- the engine turns that into an error and names
   * the float32-equivalent x6 kind.  Kinds with float32's exponent range never report. */
  virtual bool range_exceeded(rt_stream_t) { return false; }
  /* A caller-supplied network (net_host.h ExternalNet) whose function returned non-zero: its forward() queues nothing any
   * more, and whoever drives a run looks here after queueing and leaves.  clear_failure(): a new generation. */
  virtual bool callback_failed() const { return false; }
  virtual void clear_failure() {}
};
#define CO_F16_MAX 65504.0f

CoNet *co_net_create(int kind, const float *weights, size_t n_floats, size_t max_rows, rt_stream_t s);

/* ---- Rows of MANY models of one kind in one launch (a rating round's 95 checkpoints).  A row's result depends on that
 * row only, so rows of different models may share a launch if every workgroup takes the weights of its own model.  The
 * grouping kernel (nn_group.h co_k_group) turns "row r belongs to model m" into the three tables below, on the device:
 *   idx   the batch's rows ordered by model, then by row; model m's segment starts at seg_start[m] -- packed (a grouped
 *         kernel) or at m * seg_stride (the per-model fallback, whose launches need a start the host knows);
 *   wg    one entry per workgroup: model, first position in idx, rows (<= the group's tile).  Segments never share a workgroup;
 *   n_wg  entries of wg; at most rows_cap / tile + models.
 * Placement is a counting sort in (model, row) order: no atomics, the tables are the same bits from run to run. */
#define CO_GROUP_MAX_MODELS 256
#define CO_GROUP_MAX_ROWS 65535 /* the grouping kernel counts in 16-bit LDS words */
#define CO_GROUP_TILE 128       /* rows per workgroup of the tables unless the group says otherwise (the split MLP kernel's) */
struct CoGroupWG {
  int32_t model, first, count, pad;
};
struct CoGroupPlan {
  const int32_t *idx = nullptr;
  const CoGroupWG *wg = nullptr;
  const int32_t *n_wg = nullptr;
  const int32_t *seg_start = nullptr; /* [models] */
  const int32_t *seg_count = nullptr; /* [models] */
  int32_t wg_cap = 0;                 /* entries wg has room for: the grid of a grouped launch */
  int32_t seg_stride = 0;             /* 0: segments packed */
};
struct CoNetGroup {
  virtual ~CoNetGroup() {}
  virtual int kind() const = 0;
  virtual int models() const = 0;
  virtual size_t max_rows() const = 0;
  /* one kernel for every model (true), or one CoNet::forward per model segment (false): which layout of idx it reads */
  virtual bool grouped_kernel() const = 0;
  /* rows per workgroup the tables are cut for: the grouped kernel's */
  virtual int tile() const { return CO_GROUP_TILE; }
  /* the rows of d_in named by plan.idx, each through its model; results at the same row of d_eval / d_probs */
  virtual void forward(const float *d_in, int32_t rows_cap, const CoGroupPlan &plan, float *d_eval, float *d_probs, rt_stream_t s) = 0;
  /* CoNet::range_exceeded for the launch's models together (the flag is shared) */
  virtual bool range_exceeded(rt_stream_t) { return false; }
};
/* the grouped kernels of `kind`, or null if it has none (the caller then uses the fallback of nn_group.h); throws
 * std::invalid_argument like co_net_create, naming the model.  Not in the emulation build. */
CoNetGroup *co_net_group_native(int kind, const float *const *weights, int models, size_t n_floats, size_t max_rows, rt_stream_t s);
