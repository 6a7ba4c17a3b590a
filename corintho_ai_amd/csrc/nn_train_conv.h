// nn_train_conv.h -- launchers of the convolutional training kernels (nn_train_conv.hip) that ca_fitter's rescnn4 path
// (nn_train.hip) is built from.  Activations are NHWC float32 [B * 16][C], row = position * 16 + pixel.
#pragma once
#include <stdint.h>

#include "rt.h"

#define FC_C 64           /* trunk channels */
#define FC_IN_LD 16       /* input planes: 10 channels padded with zeros to one k tile row of 16 */
#define FC_BN_CHUNKS 256  /* at most this many row chunks in a BatchNorm reduction */
#define FC_WG_CHUNKS 128  /* at most this many row chunks in a 3x3 weight gradient */
#define FC_WG_FLOATS (9 * FC_C * FC_C)
#define FC_BN_PART (FC_BN_CHUNKS * 3 * 64)         /* BatchNorm chunk partials: float32 forward, float64 backward */
#define FC_BN_SCRATCH (2 * (FC_BN_PART + 2 * 64)) /* floats of those and of the two per-channel constants behind them */

/* x0[B * 16][16] = rescnn4's input planes of states[rows[r]] (nets.rescnn4_input_planes), channels 10..15 zero */
void fc_planes(rt_stream_t s, const float *states, const int32_t *rows, int B, float *x0);
/* wt[l][tap][co][ci] = w[first + l * stride][8 - tap][ci][co] for the n 64 -> 64 kernels: the operand of backward-data */
void fc_wtrans(rt_stream_t s, const float *w, int first, int stride, int n, float *wt);
/* out[row][co] (+)= bias[co] + sum over taps and ci of X[row shifted by the tap][ci] W[tap][ci][co]; cin = 10 reads X
 * with row stride FC_IN_LD, cin = 64 with FC_C.  bias may be null. */
void fc_conv3(rt_stream_t s, const float *X, int cin, const float *W, const float *bias, float *out, int B, int accumulate);
/* dW[tap][ci][co] = sum over rows of X[row shifted by the tap][ci] dZ[row][co]: per-chunk partials into part
 * ([FC_WG_CHUNKS][9 * cin * 64]), then their sum in chunk order into dW */
void fc_conv3_wgrad(rt_stream_t s, const float *X, int cin, const float *dZ, int B, float *part, float *dW);
/* BatchNorm over the R rows of Z[R][C] (C in {64, 4, 2}), then + res (or null), then ReLU -> out.  bn = gamma, beta,
 * moving mean, moving variance, C floats each.  train: batch statistics, two stage (per-chunk mean and centred sum of
 * squares in part (FC_BN_SCRATCH floats), combined in chunk order), left in stat[0..C) and stat[64..64 + C); else the
 * moving ones. */
void fc_bn_fwd(rt_stream_t s, const float *Z, const float *res, float *out, int R, int C, const float *bn, int train,
               float *part, float *stat);
/* backward of the same: dOut is the gradient at `out`; dY = dOut where out > 0 (written back to dOut when keep: the
 * residual branch's share); dZ, and dbias (identically 0), dgamma, dbeta to g[0..3C) */
void fc_bn_bwd(rt_stream_t s, float *dOut, const float *out, const float *Z, float *dZ, int R, int C, const float *bn,
               const float *stat, int keep, float *part, float *g);
