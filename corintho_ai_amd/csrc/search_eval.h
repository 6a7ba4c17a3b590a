// search_eval.h -- search layer 2: what an evaluation does to the tree.
//
// receiveEval (trainmc.cpp:269-296) in its two parts -- the leaves' priors with their Dirichlet noise (getFilteredProbs
// :212-234, generateDirichlet :236-246, setProbs :248-267), four leaves per pass, and the backups in request order
// (:280-295) -- the capture of the generator outputs a queued leaf is owed, and propagateTerminal (trainmc.cpp:497-538).
#pragma once
#include "engine_defs.h"
#include "rng.h"
#include "rules.h"
#include "wave.h"
#include "search_state.h"
#include "search_tree.h"

/* ---- receiveEval (trainmc.cpp:269-296), split in two.
 *
 * What a leaf's evaluation does to the tree has two parts.  (1) The leaf's own priors:
 * getFilteredProbs (trainmc.cpp:212-234), generateDirichlet (:236-246), setProbs (:248-267) -- a
 * function of the network's row for that leaf, of the leaf's legal moves and of the generator
 * outputs owed to it, and of nothing else.  (2) The backup of the value along the path to the root
 * (:280-295), which touches slots shared with other leaves and must run in request order.
 * Round 1 ran both inside the game's wavefront, leaf after leaf: 37 % of the search kernel's wave
 * cycles, serial per game, with ~28 of 64 lanes busy.  Part (1) is independent per LEAF: rounds 2-4 ran
 * it as a kernel of its own in front of the search launch (one wavefront per pending leaf); since round 5
 * it is back inside the step, FOUR LEAVES AT A TIME, one per 16-lane row of the game's wavefront
 * (co_prior_all / co_prior_rows below, called from co_receive_eval in front of part (2)) -- no launch of
 * its own, and no second kernel that has to agree with this one on which games step.
 *
 * The generator: a game's two searchers share one std::mt19937 (selfplayer.cpp:23-28) and the
 * reference draws a leaf's noise when the leaf's evaluation is received.  Between queueing a leaf
 * and receiving its evaluation the game draws nothing else (a move is only chosen with no request
 * pending, trainmc.cpp:139-178), so the outputs a leaf will consume are fixed when it is queued:
 * co_capture_noise copies them (raw state words, tempered by the consumer) into the game's noise
 * buffer at the end of the step and advances the generator -- the stream is consumed in the
 * reference's order, leaf by leaf in request order. */

/* the generator outputs owed to the leaves queued in this step -> noise_raw[0 .. noise_words) */
CO_DEV void co_capture_noise(CoWave &w) {
  int done = 0;
  const int total = w.noise_words;
  int staged = w.mt_staged; /* the state is in w.mt_stage: fetched when the step began (co_mcts_step_wave), in front of
                             * the step's stores -- a fetch here would stand behind all of them -- or by a twist below */
  while (done < total) {
    if (w.gc.rng_idx >= CO_MT_N) {
      if (!staged) co_mt_stage_load(w.mt, w.mt_stage);
      CO_PH(30);
      co_mt_twist_staged(w.mt, w.mt_stage);
      CO_PH(31);
      w.gc.rng_idx = 0;
      staged = 1;
    }
    int cnt = total - done;
    if (cnt > CO_MT_N - w.gc.rng_idx) cnt = CO_MT_N - w.gc.rng_idx;
    uint32_t *dst = w.noise_raw + done;
    if (staged) {
      /* (LDS reads first, then the stores in one run: see co_mt_twist_staged) */
      const uint32_t *src = w.mt_stage + w.gc.rng_idx;
      for (int base = 0; base < cnt; base += 5 * CO_WAVE) {
        LV(uint32_t, v[5]);
        FOR_LANES {
#pragma unroll
          for (int j = 0; j < 5; ++j) {
            const int i = base + j * CO_WAVE + lane;
            L(v[j]) = src[i < cnt ? i : 0];
          }
        }
        FOR_LANES {
#pragma unroll
          for (int j = 0; j < 5; ++j) {
            const int i = base + j * CO_WAVE + lane;
            if (i < cnt) dst[i] = L(v[j]);
          }
        }
      }
    } else {
      const uint32_t *src = w.mt + w.gc.rng_idx;
      /* four chunks of 64 words at a time, loads first: their latencies overlap (a step owes ~450 words) */
      for (int base = 0; base < cnt; base += 4 * CO_WAVE) {
        LV(uint32_t, v[4]);
        FOR_LANES {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int i = base + j * CO_WAVE + lane;
            L(v[j]) = src[i < cnt ? i : 0];
          }
        }
        FOR_LANES {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int i = base + j * CO_WAVE + lane;
            if (i < cnt) dst[i] = L(v[j]);
          }
        }
      }
    }
    WAVE_SYNC();
    w.gc.rng_idx += cnt;
    done += cnt;
  }
  w.mt_staged = staged;
}

/* one output for the game's own draws (opening moves, trainmc.cpp:407; a random player, match.cpp:199-200), through
 * memory; a twist there leaves the staging copy behind */
CO_DEV uint32_t co_wave_mt_next(CoWave &w) {
  if (w.gc.rng_idx >= CO_MT_N) w.mt_staged = 0;
  return co_mt_next(w.mt, &w.gc.rng_idx);
}

/* Part (1) for FOUR leaves at a time, one per row of the wavefront (round 5): the same arithmetic as co_prior_leaf --
 * which the separate priors kernel of rounds 2-4 ran, one wavefront per leaf, as a launch of its own in front of every
 * search launch: 19-50 us on each pool's chain, most of it waiting for CUs beside the network kernels.  In row form it is
 * ~550 instructions per four leaves inside the game's own step.
 *   A lane looks at move ids column + 16 q (q < 6): legal?  its rank among the legal moves = its edge; the network's prior
 *   of the move (coalesced: 16 consecutive floats of the row), the generator output of the edge -> its gamma sample
 *   (table in LDS).  Illegal moves carry +0.0: the two SEQUENTIAL float sums of the reference's loops over edges
 *   (trainmc.cpp:219-229, 238-241) then run over all 96 move ids in order -- x + 0.0 == x -- as 96 v_add_f32 with a
 *   row_newbcast source each (ROW_SEQ_SUM16), the two chains interleaved.  Weights, row maximum, 9-bit quantisation, the
 *   integer sum and the denominator as in co_prior_leaf. */
#define CO_SB_ROWS 4 /* rows of a wavefront */
/* (-DCO_PROF_PRIORS: the pass split over six stamp slots that are empty otherwise, every stamp behind a full wait) */
#if defined(CO_PROF_PRIORS) && defined(CO_PROF) && !defined(CO_EMU)
#define CO_PPH(slot)                                            \
  do {                                                          \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); \
    CO_PH(slot);                                                \
  } while (0)
#else
#define CO_PPH(slot) ((void)0)
#endif
#define CO_PRE 16
#define CO_PRE_LEAF 0
#define CO_PRE_NOFF 1
#define CO_PRE_L0 2
#define CO_PRE_L1 3
#define CO_PRE_L2 4
#define CO_PRE_ROFF 5 /* where the leaf's row of priors starts, in floats from cval / from the step's probs */
#define CO_PRE_DEPTH 6
#define CO_PRE_WORDS (7 * CO_PRE)
/* the records of pending leaves c0 .. c0 + nc - 1 (nc <= CO_PRE) -> w.pre */
CO_DEV void co_pending_records(CoWave &w, int c0, int nc) {
  const uint32_t *pend_leaf = w.pend_leaf;
  const uint4 *pend_n = (const uint4 *)w.pend_n;
  const int32_t *pend_depth = w.pend_depth;
  const int has_cval = w.cval != 0;
  const int32_t *csrc = w.csrc;
  uint32_t *pre = w.pre;
  FOR_LANES_HOT {
    if (lane < nc) {
      const int k = c0 + lane;
      const uint32_t lf = pend_leaf[k];
      const uint4 pn = pend_n[k];
      const int dp = pend_depth[k];
      const uint32_t ro = has_cval ? (uint32_t)csrc[k] * (uint32_t)CO_CACHE_VAL_FLOATS + 4u : (uint32_t)k * (uint32_t)CO_NUM_MOVES;
      pre[CO_PRE_LEAF * CO_PRE + lane] = lf;
      pre[CO_PRE_NOFF * CO_PRE + lane] = pn.x >> 8;
      pre[CO_PRE_L0 * CO_PRE + lane] = pn.y;
      pre[CO_PRE_L1 * CO_PRE + lane] = pn.z;
      pre[CO_PRE_L2 * CO_PRE + lane] = pn.w;
      pre[CO_PRE_ROFF * CO_PRE + lane] = ro;
      pre[CO_PRE_DEPTH * CO_PRE + lane] = (uint32_t)dp;
    }
  }
  WAVE_SYNC();
  w.pre_c0 = c0;
  w.pre_n = nc;
}

/* is move id column + 16 q legal in the leaf whose 96-bit mask is (l0, l1, l2), and which edge is it */
CO_DEV int co_prior_legal(uint32_t l0, uint32_t l1, uint32_t l2, int q, int c) {
  const uint32_t wd = q < 2 ? l0 : q < 4 ? l1 : l2;
  return (int)((wd >> ((16 * q + c) & 31)) & 1u);
}
CO_DEV int co_prior_rank(uint32_t l0, uint32_t l1, uint32_t l2, int q, int c) {
  const uint32_t wd = q < 2 ? l0 : q < 4 ? l1 : l2;
  const int bit = (16 * q + c) & 31;
  const int before = q < 2 ? 0 : q < 4 ? co_popc32(l0) : co_popc32(l0) + co_popc32(l1);
  return before + co_popc32(wd & ((1u << bit) - 1u));
}
/* The passes of a step, four leaves each.  Round 5 stamps (tools/prof_phases.py -DCO_PROF_PRIORS) put a pass at ~9 k
 * cycles: two trips to memory one behind the other (the leaf's record, then the row of priors and the generator words it
 * points to), the sequential sums, and the stores of the quantised priors -- behind which the NEXT pass's loads waited, the
 * counter of outstanding memory operations being retired in order.  So:
 *   - the records of ALL pending leaves are fetched once, lane k = leaf k, and a pass takes its four by a shuffle;
 *   - the loads of pass p + 1 are issued BEFORE the stores of pass p (two register sets, X and Y). */
#define CO_PRIOR_FETCH(K0, on_, leaf_, l0_, l1_, l2_, pq_, rw_)                                                          \
  {                                                                                                                      \
    LV(uint32_t, noff_);                                                                                                 \
    LV(uint32_t, roff_);                                                                                                 \
    FOR_LANES_HOT {                                                                                                      \
      int i = (K0)-c0 + (lane >> 4);                                                                                     \
      i = i < nc ? i : 0;                                                                                                \
      L(leaf_) = pre[CO_PRE_LEAF * CO_PRE + i];                                                                          \
      L(noff_) = pre[CO_PRE_NOFF * CO_PRE + i];                                                                          \
      L(roff_) = pre[CO_PRE_ROFF * CO_PRE + i];                                                                          \
      L(l0_) = pre[CO_PRE_L0 * CO_PRE + i];                                                                              \
      L(l1_) = pre[CO_PRE_L1 * CO_PRE + i];                                                                              \
      L(l2_) = pre[CO_PRE_L2 * CO_PRE + i];                                                                              \
    }                                                                                                                    \
    FOR_LANES_HOT {                                                                                                      \
      const int c = lane & 15;                                                                                           \
      const int has = (K0) + (lane >> 4) < n;                                                                            \
      L(on_) = has;                                                                                                      \
      L(l0_) = has ? L(l0_) : 0u;                                                                                        \
      L(l1_) = has ? L(l1_) : 0u;                                                                                        \
      L(l2_) = has ? L(l2_) : 0u;                                                                                        \
      const float *row = rbase + L(roff_);                                                                               \
      const uint32_t *raw = noise_raw + L(noff_);                                                                        \
      _Pragma("unroll") for (int q = 0; q < 6; ++q) {                                                                    \
        const int legal = co_prior_legal(L(l0_), L(l1_), L(l2_), q, c);                                                  \
        L(pq_[q]) = row[16 * q + c]; /* (all loads first: their latencies overlap) */                                    \
        L(rw_[q]) = raw[legal ? co_prior_rank(L(l0_), L(l1_), L(l2_), q, c) : 0];                                        \
      }                                                                                                                  \
    }                                                                                                                    \
  }
CO_DEV void co_prior_all(CoWave &w, CoTree &t, int c0, int nc, const float *probs) {
  uint4 *A = t.A;
  const uint32_t *noise_raw = w.noise_raw;
  const uint32_t *gam = w.gamma;
  const float *rbase = w.cval ? w.cval : probs;
  const float eps = w.epsilon;
  const int n = c0 + nc;
  const uint32_t *pre = w.pre;
  { /* leaves c0 .. c0 + nc - 1, whose records are in w.pre */
    CO_PPH(19);
    LV(int, on);
    LV(uint32_t, leaf);
    LV(uint32_t, l0); /* the leaf's legal moves; all zero in a row without a leaf */
    LV(uint32_t, l1);
    LV(uint32_t, l2);
    LV(float, pq[6]);
    LV(uint32_t, rw[6]);
    CO_PRIOR_FETCH(c0, on, leaf, l0, l1, l2, pq, rw)
    for (int k0 = c0; k0 < c0 + nc; k0 += CO_SB_ROWS) {
      const int more = k0 + CO_SB_ROWS < c0 + nc;
      CO_SBS(28 + (more ? CO_SB_ROWS : c0 + nc - k0) - 1, 1);
      CO_PPH(16);
      LV(float, gq[6]);
      FOR_LANES_HOT {
        const int c = lane & 15;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
          const int legal = co_prior_legal(L(l0), L(l1), L(l2), q, c);
          const float g = co_u2f(gam[co_mt_temper(L(rw[q])) % CO_NUM_GAMMA]);
          L(gq[q]) = legal ? g : 0.0f;
          L(pq[q]) = legal ? L(pq[q]) : 0.0f;
        }
      }
      /* a block of sixteen move ids none of the four leaves has a legal move in (the stack moves of an early position:
       * three of the six blocks) adds sixteen zeros: skipped */
      int live[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        LV(int, lq);
        FOR_LANES_HOT {
          const uint32_t m = q < 2 ? L(l0) : q < 4 ? L(l1) : L(l2);
          L(lq) = ((q & 1) ? m >> 16 : m & 0xFFFFu) != 0u;
        }
        live[q] = WAVE_BALLOT(lq) != 0ull;
      }
      CO_PPH(10);
      LV(float, sum);
      LV(float, dsum);
      FOR_LANES_HOT { L(sum) = L(dsum) = 0.0f; }
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        if (!live[q]) continue;
        ROW_SEQ_SUM16_2(sum, pq[q], dsum, gq[q]);
      }
      CO_PPH(25);
      LV(float, mxl);
      FOR_LANES_HOT {
        const int c = lane & 15;
        const float one_minus = (float)1 - eps;
        const float scalar = (float)(1.0 / (double)L(sum) * (double)one_minus);
        const float dscalar = (float)(1.0 / (double)L(dsum) * (double)eps);
        float mx = 0.0f; /* weights are >= 0, as the reference's max_prob start value */
#pragma unroll
        for (int q = 0; q < 6; ++q) {
          const float a = L(pq[q]) * scalar;
          const float d = L(gq[q]) * dscalar;
          const float x = a + d;
          L(pq[q]) = x; /* the move's weight from here on */
          if (co_prior_legal(L(l0), L(l1), L(l2), q, c)) mx = x > mx ? x : mx;
        }
        L(mxl) = mx;
      }
      LV(float, mxr);
      ROW_MAX_F32(mxr, mxl);
      CO_PPH(29);
      /* the next pass's loads, in front of this pass's stores */
      LV(int, on_y);
      LV(uint32_t, leaf_y);
      LV(uint32_t, l0_y);
      LV(uint32_t, l1_y);
      LV(uint32_t, l2_y);
      LV(float, pq_y[6]);
      if (more) CO_PRIOR_FETCH(k0 + CO_SB_ROWS, on_y, leaf_y, l0_y, l1_y, l2_y, pq_y, rw)
      LV(int, qs);
      FOR_LANES_HOT {
        const int c = lane & 15;
        const float denom = 511.0f / L(mxr);
        int sm = 0;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
          if (co_prior_legal(L(l0), L(l1), L(l2), q, c)) {
            const float x = L(pq[q]) * denom;
            /* lround: half away from zero (x >= 0 here; NaN/neg handled like max(1, .)) */
            const float fl = __builtin_truncf(x);
            int qq = (int)fl;
            if (x - fl >= 0.5f) qq += 1;
            if (!(qq >= 1)) qq = 1;
            sm += qq;
            const uint32_t edge = (uint32_t)co_prior_rank(L(l0), L(l1), L(l2), q, c);
            A[CO_NODE_EDGE(L(leaf), edge)].z = CO_SLOT_MP_MAKE(16 * q + c, qq);
          }
        }
        L(qs) = sm;
      }
      LV(int, fs);
      ROW_SUM_I32(fs, qs);
      FOR_LANES_HOT {
        if (L(on) && (lane & 15) == 0) {
          const float denominator = (float)(1.0 / (double)(float)L(fs));
          A[CO_NODE_INFO(L(leaf))].y = co_f2u(denominator);
        }
      }
      if (more) {
        FOR_LANES_HOT {
          L(on) = L(on_y);
          L(leaf) = L(leaf_y);
          L(l0) = L(l0_y);
          L(l1) = L(l1_y);
          L(l2) = L(l2_y);
#pragma unroll
          for (int q = 0; q < 6; ++q) L(pq[q]) = L(pq_y[q]);
        }
      }
      CO_PPH(18);
    }
  }
}

/* Part (2): the backups of up to CO_RB pending leaves at once.  The node k levels above a leaf
 * receives eval*(-1)^k - 1; every node on the path becomes searchable again (all_visited := false).
 * The slot of a shared ancestor must receive the leaves' contributions in request order (float
 * addition is not associative): the slots of all paths are fetched together, and leaf k starts from
 * the value left by the latest earlier leaf of the batch that touched the same slot (register
 * forwarding) instead of re-reading memory. */
#define CO_RB 8
/* the paths of leaves k0 .. k0 + nb - 1 -> at[k][lane = level] (all CO_PATH_MAX entries whatever the leaf's depth: the
 * loads do not wait for the depths) */
CO_DEV void co_backup_paths(CoWave &w, int k0, int nb, LVPA(uint32_t, at, CO_RB)) {
#pragma unroll
  for (int k = 0; k < CO_RB; ++k) {
    const uint32_t *pp = w.pend_path + (size_t)(k < nb ? k0 + k : k0) * CO_PATH_MAX;
    FOR_LANES { L(at[k]) = pp[lane < CO_PATH_MAX ? lane : 0]; }
  }
}
/* evl: the evaluation (bits) of leaf c0 + k in lane k, its depth in w.pre */
CO_DEV void co_backup_batch(CoWave &w, CoTree &t, int c0, int k0, int nb, LVP(uint32_t, evl), LVPA(uint32_t, at, CO_RB)) {
  uint4 *A = t.A;
  LV(uint32_t, ny[CO_RB]);
  LV(uint32_t, nw[CO_RB]);
  LV(uint32_t, nx[CO_RB]); /* (the slot's other two words, so that a slot goes back as ONE 16-byte store) */
  LV(uint32_t, nz[CO_RB]);
  LV(int, on[CO_RB]);
#pragma unroll
  for (int k = 0; k < CO_RB; ++k) {
    const int D = (int)w.pre[CO_PRE_DEPTH * CO_PRE + (k < nb ? k0 - c0 + k : k0 - c0)];
    FOR_LANES { L(on[k]) = (k < nb && lane <= D); }
  }
  CO_PH_MEM(0);
#pragma unroll
  for (int k = 0; k < CO_RB; ++k) {
    FOR_LANES {
      if (!L(on[k])) L(at[k]) = 0u;
      uint4 sl = A[L(at[k])]; /* unconditional: inactive lanes read unit 0 */
      L(nx[k]) = sl.x;
      L(ny[k]) = sl.y;
      L(nz[k]) = sl.z;
      L(nw[k]) = sl.w & ~CO_SLOT_ALL_VISITED; /* all_visited := false */
    }
  }
  CO_PH_MEM(1);
#pragma unroll
  for (int k = 0; k < CO_RB; ++k) {
    const int D = (int)w.pre[CO_PRE_DEPTH * CO_PRE + (k < nb ? k0 - c0 + k : k0 - c0)];
    const float leaf_eval = k < nb ? co_u2f(WAVE_BCAST(evl, k0 - c0 + k)) : 0.0f;
    FOR_LANES {
      if (L(on[k])) {
        uint32_t cur = L(ny[k]);
#pragma unroll
        for (int j = 0; j < k; ++j)
          if (L(on[j]) && L(at[j]) == L(at[k])) cur = L(ny[j]);
        int kk = D - lane;
        float ce = (kk & 1) ? (float)((double)leaf_eval * -1.0) : leaf_eval;
        float add = (float)((double)ce - 1.0);
        L(ny[k]) = co_f2u(co_u2f(cur) + add);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < CO_RB; ++k) {
    FOR_LANES {
      if (L(on[k])) A[L(at[k])] = make_uint4(L(nx[k]), L(ny[k]), L(nz[k]), L(nw[k]));
    }
  }
  WAVE_SYNC();
  CO_PH(3);
  w.gc.evals += (uint32_t)nb;
}

/* trainmc.cpp:269-296: the priors of the pending leaves (co_prior_all, four leaves per pass), then the backups in
 * request order */
CO_DEV void co_receive_eval(CoWave &w, CoTree &t, const float *eval, const float *probs) {
  const int n = w.gc.n_pending;
  for (int c0 = 0; c0 < n; c0 += CO_PRE) { /* (one round: searches_per_eval is 16, or 1) */
    const int nc = n - c0 < CO_PRE ? n - c0 : CO_PRE;
    /* what the backups need of the leaves' records, requested beside the priors' own first loads: depth and evaluation
     * of leaf c0 + k in lane k (one trip for the step instead of two dependent scalar loads per leaf behind the priors'
     * stores) */
    if (c0 > 0 || w.pre_n != nc) co_pending_records(w, c0, nc); /* (else: requested when the step began) */
    CO_SBS(25, c0 > 0);
    w.pre_n = 0;
    LV(uint32_t, evl);
    {
      const float *cval = w.cval;
      const uint32_t *pre = w.pre;
      FOR_LANES_HOT {
        const int i = lane < nc ? lane : 0;
        L(evl) = co_f2u(cval ? cval[pre[CO_PRE_ROFF * CO_PRE + i] - 4u] : eval[c0 + i]);
      }
    }
    LV(uint32_t, pa[CO_RB]);
    co_prior_all(w, t, c0, nc, probs);
    WAVE_SYNC();
    CO_PH_MEM(13);
    for (int k0 = c0; k0 < c0 + nc; k0 += CO_RB) {
      const int nb = c0 + nc - k0 < CO_RB ? c0 + nc - k0 : CO_RB;
      CO_SBS(26, 1);
      CO_SBS(27, k0 > c0);
      /* (requested in front of the priors' passes instead -- 8 or 16 registers across them: +-0 with the first batch's,
       * 4 % slower with both, the product build's allocation gives way; round 5) */
      co_backup_paths(w, k0, nb, pa);
      co_backup_batch(w, t, c0, k0, nb, evl, pa);
    }
  }
  CO_PROF_ADD(w, 6, (unsigned long long)n);
  w.gc.n_pending = 0;
  w.noise_words = 0;
}

/* propagateTerminal, trainmc.cpp:497-538 (including the parent-for-child draw
 * test at :518).  path_* describe root..leaf, D = index of the terminal leaf. */
CO_DEV void co_propagate_terminal(CoTree &t, const uint32_t *path_block, const uint32_t *path_slot, int D) {
  uint4 *A = t.A;
  int d = D;
  while (d > 0) {
    int rc = co_slot_result(co_load_unit(A, path_slot[d]));
    if (co_res_lost(rc)) {
      --d;
      uint4 s = co_load_unit(A, path_slot[d]);
      co_store_unit(A, path_slot[d], co_slot_set_result(s, CO_DEDUCED_WIN));
    } else {
      --d;
      uint32_t pb = path_block[d];
      int n = (int)CO_META_NEDGES(co_load_unit(A, pb).z);
      int all_known = 1;
      for (int base = 0; base < n; base += CO_WAVE) {
        LV(int, bad);
        FOR_LANES {
          int e = base + lane;
          L(bad) = 0;
          if (e < n) {
            uint4 s = A[CO_NODE_EDGE(pb, e)];
            L(bad) = (s.x == CO_NONE) || !co_res_known(co_slot_result(s));
          }
        }
        if (WAVE_BALLOT(bad)) all_known = 0;
      }
      if (!all_known) return;
      uint4 s = co_load_unit(A, path_slot[d]);
      int has_draw = co_res_drawn(co_slot_result(s)); /* the PARENT's own result, as trainmc.cpp:518 */
      co_store_unit(A, path_slot[d], co_slot_set_result(s, has_draw ? CO_DEDUCED_DRAW : CO_DEDUCED_LOSS));
    }
  }
}
