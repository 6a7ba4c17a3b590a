// search_iter.h -- search layer 5: one player's share of a step.
//
// TrainMC::doIteration (trainmc.cpp:139-178) -- the root's own request (:143-167, 198-202), the evaluations received,
// then simulations, grouped (search_group.h) or one by one (search_one.h), until the step's requests are queued, the
// searches are done or the step's budget is spent.
#pragma once
#include "engine_defs.h"
#include "rules.h"
#include "wave.h"
#include "search_state.h"
#include "search_tree.h"
#include "search_eval.h"
#include "search_puct.h"
#include "search_one.h"
#include "search_group.h"

/* the root asks for its own evaluation (trainmc.cpp:143-167, 198-202) */
CO_DEV void co_request_root(CoWave &w, CoTree &t) {
  uint4 *A = t.A;
  uint32_t root = t.tc.root;
  uint4 h0 = co_load_unit(A, root);
  uint4 h1 = co_load_unit(A, CO_NODE_INFO(root));
  WAVE_SHARED(uint32_t, one_path, 1);
  uint32_t self_slot = h1.x;
  FOR_LANES {
    if (lane == 0) one_path[0] = self_slot;
  }
  WAVE_SYNC();
  uint64_t board = (uint64_t)h0.x | ((uint64_t)h0.y << 32);
  uint32_t lm[3];
  co_legal_moves1(board, h0.z, lm); /* (a root asks once per tree; its edges hold the same moves) */
  co_request(w, board, h0.z, root, (int)CO_META_NEDGES(h0.z), lm, 0, one_path);
}

/* TrainMC::doIteration, trainmc.cpp:139-178.  Returns "turn finished". */
CO_DEV int co_mc_do_iteration(CoWave &w, CoTree &t, const float *eval, const float *probs) {
  if (t.tc.root == CO_NONE) {
    int res;
    /* a search from the start position; in analysis mode TrainMC(..., board, to_play, pieces) ->
     * createRoot(Game{...}, 0) (trainmc.cpp:38-45), whose first doIteration asks for the root's evaluation */
    const uint64_t b0 = w.analyse ? ((uint64_t)w.gc.pos_lo | ((uint64_t)w.gc.pos_hi << 32)) : 0ull;
    uint32_t b = co_create_node(w, t, b0, w.analyse ? (w.gc.pos_meta & 0x7FFFFu) : CO_META_START, 0, CO_NONE, CO_NONE, &res);
    if (b == CO_NONE) return 0;
    t.tc.root = b;
    t.tc.searches_done = 1;
    co_request_root(w, t);
    return 0;
  }
  if (t.tc.searches_done == 0) { /* (only then: the root's slot is two dependent trips to memory in front of everything else) */
    const uint4 rs = co_load_unit(t.A, co_load_unit(t.A, CO_NODE_INFO(t.tc.root)).x);
    if (co_slot_visits(rs) == 1 && co_slot_all_visited(rs)) {
      t.tc.searches_done = 1;
      co_request_root(w, t);
      return 0;
    }
  }
  /* (held: the step before stopped at its budget; its leaves were not submitted -- nothing to receive, the search goes on) */
  if (w.gc.n_pending > 0 && !(w.gc.held & 1)) co_receive_eval(w, t, eval, probs);
  w.gc.held = (w.gc.held & 2) | ((w.gc.held & 1) << 1); /* bit 1: this step continues one that was cut (co_step_tail's statistics) */
  WAVE_SHARED(uint4, root_ev, CO_WAVE);
  CoRoot rc;
  rc.valid = 0;
  rc.hdr = 0;
  rc.ev = root_ev;
  rc.e0 = 0u;
  rc.ne = 0u;
  /* How many to select together follows from how the position's simulations have been ending: everything behind one that
   * is not ordinary is selected in vain (endgames of a trained network: every second simulation a terminal leaf or a
   * dead end, ten levels down).  pe = running share of such simulations in 1/256 (seven eighths of the old estimate per
   * simulation, kept with the game from step to step): above 3/8 they run one after the other, above 5/32 two at a time. */
  int pe = w.gc.sb_cap > 0 && w.gc.sb_cap <= 256 ? w.gc.sb_cap : 0;
  /* (bit 2 of gc.held: this call has run a simulation.  A step whose budget is spent before its first one -- a deadline
   * already behind the receive phase -- still makes progress: else it would stop again and again, for ever.  In the
   * game's record because one more scalar kept across the loop costs the kernel 200 spilled registers.) */
  for (;;) {
    if (!(w.gc.n_pending < w.spe && t.tc.searches_done < w.max_searches)) break;
    if (!rc.valid) co_root_load(t, rc);

    if (co_res_known(co_slot_result(rc.cs)) || co_slot_all_visited(rc.cs)) break;
    if (w.gc.error) break;
    if ((w.gc.held & 4) && CO_STEP_SPENT(w)) {
      /* more simulations are due and this step has done its share: the next launch continues here (co_step_tail holds
       * the queued leaves back).  Everything the loop carries is in the tree, in the game's record or in `pe`. */
      w.gc.held |= 1;
      break;
    }
    CO_PH_MEM(20);
    int counted = 0;
    {
      const int cap = pe > CO_SB_PE_ONE ? 1 : pe > CO_SB_PE_TWO ? 2 : CO_SB;
      int m = w.spe - w.gc.n_pending;
      if (w.max_searches - t.tc.searches_done < m) m = w.max_searches - t.tc.searches_done;
      if (m > cap) m = cap;
      if (m > 1 && (int)CO_META_NEDGES(rc.h0.z) <= CO_WAVE) {
        const int r = co_search_rows(w, t, rc, m);
        w.gc.held |= 4;
        for (int i = 0; i < (r & 0xFF); ++i) pe -= pe >> 3;
        if (r & 0x300) {
          pe += (256 - pe) >> 3;
          counted = 1;
        }
        if (!(r & 0x200)) continue;
      }
    }
    const int pending_before = w.gc.n_pending;
    CO_SBS(8, 1);
    CO_SBP(w, 6, 1);
    co_search(w, t, rc);
    w.gc.held |= 4;
    CO_PROF_ADD(w, 5, 1ull);
    if (!counted) {
      if (w.gc.n_pending > pending_before) pe -= pe >> 3; /* (it queued a leaf: ordinary) */
      else pe += (256 - pe) >> 3;
    }
  }
  w.gc.sb_cap = pe > 0 ? pe : 0;
  /* (the root's slot only when the answer depends on it: with leaves pending -- nearly every step -- it does not) */
  if (w.gc.n_pending != 0 || (w.gc.held & 1)) return 0;
  if (t.tc.searches_done == w.max_searches) return 1;
  const uint4 rs = co_load_unit(t.A, co_load_unit(t.A, CO_NODE_INFO(t.tc.root)).x);
  return co_res_known(co_slot_result(rs));
}
