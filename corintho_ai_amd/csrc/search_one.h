// search_one.h -- search layer 4a: one simulation, the reference's way.
//
// TrainMC::search (trainmc.cpp:602-696) with chooseNext (:540-600) inlined as a lane-parallel edge scan.  Every
// simulation the grouped search (search_group.h) does not handle -- a dead end, a terminal child or leaf, a wide node,
// a deep path, a full arena -- ends here.
#pragma once
#include "engine_defs.h"
#include "rules.h"
#include "wave.h"
#include "search_state.h"
#include "search_tree.h"
#include "search_eval.h"
#include "search_puct.h"

/* One simulation: TrainMC::search (trainmc.cpp:602-696) with chooseNext
 * (:540-600) inlined as the lane-parallel edge scan.  A node's header and its
 * first 64 edge slots are requested together (one memory round trip per level). */
CO_COLD2 void co_search(CoWave &w, CoTree &t, CoRoot &rc) {
  uint4 *A = t.A;
  WAVE_SHARED(uint32_t, path_block, CO_PATH_MAX);
  WAVE_SHARED(uint32_t, path_slot, CO_PATH_MAX);
  uint32_t cur = t.tc.root;
  ++t.tc.searches_done;
  w.gc.searches++;
  uint4 h0 = rc.h0;
  uint4 h1 = rc.h1;
  uint32_t cur_slot = h1.x;
  uint4 cs = rc.cs;
  LV(uint4, ev);
  FOR_LANES { L(ev) = rc.ev[lane]; }
  int D = 0;
  int leaf_n = 0; /* legal moves of the node this simulation creates */
  uint32_t leaf_lm[3] = {0u, 0u, 0u};
  FOR_LANES {
    if (lane == 0) {
      path_block[0] = cur;
      path_slot[0] = cur_slot;
    }
  }
  WAVE_SYNC();
  CO_PH_MEM(19);
  float v_sqrt_next = co_vsqrt(w.c_puct, co_slot_visits(cs));
  while (!co_res_terminal(co_slot_result(cs))) {
    int n = (int)CO_META_NEDGES(h0.z);
    float denom = co_u2f(h1.y);
    int visits = co_slot_visits(cs);
    const float v_sqrt = v_sqrt_next;
    /* ---- chooseNext: u for every edge, strict first maximum */
    float best_u = CO_NEG_INF;
    int best_e = -1;
    uint4 best_slot = make_uint4(0, 0, 0, 0);
    for (int base = 0; base < n; base += CO_WAVE) {
      LV(float, u);
      FOR_LANES {
        int e = base + lane;
        float uu = CO_NEG_INF;
        if (base > 0 && e < n) L(ev) = A[CO_NODE_EDGE(cur, e)];
        uu = co_puct_u(L(ev), denom, v_sqrt);
        uu = e < n ? uu : CO_NEG_INF;
        L(u) = uu;
      }
      float mx = WAVE_MAX_F32(u);
      if (mx > best_u) {
        LV(int, hit);
        FOR_LANES { L(hit) = (L(u) == mx); }
        int le = co_ffs64(WAVE_BALLOT(hit)) - 1;
        best_u = mx;
        best_e = base + le;
        best_slot = WAVE_BCAST(ev, le);
      }
    }
    CO_PH(8);
    CO_PROF_ADD(w, 23, 1ull);
    CO_STEP_WORK(w, 1);
    /* ---- visit the current node (virtual loss on every node of the path) */
    cs = co_slot_set_visits(cs, visits + 1);
    cs.y = co_f2u(co_u2f(cs.y) + 1.0f);
    if (best_e < 0) {
      /* kNone: nothing searchable below; mark, undo the path, un-count the search */
      cs = co_slot_set_all_visited(cs, 1);
      co_store_slot(A, cur_slot, cs, rc);
      FOR_LANES {
        if (lane <= D) {
          uint4 s = A[path_slot[lane]];
          s = co_slot_set_visits(s, co_slot_visits(s) - 1);
          s.y = co_f2u(co_u2f(s.y) - 1.0f);
          A[path_slot[lane]] = s;
        }
      }
      WAVE_SYNC();
      --t.tc.searches_done;
      w.gc.searches--;
      rc.valid = 0;
      return;
    }
    co_store_slot(A, cur_slot, cs, rc);
    if (D == 0) rc.cs = cs;
    if (D + 1 >= CO_PATH_MAX) {
      w.gc.error |= CO_ERR_PATH_TOO_DEEP;
      return;
    }
    uint32_t child_slot = CO_NODE_EDGE(cur, (uint32_t)best_e);
    CO_PH(9);
    if (best_slot.x == CO_NONE) {
      /* kNew: expand (Node ctor from parent, node.cpp:31-39) */
      uint64_t board = (uint64_t)h0.x | ((uint64_t)h0.y << 32);
      uint32_t meta = h0.z;
      int move = (int)CO_SLOT_MOVE(best_slot.z);
      co_do_move_lane(&board, &meta, move);
      int res;
      int depth = (int)CO_META_DEPTH(h0.z) + 1;
      CO_PH(16);
      CO_PROF_ADD(w, 24, 1ull);
      uint32_t nb = co_create_node(w, t, board, meta, depth, cur, child_slot, &res, &leaf_n, leaf_lm);
      if (nb == CO_NONE) return;
      if (w.analyse) {
        /* Node::countNodes (node.cpp:179-187) without a traversal: word z of unit b + 1 counts the
         * nodes below block b; a new node adds one to every node of its path */
        FOR_LANES {
          if (lane <= D) A[CO_NODE_INFO(path_block[lane])].z += 1u;
        }
        WAVE_SYNC();
      }
      cs = CO_SLOT_NEW(nb, 0u, CO_SLOT_MP(best_slot.z), res);
      cur = nb;
      cur_slot = child_slot;
      h0 = make_uint4((uint32_t)board, (uint32_t)(board >> 32), co_meta_make(meta, depth, 0), 0u);
      ++D;
      FOR_LANES {
        if (lane == 0) {
          path_block[D] = cur;
          path_slot[D] = cur_slot;
        }
      }
      WAVE_SYNC();
      CO_PH(10);
      break;
    }
    /* kVisited: descend */
    cur = best_slot.x;
    cur_slot = child_slot;
    cs = best_slot;
    h0 = co_load_unit(A, cur);
    h1 = co_load_unit(A, CO_NODE_INFO(cur));
    FOR_LANES { L(ev) = A[CO_NODE_EDGE(cur, lane)]; }
    v_sqrt_next = co_vsqrt(w.c_puct, co_slot_visits(cs)); /* under the fetch (see co_search_rows) */
    CO_OPAQUE_V(v_sqrt_next);
    CO_PH_MEM(11);
    ++D;
    FOR_LANES {
      if (lane == 0) {
        path_block[D] = cur;
        path_slot[D] = cur_slot;
      }
    }
    WAVE_SYNC();
  }
  int r = co_slot_result(cs);
  if (co_res_terminal(r)) {
    /* trainmc.cpp:663-682.  (For a fresh child the slot is first written here.) */
    float cur_eval = co_res_drawn(r) ? 0.0f : -1.0f;
    cs.y = co_f2u(cur_eval);
    co_store_slot(A, cur_slot, cs, rc);
    co_propagate_terminal(t, path_block, path_slot, D);
    FOR_LANES {
      if (lane < D) {
        int kk = D - lane; /* kk-th ancestor receives eval*(-1)^(kk-1) - 1 */
        float ce = ((kk - 1) & 1) ? (float)((double)cur_eval * -1.0) : cur_eval;
        float add = (float)((double)ce - 1.0);
        uint4 s = A[path_slot[lane]];
        s.y = co_f2u(co_u2f(s.y) + add);
        A[path_slot[lane]] = s;
      }
    }
    WAVE_SYNC();
    rc.valid = 0;
    CO_PH(12);
  } else {
    /* trainmc.cpp:684-692: default +1 evaluation, queue the leaf */
    cs.y = co_f2u(1.0f);
    co_store_slot(A, cur_slot, cs, rc);
    uint64_t board = (uint64_t)h0.x | ((uint64_t)h0.y << 32);
    co_request(w, board, h0.z, cur, leaf_n, leaf_lm, D, path_slot);
  }
}
