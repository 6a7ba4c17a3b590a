// search_move.h -- search layer 6: the move at the end of a turn.
//
// Re-rooting (moveDown, trainmc.cpp:475-495; the "reset tree" of :398-407, 455-464), TrainMC::chooseMove and its
// variants (trainmc.cpp:110-137, 298-473), receiveOpponentMove (:180-204), the records of
// the text logs (SelfPlayer::writePreMoveLogs / writeMoveChoice, selfplayer.cpp:185-204; Node::writeMainLine,
// node.cpp:197-240), a tournament's per-player settings and random player (match.cpp:199-200), and what analysis mode
// reads off the searcher after a move (docker/choose_move.pyx:206-221).
#pragma once
#include "engine_defs.h"
#include "rules.h"
#include "wave.h"
#include "search_state.h"
#include "search_tree.h"
#include "search_eval.h"
#include "search_iter.h"

/* TrainMC::moveDown, trainmc.cpp:475-495: the chosen child becomes the root.
 * Nothing is freed: the old root's block stays behind (it still holds the new
 * root's stat slot). */
CO_DEV void co_move_down(CoTree &t, uint32_t child_block) {
  uint4 h0 = co_load_unit(t.A, child_block);
  h0.w = CO_NONE; /* null_parent */
  co_store_unit(t.A, child_block, h0);
  t.tc.root = child_block;
  t.tc.searches_done = 0;
}

/* "Reset tree": a fresh root one move below the current one
 * (trainmc.cpp:398-407, 455-464). */
CO_DEV void co_reset_tree_to_child(CoWave &w, CoTree &t, int choice) {
  uint4 h0 = co_load_unit(t.A, t.tc.root);
  uint64_t board = (uint64_t)h0.x | ((uint64_t)h0.y << 32);
  uint32_t meta = h0.z;
  int depth = (int)CO_META_DEPTH(meta) + 1;
  co_do_move_lane(&board, &meta, choice);
  int res;
  uint32_t b = co_create_node(w, t, board, meta, depth, CO_NONE, CO_NONE, &res);
  if (b == CO_NONE) return;
  t.tc.root = b;
  t.tc.searches_done = 0;
}

/* ---- per-game text logs (SelfPlayer::writePreMoveLogs / writeMoveChoice, selfplayer.cpp:185-204).  The device records the
 * numbers, the host prints them (game_logs.h GameLogs::write).  One record per move choice:
 *   1, to_play, depth, root visits, root result, root evaluation bits,
 *   nc, nc x {move, visits, evaluation bits, result, probability bits}        the root's children (writeMoves :136-183)
 *   m x {depth, move, visits, result, evaluation bits, probability bits}, -1   the main line (Node::writeMainLine,
 *                                                                              node.cpp:197-240): most visits, then the
 *                                                                              larger evaluation; a lost child at once
 *   [after the choice, co_game_step] move, board low, board high, meta of the new position
 * and for the move of a tournament's random player: 2, move, board low, board high, meta.
 * `ch` is the caller's scratch for one node's slots.  Logged games are few (Trainer's default is 10); their waves spend a
 * few microseconds here once per ply. */
CO_DEV void co_log_put(CoWave &w, int &at, int32_t v) {
  if (at + 1 < CO_LOG_CAP) {
    int32_t *dst = w.log + 1 + at;
    FOR_LANES {
      if (lane == 0) *dst = v;
    }
  }
  ++at;
}
CO_DEV void co_log_commit(CoWave &w, int at) {
  int32_t *dst = w.log;
  FOR_LANES {
    if (lane == 0) *dst = at;
  }
  WAVE_SYNC();
}

CO_DEV void co_log_ply(CoWave &w, CoTree &t, uint4 (&ch)[CO_NUM_MOVES]) {
  uint4 *A = t.A;
  uint32_t node = t.tc.root;
  uint4 h0 = co_load_unit(A, node);
  uint4 h1 = co_load_unit(A, CO_NODE_INFO(node));
  uint4 rs = co_load_unit(A, h1.x);
  int at = w.log[0];
  co_log_put(w, at, 1);
  co_log_put(w, at, w.gc.to_play);
  co_log_put(w, at, (int)CO_META_DEPTH(h0.z));
  co_log_put(w, at, co_slot_visits(rs));
  co_log_put(w, at, co_slot_result(rs));
  co_log_put(w, at, (int32_t)rs.y);
  int depth = (int)CO_META_DEPTH(h0.z);
  for (int level = 0;; ++level) {
    int n = (int)CO_META_NEDGES(h0.z);
    float denom = co_u2f(h1.y);
    WAVE_SYNC();
    for (int base = 0; base < n; base += CO_WAVE) {
      FOR_LANES {
        int e = base + lane;
        if (e < n) ch[e] = A[CO_NODE_EDGE(node, e)];
      }
    }
    WAVE_SYNC();
    if (level == 0) {
      int nc = 0;
      for (int e = 0; e < n; ++e) nc += ch[e].x != CO_NONE;
      co_log_put(w, at, nc);
      for (int e = 0; e < n; ++e) {
        if (ch[e].x == CO_NONE) continue;
        co_log_put(w, at, (int)CO_SLOT_MOVE(ch[e].z));
        co_log_put(w, at, co_slot_visits(ch[e]));
        co_log_put(w, at, (int32_t)ch[e].y);
        co_log_put(w, at, co_slot_result(ch[e]));
        co_log_put(w, at, (int32_t)co_f2u((float)CO_SLOT_PRIOR_Q(ch[e]) * denom));
      }
    }
    int best = -1, max_visits = 0;
    float max_eval = 0.0f;
    for (int e = 0; e < n; ++e) {
      if (ch[e].x == CO_NONE) continue;
      int r = co_slot_result(ch[e]), v = co_slot_visits(ch[e]);
      float ev = co_u2f(ch[e].y);
      if (co_res_lost(r)) {
        best = e;
        break;
      }
      if (v > max_visits || (v == max_visits && ev > max_eval)) {
        best = e;
        max_visits = v;
        max_eval = ev;
      }
    }
    if (best < 0) break;
    ++depth;
    co_log_put(w, at, depth);
    co_log_put(w, at, (int)CO_SLOT_MOVE(ch[best].z));
    co_log_put(w, at, co_slot_visits(ch[best]));
    co_log_put(w, at, co_slot_result(ch[best]));
    co_log_put(w, at, (int32_t)ch[best].y);
    co_log_put(w, at, (int32_t)co_f2u((float)CO_SLOT_PRIOR_Q(ch[best]) * denom));
    node = ch[best].x;
    h0 = co_load_unit(A, node);
    h1 = co_load_unit(A, CO_NODE_INFO(node));
  }
  co_log_put(w, at, -1);
  co_log_commit(w, at);
}

/* TrainMC::chooseMove and its four variants, trainmc.cpp:110-137, 298-473.
 * sample = this ply's (state[70], policy[96]) row, or null in testing mode. */
CO_COLD int co_choose_move(CoWave &w, CoTree &t, float *sample) {
  uint4 *A = t.A;
  uint32_t root = t.tc.root;
  uint4 h0 = co_load_unit(A, root);
  uint4 h1 = co_load_unit(A, CO_NODE_INFO(root));
  uint4 rs = co_load_unit(A, h1.x);
  int n = (int)CO_META_NEDGES(h0.z);
  float denom = co_u2f(h1.y);
  int rres = co_slot_result(rs);
  uint64_t board = (uint64_t)h0.x | ((uint64_t)h0.y << 32);
  float *policy = sample ? sample + CO_GAME_STATE_SIZE : (float *)0;
  if (!w.testing) {
    /* state first (70 floats), then a zeroed policy */
    WAVE_SHARED(float, srow, CO_STATE_STRIDE);
    co_write_state(board, h0.z, srow);
    WAVE_SYNC();
    FOR_LANES {
      sample[lane] = srow[lane];
      if (lane < CO_GAME_STATE_SIZE - 64) sample[64 + lane] = srow[64 + lane];
      policy[lane] = 0.0f;
      if (lane < CO_NUM_MOVES - 64) policy[64 + lane] = 0.0f;
    }
    WAVE_SYNC();
  }
  /* children in edge order = the reference's sorted sibling list */
  WAVE_SHARED(uint4, ch, CO_NUM_MOVES);
  if (w.log) co_log_ply(w, t, ch); /* (uses ch for the nodes of the main line) */
  for (int base = 0; base < n; base += CO_WAVE) {
    FOR_LANES {
      int e = base + lane;
      if (e < n) ch[e] = A[CO_NODE_EDGE(root, e)];
    }
  }
  WAVE_SYNC();
  if (w.trace_on) {
    co_trace_push(w, w.gc.to_play);
    co_trace_push(w, (int)CO_META_DEPTH(h0.z));
    co_trace_push(w, co_slot_visits(rs));
    co_trace_push(w, rres);
    co_trace_push(w, (int32_t)rs.y);
    int nc = 0;
    for (int e = 0; e < n; ++e) nc += ch[e].x != CO_NONE;
    co_trace_push(w, nc);
    for (int e = 0; e < n; ++e) {
      if (ch[e].x == CO_NONE) continue;
      co_trace_push(w, (int)CO_SLOT_MOVE(ch[e].z));
      co_trace_push(w, co_slot_visits(ch[e]));
      co_trace_push(w, (int32_t)ch[e].y);
      co_trace_push(w, co_slot_result(ch[e]));
      co_trace_push(w, co_slot_all_visited(ch[e]));
    }
  }
  int choice = 0;
  int chosen_e = -1;
  if (co_res_won(rres)) {
    /* chooseMoveWon :310-335: first child that is lost */
    for (int e = 0; e < n; ++e) {
      if (ch[e].x != CO_NONE && co_res_lost(co_slot_result(ch[e]))) {
        choice = (int)CO_SLOT_MOVE(ch[e].z);
        chosen_e = e;
        break;
      }
    }
  } else if (co_res_lost(rres) || co_res_drawn(rres)) {
    /* chooseMoveLostDrawn :337-361 */
    int max_visits = 0;
    for (int e = 0; e < n; ++e) {
      if (ch[e].x == CO_NONE) continue;
      int v = co_slot_visits(ch[e]);
      if (v > max_visits && (co_res_lost(rres) || !co_res_won(co_slot_result(ch[e])))) {
        choice = (int)CO_SLOT_MOVE(ch[e].z);
        chosen_e = e;
        max_visits = v;
      }
    }
  } else {
    /* chooseHighProbMove :298-308 (int32 max_prob, sic) */
    int32_t max_prob = 0;
    for (int e = 0; e < n; ++e) {
      float p = (float)CO_SLOT_PRIOR_Q(ch[e]) * denom;
      if (p > (float)max_prob) {
        max_prob = (int32_t)p;
        choice = (int)CO_SLOT_MOVE(ch[e].z);
      }
    }
    if ((int)CO_META_DEPTH(h0.z) < 6 && !w.testing) {
      /* chooseMoveOpening :363-427 */
      int32_t visits = 0;
      for (int e = 0; e < n; ++e)
        if (ch[e].x != CO_NONE && !co_res_won(co_slot_result(ch[e]))) visits += co_slot_visits(ch[e]);
      float denominator = (float)(1.0 / (double)(float)visits);
      FOR_LANES {
        for (int e = lane; e < n; e += CO_WAVE)
          if (ch[e].x != CO_NONE && !co_res_won(co_slot_result(ch[e])))
            policy[CO_SLOT_MOVE(ch[e].z)] = (float)co_slot_visits(ch[e]) * denominator;
      }
      WAVE_SYNC();
      if (visits == 0) {
        FOR_LANES {
          if (lane == 0) policy[choice] = 1.0f;
        }
        WAVE_SYNC();
        co_reset_tree_to_child(w, t, choice);
        return choice;
      }
      int32_t target = (int32_t)(co_wave_mt_next(w) % (uint32_t)visits);
      int32_t total = 0;
      for (int e = 0; e < n; ++e) {
        if (ch[e].x == CO_NONE || co_res_won(co_slot_result(ch[e]))) continue;
        total += co_slot_visits(ch[e]);
        if (total > target) {
          choice = (int)CO_SLOT_MOVE(ch[e].z);
          chosen_e = e;
          break;
        }
      }
      if (chosen_e < 0) {
        w.gc.error |= CO_ERR_INTERNAL;
        return choice;
      }
      co_move_down(t, ch[chosen_e].x);
      return choice;
    }
    /* chooseMoveNormal :429-473 */
    int max_visits = 0;
    float max_eval = 0.0f;
    for (int e = 0; e < n; ++e) {
      if (ch[e].x == CO_NONE) continue;
      int r = co_slot_result(ch[e]);
      if (co_res_won(r)) continue;
      float ev = co_u2f(ch[e].y);
      if (r == CO_RESULT_DRAW || r == CO_DEDUCED_DRAW) ev = 0.0f;
      int v = co_slot_visits(ch[e]);
      if (v > max_visits || (v == max_visits && ev > max_eval)) {
        choice = (int)CO_SLOT_MOVE(ch[e].z);
        chosen_e = e;
        max_visits = v;
        max_eval = ev;
      }
    }
    if (policy) {
      FOR_LANES {
        if (lane == 0) policy[choice] = 1.0f;
      }
      WAVE_SYNC();
    }
    if (max_visits == 0) {
      co_reset_tree_to_child(w, t, choice);
      return choice;
    }
    co_move_down(t, ch[chosen_e].x);
    return choice;
  }
  /* won / lost / drawn roots */
  if (policy) {
    FOR_LANES {
      if (lane == 0) policy[choice] = 1.0f;
    }
    WAVE_SYNC();
  }
  if (chosen_e < 0) {
    /* the reference would move to the first child here; it cannot happen for a
     * root whose result was deduced from its children */
    w.gc.error |= CO_ERR_INTERNAL;
    return choice;
  }
  co_move_down(t, ch[chosen_e].x);
  return choice;
}

/* TrainMC::receiveOpponentMove, trainmc.cpp:180-204.  (board, meta) is the
 * opponent's new root position.  Returns "needs an evaluation". */
CO_COLD int co_receive_opponent_move(CoWave &w, CoTree &t, int move_choice, uint64_t board, uint32_t meta_game,
                                    int depth) {
  uint4 *A = t.A;
  uint32_t root = t.tc.root;
  int n = (int)CO_META_NEDGES(co_load_unit(A, root).z);
  uint32_t found = CO_NONE;
  for (int base = 0; base < n; base += CO_WAVE) {
    LV(int, hit);
    LV(uint32_t, cb);
    FOR_LANES {
      int e = base + lane;
      L(hit) = 0;
      L(cb) = CO_NONE;
      if (e < n) {
        uint4 s = A[CO_NODE_EDGE(root, e)];
        L(cb) = s.x;
        L(hit) = (s.x != CO_NONE) && ((int)CO_SLOT_MOVE(s.z) == move_choice);
      }
    }
    uint64_t m = WAVE_BALLOT(hit);
    if (m) found = WAVE_BCAST(cb, co_ffs64(m) - 1);
  }
  if (found != CO_NONE) {
    co_move_down(t, found);
    return 0;
  }
  int res;
  uint32_t b = co_create_node(w, t, board, meta_game, depth, CO_NONE, CO_NONE, &res);
  if (b == CO_NONE) return 1;
  t.tc.root = b;
  co_request_root(w, t);
  t.tc.searches_done = 1;
  return 1;
}

/* Tournament matches (match.h, match.cpp): the two sides search with their own settings */
CO_DEV void co_use_player(CoWave &w, int p) {
  if (!w.pc) return;
  w.max_searches = w.pc[p].max_searches;
  w.spe = w.pc[p].searches_per_eval;
  w.c_puct = w.pc[p].c_puct;
  w.epsilon = w.pc[p].epsilon;
}

/* std::uniform_int_distribution<int32_t>(0, n - 1)(generator_) of match.cpp:199-200 as libstdc++
 * (GCC >= 11) computes it on a 32-bit generator: Lemire's nearly divisionless method, one
 * 64-bit product per draw, a draw consumed even for n == 1 */
CO_DEV uint32_t co_uniform_below(CoWave &w, uint32_t n) {
  unsigned long long product = (unsigned long long)co_wave_mt_next(w) * (unsigned long long)n;
  uint32_t low = (uint32_t)product;
  if (low < n) {
    uint32_t threshold = (0u - n) % n;
    while (low < threshold) {
      product = (unsigned long long)co_wave_mt_next(w) * (unsigned long long)n;
      low = (uint32_t)product;
    }
  }
  return (uint32_t)(product >> 32);
}

/* the k-th (0-based) set bit of a 96-bit legal-move mask = Node::move_id(k) */
CO_DEV int co_nth_move(const uint32_t lm[3], int k) {
  for (int wd = 0; wd < 3; ++wd) {
    int c = co_popc32(lm[wd]);
    if (k < c) {
      uint32_t m = lm[wd];
      for (int i = 0; i < k; ++i) m &= m - 1u;
      return wd * 32 + co_ffs64((uint64_t)m) - 1;
    }
    k -= c;
  }
  return -1;
}

/* Analysis mode: what docker/choose_move.pyx:206-221 reads off the DockerMC after chooseMove(), written as
 * eight words into the slot's request area: {move, Node result of the new root (util.h:57-64), nodes in
 * the kept tree (num_nodes), bits of the new root's summed evaluation (eval), legal-move mask of the new
 * root [3], 1} -- done() = result is a terminal one, drawn() = result is a draw. */
CO_DEV void co_analyse_finish(CoWave &w, CoTree &t, int choice) {
  uint4 h0 = co_load_unit(t.A, t.tc.root);
  uint4 h1 = co_load_unit(t.A, CO_NODE_INFO(t.tc.root));
  uint4 rs = co_load_unit(t.A, h1.x);
  uint32_t lm[3];
  co_legal_moves1((uint64_t)h0.x | ((uint64_t)h0.y << 32), h0.z, lm);
  uint32_t *out = (uint32_t *)w.req;
  FOR_LANES {
    if (lane == 0) {
      out[0] = (uint32_t)choice;
      out[1] = (uint32_t)co_slot_result(rs);
      out[2] = h1.z + 1u;
      out[3] = rs.y;
      out[4] = lm[0];
      out[5] = lm[1];
      out[6] = lm[2];
      out[7] = 1u;
    }
  }
  WAVE_SYNC();
}
