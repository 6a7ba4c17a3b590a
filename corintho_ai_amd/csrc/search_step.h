// search_step.h -- search layer 7: the step of one game's wavefront (co_k_mcts_step's body).
//
// SelfPlayer::doIteration and chooseMoveAndContinue (selfplayer.cpp:115-122, 246-291) and Match's (match.cpp:67-79,
// 207-251) as one loop (co_game_step); which games step and where their rows are (Trainer::doIteration,
// trainer.cpp:169-174); the evaluation-cache probe, the pool's housekeeping and the step budget, the wave's set-up, the
// hand-over of a slot to the pool's next game, and the tail that captures noise and counts the batch's rows.
#pragma once
#include "engine_defs.h"
#include "rng.h"
#include "rules.h"
#include "wave.h"
#include "search_state.h"
#include "search_tree.h"
#include "search_eval.h"
#include "search_iter.h"
#include "search_move.h"

/* One step of a game:
 *   self-play   SelfPlayer::doIteration (selfplayer.cpp:115-122) + chooseMoveAndContinue
 *               (:246-291; chooseMove :234-244, endGame :206-232),
 *   tournament  Match::doIteration (match.cpp:67-79) + chooseMoveAndContinue (:207-251; chooseMove
 *               :192-205, endGame :163-190); gc.pos_* is Match::root_, a random side
 *               (players_[i] == nullptr) has no tree.
 * The reference's mutual recursion doIteration -> chooseMoveAndContinue -> doIteration is
 * written as ONE loop so that the kernel holds a single copy of the search, of the move choice
 * and of the hand-over: inlined along the call chain they were repeated up to seven times
 * (250 KB of instructions in front of a 64 KB instruction cache).  Returns "game over". */
CO_DEV int co_game_step(CoWave &w, const float *eval, const float *probs) {
  const float *ev = eval, *pr = probs;
  if (w.gc.resume) {
    /* continuation of a deferred hand-over: selfplayer.cpp:287-288 */
    w.gc.resume = 0;
    ev = pr = (const float *)0;
  }
  if (w.gc.held & 1) ev = pr = (const float *)0; /* continuation of a step cut at its budget: nothing was submitted */
  int skip_iteration = (w.pc && w.pc[w.gc.to_play].random) /* match.cpp:68-70 */ || w.force_choose;
  int fresh_root = 0;
  for (;;) {
    if (!skip_iteration) {
      int done = co_mc_do_iteration(w, w.me, ev, pr);
      if (w.gc.error) return 0;
      /* `return players_[to_play_]->doIteration()` after createRoot (selfplayer.cpp:281-283,
       * match.cpp:236-239): the new root asks for its evaluation, so this is "not over" */
      if (fresh_root) return done;
      if (!done) return 0;
    }
    skip_iteration = 0;
    ev = pr = (const float *)0;
    /* ---- chooseMoveAndContinue, one ply per pass of the loop */
    CO_PH(20);
    int p = w.gc.to_play;
    int choice, terminal, tres, depth;
    uint64_t board;
    uint32_t meta;
    if (w.pc && w.pc[p].random) {
      board = (uint64_t)w.gc.pos_lo | ((uint64_t)w.gc.pos_hi << 32);
      meta = w.gc.pos_meta;
      uint32_t lm[3];
      co_legal_moves1(board, meta, lm);
      int n = co_popc32(lm[0]) + co_popc32(lm[1]) + co_popc32(lm[2]);
      choice = co_nth_move(lm, (int)co_uniform_below(w, (uint32_t)n));
      co_trace_push(w, -2);
      co_trace_push(w, choice);
      w.gc.plies++;
      co_do_move_lane(&board, &meta, choice);
      int lines = co_legal_moves1(board, meta, lm);
      terminal = (lm[0] | lm[1] | lm[2]) == 0u;
      tres = lines ? CO_RESULT_LOSS : CO_RESULT_DRAW;
      depth = w.gc.plies; /* root_->depth() */
      if (w.log) { /* a random side has no pre-move block (match.cpp:213-221): record type 2 */
        int at = w.log[0];
        co_log_put(w, at, 2);
        co_log_put(w, at, choice);
        co_log_put(w, at, (int32_t)(uint32_t)board);
        co_log_put(w, at, (int32_t)(uint32_t)(board >> 32));
        co_log_put(w, at, (int32_t)meta);
        co_log_commit(w, at);
      }
    } else {
      CoTree &me = w.me;
      if (!w.pc) {
        uint4 rs = co_load_unit(me.A, co_load_unit(me.A, CO_NODE_INFO(me.tc.root)).x);
        if (co_res_known(co_slot_result(rs)) && w.gc.mate_turn == 0) w.gc.mate_turn = w.gc.n_samples + 1;
      }
      float *sample = (float *)0;
      if (!w.testing) {
        if (w.gc.n_samples >= CO_MAX_PLIES) {
          w.gc.error |= CO_ERR_TOO_MANY_PLIES;
          return 0;
        }
        sample = w.samples + (size_t)w.gc.n_samples * CO_SAMPLE_FLOATS;
      }
      choice = co_choose_move(w, me, sample);
      if (w.gc.error) return 0;
      if (w.analyse) {
        co_analyse_finish(w, me, choice);
        w.gc.plies++;
        return 1;
      }
      if (!w.testing) w.gc.n_samples++;
      co_trace_push(w, choice);
      w.gc.plies++;
      /* new root of the mover = the position on the board */
      uint4 h0 = co_load_unit(me.A, me.tc.root);
      uint4 nrs = co_load_unit(me.A, co_load_unit(me.A, CO_NODE_INFO(me.tc.root)).x);
      tres = co_slot_result(nrs);
      terminal = co_res_terminal(tres);
      board = (uint64_t)h0.x | ((uint64_t)h0.y << 32);
      meta = h0.z;
      depth = (int)CO_META_DEPTH(h0.z);
      if (w.log) { /* writeMoveChoice, selfplayer.cpp:199-204 */
        int at = w.log[0];
        co_log_put(w, at, choice);
        co_log_put(w, at, (int32_t)h0.x);
        co_log_put(w, at, (int32_t)h0.y);
        co_log_put(w, at, (int32_t)meta);
        co_log_commit(w, at);
      }
    }
    if (w.pc) {
      w.gc.pos_lo = (uint32_t)board;
      w.gc.pos_hi = (uint32_t)(board >> 32);
      w.gc.pos_meta = meta & 0x7FFFFu; /* reserves and side to move */
    }
    CO_PH_MEM(2);
    if (terminal) {
      if (tres == CO_RESULT_DRAW) w.gc.result = CO_RESULT_DRAW;
      else if (p == 1) w.gc.result = CO_RESULT_LOSS;
      else w.gc.result = CO_RESULT_WIN;
      return 1;
    }
    /* hand over: the opponent becomes the player to move */
    w.gc.to_play = 1 - p;
    {
      CoTree tmp = w.me;
      w.me = w.opp;
      w.opp = tmp;
    }
    co_use_player(w, 1 - p);
    if (w.pc && w.pc[1 - p].random) {
      skip_iteration = 1;
      continue;
    }
    CoTree &nm = w.me; /* the new player to move */
    if (nm.tc.root == CO_NONE) {
      /* first move of the second player: createRoot + doIteration */
      int res;
      uint32_t b = co_create_node(w, nm, board, meta, depth, CO_NONE, CO_NONE, &res);
      if (b == CO_NONE) return 0;
      nm.tc.root = b;
      fresh_root = 1;
      continue;
    }
    if (co_receive_opponent_move(w, nm, choice, board, meta, depth)) return 0; /* needs an evaluation */
    if (w.defer_handover) {
      /* Lock-step scheduling only: games are independent, so the new mover's first searches
       * may as well run in the next step.  Without this, the few games that change turns in
       * a step run up to twice the simulations of the others and every launch waits for
       * them.  The game's own sequence of operations is unchanged. */
      w.gc.resume = 1;
      return 0;
    }
    /* else: `need_eval = !doIteration()` -- search on; a finished turn chooses again */
  }
}

/* Does game g step in this launch?  0 no, 1 yes, 2 not yet released by the staggered start.
 * (trainer.cpp:176-196 training, :216-229 arena, tourney.cpp:63-72) */
CO_DEV int co_step_gate(const EngineParams &P, int g, const GameCtl &gc) {
  if (gc.done || gc.error) return 0;
  const int tp = P.arena_state ? P.arena_state[CO_AS_MODEL] : P.to_play;
  if (P.pcfg) {
    if (tp != CO_TO_PLAY_EVERY_MODEL && P.pcfg[2 * g + gc.to_play].model_id != tp) return 0; /* tourney.cpp:66 */
  } else if (tp == 0 || tp == 1) {
    if (gc.to_play != (tp + gc.parity) % 2) return 0;
  } else if (P.stagger_div > 0) {
    if ((P.game_base + g) / P.stagger_div > P.iteration) return 2;
  }
  return 1;
}

/* first row of game g's evaluations in nn_eval / nn_probs */
CO_DEV int co_step_row(const EngineParams &P, int g, const GameCtl &gc) {
  return P.fused_pack ? gc.row_off : P.read_offset ? P.read_offset[g] : P.req_offset[g];
}

/* ---- evaluation cache (engine_defs.h EvalCache), fused training: the tail of a game's step resolves its new request
 * rows to elements of the cache's value array, ONE LANE per row:
 *   the position has an entry of this pool (evaluated in an earlier iteration, or claimed by another row of this
 *   batch, whose outputs this iteration's network launch writes: stream order)   -> that entry;
 *   an entry of ANOTHER pool: its outputs are there once that pool's network launch of the claiming iteration has
 *   completed, which the pool's next search launch publishes (EvalCache::done)     -> that entry, if published;
 *   else the row is evaluated into its scratch element (nothing is waited for, no second entry is made);
 *   no entry, an empty slot in the probe window                -> the lane claims it, the row is evaluated into it;
 *   neither (the window is full)                               -> the row is evaluated into its scratch element.
 * Rows to evaluate are numbered with one atomic per game.  Correctness does not depend on who wins a race: every
 * path resolves a row to the network kernel's outputs for exactly its position (rows are evaluated independently
 * of their batch; keys are compared in full; an entry is never moved or reused before the table is
 * emptied as a whole, between two iterations).  Header words are accessed with relaxed device-scope atomics only:
 * the XCDs' L2s are not coherent with each other within a launch, and an acquire / release would invalidate /
 * write back a whole L2 per wave.  (Round 3 first had this as a kernel of its own between the search and the
 * network: 36 us per launch beside the other pool's network kernel, most of it waiting for a SIMD.) */
CO_DEV uint32_t co_cache_hash(uint32_t k0, uint32_t k1, uint32_t k2) {
  uint32_t h = k0 * 0x9E3779B1u;
  h = (h ^ (h >> 15)) + k1 * 0x85EBCA77u;
  h = (h ^ (h >> 13)) + k2 * 0xC2B2AE3Du;
  h ^= h >> 16;
  h *= 0x27D4EB2Fu;
  return h ^ (h >> 15);
}

/* request rows [row0, row0 + n) of `req` = the pending leaves 0 .. n - 1 of game g (keys in w.pend_key) */
CO_DEV void co_cache_resolve(const EngineParams &P, CoWave &w, int g, int n, int row0) {
  const EvalCache &C = P.cache;
  const int par = P.iteration & 1;
  int may_claim = !C.no_claim;
  if (may_claim && C.guard_pools) { /* an emptying not long ago: see EvalCache::guard_from */
    for (uint32_t p = 0; p < 4u; ++p)
      if (((C.guard_pools >> p) & 1u) && co_atomic_load_u32(C.done + p) <= C.guard_from) may_claim = 0;
  }
  LV(int, slot);
  LV(int, need);
  FOR_LANES {
    int sl = -1, nd = 0;
    if (lane < n) {
      const uint4 key = w.pend_key[lane];
      const uint32_t h = co_cache_hash(key.x, key.y, key.z);
      nd = 1;
      /* Header = {board lo ^ X, board hi ^ X, reserves | 1 << 31}; X sets the frozen bit of every cell, which no
       * position has (at most one cell is frozen, game.cpp:66-71): a header word that has not been written yet (0)
       * never equals a stored word, so the three words of an entry may become visible in any order -- a reader
       * takes an entry for its position only when all three are there.  The third word is the claim: empty = 0. */
      const uint32_t x0 = key.x ^ 0x88888888u, x1 = key.y ^ 0x88888888u;
      /* The claim word also names the claiming pool (bits the key leaves free), so whose entry it is is known with
       * the claim itself; the iteration of the claim follows in word 3 and matters to the OTHER pools only. */
      const uint32_t mine = key.z | C.pool_bits;
      for (int probe = 0; probe < CO_CACHE_PROBES; ++probe) {
        const uint32_t s = (h + (uint32_t)probe) & C.mask;
        uint32_t *H = C.hdr + (size_t)s * 4;
        uint32_t e0 = co_lane_load_coherent_u32(H + 0), e1 = co_lane_load_coherent_u32(H + 1), e2 = co_lane_load_coherent_u32(H + 2);
        if (e2 == 0u) {
          if (!may_claim) break; /* (EvalCache::no_claim, guard_from: the row is evaluated into its scratch element) */
          e2 = co_lane_cas_u32(H + 2, 0u, mine);
          if (e2 == 0u) {
            co_lane_store_coherent_u32(H + 0, x0);
            co_lane_store_coherent_u32(H + 1, x1);
            co_lane_store_coherent_u32(H + 3, (uint32_t)P.iteration + 1u);
            sl = (int)s; /* ours: this row is evaluated into the entry */
            break;
          }
          if ((e2 & ~CO_CACHE_POOL_MASK) == key.z) { /* taken this instant, perhaps for the same position: look again */
            e0 = co_lane_load_coherent_u32(H + 0);
            e1 = co_lane_load_coherent_u32(H + 1);
          }
        }
        if ((e2 & ~CO_CACHE_POOL_MASK) == key.z && e0 == x0 && e1 == x1) {
          if ((e2 & CO_CACHE_POOL_MASK) == C.pool_bits) {
            sl = (int)s;
            nd = 0;
          } else {
            /* another pool's: usable iff its claiming iteration's network launch is known to be over (a stamp that
             * is not visible yet reads 0: not usable) */
            const uint32_t stamp = co_lane_load_coherent_u32(H + 3);
            const uint32_t dn = co_lane_load_coherent_u32(C.done + ((e2 & CO_CACHE_POOL_MASK) >> CO_CACHE_POOL_SHIFT));
            if (stamp != 0u && stamp <= dn) {
              sl = (int)s;
              nd = 0;
            }
          }
          break;
        }
      }
    }
    L(slot) = sl;
    L(need) = nd;
  }
  const uint64_t nm = WAVE_BALLOT(need);
  const uint32_t cnt = (uint32_t)co_popc64(nm);
  uint32_t base = 0u;
  if (cnt) base = co_atomic_add_u32(C.count + CO_CACHE_COUNT_STRIDE * par, cnt);
  int32_t *psrc = P.pend_src + (size_t)g * P.searches_per_eval;
  FOR_LANES {
    if (lane < n) {
      int src = L(slot);
      if (L(need)) {
        const uint32_t m = base + (uint32_t)co_popc64(nm & ((1ull << lane) - 1ull));
        if (src < 0) src = (int)(C.mask + 1u + C.scratch_base + m); /* this pool's scratch element m of this iteration */
        C.in_idx[m] = row0 + lane;
        C.out_idx[m] = src;
      }
      psrc[lane] = src;
    }
  }
}

/* ---- the step of one game's wavefront (co_k_mcts_step), in pieces.
 * (Round 4 also ran fused training as TWO kernels -- the receive + simulate half as a hot kernel of its own, 62 spilled
 * SGPRs instead of 260 and a third of the instructions, and the once-per-ply work (move choice, logs, re-root, hand-over,
 * slot recycling) as a second launch over a list of the games whose turn had ended.  Measured on the same box,
 * alternating libraries: 4096 games x 400 simulations, mlp12x100 f16x3, 168.0 against 160.5 ms per generation, rescnn4
 * 518.4 against 512.8 -- the second launch per iteration costs more than the spills and the instruction-cache misses
 * of the cold paths, which are not executed in the hot loop anyway.  Removed; commit 28aee16 has it.) */

/* first wave of a pool's launch: clear the counters of the NEXT iteration (nobody reads them before the next launch) */
CO_DEV void co_pool_housekeeping(const EngineParams &P, int g) {
  if (P.fused_pack && g == P.pool_lo) {
    FOR_LANES {
      if (lane == 0) {
        P.pack_counter[(P.iteration + 1) & 1] = 0ull;
        if (P.work_counter) {
          /* step budget that follows the games (EngineParams::step_budget_k16): this launch's first wavefront turns what
           * the steps of the launch before cost (CO_STEP_*: ticks of the real-time counter on the device, scans on the
           * emulation build; complete: a kernel boundary lies between) into the budget of the launch after -- the division
           * is this one wavefront's, every other one reads a finished word */
          const unsigned long long wc = P.work_counter[(P.iteration + 2) % 3];
          const uint32_t steps = (uint32_t)(wc >> 32), scans = (uint32_t)wc;
          /* the mean, smoothed over ~8 launches (in 1/256 units; CO_WC_MEAN + parity carries it from launch to launch): the
           * games of a generation that started together also choose their moves together, and a launch of first steps on
           * fresh roots says nothing about the launch two later */
          unsigned long long sm = P.work_counter[CO_WC_MEAN + ((P.iteration + 1) & 1)];
          if (steps > 0u) {
            const unsigned long long inst = ((unsigned long long)scans << 8) / steps;
            sm = sm ? (7ull * sm + inst) >> 3 : inst;
          }
          uint32_t b = 0u; /* (no limit) */
          if (sm > 0ull && P.step_budget_k16 > 0) {
            b = (uint32_t)((sm * (uint32_t)P.step_budget_k16) >> 12);
            if (b < CO_STEP_BUDGET_MIN) b = CO_STEP_BUDGET_MIN;
          }
          P.work_counter[CO_WC_MEAN + (P.iteration & 1)] = sm;
          P.work_counter[CO_WC_BUDGET + (P.iteration & 1)] = (unsigned long long)b;
          P.work_counter[(P.iteration + 1) % 3] = 0ull;
        }
        if (P.cache.hdr) {
          /* the other parity's counter of rows to evaluate was the previous iteration's (its network launch is
           * over): book it, clear it for the next iteration */
          const int op = (P.iteration & 1) ^ 1;
          P.cache.totals[0] += P.cache.count[CO_CACHE_COUNT_STRIDE * op];
          P.cache.count[CO_CACHE_COUNT_STRIDE * op] = 0u;
          /* this launch stands behind the pool's network launch of iteration - 1 in its stream: entries the pool
           * claimed in iterations < iteration (stamps <= iteration) hold their outputs -- tell the other pools */
          co_lane_store_coherent_u32(P.cache.done + (P.cache.pool_bits >> CO_CACHE_POOL_SHIFT), (uint32_t)P.iteration);
        }
      }
    }
  }
}

/* The scans a game's step may make in this launch before it stops selecting (EngineParams::step_budget), fused training
 * only.  Automatic: what the first wavefront of the launch before this one made of the launch before that
 * (co_pool_housekeeping).  No limit = a number no step reaches. */
#define CO_STEP_BUDGET_NONE (1 << 28)
CO_DEV int co_step_budget(const EngineParams &P) {
  if (!(P.fused_pack && !P.testing && !P.analyse && !P.pcfg)) return CO_STEP_BUDGET_NONE;
  int b = P.step_budget * CO_STEP_UNITS_PER_CONFIG_UNIT;
  if (P.step_budget == 0 && P.step_budget_k16 > 0 && P.work_counter) b = (int)(uint32_t)P.work_counter[CO_WC_BUDGET + ((P.iteration + 1) & 1)];
  return b > 0 ? b : CO_STEP_BUDGET_NONE;
}

/* the wavefront's view of game slot g.  (Fields a kernel never touches cost nothing: they are never loaded.) */
CO_DEV void co_wave_init(const EngineParams &P, int g, const GameCtl &gc, const TreeCtl &tc0, const TreeCtl &tc1, CoWave &w) {
  w.g = g;
  w.gc = gc;
  {
    const size_t stride = (size_t)P.cap_units + CO_ARENA_PAD;
    const int tm = 2 * g + gc.to_play, to = 2 * g + 1 - gc.to_play;
    w.me.A = P.arena + (size_t)tm * stride;
    w.me.tc = gc.to_play ? tc1 : tc0;
    w.me.cap = P.cap_units;
    w.opp.A = P.arena + (size_t)to * stride;
    w.opp.tc = gc.to_play ? tc0 : tc1;
    w.opp.cap = P.cap_units;
  }
  w.mt = P.rng + (size_t)g * CO_MT_N;
  w.pend_leaf = P.pend_leaf + (size_t)g * P.searches_per_eval;
  w.pend_depth = P.pend_depth + (size_t)g * P.searches_per_eval;
  w.pend_path = P.pend_path + (size_t)g * P.searches_per_eval * CO_PATH_MAX;
  w.pend_n = P.pend_n + (size_t)g * P.searches_per_eval * 4;
  w.pend_key = P.cache.hdr ? P.pend_key + (size_t)g * P.searches_per_eval : (uint4 *)0;
  w.noise_raw = P.noise_raw + (size_t)g * P.searches_per_eval * CO_NUM_MOVES;
  w.noise_words = (gc.held & 1) ? gc.noise_held : 0; /* a step consumes every pending leaf before it queues new ones -- unless they were held back */
  w.work = CO_STEP_START(co_step_budget(P));
  w.req = P.req + (size_t)g * P.searches_per_eval * CO_STATE_STRIDE;
  /* samples and traces belong to the GAME, not to the slot */
  w.samples = P.samples ? P.samples + (size_t)gc.gid * CO_MAX_PLIES * CO_SAMPLE_FLOATS : (float *)0;
  w.trace = P.trace ? P.trace + (size_t)gc.gid * CO_TRACE_CAP : (int32_t *)0;
  w.log = (int32_t *)0;
  if (P.log) {
    const int rec = P.log_index ? P.log_index[gc.gid] : gc.gid < P.num_logged ? gc.gid : -1;
    if (rec >= 0) w.log = P.log + (size_t)rec * CO_LOG_CAP;
  }
  w.prof = P.prof ? P.prof + (size_t)g * CO_NPROF : (unsigned long long *)0;
  w.max_searches = P.max_searches;
  w.spe = P.searches_per_eval;
  w.testing = P.testing;
  w.trace_on = P.trace_on && P.trace;
  w.defer_handover = P.defer_handover;
  w.analyse = P.analyse;
  w.force_choose = P.analyse && P.force_choose;
  w.c_puct = P.c_puct;
  w.epsilon = P.epsilon;
  w.pc = P.pcfg ? P.pcfg + 2 * g : (const PlayerCfg *)0;
  co_use_player(w, gc.to_play);
  w.cval = P.cache.hdr ? P.cache.val : (const float *)0;
  w.csrc = P.cache.hdr ? P.pend_src + (size_t)g * P.searches_per_eval : (const int32_t *)0;
}

/* The slot's game is over: file it, and in a resident-slot pool hand the slot the next unstarted game.  Returns 1 when
 * a fresh game sits in the slot (its first step -- root + request for its evaluation -- is the caller's next pass). */
CO_COLD int co_slot_next_game(const EngineParams &P, CoWave &w) {
  w.gc.done = 1;
  if (!P.results) return 0;
  {
    GameCtl *dst = P.results + w.gc.gid;
    FOR_LANES {
      if (lane == 0) *dst = w.gc;
    }
    WAVE_SYNC();
  }
  const unsigned long long next = co_atomic_add_u64(P.next_game, 1ull);
  if (next >= (unsigned long long)P.total_local) return 0; /* none left: the slot is done */
  /* Trainer::initialize for game `next` (trainer.cpp:243-255) in this slot: a fresh SelfPlayer -- own
   * generator seeded from the Trainer stream by game index, two empty trees (the arena of the finished game
   * is given back whole: the bump pointers return to zero), colour parity by global index */
  const int gid = (int)next;
  if (w.gc.to_play != 0) { /* w.me is the tree of the player to move: player 0 starts */
    CoTree tmp = w.me;
    w.me = w.opp;
    w.opp = tmp;
  }
  GameCtl fresh;
  fresh.to_play = 0; fresh.done = 0; fresh.result = 0; fresh.mate_turn = 0; fresh.n_samples = 0;
  fresh.parity = (P.game_base + gid) % 2; fresh.error = 0; fresh.n_pending = 0; fresh.rng_idx = CO_MT_N;
  fresh.plies = 0; fresh.searches = 0u; fresh.evals = 0u; fresh.nodes = 0u; fresh.trace_len = 0;
  fresh.row_off = 0; fresh.resume = 0; fresh.pos_lo = 0u; fresh.pos_hi = 0u; fresh.pos_meta = CO_META_START;
  fresh.gid = gid;
  fresh.sb_cap = 0;
  fresh.held = 0;
  fresh.noise_held = 0;
  w.gc = fresh;
  w.me.tc.root = CO_NONE; w.me.tc.searches_done = 0; w.me.tc.units_used = 0u;   /* peak_units: high-water of the slot */
  w.opp.tc.root = CO_NONE; w.opp.tc.searches_done = 0; w.opp.tc.units_used = 0u;
  w.noise_words = 0;
  w.samples = P.samples ? P.samples + (size_t)gid * CO_MAX_PLIES * CO_SAMPLE_FLOATS : (float *)0;
  w.trace = P.trace ? P.trace + (size_t)gid * CO_TRACE_CAP : (int32_t *)0;
  w.log = (int32_t *)0; /* logged games are the first ones: they start in their own slots */
  co_mt_seed(w.mt, P.seeds[gid]);
  w.mt_staged = 0;
  return 1;
}

/* End of a game's step.  Trainer::writeRequests fused into the step: reserve rows of the compact batch (any order: a
 * row's evaluation does not depend on its position; the atomic's round trip runs under the noise capture), reserve the
 * generator outputs owed to the queued leaves, resolve the rows against the evaluation cache, copy them to the batch. */
CO_DEV void co_step_tail(const EngineParams &P, CoWave &w, int g, int done) {
  const int packs = P.fused_pack && !w.gc.done && !w.gc.error;
  unsigned long long old = 0ull;
  CO_PH_MEM(25);
  if (packs && P.work_counter) {
    const int scans = CO_STEP_DONE(w, co_step_budget(P)); /* (the budget once more, from where it lies: not kept across the step) */
    /* scans of the launch over the steps BEGUN in it: the pieces of a step that was cut add their scans, not a step -- counted
     * as steps of their own they pull the mean down, the budget follows, more steps are cut: it collapses to its floor */
    if (scans > 0) co_atomic_add_u64_noret(P.work_counter + P.iteration % 3, ((w.gc.held & 2) ? 0ull : 1ull << 32) | (unsigned long long)scans);
  }
  w.gc.held &= 1;
  if (packs && w.gc.held) {
    /* the step stopped at its budget: the game is running and submits nothing; its leaves (request rows, records and keys
     * are in place) wait for the rest of their batch, the generator outputs owed to them are reserved with the others' */
    /* (still running, no rows.  A held game is counted in the pool's CO_WC_CUTS word only, which the host copies with this
     * one at every poll to tell a window without rows from "no game has a request"; a count of held games in bits 56.. of
     * this word was 8 bits wide and read 256 of them as none) */
    co_atomic_add_u64_noret(P.pack_counter + (P.iteration & 1), CO_PACK_ONE_RUNNING);
    if (P.work_counter) co_atomic_add_u64_noret(P.work_counter + CO_WC_CUTS, 1ull); /* (ca_stats.steps_cut) */
    w.gc.noise_held = w.noise_words;
    return;
  }
  if (packs) old = co_atomic_add_u64(P.pack_counter + (P.iteration & 1), CO_PACK_ONE_RUNNING | (unsigned long long)w.gc.n_pending);
  CO_PH_MEM(26);
  if (!done && !w.gc.error && w.gc.n_pending > 0) co_capture_noise(w);
  CO_PH_MEM(27);
  if (packs) {
    const int n = w.gc.n_pending;
    const int base = P.pool_row_base + (int)co_pack_rows(old);
    w.gc.row_off = base;
    /* the rows stay in the game's request area; the network kernels read them through an index array (nn.h CoNetIO):
     * with the evaluation cache the rows it has to evaluate (co_cache_resolve), else every row of the batch.  (Until
     * round 5 the rows were copied into a compact batch here: 5 KB read back and written again at the end of every
     * step, 35 k cycles of the wave's 190 k with two pools in flight.) */
    const int first = g * P.searches_per_eval;
    if (w.pend_key) {
      co_cache_resolve(P, w, g, n, first);
    } else {
      int32_t *ri = P.row_idx + base;
      FOR_LANES {
        if (lane < n) ri[lane] = first + lane;
      }
    }
  }
}

CO_DEV void co_wave_store(const EngineParams &P, const CoWave &w, int g) {
  FOR_LANES {
    if (lane == 0) {
      P.games[g] = w.gc;
      P.trees[2 * g + w.gc.to_play] = w.me.tc;
      P.trees[2 * g + 1 - w.gc.to_play] = w.opp.tc;
    }
  }
}

/* Trainer::doIteration for game g (trainer.cpp:164-236): the body of the
 * `omp parallel for`, one wavefront per game. */
CO_DEV void co_mcts_step_wave(const EngineParams &P, int g) {
  co_pool_housekeeping(P, g);
  GameCtl gc = P.games[g];
  /* both trees' control words, fetched with the game's (not behind it) */
  const TreeCtl tc0 = P.trees[2 * g], tc1 = P.trees[2 * g + 1];
  const int gate = co_step_gate(P, g, gc);
  if (gate != 1) {
    if (gate == 2 && P.fused_pack) co_atomic_add_u64(P.pack_counter + (P.iteration & 1), CO_PACK_ONE_RUNNING); /* still running */
    return;
  }
  CoWave w;
  WAVE_SHARED(uint32_t, mt_stage, CO_MT_STAGE);
  w.mt_stage = mt_stage;
  WAVE_SHARED(uint32_t, pre_rec, CO_PRE_WORDS);
  w.pre = pre_rec;
  WG_SHARED(uint32_t, lb, CO_LB_WORDS);
  co_line_breakers_to_lds(lb);
  w.lb = lb;
  WG_SHARED(uint32_t, gam, CO_NUM_GAMMA);
  { /* (the same way: every wavefront writes the same words before it reads any) */
    FOR_LANES {
#pragma unroll
      for (int i = 0; i < CO_NUM_GAMMA / CO_WAVE; ++i) gam[i * CO_WAVE + lane] = CO_GAMMA_BITS[i * CO_WAVE + lane];
    }
    WAVE_SYNC();
  }
  w.gamma = gam;
#if defined(CO_PROF) && !defined(CO_EMU)
  const unsigned long long t_wave0 = CO_CLK(), t_real0 = __builtin_amdgcn_s_memrealtime();
  for (int i = 0; i < CO_NPROF; ++i) w.pacc[i] = 0ull;
  w.tph = t_wave0;
#endif
  co_wave_init(P, g, gc, tc0, tc1, w);
  /* (in front of the generator's state: the counter of outstanding loads retires in order, and the step needs these first) */
  w.pre_n = 0;
  if (w.gc.n_pending > 0 && !(w.gc.held & 1)) co_pending_records(w, 0, w.gc.n_pending < CO_PRE ? w.gc.n_pending : CO_PRE);
  co_mt_stage_load(w.mt, w.mt_stage);
  w.mt_staged = 1;
  CO_PROF_ADD(w, 4, 1ull);
  CO_PH_MEM(22);
  int off = co_step_row(P, g, gc);
  const float *step_eval = P.nn_eval + off, *step_probs = P.nn_probs + (size_t)off * CO_NUM_MOVES;
  int done;
  for (;;) { /* one pass, unless the slot's game ends and the pool hands it the next one */
    done = co_game_step(w, step_eval, step_probs);
    if (!done) break;
    if (!co_slot_next_game(P, w)) break;
    step_eval = step_probs = (const float *)0; /* the first step of a game creates the root and asks for its evaluation */
  }
  CO_PH(20);
  co_step_tail(P, w, g, done);
  CO_PH_MEM(21);
#if defined(CO_PROF) && !defined(CO_EMU)
  w.pacc[7] = CO_CLK() - t_wave0;
  if (w.prof && (threadIdx.x & 63) == 0) {
    for (int i = 0; i < CO_NPROF; ++i) w.prof[i] += w.pacc[i];
    const unsigned long long dt = w.pacc[7];
    unsigned long long *glob = P.prof + (size_t)P.num_games * CO_NPROF;
    if (g == 1) {
      glob[0] += dt;
      glob[1] += __builtin_amdgcn_s_memrealtime() - t_real0;
    }
    atomicMax(glob + 2, dt);
#ifndef CO_PROF_SLOW_FROM
#define CO_PROF_SLOW_FROM 0
#endif
#ifndef CO_PROF_SLOW_CYCLES
#define CO_PROF_SLOW_CYCLES 280000ull
#endif
    if (dt > CO_PROF_SLOW_CYCLES && P.iteration >= CO_PROF_SLOW_FROM) { /* the waves a launch waits for: their phases apart (slot 4 counts them) */
      for (int i = 0; i < CO_NPROF; ++i) atomicAdd(glob + 24 + i, w.pacc[i]);
    }
    int bucket = (int)(dt / 50000ull);
    if (bucket > 15) bucket = 15;
    atomicAdd(glob + 4 + bucket, 1ull);
  }
#endif
  co_wave_store(P, w, g);
}
