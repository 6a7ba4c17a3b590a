// search_tree.h -- search layer 1: the tree in its arena.
//
// The ONE definition of the tree's data layout (slot word and node block, below), the accessors of a slot and of a
// Node's result (node.cpp:96-118), and the functions that write a node and queue a leaf: Node's constructors and
// initializeEdges (node.cpp:14-39, 256-283), the request of an evaluation (trainmc.cpp:684-692, 150-153).
#pragma once
#include "engine_defs.h"
#include "rules.h"
#include "wave.h"
#include "search_state.h"

/* ---- The tree's data layout: the one place that spells it out.
 *
 * A tree lives in its arena as 16-byte UNITS (uint4), bump allocated, never freed within a game (engine_defs.h).  A node
 * is a BLOCK of units at offset b:
 *   unit b          header   {board_lo, board_hi, meta, parent_block}
 *   unit b + 1      info     {self_slot, denominator(f32), nodes below (analysis mode: Node::countNodes), 0}
 *   unit b + 2 + e  slot of edge e, e < n_edges, edges in ascending move id
 *   unit b + 2 + n  (only for a detached root) the root's own stat slot
 * A SLOT is
 *   x  child_block | CO_NONE
 *   y  evaluation (f32 bits)
 *   z  move_id:7 | prior:9 | visits:16 (signed)
 *   w  result:8 | all_visited:8 (bit 8)
 * The statistics of a node (Node::evaluation_ / visits_ / result_ / all_visited_, node.h:150-186) live in the SLOT of the
 * edge that leads to it -- in its parent's block -- so that one coalesced 16 B-per-lane load of a block gives the PUCT scan
 * everything it needs (trainmc.cpp:540-600); `self_slot` is the unit offset of that slot.  meta = pieces[6] (3 bits each)
 * | to_play<<18 | depth<<19 (6 bits) | n_edges<<25 (7 bits): rules.h CO_META_*.
 *
 * The hot paths decode a slot through the MACROS below, which expand to the plain expressions; the co_slot_* functions
 * serve everyone else.  (The two are not interchangeable in the search kernel: with functions taking the slot by value at
 * the macros' sites co_k_mcts_step keeps its opcode counts and registers but not its instruction stream.) */
#define CO_NODE_HDR(b) (b)                             /* the header unit */
#define CO_NODE_INFO(b) ((b) + 1u)                     /* {self_slot, denominator, nodes below, -} */
#define CO_NODE_EDGE0(b) ((b) + 2u)                    /* the slot of edge 0 */
#define CO_NODE_EDGE(b, e) (CO_NODE_EDGE0(b) + (e))    /* the slot of edge e */
#define CO_NODE_END(b, n) CO_NODE_EDGE(b, (uint32_t)(n)) /* the unit behind the n edges: a detached root's own slot, the next block */
#define CO_NODE_FIXED_UNITS 2u                         /* header and info */
#define CO_NODE_UNITS(n) (CO_NODE_FIXED_UNITS + (uint32_t)(n)) /* of a node with n edges that is not a detached root */
/* word z */
#define CO_SLOT_MOVE(z) ((z) & 127u)                   /* move id */
#define CO_SLOT_PRIOR_Q(s) (((s).z >> 7) & 511u)       /* prior quantum, 1 .. 511 once the priors are set */
#define CO_SLOT_MP(z) ((z) & 0xFFFFu)                  /* the move | prior half-word */
#define CO_SLOT_MP_MAKE(id, q) ((uint32_t)(id) | ((uint32_t)((q) & 511) << 7))
#define CO_SLOT_VISITS_SHIFT 16
#define CO_SLOT_ONE_VISIT (1u << CO_SLOT_VISITS_SHIFT) /* what a visit adds to z; z of a slot with one visit and no move */
/* word w */
#define CO_SLOT_RESULT_MASK 0xFFu
#define CO_SLOT_RESULT(s) ((int)((s).w & CO_SLOT_RESULT_MASK))
#define CO_SLOT_ALL_VISITED 0x100u
#define CO_SLOT_ALL_VISITED_BIT(s) (((s).w >> 8) & 1u)
/* whole slots */
#define CO_SLOT_EDGE(id) make_uint4(CO_NONE, 0u, (uint32_t)(id), 0u) /* an edge nobody has taken: no child, the priors to come */
/* the slot of a freshly emitted node: one visit, all_visited until its evaluation arrives (node.h:164,186) */
#define CO_SLOT_NEW(child, eval_bits, mp, res) make_uint4(child, eval_bits, (mp) | CO_SLOT_ONE_VISIT, (uint32_t)(res) | CO_SLOT_ALL_VISITED)
/* what the slot `bs` of an untaken edge becomes in the REGISTERS of the grouped selection when a simulation takes it: the
 * slot its child will be born with (block not yet known, the default +1 evaluation of trainmc.cpp:684-692) */
#define CO_SLOT_BORN(bs) make_uint4(0u, co_f2u(1.0f), CO_SLOT_MP((bs).z) | CO_SLOT_ONE_VISIT, CO_SLOT_ALL_VISITED)

/* ---- slot helpers */
CO_DEV int co_slot_visits(uint4 s) { return (int)(int16_t)(s.z >> CO_SLOT_VISITS_SHIFT); }
CO_DEV uint4 co_slot_set_visits(uint4 s, int v) {
  s.z = CO_SLOT_MP(s.z) | ((uint32_t)(uint16_t)(int16_t)v << CO_SLOT_VISITS_SHIFT);
  return s;
}
CO_DEV int co_slot_result(uint4 s) { return CO_SLOT_RESULT(s); }
CO_DEV int co_slot_all_visited(uint4 s) { return (int)CO_SLOT_ALL_VISITED_BIT(s); }
CO_DEV uint4 co_slot_set_result(uint4 s, int r) {
  s.w = (s.w & ~CO_SLOT_RESULT_MASK) | (uint32_t)r;
  return s;
}
CO_DEV uint4 co_slot_set_all_visited(uint4 s, int a) {
  s.w = (s.w & ~CO_SLOT_ALL_VISITED) | ((uint32_t)(a & 1) << 8);
  return s;
}
/* node.cpp:96-118 */
CO_DEV int co_res_terminal(int r) { return r == CO_RESULT_LOSS || r == CO_RESULT_DRAW; }
CO_DEV int co_res_known(int r) { return r != CO_RESULT_NONE; }
CO_DEV int co_res_won(int r) { return r == CO_DEDUCED_WIN; }
CO_DEV int co_res_lost(int r) { return r == CO_RESULT_LOSS || r == CO_DEDUCED_LOSS; }
CO_DEV int co_res_drawn(int r) { return r == CO_RESULT_DRAW || r == CO_DEDUCED_DRAW; }

/* uniform 16-byte read / single-lane write of one unit */
CO_DEV uint4 co_load_unit(const uint4 *A, uint32_t off) { return A[off]; }
CO_DEV void co_store_unit(uint4 *A, uint32_t off, uint4 v) {
  FOR_LANES {
    if (lane == 0) A[off] = v;
  }
  WAVE_SYNC();
}

CO_DEV void co_trace_push(CoWave &w, int32_t v) {
  if (!w.trace_on) return;
  if (w.gc.trace_len < CO_TRACE_CAP) {
    int at = w.gc.trace_len;
    FOR_LANES {
      if (lane == 0) w.trace[at] = v;
    }
  }
  w.gc.trace_len++;
}

/* Write the node of a position whose legal moves (lm, n of them) are known -- Node ctors node.cpp:14-39 +
 * initializeEdges node.cpp:256-283: bump allocation, header, edge slots in ascending move id.  self_slot == CO_NONE
 * makes a detached root that carries its own stat slot.  Returns the block offset (CO_NONE on arena overflow). */
CO_DEV uint32_t co_emit_node(CoWave &w, CoTree &t, uint64_t board, uint32_t meta_game, int depth, uint32_t parent,
                             uint32_t self_slot, const uint32_t lm[3], int n, int res) {
  const int n01 = co_popc32(lm[0]) + co_popc32(lm[1]);
  uint32_t units = CO_NODE_UNITS(n) + (self_slot == CO_NONE ? 1u : 0u);
  if (t.tc.units_used + units > t.cap) {
    w.gc.error |= CO_ERR_ARENA_FULL;
    return CO_NONE;
  }
  uint32_t b = t.tc.units_used;
  t.tc.units_used += units;
  if (t.tc.units_used > t.tc.peak_units) t.tc.peak_units = t.tc.units_used;
  w.gc.nodes++;
  uint32_t own = self_slot == CO_NONE ? CO_NODE_END(b, n) : self_slot;
  uint32_t meta = co_meta_make(meta_game, depth, n);
  uint4 *A = t.A;
  FOR_LANES {
    if (lane == 0) A[CO_NODE_HDR(b)] = make_uint4((uint32_t)board, (uint32_t)(board >> 32), meta, parent);
    if (lane == 1) A[CO_NODE_INFO(b)] = make_uint4(own, 0u, 0u, 0u);
    if (lane == 2 && self_slot == CO_NONE)
      A[own] = CO_SLOT_NEW(CO_NONE, 0u, 0u, res);
    /* edges in ascending move id: rank = number of legal moves below this id */
    const uint64_t lm01 = (uint64_t)lm[0] | ((uint64_t)lm[1] << 32);
    if ((lm01 >> lane) & 1ull) A[CO_NODE_EDGE(b, LANE_RANK64(lm01))] = CO_SLOT_EDGE(lane);
    if (((uint64_t)lm[2] >> lane) & 1ull) A[CO_NODE_EDGE(b, n01) + LANE_RANK64((uint64_t)lm[2])] = CO_SLOT_EDGE(64 + lane);
  }
  WAVE_SYNC();
  CO_PH(15);
  return b;
}

/* Create the node for position (board, meta_game): legal moves (game.cpp:28-43), terminal result (node.cpp:256-271),
 * then co_emit_node.  *res_out = kResultLoss / kResultDraw / kResultNone. */
CO_DEV uint32_t co_create_node(CoWave &w, CoTree &t, uint64_t board, uint32_t meta_game, int depth, uint32_t parent,
                               uint32_t self_slot, int *res_out, int *n_out = (int *)0, uint32_t *lm_out = (uint32_t *)0) {
  uint32_t lm[3];
  int is_lines = co_legal_moves1(board, meta_game, lm);
  CO_PH(14);
  if (lm_out) {
    lm_out[0] = lm[0];
    lm_out[1] = lm[1];
    lm_out[2] = lm[2];
  }
  int n = co_popc32(lm[0]) + co_popc32(lm[1]) + co_popc32(lm[2]);
  int res = CO_RESULT_NONE;
  if (n == 0) res = is_lines ? CO_RESULT_LOSS : CO_RESULT_DRAW;
  *res_out = res;
  if (n_out) *n_out = n;
  return co_emit_node(w, t, board, meta_game, depth, parent, self_slot, lm, n, res);
}

/* A leaf asks for a network evaluation: TrainMC writes the state into to_eval_
 * and records the node in searched_ (trainmc.cpp:684-692, 150-153). */
CO_DEV void co_request(CoWave &w, uint64_t board, uint32_t meta, uint32_t leaf, int n_edges, const uint32_t lm[3], int D,
                       const uint32_t *path_slot) {
  int k = w.gc.n_pending;
  co_write_state(board, meta, w.req + (size_t)k * CO_STATE_STRIDE);
  CO_PH(17);
  uint32_t *pp = w.pend_path + (size_t)k * CO_PATH_MAX;
  const uint32_t pn = ((uint32_t)w.noise_words << 8) | (uint32_t)n_edges;
  w.noise_words += n_edges; /* one generator output per legal move (trainmc.cpp:236-246) */
  FOR_LANES {
    if (lane == 0) {
      w.pend_leaf[k] = leaf;
      w.pend_depth[k] = D;
    }
    if (lane < 4) w.pend_n[4 * k + lane] = lane == 0 ? pn : lm[lane == 1 ? 0 : lane == 2 ? 1 : 2];
    if (lane <= D && lane < CO_PATH_MAX) pp[lane] = path_slot[lane];
    if (lane == 0 && w.pend_key) {
      /* the request row as a key: the board and the reserves in the order Game::writeGameState lays them out (the
       * mover's first, game.cpp:53-57) -- two positions with the same key have the same 70 floats */
      const uint32_t pc = meta & 0x3FFFFu;
      const uint32_t rot = ((meta >> 18) & 1u) ? ((pc >> 9) | (pc << 9)) & 0x3FFFFu : pc;
      w.pend_key[k] = make_uint4((uint32_t)board, (uint32_t)(board >> 32), rot | 0x80000000u, 0u);
    }
  }
  WAVE_SYNC();
  w.gc.n_pending = k + 1;
  CO_PH(18);
}
