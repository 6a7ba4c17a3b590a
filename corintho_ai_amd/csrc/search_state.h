// search_state.h -- search layer 0: what one game's wavefront carries through a step.
//
// CoTree (one player's arena and its TreeCtl, TrainMC's tree: trainmc.h:145-188) and CoWave (the game's GameCtl,
// SelfPlayer selfplayer.h:86-111, with the views, LDS pointers and settings of the step), the gamma table, and the two
// clocks of a step: the CO_PROF phase stamps (diagnostic build) and the CO_STEP_* budget clock.  No reference function is
// restated here.
#pragma once
#include "engine_defs.h"
#include "rng.h"
#include "rules.h"
#include "wave.h"

CO_CONST uint32_t CO_GAMMA_BITS[CO_NUM_GAMMA] = CO_GAMMA_BITS_INIT;

#define CO_NEG_INF (-__builtin_huge_valf())

#if defined(CO_SB_STATS) && defined(CO_EMU)
/* emulation-build counters of the grouped search (tools/sb_stats.py, tests/test_search_census_cpu.py): 0 groups,
 * 1 simulations asked for, 2 committed, 3 nothing searchable, 4 terminal child, 5 wide node, 6 too deep, 7 terminal leaf /
 * full arena, 8 sequential simulations, 9 levels of the groups, 10 scans, 11 patches applied (same node, same level),
 * 12 + k: groups that committed k, 20 shared levels below the root, 21 / 22 levels scanned wave-wide for one / two rows,
 * 23 levels in row form, 24 turns taken there;
 * and of co_receive_eval (search_eval.h): 25 rounds of pending-leaf records after a step's first (more than CO_PRE leaves),
 * 26 backup batches, 27 of them after a round's first (more than CO_RB leaves), 28 + k: passes of co_prior_all that set the
 * priors of k + 1 leaves (k < CO_SB_ROWS) */
extern unsigned long long co_sb_stats[32];
extern unsigned long long co_sb_ply[8][8]; /* by game progress (plies / 4): groups, asked, committed, terminal leaves, nothing searchable, levels, sequential, - */
#define CO_SBS(i, v) __atomic_fetch_add(&co_sb_stats[i], (unsigned long long)(v), __ATOMIC_RELAXED)
#define CO_SBP(w, i, v) __atomic_fetch_add(&co_sb_ply[(w).gc.plies / 4 > 7 ? 7 : (w).gc.plies / 4][i], (unsigned long long)(v), __ATOMIC_RELAXED)
#else
#define CO_SBS(i, v) ((void)0)
#define CO_SBP(w, i, v) ((void)0)
#endif

/* In-kernel phase stamps (diagnostic build only: hipcc -DCO_PROF, tools/prof_phases.py).  A wavefront keeps ONE running
 * clock (w.tph): CO_PH(slot) charges the cycles since the previous stamp to `slot`, so the slots add up to the wave's
 * whole step; the sums live in registers and are written once, at the end of the step (a stamp is an s_memtime and a
 * wait for it, ~50 cycles).  CO_PH_MEM(slot) first waits for the wave's outstanding memory operations, so that a phase
 * that ends with loads in flight is charged their latency (it also removes the overlap the product build has).
 * Slots: 0 backup: indices, 1 backup: slots fetched, 2 move choice / hand-over, 3 backup: sums and stores,
 *   4 steps (count), 5 simulations (count), 6 evaluations received (count), 7 whole step (cycles, measured apart),
 *   8 PUCT scan, 9 virtual-loss store + path, 10 expansion: slot + path update, 11 descent: block fetch waited for,
 *   12 terminal leaf, 13 (unused), 14 expansion: legal moves, 15 expansion: node stores, 16 expansion: doMove,
 *   17 request: state row, 18 request: pending-leaf records, 19 simulation start (root copy), 20 loop control + root
 *   load, 21 step tail (noise, batch rows, cache), 22 wave set-up, 23 levels scanned (count), 24 expansions (count) */
#define CO_NPROF 32
#if defined(CO_PROF) && !defined(CO_EMU)
#define CO_CLK() __builtin_amdgcn_s_memtime()
#define CO_PROF_ADD(w, slot, v) ((w).pacc[slot] += (v))
#define CO_PH(slot)                               \
  do {                                            \
    unsigned long long now_ = CO_CLK();           \
    w.pacc[slot] += now_ - w.tph;                 \
    w.tph = now_;                                 \
  } while (0)
#define CO_PH_MEM(slot)                                               \
  do {                                                                \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");       \
    CO_PH(slot);                                                      \
  } while (0)
#else
#define CO_CLK() 0ull
#define CO_PROF_ADD(w, slot, v) ((void)0)
#define CO_PH(slot) ((void)0)
#define CO_PH_MEM(slot) ((void)0)
#endif

/* What a step's budget is counted in (EngineParams::step_budget).  The device build measures TIME -- ticks of the 100 MHz
 * real-time counter since the step began: what a launch waits for is its slowest wavefront's time, whatever made it slow
 * (depth, terminal leaves and their propagation, a SIMD shared with another pool's kernel) -- and the emulation build, which
 * has no clock and must stay deterministic, counts PUCT scans (1 scan ~ 1.6 us).  Either way ONE scalar lives across the
 * step: the deadline (device) or the scans so far minus the budget (emulation). */
#ifndef CO_EMU
#define CO_STEP_CLOCK() ((uint32_t)__builtin_amdgcn_s_memrealtime())
#define CO_STEP_UNITS_PER_CONFIG_UNIT 100 /* ca_config.step_budget > 0 is in microseconds */
#define CO_STEP_WORK(w, n) ((void)0)
#define CO_STEP_START(budget) ((int)(CO_STEP_CLOCK() + (uint32_t)(budget)))
#define CO_STEP_SPENT(w) ((int)(CO_STEP_CLOCK() - (uint32_t)(w).work) >= 0)
#define CO_STEP_DONE(w, budget) ((int)(CO_STEP_CLOCK() - ((uint32_t)(w).work - (uint32_t)(budget))))
#else
#define CO_STEP_UNITS_PER_CONFIG_UNIT 1 /* ca_config.step_budget > 0 is in scans */
#define CO_STEP_WORK(w, n) ((w).work += (n))
#define CO_STEP_START(budget) (-(budget))
#define CO_STEP_SPENT(w) ((w).work >= 0)
#define CO_STEP_DONE(w, budget) ((w).work + (budget))
#endif

struct CoTree {
  uint4 *A;      /* arena of this tree */
  TreeCtl tc;    /* register copy, written back at the end of the step */
  uint32_t cap;
};

struct CoWave {
  int g;
  GameCtl gc;
#if defined(CO_PROF) && !defined(CO_EMU)
  unsigned long long pacc[CO_NPROF], tph;
#endif
  /* the tree of the player to move and the opponent's; swapped on hand-over so that
   * no register-resident state is indexed dynamically (that would spill to scratch) */
  CoTree me, opp;
  uint32_t *mt;
  const uint32_t *gamma; /* LDS: gamma_samples (util.h), CO_NUM_GAMMA words */
  const uint32_t *lb; /* LDS: line_breakers (rules.h co_line_breakers_to_lds) */
  int mt_staged;      /* mt_stage holds the generator's current state */
  uint32_t *mt_stage; /* LDS, CO_MT_STAGE words: staging copy of the generator state for a twist (rng.h co_mt_twist_lds) */
  /* per-game views */
  uint32_t *pend_leaf;
  int32_t *pend_depth;
  uint32_t *pend_path;
  uint32_t *pend_n;
  uint4 *pend_key;      /* cache keys of the pending leaves' rows, or null */
  const float *cval;    /* evaluation cache: outputs live in cval[csrc[k] * CO_CACHE_VAL_FLOATS] for pending leaf k; null = in place */
  const int32_t *csrc;
  uint32_t *noise_raw;
  int noise_words; /* generator outputs owed to the leaves queued so far (in this step, and in the steps before it that were
                    * cut short with their leaves held back: GameCtl::held) */
  int work; /* CO_STEP_*: the step's deadline (device), or its PUCT scans so far MINUS its budget (emulation) -- the step stops
             * selecting when the clock passes it / when it reaches zero (one live scalar instead of two: with the budget kept
             * beside a count the kernel spills 170 more SGPRs) */
  /* the records of up to CO_PRE pending leaves, in the wavefront's LDS: pre[f * CO_PRE + k] = field f (CO_PRE_*) of leaf
   * pre_c0 + k, k < pre_n.  Requested with the game's other first loads (co_mcts_step_wave) -- in registers until
   * co_receive_eval they cost 44 spilled registers in the search -- and read by co_receive_eval */
  int pre_n, pre_c0;
  uint32_t *pre;
  float *req;
  float *samples;
  int32_t *trace;
  int32_t *log; /* this game's text-log record (EngineParams::log), or null */
  unsigned long long *prof;
  /* config */
  int max_searches, spe, testing, trace_on, defer_handover, analyse, force_choose;
  float c_puct, epsilon;
  const PlayerCfg *pc; /* tournament match: the two players' settings, else null */
};
