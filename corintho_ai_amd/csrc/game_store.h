// game_store.h -- the device side of a trainer's games (engine.hip ca_trainer): the slots of the pool with their trees,
// pending leaves, generators and request rows, the per-game arrays behind them (samples, traces, filed results) and the
// counters the kernels keep.  It sizes and allocates them, seeds a generation, and names them to the kernels (bind).
#pragma once
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "host.h"
#include "kernels.h"
#include "pools.h"

struct GameStore {
  int R = 0; /* slots of the pool = games resident at a time; R < G: slots are recycled (EngineParams::results) */
  bool recycle = false;
  uint32_t cap_units = 0;
  DevBuf<GameCtl> games;
  DevBuf<TreeCtl> trees;
  DevBuf<uint4> arena, pend_key;
  DevBuf<int32_t> pend_src;
  DevBuf<uint32_t> pend_leaf, pend_path, pend_n, noise_raw, rng;
  DevBuf<int32_t> pend_depth, req_offset, trace, all_done;
  DevBuf<float> req, nn_in, nn_in70, nn_eval, nn_probs, samples;
  DevBuf<int32_t> row_idx;
  DevBuf<unsigned long long> row_counter, pack_counter, work_counter, prof, next_game;
  DevBuf<GameCtl> results;    /* [G] finished games by index (recycling pools) */
  DevBuf<uint32_t> seeds_dev; /* [G] per-game generator seeds (recycling pools) */
  DevBuf<int32_t> arena_state; /* fused arena: see EngineParams::arena_state */
  DevBuf<int32_t> ctl;
  Pinned<int32_t> h_ctl; /* EngineParams::ctl of the last scan */

  size_t request_rows(int spe) const { return (size_t)R * spe; }

  /* the words of the evaluation cache behind every pending leaf (none for a trainer that can never have a cache) */
  void alloc_pend_keys(int spe, rt_stream_t s) {
    pend_key.alloc(request_rows(spe), s);
    pend_src.alloc(request_rows(spe), s);
  }

  /* can_recycle: the one mode whose games do not depend on which other games are resident (self-play training) */
  void create(const ca_config &cfg, int G, int spe, bool can_recycle, bool cache_words, rt_stream_t s) {
    uint32_t cap = cfg.arena_units;
    if (cap == 0) {
      /* a tree gains at most one node per simulation on its own turns; a node is
       * 2 + (legal moves) units, ~34 on average.  Sized for ~20 own turns of
       * typical growth; overflow is detected and reported, never silent. */
      uint64_t nodes = (uint64_t)cfg.max_searches * 14 + 64;
      cap = (uint32_t)std::min<uint64_t>(nodes * 40, 0x7FFFFFF0ull);
    }
    cap_units = cap;
    /* Resident slots.  The reference holds every game's trees at once and staggers the starts to bound them
     * (trainer.cpp:184-186); here `resident` slots hold the games in play and a slot whose game ends takes the
     * next one (training only: an arena game's trajectory depends on its batch, quirk 12).  0 = automatic: all
     * games resident if their trees fit in 5/8 of the free device memory, else as many slots as fit. */
    R = G;
    const size_t per_slot = (size_t)2 * ((size_t)cap + CO_ARENA_PAD) * sizeof(uint4) +
                            (size_t)spe * (CO_PATH_MAX * 4 + CO_NUM_MOVES * 4 + 2 * CO_STATE_STRIDE * 4 + CO_GAME_STATE_SIZE * 4 +
                                           CO_NUM_MOVES * 4 + 64) + CO_MT_N * 4 + 512;
    if (can_recycle && cfg.resident > 0 && cfg.resident < G) R = cfg.resident;
    if (can_recycle && cfg.resident == 0) {
      const size_t budget = rt_mem_free() / 8 * 5;
      const size_t per_game = (size_t)CO_MAX_PLIES * CO_SAMPLE_FLOATS * 4 + sizeof(GameCtl) + 8;
      if ((size_t)G * (per_slot + per_game) > budget) {
        size_t fit = budget > (size_t)G * per_game ? (budget - (size_t)G * per_game) / per_slot : 0;
        if (fit < 1) throw CaError(CA_ERR_DEVICE, "not enough device memory for a single resident game");
        R = (int)std::min<size_t>(fit, (size_t)G);
        if (R >= 512) R &= ~255; /* whole workgroups of the network kernels' row tiles */
      }
    }
    recycle = R < G;
    const size_t T = (size_t)2 * R, rows = request_rows(spe);
    games.alloc(R, s);
    trees.alloc(T, s);
    arena.alloc(T * ((size_t)cap + CO_ARENA_PAD), s);
    pend_leaf.alloc(rows, s);
    pend_depth.alloc(rows, s);
    pend_n.alloc(rows * 4, s);
    if (cache_words) alloc_pend_keys(spe, s);
    noise_raw.alloc(rows * CO_NUM_MOVES, s);
    pend_path.alloc(rows * CO_PATH_MAX, s);
    rng.alloc((size_t)R * CO_MT_N, s);
    req.alloc(rows * CO_STATE_STRIDE, s);
    req_offset.alloc((size_t)R + 1, s);
    nn_in.alloc(rows * CO_STATE_STRIDE, s);
    row_idx.alloc(rows, s);
    nn_in70.alloc(rows * CO_GAME_STATE_SIZE, s);
    ctl.alloc(CO_CTL_WORDS, s);
    h_ctl.alloc(CO_CTL_WORDS);
    nn_eval.alloc(rows, s);
    nn_probs.alloc(rows * CO_NUM_MOVES, s);
    if (!cfg.testing) samples.alloc((size_t)G * CO_MAX_PLIES * CO_SAMPLE_FLOATS, s); /* by game */
    if (cfg.trace) trace.alloc((size_t)G * CO_TRACE_CAP, s);                            /* by game */
    if (recycle) {
      results.alloc(G, s);
      seeds_dev.alloc(G, s);
    }
    next_game.alloc(1, s);
    all_done.alloc(1, s);
    row_counter.alloc(1, s);
    pack_counter.alloc((size_t)CO_PACK_STRIDE * CO_MAX_POOLS, s); /* a 128-byte line per pool: every wavefront of a launch adds to its pool's words */
    work_counter.alloc((size_t)CO_WC_WORDS * CO_MAX_POOLS, s);
    arena_state.alloc(CO_AS_WORDS, s);
#ifdef CO_PROF
    prof.alloc((size_t)R * CO_NPROF + 24 + CO_NPROF, s);
#endif
  }

  /* Trainer::initialize (trainer.cpp:238-256): game i is seeded with the i-th output of mt19937(cfg.seed), in global game
   * order; slot g starts with game g.  `given` (null: none) are the slots' seeds instead (a tournament's matches, given
   * positions); place(game, g) may put something else than the empty board into slot g.  Synchronises s. */
  template <class F>
  void seed(const ca_config &cfg, int G, const uint32_t *given, F &&place, rt_stream_t s) {
    size_t T = (size_t)2 * R;
    int total = cfg.total_games > 0 ? cfg.total_games : G;
    std::mt19937 gen((uint32_t)cfg.seed);
    std::vector<uint32_t> seeds(total);
    for (int i = 0; i < total; ++i) seeds[i] = (uint32_t)gen();
    std::vector<uint32_t> st((size_t)R * CO_MT_N);
    std::vector<GameCtl> hg(R);
    std::vector<TreeCtl> ht(T);
    for (int g = 0; g < R; ++g) {
      uint32_t *x = &st[(size_t)g * CO_MT_N];
      x[0] = given ? given[g] : seeds[cfg.game_base + g];
      for (int i = 1; i < CO_MT_N; ++i) x[i] = 1812433253u * (x[i - 1] ^ (x[i - 1] >> 30)) + (uint32_t)i;
      memset(&hg[g], 0, sizeof(GameCtl));
      hg[g].gid = g;
      hg[g].parity = (cfg.game_base + g) % 2;
      hg[g].rng_idx = CO_MT_N;
      hg[g].pos_meta = CO_META_START; /* Match::root_ = Node{} (match.h:91): the empty board */
      place(hg[g], g);
    }
    for (size_t t = 0; t < T; ++t) {
      ht[t].root = CO_NONE;
      ht[t].searches_done = 0;
      ht[t].units_used = 0;
      ht[t].peak_units = 0;
    }
    rt_h2d(rng.p, st.data(), st.size() * 4, s);
    rt_h2d(games.p, hg.data(), hg.size() * sizeof(GameCtl), s);
    rt_h2d(trees.p, ht.data(), ht.size() * sizeof(TreeCtl), s);
    if (recycle) {
      /* the games behind the first R: their seeds (the Trainer stream in game order) and the counter they are taken from */
      rt_h2d(seeds_dev.p, seeds.data() + cfg.game_base, (size_t)G * 4, s);
      rt_memset(results.p, 0, (size_t)G * sizeof(GameCtl), s);
    }
    const unsigned long long first_unstarted = (unsigned long long)R;
    rt_h2d(next_game.p, &first_unstarted, 8, s);
    rt_memset(row_counter.p, 0, 8, s);
    rt_memset(pack_counter.p, 0, (size_t)8 * CO_PACK_STRIDE * CO_MAX_POOLS, s);
    rt_memset(work_counter.p, 0, (size_t)8 * CO_WC_WORDS * CO_MAX_POOLS, s);
    rt_memset(arena_state.p, 0, CO_AS_WORDS * 4, s);
    rt_sync(s);
  }

  /* what stays fixed between runs, for every game of the trainer; a launch sets what is its own on a copy */
  void bind(EngineParams &P, const ca_config &cfg, int G, int spe) const {
    P.num_games = R;
    P.total_local = G;
    P.results = recycle ? results.p : nullptr;
    P.next_game = next_game.p;
    P.seeds = recycle ? seeds_dev.p : nullptr;
    P.max_searches = cfg.max_searches;
    P.searches_per_eval = spe;
    P.c_puct = cfg.c_puct;
    P.epsilon = cfg.epsilon;
    P.testing = cfg.testing;
    size_t div = (size_t)(cfg.total_games > 0 ? cfg.total_games : G) / (size_t)cfg.max_searches;
    if (div < 1) div = 1;
    /* the staggered start bounds the reference's memory (trainer.cpp:184-186); a recycling pool is bounded by its slots */
    P.stagger_div = (cfg.no_stagger || recycle) ? 0 : (int32_t)div;
    P.iteration = 0;
    P.to_play = -1;
    P.game_base = cfg.game_base;
    P.cap_units = cap_units;
    P.trace_on = cfg.trace;
    P.analyse = cfg.analyse;
    P.arena_state = nullptr;
    P.scan_phase = 0;
    P.games = games.p;
    P.trees = trees.p;
    P.arena = arena.p;
    P.pend_leaf = pend_leaf.p;
    P.pend_depth = pend_depth.p;
    P.pend_n = pend_n.p;
    P.pend_key = pend_key.p;
    P.pend_src = pend_src.p;
    P.noise_raw = noise_raw.p;
    P.pend_path = pend_path.p;
    P.rng = rng.p;
    P.req = req.p;
    P.req_offset = req_offset.p;
    P.nn_eval = nn_eval.p;
    P.nn_probs = nn_probs.p;
    P.nn_in = nn_in.p;
    P.row_idx = row_idx.p;
    P.nn_in70 = nn_in70.p;
    P.ctl = ctl.p;
    P.samples = samples.p;
    P.trace = trace.p;
    P.all_done = all_done.p;
    P.row_counter = nullptr; /* counted in fused mode only */
    P.fused_pack = 0;
    P.defer_handover = 0;
    /* ca_config.step_budget: n > 0 n microseconds (n scans on the emulation build, which has no clock:
     * CO_STEP_UNITS_PER_CONFIG_UNIT), 0 automatic (CO_STEP_BUDGET_K16 / 16 x the pool's mean), -1 none;
     * below -1 (diagnostic): automatic with the factor -n / 16 */
    P.step_budget = cfg.step_budget > 0 ? cfg.step_budget : 0;
    P.step_budget_k16 = cfg.step_budget == 0 ? CO_STEP_BUDGET_K16 : cfg.step_budget < -1 ? -cfg.step_budget : 0;
    P.work_counter = nullptr; /* a pool's own, set by FusedRun */
    P.pool_lo = 0;
    P.pool_n = R;
    P.pool_row_base = 0;
    P.pack_counter = pack_counter.p;
    P.prof = prof.p; /* (null unless a -DCO_PROF build) */
  }

  /* the highest arena use of any tree so far */
  int64_t peak_arena_units(rt_stream_t s) const {
    std::vector<TreeCtl> ht((size_t)2 * R);
    rt_d2h(ht.data(), trees.p, ht.size() * sizeof(TreeCtl), s);
    rt_sync(s);
    int64_t peak = 0;
    for (auto &x : ht) peak = std::max<int64_t>(peak, x.peak_units);
    return peak;
  }

  /* diagnostic builds (-DCO_PROF): summed in-kernel cycle stamps, see search_state.h */
  void read_prof(unsigned long long out[2 * CO_NPROF + 24], rt_stream_t s) const {
    /* nothing is written to `out` unless this is a stamped build: a caller of the shipped library with a buffer sized for
     * an earlier round's layout gets the error, not an overflow */
    if (!prof.p) throw CaError(CA_ERR_STATE, "not a -DCO_PROF build");
    for (int i = 0; i < 2 * CO_NPROF + 24; ++i) out[i] = 0;
    std::vector<unsigned long long> h((size_t)R * CO_NPROF);
    rt_d2h(h.data(), prof.p, h.size() * 8, s);
    rt_sync(s);
    for (int g = 0; g < R; ++g)
      for (int i = 0; i < CO_NPROF; ++i) out[i] += h[(size_t)g * CO_NPROF + i];
    /* [CO_NPROF ..): clocks, the histogram of wave-step times, then the phase sums of the slow wave-steps alone */
    rt_d2h(out + CO_NPROF, prof.p + (size_t)R * CO_NPROF, (size_t)(24 + CO_NPROF) * 8, s);
    rt_sync(s);
  }
};

/* A tournament's tables beside the store (tourney_host.h ca_tourney): one match per slot, both players of every match,
 * the matches' seeds, the reference's read offsets.  Empty for every other trainer. */
struct TourneyTables {
  std::vector<PlayerCfg> host_pcfg;  /* [2G] both sides of every match */
  std::vector<uint32_t> match_seeds; /* [G] */
  bool exact_offsets = false;        /* ca_tourney_set_exact_offsets */
  DevBuf<PlayerCfg> pcfg;
  DevBuf<int32_t> read_offset;

  bool active() const { return !host_pcfg.empty(); }
  void create(int R, rt_stream_t s) {
    pcfg.alloc(host_pcfg.size(), s);
    rt_h2d(pcfg.p, host_pcfg.data(), host_pcfg.size() * sizeof(PlayerCfg), s);
    read_offset.alloc((size_t)R, s);
  }
  void bind(EngineParams &P) const {
    P.pcfg = pcfg.p;
    P.read_offset = exact_offsets ? nullptr : read_offset.p; /* exact: co_step_row reads the writeRequests rows */
  }
};
