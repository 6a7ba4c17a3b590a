// pools.h -- host side of fused training: the pools of games, the evaluation cache's table they
// share (engine_defs.h EvalCache) and the run that drives them (FusedRun) on a trainer's buffers (engine.hip ca_trainer).
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "host.h"
#include "kernels.h"

#define CO_MAX_POOLS 4
#define CO_POOL_POLL 16 /* fused training: iterations between polls of a pool's counter (round 5, three pools: 4 / 8 / 16 / 32 / 64 = 134.4 / 131.6 / 130.0 / 129.8 / 130.0 ms per mlp12x100 generation, 395.0 / 393.6 / 391.9 / 391.8 / 392.9 with rescnn4) */

/* what a trainer's runs have cost, by kernel family (ca_trainer_stats) */
struct RunStats {
  double mcts_ms = 0, nn_ms = 0, pack_ms = 0;
  int64_t mcts_launches = 0, nn_launches = 0, nn_rows = 0;
  /* fused training: the launches that carried timing events (one per pool and window) */
  double mcts_timed_ms = 0, nn_timed_ms = 0, pack_timed_ms = 0;
  int64_t timed_launches = 0, nn_timed_rows = 0;
  int64_t nn_rows_evaluated = 0; /* rows the network kernels worked on (= nn_rows without the evaluation cache) */
  int64_t steps_cut = 0, step_budget_last = 0; /* ca_config.step_budget: steps of the generation that stopped at their budget; the last budget */
  int64_t cache_clears = 0;

  /* device time by kernel family, estimated from the timed launches; with_pack: the fused pools' cache probe too (the
   * arena books its compaction directly) */
  void estimate_device_times(bool with_pack) {
    if (timed_launches == 0) return;
    mcts_ms = mcts_timed_ms * (double)mcts_launches / (double)timed_launches;
    nn_ms = nn_timed_ms * (double)nn_launches / (double)timed_launches;
    if (with_pack) pack_ms = pack_timed_ms * (double)nn_launches / (double)timed_launches;
  }
};

/* the search kernel (K3) over slots [pool_lo, pool_lo + n) of e */
static void launch_mcts_step(const EngineParams &e, int n, rt_stream_t s) {
  RT_LAUNCH(co_k_mcts_step, (n + CO_K3_WAVES - 1) / CO_K3_WAVES, CO_WAVE * CO_K3_WAVES, s, e);
}

/* the evaluation cache's table: ONE for all pools of a trainer */
struct CacheTable {
  DevBuf<uint32_t> hdr;  /* [entries][4] */
  DevBuf<float> val;     /* [entries + request rows of every pool][CO_CACHE_VAL_FLOATS]: table values + one scratch element per row */
  DevBuf<uint32_t> done; /* [CO_MAX_POOLS] */
  size_t entries = 0;

  /* a power of two of at least 8192 entries per slot (a 4096-game generation at 400 simulations asks for ~4100
   * distinct positions per game), within 1/6 of the free device memory; eval_cache > 0: 2^eval_cache entries */
  void create(int eval_cache, int R, int spe, rt_stream_t s) {
    size_t want = (size_t)R * 8192, n = 1;
    while (n < want) n <<= 1;
    const size_t per = 16 + CO_CACHE_VAL_FLOATS * 4;
    while (n > 1024 && n * per > rt_mem_free() / 6) n >>= 1;
    if (eval_cache > 0) { /* given */
      n = (size_t)1 << (eval_cache < 6 ? 6 : eval_cache > 30 ? 30 : eval_cache);
      if (n * per > rt_mem_free() / 2)
        throw CaError(CA_ERR_ARG, "ca_config.eval_cache: a table of 2^" + std::to_string(eval_cache) +
                                          " entries does not fit in the free device memory");
    }
    entries = n;
    hdr.alloc(n * 4, s);
    val.alloc((n + (size_t)R * spe) * CO_CACHE_VAL_FLOATS, s);
    done.alloc(CO_MAX_POOLS, s);
  }
  void release() {
    hdr.release();
    val.release();
    done.release();
    entries = 0;
  }
  /* every entry forgotten, queued on s; a new generation also restarts the pools' iteration marks */
  void empty(rt_stream_t s, bool new_generation) {
    rt_memset(hdr.p, 0, entries * 16, s);
    if (new_generation) rt_memset(done.p, 0, 4 * CO_MAX_POOLS, s); /* (the iteration count starts again with the generation) */
  }
};

/* one independent slice of the games in fused training (FusedRun) */
struct Pool {
  Stream st;
  int lo = 0, n = 0, row_base = 0;
  bool finished = false;
  int idle = 0;
  int running = 0; /* games of the pool still running at its last poll */
  Event ev[2][4]; /* per window parity: start / after search / after cache probe / after network of the TIMED iteration */
  Event polled[2];
  int launched[2] = {0, 0};  /* iterations queued in the window of that parity */
  int word_iter[2] = {0, 0}; /* Trainer::searches_done_ of the iteration whose counter word was copied */
  int first_start = 0;       /* iteration at which the stagger releases the pool's first game (trainer.cpp:184-186) */
  int timed[2] = {0, 0};     /* the window's last iteration carries the events */
  struct Seen { /* what the end of a window copies from the device, for its last iteration */
    unsigned long long pack; /* the pool's counter word (co_pack_rows, co_pack_running) */
    unsigned long long cuts; /* the pool's steps cut so far (work_counter[CO_WC_CUTS]) */
    uint32_t evaluated;      /* rows the network evaluated (evaluation cache) */
  };
  Pinned<Seen> seen; /* [window parity], page-locked */
  unsigned long long cuts_seen = 0; /* that count at the last window collected (at the start of the run: read when it began) */
  /* the pool's own arrays of the evaluation cache, and its view of them and of the shared table (hdr null: no cache) */
  DevBuf<int32_t> in_idx, out_idx;
  DevBuf<uint32_t> count;
  DevBuf<unsigned long long> totals;
  EvalCache cache = {};
  double c_inserted_est = 0; /* entries taken since the table was last emptied (estimate: timed iteration x window) */
  Event quiet;               /* emptying the shared table: the pool's stream has reached the iteration boundary */

  /* pool p of npools over R slots: its stream, its events and the host words the counters are copied to */
  void create(int p, int npools, int R, int spe) {
    st.create();
    lo = (int)((int64_t)R * p / npools);
    n = (int)((int64_t)R * (p + 1) / npools) - lo;
    row_base = lo * spe;
    for (int w = 0; w < 2; ++w) {
      for (auto &e : ev[w]) e.create();
      polled[w].create();
    }
    seen.alloc(2);
    quiet.create();
  }

  /* with the evaluation cache: the pool's index and counter arrays and its view of `table` */
  void attach(const CacheTable &table, int p, int spe) {
    const size_t rows = (size_t)n * spe;
    in_idx.alloc(rows, st);
    out_idx.alloc(rows, st);
    count.alloc(2 * CO_CACHE_COUNT_STRIDE, st);
    totals.alloc(CO_CACHE_TOTALS, st);
    cache.hdr = table.hdr.p;
    cache.val = table.val.p;
    cache.mask = (uint32_t)(table.entries - 1);
    cache.scratch_base = (uint32_t)row_base;
    cache.pool_bits = (uint32_t)p << CO_CACHE_POOL_SHIFT;
    cache.done = table.done.p;
    cache.in_idx = in_idx.p;
    cache.out_idx = out_idx.p;
    cache.count = count.p;
    cache.totals = totals.p;
    rt_sync(st);
  }

  /* a run starts: nothing queued, every game counted as running */
  void begin_run(unsigned long long cuts, int first) {
    cuts_seen = cuts;
    finished = false;
    running = n;
    idle = 0;
    launched[0] = launched[1] = 0;
    timed[0] = timed[1] = 0;
    word_iter[0] = word_iter[1] = 0;
    first_start = first;
  }
};

/* Fused training as independent pools of games on separate streams:
 * every pool runs the loop of main.pyx:142-168 on its own slice of the game arrays and of
 * the batch buffers; the GPU overlaps one pool's search kernel with another's network
 * kernel and fills launch tails.  Per-game results do not depend on the pooling.
 *
 * The pools and, with the evaluation cache, ONE table for all of them live as long as the trainer keeps their number
 * and the cache; everything else is the state of the run in progress. */
struct FusedRun {
  CacheTable table; /* fused training with the evaluation cache (entries 0: none) */
  std::vector<Pool> pools;
  bool cache_clean = false; /* the pools' tables hold nothing of an earlier generation */
  bool host_stepped = false; /* the caller evaluates the rows (HostNet): one pool, one iteration per run */

  /* what the trainer hands a run */
  EngineParams run_params;          /* its parameters for every game, fused_pack set (the iteration: set per launch) */
  unsigned long long *work_counter = nullptr; /* [CO_MAX_POOLS][CO_WC_WORDS], the pools' words of EngineParams::work_counter */
  float *nn_eval = nullptr, *nn_probs = nullptr; /* what run_params reads the evaluations from: where the network writes them */
  CoNet *net = nullptr;
  RunStats *stats = nullptr;
  rt_stream_t stream = {}; /* the trainer's own */
  /* the run */
  int npools = 0, spe = 0;
  static constexpr int poll = CO_POOL_POLL;
  int32_t iteration = 0; /* Trainer::searches_done_ */
  int window = 0, in_window = 0, parity = 0;
  long long guard_from = -1; /* the no-claim iteration behind the last emptying in mid-generation (EvalCache::guard_from) */
  std::string failure;

  /* the pools of a fused run; eval_cache: ca_config's, < 0 without the table */
  void create(int n, int R, int eval_cache) {
    pools.clear();
    table.release(); /* (before the new table is sized by the free device memory) */
    pools.resize(n);
    for (int p = 0; p < n; ++p) {
      Pool &q = pools[p];
      q.create(p, n, R, spe);
      if (eval_cache >= 0) {
        if (p == 0) table.create(eval_cache, R, spe, q.st);
        q.attach(table, p, spe);
      }
    }
    cache_clean = true; /* freshly zeroed */
  }
  void release() {
    pools.clear();
    table.release();
  }

  /* the pools' work-counter words (EngineParams::work_counter) as the device holds them now */
  std::vector<unsigned long long> read_work_counters() {
    std::vector<unsigned long long> wc((size_t)CO_WC_WORDS * CO_MAX_POOLS);
    rt_d2h(wc.data(), work_counter, wc.size() * 8, stream);
    rt_sync(stream);
    return wc;
  }

  /* a run starts: an emptied table when the generation does (or a new network came), the pools' host-side state.
   * Returns whether the table was emptied here. */
  bool begin(bool mid_generation) {
    const bool cache_clean_now = table.entries && !cache_clean;
    if (cache_clean_now) {
      /* a generation starts with an empty table: nothing evaluated in an earlier generation is carried over */
      table.empty(pools[0].st, true);
      for (auto &q : pools) {
        if (!mid_generation) { /* (in mid-generation -- a new network, set_net -- the rows evaluated so far stay counted: ADVICE round 4) */
          rt_memset(q.count.p, 0, 2 * CO_CACHE_COUNT_STRIDE * 4, q.st);
          rt_memset(q.totals.p, 0, CO_CACHE_TOTALS * 8, q.st);
        }
        rt_sync(q.st);
        q.c_inserted_est = 0;
      }
      cache_clean = true;
    }
    /* the steps cut so far (a run that resumes a generation: not zero), what the first window of each pool is compared with */
    const std::vector<unsigned long long> wc = read_work_counters();
    const EngineParams &P = run_params;
    for (auto &q : pools)
      q.begin_run(wc[CO_WC_WORDS * (&q - &pools[0]) + CO_WC_CUTS], P.stagger_div > 0 ? (P.game_base + q.lo) / P.stagger_div : 0);
    return cache_clean_now;
  }

  /* The host never waits for the window it has just queued: at the end of window w it queues
   * an asynchronous copy of each pool's counter and then reads the copy made at the end of
   * window w-1, so every stream always holds at least one window of work.  A pool is
   * therefore seen to be finished one window late; the launches in between find no running
   * game and no batch row. */
  void collect(Pool &q, int parity) {
    if (!q.launched[parity]) return;
    rt_event_sync(q.polled[parity]);
    const Pool::Seen &w = q.seen[parity];
    const uint32_t evaluated = q.cache.hdr ? w.evaluated : co_pack_rows(w.pack);
    q.running = (int)co_pack_running(w.pack);
    /* steps cut in the window: games held their leaves back (search_step.h co_step_tail), which submits no rows for them */
    const bool holding = w.cuts != q.cuts_seen;
    q.cuts_seen = w.cuts;
    if (q.timed[parity]) {
      /* one iteration per window is timed (three event records per launch pair cost 1-4 % of
       * the wall time); its batch size is the counter word just read */
      stats->mcts_timed_ms += rt_event_elapsed_ms(q.ev[parity][0], q.ev[parity][1]);
      stats->pack_timed_ms += rt_event_elapsed_ms(q.ev[parity][1], q.ev[parity][2]); /* cache probe (nothing without a cache) */
      stats->nn_timed_ms += rt_event_elapsed_ms(q.ev[parity][2], q.ev[parity][3]);
      stats->nn_timed_rows += (int64_t)evaluated; /* rows the network kernel worked on */
      /* every evaluated row takes a table entry; the timed iteration stands for its window, whose length is what was
       * queued in it (a full window: poll; a run capped at one iteration, HostNet: that one) */
      q.c_inserted_est += (double)evaluated * q.launched[parity];
      ++stats->timed_launches;
      q.timed[parity] = 0;
    }
    q.launched[parity] = 0;
    q.finished = q.running == 0;
    if (!q.finished && co_pack_rows(w.pack) == 0 && !holding) {
      /* main.pyx:161-163 raises when NO game has a request.  A pool whose first game the
       * staggered start (trainer.cpp:184-186) has not released yet has running games and no
       * rows by construction: that is not the reference's error condition */
      /* (an iteration whose games all stopped at their step budget has no rows either -- `holding`, a window in which steps
       * were cut: that is not it) */
      if (q.word_iter[parity] > q.first_start && ++q.idle > 16) failure = "No requests during training";
    } else {
      q.idle = 0;
    }
  }

  /* The table is half full: start over (returns true).  Between two iterations of EVERY pool, when no entry is pending. */
  bool cache_empty_when_half_full() {
    if (!table.entries) return false;
    double taken = 0;
    for (auto &q : pools) taken += q.c_inserted_est;
    if (taken > 0.5 * (double)table.entries) {
      /* the table is half full: start over (a long generation asks for far more positions than any table holds;
       * what is asked for again is mostly recent -- the trees of the games in play).  Between two iterations of
       * EVERY pool, when no entry is pending: each stream has the same iterations queued at this point; pool 0's
       * stream waits for the others to get here, empties the table, and the others wait for that. */
      for (int p = 1; p < npools; ++p) {
        rt_event_record(pools[p].quiet, pools[p].st);
        rt_stream_wait(pools[0].st, pools[p].quiet);
      }
      table.empty(pools[0].st, false);
      rt_event_record(pools[0].quiet, pools[0].st);
      for (int p = 1; p < npools; ++p) rt_stream_wait(pools[p].st, pools[0].quiet);
      for (auto &q : pools) q.c_inserted_est = 0;
      ++stats->cache_clears;
      return true;
    }
    return false;
  }

  /* one iteration of pool p on its stream: the search launch (with the step's share of the engine parameters: the pool's
   * slice, its counters, the evaluation cache's claim rules) and the network launch behind it; `timed`: with HIP events */
  void queue_iteration(int p, bool emptied, bool timed) {
    Pool &q = pools[p];
    if (q.finished) return;
    EngineParams pp = run_params;
    /* Deferring the new mover's first searches to the next step (search_step.h co_game_step) balances
     * the waves of a full launch but costs the game one more iteration per ply; once the pool
     * has thinned out, an iteration is as long as its slowest wave anyway and the number of
     * iterations of the longest game is what the generation waits for.  Per-game results do
     * not depend on the choice. */
    /* (stepped by the host, HostNet: an iteration more is a round trip to the caller more -- never deferred) */
    pp.defer_handover = !host_stepped && q.running * 2 > q.n ? 1 : 0;
    pp.pool_lo = q.lo;
    pp.pool_n = q.n;
    pp.pool_row_base = q.row_base;
    pp.pack_counter = run_params.pack_counter + CO_PACK_STRIDE * p;
    pp.work_counter = work_counter + (size_t)CO_WC_WORDS * p;
    /* (Measured and not done: no automatic budget for a thin pool -- the last eighth of a pool's games, or a trainer of
     * 64 -- on the reasoning that stopping the longest game's steps only adds iterations to its chain: 386.4 against 382.6
     * ms per default generation, 120.7 against 115.3 with the MLP, 95.3 against 93.9 at 64 games.  A thin launch waits for
     * its slowest wavefront like any other.) */
    pp.cache = q.cache; /* (hdr null: no cache) */
    pp.cache.no_claim = emptied ? 1u : 0u;
    if (emptied) guard_from = iteration;
    pp.cache.guard_pools = 0u;
    if (guard_from >= 0 && iteration <= guard_from + 2 * poll + 1) {
      /* (the streams are within two windows of each other: the host waits for window w - 1 before it queues w + 1) */
      pp.cache.guard_from = (uint32_t)guard_from;
      /* the OTHER pools only: this pool's own reads of the old contents happened in its launch of iteration
       * guard_from, which stands in front of this launch in its stream -- with its own bit set, every wavefront
       * that runs before the launch's first wave has stored done[p] would lose its claims for nothing */
      for (int p2 = 0; p2 < npools; ++p2)
        if (p2 != p && !pools[p2].finished) pp.cache.guard_pools |= 1u << p2;
    }
    /* The network launch is sized by what the batch can hold: the games still running at the pool's last poll (they
     * only become fewer) times the searches per evaluation.  In a generation's thin tail the throughput kernel is
     * then not launched at all and the small-batch kernel's grid shrinks -- a launch whose workgroups all leave at
     * once still costs their dispatch (for the pixel-major kernel: one 160 KB LDS allocation per 32 rows of capacity). */
    const int cap_rows = (q.running < q.n ? (q.running > 0 ? q.running : 1) : q.n) * spe;
    Event *e = q.ev[parity];
    if (timed) rt_event_record(e[0], q.st);
    launch_mcts_step(pp, q.n, q.st);
    if (timed) rt_event_record(e[1], q.st);
    if (timed) rt_event_record(e[2], q.st);
    CoNetIO io;
    io.alone = npools == 1;
    io.row_base = q.row_base; /* (a caller-supplied network's slice of its buffers, ExternalNet) */
    const int32_t *d_rows;
    float *d_eval, *d_probs;
    if (q.cache.hdr) {
      /* the search kernel has resolved every request row to an element of the cache's value array; the network
       * evaluates the rows whose position has no entry yet, reading them through in_idx and writing straight to
       * out_idx */
      io.in_idx = q.cache.in_idx;
      io.out_idx = q.cache.out_idx;
      io.eval_stride = CO_CACHE_VAL_FLOATS;
      io.probs_stride = CO_CACHE_VAL_FLOATS;
      d_rows = (const int32_t *)(q.cache.count + CO_CACHE_COUNT_STRIDE * (iteration & 1));
      d_eval = q.cache.val;
      d_probs = q.cache.val + 4;
    } else {
      io.in_idx = run_params.row_idx + q.row_base; /* the rows stay where the games wrote them (co_step_tail) */
      d_rows = (const int32_t *)(pp.pack_counter + (iteration & 1));
      d_eval = nn_eval + q.row_base;
      d_probs = nn_probs + (size_t)q.row_base * CO_NUM_MOVES;
    }
    net->forward(run_params.req, cap_rows, d_rows, d_eval, d_probs, q.st, io);
    if (timed) rt_event_record(e[3], q.st);
    if (timed) q.timed[parity] = 1;
    q.launched[parity] = in_window + 1;
    ++stats->mcts_launches;
    ++stats->nn_launches;
  }

  /* Up to max_iterations (<= 0: until every game is over) iterations of every pool; returns how many were queued.  A
   * failure is left in `failure`; the streams are drained either way. */
  int64_t run(const EngineParams &params, CoNet *network, int n, int eval_cache, bool mid_generation, int64_t max_iterations) {
    run_params = params;
    run_params.fused_pack = 1;
    net = network;
    spe = params.searches_per_eval;
    npools = n;
    if ((int)pools.size() != npools) create(npools, params.num_games, eval_cache);
    const bool cache_clean_now = begin(mid_generation);
    rt_sync(stream);
    iteration = params.iteration;
    int64_t it = 0;
    in_window = 0, window = 0;
    bool all_finished = false;
    failure.clear();
    /* the table was emptied in mid-generation (a new network, set_net): pending leaves point into its old contents */
    bool emptied_before_resuming = cache_clean_now && mid_generation;
    guard_from = -1;
    while (!all_finished && (max_iterations <= 0 || it < max_iterations)) {
      parity = window & 1;
      bool emptied = emptied_before_resuming; /* (EvalCache::no_claim) */
      emptied_before_resuming = false;
      if (cache_empty_when_half_full()) emptied = true;
      run_params.iteration = iteration;
      for (int p = 0; p < npools; ++p)
        queue_iteration(p, emptied, in_window == poll - 1 || (max_iterations > 0 && it + 1 == max_iterations));
      if (net->callback_failed()) break; /* nothing more is queued; the drain below, as on any other exit */
      const int counter_slot = iteration & 1;
      ++iteration;
      ++it;
      ++in_window;
      if (in_window == poll || (max_iterations > 0 && it == max_iterations)) {
        for (auto &q : pools) {
          if (q.finished) continue;
          const size_t p = &q - &pools[0];
          Pool::Seen &w = q.seen[parity];
          rt_d2h(&w.pack, run_params.pack_counter + CO_PACK_STRIDE * p + counter_slot, 8, q.st);
          if (q.cache.hdr) rt_d2h(&w.evaluated, q.cache.count + CO_CACHE_COUNT_STRIDE * counter_slot, 4, q.st);
          rt_d2h(&w.cuts, work_counter + (size_t)CO_WC_WORDS * p + CO_WC_CUTS, 8, q.st);
          q.word_iter[parity] = iteration - 1;
          rt_event_record(q.polled[parity], q.st);
        }
        all_finished = true;
        for (auto &q : pools) {
          if (!q.finished) collect(q, parity ^ 1);
          if (!q.finished) all_finished = false;
        }
        in_window = 0;
        ++window;
        if (!failure.empty()) break;
      }
    }
    /* drain: read what is still in flight (the last window, or both after an iteration cap).  EVERY pool's stream is
     * synchronised here, whichever way the loop ended: that is what allows `guard_from` to belong to one run -- a
     * later run (an iteration-capped run resumed) starts with no launch of any pool in flight, so no pool can still be
     * reading elements of a table emptied in an earlier run. */
    for (auto &q : pools) {
      rt_sync(q.st);
      for (int w = 0; w < 2; ++w) collect(q, (window + w) & 1);
    }
    return it;
  }

  /* after a run: the rows the network kernels worked on with the evaluation cache */
  int64_t rows_evaluated() {
    int64_t rows = 0;
    for (auto &q : pools) {
      /* booked by the probe kernels, plus the two iterations whose counters nobody has booked yet (at most one is non-zero) */
      unsigned long long tot = 0;
      uint32_t cnt[2 * CO_CACHE_COUNT_STRIDE] = {0};
      rt_d2h(&tot, q.totals.p, 8, q.st);
      rt_d2h(cnt, q.count.p, sizeof cnt, q.st);
      rt_sync(q.st);
      rows += (int64_t)tot + cnt[0] + cnt[CO_CACHE_COUNT_STRIDE];
    }
    return rows;
  }
  /* ... and the step budget's statistics: a pool's word CO_WC_CUTS counts the steps that were cut, CO_WC_BUDGET + {0, 1}
   * hold the last two budgets */
  void budget_stats() {
    const std::vector<unsigned long long> wc = read_work_counters();
    stats->steps_cut = 0;
    for (size_t p = 0; p < pools.size(); ++p) stats->steps_cut += (int64_t)wc[CO_WC_WORDS * p + CO_WC_CUTS];
    stats->step_budget_last = run_params.step_budget > 0
                                  ? run_params.step_budget
                                  : (int64_t)std::max(wc[CO_WC_BUDGET], wc[CO_WC_BUDGET + 1]) / CO_STEP_UNITS_PER_CONFIG_UNIT;
  }
};
