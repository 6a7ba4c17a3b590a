// pools.h -- host side of fused training: the pools of games and the evaluation cache's table
// they share (engine_defs.h EvalCache).  Included by engine.hip, after its runtime owners (DevBuf, Stream, Event,
// Pinned); the run itself is ca_trainer's (run_pools).
#pragma once

#define CO_MAX_POOLS 4
#ifndef CO_POOL_POLL
#define CO_POOL_POLL 16 /* fused training: iterations between polls of a pool's counter (round 5, three pools: 4 / 8 / 16 / 32 / 64 = 134.4 / 131.6 / 130.0 / 129.8 / 130.0 ms per mlp12x100 generation, 395.0 / 393.6 / 391.9 / 391.8 / 392.9 with rescnn4) */
#endif

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
        throw EngineError(CA_ERR_ARG, "ca_config.eval_cache: a table of 2^" + std::to_string(eval_cache) +
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

/* one independent slice of the games in fused training (run_pools) */
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
  Pinned<unsigned long long> word; /* [parity] counter word copied at the end of window parity 0 / 1, [2 + parity] rows the
                             * network evaluated in that iteration (evaluation cache), [4 + parity] the pool's steps cut so far
                             * (work_counter[CO_WC_CUTS]) */
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
#ifdef CO_EXP_CU_MASK /* diagnostic build (profiles/r06_coresident.md): every pool's stream on its own share of the compute units */
    st.create_masked(p, npools, CO_EXP_CU_MASK);
#else
    st.create();
#endif
    lo = (int)((int64_t)R * p / npools);
    n = (int)((int64_t)R * (p + 1) / npools) - lo;
    row_base = lo * spe;
    for (int w = 0; w < 2; ++w) {
      for (auto &e : ev[w]) e.create();
      polled[w].create();
    }
    word.alloc(6);
    quiet.create();
  }

  /* with the evaluation cache: the pool's index and counter arrays and its view of `table` */
  void attach(const CacheTable &table, int p, int spe) {
    const size_t rows = (size_t)n * spe;
    in_idx.alloc(rows, st);
    out_idx.alloc(rows, st);
    count.alloc(8, st);
    totals.alloc(2, st);
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
