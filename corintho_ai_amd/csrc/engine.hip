// engine.hip -- host side of the self-play pool and the C ABI (include/corintho_hip.h); networks come in through
// net_host.h, fused training runs in pools.h, the words host and kernels pass each other are named in engine_defs.h.
//
// Mirrors the reference Trainer (corintho_ai/cpp/src/trainer.cpp) method by
// method; the per-game work of every method runs in the kernels of kernels.h.
// Compat mode keeps the reference protocol (the caller evaluates the network
// between doIteration calls, main.pyx:123-187); fused mode (nn_*.hip) keeps
// the whole loop on the device.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "logfmt.h"
#include "net_host.h"
#include "pools.h"

#ifdef CO_EMU
thread_local int co_emu_block_idx = 0;
#ifdef CO_SB_STATS
unsigned long long co_sb_stats[32];
unsigned long long co_sb_ply[8][8];
extern "C" unsigned long long *co_emu_sb_stats(void) { return co_sb_stats; }
extern "C" unsigned long long *co_emu_sb_ply(void) { return &co_sb_ply[0][0]; }
#endif
#endif

thread_local std::string g_last_error;
extern "C" const char *ca_last_error(void) { return g_last_error.c_str(); }
void co_set_last_error(const std::string &m) { g_last_error = m; }

struct ca_trainer {
  ca_config cfg;
  int G = 0, spe = 0; /* games of this trainer */
  int R = 0;          /* slots of the pool = games resident at a time; R < G: slots are recycled (EngineParams::results) */
  bool recycle = false;
  uint32_t cap_units = 0;
  Stream stream;
  EngineParams P; /* what stays fixed between runs; a launch takes its own copy (params) */
  DevBuf<GameCtl> games;
  DevBuf<TreeCtl> trees;
  DevBuf<uint4> arena, pend_key;
  DevBuf<int32_t> pend_src;
  DevBuf<uint32_t> pend_leaf, pend_path, pend_n, noise_raw, rng;
  DevBuf<int32_t> pend_depth, req_offset, trace, all_done;
  DevBuf<int32_t> logbuf; /* per-game text logs: EngineParams::log */
  DevBuf<int32_t> log_index; /* tournament: EngineParams::log_index */
  std::vector<int> log_game;          /* record k belongs to game log_game[k] ... */
  std::vector<std::string> log_paths; /* ... and goes to this file */
  int num_logged = 0;
  bool logs_written = false;
  DevBuf<float> req, nn_in, nn_in70, nn_eval, nn_probs, samples;
  DevBuf<int32_t> row_idx;
  DevBuf<unsigned long long> row_counter, pack_counter, work_counter, prof, next_game;
  DevBuf<GameCtl> results;   /* [G] finished games by index (recycling pools) */
  DevBuf<uint32_t> seeds_dev; /* [G] per-game generator seeds (recycling pools) */
  DevBuf<int32_t> ctl;
  Pinned<int32_t> h_ctl; /* EngineParams::ctl of the last scan (read_ctl) */
  /* buffers of the host-facing calls, kept (and grown on demand) instead of allocated per call */
  DevBuf<int32_t> ws_off, fw_rows;
  DevBuf<float> ws_gs, ws_ev, ws_pr, fw_in70, fw_in, fw_ev, fw_pr;
  /* caller buffers page-locked for direct DMA (ca_trainer_pin_host) */
  std::vector<std::pair<void *, size_t>> host_regs;
  /* host state */
  int64_t iterations = 0;
  int32_t trainer_iteration = 0; /* Trainer::searches_done_ (train mode only) */
  int scan_valid_for = 0;      /* to_play / model id the current req_offset/nn_in describe (if scan_valid) */
  int32_t last_total = 0;
  bool finished = false;
  bool any_error = false; /* the last scan saw an error bit in some game */
  bool net_used = false;  /* a network launch has been queued since the range flags were last read */
  std::vector<GameCtl> host_games;
  bool host_games_valid = false;
  /* fused mode */
  std::unique_ptr<CoNet> nets[2];
  /* a caller-supplied network function (ExternalNet) that returned non-zero: the generation is unusable until ca_trainer_reset */
  CallbackState callback{false, false, " in this generation; it cannot go on -- start a new one with ca_trainer_reset"};
  RunStats stats;
  FusedRun fused; /* fused training: the pools, their table and the run (pools.h) */
  /* the evaluation cache serves fused training (and fused analysis): one network, rows packed by the search kernel */
  /* Not for the analysis of caller-given positions (the table's header encoding relies on boards that doMove
   * produced).  Automatic (eval_cache = 0): only for a network whose rows cost more than resolving them -- the 9.65
   * MFLOP residual CNN, not the 0.25 MFLOP MLP (measured: the MLP's whole launch is 43 us for 12 k rows, the probe 15). */
  bool use_cache() const {
    if (cfg.eval_cache < 0 || tourney || cfg.analyse) return false;
    if (cfg.eval_cache > 0) return true;
    return nets[0] && nets[0]->flop_per_row() >= 1e6;
  }

  /* host-driven protocol with the evaluation cache (ca_trainer_set_host_cache): fused training on one pool, stepped one
   * iteration per doIteration, the caller as its network (net_host.h HostNet) */
  bool host_cache = false;
  int host_cache_log2 = -1; /* the table: 0 sized automatically, else 2^n entries */
  int32_t host_rows = 0;    /* rows handed to the caller by the last iteration: the cache's count word */
  HostNet host_net;

  /* tournament mode (ca_tourney): per-match players, per-match seeds, the reference's read offsets */
  bool tourney = false, exact_offsets = false;
  std::vector<PlayerCfg> host_pcfg; /* [2G] */
  std::vector<uint32_t> match_seeds; /* [G] */
  DevBuf<PlayerCfg> pcfg;
  DevBuf<int32_t> arena_state; /* fused arena: see EngineParams::arena_state */
  DevBuf<int32_t> read_offset;
  bool scan_valid = false;

  /* analysis mode: the positions (DockerMC constructor arguments) */
  std::vector<uint32_t> an_pos;   /* [G][3] board lo, board hi, meta */
  std::vector<uint32_t> an_seed;  /* [G] */
  std::vector<int32_t> an_pre;    /* [G] Node result of a position that is terminal as given, else 0 */

  ~ca_trainer() {
    for (auto &r : host_regs) rt_host_unregister(r.first);
  }

  int dev() const { return cfg.device; }
  /* the one mode whose slots are recycled: its games do not depend on which other games are resident */
  bool self_play_training() const { return !cfg.testing && !cfg.analyse && !tourney; }
  /* the device has moved on: what the host knows of the batch and of the games is stale */
  void invalidate() { scan_valid = host_games_valid = false; }

  template <typename T>
  void ensure(DevBuf<T> &b, size_t count) {
    if (b.n < count) b.alloc(count + count / 4, stream);
  }

  /* Page-lock a caller buffer (the three arrays of main.pyx:132-134 live as long as the Trainer):
   * copies from / to it are then direct DMA at PCIe speed instead of staged through the runtime's
   * bounce buffers.  The buffer must stay allocated until it is unpinned or the trainer destroyed. */
  bool pin_host(void *p, size_t bytes) {
    for (auto &r : host_regs)
      if (r.first == p && r.second >= bytes) return true;
    unpin_host(p); /* (registered with fewer bytes) */
    if (!rt_host_register(p, bytes)) return false;
    host_regs.emplace_back(p, bytes);
    return true;
  }
  void unpin_host(void *p) {
    for (size_t i = 0; i < host_regs.size(); ++i)
      if (host_regs[i].first == p) {
        rt_host_unregister(p);
        host_regs[i] = host_regs.back();
        host_regs.pop_back();
        return;
      }
  }

  /* a tournament's trainer (ca_tourney): one match per game */
  struct TourneySetup {
    std::vector<PlayerCfg> players; /* [2G] both sides of every match */
    std::vector<uint32_t> seeds;    /* [G] */
    bool exact_offsets;             /* ca_tourney_set_exact_offsets */
  };
  void init(const ca_config &c, const TourneySetup *tour = nullptr) {
    cfg = c;
    if (tour) {
      tourney = true;
      host_pcfg = tour->players;
      match_seeds = tour->seeds;
      exact_offsets = tour->exact_offsets;
    }
    if (cfg.analyse) {
      cfg.testing = 1;    /* trainmc.cpp:43 */
      cfg.no_stagger = 1;
      cfg.game_base = cfg.total_games = 0;
    }
    if (cfg.max_searches <= 0) cfg.max_searches = 1600;
    if (cfg.searches_per_eval <= 0) cfg.searches_per_eval = 16;
    if (cfg.c_puct <= 0.0f) cfg.c_puct = 1.0f;
    G = cfg.num_games;
    spe = cfg.searches_per_eval;
    rt_set_device(cfg.device);
    stream.create();
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
    const bool can_recycle = self_play_training();
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
    size_t T = (size_t)2 * R;
    games.alloc(R, stream);
    trees.alloc(T, stream);
    arena.alloc(T * ((size_t)cap + CO_ARENA_PAD), stream);
    pend_leaf.alloc((size_t)R * spe, stream);
    pend_depth.alloc((size_t)R * spe, stream);
    pend_n.alloc((size_t)R * spe * 4, stream);
    if (cfg.eval_cache >= 0 && !tourney && !cfg.analyse) {
      pend_key.alloc((size_t)R * spe, stream);
      pend_src.alloc((size_t)R * spe, stream);
    }
    noise_raw.alloc((size_t)R * spe * CO_NUM_MOVES, stream);
    pend_path.alloc((size_t)R * spe * CO_PATH_MAX, stream);
    rng.alloc((size_t)R * CO_MT_N, stream);
    req.alloc((size_t)R * spe * CO_STATE_STRIDE, stream);
    req_offset.alloc((size_t)R + 1, stream);
    nn_in.alloc((size_t)R * spe * CO_STATE_STRIDE, stream);
    row_idx.alloc((size_t)R * spe, stream);
    nn_in70.alloc((size_t)R * spe * CO_GAME_STATE_SIZE, stream);
    ctl.alloc(CO_CTL_WORDS, stream);
    h_ctl.alloc(CO_CTL_WORDS);
    nn_eval.alloc((size_t)R * spe, stream);
    nn_probs.alloc((size_t)R * spe * CO_NUM_MOVES, stream);
    if (!cfg.testing) samples.alloc((size_t)G * CO_MAX_PLIES * CO_SAMPLE_FLOATS, stream); /* by game */
    if (cfg.trace) trace.alloc((size_t)G * CO_TRACE_CAP, stream);                            /* by game */
    if (recycle) {
      results.alloc(G, stream);
      seeds_dev.alloc(G, stream);
    }
    next_game.alloc(1, stream);
    all_done.alloc(1, stream);
    row_counter.alloc(1, stream);
    pack_counter.alloc((size_t)CO_PACK_STRIDE * CO_MAX_POOLS, stream); /* a 128-byte line per pool: every wavefront of a launch adds to its pool's words */
    work_counter.alloc((size_t)CO_WC_WORDS * CO_MAX_POOLS, stream);
    arena_state.alloc(CO_AS_WORDS, stream);
    if (tourney) {
      pcfg.alloc(host_pcfg.size(), stream);
      rt_h2d(pcfg.p, host_pcfg.data(), host_pcfg.size() * sizeof(PlayerCfg), stream);
      read_offset.alloc((size_t)R, stream);
    }

    /* (an analysis trainer is reset by set_positions, once the positions and their seeds are known) */
    if (!cfg.analyse) reset_games(cfg.seed);
    memset(&P, 0, sizeof P);
    fill_params(cap, cfg.total_games > 0 ? cfg.total_games : G);
    fused.work_counter = work_counter.p;
    fused.nn_eval = nn_eval.p;
    fused.nn_probs = nn_probs.p;
    fused.stats = &stats;
    fused.stream = stream;
  }

  /* Trainer::initialize (trainer.cpp:238-256): game i is seeded with the i-th
   * output of mt19937(seed), in global game order.  Also used to start a new
   * generation in the same pool (ca_trainer_reset). */
  void reset_games(int32_t seed) {
    cfg.seed = seed;
    size_t T = (size_t)2 * R;
    int total = cfg.total_games > 0 ? cfg.total_games : G;
    std::mt19937 gen((uint32_t)cfg.seed);
    std::vector<uint32_t> seeds(total);
    for (int i = 0; i < total; ++i) seeds[i] = (uint32_t)gen();
    std::vector<uint32_t> st((size_t)R * CO_MT_N);
    std::vector<GameCtl> hg(R);
    std::vector<TreeCtl> ht(T);
    for (int g = 0; g < R; ++g) { /* slot g starts with game g */
      uint32_t *x = &st[(size_t)g * CO_MT_N];
      x[0] = tourney ? match_seeds[g] : (cfg.analyse && !an_seed.empty()) ? an_seed[g] : seeds[cfg.game_base + g];
      for (int i = 1; i < CO_MT_N; ++i) x[i] = 1812433253u * (x[i - 1] ^ (x[i - 1] >> 30)) + (uint32_t)i;
      memset(&hg[g], 0, sizeof(GameCtl));
      hg[g].gid = g;
      hg[g].parity = (cfg.game_base + g) % 2;
      hg[g].rng_idx = CO_MT_N;
      hg[g].pos_meta = CO_META_START; /* Match::root_ = Node{} (match.h:91): the empty board */
      if (cfg.analyse && !an_pos.empty()) {
        hg[g].parity = 0;
        hg[g].pos_lo = an_pos[3 * g];
        hg[g].pos_hi = an_pos[3 * g + 1];
        hg[g].pos_meta = an_pos[3 * g + 2];
        if (an_pre[g]) hg[g].done = 1; /* choose_move.pyx:194-197: a terminal position is not searched */
      }
    }
    if (cfg.analyse && !an_pos.empty()) {
      /* result rows of the positions that were terminal as given */
      std::vector<uint32_t> rows((size_t)R * spe * CO_STATE_STRIDE, 0u);
      for (int g = 0; g < R; ++g)
        if (an_pre[g]) {
          uint32_t *o = &rows[(size_t)g * spe * CO_STATE_STRIDE];
          o[0] = 0xFFFFFFFFu;
          o[1] = (uint32_t)an_pre[g];
          o[2] = 1u;
          o[7] = 1u;
        }
      rt_h2d(req.p, rows.data(), rows.size() * 4, stream);
    }
    for (size_t t = 0; t < T; ++t) {
      ht[t].root = CO_NONE;
      ht[t].searches_done = 0;
      ht[t].units_used = 0;
      ht[t].peak_units = 0;
    }
    rt_h2d(rng.p, st.data(), st.size() * 4, stream);
    rt_h2d(games.p, hg.data(), hg.size() * sizeof(GameCtl), stream);
    rt_h2d(trees.p, ht.data(), ht.size() * sizeof(TreeCtl), stream);
    if (recycle) {
      /* the games behind the first R: their seeds (the Trainer stream in game order) and the counter they are taken from */
      rt_h2d(seeds_dev.p, seeds.data() + cfg.game_base, (size_t)G * 4, stream);
      rt_memset(results.p, 0, (size_t)G * sizeof(GameCtl), stream);
    }
    const unsigned long long first_unstarted = (unsigned long long)R;
    rt_h2d(next_game.p, &first_unstarted, 8, stream);
    rt_memset(row_counter.p, 0, 8, stream);
    rt_memset(pack_counter.p, 0, (size_t)8 * CO_PACK_STRIDE * CO_MAX_POOLS, stream);
    rt_memset(work_counter.p, 0, (size_t)8 * CO_WC_WORDS * CO_MAX_POOLS, stream);
    rt_memset(arena_state.p, 0, CO_AS_WORDS * 4, stream);
    rt_sync(stream);
    iterations = 0;
    trainer_iteration = 0;
    invalidate();
    last_total = 0;
    host_rows = 0;
    finished = false;
    const int64_t cache_clears = stats.cache_clears; /* (counted over the trainer's life) */
    stats = RunStats();
    stats.cache_clears = cache_clears;
    fused.cache_clean = false; /* the next run empties the tables before the first iteration of the new generation */
    callback.failed = false;
    for (auto &n : nets)
      if (n) n->clear_failure();
    if (logbuf.p) {
      rt_memset(logbuf.p, 0, (size_t)num_logged * CO_LOG_CAP * 4, stream);
      rt_sync(stream);
    }
    logs_written = false;
  }

  /* Trainer::initialize, trainer.cpp:243-250: the first num_logged games write `<log_folder>/game_<i>.txt` (i = the game's
   * index in the generation).  Before the first iteration only. */
  void set_logging(const char *folder, int n) {
    if (tourney || cfg.analyse) throw CaError(CA_ERR_STATE, "per-game logs belong to Trainer games (self-play or arena)");
    if (iterations != 0 || trainer_iteration != 0) throw CaError(CA_ERR_STATE, "ca_trainer_set_logging: the games have started");
    if (n < 0) throw CaError(CA_ERR_ARG, "ca_trainer_set_logging: num_logged < 0");
    n -= cfg.game_base; /* a shard logs the games of the generation's first num_logged that it owns */
    if (n < 0) n = 0;
    if (n > G) n = G;
    if (n > R) /* logged games start in their own slots (mcts.h): fewer slots than logged games would write fewer files than the reference */
      throw CaError(CA_ERR_ARG, "ca_trainer_set_logging: " + std::to_string(n) + " logged games on " + std::to_string(R) +
                                        " resident slots -- a logged game must start in its own slot; raise ca_config.resident");
    std::vector<int> games;
    std::vector<std::string> paths;
    for (int g = 0; g < n; ++g) {
      games.push_back(g);
      paths.push_back(std::string(folder ? folder : "") + "/game_" + std::to_string(cfg.game_base + g) + ".txt");
    }
    set_log_records(games, paths, false);
  }

  /* record k = game games[k], printed to paths[k]; with_index: the device finds a game's record through
   * EngineParams::log_index (tournament matches added with logging = true) instead of "the first num_logged games" */
  void set_log_records(const std::vector<int> &games, const std::vector<std::string> &paths, bool with_index) {
    log_game = games;
    log_paths = paths;
    num_logged = (int)games.size();
    if (num_logged > 0) {
      logbuf.alloc((size_t)num_logged * CO_LOG_CAP, stream);
      if (with_index) {
        std::vector<int32_t> idx((size_t)G, -1);
        for (int k = 0; k < num_logged; ++k) idx[(size_t)games[k]] = k;
        log_index.alloc((size_t)G, stream);
        rt_h2d(log_index.p, idx.data(), idx.size() * 4, stream);
      }
      rt_sync(stream);
    } else {
      logbuf.release();
      log_index.release();
    }
    P.log = logbuf.p;
    P.num_logged = num_logged;
    P.log_index = with_index ? log_index.p : nullptr;
    logs_written = false;
  }

  /* the files, once every game is over (the reference writes them as the games go; a file that cannot be opened is
   * skipped without a word there too: an ofstream in its fail state) */
  void maybe_write_logs() {
    if (!logbuf.p || logs_written) return;
    logs_written = true;
    fetch_games();
    std::vector<int32_t> rec((size_t)num_logged * CO_LOG_CAP);
    rt_d2h(rec.data(), logbuf.p, rec.size() * 4, stream);
    rt_sync(stream);
    for (int k = 0; k < num_logged; ++k) {
      const int32_t *r = rec.data() + (size_t)k * CO_LOG_CAP;
      if (r[0] < 0 || r[0] > CO_LOG_CAP - 1)
        throw CaError(CA_ERR_ENGINE, "text log " + log_paths[k] + " does not fit its record (" + std::to_string(r[0]) + " words)");
      FILE *f = fopen(log_paths[k].c_str(), "w");
      if (!f) continue;
      CoLogWriter wr(f);
      const bool ok = wr.write_game(r + 1, r[0], host_games[log_game[k]].result);
      fclose(f);
      if (!ok) throw CaError(CA_ERR_ENGINE, "malformed text-log record for " + log_paths[k]);
    }
  }

  void fill_params(uint32_t cap, int total) {
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
    size_t div = (size_t)total / (size_t)cfg.max_searches;
    if (div < 1) div = 1;
    /* the staggered start bounds the reference's memory (trainer.cpp:184-186); a recycling pool is bounded by its slots */
    P.stagger_div = (cfg.no_stagger || recycle) ? 0 : (int32_t)div;
    P.iteration = 0;
    P.to_play = -1;
    P.game_base = cfg.game_base;
    P.cap_units = cap;
    P.trace_on = cfg.trace;
    P.analyse = cfg.analyse;
    P.pcfg = tourney ? pcfg.p : nullptr;
    P.read_offset = tourney && !exact_offsets ? read_offset.p : nullptr; /* exact: co_step_row reads the writeRequests rows */
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
    P.log = logbuf.p;
    P.num_logged = num_logged;
    P.log_index = log_index.p;
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
#ifdef CO_PROF
    prof.alloc((size_t)R * CO_NPROF + 24 + CO_NPROF, stream);
    P.prof = prof.p;
#else
    P.prof = nullptr;
#endif
  }

  /* the engine parameters of one launch for model `to_play` (-1: every game) at the current iteration; the launch site
   * sets whatever else is its own (fused pools, the arena's device state, force_choose) on its copy */
  EngineParams params(int to_play) const {
    EngineParams e = P;
    e.to_play = to_play;
    e.iteration = trainer_iteration;
    return e;
  }

  /* h_ctl holds what a scan for model `to_play` wrote: the batch and the flags the host goes by */
  void read_ctl(int to_play) {
    last_total = h_ctl[CO_CTL_ROWS];
    finished = h_ctl[CO_CTL_ALL_DONE] != 0;
    any_error = h_ctl[CO_CTL_ANY_ERROR] != 0;
    scan_valid_for = to_play;
    scan_valid = true;
  }
  /* offsets + compact batch for model `to_play` (K4); ONE host synchronisation, on 16 bytes */
  void pack(int to_play) {
    if (scan_valid && scan_valid_for == to_play) return;
    const EngineParams e = params(to_play);
    RT_LAUNCH(co_k_scan, 1, CO_WAVE, stream, e);
    RT_LAUNCH(co_k_compact, R, CO_WAVE, stream, e);
    rt_d2h(h_ctl, ctl.p, CO_CTL_WORDS * 4, stream);
    rt_sync(stream);
    read_ctl(to_play);
    if (finished && !any_error) maybe_write_logs();
  }

  /* host_games[i] = control block of GAME i of this trainer: the slot itself without recycling; else the filed
   * result of a finished game, the slot of a game in play, or an untouched block for a game not yet started */
  void fetch_games() {
    if (host_games_valid) return;
    host_games.resize(G);
    if (!recycle) {
      rt_d2h(host_games.data(), games.p, (size_t)G * sizeof(GameCtl), stream);
      rt_sync(stream);
    } else {
      std::vector<GameCtl> slots(R);
      rt_d2h(slots.data(), games.p, (size_t)R * sizeof(GameCtl), stream);
      rt_d2h(host_games.data(), results.p, (size_t)G * sizeof(GameCtl), stream);
      rt_sync(stream);
      for (int i = 0; i < G; ++i)
        if (!host_games[i].done) {
          memset(&host_games[i], 0, sizeof(GameCtl));
          host_games[i].gid = i;
        }
      for (int sl = 0; sl < R; ++sl) {
        const int i = slots[sl].gid;
        if (i >= 0 && i < G && !host_games[i].done) host_games[i] = slots[sl];
      }
    }
    host_games_valid = true;
  }

  void check_errors() {
    check_net_range();
    if (scan_valid && !any_error) return; /* the last scan saw no error bit in any game */
    fetch_games();
    for (int g = 0; g < G; ++g) {
      if (host_games[g].error) {
        char buf[256];
        int e = host_games[g].error;
        snprintf(buf, sizeof buf, "game %d reported engine error 0x%x (%s%s%s%s)", g, e,
                 (e & CO_ERR_ARENA_FULL) ? "search-tree arena full: raise ca_config.arena_units; " : "",
                 (e & CO_ERR_PATH_TOO_DEEP) ? "search path deeper than CO_PATH_MAX; " : "",
                 (e & CO_ERR_TOO_MANY_PLIES) ? "game longer than CO_MAX_PLIES; " : "",
                 (e & CO_ERR_INTERNAL) ? "internal inconsistency; " : "");
        throw CaError(CA_ERR_ENGINE, buf);
      }
    }
  }

  /* one launch of the search kernel on every slot, and what the host has to know afterwards: the batch of model
   * e.to_play and the games' error bits */
  void step(const EngineParams &e) {
    launch_mcts_step(e, R, stream);
    ++stats.mcts_launches;
    invalidate();
    pack(e.to_play);
    check_errors();
  }

  /* Trainer::doIteration (trainer.cpp:164-236), compat protocol */
  void need_positions() const {
    if (cfg.analyse && an_pos.empty()) throw CaError(CA_ERR_STATE, "analysis trainer: ca_trainer_set_positions first");
  }
  bool do_iteration(const float *evals, const float *probs, int to_play) {
    need_positions();
    callback.need_none_failed("ca_trainer_do_iteration");
    if (host_cache) return host_cache_iteration(evals, probs, to_play);
    if (iterations > 0) {
      pack(to_play); /* offsets the reference computes at entry */
      if (last_total > 0) {
        if (!evals || !probs) throw CaError(CA_ERR_ARG, "doIteration: null evaluations/probabilities");
        rt_h2d(nn_eval.p, evals, (size_t)last_total * 4, stream);
        rt_h2d(nn_probs.p, probs, (size_t)last_total * CO_NUM_MOVES * 4, stream);
      }
    } else {
      rt_memset(req_offset.p, 0, ((size_t)R + 1) * 4, stream);
    }
    const EngineParams e = params(to_play);
    if (to_play == -1) ++trainer_iteration;
    ++iterations;
    step(e);
    return finished;
  }

  /* the requests of model `to_play` (-1: every game; a tournament's model id) */
  int32_t num_requests(int to_play) {
    if (host_cache) return host_cache_all_games(to_play), host_rows;
    pack(to_play);
    return last_total;
  }

  void write_requests(float *out, int to_play) {
    const int32_t n = num_requests(to_play);
    if (n == 0) return;
    /* K4 (with the evaluation cache: HostNet::forward, and the iteration's run has drained) has laid the rows out as the
     * caller's array holds them: one copy, straight into it */
    rt_d2h(out, nn_in70.p, (size_t)n * CO_GAME_STATE_SIZE * 4, stream);
    rt_sync(stream);
  }

  /* ---- the host-driven protocol with the evaluation cache ---- */
  /* log2_entries < 0 off, 0 a table sized automatically, 6..30 2^n entries; at a generation boundary only */
  void set_host_cache(int32_t log2_entries) {
    if ((log2_entries >= 1 && log2_entries <= 5) || log2_entries > 30)
      throw CaError(CA_ERR_ARG, "ca_trainer_set_host_cache: log2_entries must be negative (off), 0 (automatic) or 6..30, not " +
                                        std::to_string(log2_entries));
    const bool on = log2_entries >= 0;
    if (on && !self_play_training()) /* (as use_cache(): the table's keys are positions that self-play reached) */
      throw CaError(CA_ERR_STATE, "ca_trainer_set_host_cache: the evaluation cache serves self-play training only, not a testing, "
                                  "analysis or tournament trainer");
    if (!on && !host_cache) return;
    if (iterations != 0)
      throw CaError(CA_ERR_STATE, "ca_trainer_set_host_cache: in the middle of a generation; switch before the first "
                                  "ca_trainer_do_iteration or after ca_trainer_reset");
    /* the pool and its table are built for this mode (and, switched off, rebuilt by the next ca_trainer_run for its own) */
    fused.release();
    host_cache = on;
    host_cache_log2 = log2_entries;
    fused.host_stepped = on;
    host_rows = 0;
    if (!on) return;
    if (!pend_key.p) { /* (a trainer created with ca_config.eval_cache < 0 has none yet) */
      pend_key.alloc((size_t)R * spe, stream);
      pend_src.alloc((size_t)R * spe, stream);
      P.pend_key = pend_key.p;
      P.pend_src = pend_src.p;
      rt_sync(stream);
    }
    fused.spe = spe;
    fused.create(1, R, log2_entries);
    fused.cache_clean = false; /* (the first iteration starts the generation: counters cleared with the table) */
    /* the caller's rows and answers pass through the plain protocol's own staging arrays, which this mode leaves idle */
    host_net.rows_cap = (size_t)R * spe;
    host_net.rows70 = nn_in70.p;
    host_net.ev_in = nn_eval.p;
    host_net.pr_in = nn_probs.p;
    host_net.d_ctl = ctl.p;
    host_net.h_ctl = &h_ctl[0];
    host_net.out_idx = nullptr;
  }
  void host_cache_all_games(int to_play) const {
    if (to_play != -1) throw CaError(CA_ERR_ARG, "host-driven protocol with the evaluation cache: to_play must be -1 (training)");
  }
  /* Trainer::doIteration with the cache: the answers to the rows handed out go where a network kernel would have written
   * them, then one iteration of fused training on one pool -- the search launch resolves its request rows against the
   * table and HostNet gathers the ones left over.  No step budget and no deferred hand-over: either would add round trips. */
  bool host_cache_iteration(const float *evals, const float *probs, int to_play) {
    host_cache_all_games(to_play);
    rt_stream_t st = fused.pools[0].st;
    if (host_rows > 0) {
      if (!evals || !probs) throw CaError(CA_ERR_ARG, "doIteration: null evaluations/probabilities");
      host_net.receive(evals, probs, host_rows, st);
      host_rows = 0;
    }
    EngineParams e = params(-1);
    e.step_budget = 0;
    e.step_budget_k16 = 0;
    host_net.scan_params = e;
    const int64_t n = fused.run(e, &host_net, 1, host_cache_log2, iterations > 0, 1);
    trainer_iteration += (int32_t)n;
    iterations += n;
    invalidate();
    stats.estimate_device_times(true);
    if (!fused.failure.empty()) throw CaError(CA_ERR_ENGINE, fused.failure);
    /* what the run's drain has brought: the protocol's flags and the pool's words of this iteration */
    read_ctl(-1);
    const Pool::Seen &seen = fused.pools[0].seen[0]; /* (one iteration: the window of parity 0) */
    host_rows = (int32_t)std::min<size_t>(seen.evaluated, (size_t)R * spe);
    stats.nn_rows += (int64_t)co_pack_rows(seen.pack); /* rows the games requested */
    stats.nn_rows_evaluated += host_rows;                   /* ... and the ones the caller gets */
    check_errors();
    if (finished) maybe_write_logs();
    return finished;
  }

  /* ---- Tourney (tourney.cpp) on the same pool: one match per game slot ---- */
  /* Tourney::doIteration (tourney.cpp:53-70).  `rows` = rows of the caller's two arrays: the
   * reference reads them at its own offset table (quirk 10), so the whole arrays travel. */
  void tourney_do_iteration(const float *evals, const float *probs, int32_t rows, int id) {
    size_t cap = (size_t)R * spe;
    if (rows < 0 || (size_t)rows > cap) rows = (int32_t)cap;
    const EngineParams e = params(id);
    RT_LAUNCH(co_k_scan, 1, CO_WAVE, stream, e); /* offsets at entry */
    if (rows > 0 && evals && probs) {
      rt_h2d(nn_eval.p, evals, (size_t)rows * 4, stream);
      rt_h2d(nn_probs.p, probs, (size_t)rows * CO_NUM_MOVES * 4, stream);
    }
    ++iterations;
    step(e);
  }
  bool tourney_all_done() {
    fetch_games();
    for (int g = 0; g < G; ++g)
      if (!host_games[g].done) return false;
    return true;
  }
  /* one round of ca_tourney::run for model `id`: its requests packed (Tourney::writeRequests), evaluated by `net`, its
   * matches iterated (Tourney::doIteration); a random player's dummy id (< 0) has nothing to evaluate */
  void tourney_round(int id, CoNet *net) {
    const EngineParams e = params(id);
    RT_LAUNCH(co_k_scan, 1, CO_WAVE, stream, e); /* offsets + batch of model `id` */
    if (id >= 0) {
      RT_LAUNCH(co_k_compact, G, CO_WAVE, stream, e);
      net->forward(nn_in.p, G * spe, req_offset.p + G, nn_eval.p, nn_probs.p, stream);
      ++stats.nn_launches;
    }
    launch_mcts_step(e, G, stream);
    ++stats.mcts_launches;
    ++iterations;
  }
  /* the all-done flag, refreshed by a scan for model `id` */
  bool tourney_poll_done(int id) {
    RT_LAUNCH(co_k_scan, 1, CO_WAVE, stream, params(id));
    int32_t d = 0;
    rt_d2h(&d, all_done.p, 4, stream);
    rt_sync(stream);
    return d != 0;
  }
  /* everything queued on the trainer's stream has run; what the host knew of the games is stale */
  void drain() {
    rt_sync(stream);
    invalidate();
  }
  /* ca_tourney::run is over: the rounds were queued without a look at the games */
  void tourney_rounds_done() {
    invalidate();
    check_errors();
  }
  int32_t num_samples() {
    fetch_games();
    int32_t n = 0;
    for (int g = 0; g < G; ++g) n += host_games[g].n_samples;
    return n;
  }

  /* SelfPlayer::score (selfplayer.cpp:57-64) + Trainer::score (trainer.cpp:59-68) */
  static float game_score(const GameCtl &gc) {
    if (gc.result == CO_RESULT_LOSS) return 0.0f;
    if (gc.result == CO_RESULT_WIN) return 1.0f;
    return 0.5f;
  }
  float score() {
    fetch_games();
    /* colour alternates with the GLOBAL game index (trainer.cpp:61-66) */
    float s = 0;
    for (int g = 0; g < G; ++g)
      if ((cfg.game_base + g) % 2 == 0) s += game_score(host_games[g]);
    for (int g = 0; g < G; ++g)
      if ((cfg.game_base + g) % 2 == 1) s = (float)((double)s + (1.0 - (double)game_score(host_games[g])));
    return s / (float)(size_t)G;
  }
  float avg_mate_length() {
    fetch_games();
    int32_t total = 0;
    for (int g = 0; g < G; ++g) {
      const GameCtl &gc = host_games[g];
      total += gc.mate_turn == 0 ? 0 : gc.n_samples - gc.mate_turn + 1; /* selfplayer.cpp:66-71 */
    }
    return (float)total / (float)(size_t)G;
  }

  /* ws_off = {sample offsets [G + 1], per game (plies | result << 8) [G]}: the sample kernels work by game, not by slot.
   * Returns the number of samples; nothing is uploaded when there are none or more than `cap_rows`. */
  int32_t upload_sample_index(int32_t cap_rows) {
    fetch_games();
    std::vector<int32_t> idx((size_t)2 * G + 1, 0);
    for (int g = 0; g < G; ++g) {
      idx[g + 1] = idx[g] + host_games[g].n_samples;
      idx[(size_t)G + 1 + g] = host_games[g].n_samples | (host_games[g].result << 8);
    }
    if (idx[G] == 0 || idx[G] > cap_rows) return idx[G];
    ensure(ws_off, idx.size());
    rt_h2d(ws_off.p, idx.data(), idx.size() * 4, stream);
    rt_sync(stream); /* idx is a local */
    return idx[G];
  }

  /* the guard of the three ways samples leave (`what` names the one): their number, the index of them uploaded */
  int32_t need_samples(const char *what, int32_t cap_rows = INT32_MAX) {
    if (cfg.testing) throw CaError(CA_ERR_STATE, std::string(what) + " in testing mode");
    return upload_sample_index(cap_rows);
  }
  const int32_t *ws_meta() const { return ws_off.p + G + 1; }

  void write_samples(float *gs, float *ev, float *pr) {
    const size_t n = (size_t)need_samples("writeSamples");
    if (n == 0) return;
    ensure(ws_gs, n * 8 * CO_GAME_STATE_SIZE);
    ensure(ws_ev, n * 8);
    ensure(ws_pr, n * 8 * CO_NUM_MOVES);
    RT_LAUNCH(co_k_write_samples, G, CO_WAVE, stream, P, G, (const int32_t *)ws_off.p, ws_meta(), ws_gs.p, ws_ev.p, ws_pr.p);
    rt_d2h(gs, ws_gs.p, n * 8 * CO_GAME_STATE_SIZE * 4, stream);
    rt_d2h(ev, ws_ev.p, n * 8 * 4, stream);
    rt_d2h(pr, ws_pr.p, n * 8 * CO_NUM_MOVES * 4, stream);
    rt_sync(stream);
  }

  /* un-augmented samples packed on the device into device memory: the caller's (the multi-GPU gather hands these
   * straight to RCCL), or export_samples' staging buffers */
  void pack_samples(float *d_state_policy, float *d_outcome) {
    RT_LAUNCH(co_k_pack_samples, G, CO_WAVE, stream, P, G, (const int32_t *)ws_off.p, ws_meta(), d_state_policy, d_outcome);
  }
  int32_t pack_samples_device(float *d_state_policy, float *d_outcome, int32_t cap_rows) {
    const int32_t n = need_samples("pack_samples", cap_rows);
    if (n > cap_rows) throw CaError(CA_ERR_ARG, "pack_samples: destination too small");
    if (n > 0) pack_samples(d_state_policy, d_outcome);
    rt_sync(stream);
    return n;
  }
  void export_samples(float *state_policy, float *outcome) {
    const size_t n = (size_t)need_samples("export_samples");
    if (n == 0) return;
    ensure(ws_gs, n * CO_SAMPLE_FLOATS);
    ensure(ws_ev, n);
    pack_samples(ws_gs.p, ws_ev.p);
    rt_d2h(state_policy, ws_gs.p, n * CO_SAMPLE_FLOATS * 4, stream);
    rt_d2h(outcome, ws_ev.p, n * 4, stream);
    rt_sync(stream);
  }

  /* Trainer::writeScores (trainer.cpp:115-162) */
  void write_scores(const char *file) {
    fetch_games();
    size_t n = (size_t)G;
    std::vector<float> scores(n);
    for (size_t i = 0; i < n; i += 2) scores[i] = game_score(host_games[i]);
    for (size_t i = 1; i < n; i += 2) scores[i] = (float)(1.0 - (double)game_score(host_games[i]));
    FILE *f = fopen(file, "w");
    if (!f) throw CaError(CA_ERR_IO, std::string("cannot open ") + file);
    const char *who[2] = {"First", "Second"};
    for (int side = 0; side < 2; ++side) {
      int wins = 0, draws = 0;
      for (size_t i = side; i < n; i += 2) {
        if (scores[i] == 1.0f) ++wins;
        else if (scores[i] == 0.5f) ++draws;
      }
      size_t half = n / 2;
      auto ratio = [&](size_t k) { return (double)((float)k / (float)half); };
      fprintf(f, "%s player wins: %d / %zu = %g\n", who[side], wins, half, ratio(wins));
      fprintf(f, "%s player draws: %d / %zu = %g\n", who[side], draws, half, ratio(draws));
      fprintf(f, "%s player losses: %zu / %zu = %g\n", who[side], half - wins - draws, half, ratio(half - wins - draws));
    }
    fclose(f);
  }

  /* ------------------------------------------------------------ analysis mode (DockerMC) */
  void set_positions(const int32_t *boards, const int32_t *to_play, const int32_t *pieces, const int32_t *seeds) {
    if (!cfg.analyse) throw CaError(CA_ERR_STATE, "set_positions: not an analysis trainer (ca_config.analyse)");
    if (iterations > 0) throw CaError(CA_ERR_STATE, "set_positions after the first iteration");
    an_pos.assign((size_t)3 * G, 0u);
    an_seed.assign(G, 0u);
    an_pre.assign(G, 0);
    std::vector<uint64_t> hb(G);
    std::vector<uint32_t> hm(G);
    for (int g = 0; g < G; ++g) {
      uint64_t b = 0;
      for (int i = 0; i < 64; ++i) {
        int v = boards[(size_t)g * 64 + i];
        if (v != 0 && v != 1) throw CaError(CA_ERR_ARG, "set_positions: board entries must be 0 or 1");
        if (v) b |= 1ull << i;
      }
      uint32_t meta = 0;
      for (int i = 0; i < 6; ++i) {
        int pc = pieces[(size_t)g * 6 + i];
        if (pc < 0 || pc > 4) throw CaError(CA_ERR_ARG, "set_positions: piece counts must be 0..4");
        meta |= (uint32_t)pc << (3 * i);
      }
      if (to_play[g] != 0 && to_play[g] != 1) throw CaError(CA_ERR_ARG, "set_positions: to_play must be 0 or 1");
      meta |= (uint32_t)to_play[g] << 18;
      an_pos[3 * g] = (uint32_t)b;
      an_pos[3 * g + 1] = (uint32_t)(b >> 32);
      an_pos[3 * g + 2] = meta;
      an_seed[g] = (uint32_t)seeds[g];
      hb[g] = b;
      hm[g] = meta;
    }
    /* Node result of every given position (node.cpp:256-271), by the rule kernel */
    DevBuf<uint64_t> db;
    DevBuf<uint32_t> dm, dk;
    DevBuf<int32_t> dl;
    db.upload(hb.data(), G, stream); dm.upload(hm.data(), G, stream); dk.alloc((size_t)G * 3, stream); dl.alloc(G, stream);
    RT_LAUNCH(co_k_rules_batch, G, CO_WAVE, stream, (const uint64_t *)db.p, (const uint32_t *)dm.p, G, dk.p, dl.p);
    std::vector<uint32_t> mk((size_t)G * 3);
    std::vector<int32_t> ln(G);
    rt_d2h(mk.data(), dk.p, mk.size() * 4, stream);
    rt_d2h(ln.data(), dl.p, ln.size() * 4, stream);
    rt_sync(stream);
    for (int g = 0; g < G; ++g)
      if ((mk[3 * g] | mk[3 * g + 1] | mk[3 * g + 2]) == 0u) an_pre[g] = ln[g] ? CO_RESULT_LOSS : CO_RESULT_DRAW;
    reset_games(cfg.seed);
  }

  void analysis(int32_t *out) {
    if (!cfg.analyse) throw CaError(CA_ERR_STATE, "not an analysis trainer");
    /* the eight result words at the head of each slot's request area (mcts.h co_analyse_finish): one strided copy */
    std::vector<uint32_t> rows((size_t)G * 8);
    rt_d2h_2d(rows.data(), 32, req.p, (size_t)spe * CO_STATE_STRIDE * 4, 32, (size_t)G, stream);
    rt_sync(stream);
    fetch_games();
    for (int g = 0; g < G; ++g) {
      const uint32_t *r = &rows[(size_t)g * 8];
      int32_t *o = out + (size_t)g * 8;
      if (!host_games[g].done || r[7] != 1u) throw CaError(CA_ERR_STATE, "analysis: search of position " + std::to_string(g) + " is not finished");
      const int res = (int)r[1];
      o[0] = (int32_t)r[0];
      o[1] = res == CO_RESULT_LOSS || res == CO_RESULT_DRAW;   /* Node::terminal, node.cpp:96-98 */
      o[2] = res == CO_RESULT_DRAW || res == CO_DEDUCED_DRAW;  /* Node::drawn */
      o[3] = (int32_t)r[2];
      o[4] = (int32_t)r[3];
      o[5] = (int32_t)r[4];
      o[6] = (int32_t)r[5];
      o[7] = (int32_t)r[6];
    }
  }

  /* DockerMC::chooseMove on searches that have not ended (the reference's loop leaves on a time limit,
   * choose_move.pyx:110-117, and then calls chooseMove unconditionally, :199): every unfinished position
   * chooses on its tree as it stands; evaluations still pending are never received (trainmc.cpp:110-137 does
   * not look at searched_).  Before the first iteration the root is created first, as the constructor does. */
  void finish_analysis() {
    if (!cfg.analyse) throw CaError(CA_ERR_STATE, "ca_trainer_finish: not an analysis trainer");
    if (iterations == 0) do_iteration(nullptr, nullptr, -1);
    EngineParams e = params(-1);
    e.force_choose = 1;
    step(e);
  }

  /* ------------------------------------------------------------ fused mode */
  /* the network `spec` names as slot `slot` (net_host.h NetSpec: weights of a kind, or the caller's own function) */
  void set_net(int slot, const NetSpec &spec, const char *who) {
    if (slot < 0 || slot > 1) throw CaError(CA_ERR_ARG, "net slot must be 0 or 1");
    install_net(slot, spec.make((size_t)R * spe, stream, &callback, ", this trainer", " (ca_trainer_request_rows)"), who);
  }

  /* a new network takes its slot */
  void install_net(int slot, std::unique_ptr<CoNet> fresh, const char *who) {
    if (slot == 0 && !fused.pools.empty() && !host_cache) { /* (host_cache: the pool and its table are that mode's, whatever the network) */
      /* Does the new network change whether fused training keeps an evaluation cache?  The tables are part of the
       * pools, and in the middle of a generation the pending leaves point into them (pend_src): refuse that. */
      std::unique_ptr<CoNet> old = std::move(nets[0]);
      nets[0] = std::move(fresh);
      const bool toggles = (fused.table.entries != 0) != use_cache();
      if (toggles && iterations > 0 && !finished) {
        nets[0] = std::move(old);
        throw CaError(CA_ERR_STATE, std::string(who) + ": this network turns the evaluation cache " +
                                            std::string(fused.table.entries ? "off" : "on") +
                                            " in the middle of a generation; finish or reset the generation first");
      }
      if (toggles) fused.release(); /* rebuilt with / without the table */
    } else {
      nets[slot] = std::move(fresh);
    }
    /* entries filled by the previous network must not serve the new one: the next run empties the tables (the value
     * elements the pending leaves point to stay: those rows WERE evaluated by the network in place when they were queued) */
    if (slot == 0) fused.cache_clean = false;
  }

  /* A caller-supplied network function returned non-zero (ExternalNet): the run that saw it has left through its drain;
   * the games hold evaluations that were never written, so the generation is over until ca_trainer_reset. */
  void check_callback() {
    for (int slot = 0; slot < 2; ++slot)
      if (nets[slot] && nets[slot]->callback_failed()) invalidate(), callback.check(nets[slot].get(), "slot " + std::to_string(slot));
  }

  void check_net_range() {
    if (!net_used) return; /* (no copy and stream wait per slot when nothing ran) */
    /* the device flag is sticky for the life of the network object: net_used is cleared only when every slot is clean, so
     * that every later check (export, score, write samples) raises again until set_net replaces the slot */
    for (int slot = 0; slot < 2; ++slot) ::check_net_range(nets[slot].get(), stream, "network slot " + std::to_string(slot));
    net_used = false;
  }

  /* host rows in, host results out (ca_trainer_net_forward): persistent device buffers; the rows travel as
   * the caller holds them (70 floats) and are widened to the kernels' 80-float rows on the device */
  void net_forward_host(int slot, const float *states, int32_t n, float *evals, float *probs) {
    if (slot < 0 || slot > 1 || !nets[slot]) throw CaError(CA_ERR_STATE, "net slot not set");
    callback.need_none_failed("ca_trainer_net_forward");
    CoNet *net = nets[slot].get();
    if (n < 0 || (size_t)n > net->max_rows()) throw CaError(CA_ERR_ARG, "net_forward: more rows than num_games*searches_per_eval");
    if (n == 0) return;
    ensure(fw_in70, (size_t)n * CO_GAME_STATE_SIZE);
    ensure(fw_in, (size_t)n * CO_STATE_STRIDE);
    ensure(fw_ev, (size_t)n);
    ensure(fw_pr, (size_t)n * CO_NUM_MOVES);
    ensure(fw_rows, 1);
    rt_h2d(fw_in70.p, states, (size_t)n * CO_GAME_STATE_SIZE * 4, stream);
    rt_h2d(fw_rows.p, &n, 4, stream);
    expand_rows(fw_in70.p, fw_in.p, n, stream);
    net_used = true;
    net->forward(fw_in.p, n, fw_rows.p, fw_ev.p, fw_pr.p, stream);
    if (net->callback_failed()) {
      rt_sync(stream);
      check_callback();
    }
    rt_d2h(evals, fw_ev.p, (size_t)n * 4, stream);
    rt_d2h(probs, fw_pr.p, (size_t)n * CO_NUM_MOVES * 4, stream);
    rt_sync(stream);
    check_net_range();
  }

  /* kernel-only timing of a network on `rows` resident rows (HIP events on the engine's stream);
   * diagnostics and the per-kernel roofline of bench.py */
  float net_bench(int slot, const float *states, int32_t rows, int32_t reps) {
    if (slot < 0 || slot > 1 || !nets[slot]) throw CaError(CA_ERR_STATE, "net slot not set");
    if ((size_t)rows > std::min(nets[slot]->max_rows(), (size_t)R * spe)) throw CaError(CA_ERR_ARG, "net_bench: too many rows");
    DevBuf<int32_t> d_n;
    d_n.alloc(1, stream);
    ensure(fw_in70, (size_t)rows * CO_GAME_STATE_SIZE); /* (not nn_in70: the protocols hand that one to the caller) */
    rt_h2d(fw_in70.p, states, (size_t)rows * CO_GAME_STATE_SIZE * 4, stream);
    rt_h2d(d_n.p, &rows, 4, stream);
    expand_rows(fw_in70.p, nn_in.p, rows, stream);
    net_used = true;
    nets[slot]->forward(nn_in.p, rows, d_n.p, nn_eval.p, nn_probs.p, stream); /* warm */
    Event e0, e1;
    e0.create();
    e1.create();
    rt_event_record(e0, stream);
    for (int i = 0; i < reps; ++i) nets[slot]->forward(nn_in.p, rows, d_n.p, nn_eval.p, nn_probs.p, stream);
    rt_event_record(e1, stream);
    rt_sync(stream);
    return rt_event_elapsed_ms(e0, e1) / (float)reps;
  }

  /* diagnostic builds (-DCO_PROF): summed in-kernel cycle stamps, see mcts.h */
  void read_prof(unsigned long long out[2 * CO_NPROF + 24]) {
    /* nothing is written to `out` unless this is a stamped build: a caller of the shipped library with a buffer sized for
     * an earlier round's layout gets the error, not an overflow */
    if (!prof.p) throw CaError(CA_ERR_STATE, "not a -DCO_PROF build");
    for (int i = 0; i < 2 * CO_NPROF + 24; ++i) out[i] = 0;
    std::vector<unsigned long long> h((size_t)R * CO_NPROF);
    rt_d2h(h.data(), prof.p, h.size() * 8, stream);
    rt_sync(stream);
    for (int g = 0; g < R; ++g)
      for (int i = 0; i < CO_NPROF; ++i) out[i] += h[(size_t)g * CO_NPROF + i];
    /* [CO_NPROF ..): clocks, the histogram of wave-step times, then the phase sums of the slow wave-steps alone */
    rt_d2h(out + CO_NPROF, prof.p + (size_t)R * CO_NPROF, (size_t)(24 + CO_NPROF) * 8, stream);
    rt_sync(stream);
  }

  void read_stats(ca_stats *out) {
    fetch_games();
    memset(out, 0, sizeof *out);
    for (int g = 0; g < G; ++g) {
      out->searches += host_games[g].searches;
      out->evals += host_games[g].evals;
      out->nodes += host_games[g].nodes;
      out->plies += host_games[g].plies;
    }
    std::vector<TreeCtl> ht((size_t)2 * R);
    rt_d2h(ht.data(), trees.p, ht.size() * sizeof(TreeCtl), stream);
    rt_sync(stream);
    for (auto &x : ht) out->peak_arena_units = std::max<int64_t>(out->peak_arena_units, x.peak_units);
    out->iterations = iterations;
    out->mcts_ms = stats.mcts_ms;
    out->nn_ms = stats.nn_ms;
    out->pack_ms = stats.pack_ms;
    out->mcts_launches = stats.mcts_launches;
    out->nn_launches = stats.nn_launches;
    out->nn_rows = stats.nn_rows;
    out->pools = fused.pools.empty() ? 1 : (int64_t)fused.pools.size();
    out->resident_slots = R;
    out->nn_rows_evaluated = stats.nn_rows_evaluated;
    out->steps_cut = stats.steps_cut;
    out->step_budget_last = stats.step_budget_last;
    out->timed_launches = stats.timed_launches;
    out->nn_timed_rows = stats.nn_timed_rows;
    out->mcts_timed_ms = stats.mcts_timed_ms;
    out->nn_timed_ms = stats.nn_timed_ms;
  }

  /* the control block of game (or match) `game`, as the device holds it now */
  const GameCtl &game(int game, const char *what = "game index out of range") {
    if (game < 0 || game >= G) throw CaError(CA_ERR_ARG, what);
    fetch_games();
    return host_games[game];
  }
  /* out[8] = {side to move, done, result, samples, pending requests, error, mate turn, plies} */
  void game_info(int g, int32_t out[8]) {
    const GameCtl &gc = game(g);
    out[0] = gc.to_play; out[1] = gc.done; out[2] = gc.result; out[3] = gc.n_samples;
    out[4] = gc.done ? 0 : gc.n_pending; out[5] = gc.error; out[6] = gc.mate_turn; out[7] = gc.plies;
  }

  void read_trace(int g, int32_t *out, int32_t cap, int32_t *n) {
    if (!cfg.trace) throw CaError(CA_ERR_STATE, "trace not enabled");
    int32_t len = game(g).trace_len;
    if (len > CO_TRACE_CAP) throw CaError(CA_ERR_ENGINE, "trace buffer overflow");
    *n = len;
    int32_t c = std::min(len, cap);
    if (out && c > 0) {
      rt_d2h(out, trace.p + (size_t)g * CO_TRACE_CAP, (size_t)c * 4, stream);
      rt_sync(stream);
    }
  }

  /* fused training (or N position searches) in `npools` pools: the run is FusedRun's (pools.h); what it leaves is read here */
  bool run_pools(int64_t max_iterations, int npools) {
    net_used = true;
    const int64_t n = fused.run(params(-1), nets[0].get(), npools, use_cache() ? cfg.eval_cache : -1, iterations > 0, max_iterations);
    trainer_iteration += (int32_t)n;
    iterations += n;
    invalidate();
    /* the run is over (its streams are drained): device times from the timed launches, errors, the rows evaluated, the
     * step budget's statistics */
    stats.estimate_device_times(true);
    check_callback();
    if (!fused.failure.empty()) throw CaError(CA_ERR_ENGINE, fused.failure);
    pack(-1); /* refresh the done flag and the batch description */
    check_errors();
    fetch_games();
    stats.nn_rows = 0;
    for (int g = 0; g < G; ++g) stats.nn_rows += host_games[g].evals; /* every consumed row was requested once */
    stats.nn_rows_evaluated = use_cache() ? fused.rows_evaluated() : stats.nn_rows;
    fused.budget_stats();
    return finished;
  }

  bool run(int64_t max_iterations) {
    need_positions();
    callback.need_none_failed("ca_trainer_run");
    if (host_cache)
      throw CaError(CA_ERR_STATE, "ca_trainer_run: the host-driven protocol drives this trainer's generations with the evaluation "
                                  "cache; switch it off first (ca_trainer_set_host_cache with a negative size)");
    if (!nets[0]) throw CaError(CA_ERR_STATE, "ca_trainer_run: no network set (ca_trainer_set_net)");
    if (cfg.testing && !cfg.analyse && !nets[1]) throw CaError(CA_ERR_STATE, "arena mode needs both networks");
    if (!cfg.testing || cfg.analyse) { /* one network, every slot active: self-play training, or N position searches */
      /* automatic: three pools from 3072 resident games on (round 5, one box, same library, 4096 games x 400: rescnn4 f16x3
       * 417.9 -> 407.6 ms per generation, mlp12x100 f16x3 145.4 -> 138.3 -- with the grouped search a pool's search launch is
       * short enough for a third pool to fit under the other two's network launches), two from 2048, else one */
      int npools = cfg.pools > 0 ? cfg.pools : (R >= 3072 ? 3 : R >= 2048 ? 2 : 1);
      if (npools > CO_MAX_POOLS) npools = CO_MAX_POOLS;
      if (npools > R) npools = R;
      return run_pools(max_iterations, npools);
    }
    return run_arena(max_iterations);
  }

  /* arena (main.pyx:142-168 with is_testing): one model is served per iteration and hands over
   * when its batch comes back empty.  The model to move lives on the device (arena_state, kept
   * by the two scans of an iteration), both networks are queued every iteration and the idle
   * one finds a row count of zero, so the host only looks every eighth iteration.  Requests
   * are packed by K4 in game order (the reference's request order). */
  bool run_arena(int64_t max_iterations) {
    const int poll = 8;
    Event ev[4];
    for (auto &e : ev) e.create();
    EngineParams e = params(0);
    e.arena_state = arena_state.p;
    e.row_counter = row_counter.p;
    int64_t it = 0;
    int32_t st[CO_AS_WORDS] = {};
    std::string failure;
    while (!finished && (max_iterations <= 0 || it < max_iterations)) {
      const bool timed = (it % poll) == poll - 1 || (max_iterations > 0 && it + 1 == max_iterations);
      e.iteration = trainer_iteration;
      e.scan_phase = 0;
      RT_LAUNCH(co_k_scan, 1, CO_WAVE, stream, e); /* offsets at entry (trainer.cpp:208-215) */
      if (timed) rt_event_record(ev[0], stream);
      launch_mcts_step(e, R, stream);
      if (timed) rt_event_record(ev[1], stream);
      e.scan_phase = 1;
      RT_LAUNCH(co_k_scan, 1, CO_WAVE, stream, e);
      RT_LAUNCH(co_k_compact, R, CO_WAVE, stream, e);
      if (timed) rt_event_record(ev[2], stream);
      net_used = true;
      for (int slot = 0; slot < 2; ++slot) /* get_predictions, main.pyx:74-81 */
        nets[slot]->forward(nn_in.p, R * spe, arena_state.p + CO_AS_ROWS + slot, nn_eval.p, nn_probs.p, stream);
      if (nets[0]->callback_failed() || nets[1]->callback_failed()) break; /* (a caller-supplied network: nothing more is queued) */
      if (timed) rt_event_record(ev[3], stream);
      ++iterations;
      ++it;
      ++stats.mcts_launches;
      ++stats.nn_launches;
      if (timed) {
        int32_t d = 0;
        rt_d2h(&d, all_done.p, 4, stream);
        rt_d2h(st, arena_state.p, sizeof st, stream);
        rt_sync(stream);
        finished = d != 0;
        stats.mcts_timed_ms += rt_event_elapsed_ms(ev[0], ev[1]);
        stats.nn_timed_ms += rt_event_elapsed_ms(ev[2], ev[3]);
        stats.pack_ms += rt_event_elapsed_ms(ev[1], ev[2]) * poll;
        stats.nn_timed_rows += st[CO_AS_ROWS] + st[CO_AS_ROWS + 1];
        ++stats.timed_launches;
        if (!finished && st[CO_AS_EMPTY] > 4) {
          failure = "arena: no model has requests";
          break;
        }
      }
    }
    rt_sync(stream);
    rt_d2h(st, arena_state.p, sizeof st, stream);
    rt_sync(stream);
    invalidate();
    stats.estimate_device_times(false);
    check_callback();
    if (!failure.empty()) throw CaError(CA_ERR_ENGINE, failure);
    pack(st[CO_AS_MODEL]); /* refresh the done flag and the batch description */
    check_errors();
    unsigned long long rows = 0;
    rt_d2h(&rows, row_counter.p, 8, stream);
    rt_sync(stream);
    stats.nn_rows = (int64_t)rows;
    stats.nn_rows_evaluated = stats.nn_rows;
    return finished;
  }
};

/* ---- Tourney (tourney.cpp): its matches are the games of one trainer */
struct ca_tourney {
  int device = 0;
  uint32_t arena_units = 0;
  int trace = 0;
  std::map<int, PlayerCfg> players;            /* Tourney::players_ (tourney.h:42) */
  std::vector<std::pair<int, int>> matches;    /* addMatch order */
  std::vector<char> match_logging;             /* addMatch's `logging` */
  std::string log_folder;                      /* Tourney::log_folder_ (tourney.h:46) */
  bool seen_done = false;
  std::mt19937 generator;                      /* default constructed: seed 5489 (tourney.h:43) */
  std::vector<uint32_t> seeds;
  std::unique_ptr<ca_trainer> pool;            /* built at the first query after the last addMatch */
  CallbackState callback{false, false, "; this tournament cannot go on"}; /* a caller-supplied network function that failed */
  std::map<int, NetSpec> net_specs;            /* fused mode: model id -> network (ca_tourney_set_net, _set_net_fn) */
  std::map<int, std::unique_ptr<CoNet>> nets;
  int dev() const { return device; }
  bool exact_offsets = false;                  /* ca_tourney_set_exact_offsets */

  /* The loop of rating/tourney.pyx:122-160 with the networks on the GPU: for every model id in
   * ascending order, pack that model's requests (Tourney::writeRequests), evaluate them, iterate
   * its matches (Tourney::doIteration, which reads the evaluations through the reference's offset
   * table).  The evaluation arrays persist between rounds like the driver's, so the result is the
   * one the compat protocol gives with the same networks. */
  bool run(int64_t max_rounds) {
    callback.need_none_failed("ca_tourney_run");
    ca_trainer &p = built();
    std::vector<int> ids;
    for (auto &m : matches)
      for (int pid : {m.first, m.second}) {
        int id = players.at(pid).model_id;
        if (std::find(ids.begin(), ids.end(), id) == ids.end()) ids.push_back(id);
      }
    std::sort(ids.begin(), ids.end());
    for (int id : ids) {
      if (id < 0) continue;
      if (!nets.count(id)) {
        auto it = net_specs.find(id);
        if (it == net_specs.end()) throw CaError(CA_ERR_STATE, "ca_tourney_run: no network for model id " + std::to_string(id));
        nets[id] = it->second.make((size_t)p.G * p.spe, p.stream, &callback, " for model id " + std::to_string(id) + ", this tournament");
      }
    }
    int64_t rounds = 0;
    bool done = p.tourney_all_done();
    int failed_id = -1;
    while (!done && (max_rounds <= 0 || rounds < max_rounds)) {
      for (int id : ids) {
        p.tourney_round(id, id >= 0 ? nets[id].get() : nullptr);
        if (id >= 0 && nets[id]->callback_failed()) { /* (a caller-supplied network: nothing more is queued) */
          failed_id = id;
          break;
        }
      }
      if (failed_id >= 0) break;
      ++rounds;
      /* the host looks at the all-done flag every eighth round only (a round that finds every match
       * finished launches kernels that return at once), so the queue never runs dry in between */
      if ((rounds & 7) == 0 || (max_rounds > 0 && rounds >= max_rounds)) done = p.tourney_poll_done(ids.front());
    }
    if (failed_id >= 0) {
      p.drain();
      callback.check(nets[failed_id].get(), "model id " + std::to_string(failed_id));
    }
    p.tourney_rounds_done();
    if (done) all_done(); /* (writes the match logs) */
    return done;
  }

  /* Tourney::all_done (tourney.cpp:14-21); the log files of the matches are written the first time it is true */
  bool all_done() {
    ca_trainer &p = built();
    const bool done = p.tourney_all_done();
    if (done && !seen_done) {
      seen_done = true;
      p.maybe_write_logs();
    }
    return done;
  }

  ca_trainer &built_or_state() {
    try {
      return built();
    } catch (const std::exception &e) {
      throw CaError(CA_ERR_STATE, e.what());
    }
  }
  ca_trainer &built() {
    if (pool) return *pool;
    if (matches.empty()) throw CaError(CA_ERR_STATE, "tourney without matches");
    ca_trainer::TourneySetup setup{{}, seeds, exact_offsets};
    ca_config c;
    memset(&c, 0, sizeof c);
    c.num_games = (int32_t)matches.size();
    c.device = device;
    c.testing = 1;
    c.no_stagger = 1;
    c.trace = trace;
    c.arena_units = arena_units;
    c.c_puct = 1.0f;
    c.max_searches = 1;
    c.searches_per_eval = 1;
    for (auto &m : matches) {
      for (int side = 0; side < 2; ++side) {
        const PlayerCfg &p = players.at(side == 0 ? m.first : m.second);
        setup.players.push_back(p);
        if (!p.random) {
          c.max_searches = std::max(c.max_searches, p.max_searches);
          c.searches_per_eval = std::max(c.searches_per_eval, p.searches_per_eval);
        }
      }
    }
    auto t = std::make_unique<ca_trainer>();
    t->init(c, &setup);
    /* tourney.cpp:83-96: a match added with logging = true writes <log_folder>/match_<p1>_<p2>_<index>.txt */
    std::vector<int> logged;
    std::vector<std::string> paths;
    for (size_t i = 0; i < matches.size(); ++i)
      if (match_logging[i]) {
        logged.push_back((int)i);
        paths.push_back(log_folder + "/match_" + std::to_string(matches[i].first) + "_" + std::to_string(matches[i].second) + "_" +
                        std::to_string(i) + ".txt");
      }
    if (!logged.empty()) t->set_log_records(logged, paths, true);
    pool = std::move(t);
    return *pool;
  }
};

/* ------------------------------------------------------------------- C ABI */
extern "C" int ca_device_check(int device) {
#ifdef CO_EMU
  (void)device;
  return CA_OK;
#else
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= device) {
    g_last_error = "no HIP device " + std::to_string(device) + " visible";
    return CA_ERR_DEVICE;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
    g_last_error = "hipGetDeviceProperties failed";
    return CA_ERR_DEVICE;
  }
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
    g_last_error = std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
    return CA_ERR_DEVICE;
  }
  return CA_OK;
#endif
}

/* An entry point without a handle (the *_create calls, the stand-alone test entry points): the device checked and made
 * current, then the body under the guard ... */
template <class F>
static int on_device(int device, F &&body) {
  const int rc = ca_device_check(device);
  if (rc != CA_OK) return rc;
  return co_guard([&] {
    rt_set_device(device);
    body();
  });
}
/* ... with a stream of its own */
template <class F>
static int on_device_stream(int device, F &&body) {
  return on_device(device, [&] {
    Stream s;
    s.create();
    body(s);
  });
}

/* the reference's to_play: 0 / 1 an arena model, anything else every game */
static int norm_to_play(int to_play) { return to_play == 0 || to_play == 1 ? to_play : -1; }

extern "C" int ca_trainer_create(const ca_config *cfg, ca_trainer **out) {
  if (!cfg || !out) {
    g_last_error = "null argument";
    return CA_ERR_ARG;
  }
  *out = nullptr;
  /* the asserts of trainer.cpp:25-34, as errors */
  if (cfg->num_games <= 0 || cfg->max_searches < 0 || cfg->searches_per_eval < 0 || cfg->epsilon < 0.0f ||
      cfg->epsilon > 1.0f || cfg->num_logged != 0 ||
      (cfg->max_searches > 0 && cfg->searches_per_eval > cfg->max_searches) ||
      (cfg->total_games > 0 && cfg->game_base + cfg->num_games > cfg->total_games) || cfg->game_base < 0) {
    g_last_error = "ca_trainer_create: invalid configuration (num_logged must be 0 on device)";
    return CA_ERR_ARG;
  }
  return on_device(cfg->device, [&] {
    auto t = std::make_unique<ca_trainer>();
    t->init(*cfg);
    *out = t.release();
  });
}

extern "C" void ca_trainer_destroy(ca_trainer *t) { delete t; }

extern "C" int ca_trainer_num_requests(ca_trainer *t, int to_play, int32_t *out) {
  return co_guard(t, [&] { *out = t->num_requests(norm_to_play(to_play)); });
}
extern "C" int ca_trainer_num_samples(ca_trainer *t, int32_t *out) { return co_guard(t, [&] { *out = t->num_samples(); }); }
extern "C" int ca_trainer_score(ca_trainer *t, float *out) { return co_guard(t, [&] { *out = t->score(); }); }
extern "C" int ca_trainer_avg_mate_length(ca_trainer *t, float *out) { return co_guard(t, [&] { *out = t->avg_mate_length(); }); }
extern "C" int ca_trainer_write_requests(ca_trainer *t, float *gs, int to_play) {
  return co_guard(t, [&] { t->write_requests(gs, norm_to_play(to_play)); });
}
extern "C" int ca_trainer_write_samples(ca_trainer *t, float *gs, float *ev, float *pr) {
  return co_guard(t, [&] { t->write_samples(gs, ev, pr); });
}
extern "C" int ca_trainer_write_scores(ca_trainer *t, const char *file) { return co_guard(t, [&] { t->write_scores(file); }); }
extern "C" int ca_trainer_do_iteration(ca_trainer *t, const float *ev, const float *pr, int to_play, int32_t *all_done) {
  return co_guard(t, [&] { *all_done = t->do_iteration(ev, pr, norm_to_play(to_play)) ? 1 : 0; });
}
extern "C" int ca_trainer_set_net(ca_trainer *t, int slot, int kind, const float *w, size_t n) {
  return co_guard(t, [&] { t->set_net(slot, NetSpec(kind, w, n), "ca_trainer_set_net"); });
}
extern "C" int ca_trainer_set_net_fn(ca_trainer *t, int slot, ca_net_fn fn, void *user, float *d_states, float *d_evals,
                                     float *d_probs, int32_t max_rows, double flop_per_row) {
  return co_guard(t, [&] {
    t->set_net(slot, NetSpec("ca_trainer_set_net_fn", {fn, user, d_states, d_evals, d_probs, max_rows, flop_per_row}), "ca_trainer_set_net_fn");
  });
}
extern "C" int ca_trainer_request_rows(ca_trainer *t, int32_t *rows) {
  return co_guard(t, [&] {
    if (!rows) throw CaError(CA_ERR_ARG, "ca_trainer_request_rows: null argument");
    *rows = t->R * t->spe;
  });
}
extern "C" int ca_trainer_set_host_cache(ca_trainer *t, int32_t log2_entries) {
  return co_guard(t, [&] { t->set_host_cache(log2_entries); });
}
extern "C" int ca_trainer_run(ca_trainer *t, int64_t max_iterations, int32_t *all_done) {
  return co_guard(t, [&] { *all_done = t->run(max_iterations) ? 1 : 0; });
}
extern "C" int ca_trainer_export_samples(ca_trainer *t, float *sp, float *oc) { return co_guard(t, [&] { t->export_samples(sp, oc); }); }
extern "C" int ca_trainer_pack_samples_device(ca_trainer *t, void *d_sp, void *d_oc, int32_t cap_rows, int32_t *n_rows) {
  return co_guard(t, [&] { *n_rows = t->pack_samples_device((float *)d_sp, (float *)d_oc, cap_rows); });
}
extern "C" int ca_trainer_pin_host(ca_trainer *t, void *p, size_t bytes, int32_t *pinned) {
  return co_guard(t, [&] { *pinned = t->pin_host(p, bytes) ? 1 : 0; });
}
extern "C" int ca_trainer_unpin_host(ca_trainer *t, void *p) { return co_guard(t, [&] { t->unpin_host(p); }); }
extern "C" int ca_trainer_set_positions(ca_trainer *t, const int32_t *boards, const int32_t *to_play, const int32_t *pieces,
                                        const int32_t *seeds) {
  return co_guard(t, [&] { t->set_positions(boards, to_play, pieces, seeds); });
}
extern "C" int ca_trainer_analysis(ca_trainer *t, int32_t *out) { return co_guard(t, [&] { t->analysis(out); }); }
extern "C" int ca_trainer_finish(ca_trainer *t) { return co_guard(t, [&] { t->finish_analysis(); }); }
extern "C" int ca_trainer_set_logging(ca_trainer *t, const char *log_folder, int32_t num_logged) {
  return co_guard(t, [&] { t->set_logging(log_folder, num_logged); });
}
extern "C" int ca_trainer_reset(ca_trainer *t, int32_t seed) { return co_guard(t, [&] { t->reset_games(seed); }); }
extern "C" int ca_trainer_device(ca_trainer *t, int32_t *device) {
  return co_guard(t, [&] {
    if (!device) throw CaError(CA_ERR_ARG, "ca_trainer_device: null argument");
    *device = t->dev();
  });
}
/* diagnostic builds (-DCO_PROF), see ca_trainer::read_prof; not in the public header */
extern "C" int ca_trainer_prof(ca_trainer *t, unsigned long long out[2 * CO_NPROF + 24]) {
  return co_guard(t, [&] { t->read_prof(out); });
}

extern "C" int ca_trainer_net_forward(ca_trainer *t, int slot, const float *states, int32_t n, float *evals, float *probs) {
  return co_guard(t, [&] { t->net_forward_host(slot, states, n, evals, probs); });
}
extern "C" int ca_trainer_net_bench(ca_trainer *t, int slot, const float *states, int32_t rows, int32_t reps, float *ms_per_call) {
  return co_guard(t, [&] { *ms_per_call = t->net_bench(slot, states, rows, reps); });
}

extern "C" int ca_expand_samples(int device, const float *state_policy, const float *outcome, int32_t n, float *gs, float *ev,
                                 float *pr) {
  /* host-side K7 for gathered shards: same gathers as co_k_write_samples */
  (void)device;
  static const int32_t SS[8][16] = CO_SPACE_SYM_INIT;
  static const int32_t MS[8][96] = CO_MOVE_SYM_INIT;
  for (int32_t i = 0; i < n; ++i) {
    const float *st = state_policy + (size_t)i * CO_SAMPLE_FLOATS;
    const float *pol = st + CO_GAME_STATE_SIZE;
    for (int k = 0; k < 8; ++k) {
      float *g = gs + ((size_t)i * 8 + k) * CO_GAME_STATE_SIZE;
      float *p = pr + ((size_t)i * 8 + k) * CO_NUM_MOVES;
      for (int j = 0; j < 64; ++j) g[j] = st[SS[k][j / 4] * 4 + j % 4];
      for (int j = 64; j < CO_GAME_STATE_SIZE; ++j) g[j] = st[j];
      for (int j = 0; j < CO_NUM_MOVES; ++j) p[j] = pol[MS[k][j]];
      ev[(size_t)i * 8 + k] = outcome[i];
    }
  }
  return CA_OK;
}

extern "C" int ca_trainer_stats(ca_trainer *t, ca_stats *out) { return co_guard(t, [&] { t->read_stats(out); }); }
extern "C" int ca_trainer_game_info(ca_trainer *t, int game, int32_t out[8]) { return co_guard(t, [&] { t->game_info(game, out); }); }
extern "C" int ca_trainer_trace(ca_trainer *t, int game, int32_t *out, int32_t cap, int32_t *n) {
  return co_guard(t, [&] { t->read_trace(game, out, cap, n); });
}

/* ---- Tourney C ABI */
extern "C" int ca_tourney_create(int device, uint32_t arena_units, int trace, ca_tourney **out) {
  return on_device(device, [&] {
    if (!out) throw CaError(CA_ERR_ARG, "null output pointer");
    auto t = std::make_unique<ca_tourney>();
    t->device = device;
    t->arena_units = arena_units;
    t->trace = trace;
    *out = t.release();
  });
}
extern "C" void ca_tourney_destroy(ca_tourney *t) { delete t; }

extern "C" int ca_tourney_add_player(ca_tourney *t, int32_t player_id, int32_t model_id, int32_t max_searches,
                                     int32_t searches_per_eval, float c_puct, float epsilon, int32_t random) {
  return co_guard(t, [&] {
    if (t->pool) throw CaError(CA_ERR_STATE, "addPlayer after the tournament has started");
    if (!random && (max_searches <= 0 || searches_per_eval <= 0)) throw CaError(CA_ERR_ARG, "addPlayer: bad search settings");
    PlayerCfg p;
    memset(&p, 0, sizeof p);
    p.player_id = player_id;
    p.model_id = model_id;
    p.max_searches = max_searches;
    p.searches_per_eval = searches_per_eval;
    p.c_puct = c_puct;
    p.epsilon = epsilon;
    p.random = random ? 1 : 0;
    t->players[player_id] = p;
  });
}

extern "C" int ca_tourney_add_match(ca_tourney *t, int32_t player1, int32_t player2, int32_t logging) {
  return co_guard(t, [&] {
    if (t->pool) throw CaError(CA_ERR_STATE, "addMatch after the tournament has started");
    if (!t->players.count(player1) || !t->players.count(player2)) throw CaError(CA_ERR_ARG, "addMatch: unknown player");
    if (t->players[player1].random && t->players[player2].random)
      throw CaError(CA_ERR_ARG, "addMatch: at most one random player per match (match.cpp:72)");
    t->matches.emplace_back(player1, player2);
    t->match_logging.push_back(logging ? 1 : 0);
    t->seeds.push_back((uint32_t)t->generator()); /* tourney.cpp:86 */
  });
}
extern "C" int ca_tourney_set_log_folder(ca_tourney *t, const char *log_folder) {
  return co_guard(t, [&] {
    if (t->pool) throw CaError(CA_ERR_STATE, "set_log_folder after the tournament has started");
    t->log_folder = log_folder ? log_folder : "";
  });
}

/* the network of model `model_id`, made when the tournament next runs (NetSpec::make) */
static void tourney_set_net(ca_tourney *t, int32_t model_id, NetSpec spec) {
  if (model_id < 0) throw CaError(CA_ERR_ARG, "negative model ids are the dummy ids of random players");
  t->net_specs[model_id] = std::move(spec);
  t->nets.erase(model_id);
}
extern "C" int ca_tourney_set_net(ca_tourney *t, int32_t model_id, int32_t kind, const float *weights, size_t n_floats) {
  return co_guard(t, [&] {
    if (!weights || n_floats == 0) throw CaError(CA_ERR_ARG, "ca_tourney_set_net: no weights");
    tourney_set_net(t, model_id, NetSpec(kind, weights, n_floats).keep());
  });
}
extern "C" int ca_tourney_set_net_fn(ca_tourney *t, int32_t model_id, ca_net_fn fn, void *user, float *d_states, float *d_evals,
                                     float *d_probs, int32_t max_rows, double flop_per_row) {
  return co_guard(t, [&] {
    tourney_set_net(t, model_id, NetSpec("ca_tourney_set_net_fn", {fn, user, d_states, d_evals, d_probs, max_rows, flop_per_row}));
  });
}
extern "C" int ca_tourney_set_exact_offsets(ca_tourney *t, int32_t on) {
  return co_guard(t, [&] {
    if (t->pool) throw CaError(CA_ERR_STATE, "set_exact_offsets after the tournament has started");
    t->exact_offsets = on != 0;
  });
}
extern "C" int ca_tourney_run(ca_tourney *t, int64_t max_rounds, int32_t *all_done) {
  return co_guard(t, [&] { *all_done = t->run(max_rounds) ? 1 : 0; });
}
extern "C" int ca_tourney_all_done(ca_tourney *t, int32_t *out) { return co_guard(t, [&] { *out = t->all_done() ? 1 : 0; }); }
extern "C" int ca_tourney_num_requests(ca_tourney *t, int32_t id, int32_t *out) {
  return co_guard(t, [&] { *out = t->built().num_requests(id); });
}
extern "C" int ca_tourney_write_requests(ca_tourney *t, float *game_states, int32_t id) {
  return co_guard(t, [&] { t->built().write_requests(game_states, id); });
}
extern "C" int ca_tourney_do_iteration(ca_tourney *t, const float *evaluations, const float *probabilities,
                                       int32_t rows, int32_t id) {
  return co_guard(t, [&] { t->built().tourney_do_iteration(evaluations, probabilities, rows, id); });
}
extern "C" int ca_tourney_num_matches(ca_tourney *t, int32_t *out) { return co_guard(t, [&] { *out = (int32_t)t->matches.size(); }); }
/* out[8] = {player id 1, player id 2, done, result (util.h:57-64, first player's view), side to move, pending
 * requests, plies, error} */
extern "C" int ca_tourney_match_info(ca_tourney *t, int32_t match, int32_t out[8]) {
  return co_guard(t, [&] {
    const GameCtl &gc = t->built().game(match, "match index out of range");
    out[0] = t->matches[match].first;
    out[1] = t->matches[match].second;
    out[2] = gc.done;
    out[3] = gc.result;
    out[4] = gc.to_play;
    out[5] = gc.done ? 0 : gc.n_pending;
    out[6] = gc.plies;
    out[7] = gc.error;
  });
}
extern "C" int ca_tourney_match_score(ca_tourney *t, int32_t match, float *out) {
  return co_guard(t, [&] {
    *out = ca_trainer::game_score(t->built().game(match, "match index out of range")); /* Match::score, match.cpp:52-58 */
  });
}
/* Tourney::writeScores, tourney.cpp:33-41: "id1 id2 score" per finished match */
extern "C" int ca_tourney_write_scores(ca_tourney *t, const char *filename) {
  return co_guard(t, [&] {
    ca_trainer &p = t->built();
    std::ofstream f(filename);
    if (!f) throw CaError(CA_ERR_ARG, std::string("cannot open ") + filename);
    for (int g = 0; g < (int)t->matches.size(); ++g) {
      const GameCtl &gc = p.game(g);
      if (gc.done) f << t->matches[g].first << ' ' << t->matches[g].second << ' ' << ca_trainer::game_score(gc) << '\n';
    }
  });
}
/* the trace and the statistics of the tournament's trainer; a tournament that cannot be built is CA_ERR_STATE here */
extern "C" int ca_tourney_trace(ca_tourney *t, int32_t match, int32_t *out, int32_t cap, int32_t *n_out) {
  return co_guard(t, [&] { t->built_or_state().read_trace(match, out, cap, n_out); });
}
extern "C" int ca_tourney_stats(ca_tourney *t, ca_stats *out) {
  return co_guard(t, [&] { t->built_or_state().read_stats(out); });
}

/* ---- the library's own network kernels on device memory, without a trainer (ca_net_*): a CoNet and the 80-float rows the
 * kernels read, i.e. ca_trainer::net_forward_host without its copies */
struct ca_net {
  int device = 0;
  Stream stream;
  std::unique_ptr<CoNet> net;
  DevBuf<float> rows80; /* [max_rows][CO_STATE_STRIDE] */
  /* ONE row buffer: a call on another stream than the last one (the pools of a fused run) starts behind that one's kernels */
  Event used;
  rt_stream_t used_on = {};
  bool used_once = false;
  int dev() const { return device; }

  void forward_device(const float *d_states, int32_t rows_cap, const int32_t *d_rows, float *d_evals, float *d_probs, void *stream_arg) {
    if (!d_states || !d_rows || !d_evals || !d_probs) throw CaError(CA_ERR_ARG, "ca_net_forward_device: null buffer");
    if (rows_cap < 0 || (size_t)rows_cap > net->max_rows()) throw CaError(CA_ERR_ARG, "ca_net_forward_device: more rows than the net's max_rows");
    if (rows_cap == 0) return;
    const rt_stream_t s = stream_arg ? (rt_stream_t)(intptr_t)stream_arg : (rt_stream_t)stream;
    if (used_once && used_on != s) rt_stream_wait(s, used);
    expand_rows(d_states, rows80.p, rows_cap, s);
    net->forward(rows80.p, rows_cap, d_rows, d_evals, d_probs, s);
    rt_event_record(used, s);
    used_on = s;
    used_once = true;
    if (!stream_arg) {
      rt_sync(s);
      check_net_range(net.get(), s, "ca_net_forward_device");
    }
  }
};

extern "C" int ca_net_create(int device, int kind, const float *weights, size_t n_floats, int32_t max_rows, ca_net **out) {
  return on_device_stream(device, [&](Stream &s) {
    if (!out || !weights || max_rows <= 0) throw CaError(CA_ERR_ARG, "ca_net_create: null argument or max_rows < 1");
    *out = nullptr;
    auto n = std::make_unique<ca_net>();
    n->device = device;
    n->stream = std::move(s);
    n->used.create();
    n->net = NetSpec(kind, weights, n_floats).make((size_t)max_rows, n->stream, nullptr);
    n->rows80.alloc((size_t)max_rows * CO_STATE_STRIDE, n->stream);
    rt_sync(n->stream);
    *out = n.release();
  });
}
extern "C" int ca_net_forward_device(ca_net *n, const float *d_states, int32_t rows_cap, const int32_t *d_rows, float *d_evals,
                                     float *d_probs, void *stream) {
  return co_guard(n, [&] { n->forward_device(d_states, rows_cap, d_rows, d_evals, d_probs, stream); });
}
extern "C" void ca_net_destroy(ca_net *n) { delete n; }

/* ---- stand-alone test entry points, each on a stream of its own */

extern "C" int ca_rules_legal_moves(int device, const uint64_t *boards, const uint32_t *metas, int32_t n, uint32_t *masks,
                                    int32_t *is_lines) {
  return on_device_stream(device, [&](Stream &ts) {
    DevBuf<uint64_t> b;
    DevBuf<uint32_t> m, mk;
    DevBuf<int32_t> ln;
    b.upload(boards, n, ts); m.upload(metas, n, ts); mk.alloc((size_t)n * 3, ts); ln.alloc(n, ts);
    RT_LAUNCH(co_k_rules_batch, n, CO_WAVE, ts, (const uint64_t *)b.p, (const uint32_t *)m.p, n, mk.p, ln.p);
    rt_d2h(masks, mk.p, (size_t)n * 12, ts);
    rt_d2h(is_lines, ln.p, (size_t)n * 4, ts);
    rt_sync(ts);
  });
}

extern "C" int ca_rules_do_move(int device, uint64_t *boards, uint32_t *metas, const int32_t *moves, int32_t n, float *states) {
  return on_device_stream(device, [&](Stream &ts) {
    DevBuf<uint64_t> b;
    DevBuf<uint32_t> m;
    DevBuf<int32_t> mv;
    DevBuf<float> st;
    b.upload(boards, n, ts); m.upload(metas, n, ts); mv.upload(moves, n, ts); st.alloc((size_t)n * CO_STATE_STRIDE, ts);
    RT_LAUNCH(co_k_domove_batch, n, CO_WAVE, ts, b.p, m.p, (const int32_t *)mv.p, n, st.p);
    std::vector<float> tmp((size_t)n * CO_STATE_STRIDE);
    rt_d2h(boards, b.p, (size_t)n * 8, ts);
    rt_d2h(metas, m.p, (size_t)n * 4, ts);
    rt_d2h(tmp.data(), st.p, tmp.size() * 4, ts);
    rt_sync(ts);
    for (int i = 0; i < n; ++i)
      memcpy(states + (size_t)i * CO_GAME_STATE_SIZE, &tmp[(size_t)i * CO_STATE_STRIDE], CO_GAME_STATE_SIZE * 4);
  });
}

extern "C" int ca_rules_rows(int device, uint64_t *boards, uint32_t *metas, const int32_t *moves, int32_t n, uint32_t *masks) {
  return on_device_stream(device, [&](Stream &ts) {
    DevBuf<uint64_t> b;
    DevBuf<uint32_t> m, mk;
    DevBuf<int32_t> mv;
    b.upload(boards, n, ts); m.upload(metas, n, ts); mv.upload(moves, n, ts); mk.alloc((size_t)n * 3, ts);
    RT_LAUNCH(co_k_rules_rows, (n + 3) / 4, CO_WAVE, ts, b.p, m.p, (const int32_t *)mv.p, n, mk.p);
    rt_d2h(boards, b.p, (size_t)n * 8, ts);
    rt_d2h(metas, m.p, (size_t)n * 4, ts);
    rt_d2h(masks, mk.p, (size_t)n * 12, ts);
    rt_sync(ts);
  });
}

extern "C" int ca_rng_draw(int device, uint32_t seed, int32_t n, int32_t chunk, uint32_t *out) {
  return on_device_stream(device, [&](Stream &ts) {
    if (chunk < 1 || chunk > CO_WAVE) throw CaError(CA_ERR_ARG, "chunk must be 1..64");
    std::vector<uint32_t> x(CO_MT_N);
    x[0] = seed;
    for (int i = 1; i < CO_MT_N; ++i) x[i] = 1812433253u * (x[i - 1] ^ (x[i - 1] >> 30)) + (uint32_t)i;
    DevBuf<uint32_t> mt, o;
    DevBuf<int32_t> idx;
    const int32_t i0 = CO_MT_N;
    mt.upload(x.data(), CO_MT_N, ts); idx.upload(&i0, 1, ts); o.alloc(n, ts);
    RT_LAUNCH(co_k_rng_draw, 1, CO_WAVE, ts, mt.p, idx.p, n, chunk, o.p);
    rt_d2h(out, o.p, (size_t)n * 4, ts);
    rt_sync(ts);
  });
}

extern "C" int ca_fp_probe(int device, const float *in, int32_t n, float *out) {
  return on_device_stream(device, [&](Stream &ts) {
    DevBuf<float> di, dout;
    di.upload(in, (size_t)n * 8, ts); dout.alloc((size_t)n * 8, ts);
    RT_LAUNCH(co_k_fp_probe, (n + CO_WAVE - 1) / CO_WAVE, CO_WAVE, ts, (const float *)di.p, n, dout.p);
    rt_d2h(out, dout.p, (size_t)n * 32, ts);
    rt_sync(ts);
  });
}
