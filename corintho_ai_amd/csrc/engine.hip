// engine.hip -- host side of the self-play pool and the C ABI (include/corintho_hip.h): the one translation unit of the
// engine.  ca_trainer below is configuration and orchestration; what it orchestrates owns its own state:
//   game_store.h     GameStore: the device side of the games (sizing, allocations, seeding, EngineParams);
//                    TourneyTables: a tournament's per-match tables beside it
//   game_view.h      GameView: the host's copy of the games by game index, and what is read off it
//   game_logs.h      GameLogs: the per-game text logs (printed by logfmt.h)
//   samples_host.h   SampleExits: the three ways samples leave; ca_expand_samples
//   net_host.h       how a network comes in (NetSpec, HostNet, ExternalNet); HostForward: host rows through a network
//   nn_group.h       rows of many models in one network launch: the grouping kernels, GroupPlanner, ca_net_group
//   analysis_host.h  AnalysisPositions: given positions in, their result words out
//   pools.h          FusedRun: fused training on pools of the games
//   host.h           owners of runtime resources, HostPins, the guards of the entry points
//   tourney_host.h   ca_tourney and its C ABI, on the trainer's primitives
//   probes.h         ca_net_* and the stand-alone test entry points
// The words host and kernels pass each other are named in engine_defs.h.
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
#include <memory>
#include <string>
#include <vector>

#include "analysis_host.h"
#include "game_logs.h"
#include "game_store.h"
#include "game_view.h"
#include "net_host.h"
#include "nn_group.h"
#include "pools.h"
#include "samples_host.h"

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
  Stream stream;      /* (first: it outlives every buffer and network) */
  EngineParams P;     /* what stays fixed between runs (rebind); a launch takes its own copy (params) */
  GameStore store;
  GameView view;
  GameLogs logs;
  SampleExits samples;
  HostForward host_forward;
  AnalysisPositions positions; /* analysis mode */
  TourneyTables tour;          /* tournament mode (ca_tourney) */
  /* host state */
  int64_t iterations = 0;
  int32_t trainer_iteration = 0; /* Trainer::searches_done_ (train mode only) */
  bool scan_valid = false;
  int scan_valid_for = 0;      /* to_play / model id the current req_offset/nn_in describe (if scan_valid) */
  int32_t last_total = 0;
  bool finished = false;
  bool any_error = false; /* the last scan saw an error bit in some game */
  bool net_used = false;  /* a network launch has been queued since the range flags were last read */
  /* fused mode */
  std::unique_ptr<CoNet> nets[2];
  /* a caller-supplied network function (ExternalNet) that returned non-zero: the generation is unusable until ca_trainer_reset */
  CallbackState callback{false, false, " in this generation; it cannot go on -- start a new one with ca_trainer_reset"};
  RunStats stats;
  FusedRun fused; /* fused training: the pools, their table and the run (pools.h) */
  /* host-driven protocol with the evaluation cache (ca_trainer_set_host_cache): fused training on one pool, stepped one
   * iteration per doIteration, the caller as its network (net_host.h HostNet) */
  bool host_cache = false;
  int host_cache_log2 = -1; /* the table: 0 sized automatically, else 2^n entries */
  int32_t host_rows = 0;    /* rows handed to the caller by the last iteration: the cache's count word */
  HostNet host_net;
  HostPins pins; /* (last: the registrations are released before anything else goes) */

  int dev() const { return cfg.device; }
  /* the one mode whose slots are recycled: its games do not depend on which other games are resident */
  bool self_play_training() const { return !cfg.testing && !cfg.analyse && !tour.active(); }
  /* the evaluation cache serves fused training (and fused analysis): one network, rows packed by the search kernel */
  /* Not for the analysis of caller-given positions (the table's header encoding relies on boards that doMove
   * produced).  Automatic (eval_cache = 0): only for a network whose rows cost more than resolving them -- the 9.65
   * MFLOP residual CNN, not the 0.25 MFLOP MLP (measured: the MLP's whole launch is 43 us for 12 k rows, the probe 15). */
  bool use_cache() const {
    if (cfg.eval_cache < 0 || tour.active() || cfg.analyse) return false;
    if (cfg.eval_cache > 0) return true;
    return nets[0] && nets[0]->flop_per_row() >= 1e6;
  }
  /* the device has moved on: what the host knows of the batch and of the games is stale */
  void invalidate() { scan_valid = view.valid = false; }
  /* rows one launch can ask a network for (ca_trainer_request_rows) */
  size_t request_rows() const { return store.request_rows(spe); }
  /* the games by game index, as the device holds them now */
  const std::vector<GameCtl> &games() { return view.fetch(store, G, stream); }

  /* tables: a tournament's trainer (ca_tourney), one match per game */
  void init(const ca_config &c, TourneyTables tables = TourneyTables()) {
    cfg = c;
    tour = std::move(tables);
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
    store.create(cfg, G, spe, self_play_training(), cfg.eval_cache >= 0 && !tour.active() && !cfg.analyse, stream);
    if (tour.active()) tour.create(store.R, stream);
    /* (an analysis trainer is reset by set_positions, once the positions and their seeds are known) */
    if (!cfg.analyse) reset_games(cfg.seed);
    rebind();
    fused.work_counter = store.work_counter.p;
    fused.nn_eval = store.nn_eval.p;
    fused.nn_probs = store.nn_probs.p;
    fused.stats = &stats;
    fused.stream = stream;
  }

  /* P from the parts that own what it names; nothing else assigns a field of P */
  void rebind() {
    memset(&P, 0, sizeof P);
    store.bind(P, cfg, G, spe);
    logs.bind(P);
    tour.bind(P);
  }

  /* Trainer::initialize (trainer.cpp:238-256); also starts a new generation in the same pool (ca_trainer_reset) */
  void reset_games(int32_t seed) {
    cfg.seed = seed;
    if (positions.given()) positions.write_terminal_rows(store.req.p, (size_t)spe * CO_STATE_STRIDE, stream);
    store.seed(cfg, G, tour.active() ? tour.match_seeds.data() : positions.given() ? positions.seed.data() : nullptr,
               [&](GameCtl &gc, int g) {
                 if (positions.given()) positions.place(gc, g);
               },
               stream);
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
    logs.clear(stream);
  }

  /* Trainer::initialize, trainer.cpp:243-250: the first num_logged games write `<log_folder>/game_<i>.txt` (i = the game's
   * index in the generation).  Before the first iteration only. */
  void set_logging(const char *folder, int n) {
    if (tour.active() || cfg.analyse) throw CaError(CA_ERR_STATE, "per-game logs belong to Trainer games (self-play or arena)");
    if (iterations != 0 || trainer_iteration != 0) throw CaError(CA_ERR_STATE, "ca_trainer_set_logging: the games have started");
    if (n < 0) throw CaError(CA_ERR_ARG, "ca_trainer_set_logging: num_logged < 0");
    n -= cfg.game_base; /* a shard logs the games of the generation's first num_logged that it owns */
    if (n < 0) n = 0;
    if (n > G) n = G;
    if (n > store.R) /* logged games start in their own slots (search_step.h co_slot_next_game): fewer slots than logged games would write fewer files than the reference */
      throw CaError(CA_ERR_ARG, "ca_trainer_set_logging: " + std::to_string(n) + " logged games on " + std::to_string(store.R) +
                                        " resident slots -- a logged game must start in its own slot; raise ca_config.resident");
    std::vector<int> first(n);
    for (int g = 0; g < n; ++g) first[g] = g;
    set_log_records(first, GameLogs::game_paths(folder, cfg.game_base, n), false);
  }
  void set_log_records(const std::vector<int> &which, const std::vector<std::string> &paths, bool with_index) {
    logs.set_records(which, paths, with_index, G, stream);
    rebind();
  }
  /* the log files, the first time every game is over */
  void write_logs_once() {
    if (logs.pending()) logs.write(games(), stream);
  }

  /* the engine parameters of one launch for model `to_play` (-1: every game) at the current iteration; the launch site
   * sets whatever else is its own (fused pools, the arena's device state, force_choose) on its copy */
  EngineParams params(int to_play) const {
    EngineParams e = P;
    e.to_play = to_play;
    e.iteration = trainer_iteration;
    return e;
  }

  /* K4 for model e.to_play, queued: its offsets (and the flags of EngineParams::ctl), then its compact batch */
  void scan(const EngineParams &e) { RT_LAUNCH(co_k_scan, 1, CO_WAVE, stream, e); }
  void compact(const EngineParams &e) { RT_LAUNCH(co_k_compact, store.R, CO_WAVE, stream, e); }
  /* h_ctl holds what a scan for model `to_play` wrote: the batch and the flags the host goes by */
  void read_ctl(int to_play) {
    last_total = store.h_ctl[CO_CTL_ROWS];
    finished = store.h_ctl[CO_CTL_ALL_DONE] != 0;
    any_error = store.h_ctl[CO_CTL_ANY_ERROR] != 0;
    scan_valid_for = to_play;
    scan_valid = true;
  }
  /* scan + compact + read for model `to_play`; ONE host synchronisation, on 16 bytes */
  void pack(int to_play) {
    if (scan_valid && scan_valid_for == to_play) return;
    const EngineParams e = params(to_play);
    scan(e);
    compact(e);
    rt_d2h(store.h_ctl, store.ctl.p, CO_CTL_WORDS * 4, stream);
    rt_sync(stream);
    read_ctl(to_play);
    if (finished && !any_error) write_logs_once();
  }
  /* the all-done flag, refreshed by a scan for model `to_play` */
  bool poll_all_done(int to_play) {
    scan(params(to_play));
    int32_t d = 0;
    rt_d2h(&d, store.all_done.p, 4, stream);
    rt_sync(stream);
    return d != 0;
  }

  /* the caller's answers to `rows` request rows go where a network kernel would have written them; false: there were
   * none to take (no rows, or null arrays) */
  bool upload_answers(const float *evals, const float *probs, int32_t rows) {
    if (rows <= 0 || !evals || !probs) return false;
    rt_h2d(store.nn_eval.p, evals, (size_t)rows * 4, stream);
    rt_h2d(store.nn_probs.p, probs, (size_t)rows * CO_NUM_MOVES * 4, stream);
    return true;
  }

  void check_errors() {
    check_net_range();
    if (scan_valid && !any_error) return; /* the last scan saw no error bit in any game */
    throw_game_errors(games());
  }

  /* one launch of the search kernel on every slot, and what the host has to know afterwards: the batch of model
   * e.to_play and the games' error bits */
  void step(const EngineParams &e) {
    launch_mcts_step(e, store.R, stream);
    ++stats.mcts_launches;
    invalidate();
    pack(e.to_play);
    check_errors();
  }
  /* one iteration queued without a look at what it leaves: the batch of model e.to_play packed, evaluated by `net`
   * (null: nothing to evaluate), its games stepped */
  void queue_iteration(const EngineParams &e, CoNet *net) {
    scan(e);
    if (net) {
      compact(e);
      net->forward(store.nn_in.p, store.R * spe, store.req_offset.p + store.R, store.nn_eval.p, store.nn_probs.p, stream);
      ++stats.nn_launches;
    }
    launch_mcts_step(e, store.R, stream);
    ++stats.mcts_launches;
    ++iterations;
  }
  /* the same for EVERY model of a tournament at once (tourney_host.h, a grouped round): one scan, one compaction, the
   * rows grouped by the model of the player to move (slot_model: nn_group.h co_k_group_rows), one grouped network
   * launch, one search launch that steps every match */
  void queue_grouped_iteration(CoNetGroup *group, GroupPlanner &planner, const int32_t *slot_model, int32_t *row_model) {
    const EngineParams e = params(CO_TO_PLAY_EVERY_MODEL);
    scan(e);
    compact(e);
    RT_LAUNCH(co_k_group_rows, store.R, CO_WAVE, stream, e, slot_model, row_model);
    planner.run(row_model, store.req_offset.p + store.R, stream);
    group->forward(store.nn_in.p, store.R * spe, planner.plan(), store.nn_eval.p, store.nn_probs.p, stream);
    ++stats.nn_launches;
    launch_mcts_step(e, store.R, stream);
    ++stats.mcts_launches;
    ++iterations;
  }
  /* ... and the look, once the caller is through queuing */
  void queued_iterations_done() {
    invalidate();
    check_errors();
  }
  /* everything queued on the trainer's stream has run; what the host knew of the games is stale */
  void drain() {
    rt_sync(stream);
    invalidate();
  }

  /* Trainer::doIteration (trainer.cpp:164-236), compat protocol */
  void need_positions() const {
    if (cfg.analyse && !positions.given()) throw CaError(CA_ERR_STATE, "analysis trainer: ca_trainer_set_positions first");
  }
  bool do_iteration(const float *evals, const float *probs, int to_play) {
    need_positions();
    callback.need_none_failed("ca_trainer_do_iteration");
    if (host_cache) return host_cache_iteration(evals, probs, to_play);
    if (iterations > 0) {
      pack(to_play); /* offsets the reference computes at entry */
      if (last_total > 0 && !upload_answers(evals, probs, last_total))
        throw CaError(CA_ERR_ARG, "doIteration: null evaluations/probabilities");
    } else {
      rt_memset(store.req_offset.p, 0, ((size_t)store.R + 1) * 4, stream);
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
    rt_d2h(out, store.nn_in70.p, (size_t)n * CO_GAME_STATE_SIZE * 4, stream);
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
    if (!store.pend_key.p) { /* (a trainer created with ca_config.eval_cache < 0 has none yet) */
      store.alloc_pend_keys(spe, stream);
      rebind();
      rt_sync(stream);
    }
    fused.spe = spe;
    fused.create(1, store.R, log2_entries);
    fused.cache_clean = false; /* (the first iteration starts the generation: counters cleared with the table) */
    /* the caller's rows and answers pass through the plain protocol's own staging arrays, which this mode leaves idle */
    host_net.rows_cap = request_rows();
    host_net.rows70 = store.nn_in70.p;
    host_net.ev_in = store.nn_eval.p;
    host_net.pr_in = store.nn_probs.p;
    host_net.d_ctl = store.ctl.p;
    host_net.h_ctl = &store.h_ctl[0];
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
    host_rows = (int32_t)std::min<size_t>(seen.evaluated, request_rows());
    stats.nn_rows += (int64_t)co_pack_rows(seen.pack); /* rows the games requested */
    stats.nn_rows_evaluated += host_rows;                   /* ... and the ones the caller gets */
    check_errors();
    if (finished) write_logs_once();
    return finished;
  }

  /* ---- samples: the guard of the three ways they leave (`what` names the one): their number, the index of them uploaded */
  int32_t need_samples(const char *what, int32_t cap_rows = INT32_MAX) {
    if (cfg.testing) throw CaError(CA_ERR_STATE, std::string(what) + " in testing mode");
    return samples.index(games(), cap_rows, stream);
  }
  void write_samples(float *gs, float *ev, float *pr) {
    const size_t n = (size_t)need_samples("writeSamples");
    if (n > 0) samples.write(P, G, n, gs, ev, pr, stream);
  }
  int32_t pack_samples_device(float *d_state_policy, float *d_outcome, int32_t cap_rows) {
    const int32_t n = need_samples("pack_samples", cap_rows);
    if (n > cap_rows) throw CaError(CA_ERR_ARG, "pack_samples: destination too small");
    if (n > 0) samples.pack(P, G, d_state_policy, d_outcome, stream);
    rt_sync(stream);
    return n;
  }
  void export_samples(float *state_policy, float *outcome) {
    const size_t n = (size_t)need_samples("export_samples");
    if (n > 0) samples.export_host(P, G, n, state_policy, outcome, stream);
  }

  /* ------------------------------------------------------------ analysis mode (DockerMC) */
  void set_positions(const int32_t *boards, const int32_t *to_play, const int32_t *pieces, const int32_t *seeds) {
    if (!cfg.analyse) throw CaError(CA_ERR_STATE, "set_positions: not an analysis trainer (ca_config.analyse)");
    if (iterations > 0) throw CaError(CA_ERR_STATE, "set_positions after the first iteration");
    positions.set(boards, to_play, pieces, seeds, G, stream);
    reset_games(cfg.seed);
  }
  void analysis(int32_t *out) {
    if (!cfg.analyse) throw CaError(CA_ERR_STATE, "not an analysis trainer");
    AnalysisPositions::read(store.req.p, (size_t)spe * CO_STATE_STRIDE, games(), out, stream);
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
  /* the network `spec` names, for launches of up to request_rows() rows on the trainer's stream */
  std::unique_ptr<CoNet> make_net(const NetSpec &spec, CallbackState *guard, const std::string &asker, const char *hint = "") {
    return spec.make(request_rows(), stream, guard, asker, hint);
  }
  /* ... as slot `slot` (net_host.h NetSpec: weights of a kind, or the caller's own function) */
  void set_net(int slot, const NetSpec &spec, const char *who) {
    if (slot < 0 || slot > 1) throw CaError(CA_ERR_ARG, "net slot must be 0 or 1");
    install_net(slot, make_net(spec, &callback, ", this trainer", " (ca_trainer_request_rows)"), who);
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

  /* host rows in, host results out (ca_trainer_net_forward) */
  void net_forward_host(int slot, const float *states, int32_t n, float *evals, float *probs) {
    if (slot < 0 || slot > 1 || !nets[slot]) throw CaError(CA_ERR_STATE, "net slot not set");
    callback.need_none_failed("ca_trainer_net_forward");
    CoNet *net = nets[slot].get();
    if (n < 0 || (size_t)n > net->max_rows()) throw CaError(CA_ERR_ARG, "net_forward: more rows than num_games*searches_per_eval");
    if (n == 0) return;
    net_used = true;
    host_forward.forward(net, states, n, stream);
    if (net->callback_failed()) {
      rt_sync(stream);
      check_callback();
    }
    host_forward.results(n, evals, probs, stream);
    check_net_range();
  }

  /* kernel-only timing of a network on `rows` resident rows (HIP events on the engine's stream);
   * diagnostics and the per-kernel roofline of bench.py */
  float net_bench(int slot, const float *states, int32_t rows, int32_t reps) {
    if (slot < 0 || slot > 1 || !nets[slot]) throw CaError(CA_ERR_STATE, "net slot not set");
    if ((size_t)rows > std::min(nets[slot]->max_rows(), request_rows())) throw CaError(CA_ERR_ARG, "net_bench: too many rows");
    DevBuf<int32_t> d_n;
    d_n.alloc(1, stream);
    rt_h2d(d_n.p, &rows, 4, stream);
    host_forward.stage(states, rows, store.nn_in.p, stream);
    net_used = true;
    nets[slot]->forward(store.nn_in.p, rows, d_n.p, store.nn_eval.p, store.nn_probs.p, stream); /* warm */
    Event e0, e1;
    e0.create();
    e1.create();
    rt_event_record(e0, stream);
    for (int i = 0; i < reps; ++i) nets[slot]->forward(store.nn_in.p, rows, d_n.p, store.nn_eval.p, store.nn_probs.p, stream);
    rt_event_record(e1, stream);
    rt_sync(stream);
    return rt_event_elapsed_ms(e0, e1) / (float)reps;
  }

  void read_stats(ca_stats *out) {
    memset(out, 0, sizeof *out);
    add_game_sums(games(), out);
    out->peak_arena_units = store.peak_arena_units(stream);
    out->iterations = iterations;
    out->mcts_ms = stats.mcts_ms;
    out->nn_ms = stats.nn_ms;
    out->pack_ms = stats.pack_ms;
    out->mcts_launches = stats.mcts_launches;
    out->nn_launches = stats.nn_launches;
    out->nn_rows = stats.nn_rows;
    out->pools = fused.pools.empty() ? 1 : (int64_t)fused.pools.size();
    out->resident_slots = store.R;
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
    return games()[game];
  }

  void read_trace(int g, int32_t *out, int32_t cap, int32_t *n) {
    if (!cfg.trace) throw CaError(CA_ERR_STATE, "trace not enabled");
    int32_t len = game(g).trace_len;
    if (len > CO_TRACE_CAP) throw CaError(CA_ERR_ENGINE, "trace buffer overflow");
    *n = len;
    int32_t c = std::min(len, cap);
    if (out && c > 0) {
      rt_d2h(out, store.trace.p + (size_t)g * CO_TRACE_CAP, (size_t)c * 4, stream);
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
    stats.nn_rows = 0;
    for (const GameCtl &gc : games()) stats.nn_rows += gc.evals; /* every consumed row was requested once */
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
      const int R = store.R;
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
    const int R = store.R;
    Event ev[4];
    for (auto &e : ev) e.create();
    EngineParams e = params(0);
    e.arena_state = store.arena_state.p;
    e.row_counter = store.row_counter.p;
    int64_t it = 0;
    int32_t st[CO_AS_WORDS] = {};
    std::string failure;
    while (!finished && (max_iterations <= 0 || it < max_iterations)) {
      const bool timed = (it % poll) == poll - 1 || (max_iterations > 0 && it + 1 == max_iterations);
      e.iteration = trainer_iteration;
      e.scan_phase = 0;
      scan(e); /* offsets at entry (trainer.cpp:208-215) */
      if (timed) rt_event_record(ev[0], stream);
      launch_mcts_step(e, R, stream);
      if (timed) rt_event_record(ev[1], stream);
      e.scan_phase = 1;
      scan(e);
      compact(e);
      if (timed) rt_event_record(ev[2], stream);
      net_used = true;
      for (int slot = 0; slot < 2; ++slot) /* get_predictions, main.pyx:74-81 */
        nets[slot]->forward(store.nn_in.p, R * spe, store.arena_state.p + CO_AS_ROWS + slot, store.nn_eval.p, store.nn_probs.p, stream);
      if (nets[0]->callback_failed() || nets[1]->callback_failed()) break; /* (a caller-supplied network: nothing more is queued) */
      if (timed) rt_event_record(ev[3], stream);
      ++iterations;
      ++it;
      ++stats.mcts_launches;
      ++stats.nn_launches;
      if (timed) {
        int32_t d = 0;
        rt_d2h(&d, store.all_done.p, 4, stream);
        rt_d2h(st, store.arena_state.p, sizeof st, stream);
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
    rt_d2h(st, store.arena_state.p, sizeof st, stream);
    rt_sync(stream);
    invalidate();
    stats.estimate_device_times(false);
    check_callback();
    if (!failure.empty()) throw CaError(CA_ERR_ENGINE, failure);
    pack(st[CO_AS_MODEL]); /* refresh the done flag and the batch description */
    check_errors();
    unsigned long long rows = 0;
    rt_d2h(&rows, store.row_counter.p, 8, stream);
    rt_sync(stream);
    stats.nn_rows = (int64_t)rows;
    stats.nn_rows_evaluated = stats.nn_rows;
    return finished;
  }
};

#include "tourney_host.h"

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
extern "C" int ca_trainer_num_samples(ca_trainer *t, int32_t *out) { return co_guard(t, [&] { *out = num_samples(t->games()); }); }
extern "C" int ca_trainer_score(ca_trainer *t, float *out) { return co_guard(t, [&] { *out = score(t->games(), t->cfg.game_base); }); }
extern "C" int ca_trainer_avg_mate_length(ca_trainer *t, float *out) { return co_guard(t, [&] { *out = avg_mate_length(t->games()); }); }
extern "C" int ca_trainer_write_requests(ca_trainer *t, float *gs, int to_play) {
  return co_guard(t, [&] { t->write_requests(gs, norm_to_play(to_play)); });
}
extern "C" int ca_trainer_write_samples(ca_trainer *t, float *gs, float *ev, float *pr) {
  return co_guard(t, [&] { t->write_samples(gs, ev, pr); });
}
extern "C" int ca_trainer_write_scores(ca_trainer *t, const char *file) { return co_guard(t, [&] { write_scores(t->games(), file); }); }
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
    *rows = (int32_t)t->request_rows();
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
  return co_guard(t, [&] { *pinned = t->pins.pin(p, bytes) ? 1 : 0; });
}
extern "C" int ca_trainer_unpin_host(ca_trainer *t, void *p) { return co_guard(t, [&] { t->pins.unpin(p); }); }
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
/* diagnostic builds (-DCO_PROF), see GameStore::read_prof; not in the public header */
extern "C" int ca_trainer_prof(ca_trainer *t, unsigned long long out[2 * CO_NPROF + 24]) {
  return co_guard(t, [&] { t->store.read_prof(out, t->stream); });
}

extern "C" int ca_trainer_net_forward(ca_trainer *t, int slot, const float *states, int32_t n, float *evals, float *probs) {
  return co_guard(t, [&] { t->net_forward_host(slot, states, n, evals, probs); });
}
extern "C" int ca_trainer_net_bench(ca_trainer *t, int slot, const float *states, int32_t rows, int32_t reps, float *ms_per_call) {
  return co_guard(t, [&] { *ms_per_call = t->net_bench(slot, states, rows, reps); });
}

extern "C" int ca_trainer_stats(ca_trainer *t, ca_stats *out) { return co_guard(t, [&] { t->read_stats(out); }); }
extern "C" int ca_trainer_game_info(ca_trainer *t, int game, int32_t out[8]) { return co_guard(t, [&] { game_info(t->game(game), out); }); }
extern "C" int ca_trainer_trace(ca_trainer *t, int game, int32_t *out, int32_t cap, int32_t *n) {
  return co_guard(t, [&] { t->read_trace(game, out, cap, n); });
}

#include "probes.h"
