// tourney_host.h -- Tourney (tourney.cpp) on a trainer's pool: its matches are the games of one ca_trainer, one match per
// slot (game_store.h TourneyTables), built at the first query after the last addMatch; the reference's protocol and the
// fused rounds on the trainer's primitives, and the tournament's C ABI.  Included by engine.hip behind ca_trainer.
#pragma once
#include <fstream>
#include <map>
#include <random>

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
  /* ca_tourney_set_grouped: a round serves every model at once -- one scan, one compaction, one grouped network launch
   * (nn_group.h) and one search launch, whatever the number of models.  With exact offsets a match reads its own rows,
   * so its play depends on nothing but its own evaluations and the order in which matches are stepped does not matter. */
  bool grouped = false;
  int path_ran = 0;                            /* ca_stats.tourney_path: the path ca_tourney_run last took */
  std::unique_ptr<CoNetGroup> group;           /* the models of group_ids, in that order */
  std::vector<int> group_ids;
  GroupPlanner planner;
  DevBuf<int32_t> slot_model, row_model;       /* [2 matches] dense model of a match's side (< 0: random); [request rows] */

  /* Tourney::doIteration (tourney.cpp:53-70).  `rows` = rows of the caller's two arrays: the
   * reference reads them at its own offset table (quirk 10), so the whole arrays travel. */
  void do_iteration(const float *evals, const float *probs, int32_t rows, int id) {
    ca_trainer &p = built();
    const int32_t cap = (int32_t)p.request_rows();
    if (rows < 0 || rows > cap) rows = cap;
    const EngineParams e = p.params(id);
    p.scan(e); /* offsets at entry */
    p.upload_answers(evals, probs, rows);
    ++p.iterations;
    p.step(e);
  }

  /* The loop of rating/tourney.pyx:122-160 with the networks on the GPU: for every model id in
   * ascending order, pack that model's requests (Tourney::writeRequests), evaluate them, iterate
   * its matches (Tourney::doIteration, which reads the evaluations through the reference's offset
   * table); a random player's dummy id (< 0) has nothing to evaluate.  The evaluation arrays persist
   * between rounds like the driver's, so the result is the one the compat protocol gives with the
   * same networks. */
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
    /* grouped: every model must be one of the library's kinds (a caller's function evaluates its own launch), and one
     * kind for all; models of several kinds are served by the per-model path */
    bool use_group = grouped;
    if (grouped) {
      int kind = 0;
      for (int id : ids) {
        if (id < 0) continue;
        auto it = net_specs.find(id);
        if (it == net_specs.end()) throw CaError(CA_ERR_STATE, "ca_tourney_run: no network for model id " + std::to_string(id));
        if (it->second.f.fn)
          throw CaError(CA_ERR_STATE, "ca_tourney_run: a grouped tournament evaluates every model in one launch of the library's kernels; model id " +
                                          std::to_string(id) + " is a caller-supplied function (ca_tourney_set_net_fn)");
        if (kind && it->second.kind != kind) use_group = false;
        kind = it->second.kind;
      }
      if (!kind) use_group = false; /* (random players only) */
      /* more rows or models than the grouping kernel's tables hold: the per-model path, which has no such limit */
      int n_models = 0;
      for (int id : ids) n_models += id >= 0;
      if (p.request_rows() > CO_GROUP_MAX_ROWS || n_models > CO_GROUP_MAX_MODELS) use_group = false;
    }
    for (int id : ids) {
      if (id < 0 || use_group) continue;
      if (!nets.count(id)) {
        auto it = net_specs.find(id);
        if (it == net_specs.end()) throw CaError(CA_ERR_STATE, "ca_tourney_run: no network for model id " + std::to_string(id));
        nets[id] = p.make_net(it->second, &callback, " for model id " + std::to_string(id) + ", this tournament");
      }
    }
    if (use_group) return run_grouped(p, ids, max_rounds);
    path_ran = 1;
    int64_t rounds = 0;
    bool done = all_games_done(p.games());
    int failed_id = -1;
    while (!done && (max_rounds <= 0 || rounds < max_rounds)) {
      for (int id : ids) {
        p.queue_iteration(p.params(id), id >= 0 ? nets[id].get() : nullptr);
        if (id >= 0 && nets[id]->callback_failed()) { /* (a caller-supplied network: nothing more is queued) */
          failed_id = id;
          break;
        }
      }
      if (failed_id >= 0) break;
      ++rounds;
      /* the host looks at the all-done flag every eighth round only (a round that finds every match
       * finished launches kernels that return at once), so the queue never runs dry in between */
      if ((rounds & 7) == 0 || (max_rounds > 0 && rounds >= max_rounds)) done = p.poll_all_done(ids.front());
    }
    if (failed_id >= 0) {
      p.drain();
      callback.check(nets[failed_id].get(), "model id " + std::to_string(failed_id));
    }
    p.queued_iterations_done();
    if (done) all_done(); /* (writes the match logs) */
    return done;
  }

  /* the rounds of a grouped tournament (ca_tourney_set_grouped) */
  bool run_grouped(ca_trainer &p, const std::vector<int> &ids, int64_t max_rounds) {
    std::vector<int> models;
    for (int id : ids)
      if (id >= 0) models.push_back(id);
    if (!group || models != group_ids) {
      std::vector<const float *> w;
      size_t n_floats = 0;
      for (int id : models) {
        const NetSpec &sp = net_specs.at(id);
        const size_t n = sp.weights ? sp.n_floats : sp.kept.size();
        if (n_floats && n != n_floats) throw CaError(CA_ERR_ARG, "ca_tourney_run: model id " + std::to_string(id) + " has another weight count than the models before it");
        n_floats = n;
        w.push_back(sp.weights ? sp.weights : sp.kept.data());
      }
      const size_t rows = p.request_rows();
      group = co_net_group_make(net_specs.at(models[0]).kind, w.data(), (int)models.size(), n_floats, rows, p.stream);
      planner.create((int)models.size(), rows, !group->grouped_kernel(), p.stream, group->tile());
      std::vector<int32_t> sm;
      for (auto &m : matches)
        for (int pid : {m.first, m.second}) {
          const int id = players.at(pid).model_id;
          sm.push_back(id < 0 ? -1 : (int32_t)(std::find(models.begin(), models.end(), id) - models.begin()));
        }
      slot_model.upload(sm.data(), sm.size(), p.stream);
      row_model.alloc(rows, p.stream);
      rt_sync(p.stream); /* (sm leaves scope) */
      group_ids = models;
    }
    path_ran = 2;
    int64_t rounds = 0;
    bool done = all_games_done(p.games());
    while (!done && (max_rounds <= 0 || rounds < max_rounds)) {
      p.queue_grouped_iteration(group.get(), planner, slot_model.p, row_model.p);
      ++rounds;
      /* (the look every eighth round: see run) */
      if ((rounds & 7) == 0 || (max_rounds > 0 && rounds >= max_rounds)) done = p.poll_all_done(CO_TO_PLAY_EVERY_MODEL);
    }
    p.queued_iterations_done();
    std::string names = "model ids";
    for (int id : models) names += " " + std::to_string(id);
    check_group_range(group.get(), p.stream, "ca_tourney_run", names);
    if (done) all_done();
    return done;
  }

  /* Tourney::all_done (tourney.cpp:14-21); the log files of the matches are written the first time it is true */
  bool all_done() {
    ca_trainer &p = built();
    const bool done = all_games_done(p.games());
    if (done && !seen_done) {
      seen_done = true;
      p.write_logs_once();
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
    TourneyTables tables;
    tables.match_seeds = seeds;
    tables.exact_offsets = exact_offsets;
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
        tables.host_pcfg.push_back(p);
        if (!p.random) {
          c.max_searches = std::max(c.max_searches, p.max_searches);
          c.searches_per_eval = std::max(c.searches_per_eval, p.searches_per_eval);
        }
      }
    }
    auto t = std::make_unique<ca_trainer>();
    t->init(c, std::move(tables));
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
    if (model_id == CO_TO_PLAY_EVERY_MODEL) throw CaError(CA_ERR_ARG, "addPlayer: this model id is reserved");
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
  t->group.reset(); /* (rebuilt by the next grouped run) */
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
    if (t->grouped && !on) throw CaError(CA_ERR_STATE, "set_exact_offsets: a grouped tournament (ca_tourney_set_grouped) needs exact offsets");
    t->exact_offsets = on != 0;
  });
}
/* the generator addMatch draws the matches' seeds from (tourney.h:43: default constructed, seed 5489), seeded anew */
extern "C" int ca_tourney_set_seed(ca_tourney *t, uint32_t seed) {
  return co_guard(t, [&] {
    if (!t->matches.empty()) throw CaError(CA_ERR_STATE, "set_seed after the first addMatch");
    t->generator.seed(seed);
  });
}
extern "C" int ca_tourney_set_grouped(ca_tourney *t, int32_t on) {
  return co_guard(t, [&] {
    if (t->pool) throw CaError(CA_ERR_STATE, "set_grouped after the tournament has started");
    t->grouped = on != 0;
    if (on) t->exact_offsets = true;
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
  return co_guard(t, [&] { t->do_iteration(evaluations, probabilities, rows, id); });
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
    *out = game_score(t->built().game(match, "match index out of range")); /* Match::score, match.cpp:52-58 */
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
      if (gc.done) f << t->matches[g].first << ' ' << t->matches[g].second << ' ' << game_score(gc) << '\n';
    }
  });
}
/* the trace and the statistics of the tournament's trainer; a tournament that cannot be built is CA_ERR_STATE here */
extern "C" int ca_tourney_trace(ca_tourney *t, int32_t match, int32_t *out, int32_t cap, int32_t *n_out) {
  return co_guard(t, [&] { t->built_or_state().read_trace(match, out, cap, n_out); });
}
extern "C" int ca_tourney_stats(ca_tourney *t, ca_stats *out) {
  return co_guard(t, [&] {
    t->built_or_state().read_stats(out);
    out->tourney_path = t->path_ran;
  });
}
