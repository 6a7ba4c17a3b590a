// game_view.h -- the host's copy of a trainer's games (GameCtl by GAME index, whatever slot a game was played in) and what
// is read off it: scores, sample counts, statistics, the games' error bits.
#pragma once
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "game_store.h"

struct GameView {
  std::vector<GameCtl> games;
  bool valid = false; /* false: the device has moved on since the copy */

  /* games[i] = control block of GAME i of the trainer: the slot itself without recycling; else the filed
   * result of a finished game, the slot of a game in play, or an untouched block for a game not yet started */
  const std::vector<GameCtl> &fetch(const GameStore &store, int G, rt_stream_t s) {
    if (valid) return games;
    const int R = store.R;
    games.resize(G);
    if (!store.recycle) {
      rt_d2h(games.data(), store.games.p, (size_t)G * sizeof(GameCtl), s);
      rt_sync(s);
    } else {
      std::vector<GameCtl> slots(R);
      rt_d2h(slots.data(), store.games.p, (size_t)R * sizeof(GameCtl), s);
      rt_d2h(games.data(), store.results.p, (size_t)G * sizeof(GameCtl), s);
      rt_sync(s);
      for (int i = 0; i < G; ++i)
        if (!games[i].done) {
          memset(&games[i], 0, sizeof(GameCtl));
          games[i].gid = i;
        }
      for (int sl = 0; sl < R; ++sl) {
        const int i = slots[sl].gid;
        if (i >= 0 && i < G && !games[i].done) games[i] = slots[sl];
      }
    }
    valid = true;
    return games;
  }
};

/* ---- read off the games `g` of a trainer (GameView::fetch) */

/* the first game with an error bit set ends the call */
inline void throw_game_errors(const std::vector<GameCtl> &g) {
  for (size_t i = 0; i < g.size(); ++i)
    if (g[i].error) {
      char buf[256];
      int e = g[i].error;
      snprintf(buf, sizeof buf, "game %d reported engine error 0x%x (%s%s%s%s)", (int)i, e,
               (e & CO_ERR_ARENA_FULL) ? "search-tree arena full: raise ca_config.arena_units; " : "",
               (e & CO_ERR_PATH_TOO_DEEP) ? "search path deeper than CO_PATH_MAX; " : "",
               (e & CO_ERR_TOO_MANY_PLIES) ? "game longer than CO_MAX_PLIES; " : "",
               (e & CO_ERR_INTERNAL) ? "internal inconsistency; " : "");
      throw CaError(CA_ERR_ENGINE, buf);
    }
}

inline bool all_games_done(const std::vector<GameCtl> &g) {
  for (const GameCtl &gc : g)
    if (!gc.done) return false;
  return true;
}

inline int32_t num_samples(const std::vector<GameCtl> &g) {
  int32_t n = 0;
  for (const GameCtl &gc : g) n += gc.n_samples;
  return n;
}

/* SelfPlayer::score (selfplayer.cpp:57-64) + Trainer::score (trainer.cpp:59-68) */
inline float game_score(const GameCtl &gc) {
  if (gc.result == CO_RESULT_LOSS) return 0.0f;
  if (gc.result == CO_RESULT_WIN) return 1.0f;
  return 0.5f;
}
inline float score(const std::vector<GameCtl> &g, int game_base) {
  /* colour alternates with the GLOBAL game index (trainer.cpp:61-66) */
  float s = 0;
  for (size_t i = 0; i < g.size(); ++i)
    if ((game_base + (int)i) % 2 == 0) s += game_score(g[i]);
  for (size_t i = 0; i < g.size(); ++i)
    if ((game_base + (int)i) % 2 == 1) s = (float)((double)s + (1.0 - (double)game_score(g[i])));
  return s / (float)g.size();
}
inline float avg_mate_length(const std::vector<GameCtl> &g) {
  int32_t total = 0;
  for (const GameCtl &gc : g) total += gc.mate_turn == 0 ? 0 : gc.n_samples - gc.mate_turn + 1; /* selfplayer.cpp:66-71 */
  return (float)total / (float)g.size();
}

/* Trainer::writeScores (trainer.cpp:115-162) */
inline void write_scores(const std::vector<GameCtl> &g, const char *file) {
  size_t n = g.size();
  std::vector<float> scores(n);
  for (size_t i = 0; i < n; i += 2) scores[i] = game_score(g[i]);
  for (size_t i = 1; i < n; i += 2) scores[i] = (float)(1.0 - (double)game_score(g[i]));
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

/* the per-game sums of ca_stats */
inline void add_game_sums(const std::vector<GameCtl> &g, ca_stats *out) {
  for (const GameCtl &gc : g) {
    out->searches += gc.searches;
    out->evals += gc.evals;
    out->nodes += gc.nodes;
    out->plies += gc.plies;
  }
}

/* out[8] = {side to move, done, result, samples, pending requests, error, mate turn, plies} */
inline void game_info(const GameCtl &gc, int32_t out[8]) {
  out[0] = gc.to_play; out[1] = gc.done; out[2] = gc.result; out[3] = gc.n_samples;
  out[4] = gc.done ? 0 : gc.n_pending; out[5] = gc.error; out[6] = gc.mate_turn; out[7] = gc.plies;
}
