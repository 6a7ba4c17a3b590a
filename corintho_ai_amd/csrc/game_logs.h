// game_logs.h -- the per-game text logs of a trainer: the records the search kernel fills (EngineParams::log), which games
// they belong to, and the files logfmt.h prints them into once every game is over.
#pragma once
#include <stdio.h>

#include <string>
#include <vector>

#include "host.h"
#include "logfmt.h"

struct GameLogs {
  DevBuf<int32_t> logbuf;         /* EngineParams::log */
  DevBuf<int32_t> log_index;      /* tournament: EngineParams::log_index */
  std::vector<int> game;          /* record k belongs to game game[k] ... */
  std::vector<std::string> paths; /* ... and goes to this file */
  int num_logged = 0;
  bool written = false;

  /* Trainer::initialize, trainer.cpp:243-250: game g of a shard writes `<folder>/game_<game_base + g>.txt` */
  static std::vector<std::string> game_paths(const char *folder, int game_base, int n) {
    std::vector<std::string> p;
    for (int g = 0; g < n; ++g) p.push_back(std::string(folder ? folder : "") + "/game_" + std::to_string(game_base + g) + ".txt");
    return p;
  }

  /* record k = game games[k] of G, printed to files[k]; with_index: the device finds a game's record through
   * EngineParams::log_index (tournament matches added with logging = true) instead of "the first num_logged games" */
  void set_records(const std::vector<int> &games, const std::vector<std::string> &files, bool with_index, int G, rt_stream_t s) {
    game = games;
    paths = files;
    num_logged = (int)games.size();
    logbuf.release();
    log_index.release();
    if (num_logged > 0) {
      logbuf.alloc((size_t)num_logged * CO_LOG_CAP, s);
      if (with_index) {
        std::vector<int32_t> idx((size_t)G, -1);
        for (int k = 0; k < num_logged; ++k) idx[(size_t)games[k]] = k;
        log_index.alloc((size_t)G, s);
        rt_h2d(log_index.p, idx.data(), idx.size() * 4, s);
      }
      rt_sync(s);
    }
    written = false;
  }
  void bind(EngineParams &P) const {
    P.log = logbuf.p;
    P.num_logged = num_logged;
    P.log_index = log_index.p;
  }

  /* a new generation: empty records, files to write again */
  void clear(rt_stream_t s) {
    if (logbuf.p) {
      rt_memset(logbuf.p, 0, (size_t)num_logged * CO_LOG_CAP * 4, s);
      rt_sync(s);
    }
    written = false;
  }

  bool pending() const { return logbuf.p && !written; }
  /* the files, once every game is over (the reference writes them as the games go; a file that cannot be opened is
   * skipped without a word there too: an ofstream in its fail state); `games`: GameView::fetch */
  void write(const std::vector<GameCtl> &games, rt_stream_t s) {
    written = true;
    std::vector<int32_t> rec((size_t)num_logged * CO_LOG_CAP);
    rt_d2h(rec.data(), logbuf.p, rec.size() * 4, s);
    rt_sync(s);
    for (int k = 0; k < num_logged; ++k) {
      const int32_t *r = rec.data() + (size_t)k * CO_LOG_CAP;
      if (r[0] < 0 || r[0] > CO_LOG_CAP - 1)
        throw CaError(CA_ERR_ENGINE, "text log " + paths[k] + " does not fit its record (" + std::to_string(r[0]) + " words)");
      FILE *f = fopen(paths[k].c_str(), "w");
      if (!f) continue;
      CoLogWriter wr(f);
      const bool ok = wr.write_game(r + 1, r[0], games[game[k]].result);
      fclose(f);
      if (!ok) throw CaError(CA_ERR_ENGINE, "malformed text-log record for " + paths[k]);
    }
  }
};
