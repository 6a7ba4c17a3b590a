// analysis_host.h -- the positions of an analysis trainer (ca_config.analyse: DockerMC constructor arguments, one per
// game): their decoding and validation, how a generation's slots start from them, and the eight result words per position
// at the head of each slot's request area -- written here for a position that is terminal as given, by the search kernel
// (search_move.h co_analyse_finish) for every other, decoded here for ca_trainer_analysis.
#pragma once
#include <string>
#include <vector>

#include "host.h"
#include "kernels.h"

struct AnalysisPositions {
  std::vector<uint32_t> pos;  /* [G][3] board lo, board hi, meta */
  std::vector<uint32_t> seed; /* [G] */
  std::vector<int32_t> pre;   /* [G] Node result of a position that is terminal as given, else 0 */

  bool given() const { return !pos.empty(); }

  void set(const int32_t *boards, const int32_t *to_play, const int32_t *pieces, const int32_t *seeds, int G, rt_stream_t s) {
    pos.assign((size_t)3 * G, 0u);
    seed.assign(G, 0u);
    pre.assign(G, 0);
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
      pos[3 * g] = (uint32_t)b;
      pos[3 * g + 1] = (uint32_t)(b >> 32);
      pos[3 * g + 2] = meta;
      seed[g] = (uint32_t)seeds[g];
      hb[g] = b;
      hm[g] = meta;
    }
    /* Node result of every given position (node.cpp:256-271), by the rule kernel */
    DevBuf<uint64_t> db;
    DevBuf<uint32_t> dm, dk;
    DevBuf<int32_t> dl;
    db.upload(hb.data(), G, s); dm.upload(hm.data(), G, s); dk.alloc((size_t)G * 3, s); dl.alloc(G, s);
    RT_LAUNCH(co_k_rules_batch, G, CO_WAVE, s, (const uint64_t *)db.p, (const uint32_t *)dm.p, G, dk.p, dl.p);
    std::vector<uint32_t> mk((size_t)G * 3);
    std::vector<int32_t> ln(G);
    rt_d2h(mk.data(), dk.p, mk.size() * 4, s);
    rt_d2h(ln.data(), dl.p, ln.size() * 4, s);
    rt_sync(s);
    for (int g = 0; g < G; ++g)
      if ((mk[3 * g] | mk[3 * g + 1] | mk[3 * g + 2]) == 0u) pre[g] = ln[g] ? CO_RESULT_LOSS : CO_RESULT_DRAW;
  }

  /* slot g of a new generation starts from position g */
  void place(GameCtl &gc, int g) const {
    gc.parity = 0;
    gc.pos_lo = pos[3 * g];
    gc.pos_hi = pos[3 * g + 1];
    gc.pos_meta = pos[3 * g + 2];
    if (pre[g]) gc.done = 1; /* choose_move.pyx:194-197: a terminal position is not searched */
  }

  /* ---- the result words r[0..7] of a position: {move (-1: none), Node result, nodes, evaluation bits, legal-move mask
   * [3] of the new position, 1 = written}.  `req`: the slots' request areas, `row_floats` apart */
  /* result rows of the positions that were terminal as given; the others' cleared (queued on s) */
  void write_terminal_rows(float *req, size_t row_floats, rt_stream_t s) const {
    const size_t G = pre.size();
    std::vector<uint32_t> rows(G * row_floats, 0u);
    for (size_t g = 0; g < G; ++g)
      if (pre[g]) {
        uint32_t *o = &rows[g * row_floats];
        o[0] = 0xFFFFFFFFu;
        o[1] = (uint32_t)pre[g];
        o[2] = 1u;
        o[7] = 1u;
      }
    rt_h2d(req, rows.data(), rows.size() * 4, s);
  }
  /* out[g][8] as ca_trainer_analysis documents it; `games`: GameView::fetch */
  static void read(const float *req, size_t row_floats, const std::vector<GameCtl> &games, int32_t *out, rt_stream_t s) {
    const size_t G = games.size();
    std::vector<uint32_t> rows(G * 8);
    rt_d2h_2d(rows.data(), 32, req, row_floats * 4, 32, G, s); /* one strided copy */
    rt_sync(s);
    for (size_t g = 0; g < G; ++g) {
      const uint32_t *r = &rows[g * 8];
      int32_t *o = out + g * 8;
      if (!games[g].done || r[7] != 1u) throw CaError(CA_ERR_STATE, "analysis: search of position " + std::to_string(g) + " is not finished");
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
};
