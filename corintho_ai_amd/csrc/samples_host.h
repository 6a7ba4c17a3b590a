// samples_host.h -- the three ways a finished generation's samples leave a trainer (Trainer::writeSamples with the eight
// symmetries, un-augmented rows to the host, un-augmented rows into device memory) on staging buffers kept between calls,
// and the host's own symmetry expansion of gathered rows (ca_expand_samples).
#pragma once
#include <vector>

#include "host.h"
#include "kernels.h"

struct SampleExits {
  DevBuf<int32_t> ws_off; /* {sample offsets [G + 1], per game (plies | result << 8) [G]}: the sample kernels work by game, not by slot */
  DevBuf<float> ws_gs, ws_ev, ws_pr;

  /* the index of the samples of `games` (GameView::fetch) uploaded; returns their number -- nothing is uploaded when
   * there are none or more than `cap_rows` */
  int32_t index(const std::vector<GameCtl> &games, int32_t cap_rows, rt_stream_t s) {
    const size_t G = games.size();
    std::vector<int32_t> idx(2 * G + 1, 0);
    for (size_t g = 0; g < G; ++g) {
      idx[g + 1] = idx[g] + games[g].n_samples;
      idx[G + 1 + g] = games[g].n_samples | (games[g].result << 8);
    }
    if (idx[G] == 0 || idx[G] > cap_rows) return idx[G];
    ws_off.grow(idx.size(), s);
    rt_h2d(ws_off.p, idx.data(), idx.size() * 4, s);
    rt_sync(s); /* idx is a local */
    return idx[G];
  }
  const int32_t *meta(int G) const { return ws_off.p + G + 1; }

  /* the calls below follow index() on the same games: n = what it returned (> 0), P and G the trainer's */
  void write(const EngineParams &P, int G, size_t n, float *gs, float *ev, float *pr, rt_stream_t s) {
    ws_gs.grow(n * 8 * CO_GAME_STATE_SIZE, s);
    ws_ev.grow(n * 8, s);
    ws_pr.grow(n * 8 * CO_NUM_MOVES, s);
    RT_LAUNCH(co_k_write_samples, G, CO_WAVE, s, P, G, (const int32_t *)ws_off.p, meta(G), ws_gs.p, ws_ev.p, ws_pr.p);
    rt_d2h(gs, ws_gs.p, n * 8 * CO_GAME_STATE_SIZE * 4, s);
    rt_d2h(ev, ws_ev.p, n * 8 * 4, s);
    rt_d2h(pr, ws_pr.p, n * 8 * CO_NUM_MOVES * 4, s);
    rt_sync(s);
  }
  /* un-augmented samples packed on the device into device memory: the caller's (the multi-GPU gather hands these
   * straight to RCCL), or export_host's staging buffers */
  void pack(const EngineParams &P, int G, float *d_state_policy, float *d_outcome, rt_stream_t s) {
    RT_LAUNCH(co_k_pack_samples, G, CO_WAVE, s, P, G, (const int32_t *)ws_off.p, meta(G), d_state_policy, d_outcome);
  }
  void export_host(const EngineParams &P, int G, size_t n, float *state_policy, float *outcome, rt_stream_t s) {
    ws_gs.grow(n * CO_SAMPLE_FLOATS, s);
    ws_ev.grow(n, s);
    pack(P, G, ws_gs.p, ws_ev.p, s);
    rt_d2h(state_policy, ws_gs.p, n * CO_SAMPLE_FLOATS * 4, s);
    rt_d2h(outcome, ws_ev.p, n * 4, s);
    rt_sync(s);
  }
};

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
