// nn_group.h -- rows of many models of one kind through ONE network launch (nn.h CoNetGroup): the grouping kernels that
// turn "row r belongs to model m" into the index list and the workgroup table of a grouped launch, on the device; the
// buffers they fill (GroupPlanner); the generic fallback, one CoNet::forward per model segment on the same index lists,
// for kinds without a grouped kernel and for the emulation build; ca_net_group and its C ABI.  Included by engine.hip.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "net_host.h"

/* ---- kernels (wave style, wave.h: they run in the emulation build too) */
struct CoGroupArgs {
  const int32_t *row_model; /* [rows] dense model index of every row; outside 0 .. models - 1: the row is in no segment */
  const int32_t *d_rows;    /* the batch's row count, on the device */
  int32_t rows_cap, models, tile, seg_stride, wg_cap;
  int32_t *idx;
  CoGroupWG *wg;
  int32_t *n_wg, *seg_start, *seg_count;
};
#define CO_GROUP_HS (CO_WAVE + 1) /* lanes of one model's counters, padded by one: the per-model passes read them lane-parallel */

/* the 64 values of `v` (an LDS array) -> each lane's exclusive prefix, the total returned: 64 uniform additions */
#define CO_GROUP_LANE_SCAN(v, base, total) \
  {                                        \
    total = 0;                             \
    FOR_LANES { L(base) = 0; }             \
    for (int l_ = 0; l_ < CO_WAVE; ++l_) { \
      const int v_ = v[l_];                \
      FOR_LANES {                          \
        if (lane == l_) L(base) = total;   \
      }                                    \
      total += v_;                         \
    }                                      \
  }

/* A stable counting sort of the rows by model, by a single wavefront.  Lane l owns the contiguous rows
 * [l chunk, (l + 1) chunk) and column l of the counters, model m the 64 counters hist[m][.]: the order (model, lane, row
 * within the lane's chunk) IS (model, row).  Nothing is decided by an atomic: the tables are the same bits every run.
 * Lane l also owns the models [l K, (l + 1) K) in the passes that go by model. */
CO_KERNEL co_k_group(CoGroupArgs A) {
  WG_SHARED(uint16_t, hist, CO_GROUP_MAX_MODELS * CO_GROUP_HS);
  WG_SHARED(int32_t, cnt, CO_GROUP_MAX_MODELS);  /* rows of model m */
  WG_SHARED(int32_t, segb, CO_GROUP_MAX_MODELS); /* where its segment starts in idx */
  WG_SHARED(int32_t, lsum, CO_WAVE);
  int rows = A.d_rows[0];
  rows = rows < 0 ? 0 : rows > A.rows_cap ? A.rows_cap : rows;
  const int M = A.models, chunk = (rows + CO_WAVE - 1) / CO_WAVE, K = (M + CO_WAVE - 1) / CO_WAVE;
  FOR_LANES {
    for (int m = 0; m < M; ++m) hist[m * CO_GROUP_HS + lane] = 0;
  }
  WAVE_SYNC();
  FOR_LANES {
    for (int i = 0; i < chunk; ++i) {
      const int r = lane * chunk + i;
      if (r < rows) {
        const int m = A.row_model[r];
        if (m >= 0 && m < M) hist[m * CO_GROUP_HS + lane] = (uint16_t)(hist[m * CO_GROUP_HS + lane] + 1);
      }
    }
  }
  WAVE_SYNC();
  /* by model: the counters become the exclusive prefix over the lanes, their sum the model's rows */
  FOR_LANES {
    int s = 0;
    for (int j = 0; j < K; ++j) {
      const int m = lane * K + j;
      if (m < M) {
        int run = 0;
        for (int l = 0; l < CO_WAVE; ++l) {
          const int v = hist[m * CO_GROUP_HS + l];
          hist[m * CO_GROUP_HS + l] = (uint16_t)run;
          run += v;
        }
        cnt[m] = run;
        s += run;
      }
    }
    lsum[lane] = s;
  }
  WAVE_SYNC();
  LV(int, base);
  int total;
  CO_GROUP_LANE_SCAN(lsum, base, total)
  WAVE_SYNC();
  FOR_LANES {
    int s = L(base), w = 0;
    for (int j = 0; j < K; ++j) {
      const int m = lane * K + j;
      if (m < M) {
        const int at = A.seg_stride ? m * A.seg_stride : s;
        segb[m] = at;
        A.seg_start[m] = at;
        A.seg_count[m] = cnt[m];
        s += cnt[m];
        w += (cnt[m] + A.tile - 1) / A.tile;
      }
    }
    lsum[lane] = w;
  }
  WAVE_SYNC();
  /* the index list: a row goes to its model's segment, behind the rows of the lanes in front and its lane's earlier ones */
  FOR_LANES {
    for (int i = 0; i < chunk; ++i) {
      const int r = lane * chunk + i;
      if (r < rows) {
        const int m = A.row_model[r];
        if (m >= 0 && m < M) {
          const int at = hist[m * CO_GROUP_HS + lane];
          hist[m * CO_GROUP_HS + lane] = (uint16_t)(at + 1);
          A.idx[segb[m] + at] = r;
        }
      }
    }
  }
  /* the workgroup table: ceil(rows of m / tile) entries per model, in model order */
  CO_GROUP_LANE_SCAN(lsum, base, total)
  FOR_LANES {
    int w = L(base);
    for (int j = 0; j < K; ++j) {
      const int m = lane * K + j;
      if (m < M) {
        for (int o = 0; o < cnt[m]; o += A.tile) {
          if (w < A.wg_cap) {
            CoGroupWG e;
            e.model = m;
            e.first = segb[m] + o;
            e.count = cnt[m] - o < A.tile ? cnt[m] - o : A.tile;
            e.pad = 0;
            A.wg[w] = e;
          }
          ++w;
        }
      }
    }
    if (lane == 0) A.n_wg[0] = total < A.wg_cap ? total : A.wg_cap;
  }
}

/* a tournament's batch (co_k_scan and co_k_compact for every model at once): the rows of match g are its pending
 * requests, their model the one of the player to move; slot_model[2 g + side] is its dense index (< 0: a random player,
 * who asks for nothing).  One wavefront per match. */
CO_KERNEL co_k_group_rows(EngineParams P, const int32_t *slot_model, int32_t *row_model) {
  const int g = CO_BLOCK_IDX;
  if (g >= P.num_games) return;
  const GameCtl gc = P.games[g];
  if (!co_game_active(P, g, gc, P.to_play)) return;
  const int m = slot_model[2 * g + gc.to_play], n = gc.n_pending, at = P.req_offset[g];
  FOR_LANES {
    for (int i = lane; i < n; i += CO_WAVE) row_model[at + i] = m;
  }
}

/* ---- the tables of one launch and the kernel that fills them */
struct GroupPlanner {
  DevBuf<int32_t> idx, n_wg, seg_start, seg_count;
  DevBuf<CoGroupWG> wg;
  int32_t models = 0, rows_cap = 0, seg_stride = 0, wg_cap = 0, tile = CO_GROUP_TILE;

  /* strided: model m's segment at m * rows_cap (the fallback); else packed (a grouped kernel) */
  void create(int models_, size_t rows_cap_, bool strided, rt_stream_t s, int tile_ = CO_GROUP_TILE) {
    tile = tile_;
    if (models_ < 1 || models_ > CO_GROUP_MAX_MODELS)
      throw CaError(CA_ERR_ARG, "a network group holds 1 .. " + std::to_string(CO_GROUP_MAX_MODELS) + " models, not " + std::to_string(models_));
    if (rows_cap_ < 1 || rows_cap_ > CO_GROUP_MAX_ROWS)
      throw CaError(CA_ERR_ARG, "a network group's launch holds 1 .. " + std::to_string(CO_GROUP_MAX_ROWS) + " rows, not " + std::to_string(rows_cap_));
    models = models_;
    rows_cap = (int32_t)rows_cap_;
    seg_stride = strided ? rows_cap : 0;
    wg_cap = rows_cap / tile + models; /* the worst case: every model ends in a partial workgroup */
    idx.alloc(strided ? (size_t)models * rows_cap : (size_t)rows_cap, s);
    wg.alloc((size_t)wg_cap, s);
    n_wg.alloc(1, s);
    seg_start.alloc((size_t)models, s);
    seg_count.alloc((size_t)models, s);
  }
  CoGroupPlan plan() const {
    CoGroupPlan p;
    p.idx = idx.p, p.wg = wg.p, p.n_wg = n_wg.p, p.seg_start = seg_start.p, p.seg_count = seg_count.p;
    p.wg_cap = wg_cap, p.seg_stride = seg_stride;
    return p;
  }
  /* queued on s: the tables for the first d_rows[0] rows of row_model */
  void run(const int32_t *row_model, const int32_t *d_rows, rt_stream_t s) {
    CoGroupArgs a;
    a.row_model = row_model, a.d_rows = d_rows;
    a.rows_cap = rows_cap, a.models = models, a.tile = tile, a.seg_stride = seg_stride, a.wg_cap = wg_cap;
    a.idx = idx.p, a.wg = wg.p, a.n_wg = n_wg.p, a.seg_start = seg_start.p, a.seg_count = seg_count.p;
    RT_LAUNCH(co_k_group, 1, CO_WAVE, s, a);
  }
};

/* ---- the generic fallback: M networks, one CoNet::forward per model segment through the same index lists */
struct FallbackNetGroup : CoNetGroup {
  std::vector<std::unique_ptr<CoNet>> nets;
  int k = 0;
  size_t cap = 0;
  int kind() const override { return k; }
  int models() const override { return (int)nets.size(); }
  size_t max_rows() const override { return cap; }
  bool grouped_kernel() const override { return false; }
  void forward(const float *d_in, int32_t rows_cap, const CoGroupPlan &plan, float *d_eval, float *d_probs, rt_stream_t s) override {
    if (!plan.seg_stride) throw CaError(CA_ERR_STATE, "FallbackNetGroup: index lists without a fixed segment stride");
    for (size_t m = 0; m < nets.size(); ++m) {
      CoNetIO io;
      io.in_idx = io.out_idx = plan.idx + m * (size_t)plan.seg_stride;
      nets[m]->forward(d_in, rows_cap, plan.seg_count + m, d_eval, d_probs, s, io);
    }
  }
  bool range_exceeded(rt_stream_t s) override {
    bool any = false;
    for (auto &n : nets) any = n->range_exceeded(s) || any;
    return any;
  }
};

/* the group of `kind` on M weight sets for launches of up to max_rows rows: its grouped kernels where the kind has them,
 * else the fallback.  What is wrong with a weight set is reported with the model's index. */
static std::unique_ptr<CoNetGroup> co_net_group_make(int kind, const float *const *weights, int models, size_t n_floats, size_t max_rows,
                                                     rt_stream_t s) {
  if (models < 1 || models > CO_GROUP_MAX_MODELS)
    throw CaError(CA_ERR_ARG, "a network group holds 1 .. " + std::to_string(CO_GROUP_MAX_MODELS) + " models, not " + std::to_string(models));
  for (int m = 0; m < models; ++m)
    if (!weights || !weights[m]) throw CaError(CA_ERR_ARG, "network group: no weights for model " + std::to_string(m));
#ifndef CO_EMU
  try {
    if (CoNetGroup *g = co_net_group_native(kind, weights, models, n_floats, max_rows, s)) return std::unique_ptr<CoNetGroup>(g);
  } catch (const std::invalid_argument &e) {
    throw CaError(CA_ERR_ARG, e.what());
  }
#endif
  auto g = std::make_unique<FallbackNetGroup>();
  g->k = kind, g->cap = max_rows;
  for (int m = 0; m < models; ++m) {
    try {
      g->nets.push_back(NetSpec(kind, weights[m], n_floats).make(max_rows, s, nullptr));
    } catch (const CaError &e) {
      throw CaError(e.code, "model " + std::to_string(m) + " of the group: " + e.what());
    }
  }
  return g;
}

/* an f16x3 group met an operand beyond fp16's range: the flag is the launch's, so the error names its models */
static void check_group_range(CoNetGroup *g, rt_stream_t s, const std::string &who, const std::string &models) {
  if (g && g->range_exceeded(s))
    throw CaError(CA_ERR_ENGINE, who + ": an activation left the fp16 range of the f16x3 kernels (|x| > 65504) in a grouped launch of " + models +
                                     "; its evaluations are not valid -- use the float32-equivalent x6 kind of the same network");
}

/* ---- a group on host rows, without a trainer (ca_net_group_*) */
struct ca_net_group {
  int device = 0;
  Stream stream;
  std::unique_ptr<CoNetGroup> group;
  GroupPlanner planner;
  HostForward host;
  DevBuf<int32_t> row_model, d_n;
  int dev() const { return device; }

  void forward(const float *states, const int32_t *model_of_row, int32_t n, float *evals, float *probs) {
    if (n < 0 || (size_t)n > group->max_rows()) throw CaError(CA_ERR_ARG, "ca_net_group_forward: more rows than the group's max_rows");
    if (n == 0) return;
    if (!states || !model_of_row || !evals || !probs) throw CaError(CA_ERR_ARG, "ca_net_group_forward: null array");
    for (int32_t r = 0; r < n; ++r)
      if (model_of_row[r] < 0 || model_of_row[r] >= group->models())
        throw CaError(CA_ERR_ARG, "ca_net_group_forward: row " + std::to_string(r) + " names model " + std::to_string(model_of_row[r]) + " of " +
                                          std::to_string(group->models()));
    rt_stream_t s = stream;
    host.fw_ev.grow((size_t)n, s);
    host.fw_pr.grow((size_t)n * CO_NUM_MOVES, s);
    const float *rows = host.stage(states, n, nullptr, s);
    rt_h2d(row_model.p, model_of_row, (size_t)n * 4, s);
    rt_h2d(d_n.p, &n, 4, s);
    planner.run(row_model.p, d_n.p, s);
    group->forward(rows, n, planner.plan(), host.fw_ev.p, host.fw_pr.p, s);
    host.results(n, evals, probs, s);
    check_group_range(group.get(), s, "ca_net_group_forward", "models 0 .. " + std::to_string(group->models() - 1));
  }

  /* kernel-only times (HIP events on the group's stream) of `reps` launches on the same rows: out_ms[0] the grouping
   * kernel, out_ms[1] the network launch(es), per call */
  void bench(const float *states, const int32_t *model_of_row, int32_t n, int32_t reps, float *out_ms) {
    if (n < 1 || (size_t)n > group->max_rows() || reps < 1 || !out_ms)
      throw CaError(CA_ERR_ARG, "ca_net_group_bench: 1 .. max_rows rows, one or more repetitions");
    std::vector<float> ev((size_t)n), pr((size_t)n * CO_NUM_MOVES);
    forward(states, model_of_row, n, ev.data(), pr.data()); /* (checks the arrays, stages the rows, warms up) */
    rt_stream_t s = stream;
    Event e0, e1, e2;
    e0.create(), e1.create(), e2.create();
    rt_event_record(e0, s);
    for (int i = 0; i < reps; ++i) planner.run(row_model.p, d_n.p, s);
    rt_event_record(e1, s);
    for (int i = 0; i < reps; ++i) group->forward(host.fw_in.p, n, planner.plan(), host.fw_ev.p, host.fw_pr.p, s);
    rt_event_record(e2, s);
    rt_sync(s);
    out_ms[0] = rt_event_elapsed_ms(e0, e1) / (float)reps;
    out_ms[1] = rt_event_elapsed_ms(e1, e2) / (float)reps;
  }
};

extern "C" int ca_net_group_create(int device, int kind, const float *const *weights, int32_t models, size_t n_floats, int32_t max_rows,
                                   ca_net_group **out) {
  return on_device_stream(device, [&](Stream &s) {
    if (!out || !weights || max_rows <= 0) throw CaError(CA_ERR_ARG, "ca_net_group_create: null argument or max_rows < 1");
    *out = nullptr;
    auto g = std::make_unique<ca_net_group>();
    g->device = device;
    g->stream = std::move(s);
    g->group = co_net_group_make(kind, weights, models, n_floats, (size_t)max_rows, g->stream);
    g->planner.create(models, (size_t)max_rows, !g->group->grouped_kernel(), g->stream, g->group->tile());
    g->row_model.alloc((size_t)max_rows, g->stream);
    g->d_n.alloc(1, g->stream);
    rt_sync(g->stream);
    *out = g.release();
  });
}
extern "C" int ca_net_group_forward(ca_net_group *g, const float *states, const int32_t *model_of_row, int32_t n, float *evals, float *probs) {
  return co_guard(g, [&] { g->forward(states, model_of_row, n, evals, probs); });
}
extern "C" int ca_net_group_bench(ca_net_group *g, const float *states, const int32_t *model_of_row, int32_t n, int32_t reps, float out_ms[2]) {
  return co_guard(g, [&] { g->bench(states, model_of_row, n, reps, out_ms); });
}
extern "C" int ca_net_group_info(ca_net_group *g, int32_t out[6]) {
  return co_guard(g, [&] {
    const GroupPlanner &p = g->planner;
    out[0] = p.models, out[1] = p.rows_cap, out[2] = g->group->grouped_kernel() ? 1 : 0, out[3] = p.tile;
    out[4] = (int32_t)p.idx.n, out[5] = p.wg_cap;
  });
}
extern "C" int ca_net_group_tables(ca_net_group *g, int32_t *idx, int32_t *wg, int32_t *n_wg, int32_t *seg_start, int32_t *seg_count) {
  return co_guard(g, [&] {
    if (!idx || !wg || !n_wg || !seg_start || !seg_count) throw CaError(CA_ERR_ARG, "ca_net_group_tables: null array");
    const GroupPlanner &p = g->planner;
    rt_stream_t s = g->stream;
    rt_d2h(idx, p.idx.p, p.idx.n * 4, s);
    rt_d2h(wg, p.wg.p, (size_t)p.wg_cap * sizeof(CoGroupWG), s);
    rt_d2h(n_wg, p.n_wg.p, 4, s);
    rt_d2h(seg_start, p.seg_start.p, (size_t)p.models * 4, s);
    rt_d2h(seg_count, p.seg_count.p, (size_t)p.models * 4, s);
    rt_sync(s);
  });
}
extern "C" void ca_net_group_destroy(ca_net_group *g) { delete g; }
