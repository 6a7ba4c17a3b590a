// net_host.h -- the one way a network enters the engine (engine.hip: trainer, tournament, ca_net): what the caller named
// (NetSpec) becomes a CoNet in NetSpec::make; the two networks that are the caller's own code (HostNet on the host,
// ExternalNet on the device) with the row helpers they share, and the state of a handle whose networks call back.
#pragma once
#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "host.h"
#include "kernels.h"

/* ---- rows as the caller holds them (70 floats) and as the kernels read and write them */
/* d80[r] = d70[r] widened to the network kernels' CO_STATE_STRIDE floats, for r < rows */
static void expand_rows(const float *d70, float *d80, int rows, rt_stream_t s) {
  const int nb = std::min(rows * CO_STATE_STRIDE / CO_WAVE + 1, 1024);
  RT_LAUNCH(co_k_expand_rows, nb, CO_WAVE, s, d70, d80, rows, nb);
}
/* one thread per float (kernels.h co_k_host_rows_out / _in) */
static int host_rows_blocks(size_t floats) { return (int)((floats + CO_WAVE * CO_WAVES_PER_BLOCK - 1) / (CO_WAVE * CO_WAVES_PER_BLOCK)); }
/* out70[r] = request row in_idx[r] of `req` for r < d_rows[0], zero up to cap */
static void gather_rows(const float *req, const int32_t *in_idx, const int32_t *d_rows, int cap, float *out70, rt_stream_t s) {
  RT_LAUNCH(co_k_host_rows_out, host_rows_blocks((size_t)cap * CO_GAME_STATE_SIZE), CO_WAVE * CO_WAVES_PER_BLOCK, s, req, in_idx,
            (const uint32_t *)d_rows, cap, out70);
}
/* the answers to `rows` rows (and to no more than d_rows[0] of them; null: all) go where a network kernel writes through io */
static void scatter_rows(const float *evals, const float *probs, const int32_t *out_idx, const int32_t *d_rows, int rows, float *d_eval,
                         float *d_probs, int eval_stride, int probs_stride, rt_stream_t s) {
  RT_LAUNCH(co_k_host_rows_in, host_rows_blocks((size_t)rows * (1 + CO_NUM_MOVES)), CO_WAVE * CO_WAVES_PER_BLOCK, s, evals, probs, out_idx,
            (const uint32_t *)d_rows, rows, d_eval, d_probs, eval_stride, probs_stride);
}

/* nn.h range_exceeded: an f16x3 network met an operand beyond fp16's range -- its outputs since are NaN or wrong */
static void check_net_range(CoNet *net, rt_stream_t s, const std::string &who) {
  if (net && net->range_exceeded(s))
    throw CaError(CA_ERR_ENGINE, who + ": an activation left the fp16 range of the f16x3 kernels (|x| > 65504); the evaluations "
                                       "are not valid -- use the float32-equivalent x6 kind of the same network");
}

/* Host rows through a network (ca_trainer_net_forward, ca_trainer_net_bench): device buffers kept, and grown on demand,
 * between calls; the rows travel as the caller holds them (70 floats) and are widened to the kernels' 80 on the device */
struct HostForward {
  DevBuf<int32_t> fw_rows;
  DevBuf<float> fw_in70, fw_in, fw_ev, fw_pr;

  /* states[n][70] -> d80 (null: a buffer of this object's), widened; queued on s */
  float *stage(const float *states, int32_t n, float *d80, rt_stream_t s) {
    fw_in70.grow((size_t)n * CO_GAME_STATE_SIZE, s); /* (not the protocols' own row array: they hand that one to the caller) */
    if (!d80) fw_in.grow((size_t)n * CO_STATE_STRIDE, s), d80 = fw_in.p;
    rt_h2d(fw_in70.p, states, (size_t)n * CO_GAME_STATE_SIZE * 4, s);
    expand_rows(fw_in70.p, d80, n, s);
    return d80;
  }
  /* the n staged rows through `net`, the results left in fw_ev / fw_pr */
  void forward(CoNet *net, const float *states, int32_t n, rt_stream_t s) {
    fw_ev.grow((size_t)n, s);
    fw_pr.grow((size_t)n * CO_NUM_MOVES, s);
    fw_rows.grow(1, s);
    const float *rows = stage(states, n, nullptr, s);
    rt_h2d(fw_rows.p, &n, 4, s);
    net->forward(rows, n, fw_rows.p, fw_ev.p, fw_pr.p, s);
  }
  void results(int32_t n, float *evals, float *probs, rt_stream_t s) {
    rt_d2h(evals, fw_ev.p, (size_t)n * 4, s);
    rt_d2h(probs, fw_pr.p, (size_t)n * CO_NUM_MOVES * 4, s);
    rt_sync(s);
  }
};

/* ---- A handle whose networks may be the caller's functions (ca_net_fn): `in_callback` is what co_guard (host.h) refuses
 * entry points on while one of them runs; one that returned non-zero ends what the handle was doing for good */
struct CallbackState {
  bool in_callback = false;
  bool failed = false;
  const char *after_failure = ""; /* the owner's words for what cannot go on */

  /* `net` (null: none) has failed: CA_ERR_CALLBACK naming it, and every later need_none_failed refuses */
  void check(const CoNet *net, const std::string &which) {
    if (!net || !net->callback_failed()) return;
    failed = true;
    throw CaError(CA_ERR_CALLBACK, "the caller-supplied network function of " + which + " returned non-zero");
  }
  void need_none_failed(const char *who) const {
    if (failed) throw CaError(CA_ERR_STATE, std::string(who) + ": a caller-supplied network function failed" + after_failure);
  }
};

/* The "network" of the host-driven protocol with the evaluation cache (ca_trainer_set_host_cache): its forward pass is
 * the round trip to the caller.  forward() -- FusedRun queues it behind the search launch like any network -- gathers the
 * rows the cache could not resolve into a dense [n][70] array for Trainer::writeRequests and has the protocol's flags
 * (co_k_scan: all done, any error) copied to the host with them; receive(), queued in front of the NEXT search launch,
 * scatters the caller's answers to the elements of the cache's value array a network kernel would have written. */
struct HostNet : CoNet {
  /* the trainer's, set once */
  size_t rows_cap = 0;
  float *rows70 = nullptr;               /* [rows_cap][70] the rows to hand out */
  float *ev_in = nullptr, *pr_in = nullptr; /* [rows_cap], [rows_cap][96] the caller's answers on the device */
  int32_t *d_ctl = nullptr, *h_ctl = nullptr; /* EngineParams::ctl and its page-locked copy */
  EngineParams scan_params = {};         /* the games, for co_k_scan */
  /* of the last forward(): where the answers go */
  const int32_t *out_idx = nullptr;
  float *val = nullptr;

  size_t max_rows() const override { return rows_cap; }
  int kind() const override { return 0; }
  double flop_per_row() const override { return 0.0; }
  void forward(const float *d_in, int32_t cap, const int32_t *d_rows, float *d_eval, float *, rt_stream_t s,
               const CoNetIO &io = CoNetIO()) override {
    if (!io.in_idx || !io.out_idx || io.eval_stride != CO_CACHE_VAL_FLOATS || io.probs_stride != CO_CACHE_VAL_FLOATS)
      throw CaError(CA_ERR_STATE, "HostNet: rows that did not come through the evaluation cache");
    if (cap < 0 || (size_t)cap > rows_cap) cap = (int32_t)rows_cap;
    out_idx = io.out_idx;
    val = d_eval;
    if (cap > 0) gather_rows(d_in, io.in_idx, d_rows, cap, rows70, s);
    RT_LAUNCH(co_k_scan, 1, CO_WAVE, s, scan_params);
    rt_d2h(h_ctl, d_ctl, CO_CTL_WORDS * 4, s);
  }
  /* evals[n], probs[n][96]: the answers to the n rows of the last forward(), in its order */
  void receive(const float *evals, const float *probs, int32_t n, rt_stream_t s) {
    if (n <= 0) return;
    if ((size_t)n > rows_cap || !out_idx) throw CaError(CA_ERR_STATE, "HostNet: answers to rows that were not handed out");
    rt_h2d(ev_in, evals, (size_t)n * 4, s);
    rt_h2d(pr_in, probs, (size_t)n * CO_NUM_MOVES * 4, s);
    scatter_rows(ev_in, pr_in, out_idx, nullptr, n, val, val + 4, CO_CACHE_VAL_FLOATS, CO_CACHE_VAL_FLOATS, s);
  }
};

/* The caller's own network inside a run (ca_trainer_set_net_fn, ca_tourney_set_net_fn): forward() lays the launch's request
 * rows out densely in the caller's DEVICE buffer -- 70 floats each, the rows beyond the device's count zeroed -- calls the
 * caller's function on the launch's stream, and scatters the answers it leaves in the caller's two output buffers to where
 * a network kernel would have written them (CoNetIO).  Nothing comes back to the host: the function is handed the
 * capacity of the launch and a device pointer to the count.  The pools of a fused run call forward() on their own
 * streams without waiting for each other; each works in rows [io.row_base, io.row_base + rows_cap) of the buffers. */
struct NetFn { /* as the caller gave them */
  ca_net_fn fn;
  void *user;
  float *states, *evals, *probs; /* device buffers [max_rows][70], [max_rows], [max_rows][96] */
  int32_t max_rows;
  double flop_per_row;
};
struct ExternalNet : CoNet {
  NetFn f = {};
  CallbackState *owner = nullptr; /* an entry point of the owning handle called from inside fn is refused (host.h co_guard) */
  bool failed = false;

  size_t max_rows() const override { return (size_t)f.max_rows; }
  int kind() const override { return 0; }
  double flop_per_row() const override { return f.flop_per_row; }
  bool callback_failed() const override { return failed; }
  void clear_failure() override { failed = false; }
  void forward(const float *d_in, int32_t cap, const int32_t *d_rows, float *d_eval, float *d_probs, rt_stream_t s,
               const CoNetIO &io = CoNetIO()) override {
    if (failed || cap <= 0) return;
    const size_t row0 = (size_t)io.row_base;
    if (io.row_base < 0 || row0 + (size_t)cap > max_rows())
      throw CaError(CA_ERR_STATE, "caller-supplied network: rows " + std::to_string(row0) + " .. " + std::to_string(row0 + (size_t)cap) +
                                          " are beyond the " + std::to_string(f.max_rows) + " rows of its buffers");
    gather_rows(d_in, io.in_idx, d_rows, cap, f.states + row0 * CO_GAME_STATE_SIZE, s);
    owner->in_callback = true;
    int rc;
    try {
      rc = f.fn(f.user, (int32_t)row0, cap, d_rows, (void *)(intptr_t)s);
    } catch (...) { /* (a function that throws through a C boundary has already broken its contract) */
      rc = -1;
    }
    owner->in_callback = false;
    if (rc != 0) {
      failed = true;
      return;
    }
    scatter_rows(f.evals + row0, f.probs + row0 * CO_NUM_MOVES, io.out_idx, d_rows, cap, d_eval, d_probs, io.eval_stride, io.probs_stride, s);
  }
};

/* What a caller names as a network: weights of one of the library's kinds (nn.h CO_NET_*), or a function of its own with
 * the three device buffers it works in.  Checked where it is given; make() is the one place it becomes a CoNet. */
struct NetSpec {
  int kind = 0;
  const float *weights = nullptr; /* the caller's, not looked at before make() ... */
  size_t n_floats = 0;
  std::vector<float> kept;        /* ... or a copy (keep()): a tournament makes its networks later than the call that named them */
  NetFn f = {};         /* f.fn null: the weights */
  const char *who = ""; /* the entry point that named the function, for the messages */

  NetSpec() = default;
  NetSpec(int kind_, const float *w, size_t n) : kind(kind_), weights(w), n_floats(n) {}
  NetSpec(const char *who_, const NetFn &fn) : f(fn), who(who_) {
    if (!f.fn || !f.states || !f.evals || !f.probs) throw CaError(CA_ERR_ARG, std::string(who) + ": null function or buffer");
    if (f.max_rows <= 0 || !(f.flop_per_row >= 0.0))
      throw CaError(CA_ERR_ARG, std::string(who) + ": max_rows must be positive, flop_per_row 0 (unknown) or positive");
  }
  NetSpec keep() && { return kept.assign(weights, weights + n_floats), weights = nullptr, std::move(*this); }
  /* the network, for launches of up to `rows_needed` rows queued on s.  `asker` and `hint` finish the sentence about a
   * caller's buffers that are too small: "<who>: buffers of N rows<asker> asks for up to M<hint>" */
  std::unique_ptr<CoNet> make(size_t rows_needed, rt_stream_t s, CallbackState *guard, const std::string &asker = "",
                              const char *hint = "") const {
    if (f.fn) {
      if ((size_t)f.max_rows < rows_needed)
        throw CaError(CA_ERR_ARG, std::string(who) + ": buffers of " + std::to_string(f.max_rows) + " rows" + asker + " asks for up to " +
                                          std::to_string(rows_needed) + hint);
      auto n = std::make_unique<ExternalNet>();
      n->f = f, n->owner = guard;
      return n;
    }
    std::unique_ptr<CoNet> n;
    try {
      n.reset(co_net_create(kind, weights ? weights : kept.data(), weights ? n_floats : kept.size(), rows_needed, s));
    } catch (const std::invalid_argument &e) { /* weights outside the kind's operand range (nn.h range_exceeded) */
      throw CaError(CA_ERR_ARG, e.what());
    }
    if (!n) throw CaError(CA_ERR_ARG, "unknown net kind or bad weight count");
    return n;
  }
};
