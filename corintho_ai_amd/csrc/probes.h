// probes.h -- entry points that need no trainer, each on a stream of its own: the library's network kernels on device
// memory (ca_net_*), and the rule layer, the generator and the floating-point contract on batches, for the tests.
// Included by engine.hip.
#pragma once
#include <memory>
#include <vector>

#include "net_host.h"

/* ---- the library's own network kernels on device memory, without a trainer (ca_net_*): a CoNet and the 80-float rows the
 * kernels read, i.e. ca_trainer_net_forward (HostForward) without its copies */
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
    launch(d_states, rows_cap, rows_cap, d_rows, d_evals, d_probs, CoNetIO(), stream_arg, "ca_net_forward_device");
  }

  /* the same launch as a fused run shapes it (pools.h Pools::launch): rows read through io.in_idx from the first state_rows
   * rows of d_states, outputs through io.out_idx at io's strides, io.alone */
  void forward_device_io(const float *d_states, int32_t state_rows, int32_t rows_cap, const int32_t *d_rows, float *d_evals,
                         float *d_probs, const CoNetIO &io, void *stream_arg) {
    const char *who = "ca_net_forward_device_io";
    if (!d_states || !d_rows || !d_evals || !d_probs) throw CaError(CA_ERR_ARG, std::string(who) + ": null buffer");
    if (rows_cap < 0 || (size_t)rows_cap > net->max_rows() || state_rows < 0 || (size_t)state_rows > net->max_rows())
      throw CaError(CA_ERR_ARG, std::string(who) + ": more rows than the net's max_rows");
    if (!io.in_idx && state_rows < rows_cap)
      throw CaError(CA_ERR_ARG, std::string(who) + ": without in_idx the launch reads rows_cap rows, state_rows is fewer");
    if (io.eval_stride < 1 || io.probs_stride < CO_NET_NUM_MOVES)
      throw CaError(CA_ERR_ARG, std::string(who) + ": eval_stride < 1 or probs_stride < 96");
    if (rows_cap == 0) return;
    launch(d_states, state_rows, rows_cap, d_rows, d_evals, d_probs, io, stream_arg, who);
  }

  void launch(const float *d_states, int32_t state_rows, int32_t rows_cap, const int32_t *d_rows, float *d_evals, float *d_probs,
              const CoNetIO &io, void *stream_arg, const char *who) {
    const rt_stream_t s = stream_arg ? (rt_stream_t)(intptr_t)stream_arg : (rt_stream_t)stream;
    if (used_once && used_on != s) rt_stream_wait(s, used);
    expand_rows(d_states, rows80.p, state_rows, s);
    net->forward(rows80.p, rows_cap, d_rows, d_evals, d_probs, s, io);
    rt_event_record(used, s);
    used_on = s;
    used_once = true;
    if (!stream_arg) {
      rt_sync(s);
      check_net_range(net.get(), s, who);
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
/* (the indices themselves cannot be checked here: they live on the device and are read by the kernels, include/corintho_hip.h) */
extern "C" int ca_net_forward_device_io(ca_net *n, const float *d_states, int32_t state_rows, int32_t rows_cap, const int32_t *d_rows,
                                        const int32_t *d_in_idx, const int32_t *d_out_idx, float *d_evals, int32_t eval_stride,
                                        float *d_probs, int32_t probs_stride, int32_t alone, void *stream) {
  return co_guard(n, [&] {
    CoNetIO io;
    io.in_idx = d_in_idx, io.out_idx = d_out_idx, io.eval_stride = eval_stride, io.probs_stride = probs_stride, io.alone = alone != 0;
    n->forward_device_io(d_states, state_rows, rows_cap, d_rows, d_evals, d_probs, io, stream);
  });
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
