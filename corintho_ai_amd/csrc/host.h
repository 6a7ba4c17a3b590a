// host.h -- the host plumbing every source shares: owners of runtime resources, the error type and the guard of the C
// ABI's entry points, and what the inference networks' constructors have in common (the f16 range flag, the folded
// BatchNorm constants; the 16-bit operand terms of the split-precision kinds: nn_split.h).  Builds on rt.h, so it
// compiles under -DCO_EMU too.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/corintho_hip.h"
#include "nn.h"
#include "rt.h"

/* ---- Owners of runtime resources: move-only, null until allocated or created, released once by their destructor */
template <typename T>
struct DevBuf {
  T *p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept { return std::swap(p, o.p), std::swap(n, o.n), *this; }
  void alloc(size_t count, rt_stream_t s) { /* zeroed, the clear queued on s (rt.h) */
    release();
    n = count;
    rt_malloc((void **)&p, count * sizeof(T), s);
  }
  /* zeroed room for h's n values, and the copy of them queued behind the clear; h must live until s is synchronised */
  void upload(const T *h, size_t count, rt_stream_t s) {
    alloc(count, s);
    rt_h2d(p, h, count * sizeof(T), s);
  }
  /* room for `count` values, a quarter more when it has to grow (buffers kept between calls); what it held is lost */
  void grow(size_t count, rt_stream_t s) {
    if (n < count) alloc(count + count / 4, s);
  }
  void release() {
    if (p) rt_free(p);
    p = nullptr;
    n = 0;
  }
  ~DevBuf() { release(); }
};

template <typename H, void (*Destroy)(H)>
struct RtHandle {
  H h = {};
  RtHandle() = default;
  RtHandle(RtHandle &&o) noexcept : h(o.h) { o.h = H{}; }
  RtHandle &operator=(RtHandle &&o) noexcept { return std::swap(h, o.h), *this; }
  ~RtHandle() { Destroy(h); }
  operator H() const { return h; }
};
struct Stream : RtHandle<rt_stream_t, rt_stream_destroy> {
  void create() { rt_stream_create(&h); }
};
struct Event : RtHandle<rt_event_t, rt_event_destroy> {
  void create() { rt_event_create(&h); }
};
template <typename T>
struct Pinned : RtHandle<void *, rt_host_free> { /* page-locked host memory */
  void alloc(size_t count) {
    rt_host_alloc(&h, count * sizeof(T));
    memset(h, 0, count * sizeof(T));
  }
  T &operator[](size_t i) const { return ((T *)h)[i]; }
};

/* Caller buffers page-locked for direct DMA (ca_trainer_pin_host: the three arrays of main.pyx:132-134 live as long as
 * the Trainer): copies from / to them are then at PCIe speed instead of staged through the runtime's bounce buffers.  A
 * buffer must stay allocated until it is unpinned or its owner destroyed. */
struct HostPins {
  std::vector<std::pair<void *, size_t>> regs;
  HostPins() = default;
  HostPins(const HostPins &) = delete;
  HostPins &operator=(const HostPins &) = delete;
  ~HostPins() {
    for (auto &r : regs) rt_host_unregister(r.first);
  }
  bool pin(void *p, size_t bytes) {
    for (auto &r : regs)
      if (r.first == p && r.second >= bytes) return true;
    unpin(p); /* (registered with fewer bytes) */
    if (!rt_host_register(p, bytes)) return false;
    regs.emplace_back(p, bytes);
    return true;
  }
  void unpin(void *p) {
    for (size_t i = 0; i < regs.size(); ++i)
      if (regs[i].first == p) {
        rt_host_unregister(p);
        regs[i] = regs.back();
        regs.pop_back();
        return;
      }
  }
};

/* ---- Errors of the C ABI: an exception that carries the CA_ERR_* code its entry point returns */
struct CaError : std::runtime_error {
  int code;
  CaError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

/* the text behind ca_last_error (engine.hip), per thread */
extern thread_local std::string g_last_error;
void co_set_last_error(const std::string &m);

/* the body of an entry point; what it throws becomes the return code and ca_last_error */
template <class F>
int co_guard(F &&body) {
  try {
    body();
    return CA_OK;
  } catch (const CaError &e) {
    co_set_last_error(e.what());
    return e.code;
  } catch (const std::exception &e) {
    co_set_last_error(e.what());
    return CA_ERR_DEVICE;
  }
}
/* is the handle inside a caller-supplied network function (ca_net_fn)?  Handles without that state (net_host.h
 * CallbackState): never */
template <class H>
auto co_in_callback(const H *h, int) -> decltype((bool)h->callback.in_callback) { return h->callback.in_callback; }
template <class H>
bool co_in_callback(const H *, long) { return false; }

/* ... of an entry point on a handle (trainer, tourney, fitter).  Its device is selected first: the caller's thread may
 * have another one current (two trainers on two GPUs in one process; torch.cuda.set_device between calls) */
template <class H, class F>
int co_guard(H *h, F &&body) {
  return co_guard([&] {
    if (!h) throw CaError(CA_ERR_ARG, "null handle");
    if (co_in_callback(h, 0))
      throw CaError(CA_ERR_STATE, "called from inside a caller-supplied network function (ca_net_fn) of the same handle");
    rt_set_device(h->dev());
    body();
  });
}

/* An entry point without a handle (the *_create calls, the stand-alone probes): the device checked and made current, then
 * the body under the guard ... */
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

/* the kernels' out-of-range flag of an f16x3 network (nn.h range_exceeded); never allocated: never raised */
struct RangeFlag {
  DevBuf<uint32_t> flag;
  void alloc(rt_stream_t s) { flag.alloc(1, s); }
  uint32_t *ptr() const { return flag.p; }
  bool read(rt_stream_t s) const {
    if (!flag.p) return false;
    uint32_t v = 0;
    rt_d2h(&v, flag.p, 4, s);
    rt_sync(s);
    return v != 0;
  }
};

/* BatchNormalization at inference, gamma (x - mean) / sqrt(var + eps) + beta, as the float32 constants a x + c */
inline void bn_fold(const float *gamma, const float *beta, const float *mean, const float *var, int n, float *a, float *c) {
  for (int i = 0; i < n; ++i) {
    a[i] = (float)((double)gamma[i] / sqrt((double)var[i] + CO_BN_EPS));
    c[i] = (float)((double)beta[i] - (double)mean[i] * (double)a[i]);
  }
}
/* ... BatchNorm j (n channels) of the flat weights w with layout L (nn_layout.h) */
template <class L>
void bn_fold(const float *w, const L &lay, int j, int n, float *a, float *c) {
  bn_fold(w + lay.gamma(j), w + lay.beta(j), w + lay.mean(j), w + lay.var(j), n, a, c);
}
