// host.h -- the host plumbing every source shares: owners of runtime resources, the error type and the guard of the C
// ABI's entry points, and what the inference networks' constructors have in common (16-bit operand terms, the f16
// range flag, the folded BatchNorm constants).  Builds on rt.h, so it compiles under -DCO_EMU too.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <stdexcept>
#include <string>
#include <utility>

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

/* ---- 16-bit operand terms of the split-precision kernels, as the host packs them */
inline uint16_t bf16_rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint32_t a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40); /* NaN: the rounding add could carry a full mantissa into a finite number */
  if (a >= 0x7f7f8000u && a < 0x7f800000u) return (uint16_t)(u >> 16); /* ... or a finite one to infinity: the largest bf16, the next term takes the rest */
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline float bf16_to_f(uint16_t h) {
  uint32_t u = (uint32_t)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
/* float -> IEEE binary16, round to nearest even, subnormals kept (what v_cvt_f16_f32 gives); in integer arithmetic, so
 * that a host compiler without a 16-bit float type gives the same bits */
inline uint16_t f16_rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint32_t sign = (u >> 16) & 0x8000u;
  u &= 0x7fffffffu;
  if (u > 0x7f800000u) return (uint16_t)(sign | 0x7e00u | ((u >> 13) & 0x1ffu)); /* NaN */
  if (u >= 0x47800000u) return (uint16_t)(sign | 0x7c00u);                        /* 2^16 and beyond, infinity */
  uint32_t r, rem, half;
  if (u < 0x38800000u) { /* below 2^-14: a multiple of fp16's subnormal quantum 2^-24 */
    if (u <= 0x33000000u) return (uint16_t)sign; /* up to 2^-25, the tie included: zero */
    const int shift = 126 - (int)(u >> 23);      /* 14 .. 24 */
    const uint32_t m = (u & 0x7fffffu) | 0x800000u;
    r = m >> shift;
    rem = m & ((1u << shift) - 1u);
    half = 1u << (shift - 1);
  } else {
    r = (u - 0x38000000u) >> 13; /* exponent rebiased; a carry out of the mantissa below is the next exponent (65520: infinity) */
    rem = u & 0x1fffu;
    half = 0x1000u;
  }
  if (rem > half || (rem == half && (r & 1u))) ++r;
  return (uint16_t)(sign | r);
}
inline float f16_to_f(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
  float f;
  if (e == 0) { /* zero or subnormal: m quanta of 2^-24, exact */
    f = (float)m * 5.9604644775390625e-8f;
    return sign ? -f : f;
  }
  const uint32_t u = sign | (e == 31 ? 0x7f800000u : (e + 112u) << 23) | (m << 13);
  memcpy(&f, &u, 4);
  return f;
}
/* v -> nt 16-bit terms: bf16(v) (f16: fp16(v)), the same of the remainder, ... (the device's m3_split / rcs_split).  An
 * f16 caller checks |v| <= CO_F16_MAX first. */
inline void split_terms(float v, int nt, bool f16, uint16_t *out) {
  for (int i = 0; i < nt; ++i) {
    out[i] = f16 ? f16_rne(v) : bf16_rne(v);
    v = v - (f16 ? f16_to_f(out[i]) : bf16_to_f(out[i]));
  }
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
