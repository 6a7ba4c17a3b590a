// search_puct.h -- search layer 3: the arithmetic of a PUCT scan and the root copy.
//
// The body of chooseNext's loop (trainmc.cpp:540-600) for one edge (co_puct_u), its correctly rounded small divisions
// and the exploration factor (:549), the pass of a simulation through a node (:609-623), and CoRoot: the copy of the
// root that the simulations of one step share.
#pragma once
#include "engine_defs.h"
#include "wave.h"
#include "search_state.h"
#include "search_tree.h"

/* x / d for a float x and an integer d in [1, 2^15] as the correctly rounded double quotient --
 * what the reference's double division gives (trainmc.cpp:565-568) -- without the full IEEE
 * division sequence (two v_div_scale, v_rcp_f64, seven fma, v_div_fmas, v_div_fixup; the two
 * quotients and the square root of a PUCT scan were ~45 double-rate instructions per level and
 * the largest single cost of a simulation).  r = 1/d to double precision from the float
 * reciprocal and two Newton steps; q0 = RN(x r); e = x - d q0 is exact (d has 16 bits and x is
 * a multiple of ulp(q0)); q = RN(q0 + e r) = RN(x/d (1 + 2^-51 ulp)).  x/d is either a double
 * itself or at least ulp/(2 d) >= 2^-17 ulp away from every rounding boundary, so q = RN(x/d).
 * (A zero quotient may differ in sign; pv >= +0 makes the PUCT sum the same.)  The seed only has
 * to be good to ~20 bits, so the emulation build's 1.0f / d and v_rcp_f32 give the same q. */
CO_DEV double co_recip_small(float df) {
#ifdef CO_EMU
  float rf = 1.0f / df;
#else
  float rf = __builtin_amdgcn_rcpf(df);
#endif
  double d = (double)df;
  double r = (double)rf;
  double e = __builtin_fma(-d, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-d, r, 1.0);
  r = __builtin_fma(r, e, r);
  return r;
}
/* x / df given r = co_recip_small(df) */
CO_DEV double co_div_with(double x, float df, double r) {
  double d = (double)df;
  double q0 = x * r;
  double rem = __builtin_fma(-d, q0, x);
  return __builtin_fma(rem, r, q0);
}
CO_DEV double co_div_small(double x, float df) { return co_div_with(x, df, co_recip_small(df)); }

/* Copy of the root kept across the simulations of one step, so that a simulation starts without any
 * dependent load: header and stat slot in registers, the first 64 edge slots (the whole PUCT scan of
 * the root for all but the widest positions) in LDS.  Every simulation reads them and changes one:
 * stores to a root edge slot go to memory AND to the copy (co_store_slot); the rare paths that
 * rewrite several path slots in memory (terminal leaf, dead end) drop the copy (valid = 0). */
struct CoRoot {
  uint4 h0, h1, cs;
  int valid;
  int hdr;        /* h0, h1, e0, ne are the root's (they do not change while a step searches): a dropped copy is made good
                   * again by ONE trip to memory -- own slot and edge slots together -- instead of two dependent ones */
  uint4 *ev;      /* LDS: edge slots 0..63 of the root */
  uint32_t e0;    /* unit offset of the root's edge slot 0 */
  uint32_t ne;    /* edge slots held: min(edges, 64) */
};

/* the exploration factor of a PUCT scan (trainmc.cpp:549): float(double(c_puct) * sqrt(double(float(visits)))).
 * (Computing it one step ahead, in the shadow of the descent's block fetch, was measured in round 4: the generation 5 %
 * SLOWER -- two more values live across the scan loop cost more than the hidden chain saves.) */
CO_DEV float co_vsqrt(float c_puct, int visits) { return (float)((double)c_puct * co_sqrt_f64((double)(float)visits)); }

CO_DEV void co_root_load(CoTree &t, CoRoot &rc) {
  if (!rc.hdr) {
    rc.h0 = co_load_unit(t.A, t.tc.root);
    rc.h1 = co_load_unit(t.A, CO_NODE_INFO(t.tc.root));
    rc.e0 = CO_NODE_EDGE0(t.tc.root);
    uint32_t n = CO_META_NEDGES(rc.h0.z);
    rc.ne = n < (uint32_t)CO_WAVE ? n : (uint32_t)CO_WAVE;
    rc.hdr = 1;
  }
  rc.cs = co_load_unit(t.A, rc.h1.x);
  const uint4 *A = t.A;
  FOR_LANES { rc.ev[lane] = A[rc.e0 + lane]; } /* arena is padded: lanes >= n read unused units */
  WAVE_SYNC();
  rc.valid = 1;
}


/* single-lane store of a stat slot, mirrored into the root copy when it is one of the root's edge slots */
CO_DEV void co_store_slot(uint4 *A, uint32_t slot, uint4 v, CoRoot &rc) {
  const uint32_t idx = slot - rc.e0; /* unsigned: anything outside the root's edges is >= ne */
  FOR_LANES {
    if (lane == 0) {
      A[slot] = v;
      if (idx < rc.ne) rc.ev[idx] = v;
    }
  }
  WAVE_SYNC();
}

/* u of ONE edge, from its slot (the body of chooseNext's loop, trainmc.cpp:553-579), per lane.  Branch-free: every lane
 * evaluates both forms and selects (one f64 pair per level whatever the mix of edges; divergent branches here cost more
 * than they save). */
CO_DEV float co_puct_u(uint4 s, float denom, float v_sqrt) {
  float prob = (float)CO_SLOT_PRIOR_Q(s) * denom;
  float pv = prob * v_sqrt;
  int r = CO_SLOT_RESULT(s);
  int has_child = s.x != CO_NONE;
  int drawn = (r == CO_RESULT_DRAW) | (r == CO_DEDUCED_DRAW);
  int searchable = ((r == CO_RESULT_NONE) | drawn) & !CO_SLOT_ALL_VISITED_BIT(s);
  int vis = co_slot_visits(s);
  float cv = (float)(vis > 0 ? vis : 1); /* 1 .. 32767 */
  /* (Measured in round 6: with both quotients as single-precision products with v_rcp_f32 -- NOT the reference's bits; the
   * ceiling of any scheme that scans approximately and verifies -- a generation is 1-2.6 % shorter: not what a scan costs.) */
  double a = co_div_small(-(double)co_u2f(s.y), cv);
  double b = co_div_small((double)pv, cv + 1.0f);
  float uv = (float)(a + b);
  float uc = drawn ? pv : uv;           /* visited child (trainmc.cpp:561-569; a drawn one without the /(n + 1): quirk 6) */
  uc = searchable ? uc : CO_NEG_INF;
  return has_child ? uc : pv;           /* unvisited edge (:575-577) */
}

/* a simulation passes through a node: increment_visits + increase_evaluation(1.0) (trainmc.cpp:609-623), on its stat slot */
CO_DEV uint4 co_slot_pass(uint4 s) {
  s = co_slot_set_visits(s, co_slot_visits(s) + 1);
  s.y = co_f2u(co_u2f(s.y) + 1.0f);
  return s;
}
