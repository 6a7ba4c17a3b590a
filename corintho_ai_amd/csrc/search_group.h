// search_group.h -- search layer 4b: up to CO_SB simulations of a step selected together (co_search_rows).
//
// Restates TrainMC::search (trainmc.cpp:602-696) and chooseNext (:540-600) for the simulations that end the ordinary
// way, with the arena, the pending-leaf records and the generator left bit for bit as the sequential search
// (search_one.h) leaves them.
//
// This header is ONE function and stays one.  Extracting its phases into force-inlined functions is not a neutral
// refactoring: with the first phase (the shared-node scans) in a function taking references, co_k_mcts_step came out
// with another instruction stream -- v_readlane_b32 1169 -> 1049, v_writelane_b32 384 -> 352, and a flat_load_dwordx4
// where a global load was.  The kernel sits on a register cliff; cutting this function up is a
// performance change and has to pay for a same-machine A/B.
#pragma once
#include "engine_defs.h"
#include "rules.h"
#include "wave.h"
#include "search_state.h"
#include "search_tree.h"
#include "search_eval.h"
#include "search_puct.h"

/* ---- Several simulations of a step at a time (round 5).
 *
 * The reference runs the simulations of a step one after another (trainmc.cpp:169-173), and so did this kernel: every
 * simulation a chain of dependent waits -- root scan, block fetch, scan, store, expansion, request -- ~10 k cycles of a
 * lone wavefront, sixteen times per launch.  But under the virtual loss a simulation that ends the ORDINARY way -- it
 * descends through visited, non-terminal children and creates one new, non-terminal leaf -- changes the tree in a way
 * that is known the moment each of its choices is made: the chosen child's slot gets one visit and +1.0 (:609-623;
 * a new child is born with all_visited set and cannot be chosen again before its evaluation arrives, quirk 3), and nothing
 * else a later scan of the step looks at.  So CO_SB simulations are SELECTED together, level by level:
 *   - every simulation scans its node's edge slots in registers; a slot another simulation of the group has changed at
 *     this level is patched in first (same node <=> same level: it is a tree), in simulation order -- at the root that is
 *     all of them, deeper down only those that chose the same child;
 *   - the blocks of all the children descended to are requested together: one memory round trip per LEVEL of the group;
 *   - nothing is written while selecting.  Then, in simulation order, each leaf is expanded and the simulation's stores are
 *     issued (path slots, node, request) -- the same values in the same order as one after another, so the arena, the
 *     pending-leaf records and the generator are bit for bit what the sequential search leaves.
 * A simulation that turns out NOT to be ordinary (nothing searchable below a node, a terminal child or a terminal new
 * leaf, a node wider than the wavefront, a path beyond CO_SB_DEPTH, a full arena) ends the group in front of it: the
 * simulations before it are committed, it is run by co_search on the committed tree, the ones behind it are selected
 * again in the next group (their selection is discarded -- nothing was written). */
#define CO_SB_PE_ONE 96
#define CO_SB_PE_TWO 40
#define CO_SB_DEPTH 12 /* levels a grouped simulation may pass (a level = a lane of its row when it commits: at most 16) */
/* co_search_rows' records in LDS, [simulation][level]: sb_block and sb_cs have CO_SB_DEPTH levels, sb_slot one more (the
 * new child's slot, one level below the last node scanned; written CO_SB_SLOT_AT(j, lv) + 1: the sum in the order it
 * had before the index had a name) */
#define CO_SB_AT(j, lv) ((j) * CO_SB_DEPTH + (lv))
#define CO_SB_SLOT_AT(j, lv) ((j) * (CO_SB_DEPTH + 1) + (lv))

/* (the emulation build's counters CO_SBS / CO_SBP: search_state.h) */

/* m = simulations that are certainly due (1 < m <= CO_SB = 4: each adds one pending leaf and one search).  Returns how
 * many were committed; fewer than m: the next one takes co_search.
 *
 * The group's four simulations live in the four ROWS of the wavefront (16 lanes each, the rows of the DPP unit):
 *   root    the root's edge slots in registers (one per lane), scanned once per simulation, the chosen slot patched in
 *           place -- sequential by nature, wave-wide;
 *   below   row j descends simulation j: its node's edge slots as up to four per lane (edge = 16 k + column), row maximum
 *           and first-maximum by DPP, the winner's slot by ds_bpermute -- one instruction stream for the four descents.
 *           Rows that meet in one node take turns in simulation order, the later one's copy patched with what the
 *           earlier one changed;
 *   commit  in simulation order (co_search_commit). */
CO_DEV int co_search_rows(CoWave &w, CoTree &t, CoRoot &rc, int m) {
  uint4 *A = t.A;
  WAVE_SHARED(uint32_t, sb_block, CO_SB * CO_SB_DEPTH);       /* [sim][level] node scanned */
  WAVE_SHARED(uint32_t, sb_slot, CO_SB * (CO_SB_DEPTH + 1));  /* [sim][level] its stat slot; [leaf level] the new child's */
  WAVE_SHARED(uint4, sb_cs, CO_SB * CO_SB_DEPTH);             /* [sim][level] that slot after the pass */
  WAVE_SHARED(uint4, sb_hand, CO_SB * 2);                     /* root -> row j: {child block, child slot, z of the chosen slot, -}, the chosen slot */
  WAVE_SHARED(uint4, sb_leaf, CO_SB * 2);                     /* row j's leaf: {its parent's board lo, hi, meta, block}, {the chosen slot's move | prior, the leaf's slot, -, -} */
  WAVE_SHARED(int, sb_kn, CO_SB);                             /* sim j found nothing searchable below the node of this level (else -1) */
  FOR_LANES_HOT {
    if (lane < CO_SB) sb_kn[lane] = -1;
  }
  WAVE_SYNC();
  int bad = m; /* the first simulation that is not ordinary */
  /* ---- the root, simulation after simulation; and on down for as long as ALL of them take the same child (a forced
   * line, a trained network's favourite: rows that share a node would take turns anyway -- one wave-wide scan per
   * simulation, the chosen slot patched in registers, is half the instructions of a turn in row form) */
  uint32_t shX = t.tc.root; /* the shared node, its own stat slot and header */
  uint32_t shown = rc.h1.x;
  uint4 shh0 = rc.h0;
  int lev0 = 0;             /* its level */
  {
    int n0 = (int)CO_META_NEDGES(rc.h0.z);
    float denom0 = co_u2f(rc.h1.y);
    LV(uint4, ev);
    FOR_LANES_HOT { L(ev) = rc.ev[lane]; }
    uint4 rcs = rc.cs;
    /* What a scan of this node needs of each edge, kept across the group's scans (co_puct_u in two halves): the
     * exploitation term a = -E / V, the reciprocal of V + 1 for the exploration term, the prior, and which form u takes
     * (0 unvisited, 1 visited, 2 drawn, 3 not to be searched).  Only the chosen edge changes between two scans -- one
     * more visit, +1.0: its a is the old reciprocal's quotient, its reciprocal is made anew.  And the exploration factors
     * of the group's scans (visits, visits + 1, ...: one double-precision square root each) come from ONE pass, a lane each. */
    LV(double, ea);
    LV(double, er);
    LV(float, ecv1);
    LV(float, eprob);
    LV(int, emode);
    LV(float, vsl);
    for (;;) {
      const int msel = bad < m ? bad : m;
      uint32_t same_slot = CO_NONE; /* the child every simulation so far has taken, 0 = not one child (or a new one) */
      uint4 first_bs = make_uint4(0u, 0u, 0u, 0u);
      {
        const int v0 = co_slot_visits(rcs);
        FOR_LANES_HOT {
          const uint4 s = L(ev);
          const int r = CO_SLOT_RESULT(s);
          const int has_child = s.x != CO_NONE;
          const int drawn = (r == CO_RESULT_DRAW) | (r == CO_DEDUCED_DRAW);
          const int searchable = ((r == CO_RESULT_NONE) | drawn) & !CO_SLOT_ALL_VISITED_BIT(s);
          const int vis = co_slot_visits(s);
          const float cv = (float)(vis > 0 ? vis : 1);
          L(eprob) = (float)CO_SLOT_PRIOR_Q(s) * denom0;
          L(ea) = co_div_small(-(double)co_u2f(s.y), cv);
          L(ecv1) = cv + 1.0f;
          L(er) = co_recip_small(L(ecv1));
          L(emode) = !has_child ? 0 : !searchable ? 3 : drawn ? 2 : 1;
          L(vsl) = co_vsqrt(w.c_puct, v0 + (lane < CO_SB ? lane : 0));
        }
      }
      for (int j = 0; j < msel; ++j) {
        CO_SBS(10, 1);
        CO_PROF_ADD(w, 23, 1ull);
        CO_STEP_WORK(w, 1);
        const float v_sqrt = WAVE_BCAST(vsl, j);
        LV(float, u);
        FOR_LANES_HOT {
          const float pv = L(eprob) * v_sqrt;
          const double bq = co_div_with((double)pv, L(ecv1), L(er));
          const float uv = (float)(L(ea) + bq);
          const int md = L(emode);
          const float uu = md == 1 ? uv : md == 3 ? CO_NEG_INF : pv;
          L(u) = lane < n0 ? uu : CO_NEG_INF;
        }
        const float mx = WAVE_MAX_F32(u);
        rcs = co_slot_pass(rcs);
        if (!(mx > CO_NEG_INF)) {
          CO_SBS(3, 1);
          bad = j;
          const uint32_t xo = shown;
          const int lv = lev0;
          FOR_LANES_HOT {
            if (lane == 0) { /* (for the tail below: this node's slot and its value after the pass) */
              sb_slot[CO_SB_SLOT_AT(j, lv)] = xo;
              sb_cs[CO_SB_AT(j, lv)] = rcs;
              sb_kn[j] = lv;
            }
          }
          break;
        }
        LV(int, hit);
        FOR_LANES_HOT { L(hit) = (L(u) == mx); }
        const int le = co_ffs64(WAVE_BALLOT(hit)) - 1;
        const uint4 bs = WAVE_BCAST(ev, le);
        if (bs.x != CO_NONE && co_res_terminal(co_slot_result(bs))) {
          CO_SBS(4, 1);
          bad = j;
          break;
        }
        const uint32_t child_slot = CO_NODE_EDGE(shX, (uint32_t)le);
        const uint4 nv = bs.x == CO_NONE ? CO_SLOT_BORN(bs) : co_slot_pass(bs);
        if (j == 0) {
          same_slot = bs.x == CO_NONE ? 0u : child_slot;
          first_bs = bs;
        } else if (child_slot != same_slot) {
          same_slot = 0u;
        }
        const uint32_t xb = shX, xo = shown;
        const int lv = lev0;
        FOR_LANES_HOT {
          if (lane == le) {
            L(ev) = nv;
            if (L(emode) == 0) {
              L(emode) = 3; /* a new child: all_visited until its evaluation arrives */
            } else {
              L(ea) = co_div_with(-(double)co_u2f(nv.y), L(ecv1), L(er));
              L(ecv1) = L(ecv1) + 1.0f;
              L(er) = co_recip_small(L(ecv1));
            }
          }
          if (lane == 0) {
            sb_block[CO_SB_AT(j, lv)] = xb;
            sb_slot[CO_SB_SLOT_AT(j, lv)] = xo;
            sb_slot[CO_SB_SLOT_AT(j, lv) + 1] = child_slot;
            sb_cs[CO_SB_AT(j, lv)] = rcs;
            sb_hand[2 * j] = make_uint4(bs.x, child_slot, bs.z, 0u);
            sb_hand[2 * j + 1] = bs;
          }
        }
      }
      WAVE_SYNC();
      const int left = bad < m ? bad : m;
      if (left < 2 || same_slot == 0u || same_slot == CO_NONE || lev0 + 3 >= CO_SB_DEPTH) break;
      /* every simulation left went to the same visited child: that node is shared as well */
      CO_SBS(20, 1);
      shX = first_bs.x;
      shown = same_slot;
      rcs = first_bs;
      ++lev0;
      CO_SBS(9, 1);
      shh0 = co_load_unit(A, shX);
      denom0 = co_u2f(co_load_unit(A, CO_NODE_INFO(shX)).y);
      {
        const uint32_t e0 = CO_NODE_EDGE0(shX);
        FOR_LANES_HOT { L(ev) = A[e0 + lane]; }
      }
      n0 = (int)CO_META_NEDGES(shh0.z);
      if (n0 > CO_WAVE) { /* (a node wider than the wavefront: co_search's) */
        CO_SBS(5, 1);
        bad = 0;
        break;
      }
    }
  }
  CO_PH(28);
  /* ---- below the root: row j = simulation j */
  LV(uint32_t, X);
  LV(uint32_t, slot);
  LV(uint4, cs);
  LV(int, act);
  LV(int, leafD);      /* level of the new leaf, 0 = none (yet) */
  {
    const int nsel = bad < m ? bad : m;
    const uint4 rh0 = shh0;
    const uint32_t root = shX;
    FOR_LANES_HOT {
      const int r = lane >> 4;
      const uint4 h = sb_hand[2 * r], c = sb_hand[2 * r + 1];
      const int valid = r < nsel;
      const int isnew = valid && h.x == CO_NONE;
      L(X) = h.x;
      L(slot) = h.y;
      L(cs) = c;
      L(act) = valid && !isnew;
      L(leafD) = isnew ? lev0 + 1 : 0;
      if (isnew && (lane & 15) == 0) { /* a new edge of the shared node: the leaf is one level below it */
        sb_leaf[2 * r] = make_uint4(rh0.x, rh0.y, rh0.z, root);
        sb_leaf[2 * r + 1] = make_uint4(CO_SLOT_MP(h.z), h.y, 0u, 0u);
      }
    }
  }
  for (int lev = lev0 + 1;; ++lev) {
    if (!WAVE_BALLOT(act)) break;
    CO_SBS(9, 1);
    if (lev + 1 >= CO_SB_DEPTH) { /* too deep for the group's records */
      const int fr = (co_ffs64(WAVE_BALLOT(act)) - 1) >> 4;
      CO_SBS(6, 1);
      if (fr < bad) bad = fr;
      break;
    }
    {
      /* One or two rows left descending (the deep, narrow trees of a trained network: most levels): the row form costs
       * ~300 instructions a level however few rows are busy, a wave-wide scan ~110 -- so these rows are scanned wave-wide,
       * one after the other, their blocks fetched together.  (With the reference's last checkpoint the grouped search was
       * 8 % SLOWER than round 4's sequential one before this path existed) */
      const uint64_t am = WAVE_BALLOT(act);
      const int a0 = (int)(am & 1ull), a1 = (int)((am >> 16) & 1ull), a2 = (int)((am >> 32) & 1ull), a3 = (int)((am >> 48) & 1ull);
      if (a0 + a1 + a2 + a3 <= 2) {
        CO_SBS(20 + (a0 + a1 + a2 + a3), 1);
        const int r0 = a0 ? 0 : a1 ? 1 : a2 ? 2 : 3;
        const int r1 = a0 + a1 + a2 + a3 < 2 ? -1 : (a3 ? 3 : a2 ? 2 : 1); /* (the last active row: with two, the other one) */
        uint32_t wx[2], ws[2];
        uint4 wc[2], wh[2];
        uint32_t wd[2];
        LV(uint4, we[2]);
        int wr[2] = {r0, r1};
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int r = wr[i] < 0 ? r0 : wr[i];
          wx[i] = WAVE_BCAST(X, 16 * r);
          ws[i] = WAVE_BCAST(slot, 16 * r);
          wc[i] = WAVE_BCAST(cs, 16 * r);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          wh[i] = co_load_unit(A, wx[i]);
          wd[i] = co_load_unit(A, CO_NODE_INFO(wx[i])).y;
          const uint32_t e0 = CO_NODE_EDGE0(wx[i]);
          FOR_LANES_HOT { L(we[i]) = A[e0 + lane]; }
        }
        /* the exploration factors (a double-precision square root each: ~20 dependent instructions) depend on the rows'
         * own slots only: computed HERE, while the blocks are on their way -- left to the compiler they stand behind the
         * first use of the headers (the wide-node test), i.e. behind the wait */
        float wvs[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          wvs[i] = co_vsqrt(w.c_puct, co_slot_visits(wc[i]));
          CO_OPAQUE_V(wvs[i]);
        }
        CO_PH_MEM(11);
        uint32_t pX = CO_NONE;
        int pe = -1;
        uint4 pv = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int r = wr[i];
          if (r < 0 || r >= bad) continue;
          CO_SBS(10, 1);
          CO_PROF_ADD(w, 23, 1ull);
          CO_STEP_WORK(w, 1);
          const int n = (int)CO_META_NEDGES(wh[i].z);
          int gone = 0; /* the row's simulation is not ordinary */
          int le = 0;
          uint4 bs = make_uint4(0u, 0u, 0u, 0u);
          if (n > CO_WAVE) {
            CO_SBS(5, 1);
            gone = 1;
          } else {
            const float denom = co_u2f(wd[i]);
            const float v_sqrt = wvs[i];
            LV(float, u);
            FOR_LANES_HOT {
              uint4 sl = L(we[i]);
              if (pe >= 0 && pX == wx[i] && lane == pe) { /* the row before scanned this very node */
                sl = pv;
                CO_SBS(11, 1);
              }
              L(we[i]) = sl;
              const float uu = co_puct_u(sl, denom, v_sqrt);
              L(u) = lane < n ? uu : CO_NEG_INF;
            }
            const float mx = WAVE_MAX_F32(u);
            wc[i] = co_slot_pass(wc[i]);
            if (!(mx > CO_NEG_INF)) {
              CO_SBS(3, 1);
              gone = 1;
              const uint32_t xs = ws[i];
              const uint4 xc = wc[i];
              FOR_LANES_HOT {
                if (lane == 0) {
                  sb_slot[CO_SB_SLOT_AT(r, lev)] = xs;
                  sb_cs[CO_SB_AT(r, lev)] = xc;
                  sb_kn[r] = lev;
                }
              }
            } else {
              LV(int, hit);
              FOR_LANES_HOT { L(hit) = (L(u) == mx); }
              le = co_ffs64(WAVE_BALLOT(hit)) - 1;
              bs = WAVE_BCAST(we[i], le);
              if (bs.x != CO_NONE && co_res_terminal(co_slot_result(bs))) {
                CO_SBS(4, 1);
                gone = 1;
              }
            }
          }
          if (gone) {
            if (r < bad) bad = r;
            FOR_LANES_HOT {
              if ((lane >> 4) >= r) L(act) = 0;
            }
            continue;
          }
          const uint32_t child_slot = CO_NODE_EDGE(wx[i], (uint32_t)le);
          const int isnew = bs.x == CO_NONE;
          pX = wx[i];
          pe = le;
          pv = isnew ? CO_SLOT_BORN(bs) : co_slot_pass(bs);
          const uint32_t xb = wx[i], xs = ws[i];
          const uint4 xc = wc[i], xh = wh[i];
          FOR_LANES_HOT {
            if (lane == 0) {
              sb_block[CO_SB_AT(r, lev)] = xb;
              sb_slot[CO_SB_SLOT_AT(r, lev)] = xs;
              sb_slot[CO_SB_SLOT_AT(r, lev) + 1] = child_slot;
              sb_cs[CO_SB_AT(r, lev)] = xc;
              if (isnew) {
                sb_leaf[2 * r] = make_uint4(xh.x, xh.y, xh.z, xb);
                sb_leaf[2 * r + 1] = make_uint4(CO_SLOT_MP(bs.z), child_slot, 0u, 0u);
              }
            }
            if ((lane >> 4) == r) {
              if (isnew) {
                L(leafD) = lev + 1;
                L(act) = 0;
              } else {
                L(X) = bs.x;
                L(slot) = child_slot;
                L(cs) = bs;
              }
            }
          }
        }
        WAVE_SYNC();
        CO_PH(8);
        continue;
      }
    }
    CO_SBS(23, 1);
    /* the nodes of this level: header and up to 64 edge slots, four per lane */
    LV(uint4, h0);
    LV(uint32_t, dnb);
    LV(uint4, e0);
    LV(uint4, e1);
    LV(uint4, e2);
    LV(uint4, e3);
    FOR_LANES_HOT {
      if (L(act)) {
        const uint32_t b = L(X);
        const uint32_t c = CO_NODE_EDGE(b, (uint32_t)(lane & 15));
        L(h0) = A[CO_NODE_HDR(b)];
        L(dnb) = A[CO_NODE_INFO(b)].y;
        L(e0) = A[c]; /* the arena is padded: slots beyond the node's edges are read and not used */
        L(e1) = A[c + 16u];
        L(e2) = A[c + 32u];
        L(e3) = A[c + 48u];
      }
    }
    LV(float, vs); /* (a row's exploration factor is its node's: once per level, under the fetch -- not once per turn) */
    FOR_LANES_HOT {
      L(vs) = co_vsqrt(w.c_puct, co_slot_visits(L(cs)));
      CO_OPAQUE_V(L(vs));
    }
    CO_PH_MEM(11);
    LV(int, todo);
    LV(int, wide);
    FOR_LANES_HOT {
      L(wide) = L(act) && (int)CO_META_NEDGES(L(h0).z) > CO_WAVE;
      L(todo) = L(act) && !L(wide);
    }
    {
      const uint64_t wm = WAVE_BALLOT(wide);
      if (wm) {
        const int fr = (co_ffs64(wm) - 1) >> 4;
        CO_SBS(5, 1);
        if (fr < bad) bad = fr;
      }
    }
    for (;;) {
      /* rows behind a simulation that is not ordinary are dropped */
      FOR_LANES_HOT {
        if ((lane >> 4) >= bad) {
          L(todo) = 0;
          L(act) = 0;
        }
      }
      const uint64_t tm = WAVE_BALLOT(todo);
      if (!tm) break;
      CO_SBS(24, 1);
      CO_STEP_WORK(w, 2); /* (a turn in row form: the instructions of two to three wave-wide scans) */
      /* a row waits while an earlier row of the same node has yet to scan it */
      const uint32_t x0 = WAVE_BCAST(X, 0), x1 = WAVE_BCAST(X, 16), x2 = WAVE_BCAST(X, 32);
      const int t0 = (int)(tm & 1ull), t1 = (int)((tm >> 16) & 1ull), t2 = (int)((tm >> 32) & 1ull);
      LV(int, ready);
      LV(float, bu);
      LV(uint32_t, be);
      LV(uint32_t, bx);
      LV(uint32_t, by);
      LV(uint32_t, bz);
      LV(uint32_t, bw);
      FOR_LANES_HOT {
        const int r = lane >> 4;
        const int blocked = (r > 0 && t0 && x0 == L(X)) || (r > 1 && t1 && x1 == L(X)) || (r > 2 && t2 && x2 == L(X));
        L(ready) = L(todo) && !blocked;
        L(bu) = CO_NEG_INF;
        L(be) = 255u;
        L(bx) = L(by) = L(bz) = L(bw) = 0u;
        if (L(ready)) {
          CO_SBS(10, (lane & 15) == 0);
          CO_PROF_ADD(w, 23, 0ull);
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        LV(int, more);
        FOR_LANES_HOT { L(more) = L(ready) && (int)CO_META_NEDGES(L(h0).z) > 16 * k; }
        if (!WAVE_BALLOT(more)) break;
        FOR_LANES_HOT {
          const uint4 sl = k == 0 ? L(e0) : k == 1 ? L(e1) : k == 2 ? L(e2) : L(e3);
          const int e = 16 * k + (lane & 15);
          float uu = co_puct_u(sl, co_u2f(L(dnb)), L(vs));
          uu = (L(ready) && e < (int)CO_META_NEDGES(L(h0).z)) ? uu : CO_NEG_INF;
          if (uu > L(bu)) { /* strict: a lane keeps its first maximum */
            L(bu) = uu;
            L(be) = (uint32_t)e;
            L(bx) = sl.x;
            L(by) = sl.y;
            L(bz) = sl.z;
            L(bw) = sl.w;
          }
        }
      }
      LV(float, mx);
      ROW_MAX_F32(mx, bu);
      LV(uint32_t, cand);
      FOR_LANES_HOT { L(cand) = (L(bu) == L(mx) && L(mx) > CO_NEG_INF) ? L(be) : 255u; }
      LV(uint32_t, emin);
      ROW_MIN_U32(emin, cand); /* the first maximum in edge order (trainmc.cpp:581: strictly greater) */
      LV(int, col);
      FOR_LANES_HOT { L(col) = (int)(L(emin) & 15u); }
      ROW_SHFL_U32(bx, bx, col);
      ROW_SHFL_U32(by, by, col);
      ROW_SHFL_U32(bz, bz, col);
      ROW_SHFL_U32(bw, bw, col);
      /* what the scan did: this node's own slot, the records, the leaf or the child, the patch for rows that wait */
      LV(int, isbad);
      LV(int, fin);
      LV(uint32_t, pX);
      LV(uint4, nv);
      FOR_LANES_HOT {
        L(isbad) = 0;
        L(fin) = L(ready);
        L(pX) = L(X);
        L(nv) = make_uint4(0u, 0u, 0u, 0u);
        if (L(ready)) {
          const int r = lane >> 4;
          const uint4 bs = make_uint4(L(bx), L(by), L(bz), L(bw));
          const int none = L(emin) == 255u;
          const int isnew = bs.x == CO_NONE;
          const int term = !isnew && co_res_terminal(co_slot_result(bs));
          L(cs) = co_slot_pass(L(cs));
          L(isbad) = none || term;
          const uint32_t child_slot = CO_NODE_EDGE(L(X), L(emin));
          if (!L(isbad)) {
            if ((lane & 15) == 0) {
              sb_block[CO_SB_AT(r, lev)] = L(X);
              sb_slot[CO_SB_SLOT_AT(r, lev)] = L(slot);
              sb_slot[CO_SB_SLOT_AT(r, lev) + 1] = child_slot;
              sb_cs[CO_SB_AT(r, lev)] = L(cs);
            }
            if (isnew) {
              L(nv) = CO_SLOT_BORN(bs);
              L(leafD) = lev + 1;
              if ((lane & 15) == 0) {
                sb_leaf[2 * r] = make_uint4(L(h0).x, L(h0).y, L(h0).z, L(X));
                sb_leaf[2 * r + 1] = make_uint4(CO_SLOT_MP(bs.z), child_slot, 0u, 0u);
              }
              L(act) = 0;
            } else {
              L(nv) = co_slot_pass(bs);
              L(X) = bs.x;
              L(slot) = child_slot;
              L(cs) = bs;
            }
          } else {
            if (none) CO_SBS(3, (lane & 15) == 0);
            else CO_SBS(4, (lane & 15) == 0);
            if (none && (lane & 15) == 0) {
              sb_slot[CO_SB_SLOT_AT(r, lev)] = L(slot);
              sb_cs[CO_SB_AT(r, lev)] = L(cs);
              sb_kn[r] = lev;
            }
            L(act) = 0;
          }
          L(todo) = 0;
        }
      }
      {
        const uint64_t bm = WAVE_BALLOT(isbad);
        if (bm) {
          const int fr = (co_ffs64(bm) - 1) >> 4;
          if (fr < bad) bad = fr;
        }
      }
      /* rows that wait at a node one of the finished rows has just scanned: take its change */
      const uint64_t fm = WAVE_BALLOT(fin), wm2 = WAVE_BALLOT(todo);
      if (wm2) {
#pragma unroll
        for (int r2 = 0; r2 < CO_SB - 1; ++r2) {
          if (!((fm >> (16 * r2)) & 1ull)) continue;
          const uint32_t px = WAVE_BCAST(pX, 16 * r2);
          const uint32_t pe = WAVE_BCAST(emin, 16 * r2);
          const uint4 pv = WAVE_BCAST(nv, 16 * r2);
          FOR_LANES_HOT {
            if (L(todo) && (lane >> 4) > r2 && L(X) == px && (uint32_t)(lane & 15) == (pe & 15u)) {
              CO_SBS(11, 1);
              const uint32_t k = pe >> 4;
              if (k == 0u) L(e0) = pv;
              else if (k == 1u) L(e1) = pv;
              else if (k == 2u) L(e2) = pv;
              else L(e3) = pv;
            }
          }
        }
      }
    }
    CO_PH(8);
  }
  WAVE_SYNC();
  /* ---- expand: the four leaves at once, one per row (rules.h co_legal_moves_rows) */
  int nsel = bad < m ? bad : m;
  LV(int, on);
  LV(uint32_t, nb0);
  LV(uint32_t, nb1);
  LV(uint32_t, nmeta);
  LV(uint32_t, l0);
  LV(uint32_t, l1);
  LV(uint32_t, l2);
  LV(int, nl); /* legal moves of the row's leaf */
  LV(uint32_t, lz);    /* the chosen slot's move and prior */
  LV(uint32_t, lpar);  /* the leaf's parent block, the leaf's slot, the parent's meta word */
  LV(uint32_t, lslot);
  LV(uint32_t, lmeta);
  FOR_LANES_HOT {
    L(on) = (lane >> 4) < nsel;
    const uint4 la = sb_leaf[2 * (lane >> 4)], lb = sb_leaf[2 * (lane >> 4) + 1];
    L(lz) = lb.x;
    L(lslot) = lb.y;
    L(lpar) = la.w;
    L(lmeta) = la.z;
    uint64_t b = (uint64_t)la.x | ((uint64_t)la.y << 32);
    uint32_t mm = la.z;
    if (L(on)) co_do_move_lane(&b, &mm, (int)CO_SLOT_MOVE(L(lz)));
    L(nb0) = (uint32_t)b;
    L(nb1) = (uint32_t)(b >> 32);
    L(nmeta) = mm;
  }
  LV(int, lin);
  co_legal_moves_rows(nb0, nb1, nmeta, on, l0, l1, l2, lin, w.lb);
  FOR_LANES_HOT { L(nl) = L(on) ? co_popc32(L(l0)) + co_popc32(L(l1)) + co_popc32(L(l2)) : 0; }
  int term = -1; /* the simulation whose new leaf is terminal: committed behind the others, ends the group */
  {
    /* a terminal leaf ends the group behind it, a full arena in front of it (co_search reports it); the others get
     * their blocks */
    uint32_t used = t.tc.units_used;
    int j = 0;
    for (; j < nsel; ++j) {
      const int n = WAVE_BCAST(nl, 16 * j);
      if (CO_NODE_END(used, n) > t.cap) break;
      if (n == 0) {
        CO_SBS(7, 1);
        term = j;
        break;
      }
      used += CO_NODE_UNITS(n);
    }
    if (j < nsel && term < 0) bad = j; /* (not ordinary, and not handled here) */
    nsel = j;
  }
  CO_PH(14);
  int done = nsel;
  if (nsel > 0) {
    const int n0 = WAVE_BCAST(nl, 0), n1 = WAVE_BCAST(nl, 16), n2 = WAVE_BCAST(nl, 32), n3 = WAVE_BCAST(nl, 48);
    const uint32_t base0 = t.tc.units_used;
    const int noise0 = w.noise_words, k0 = w.gc.n_pending;
    /* ---- commit.  (1) the slots the simulations passed through: every (simulation, level) one lane; a slot several
     * simulations of the group passed takes the LAST one's value (it has the earlier passes in it) */
    const int dl[CO_SB] = {WAVE_BCAST(leafD, 0), WAVE_BCAST(leafD, 16), WAVE_BCAST(leafD, 32), WAVE_BCAST(leafD, 48)};
    FOR_LANES_HOT {
      const int r = lane >> 4, c = lane & 15;
      if (r < nsel && c < L(leafD)) {
        const uint32_t sl = sb_slot[CO_SB_SLOT_AT(r, c)];
        int last = 1;
#pragma unroll
        for (int r2 = 1; r2 < CO_SB; ++r2)
          if (r2 > r && r2 < nsel && c < dl[r2] && sb_slot[CO_SB_SLOT_AT(r2, c)] == sl) last = 0;
        if (last) {
          const uint4 v = sb_cs[CO_SB_AT(r, c)];
          A[sl] = v;
          const uint32_t idx = sl - rc.e0;
          if (idx < rc.ne) rc.ev[idx] = v;
        }
      }
    }
    for (int j = 0; j < nsel; ++j) rc.cs = co_slot_pass(rc.cs);
    CO_PH(9);
    /* (2) the new nodes: blocks in simulation order (the bump pointer of the sequential search), header, edges in
     * ascending move id */
    LV(uint32_t, nblk);
    LV(int, noff); /* generator outputs owed to the leaves queued before this one */
    FOR_LANES_HOT {
      const int r = lane >> 4, c = lane & 15;
      const uint32_t before = (r > 0 ? CO_NODE_UNITS(n0) : 0u) + (r > 1 ? CO_NODE_UNITS(n1) : 0u) + (r > 2 ? CO_NODE_UNITS(n2) : 0u);
      L(nblk) = base0 + before;
      L(noff) = noise0 + (r > 0 ? n0 : 0) + (r > 1 ? n1 : 0) + (r > 2 ? n2 : 0);
      if (r < nsel) {
        const uint32_t b = L(nblk);
        const int depth = (int)CO_META_DEPTH(L(lmeta)) + 1;
        if (c == 0) A[CO_NODE_HDR(b)] = make_uint4(L(nb0), L(nb1), co_meta_make(L(nmeta), depth, L(nl)), L(lpar));
        if (c == 1) A[CO_NODE_INFO(b)] = make_uint4(L(lslot), 0u, 0u, 0u);
        const int c0 = co_popc32(L(l0)), c01 = c0 + co_popc32(L(l1));
#pragma unroll
        for (int q = 0; q < 6; ++q) {
          const int id = 16 * q + c;
          const uint32_t wd = q < 2 ? L(l0) : q < 4 ? L(l1) : L(l2);
          const int bit = id & 31;
          if ((wd >> bit) & 1u) {
            const int rank = (q < 2 ? 0 : q < 4 ? c0 : c01) + co_popc32(wd & ((1u << bit) - 1u));
            A[CO_NODE_EDGE(b, (uint32_t)rank)] = CO_SLOT_EDGE(id);
          }
        }
        /* (3) the leaf's own slot, in its parent's block (and in the root copy when the parent is the root) */
        if (c == 2) {
          const uint4 v = CO_SLOT_NEW(b, co_f2u(1.0f), L(lz), CO_RESULT_NONE);
          A[L(lslot)] = v;
          const uint32_t idx = L(lslot) - rc.e0;
          if (idx < rc.ne) rc.ev[idx] = v;
        }
      }
    }
    {
      const uint32_t units = CO_NODE_FIXED_UNITS * (uint32_t)nsel + (uint32_t)(n0 + (nsel > 1 ? n1 : 0) + (nsel > 2 ? n2 : 0) + (nsel > 3 ? n3 : 0));
      t.tc.units_used = base0 + units;
      if (t.tc.units_used > t.tc.peak_units) t.tc.peak_units = t.tc.units_used;
      w.gc.nodes += (uint32_t)nsel;
      t.tc.searches_done += nsel;
      w.gc.searches += (uint32_t)nsel;
    }
    CO_PH(15);
    CO_PROF_ADD(w, 24, (unsigned long long)nsel);
    if (w.analyse) {
      /* Node::countNodes without a traversal (co_search): every node of a path counts the new node below it */
      for (int j = 0; j < nsel; ++j) {
        const int D = WAVE_BCAST(leafD, 16 * j);
        FOR_LANES_HOT {
          if (lane < D) A[CO_NODE_INFO(sb_block[CO_SB_AT(j, lane)])].z += 1u;
        }
        WAVE_SYNC();
      }
    }
    /* (4) the requests (co_request): state rows, pending-leaf records, cache keys -- leaf k0 + r from row r */
    {
      float *req = w.req;
      uint32_t *pend_leaf = w.pend_leaf, *pend_path = w.pend_path, *pend_n = w.pend_n;
      int32_t *pend_depth = w.pend_depth;
      uint4 *pend_key = w.pend_key;
      FOR_LANES_HOT {
        const int r = lane >> 4, c = lane & 15;
        if (r < nsel) {
          const int k = k0 + r;
          const uint64_t b = (uint64_t)L(nb0) | ((uint64_t)L(nb1) << 32);
          /* Game::writeGameState (game.cpp:45-58): a lane writes its cell's four floats, lanes 0..3 the reserves (the
           * mover's first) and the padding */
          uint4 *row = (uint4 *)(req + (size_t)k * CO_STATE_STRIDE);
          const uint32_t nib = (uint32_t)(b >> (4 * c)) & 15u;
          const uint32_t one = co_f2u(1.0f);
          row[c] = make_uint4((nib & 1u) ? one : 0u, (nib & 2u) ? one : 0u, (nib & 4u) ? one : 0u, (nib & 8u) ? one : 0u);
          const uint32_t pcs = L(nmeta) & 0x3FFFFu;
          const uint32_t rot = CO_META_TO_PLAY(L(nmeta)) ? ((pcs >> 9) | (pcs << 9)) & 0x3FFFFu : pcs;
          if (c < 4) {
            uint32_t f[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int x = 4 * c + i;
              f[i] = x < 6 ? co_f2u((float)((rot >> (3 * x)) & 7u) * 0.25f) : 0u;
            }
            row[16 + c] = make_uint4(f[0], f[1], f[2], f[3]);
          }
          if (c == 4) {
            pend_leaf[k] = L(nblk);
            pend_depth[k] = L(leafD);
          }
          if (c >= 5 && c < 9) pend_n[4 * k + (c - 5)] = c == 5 ? (((uint32_t)L(noff) << 8) | (uint32_t)L(nl)) : c == 6 ? L(l0) : c == 7 ? L(l1) : L(l2);
          if (c == 9 && pend_key) pend_key[k] = make_uint4(L(nb0), L(nb1), rot | 0x80000000u, 0u);
          if (c <= L(leafD)) pend_path[(size_t)k * CO_PATH_MAX + c] = sb_slot[CO_SB_SLOT_AT(r, c)];
        }
      }
      w.gc.n_pending = k0 + nsel;
      w.noise_words = noise0 + n0 + (nsel > 1 ? n1 : 0) + (nsel > 2 ? n2 : 0) + (nsel > 3 ? n3 : 0);
    }
    WAVE_SYNC();
    CO_PH(17);
  }
  if (term >= 0) {
    /* ---- the terminal leaf of simulation `term` (trainmc.cpp:663-682), on the tree the simulations before it have been
     * committed to: its passes, the node, the result carried up (propagateTerminal), the default evaluations of its path
     * replaced by the result.  The root copy is dropped: the caller loads it again and looks at the root's result. */
    const int j = term;
    const int D = WAVE_BCAST(leafD, 16 * j);
    const uint64_t board = (uint64_t)WAVE_BCAST(nb0, 16 * j) | ((uint64_t)WAVE_BCAST(nb1, 16 * j) << 32);
    const uint32_t meta = WAVE_BCAST(nmeta, 16 * j), z = WAVE_BCAST(lz, 16 * j), parent = WAVE_BCAST(lpar, 16 * j);
    const uint32_t child_slot = WAVE_BCAST(lslot, 16 * j);
    const int depth = (int)CO_META_DEPTH(WAVE_BCAST(lmeta, 16 * j)) + 1;
    const int res = WAVE_BCAST(lin, 16 * j) ? CO_RESULT_LOSS : CO_RESULT_DRAW;
    uint32_t *pslot = &sb_slot[CO_SB_SLOT_AT(j, 0)];
    uint32_t *pblock = &sb_block[CO_SB_AT(j, 0)];
    ++t.tc.searches_done;
    w.gc.searches++;
    FOR_LANES_HOT {
      if (lane < D) {
        const uint32_t sl = pslot[lane];
        const uint4 v = sb_cs[CO_SB_AT(j, lane)];
        A[sl] = v;
        const uint32_t idx = sl - rc.e0;
        if (idx < rc.ne) rc.ev[idx] = v;
      }
    }
    WAVE_SYNC();
    const uint32_t none[3] = {0u, 0u, 0u};
    const uint32_t nb = co_emit_node(w, t, board, meta, depth, parent, child_slot, none, 0, res);
    if (nb != CO_NONE) {
      if (w.analyse) {
        FOR_LANES_HOT {
          if (lane < D) A[CO_NODE_INFO(pblock[lane])].z += 1u;
        }
        WAVE_SYNC();
      }
      const float cur_eval = res == CO_RESULT_DRAW ? 0.0f : -1.0f;
      co_store_slot(A, child_slot, CO_SLOT_NEW(nb, co_f2u(cur_eval), z, res), rc);
      co_propagate_terminal(t, pblock, pslot, D);
      FOR_LANES_HOT {
        if (lane < D) {
          int kk = D - lane; /* kk-th ancestor receives eval*(-1)^(kk-1) - 1 */
          float ce = ((kk - 1) & 1) ? (float)((double)cur_eval * -1.0) : cur_eval;
          float add = (float)((double)ce - 1.0);
          uint4 s = A[pslot[lane]];
          s.y = co_f2u(co_u2f(s.y) + add);
          A[pslot[lane]] = s;
        }
      }
      WAVE_SYNC();
      CO_PROF_ADD(w, 5, 1ull);
    }
    rc.valid = 0;
    CO_PH(12);
  }
  int dead_end = 0;
  if (term < 0 && done < m && done == bad) {
    WAVE_SYNC();
    const int D = sb_kn[bad];
    if (D >= 0) {
      /* ---- simulation `bad` found nothing searchable below the node at level D (kNone, trainmc.cpp:625-640), on the tree
       * the simulations before it have been committed to: the node becomes all_visited, the passes along the path are
       * taken back (+1 visit, +1.0 and then -1 visit, -1.0: two float operations, as the reference does them), the search
       * is not counted.  The root copy is dropped. */
      const int j = bad;
      FOR_LANES_HOT {
        if (lane <= D) {
          uint4 v = sb_cs[CO_SB_AT(j, lane)];
          if (lane == D) v = co_slot_set_all_visited(v, 1);
          v = co_slot_set_visits(v, co_slot_visits(v) - 1);
          v.y = co_f2u(co_u2f(v.y) - 1.0f);
          A[sb_slot[CO_SB_SLOT_AT(j, lane)]] = v;
        }
      }
      WAVE_SYNC();
      rc.valid = 0;
      dead_end = 1;
    }
  }
  CO_SBS(0, 1);
  CO_SBS(1, m);
  CO_SBS(2, done);
  CO_SBP(w, 0, 1);
  CO_SBP(w, 1, m);
  CO_SBP(w, 2, done);
  CO_SBP(w, 3, term >= 0);
  CO_SBP(w, 4, term < 0 && !dead_end && done < m);
  CO_SBS(12 + done, 1);
  CO_PROF_ADD(w, 5, (unsigned long long)done);
  /* simulations committed | 0x100: a terminal leaf behind them ended the group (done here) | 0x200: the group stopped at a
   * simulation that is neither ordinary nor a terminal leaf -- the caller's next simulation takes co_search */
  return done | (term >= 0 || dead_end ? 0x100 : 0) | (term < 0 && !dead_end && done < m ? 0x200 : 0);
}
