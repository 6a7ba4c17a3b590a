// nn_samples.hip -- merging the duplicate positions of a packed data set on the device (ca_fitter_merge_duplicates,
// corintho_hip.h; DESIGN.md, "Merging duplicate positions").  Two samples are equal when their 70 state floats have the
// same bits; a group of equal samples becomes one sample at the rank of its first member, with the weighted mean of the
// members' policies and outcomes, summed in float64 over the members in ascending index, and the sum of their weights.
//
//   1  sm_k_insert    a 64-bit hash of the state's words; an open-addressing table of >= 2 n slots that hold sample
//                     indices: an empty slot is claimed by compare-and-swap, a slot whose sample has the same 70 words
//                     takes atomicMin of the index.  Whatever the timing, every state owns one slot and the slot ends as
//                     the state's smallest index, its representative
//   2  sm_k_rep       rep[i] = the representative of sample i
//   3  sort           stable least-significant-digit radix sort of (rep, index), 8 bits a pass: per 256-key tile a
//                     histogram (sm_k_hist), one exclusive scan over [digit][tile], and the scatter (sm_k_scatter) in
//                     which a key's rank among its tile's equal digits is counted in LDS.  Groups come out in the order
//                     of their first members, a group's members in ascending index
//   4  flags, scan    leaders of the sorted keys -> the groups' ranks and first positions (sm_k_flags, sm_k_starts)
//   5  sm_k_segment   one wavefront per group: lanes hold the 96 policy sums and the outcome sum in float64 and walk
//                     the members in order
//   6  sm_k_total     the sum of the groups' weights, in order (normalisation), and the scan of the groups that stay
//   7  sm_k_compact   groups of weight zero leave; the others go to buffers of their own, the weights scaled
// Integer atomics only, and no workgroup waits for another: every scan and every sort pass is a launch of its own.  The
// probe loop is bounded by the table's size and raises a flag (CA_ERR_INTERNAL) when it runs out; so does a sort
// position or a member index outside [0, n).  The products w * p of two float32 are exact in float64; the division and
// the conversions are IEEE (the build has no fast-math: build.py).
//
// Also here: the canonical orientation of a packed set's samples (ca_fitter_canonicalize; DESIGN.md, "Canonical
// orientation"), sm_k_canonicalize, after which the merge above is a merge up to the eight symmetries.
#include "nn_train.h"
#include "tables.inc"

/* the engine's symmetry tables (kernels.h CO_SPACE_SYM, CO_MOVE_SYM), from the same initialisers of tables.inc */
__constant__ int32_t SM_SPACE_SYM[CA_NUM_SYMMETRIES][16] = CO_SPACE_SYM_INIT;
__constant__ int32_t SM_MOVE_SYM[CA_NUM_SYMMETRIES][CA_NUM_MOVES] = CO_MOVE_SYM_INIT;

#define SM_STATE CA_GAME_STATE_SIZE
#define SM_ROW (CA_GAME_STATE_SIZE + CA_NUM_MOVES)
#define SM_TILE 256  /* keys of one sort tile: one per thread */
#define SM_SCAN 1024 /* entries of one scan block: one per thread */

__global__ __launch_bounds__(256) void sm_k_insert(const uint32_t *__restrict__ sp, int n, int32_t *table, uint32_t mask,
                                                  int32_t *__restrict__ slot_of, uint32_t *flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t *a = sp + (long)i * SM_ROW;
  uint64_t h = 0x9E3779B97F4A7C15ull;
  for (int c = 0; c < SM_STATE; ++c) { /* the words are floats, mostly 0.0 and 1.0: the shift brings their high bits down */
    h = (h ^ a[c]) * 0x100000001B3ull;
    h ^= h >> 29;
  }
  h ^= h >> 32;
  uint32_t slot = (uint32_t)h & mask;
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    const int32_t prev = atomicCAS(&table[slot], -1, i);
    if (prev == -1) { /* claimed */
      slot_of[i] = (int32_t)slot;
      return;
    }
    /* the slot's sample: whichever index is read, its state is the slot's for good (atomicMin swaps equal states) */
    const uint32_t *b = sp + (long)prev * SM_ROW;
    bool same = true;
    for (int c = 0; c < SM_STATE; ++c)
      if (a[c] != b[c]) {
        same = false;
        break;
      }
    if (same) {
      atomicMin(&table[slot], i);
      slot_of[i] = (int32_t)slot;
      return;
    }
    slot = (slot + 1) & mask;
  }
  slot_of[i] = -1;
  *flag = 1u;
}

__global__ __launch_bounds__(256) void sm_k_rep(const int32_t *__restrict__ table, const int32_t *__restrict__ slot_of, int n,
                                               int32_t *__restrict__ key, int32_t *__restrict__ val, uint32_t *flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t sl = slot_of[i];
  int32_t r = sl >= 0 ? table[sl] : -1;
  if (r < 0 || r > i) { /* cannot be: the slot holds the smallest index of i's state */
    *flag = 1u;
    r = i;
  }
  key[i] = r;
  val[i] = i;
}

/* hist[d][tile] = how many keys of the tile have digit d */
__global__ __launch_bounds__(SM_TILE) void sm_k_hist(const int32_t *__restrict__ key, int n, int shift, int32_t *__restrict__ hist,
                                                    int tiles) {
  __shared__ int h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int i = blockIdx.x * SM_TILE + threadIdx.x;
  if (i < n) atomicAdd(&h[(key[i] >> shift) & 255], 1);
  __syncthreads();
  hist[(long)threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];
}

/* off[d][tile]: the exclusive scan of hist, the position of the tile's first key of digit d.  A key goes behind the
 * tile's earlier keys of the same digit (counted in LDS), which keeps the pass stable. */
__global__ __launch_bounds__(SM_TILE) void sm_k_scatter(const int32_t *__restrict__ key, const int32_t *__restrict__ val, int n,
                                                       int shift, const int32_t *__restrict__ off, int tiles,
                                                       int32_t *__restrict__ key_out, int32_t *__restrict__ val_out,
                                                       uint32_t *flag) {
  __shared__ int dg[SM_TILE];
  const int t = threadIdx.x, i = blockIdx.x * SM_TILE + t;
  const int32_t k = i < n ? key[i] : 0;
  const int d = i < n ? (k >> shift) & 255 : 256; /* 256: no key's digit */
  dg[t] = d;
  __syncthreads();
  if (i >= n) return;
  int r = 0;
  for (int j = 0; j < t; ++j) r += dg[j] == d; /* every lane reads the same word: a broadcast */
  const int pos = off[(long)d * tiles + blockIdx.x] + r;
  if ((unsigned)pos >= (unsigned)n) {
    *flag = 1u;
    return;
  }
  key_out[pos] = k;
  val_out[pos] = val[i];
}

/* inclusive scan of one value per thread of a 1024-thread block, in t; returns the thread's inclusive sum */
__device__ __forceinline__ int sm_block_scan(int *t, int v) {
  const int x = threadIdx.x;
  t[x] = v;
  __syncthreads();
  for (int o = 1; o < SM_SCAN; o <<= 1) {
    const int y = x >= o ? t[x - o] : 0;
    __syncthreads();
    t[x] += y;
    __syncthreads();
  }
  return t[x];
}

/* exclusive scan of a[0..m) in three launches: within blocks of 1024 (the blocks' totals to sums), the totals by one
 * block, and the totals added */
__global__ __launch_bounds__(SM_SCAN) void sm_k_scan_block(int32_t *__restrict__ a, long m, int32_t *__restrict__ sums) {
  __shared__ int t[SM_SCAN];
  const long i = (long)blockIdx.x * SM_SCAN + threadIdx.x;
  const int v = i < m ? a[i] : 0;
  const int inc = sm_block_scan(t, v);
  if (i < m) a[i] = inc - v;
  if (threadIdx.x == SM_SCAN - 1) sums[blockIdx.x] = inc;
}

__global__ __launch_bounds__(SM_SCAN) void sm_k_scan_sums(int32_t *__restrict__ sums, int nb) {
  __shared__ int t[SM_SCAN];
  int carry = 0;
  for (int base = 0; base < nb; base += SM_SCAN) {
    const int i = base + threadIdx.x;
    const int v = i < nb ? sums[i] : 0;
    const int inc = sm_block_scan(t, v);
    if (i < nb) sums[i] = carry + inc - v;
    carry += t[SM_SCAN - 1];
    __syncthreads(); /* t is written again by the next chunk */
  }
}

__global__ __launch_bounds__(SM_SCAN) void sm_k_scan_add(int32_t *__restrict__ a, long m, const int32_t *__restrict__ sums) {
  const long i = (long)blockIdx.x * SM_SCAN + threadIdx.x;
  if (i < m) a[i] += sums[blockIdx.x];
}

/* lead[p] = 1 where a group begins in the sorted keys; lead[n] = 0, so that its exclusive scan ends in the group count */
__global__ __launch_bounds__(256) void sm_k_flags(const int32_t *__restrict__ key, int n, int32_t *__restrict__ lead) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p > n) return;
  lead[p] = p < n && (p == 0 || key[p] != key[p - 1]);
}

/* rank[p]: the exclusive scan of lead.  start[g] = the first position of group g, start[groups] = n */
__global__ __launch_bounds__(256) void sm_k_starts(const int32_t *__restrict__ key, const int32_t *__restrict__ rank, int n,
                                                  int32_t *__restrict__ start) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p > n) return;
  if (p == n || p == 0 || key[p] != key[p - 1]) start[rank[p]] = p; /* rank[p] <= p <= n: start has n + 1 entries */
}

/* One wavefront per group g, its members val[start[g] .. start[g + 1]) in ascending sample index.  Lane l sums policy
 * entry l and, l < 32: policy entry 64 + l, l == 32: the outcome; every lane sums the weight.  The members' indices,
 * weights and outcomes are loaded 64 at a time, one per lane, and handed round; the loads of the policy rows do not
 * depend on one another.  Leaves the merged sample in tsp[g], toc[g], its weight in tw[g] and keep[g] = (weight > 0). */
__global__ __launch_bounds__(256) void sm_k_segment(const float *__restrict__ sp, const float *__restrict__ oc,
                                                   const float *__restrict__ wt, const int32_t *__restrict__ val,
                                                   const int32_t *__restrict__ start, int groups, int n,
                                                   float *__restrict__ tsp, float *__restrict__ toc, double *__restrict__ tw,
                                                   int32_t *__restrict__ keep, uint32_t *flag) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g > groups) return; /* whole waves leave; the kernel has no barrier */
  if (g == groups) {
    if (lane == 0) keep[g] = 0; /* the scan's last entry */
    return;
  }
  const int p0 = start[g], p1 = start[g + 1];
  double a0 = 0.0, a1 = 0.0, W = 0.0;
  int first = 0;
  bool bad = p0 < 0 || p1 > n || p0 >= p1;
  for (int base = p0; base < p1 && !bad; base += 64) {
    const int cnt = p1 - base < 64 ? p1 - base : 64;
    int mi = lane < cnt ? val[base + lane] : 0;
    if ((unsigned)mi >= (unsigned)n) mi = -1;
    if (__any(mi < 0)) {
      bad = true;
      break;
    }
    const float mw = lane < cnt ? (wt ? wt[mi] : 1.0f) : 0.0f;
    const float mz = lane < cnt ? oc[mi] : 0.0f;
    if (base == p0) first = __shfl(mi, 0);
    for (int k = 0; k < cnt; k += 4) { /* four members' rows in flight, then their terms in order */
      float w[4], x0[4], x1[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kk = k + j < cnt ? k + j : k;
        const float *row = sp + (long)__shfl(mi, kk) * SM_ROW + SM_STATE;
        const float z = __shfl(mz, kk);
        w[j] = __shfl(mw, kk);
        x0[j] = row[lane];
        x1[j] = lane < 32 ? row[64 + lane] : z;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (k + j < cnt) {
          const double dw = (double)w[j];
          a0 += dw * (double)x0[j];
          a1 += dw * (double)x1[j];
          W += dw;
        }
    }
  }
  if (bad) { /* (wave-uniform) cannot be: start and val come from the sort */
    if (lane == 0) {
      *flag = 1u;
      tw[g] = 0.0;
      keep[g] = 0;
    }
    return;
  }
  const bool some = W > 0.0;
  float *out = tsp + (long)g * SM_ROW;
  const float *src = sp + (long)first * SM_ROW;
  out[lane] = src[lane];
  if (lane < SM_STATE - 64) out[64 + lane] = src[64 + lane];
  out[SM_STATE + lane] = some ? (float)(a0 / W) : 0.0f;
  const float r1 = some ? (float)(a1 / W) : 0.0f;
  if (lane < 32) out[SM_STATE + 64 + lane] = r1;
  if (lane == 32) toc[g] = r1;
  if (lane == 0) {
    tw[g] = W;
    keep[g] = some ? 1 : 0;
  }
}

/* total[0] = tw[0] + tw[1] + ... in that order, by one thread; the 256 load for it.  (A group of weight zero adds
 * nothing, so this is the sum over the groups that stay.) */
__global__ __launch_bounds__(256) void sm_k_total(const double *__restrict__ tw, int groups, double *__restrict__ total) {
  __shared__ double t[256];
  double s = 0.0;
  for (int base = 0; base < groups; base += 256) {
    t[threadIdx.x] = base + threadIdx.x < groups ? tw[base + threadIdx.x] : 0.0;
    __syncthreads();
    if (threadIdx.x == 0)
      for (int k = 0; k < 256; ++k) s += t[k];
    __syncthreads();
  }
  if (threadIdx.x == 0) total[0] = s;
}

/* rank[g]: the exclusive scan of keep, rank[groups] = how many stay.  One thread per float of the groups' rows. */
__global__ __launch_bounds__(256) void sm_k_compact(const float *__restrict__ tsp, const float *__restrict__ toc,
                                                   const double *__restrict__ tw, const int32_t *__restrict__ rank, int groups,
                                                   int normalize, const double *__restrict__ total, int cap,
                                                   float *__restrict__ osp, float *__restrict__ ooc, float *__restrict__ owt) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)groups * SM_ROW) return;
  const int g = (int)(e / SM_ROW), c = (int)(e % SM_ROW);
  const double w = tw[g];
  if (!(w > 0.0)) return;
  const int r = rank[g];
  if (r >= cap) return; /* (cap is rank[groups]: cannot be) */
  osp[(long)r * SM_ROW + c] = tsp[e];
  if (c == 0) {
    ooc[r] = toc[g];
    owt[r] = (float)(normalize ? w * ((double)rank[groups] / total[0]) : w);
  }
}

/* The canonical orientation of a sample (ca_fitter_canonicalize, corintho_hip.h; DESIGN.md, "Canonical orientation"),
 * in place.  One wavefront per sample, four per workgroup as sm_k_segment.  Lane l holds board word l as its bit
 * pattern; candidate k is one cross-lane gather of it, the source lane SS[k][l / 4] * 4 + l % 4 from the table.  A
 * candidate is compared with the best so far by the ballot of the lanes where they differ: the first such lane holds
 * the most significant difference, and the two words there decide, as unsigned integers.  Everything the decision
 * reads is the same in all lanes, so it is wave-uniform and the kernel has no LDS and no barrier.  On a tie the earlier
 * k stays.  The policy moves through MC[k*] (MS with rows 2 and 6 exchanged, from the one table) in the same way: two
 * registers hold its 96 entries.  The row's floats are all in registers before any is stored, and a sample with
 * k* == 0 stores nothing; cells 64..69 never move.  moved: the count of samples with k* != 0, an integer atomic. */
__global__ __launch_bounds__(256) void sm_k_canonicalize(float *__restrict__ sp, int n, int32_t *__restrict__ moved) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return; /* whole waves leave; the kernel has no barrier */
  uint32_t *row = (uint32_t *)sp + (long)i * SM_ROW;
  const uint32_t w = row[lane];
  const uint32_t p0 = row[SM_STATE + lane];
  const uint32_t p1 = lane < CA_NUM_MOVES - 64 ? row[SM_STATE + 64 + lane] : 0u;
  uint32_t best = w;
  int kb = 0;
  for (int k = 1; k < CA_NUM_SYMMETRIES; ++k) {
    const uint32_t cand = (uint32_t)__shfl((int)w, SM_SPACE_SYM[k][lane >> 2] * 4 + (lane & 3));
    const unsigned long long diff = __ballot(cand != best);
    if (diff == 0ull) continue; /* (wave-uniform) a tie: the lower k stays */
    const int at = __ffsll(diff) - 1;
    const uint32_t a = (uint32_t)__shfl((int)cand, at), b = (uint32_t)__shfl((int)best, at);
    if (a < b) {
      best = cand;
      kb = k;
    }
  }
  if (kb == 0) return; /* (wave-uniform) */
  const int km = (kb & 3) == 2 ? kb ^ 4 : kb; /* MC's row kb */
  const int m0 = SM_MOVE_SYM[km][lane], m1 = lane < CA_NUM_MOVES - 64 ? SM_MOVE_SYM[km][64 + lane] : 0;
  /* entry m comes from lane m % 64 of the register that holds it; every lane takes part in every gather */
  const uint32_t q0a = (uint32_t)__shfl((int)p0, m0 & 63), q0b = (uint32_t)__shfl((int)p1, m0 & 63);
  const uint32_t q1a = (uint32_t)__shfl((int)p0, m1 & 63), q1b = (uint32_t)__shfl((int)p1, m1 & 63);
  row[lane] = best;
  row[SM_STATE + lane] = m0 < 64 ? q0a : q0b;
  if (lane < CA_NUM_MOVES - 64) row[SM_STATE + 64 + lane] = m1 < 64 ? q1a : q1b;
  if (lane == 0) atomicAdd(moved, 1);
}

/* ------------------------------------------------------------------ host */
int32_t ft_canonicalize(rt_stream_t s, float *sp, int32_t n) {
  if (n <= 0) return 0;
  DevBuf<int32_t> moved;
  moved.alloc(1, s); /* zeroed */
  RT_LAUNCH(sm_k_canonicalize, (n + 3) / 4, 256, s, sp, n, moved.p);
  int32_t m = 0;
  rt_d2h(&m, moved.p, sizeof(m), s);
  rt_sync(s);
  if (m < 0 || m > n) throw CaError(CA_ERR_INTERNAL, "ca_fitter_canonicalize: moved count out of range");
  return m;
}

/* exclusive scan of a[0..m) in place; sums: room for ceil(m / 1024) values */
static void sm_scan(rt_stream_t s, int32_t *a, long m, int32_t *sums) {
  const int nb = (int)((m + SM_SCAN - 1) / SM_SCAN);
  RT_LAUNCH(sm_k_scan_block, nb, SM_SCAN, s, a, m, sums);
  RT_LAUNCH(sm_k_scan_sums, 1, SM_SCAN, s, sums, nb);
  RT_LAUNCH(sm_k_scan_add, nb, SM_SCAN, s, a, m, (const int32_t *)sums);
}

static void sm_check(rt_stream_t s, const uint32_t *flag, const char *where) {
  uint32_t v = 0;
  rt_d2h(&v, flag, sizeof(v), s);
  rt_sync(s);
  if (v) throw CaError(CA_ERR_INTERNAL, std::string("ca_fitter_merge_duplicates: ") + where);
}

FtMerged ft_merge_duplicates(rt_stream_t s, const float *sp, const float *oc, const float *wt, int32_t n, bool normalize) {
  FtMerged out;
  if (n <= 0) return out;
  const int grid = (n + 255) / 256, grid1 = (n + 1 + 255) / 256;
  /* 1, 2: the representatives */
  uint32_t slots = 1024;
  while (slots < 2u * (uint32_t)n) slots <<= 1; /* n <= INT32_MAX / 8: no overflow */
  DevBuf<uint32_t> flag;
  DevBuf<int32_t> table, slot_of, key[2], val[2];
  flag.alloc(1, s);
  table.alloc(slots, s);
  rt_memset(table.p, 0xff, (size_t)slots * sizeof(int32_t), s); /* -1: empty */
  slot_of.alloc((size_t)n, s);
  for (int k = 0; k < 2; ++k) key[k].alloc((size_t)n, s), val[k].alloc((size_t)n, s);
  RT_LAUNCH(sm_k_insert, grid, 256, s, (const uint32_t *)sp, n, table.p, slots - 1, slot_of.p, flag.p);
  sm_check(s, flag.p, "the hash table ran full");
  RT_LAUNCH(sm_k_rep, grid, 256, s, (const int32_t *)table.p, (const int32_t *)slot_of.p, n, key[0].p, val[0].p, flag.p);
  /* 3: stable sort of (rep, index) by rep */
  const int tiles = (n + SM_TILE - 1) / SM_TILE;
  const long hn = 256L * tiles;
  DevBuf<int32_t> hist, sums;
  hist.alloc((size_t)hn, s);
  const long longest = hn > (long)n + 1 ? hn : (long)n + 1;
  sums.alloc((size_t)((longest + SM_SCAN - 1) / SM_SCAN), s);
  int bits = 1;
  while (bits < 31 && (1L << bits) < n) ++bits;
  int cur = 0;
  for (int shift = 0; shift < bits; shift += 8) {
    RT_LAUNCH(sm_k_hist, tiles, SM_TILE, s, (const int32_t *)key[cur].p, n, shift, hist.p, tiles);
    sm_scan(s, hist.p, hn, sums.p);
    RT_LAUNCH(sm_k_scatter, tiles, SM_TILE, s, (const int32_t *)key[cur].p, (const int32_t *)val[cur].p, n, shift,
              (const int32_t *)hist.p, tiles, key[cur ^ 1].p, val[cur ^ 1].p, flag.p);
    cur ^= 1;
  }
  /* 4: the groups */
  DevBuf<int32_t> rank, start;
  rank.alloc((size_t)n + 1, s);
  start.alloc((size_t)n + 1, s);
  RT_LAUNCH(sm_k_flags, grid1, 256, s, (const int32_t *)key[cur].p, n, rank.p);
  sm_scan(s, rank.p, (long)n + 1, sums.p);
  RT_LAUNCH(sm_k_starts, grid1, 256, s, (const int32_t *)key[cur].p, (const int32_t *)rank.p, n, start.p);
  int32_t groups = 0;
  rt_d2h(&groups, rank.p + n, sizeof(groups), s);
  sm_check(s, flag.p, "the sort left its range"); /* (synchronises) */
  if (groups < 1 || groups > n) throw CaError(CA_ERR_INTERNAL, "ca_fitter_merge_duplicates: group count out of range");
  /* the stream is idle: what the groups' pass does not read goes before its buffers come */
  table.release(), slot_of.release(), hist.release(), key[0].release(), key[1].release(), val[cur ^ 1].release();
  /* 5, 6: the groups' samples and weights */
  DevBuf<float> tsp, toc;
  DevBuf<double> tw, total;
  DevBuf<int32_t> keep;
  tsp.alloc((size_t)groups * SM_ROW, s);
  toc.alloc((size_t)groups, s);
  tw.alloc((size_t)groups, s);
  total.alloc(1, s);
  keep.alloc((size_t)groups + 1, s);
  RT_LAUNCH(sm_k_segment, (groups + 1 + 3) / 4, 256, s, sp, oc, wt, (const int32_t *)val[cur].p, (const int32_t *)start.p, groups,
            n, tsp.p, toc.p, tw.p, keep.p, flag.p);
  RT_LAUNCH(sm_k_total, 1, 256, s, (const double *)tw.p, groups, total.p);
  sm_scan(s, keep.p, (long)groups + 1, sums.p);
  int32_t after = 0;
  rt_d2h(&after, keep.p + groups, sizeof(after), s);
  sm_check(s, flag.p, "a group's members left their range");
  if (after < 0 || after > groups) throw CaError(CA_ERR_INTERNAL, "ca_fitter_merge_duplicates: kept count out of range");
  /* 7: into buffers of their own */
  out.count = after;
  out.cap = after > 0 ? after : 1;
  out.sp.alloc((size_t)out.cap * SM_ROW, s);
  out.oc.alloc((size_t)out.cap, s);
  out.wt.alloc((size_t)out.cap, s);
  const long floats = (long)groups * SM_ROW;
  RT_LAUNCH(sm_k_compact, (int)((floats + 255) / 256), 256, s, (const float *)tsp.p, (const float *)toc.p, (const double *)tw.p,
            (const int32_t *)keep.p, groups, normalize ? 1 : 0, (const double *)total.p, after, out.sp.p, out.oc.p, out.wt.p);
  rt_sync(s); /* before the temporaries are freed */
  return out;
}
