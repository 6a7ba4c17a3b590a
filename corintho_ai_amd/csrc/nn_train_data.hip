// nn_train_data.hip -- the fitter's data set (FtData, nn_train.h; DESIGN.md, "Network training", "The packed data
// set").  It has two forms.  Expanded: the three arrays of Trainer::writeSamples, 8 symmetry copies of every sample,
// which the networks' input kernels and the loss kernels read through the batch's row indices.  Packed: the
// un-augmented rows of co_k_pack_samples, whose 8n virtual rows (row v = sample v / 8 under symmetry v % 8) exist only
// batch by batch: one launch (ft_k_assemble) writes the batch's rows as the expanded arrays would hold them and the
// same kernels, launched the same way, read that batch through an identity index -- so a step is the same to the bit in
// either form.  Here: ft_k_assemble and the symmetry tables it gathers through (and ft_k_assemble_consistent, the packed
// rows through the consistent move table: CA_AUG_CONSISTENT); the set's buffers, counts and sample weights; the row
// checks and the rows of a call; growing, sliding, dropping, merging and canonicalizing of a packed set; fetch_rows.
#include "nn_train.h"
#include "tables.inc"

/* the engine's symmetry tables (kernels.h CO_SPACE_SYM, CO_MOVE_SYM), from the same initialisers of tables.inc */
__constant__ int32_t FT_SPACE_SYM[CA_NUM_SYMMETRIES][16] = CO_SPACE_SYM_INIT;
__constant__ int32_t FT_MOVE_SYM[CA_NUM_SYMMETRIES][CA_NUM_MOVES] = CO_MOVE_SYM_INIT;

/* where a batch's rows are fetched from: a packed set (sp != null) or an expanded one */
struct FtSource {
  const float *sp, *oc;               /* state_policy[n][166], outcome[n] */
  const float *states, *evals, *probs; /* [n][70], [n], [n][96] */
};

/* The batch of rows[0..B) written compactly: bs[r] = the state, be[r] = the value label and bp[r] = the policy of row
 * rows[r].  Of a packed set that is virtual row v = rows[r]: sample v / 8 under symmetry k = v % 8, the gathers of
 * co_k_write_samples (state cell j < 64 from SS[k][j / 4] * 4 + j % 4, cells 64..69 as they are, policy entry m from
 * MS[k][m]).  One thread per float of the batch's 166-float rows, so a wave writes consecutive floats and reads within
 * one or two 664-byte samples.  WEIGHTED: bw[r] = the row's sample weight as well, next to be[r], from wt (one weight
 * per packed sample or per expanded row).  The two operands stand last, so that the unweighted instantiation, which
 * reads neither, is instruction for instruction the kernel it was before weights existed. */
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void ft_k_assemble(FtSource d, const int32_t *__restrict__ rows, int B,
                                                    float *__restrict__ bs, float *__restrict__ be,
                                                    float *__restrict__ bp, const float *__restrict__ wt,
                                                    float *__restrict__ bw) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * FT_SAMPLE_FLOATS) return;
  const int r = e / FT_SAMPLE_FLOATS, c = e % FT_SAMPLE_FLOATS;
  const int v = rows[r];
  if (d.sp) {
    const int i = v >> 3, k = v & 7;
    const float *src = d.sp + (long)i * FT_SAMPLE_FLOATS;
    if (c < CA_GAME_STATE_SIZE) {
      bs[(long)r * CA_GAME_STATE_SIZE + c] = src[c < 64 ? FT_SPACE_SYM[k][c >> 2] * 4 + (c & 3) : c];
    } else {
      const int m = c - CA_GAME_STATE_SIZE;
      bp[(long)r * CA_NUM_MOVES + m] = src[CA_GAME_STATE_SIZE + FT_MOVE_SYM[k][m]];
    }
    if (c == 0) be[r] = d.oc[i];
    if (WEIGHTED && c == 0) bw[r] = wt[i];
  } else {
    if (c < CA_GAME_STATE_SIZE) {
      bs[(long)r * CA_GAME_STATE_SIZE + c] = d.states[(long)v * CA_GAME_STATE_SIZE + c];
    } else {
      const int m = c - CA_GAME_STATE_SIZE;
      bp[(long)r * CA_NUM_MOVES + m] = d.probs[(long)v * CA_NUM_MOVES + m];
    }
    if (c == 0) be[r] = d.evals[v];
    if (WEIGHTED && c == 0) bw[r] = wt[v];
  }
}

/* The packed half of ft_k_assemble under CA_AUG_CONSISTENT: the policy goes through MC[k], which is MS with rows 2 and
 * 6 exchanged -- row k ^ 4 of the one table where (k & 3) == 2.  A kernel of its own, for a packed set only (d.sp is
 * never null here): sharing a body with ft_k_assemble changed that kernel's weighted instantiation, and the kernels of
 * the reference's pairing stay instruction for instruction what they were before there was a choice. */
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void ft_k_assemble_consistent(FtSource d, const int32_t *__restrict__ rows, int B,
                                                               float *__restrict__ bs, float *__restrict__ be,
                                                               float *__restrict__ bp, const float *__restrict__ wt,
                                                               float *__restrict__ bw) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * FT_SAMPLE_FLOATS) return;
  const int r = e / FT_SAMPLE_FLOATS, c = e % FT_SAMPLE_FLOATS;
  const int v = rows[r];
  const int i = v >> 3, k = v & 7;
  const float *src = d.sp + (long)i * FT_SAMPLE_FLOATS;
  if (c < CA_GAME_STATE_SIZE) {
    bs[(long)r * CA_GAME_STATE_SIZE + c] = src[c < 64 ? FT_SPACE_SYM[k][c >> 2] * 4 + (c & 3) : c];
  } else {
    const int m = c - CA_GAME_STATE_SIZE;
    bp[(long)r * CA_NUM_MOVES + m] = src[CA_GAME_STATE_SIZE + FT_MOVE_SYM[(k & 3) == 2 ? k ^ 4 : k][m]];
  }
  if (c == 0) be[r] = d.oc[i];
  if (WEIGHTED && c == 0) bw[r] = wt[i];
}

/* ------------------------------------------------------------------ host */
void FtData::assemble(const int32_t *rows, int B) {
  const FtSource src = {expanded ? nullptr : sp.p, oc.p, states.p, evals.p, probs.p};
  const int grid = (B * FT_SAMPLE_FLOATS + 255) / 256;
  const bool consistent = !expanded && aug == CA_AUG_CONSISTENT; /* an expanded set's rows are the caller's */
  if (consistent && weighted)
    RT_LAUNCH(ft_k_assemble_consistent<true>, grid, 256, s, src, rows, B, bstates.p, bevals.p, bprobs.p, (const float *)wt.p,
              bwts.p);
  else if (consistent)
    RT_LAUNCH(ft_k_assemble_consistent<false>, grid, 256, s, src, rows, B, bstates.p, bevals.p, bprobs.p,
              (const float *)nullptr, (float *)nullptr);
  else if (weighted)
    RT_LAUNCH(ft_k_assemble<true>, grid, 256, s, src, rows, B, bstates.p, bevals.p, bprobs.p, (const float *)wt.p, bwts.p);
  else
    RT_LAUNCH(ft_k_assemble<false>, grid, 256, s, src, rows, B, bstates.p, bevals.p, bprobs.p, (const float *)nullptr,
              (float *)nullptr);
}

FtBatch FtData::batch(const int32_t *rows, int B) {
  if (expanded) return FtBatch{rows, states.p, evals.p, probs.p, weighted ? wt.p : nullptr};
  assemble(rows, B);
  return FtBatch{ident.p, bstates.p, bevals.p, bprobs.p, weighted ? bwts.p : nullptr};
}

void FtData::need_data() const {
  if (n <= 0) throw CaError(CA_ERR_STATE, "ca_fitter: no data (ca_fitter_set_data, ca_fitter_add_samples)");
}
void FtData::check_batch(int32_t batch) const {
  if (batch < 1 || batch > max_batch) throw CaError(CA_ERR_ARG, "ca_fitter: batch must be in [1, max_batch]");
}
void FtData::check_rows(const int32_t *rows, int32_t nr) const {
  if (nr < 0 || nr > n) throw CaError(CA_ERR_ARG, "ca_fitter: more rows than the data set holds");
  check_range(rows, nr);
}
void FtData::check_range(const int32_t *rows, int32_t nr) const {
  for (int32_t i = 0; i < nr; ++i)
    if (rows[i] < 0 || rows[i] >= n) throw CaError(CA_ERR_ARG, "ca_fitter: row index out of range");
}

/* Room in idx for the nr rows of a call: an expanded set has it from set_expanded, a packed one takes what its largest
 * call asked for, not a share of its capacity. */
void FtData::need_idx(int32_t nr) {
  if (idx_cap >= nr) return;
  idx.alloc((size_t)nr, s);
  idx_cap = nr;
}
const int32_t *FtData::upload(const int32_t *rows, int32_t nr) {
  rt_h2d(idx.p, rows, (size_t)nr * sizeof(int32_t), s);
  return idx.p;
}

/* the buffers of an assembled batch */
void FtData::need_stage() {
  if (bidx.p) return;
  std::vector<int32_t> id((size_t)max_batch);
  for (int32_t i = 0; i < max_batch; ++i) id[i] = i;
  bstates.alloc((size_t)max_batch * CA_GAME_STATE_SIZE, s);
  bevals.alloc((size_t)max_batch, s);
  bprobs.alloc((size_t)max_batch * CA_NUM_MOVES, s);
  bwts.alloc((size_t)max_batch, s);
  ident.alloc((size_t)max_batch, s);
  rt_h2d(ident.p, id.data(), id.size() * sizeof(int32_t), s);
  rt_sync(s); /* id is a local */
  bidx.alloc((size_t)max_batch, s);
}

void FtData::clear() {
  n = 0, ns = 0, cap = 0, idx_cap = 0, expanded = false, weighted = false;
  states.release(), evals.release(), probs.release(), sp.release(), oc.release(), idx.release(), wt.release();
}

void FtData::set_expanded(const float *st, const float *ev, const float *pr, int32_t count) {
  clear(); /* no data while the buffers are being replaced: a failure below leaves the fitter without, not with half */
  expanded = true;
  states.alloc((size_t)count * CA_GAME_STATE_SIZE, s);
  evals.alloc((size_t)count, s);
  probs.alloc((size_t)count * CA_NUM_MOVES, s);
  idx.alloc((size_t)count, s);
  idx_cap = count;
  rt_h2d(states.p, st, (size_t)count * CA_GAME_STATE_SIZE * sizeof(float), s);
  rt_h2d(evals.p, ev, (size_t)count * sizeof(float), s);
  rt_h2d(probs.p, pr, (size_t)count * CA_NUM_MOVES * sizeof(float), s);
  rt_sync(s);
  n = count;
}

/* The packed rows [first, first + count) to the front of the buffers they are in (a slide of the window), device to
 * device without a second buffer: in pieces of `first` rows from the front, each of which ends before its source
 * begins, queued in order on one stream.  Only a drop of less than 1/64 of what stays goes through new buffers. */
void FtData::slide_samples(int32_t first, int32_t count) {
  if ((int64_t)first * 64 < count) {
    move_samples(first, count, cap);
    return;
  }
  for (int32_t d = 0; d < count; d += first) {
    const size_t k = (size_t)(count - d < first ? count - d : first);
    rt_d2d(sp.p + (size_t)d * FT_SAMPLE_FLOATS, sp.p + ((size_t)d + first) * FT_SAMPLE_FLOATS,
           k * FT_SAMPLE_FLOATS * sizeof(float), s);
    rt_d2d(oc.p + d, oc.p + d + first, k * sizeof(float), s);
    if (weighted) rt_d2d(wt.p + d, wt.p + d + first, k * sizeof(float), s);
  }
  rt_sync(s);
}

/* the packed rows [first, first + count) to the front of new buffers with room for new_cap samples, device to device */
void FtData::move_samples(int32_t first, int32_t count, int32_t new_cap) {
  DevBuf<float> nsp, noc, nwt;
  nsp.alloc((size_t)new_cap * FT_SAMPLE_FLOATS, s);
  noc.alloc((size_t)new_cap, s);
  if (weighted) {
    nwt.alloc((size_t)new_cap, s);
    rt_d2d(nwt.p, wt.p + first, (size_t)count * sizeof(float), s);
  }
  rt_d2d(nsp.p, sp.p + (size_t)first * FT_SAMPLE_FLOATS, (size_t)count * FT_SAMPLE_FLOATS * sizeof(float), s);
  rt_d2d(noc.p, oc.p + first, (size_t)count * sizeof(float), s);
  rt_sync(s); /* before the old buffers are freed */
  std::swap(sp, nsp);
  std::swap(oc, noc);
  if (weighted) std::swap(wt, nwt);
  cap = new_cap;
}

void FtData::reserve(int32_t add) {
  if (expanded) throw CaError(CA_ERR_STATE, "ca_fitter: the data set is expanded (ca_fitter_clear_data first)");
  if (weighted) throw CaError(CA_ERR_STATE, "ca_fitter: the data set carries sample weights (ca_fitter_clear_data first)");
  if (add < 0) throw CaError(CA_ERR_ARG, "ca_fitter: negative sample count");
  const int64_t need = (int64_t)ns + add, most = INT32_MAX / CA_NUM_SYMMETRIES;
  if (need > most) throw CaError(CA_ERR_ARG, "ca_fitter: more than INT32_MAX virtual rows");
  need_stage();
  if (need <= cap) return;
  int64_t nc = 2 * (int64_t)cap > need ? 2 * (int64_t)cap : need;
  nc = nc < 1024 ? 1024 : nc > most ? most : nc;
  move_samples(0, ns, (int32_t)nc);
}

void FtData::add(const float *state_policy, const float *outcome, int32_t count, FtCopy copy) {
  reserve(count);
  copy(sp_end(), state_policy, (size_t)count * FT_SAMPLE_FLOATS * sizeof(float), s);
  copy(oc_end(), outcome, (size_t)count * sizeof(float), s);
  rt_sync(s);
  added(count);
}

void FtData::drop(int32_t n_oldest) {
  if (expanded) throw CaError(CA_ERR_STATE, "ca_fitter_drop_samples: the data set is expanded");
  if (n_oldest < 0 || n_oldest > ns) throw CaError(CA_ERR_ARG, "ca_fitter_drop_samples: more than the set holds");
  if (n_oldest == 0) return;
  rt_sync(s);
  if (n_oldest < ns) slide_samples(n_oldest, ns - n_oldest);
  added(-n_oldest);
}

void FtData::merge(bool normalize, int32_t *before, int32_t *after) {
  if (expanded) throw CaError(CA_ERR_STATE, "ca_fitter_merge_duplicates: the data set is expanded");
  if (ns <= 0) throw CaError(CA_ERR_STATE, "ca_fitter_merge_duplicates: no samples (ca_fitter_add_samples)");
  rt_sync(s);
  FtMerged m = ft_merge_duplicates(s, sp.p, oc.p, weighted ? wt.p : nullptr, ns, normalize);
  /* the merged samples are in buffers of their own: swapped in as move_samples does; nothing waits on the old ones */
  *before = ns;
  *after = m.count;
  std::swap(sp, m.sp);
  std::swap(oc, m.oc);
  std::swap(wt, m.wt);
  weighted = true;
  cap = m.cap;
  added(m.count - ns);
}

void FtData::set_augmentation(int32_t a) {
  if (a != CA_AUG_REFERENCE && a != CA_AUG_CONSISTENT)
    throw CaError(CA_ERR_ARG, "ca_fitter_set_augmentation: the augmentation must be CA_AUG_REFERENCE or CA_AUG_CONSISTENT");
  rt_sync(s);
  aug = a;
}

void FtData::canonicalize(int32_t *moved) {
  if (expanded) throw CaError(CA_ERR_STATE, "ca_fitter_canonicalize: the data set is expanded");
  if (ns <= 0) throw CaError(CA_ERR_STATE, "ca_fitter_canonicalize: no samples (ca_fitter_add_samples)");
  rt_sync(s);
  *moved = ft_canonicalize(s, sp.p, ns);
}

void FtData::set_weights(const float *weights, int32_t count) {
  need_data();
  if (!weights) { /* back to the unweighted set */
    rt_sync(s);
    weighted = false;
    wt.release();
    return;
  }
  if (count != units())
    throw CaError(CA_ERR_ARG, "ca_fitter_set_sample_weights: " + std::to_string(units()) + " weights are needed, got " +
                                  std::to_string(count));
  for (int32_t i = 0; i < count; ++i)
    if (!ft_finite_nonneg(weights[i])) throw CaError(CA_ERR_ARG, "ca_fitter_set_sample_weights: every weight must be finite and >= 0");
  if (!weighted) wt.alloc((size_t)(expanded ? n : cap), s);
  rt_h2d(wt.p, weights, (size_t)count * sizeof(float), s);
  rt_sync(s);
  weighted = true;
}

void FtData::get_weights(float *out, int32_t count) {
  need_data();
  if (!out || count != units())
    throw CaError(CA_ERR_ARG, "ca_fitter_get_sample_weights: null output, or not the " + std::to_string(units()) +
                                  " weights of the set");
  if (!weighted) { /* an unweighted set counts every row once */
    for (int32_t i = 0; i < count; ++i) out[i] = 1.0f;
    return;
  }
  rt_d2h(out, wt.p, (size_t)count * sizeof(float), s);
  rt_sync(s);
}

void FtData::fetch_rows(const int32_t *rows, int32_t n_rows, float *st, float *ev, float *pr) {
  need_data();
  if (!rows || !st || !ev || !pr || n_rows < 0) throw CaError(CA_ERR_ARG, "ca_fitter_fetch_rows: null or negative");
  check_range(rows, n_rows);
  need_stage();
  for (int32_t r0 = 0; r0 < n_rows; r0 += max_batch) {
    const int B = n_rows - r0 < max_batch ? n_rows - r0 : max_batch;
    rt_h2d(bidx.p, rows + r0, (size_t)B * sizeof(int32_t), s);
    assemble(bidx.p, B);
    rt_d2h(st + (size_t)r0 * CA_GAME_STATE_SIZE, bstates.p, (size_t)B * CA_GAME_STATE_SIZE * sizeof(float), s);
    rt_d2h(ev + r0, bevals.p, (size_t)B * sizeof(float), s);
    rt_d2h(pr + (size_t)r0 * CA_NUM_MOVES, bprobs.p, (size_t)B * CA_NUM_MOVES * sizeof(float), s);
    rt_sync(s);
  }
}
