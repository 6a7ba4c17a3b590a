/* corintho_hip.h -- C ABI of libcorintho_hip.so, the MI355X self-play engine.
 *
 * Drop-in boundary for the reference's hot path.  The reference exposes a C++
 * class consumed at source level by Cython
 * (corintho_ai/python/main.pyx:17-38  `cdef cppclass Trainer`, declared in
 * corintho_ai/cpp/include/trainer.h:17-81).  Each entry point below replaces
 * one member of that class; corintho_ai_amd/cpp/trainer.h wraps them back into
 * a `class Trainer` with the reference's exact signatures, so main.pyx compiles
 * against it unchanged.
 *
 * Conventions: every function returns 0 on success and a negative code on
 * failure; ca_last_error() gives the message (thread local).  All buffers are
 * caller-owned host memory, C-contiguous float32, laid out exactly as the
 * reference lays them out (main.pyx:132-134, 194-198).  No pointer is retained
 * across calls.  One ca_trainer drives one GPU; it is not thread safe (the
 * reference is called with the GIL held).
 */
#ifndef CORINTHO_HIP_H
#define CORINTHO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CA_GAME_STATE_SIZE 70 /* util.h:42 kGameStateSize */
#define CA_NUM_MOVES 96       /* util.h:44 kNumMoves */
#define CA_NUM_SYMMETRIES 8   /* util.h:48 kNumSymmetries */

#define CA_OK 0
#define CA_ERR_ARG -1
#define CA_ERR_DEVICE -2   /* HIP failure, no GPU, extension built for another arch */
#define CA_ERR_ENGINE -3   /* a game reported an engine error (arena full, ...) */
#define CA_ERR_STATE -4    /* call made in the wrong state */
#define CA_ERR_IO -5
#define CA_ERR_CALLBACK -6 /* a caller-supplied network function returned non-zero */
#define CA_ERR_INTERNAL -7 /* a device pass found a state that cannot be (ca_fitter_merge_duplicates) */

typedef struct ca_trainer ca_trainer;

/* Trainer::Trainer arguments (trainer.h:22-25) followed by device options that
 * have no reference counterpart.  Zero-initialise, then fill. */
typedef struct ca_config {
  /* reference ctor arguments, same meaning and defaults as trainer.h:22-25 */
  int32_t num_games;
  int32_t seed;
  int32_t max_searches;       /* default 1600 */
  int32_t searches_per_eval;  /* default 16 */
  float c_puct;               /* default 1.0 */
  float epsilon;              /* default 0.25 */
  int32_t num_logged;         /* must be 0 here: the per-game text logs are switched on by ca_trainer_set_logging */
  int32_t num_threads;        /* accepted and ignored (OpenMP width of the reference) */
  int32_t testing;            /* arena mode: no samples, no opening temperature */
  /* device options */
  int32_t device;             /* HIP device ordinal */
  int32_t no_stagger;         /* 1: start every game at iteration 0 (trainer.cpp:184-186 is a
                                 memory heuristic; per-game results do not depend on it) */
  uint32_t arena_units;       /* 16-byte units per search tree; 0 = default from max_searches */
  int32_t trace;              /* keep a per-ply trace for the parity tests */
  /* sharding (multi-GPU): this trainer owns games [game_base, game_base+num_games) of a
   * generation of total_games games; seeds are drawn from the Trainer stream in global
   * order and parity = global index % 2 (trainer.cpp:243-255).  0/0 = unsharded. */
  int32_t game_base;
  int32_t total_games;
  /* fused training: number of independent game pools run on separate HIP streams of the same
   * GPU (one pool's search overlaps another's network kernel); 0 = automatic */
  int32_t pools;
  /* analysis mode (DockerMC, dockermc.h:13-51): every "game" is ONE position to search,
   * given by ca_trainer_set_positions; testing is implied; a slot is finished by its first chooseMove */
  int32_t analyse;
  /* Resident slots (training mode only).  The reference holds the trees of all num_games games and staggers their
   * starts to bound the memory (trainer.cpp:184-186).  Here `resident` slots hold the games in play; a slot whose
   * game ends takes the next game (its generator seeded from the Trainer stream by game index, trainer.cpp:243-255,
   * so no game's result depends on the slot or moment it starts), and the finished game's tree memory is given back
   * whole.  0 = automatic (all games resident when their trees fit in 5/8 of the free device memory, else as many
   * slots as fit); >= num_games or < 0 = all resident.  With fewer slots than games the staggered start is off. */
  int32_t resident;
  /* Evaluation cache of fused training (ca_trainer_run): a request row whose position was evaluated earlier in the same
   * generation receives the stored outputs instead of a second evaluation -- bit for bit what the network kernel would
   * write again, since a row's outputs depend on the row only.  Emptied at the start of every generation (and whenever
   * it is half full).  0 = on, table sized from the pool and the free memory; n > 0 = on with 2^n entries (one table for all pools of the trainer);
   * negative = off.  (The reference evaluates every request, main.pyx:70-83; results are identical either way.) */
  int32_t eval_cache;
  /* Fused training: a game's step (the body of Trainer::doIteration's loop for that game, trainer.cpp:175-196) stops
   * selecting once it has run for this long and goes on in the next iteration; the leaves it has queued are held back until
   * the batch of searches_per_eval is complete (or the move's searches run out), so the game performs exactly the
   * reference's sequence of operations -- only spread over more iterations.  It bounds what a launch waits for: its
   * slowest game (endgame positions under a trained network: simulations ten levels deep, half of them ending in
   * terminal leaves that queue nothing).  0 = automatic (1.5 x the running mean of the pool's steps), n > 0 = n
   * microseconds, -1 = no limit (below -1, diagnostic: automatic with the factor -n / 16).  Results are identical either
   * way; the number of iterations of a generation is not. */
  int32_t step_budget;
} ca_config;

const char *ca_last_error(void);
/* 0 if a usable gfx950 device is visible */
int ca_device_check(int device);

/* Trainer::Trainer (trainer.cpp:18-37) / ~Trainer */
int ca_trainer_create(const ca_config *cfg, ca_trainer **out);
void ca_trainer_destroy(ca_trainer *t);

/* Trainer::initialize, trainer.cpp:243-250: the first num_logged games of the generation write
 * `<log_folder>/game_<i>.txt` (i = game_base + index), the text SelfPlayer prints at every move choice
 * (selfplayer.cpp:124-232; main line node.cpp:197-240).  Call before the first iteration.  The search kernel records
 * the numbers; the files are written when the last game is over (the reference writes as it goes), byte for byte the
 * reference's text.  A file that cannot be opened is skipped silently, as the reference's ofstream is.  Self-play and
 * arena trainers only. */
int ca_trainer_set_logging(ca_trainer *t, const char *log_folder, int32_t num_logged);

/* int Trainer::num_requests(int to_play) -- trainer.cpp:39-49 */
int ca_trainer_num_requests(ca_trainer *t, int to_play, int32_t *out);
/* int Trainer::num_samples() -- trainer.cpp:51-57 */
int ca_trainer_num_samples(ca_trainer *t, int32_t *out);
/* float Trainer::score() -- trainer.cpp:59-68 */
int ca_trainer_score(ca_trainer *t, float *out);
/* float Trainer::avg_mate_length() -- trainer.cpp:70-77 */
int ca_trainer_avg_mate_length(ca_trainer *t, float *out);
/* void Trainer::writeRequests(float *game_states, int to_play) -- trainer.cpp:79-101
 * game_states: [num_requests(to_play)][70] */
int ca_trainer_write_requests(ca_trainer *t, float *game_states, int to_play);
/* void Trainer::writeSamples(float*, float*, float*) -- trainer.cpp:103-113
 * [n*8][70], [n*8], [n*8][96] with n = num_samples() */
int ca_trainer_write_samples(ca_trainer *t, float *game_states, float *eval_samples, float *prob_samples);
/* void Trainer::writeScores(const std::string &file) -- trainer.cpp:115-162 */
int ca_trainer_write_scores(ca_trainer *t, const char *file);
/* bool Trainer::doIteration(float eval[], float probs[], int to_play) -- trainer.cpp:164-236
 * evaluations: [num_requests], probabilities: [num_requests][96] for the rows last
 * written by writeRequests(to_play); ignored on the first call.  *all_done = return value. */
int ca_trainer_do_iteration(ca_trainer *t, const float *evaluations, const float *probabilities, int to_play,
                            int32_t *all_done);

/* Host-driven protocol with the evaluation cache (training mode only).  log2_entries: 0 = table sized
 * automatically (as ca_config.eval_cache = 0 sizes it), 6..30 = 2^n entries, negative = off (the default).
 * Allowed only at a generation boundary: before the first ca_trainer_do_iteration, or after ca_trainer_reset.
 *
 * With it on the three protocol calls above keep their signatures and hand the caller only the request rows whose
 * position has no stored evaluation in this generation (to_play must be -1):
 *   ca_trainer_num_requests   n = the positions to evaluate: the request rows the cache could resolve neither to an
 *                             earlier row of this generation nor to another row of this batch.  n may be 0 while games
 *                             are still running (every row was served from the table): that is not the reference's
 *                             "No requests during training" condition, just call ca_trainer_do_iteration again.
 *   ca_trainer_write_requests writes those n rows, [n][70], densely.  Their ORDER IS UNSPECIFIED: a game reserves its
 *                             rows with an atomic, so it is not the reference's game order and may differ between runs.
 *   ca_trainer_do_iteration   evaluations[n], probabilities[n][96] answer exactly those rows in that order.
 * all_done, num_samples, write_samples, score, write_scores, the game logs and the traces are unchanged.
 * PRECONDITION: the caller's network gives a row the same outputs in whatever batch it stands.  Then every game's
 * results equal the plain protocol's bit for bit; a network that is not batch-invariant gets "evaluated once, reused".
 * The number of iterations of a generation may differ from the plain protocol's.  ca_stats: nn_rows = rows the games
 * requested, nn_rows_evaluated = rows handed to the caller, iterations = ca_trainer_do_iteration calls.
 * CA_ERR_STATE: a testing, analysis or tournament trainer; switching in mid-generation; ca_trainer_run while it is on.
 * CA_ERR_ARG: log2_entries in 1..5 or above 30; to_play other than -1 in the three calls while it is on. */
int ca_trainer_set_host_cache(ca_trainer *t, int32_t log2_entries);

/* Optional, for the reference protocol above: page-lock a caller-owned array (the three arrays the
 * reference's play loop allocates once and passes to every call, main.pyx:132-134) so that the
 * per-iteration copies from / to it are direct DMA at PCIe speed instead of staged copies from
 * pageable memory.  The array must stay allocated until ca_trainer_unpin_host or
 * ca_trainer_destroy.  *pinned = 0 if the runtime refused (the calls still work, slower). */
int ca_trainer_pin_host(ca_trainer *t, void *p, size_t bytes, int32_t *pinned);
int ca_trainer_unpin_host(ca_trainer *t, void *p);

/* ---------------- analysis of N positions (replaces N x `class DockerMC`, dockermc.h:13-51) ----------------
 * A trainer created with ca_config.analyse = 1 searches num_games independent positions, one wavefront
 * each -- what docker/choose_move.pyx does for one position with one DockerMC, batched.  Position i is the
 * DockerMC constructor's (seed, board[64] (bit = cell*4 + {base, column, capital, frozen}), to_play,
 * pieces[6]) (dockermc.cpp:11-19, game.cpp:14-26); max_searches, searches_per_eval, c_puct, epsilon come
 * from ca_config.  Call once, before the first iteration.  Then either protocol applies: the reference's
 * (ca_trainer_do_iteration / num_requests / write_requests with to_play = -1: DockerMC::doIteration /
 * num_requests / writeRequests over all positions at once) or the fused one (ca_trainer_set_net +
 * ca_trainer_run).  A position whose search is over has chosen its move (DockerMC::chooseMove). */
int ca_trainer_set_positions(ca_trainer *t, const int32_t *boards /* [n][64] */, const int32_t *to_play /* [n] */,
                             const int32_t *pieces /* [n][6] */, const int32_t *seeds /* [n] */);
/* out[i] = {move (chooseMove; -1: the given position was already terminal), done (DockerMC::done of the
 * position after the move), drawn (DockerMC::drawn), nodes (num_nodes), evaluation bits (float eval()),
 * legal-move mask of the new position [3] (getLegalMoves)}: what choose_move.pyx:206-221 reads */
int ca_trainer_analysis(ca_trainer *t, int32_t *out /* [n][8] */);
/* DockerMC::chooseMove (dockermc.cpp:48-50) on searches that have NOT ended: docker/choose_move.pyx:110-117 leaves
 * its loop on a time limit as well as on doIteration returning true, and calls chooseMove either way (:199).
 * Every position that has not finished chooses its move on its tree as it stands (TrainMC::chooseMove,
 * trainmc.cpp:110-137; evaluations still pending are not received); afterwards ca_trainer_analysis reports all
 * positions.  Before any iteration, the root is created first (the TrainMC constructor's createRoot). */
int ca_trainer_finish(ca_trainer *t);

/* ---------------- fused mode (no reference counterpart; opt-in) ----------------
 * The network runs on the device, so the play loop of main.pyx:123-187 never
 * leaves the GPU.  Weights are a flat float32 buffer in the layout documented in
 * corintho_ai_amd/nets.py for each kind. */
#define CA_NET_MLP12X100 1 /* the reference architecture, wrapper.py:256-271 */
#define CA_NET_RESCNN4 2   /* the north-star 4-block residual CNN, fp32 MFMA */
#define CA_NET_RESCNN4_X3 3 /* the same network and weights; 3x3 convolutions at bf16x3 split precision
                              (bf16 MFMA, fp32 accumulate; within 2e-5 of the fp32 result) */
#define CA_NET_MLP12X100_X3 4 /* the reference architecture and weights; dense layers at bf16x3 split precision */
/* float32-equivalent arithmetic on the bf16 matrix pipe ("bf16x6"): both operands of every matrix product as
 * THREE bf16 terms whose sum is the float32 value, the six products down to 2^-16 of the leading one kept (the
 * dropped ones are below one float32 rounding of the product), fp32 accumulation.  Error against a float64
 * evaluation = that of the fp32-MFMA kinds 1 and 2 (tests/test_net_precision.py). */
#define CA_NET_RESCNN4_X6 5
#define CA_NET_MLP12X100_X6 6
/* "f16x3": both operands of every matrix product as TWO fp16 terms, x = fp16(x) + fp16(x - fp16(x)) -- 22 significand
 * bits each -- and the three products w0 x0 + w0 x1 + w1 x0 on the fp16 matrix pipe, fp32 accumulation: the dropped
 * terms are 2^-22 of a product.  Float32-class results at half the matrix work of bf16x6; error against float64
 * measured beside the other kinds in tests/test_net_precision.py. */
#define CA_NET_RESCNN4_H3 8
#define CA_NET_MLP12X100_H3 9
/* slot 0 = best model (training, and arena `to_play == 1`), slot 1 = new model (arena
 * `to_play == 0`), as get_predictions chooses them (main.pyx:70-83) */
int ca_trainer_set_net(ca_trainer *t, int slot, int kind, const float *weights, size_t n_floats);
/* ---- the caller's own network in fused mode ----
 * rows a network of this trainer must be able to take: resident slots x searches_per_eval */
int ca_trainer_request_rows(ca_trainer *t, int32_t *rows);
/* The caller's network as slot `slot` of fused mode.  The three DEVICE buffers are the caller's, on the trainer's device,
 * of max_rows rows (>= ca_trainer_request_rows), and stay allocated until the slot is replaced or the trainer destroyed:
 *   d_states [max_rows][70]   written by the library: request rows, the reference's layout (writeRequests)
 *   d_evals  [max_rows]       written by fn
 *   d_probs  [max_rows][96]   written by fn
 * fn(user, row0, cap_rows, d_rows, stream): rows [row0, row0 + cap_rows) of d_states are ready on `stream` (a
 * hipStream_t); the first *d_rows of them (a device int32, <= cap_rows; the host does not know it) are positions, the
 * rest are zero.  fn enqueues, on `stream` or ordered against it, work that leaves the answers in the same rows of
 * d_evals / d_probs, and returns 0; it need not synchronise.  Answers to rows beyond *d_rows are ignored.
 *
 * The caller evaluates cap_rows rows, not *d_rows: that is the price of never asking the host.  A fused training run
 * shrinks cap_rows to (games still running) x searches_per_eval as a pool thins out.  The arena queues both models in
 * every iteration and the idle one finds a count of 0: its function is asked for cap_rows zero rows.
 *
 * The contract of fn:
 *   - It is called on the thread that called ca_trainer_run / ca_trainer_net_forward / ca_tourney_run, never
 *     concurrently and never after that call has returned.
 *   - It must not call an entry point on the same trainer (tourney): that call returns CA_ERR_STATE.
 *   - Fused training calls it once per pool and iteration, with that pool's row0.  The pools' row ranges are disjoint,
 *     so work enqueued for one pool may still be running when fn is called for the next.  The arena, tournaments,
 *     ca_trainer_net_forward and ca_trainer_net_bench call it with row0 = 0.
 *   - PRECONDITION of the evaluation cache (ca_config.eval_cache), as for ca_trainer_set_host_cache: the caller's network
 *     gives a row the same outputs in whatever batch it stands.  Then every game's results equal the built-in path's bit
 *     for bit; a network that is not batch-invariant gets "evaluated once, reused".
 *   - flop_per_row is what the automatic rule of ca_config.eval_cache = 0 reads (a cache from 1e6 on): 0 = unknown, then
 *     no automatic cache; ca_config.eval_cache > 0 still forces one.
 * A non-zero return of fn ends the run: nothing more is queued, every stream is drained as on any other exit, and the
 * call returns CA_ERR_CALLBACK with the slot (model id) in ca_last_error().  The generation is unusable until
 * ca_trainer_reset: ca_trainer_run, ca_trainer_do_iteration and ca_trainer_net_forward return CA_ERR_STATE and say so (a
 * tournament has no reset: ca_tourney_run keeps returning CA_ERR_STATE).
 * CA_ERR_ARG: a slot other than 0 / 1, a null function or buffer, max_rows below ca_trainer_request_rows.  CA_ERR_STATE:
 * a replacement that would turn the evaluation cache on or off in mid-generation, as ca_trainer_set_net. */
typedef int (*ca_net_fn)(void *user, int32_t row0, int32_t cap_rows, const int32_t *d_rows, void *stream);
int ca_trainer_set_net_fn(ca_trainer *t, int slot, ca_net_fn fn, void *user, float *d_states, float *d_evals,
                          float *d_probs, int32_t max_rows, double flop_per_row);
/* Run the whole generation on the device.  max_iterations 0 = until done. */
int ca_trainer_run(ca_trainer *t, int64_t max_iterations, int32_t *all_done);
/* One network evaluation of host rows through the device kernels (numerics tests):
 * states [n][70] -> evals [n], probs [n][96] */
int ca_trainer_net_forward(ca_trainer *t, int slot, const float *states, int32_t n, float *evals, float *probs);

/* Kernel-only time of one network evaluation of `rows` resident rows (average of `reps`
 * launches, HIP events) -- diagnostics */
int ca_trainer_net_bench(ca_trainer *t, int slot, const float *states, int32_t rows, int32_t reps, float *ms_per_call);

/* Un-augmented samples for the multi-GPU gather: n = num_samples() rows of
 * (state[70], policy[96]) + outcome[n] in game order; the x8 symmetry expansion
 * is applied after the gather by ca_expand_samples. */
int ca_trainer_export_samples(ca_trainer *t, float *state_policy /* [n][166] */, float *outcome /* [n] */);
/* The same rows packed on the device into caller-owned DEVICE buffers
 * ([cap_rows][166] and [cap_rows] float32), ready for an RCCL all-gather. */
int ca_trainer_pack_samples_device(ca_trainer *t, void *d_state_policy, void *d_outcome, int32_t cap_rows,
                                   int32_t *n_rows);
/* Start a new generation in the same pool: Trainer::initialize (trainer.cpp:238-256)
 * with a new seed, without reallocating the device buffers. */
int ca_trainer_reset(ca_trainer *t, int32_t seed);
/* the HIP device ordinal the trainer was created on (ca_config.device) */
int ca_trainer_device(ca_trainer *t, int32_t *device);
int ca_expand_samples(int device, const float *state_policy, const float *outcome, int32_t n, float *game_states,
                      float *eval_samples, float *prob_samples);

/* ---------------- introspection (tests, bench) ---------------- */
typedef struct ca_stats {
  int64_t searches;      /* simulations run */
  int64_t evals;         /* leaf evaluations consumed */
  int64_t nodes;         /* nodes created */
  int64_t plies;
  int64_t iterations;    /* doIteration calls / fused steps */
  int64_t peak_arena_units; /* high-water mark over all trees */
  double mcts_ms, nn_ms, pack_ms; /* device time by kernel family (fused mode, HIP events) */
  int64_t mcts_launches, nn_launches;
  int64_t nn_rows;       /* rows evaluated by the network kernels */
  int64_t pools;         /* pools the last ca_trainer_run used (1 in arena mode) */
  /* fused training times one iteration per pool and polling window of 16 (CO_POOL_POLL), the arena one
   * iteration in 8, with HIP events (mcts_ms / nn_ms
   * above are then estimates: timed sums scaled by launches / timed launches); exact figures of
   * the timed launches: */
  int64_t timed_launches; /* search + network launch pairs that carried events */
  int64_t nn_timed_rows;  /* batch rows of those network launches */
  double mcts_timed_ms, nn_timed_ms;
  int64_t resident_slots; /* slots of the pool (= num_games unless it recycles, ca_config.resident) */
  int64_t nn_rows_evaluated; /* rows the network kernels worked on; nn_rows - this = rows served by the evaluation cache */
  int64_t steps_cut;         /* ca_config.step_budget: game steps of the generation (since ca_trainer_reset, over every ca_trainer_run) that stopped at their budget and went on in the next iteration */
  int64_t step_budget_last;  /* the budget (microseconds) the first pool's last launch worked under; 0 = none */
  int64_t tourney_path;      /* ca_tourney_stats: the path the last ca_tourney_run took -- 0 none yet, 1 one iteration per model id, 2 grouped (ca_tourney_set_grouped) */
} ca_stats;
int ca_trainer_stats(ca_trainer *t, ca_stats *out);
/* per-game: {to_play, done, result, n_samples, n_pending, error, mate_turn, plies} */
int ca_trainer_game_info(ca_trainer *t, int game, int32_t out[8]);
/* per-ply trace of one game, same record format as the oracle's; returns words via *n */
int ca_trainer_trace(ca_trainer *t, int game, int32_t *out, int32_t cap, int32_t *n);
/* diagnostic builds of the library (-DCO_PROF) only: summed in-kernel cycle stamps of the search kernel
 * (slots documented in csrc/search_state.h); the shipped build returns CA_ERR_STATE */
int ca_trainer_prof(ca_trainer *t, unsigned long long out[88]);

/* ---- Tourney: replaces `class Tourney` of corintho_ai/cpp/include/tourney.h:13-46
 * consumed by corintho_ai/rating/tourney.pyx:15-31.  One match = one slot of a device pool
 * (two search trees, one wavefront); the pool is built at the first query after the last
 * ca_tourney_add_match.  Model ids are the caller's (negative = the dummy ids of random
 * players, tourney.pyx:131-134). ---- */
typedef struct ca_tourney ca_tourney;
/* Tourney(num_threads, log_folder), tourney.h:15 (threads have no device meaning; the folder: ca_tourney_set_log_folder) */
int ca_tourney_create(int device, uint32_t arena_units, int trace, ca_tourney **out);
/* Tourney::log_folder_ (tourney.h:46): where the matches added with logging = true write
 * `match_<player1>_<player2>_<index>.txt` (tourney.cpp:90-95; the text of match.cpp:78-190).  Before the first query.
 * The files are written when the last match is over (the reference writes them as the matches go); one that cannot
 * be opened is skipped silently, as the reference's ofstream is. */
int ca_tourney_set_log_folder(ca_tourney *t, const char *log_folder);
void ca_tourney_destroy(ca_tourney *t);
/* Tourney::addPlayer, tourney.cpp:72-78 */
int ca_tourney_add_player(ca_tourney *t, int32_t player_id, int32_t model_id, int32_t max_searches,
                          int32_t searches_per_eval, float c_puct, float epsilon, int32_t random);
/* Tourney::addMatch, tourney.cpp:80-96: the match's generator is seeded with the next output of
 * the tourney's default-constructed std::mt19937; `logging`: the match writes its text log (ca_tourney_set_log_folder) */
int ca_tourney_add_match(ca_tourney *t, int32_t player1, int32_t player2, int32_t logging);
/* Tourney::all_done, tourney.cpp:14-21 */
int ca_tourney_all_done(ca_tourney *t, int32_t *out);
/* Tourney::num_requests(id), tourney.cpp:23-31 */
int ca_tourney_num_requests(ca_tourney *t, int32_t id, int32_t *out);
/* Tourney::writeRequests(game_states, id), tourney.cpp:43-51: [num_requests(id)][70] */
int ca_tourney_write_requests(ca_tourney *t, float *game_states, int32_t id);
/* Tourney::doIteration(eval, probs, id), tourney.cpp:53-70.  `rows` = rows of the two caller
 * arrays (eval[rows], probs[rows][96]): matches read them through the reference's own offset
 * table (tourney.cpp:55-62), which can differ from the writeRequests order */
int ca_tourney_do_iteration(ca_tourney *t, const float *evaluations, const float *probabilities, int32_t rows,
                            int32_t id);
/* Fused mode (not in the reference): the networks run on the GPU too.  ca_tourney_set_net
 * gives model `model_id` its network (kinds and weight layouts as ca_trainer_set_net);
 * ca_tourney_run plays the loop of rating/tourney.pyx:122-160 on the device, model ids in
 * ascending order, until every match is done or `max_rounds` rounds have run (0 = no limit).
 * The network is built when ca_tourney_run first needs it, and what is wrong with it is reported
 * there as ca_trainer_set_net reports it: CA_ERR_ARG for an unknown kind, a bad weight count or
 * f16x3 weights beyond fp16's range. */
int ca_tourney_set_net(ca_tourney *t, int32_t model_id, int32_t kind, const float *weights, size_t n_floats);
/* the caller's own network for model `model_id` (see ca_trainer_set_net_fn); max_rows is checked against matches x the
 * largest searches_per_eval when the tournament is built (CA_ERR_ARG from ca_tourney_run) */
int ca_tourney_set_net_fn(ca_tourney *t, int32_t model_id, ca_net_fn fn, void *user, float *d_states, float *d_evals,
                          float *d_probs, int32_t max_rows, double flop_per_row);
int ca_tourney_run(ca_tourney *t, int64_t max_rounds, int32_t *all_done);
/* Diagnostic (not in the reference): 1 = every match reads its evaluations at the rows Tourney::writeRequests
 * gave it, instead of through Tourney::doIteration's own offset table (tourney.cpp:55-62, SURVEY 8a quirk 10,
 * which hands most matches the rows of OTHER matches).  Before the first query; default 0 = the reference's table. */
int ca_tourney_set_exact_offsets(ca_tourney *t, int32_t on);
/* Not in the reference: 1 = ca_tourney_run serves EVERY model in one round -- one scan, one compaction, one grouped network
 * launch (every workgroup takes the weights of its own model) and one search launch that steps every match, whatever the
 * number of models; ca_stats.nn_launches and mcts_launches then grow by 1 per round.  It turns exact offsets on (a match
 * must read its own rows for its play not to depend on the order of the steps); a later ca_tourney_set_exact_offsets(0)
 * is CA_ERR_STATE.  Before the first query, else CA_ERR_STATE.  ca_tourney_run then refuses a model that is a caller's
 * function (CA_ERR_STATE); if the models are not all of one kind, or there are more than 256 of them or more than 65535
 * request rows (matches x the largest searches_per_eval), it takes the per-model path, and ca_stats.tourney_path says
 * which one ran. */
int ca_tourney_set_grouped(ca_tourney *t, int32_t on);
/* Not in the reference, whose Tourney draws every match's seed from a default-constructed std::mt19937 (tourney.h:43):
 * that generator seeded with `seed` instead, so that the parts of a rating round play different games.  Before the first
 * addMatch, else CA_ERR_STATE. */
int ca_tourney_set_seed(ca_tourney *t, uint32_t seed);
/* Tourney::writeScores, tourney.cpp:33-41 */
int ca_tourney_write_scores(ca_tourney *t, const char *filename);
int ca_tourney_num_matches(ca_tourney *t, int32_t *out);
/* out[8] = {player id 1, player id 2, done, result for the first player, side to move, pending requests, plies, error} */
int ca_tourney_match_info(ca_tourney *t, int32_t match, int32_t out[8]);
/* Match::score, match.cpp:52-58 */
int ca_tourney_match_score(ca_tourney *t, int32_t match, float *out);
int ca_tourney_trace(ca_tourney *t, int32_t match, int32_t *out, int32_t cap, int32_t *n);
int ca_tourney_stats(ca_tourney *t, ca_stats *out);

/* ---- The library's own network kernels on device memory, without a trainer (what ca_trainer_net_forward does after its
 * upload): d_states [rows_cap][70], *d_rows valid rows (a device int32), -> d_evals [rows_cap], d_probs [rows_cap][96]; rows
 * from *d_rows on are left untouched.  Queued on `stream` (a hipStream_t; NULL: the net's own stream, synchronised before
 * the call returns, and an f16x3 kind's range flag checked: CA_ERR_ENGINE).  Kinds and weight layouts as
 * ca_trainer_set_net; rows_cap <= max_rows.  A net holds one staging buffer: a call on another stream than the previous
 * one starts behind the previous call's kernels.  This is what a ca_net_fn calls to run one of the library's networks. */
typedef struct ca_net ca_net;
int ca_net_create(int device, int kind, const float *weights, size_t n_floats, int32_t max_rows, ca_net **out);
int ca_net_forward_device(ca_net *n, const float *d_states, int32_t rows_cap, const int32_t *d_rows, float *d_evals,
                          float *d_probs, void *stream);
/* The same launch with the indirection a fused run gives it: row r < *d_rows of the launch is read from row d_in_idx[r] of
 * d_states [state_rows][70] (NULL: row r; state_rows >= rows_cap then) and its outputs go to element d_out_idx[r] (NULL: r)
 * of d_evals, eval_stride floats per element, and of d_probs, probs_stride floats per element; nothing else is written.
 * The two output pointers may name one array (the evaluation cache's: strides 100, d_probs = d_evals + 4).  alone: 0 = other
 * streams keep the GPU busy too, the kernels may choose for throughput (1: what ca_net_forward_device passes).
 * CA_ERR_ARG: state_rows or rows_cap beyond max_rows, eval_stride < 1, probs_stride < 96, a null d_states, d_rows, d_evals
 * or d_probs.  THE INDICES ARE NOT CHECKED -- they live on the device and the kernels read them: every entry below *d_rows
 * must be below state_rows (d_in_idx) or inside the caller's output arrays (d_out_idx), without repeats in d_out_idx;
 * entries from *d_rows on are never read.  Stream, staging buffer and range flag as ca_net_forward_device. */
int ca_net_forward_device_io(ca_net *n, const float *d_states, int32_t state_rows, int32_t rows_cap, const int32_t *d_rows,
                             const int32_t *d_in_idx, const int32_t *d_out_idx, float *d_evals, int32_t eval_stride,
                             float *d_probs, int32_t probs_stride, int32_t alone, void *stream);
void ca_net_destroy(ca_net *n);

/* ---- Many models of one kind on one set of rows, in one launch: `models` (1..256) weight sets of `kind`, n_floats each
 * (layouts as ca_trainer_set_net).  ca_net_group_forward: states [n][70] on the host, model_of_row[n] in 0 .. models - 1
 * -> evals [n], probs [n][96]; row r is evaluated by model model_of_row[r], to the same bits as by that model alone.  The
 * split-precision kinds of mlp12x100 and rescnn4 at f16x3 run ONE kernel whose workgroups each take their own model's
 * weights; every other kind one launch per model on the same index lists.  An f16x3 weight set beyond fp16's range is refused at creation with the
 * model's index (CA_ERR_ARG); an activation beyond it is CA_ERR_ENGINE from the forward, naming the launch's models.
 * n <= max_rows <= 65535. */
typedef struct ca_net_group ca_net_group;
int ca_net_group_create(int device, int kind, const float *const *weights, int32_t models, size_t n_floats, int32_t max_rows,
                        ca_net_group **out);
int ca_net_group_forward(ca_net_group *g, const float *states, const int32_t *model_of_row, int32_t n, float *evals, float *probs);
/* out[6] = {models, max_rows, 1 if one grouped kernel serves the group, rows per workgroup of the tables, entries of the
 * index list, entries of the workgroup table} */
int ca_net_group_info(ca_net_group *g, int32_t out[6]);
/* diagnostic: the tables the last forward left on the device -- the index list (rows by model, then by row; model m's
 * segment at seg_start[m], seg_count[m] rows), the workgroup table [entries][4] = {model, first index, rows, 0} and the
 * number of its entries in use */
int ca_net_group_tables(ca_net_group *g, int32_t *idx, int32_t *wg, int32_t *n_wg, int32_t *seg_start, int32_t *seg_count);
/* diagnostic: kernel-only times (HIP events) of `reps` launches on these rows, milliseconds per call: out_ms[0] the
 * grouping kernel, out_ms[1] the network launch (or the per-model launches of a kind without a grouped kernel) */
int ca_net_group_bench(ca_net_group *g, const float *states, const int32_t *model_of_row, int32_t n, int32_t reps, float out_ms[2]);
void ca_net_group_destroy(ca_net_group *g);

/* rule layer on a batch of positions (one wavefront each): legal-move masks + is_lines */
int ca_rules_legal_moves(int device, const uint64_t *boards, const uint32_t *metas, int32_t n, uint32_t *masks /* [n][3] */,
                         int32_t *is_lines);
/* apply moves[i] (or -1 for none) and expand the 70-float state */
int ca_rules_do_move(int device, uint64_t *boards, uint32_t *metas, const int32_t *moves, int32_t n,
                     float *states /* [n][70] */);
/* the same two through the search's four-positions-per-wavefront rule layer (csrc/rules.h co_do_move_lane,
 * co_legal_moves_rows): apply moves[i] (or -1 for none), then the legal-move mask of the new position */
int ca_rules_rows(int device, uint64_t *boards, uint32_t *metas, const int32_t *moves, int32_t n, uint32_t *masks /* [n][3] */);
/* std::mt19937 through the device draw path: n outputs for `seed`, drawn `chunk` at a time */
int ca_rng_draw(int device, uint32_t seed, int32_t n, int32_t chunk, uint32_t *out);
/* floating-point contract probe, see kernels.h co_k_fp_probe: in [n][8] -> out [n][8] */
int ca_fp_probe(int device, const float *in, int32_t n, float *out);


/* ---- network training (not in the reference, whose generation step calls Keras model.fit, main.pyx:221-272) ----
 * A ca_fitter fits mlp12x100 (CO_NET_MLP12X100's weights) on the device the way the reference's compiled Keras model
 * does: Adam, MSE on the value head plus 0.25 x categorical cross-entropy on the policy head, BatchNormalization in
 * training mode (batch mean and biased variance; moving statistics with momentum 0.99).  Weights, and Adam's m and v,
 * are in the flat Keras get_weights() layout of ca_trainer_set_net (m and v are 0 at the moving statistics).  Losses:
 * out_losses[3] = {value + 0.25 policy, value (MSE), policy (cross-entropy)}, means over the rows. */
typedef struct ca_fitter ca_fitter;
/* max_batch: the largest batch of ca_fitter_train / _evaluate / _gradients */
int ca_fitter_create(int device, int32_t max_batch, ca_fitter **out);
/* the same for `net` = CA_NET_MLP12X100 (what ca_fitter_create makes) or CA_NET_RESCNN4: the residual CNN in the flat
 * layout of ca_trainer_set_net, by the same recipe -- every convolution's and both head convolutions' BatchNorm takes
 * its statistics per channel over the batch's B x 16 (row, pixel) pairs.  Any other net: CA_ERR_ARG.  Every entry
 * point below serves both; n_floats is checked against the fitter's own weight count. */
int ca_fitter_create_net(int device, int32_t net, int32_t max_batch, ca_fitter **out);
void ca_fitter_destroy(ca_fitter *f);
int ca_fitter_set_weights(ca_fitter *f, const float *weights, size_t n_floats);
int ca_fitter_get_weights(ca_fitter *f, float *weights, size_t n_floats);
/* Adam's slots and step count (Keras optimizer.iterations); a new fitter starts from zeros */
int ca_fitter_set_optimizer(ca_fitter *f, const float *m, const float *v, size_t n_floats, int64_t iterations);
int ca_fitter_get_optimizer(ca_fitter *f, float *m, float *v, size_t n_floats, int64_t *iterations);
/* the sample set, as samples_io.samples_for_training returns it; copied to the device.  It replaces whatever set the
 * fitter held, a packed one included (below), with an expanded one. */
int ca_fitter_set_data(ca_fitter *f, const float *states /* [n][70] */, const float *evals /* [n] */,
                       const float *probs /* [n][96] */, int32_t n);
/* one epoch: batches of `batch` rows taken in the order of rows[] (the last one partial), one Adam step each at
 * learning rate `learning_rate`.  out_losses: means of the batch losses (each before its step) weighted by batch size;
 * batch_losses (may be null): [ceil(n_rows / batch)][3] */
int ca_fitter_train(ca_fitter *f, const int32_t *rows, int32_t n_rows, int32_t batch, float learning_rate,
                    double *out_losses, float *batch_losses);
/* inference mode (moving statistics) on rows [row0, row0 + n_rows), in batches of `batch` */
int ca_fitter_evaluate(ca_fitter *f, int32_t row0, int32_t n_rows, int32_t batch, double *out_losses);
/* the gradient of one batch's loss with respect to every weight (0 at the moving statistics); nothing is updated */
int ca_fitter_gradients(ca_fitter *f, const int32_t *rows, int32_t n_rows, float *grads, double *out_losses);

/* ---- the packed data set: un-augmented samples that stay on the device ----
 * A fitter's data set has one of two forms.  Expanded (ca_fitter_set_data): the 8 symmetry copies of every sample, as
 * Trainer::writeSamples lays them out, 5 344 bytes per sample.  Packed (the calls below): state_policy[n][166] and
 * outcome[n], the rows of ca_trainer_export_samples / ca_trainer_pack_samples_device, 668 bytes per sample.  A packed
 * set of n samples presents 8 n VIRTUAL rows: row v is sample v / 8 under symmetry v % 8, the row order of
 * ca_trainer_write_samples and ca_expand_samples.  ca_fitter_train, _evaluate and _gradients take virtual rows then;
 * the symmetry is applied while a batch is fetched, and every step is the same to the bit as on the expanded set. */
/* empties the data set, whichever form it has; the next ca_fitter_add_* makes it packed */
int ca_fitter_clear_data(ca_fitter *f);
/* appends n packed rows from the host.  On an expanded set: CA_ERR_STATE; more than INT32_MAX virtual rows: CA_ERR_ARG.
 * The capacity grows geometrically and the rows already there move device to device. */
int ca_fitter_add_samples(ca_fitter *f, const float *state_policy /* [n][166] */, const float *outcome /* [n] */, int32_t n);
/* the same from device memory of the fitter's device (the buffers of an RCCL gather, dist.SampleGather(on_device=True));
 * whatever produced them must have finished.  Copied device to device before the call returns. */
int ca_fitter_add_device_samples(ca_fitter *f, const void *d_state_policy, const void *d_outcome, int32_t n);
/* appends the samples of a finished training-mode trainer on the fitter's device, packed by the trainer
 * (ca_trainer_pack_samples_device) straight into the fitter's buffers; *n_added = ca_trainer_num_samples.  A
 * testing-mode trainer: that call's error (CA_ERR_STATE); a trainer on another device: CA_ERR_ARG. */
int ca_fitter_add_trainer_samples(ca_fitter *f, ca_trainer *t, int32_t *n_added);
/* removes the n_oldest first samples of a packed set (the replay window slides); the others keep their order and
 * virtual row v becomes v - 8 n_oldest.  More than the set holds: CA_ERR_ARG. */
int ca_fitter_drop_samples(ca_fitter *f, int32_t n_oldest);
/* *rows = the rows ca_fitter_train can address, *samples = the packed samples (0 for an expanded set) */
int ca_fitter_data_info(ca_fitter *f, int32_t *rows, int32_t *samples);
/* Diagnostic: the batch a step on rows[] would read, copied to the host -- states [n_rows][70], evals [n_rows],
 * probs [n_rows][96] -- through the kernel that assembles a packed set's batches (for an expanded set, the same
 * kernel's plain row copy).  n_rows is not bound by max_batch. */
int ca_fitter_fetch_rows(ca_fitter *f, const int32_t *rows, int32_t n_rows, float *states, float *evals, float *probs);

/* ---- sample weights (Keras's model.fit(sample_weight=...), reduction SUM_OVER_BATCH_SIZE) ----
 * A data set may carry one float32 weight per row (expanded) or per un-augmented sample (packed: virtual row v has the
 * weight of sample v / 8).  A batch of B rows then has the value loss (1/B) sum_r w_r (tanh v_r - z_r)^2 and the policy
 * loss (1/B) sum_r w_r CE_r -- the divisor is B, not sum w -- and ca_fitter_train, _evaluate and _gradients report and
 * differentiate these.  BatchNorm statistics stay unweighted: a row of weight 0 still counts in them.  A set whose
 * weights were never set runs the unweighted kernels, bit for bit what it ran before weights existed.  The weights move
 * with their samples in ca_fitter_drop_samples; ca_fitter_add_* on a set that carries weights: CA_ERR_STATE
 * (ca_fitter_clear_data first).  ca_fitter_set_data and ca_fitter_clear_data remove them. */
/* n must be the set's rows (expanded) or samples (packed), every weight finite and >= 0: else CA_ERR_ARG and nothing
 * changes.  weights == NULL removes the weights (n is not looked at).  No data: CA_ERR_STATE. */
int ca_fitter_set_sample_weights(ca_fitter *f, const float *weights, int32_t n);
/* reads them back; an unweighted set gives 1.0 for every row or sample */
int ca_fitter_get_sample_weights(ca_fitter *f, float *out, int32_t n);
/* Merges the duplicate positions of a packed set on the device.  Two samples are equal when their 70 state floats have
 * the same bit patterns.  A group of equal samples is replaced by one sample at the rank of its first member (groups keep
 * the order of their first members).  With w_i the members' weights (1 on an unweighted set) and the sums taken in
 * float64 over the members in ascending sample index:
 *     W = sum w_i,  policy[m] = (sum w_i p_i[m]) / W,  outcome = (sum w_i z_i) / W,  each rounded once to float32,
 * and the new weight is W.  A group with W = 0 (every member of weight 0) is dropped, members and all.  normalize != 0:
 * every new weight is then W * (after / sum W), in float64 (the groups' W summed in order), rounded once: the weights
 * have mean one, so a weighted fit keeps the loss scale of an unweighted one.  *before and *after: the samples before and
 * after.  The set carries weights from here on.  An expanded or an empty set: CA_ERR_STATE.  CA_ERR_INTERNAL: a device
 * pass reported an impossible state (its probe loops are bounded); the set is unchanged. */
int ca_fitter_merge_duplicates(ca_fitter *f, int normalize, int32_t *before, int32_t *after);

/* ---- the augmentation of a packed set, and its canonical orientation ("Canonical orientation") ----
 * SS = the space table and MS = the move table of the reference (space_symmetries, move_symmetries).  The reference
 * pairs SS[k] with MS[k] (selfplayer.cpp:95-108), but MS[2] is the move permutation of the quarter-turn SS[6] performs
 * and MS[6] that of SS[2]: the two tables do not belong together for k = 2 and 6.  MC is MS with rows 2 and 6 exchanged,
 * MC[k] = MS[(k & 3) == 2 ? k ^ 4 : k]; with it (state through SS[k], policy through MC[k]) is one action of the eight
 * symmetries on a sample.
 *   CA_AUG_REFERENCE   virtual row 8 i + k of a packed set: policy through MS[k], as the reference expands (the default)
 *   CA_AUG_CONSISTENT  the policy through MC[k]; state and outcome as before
 * A property of the fitter, not of the set: it stays until set again, through ca_fitter_clear_data too, and never touches
 * an expanded set (ca_fitter_set_data), whose rows are the caller's.  Any other value: CA_ERR_ARG, nothing changes. */
#define CA_AUG_REFERENCE 0
#define CA_AUG_CONSISTENT 1
int ca_fitter_set_augmentation(ca_fitter *f, int32_t augmentation);
int ca_fitter_get_augmentation(ca_fitter *f, int32_t *augmentation);
/* Brings every sample of a packed set into its canonical orientation, in place on the device.  Of a sample (s, p) the
 * eight candidates are s_k[c] = s[SS[k][c >> 2] * 4 + (c & 3)] for c < 64 (cells 64..69 do not move); k* is the k whose
 * candidate is smallest when words 0..63 are compared in ascending order as unsigned 32-bit patterns, the lowest k on a
 * tie; the sample becomes (s_k*, p[MC[k*]]).  The policy moves through MC whatever the augmentation is: MC is the only
 * pairing that is a group action.  Outcomes and weights are untouched, and the set does not become a weighted one.
 * *moved: how many samples had k* != 0.  Samples that are images of one another have equal states afterwards, so
 * ca_fitter_merge_duplicates then merges up to symmetry.  An expanded or an empty set: CA_ERR_STATE. */
int ca_fitter_canonicalize(ca_fitter *f, int32_t *moved);

/* ---- fit options: the L1L2 regulariser, decoupled weight decay and gradient clipping, on the device ----
 * What the reference's model declares and leaves at zero (kernel_regularizer=regularizers.L1L2() on its twelve hidden
 * Dense layers, wrapper.py:263) and what its optimizer's constructor takes (Adam(weight_decay=, clipnorm=,
 * global_clipnorm=, clipvalue=), wrapper.py:273).  This comment is the definition.
 *
 * A network's flat weight vector is a sequence of TENSORS, contiguous ranges (ca_fitter_tensor_table; in Python
 * nets.tensor_table): the pieces of the MLP's layers, the entries of nets._rescnn4_shapes().  A tensor has a class:
 *   CA_TENSOR_TRUNK_KERNEL  mlp12x100: the 12 hidden Dense kernels;  rescnn4: stem_k and b{0..3}_c{1,2}_k
 *   CA_TENSOR_HEAD_KERNEL   mlp12x100: Kv and Kp;                    rescnn4: p_k, p_dk, v_k, v_d1k, v_d2k
 *   CA_TENSOR_BIAS, CA_TENSOR_GAMMA, CA_TENSOR_BETA, CA_TENSOR_MOVING (a moving mean or variance: not trainable)
 *
 * One step at learning rate lr.  w: the weights before the step; g: the summed data gradient, the very floats
 * ca_fitter_gradients returns (which keeps its meaning whatever the options: the gradient of the data loss).
 *   1. regulariser   on the regularised tensors (regularize = 0: the trunk kernels, where the reference puts its
 *                    regulariser; 1: all kernels) r_i = l1 sgn(w_i) + (2 l2) w_i, sgn(+-0) = 0; elsewhere r_i = 0.
 *                    g' = g + r, evaluated in float64 and rounded once to float32 (so nothing is lost where g and r
 *                    cancel); l1 and l2 themselves are float32 values.
 *   2. clipping      of g' on the trainable tensors, by at most one of
 *                      clipvalue c        g'' = min(max(g', -c), c)
 *                      clipnorm c         per tensor T: n_T = sqrt(sum g'_i^2), g'' = g' s_T, s_T = float32(c / max(n_T, c))
 *                      global_clipnorm c  the same with one norm over all trainable tensors
 *                    An unclipped tensor has s = 1.0f exactly: its bits do not change.  A norm that is not finite is
 *                    not treated specially.
 *   3. decay         decoupled (Keras Adam(weight_decay=), biases, gamma and beta excluded): on every kernel, trunk and
 *                    head, w' = w - (lr weight_decay) w -- the multiplier is lr, not Adam's lr_t; elsewhere w' = w.
 *   4. Adam          as defined under "Adam's arguments" below, on g'' from w'; the moving statistics move as without
 *                    options.
 *   5. loss          total = value + 0.25 policy + R(w), R = l1 sum |w_i| + l2 sum w_i^2 over the regularised tensors:
 *                    in ca_fitter_train (out_losses[0]; batch_losses[][0] with the w from before that batch's step) and in
 *                    ca_fitter_evaluate, as Keras adds layer losses to loss and val_loss.  out_losses[1] and [2] do
 *                    not change.
 * The sums of R and of the norms are accumulated in float64 in a fixed order (a tree of fixed shape over fixed pieces
 * of the weight vector) without float atomics: two identical fits stay bitwise identical.  With every option 0 a step
 * launches the kernels it launches without this section and produces the same bytes. */
#define CA_TENSOR_TRUNK_KERNEL 0
#define CA_TENSOR_HEAD_KERNEL 1
#define CA_TENSOR_BIAS 2
#define CA_TENSOR_GAMMA 3
#define CA_TENSOR_BETA 4
#define CA_TENSOR_MOVING 5
typedef struct ca_fit_options {
  uint32_t struct_size; /* sizeof(ca_fit_options) of the caller: the library reads and writes min(struct_size, its own
                           sizeof) bytes and takes the defaults for what the caller's struct does not have */
  int32_t regularize;   /* 0: l1 and l2 on the trunk kernels, 1: on all kernels */
  float l1, l2;
  float weight_decay;
  float clipvalue, clipnorm, global_clipnorm; /* at most one of the three */
} ca_fit_options; /* every option 0: off */
/* what the steps of the last ca_fitter_train did; all 0 when no option is set */
typedef struct ca_fit_stats {
  uint32_t struct_size; /* as above */
  uint32_t reserved;
  int64_t steps;         /* steps of the call */
  int64_t clipped_steps; /* ... in which clipping changed anything */
  double regularization; /* mean over the steps of R(w), w from before each step */
  double grad_norm;      /* mean and ... */
  double grad_norm_max;  /* ... maximum over the steps of the norm of g' over all trainable tensors, before clipping */
} ca_fit_stats;
/* CA_ERR_ARG and nothing changes: a negative or non-finite value, regularize outside 0..1, more than one clip mode, a
 * struct_size below 4.  The options stay, across ca_fitter_set_weights, _set_optimizer and every change of the data,
 * until they are set again. */
int ca_fitter_set_options(ca_fitter *f, const ca_fit_options *options);
/* out->struct_size must be set by the caller; on return it is the number of bytes written */
int ca_fitter_get_options(ca_fitter *f, ca_fit_options *out);
int ca_fitter_train_stats(ca_fitter *f, ca_fit_stats *out);
/* the network's tensors in the order of the weight vector: out[k] = {offset, floats, class} of the first
 * min(cap, *count) of them; *count = how many there are (out may be null with cap 0) */
int ca_fitter_tensor_table(ca_fitter *f, int32_t *out /* [cap][3] */, int32_t cap, int32_t *count);

/* ---- Adam's arguments: beta_1, beta_2, epsilon, AMSGrad and averaged weights, on the device ----
 * What Keras's Adam(beta_1=, beta_2=, epsilon=, amsgrad=, use_ema=, ema_momentum=, ema_overwrite_frequency=) takes.
 * This comment is the definition.
 *
 * One step at learning rate lr for trainable weight i.  g'' and w' are what the fit options' steps 1 to 3 leave; without
 * options they are the summed gradient g of ca_fitter_gradients and w.  Everything is float32, in this operation order,
 * without contraction:
 *     t     = float(iterations + 1)
 *     lr_t  = lr * (sqrtf(1 - powf(beta_2, t)) / (1 - powf(beta_1, t)))      on the host
 *     m'    = m + (g'' - m) * (1.0f - beta_1)
 *     v'    = v + (g''*g'' - v) * (1.0f - beta_2)
 *     d     = amsgrad ? (h' = max(h, v')) : v'                               h: the third slot, "vhat"
 *     w''   = w' - lr_t * m' / (sqrtf(d) + epsilon)
 *     a'    = a + (w'' - a) * (1.0f - ema_momentum)                          only with ema_momentum > 0; a: the average
 *     w'''  = a'   if ema_overwrite_frequency = k > 0 and (iterations + 1) % k == 0, else w''
 * A moving statistic moves as without these arguments, and its entry of a is rewritten with its new value at every step
 * that averages, so the average is always a complete, usable weight vector.  m, v and h are 0 at moving statistics.
 * Step 4 of the fit options ("Adam as without options") is this Adam.
 *
 * State.  h is 0 on a new fitter and after every ca_fitter_set_optimizer.  The average is INVALID on a new fitter and
 * after every ca_fitter_set_weights; the first step with ema_momentum > 0 that finds it invalid first copies the
 * pre-step weights into it; installing one with ca_fitter_set_slot makes it valid.  Neither slot occupies device memory
 * before its first use.  With every argument at its default a step launches the kernels it launches without this
 * section and produces the same bytes. */
typedef struct ca_fit_adam {
  uint32_t struct_size; /* as ca_fit_options': min(struct_size, the library's sizeof) bytes are read and written */
  float beta_1, beta_2; /* in [0, 1); 0 is a legal value, so the defaults are NOT zeros: use CA_FIT_ADAM_INIT */
  float epsilon;        /* finite and > 0 */
  int32_t amsgrad;      /* 0 or not 0 */
  float ema_momentum;   /* in [0, 1); 0: no averaging */
  int32_t ema_overwrite_frequency; /* k >= 0; k > 0 needs ema_momentum > 0 */
} ca_fit_adam;
/* the Adam defaults: what a new fitter has, and what a caller's shorter struct leaves to the library */
#define CA_FIT_ADAM_INIT {sizeof(ca_fit_adam), 0.9f, 0.999f, 1e-7f, 0, 0.0f, 0}
#define CA_SLOT_VHAT 0
#define CA_SLOT_AVERAGE 1
/* CA_ERR_ARG and nothing changes unless, judged in float32: 0 <= beta_1 < 1, 0 <= beta_2 < 1, epsilon finite and > 0,
 * 0 <= ema_momentum < 1, ema_overwrite_frequency >= 0 and > 0 only with ema_momentum > 0 (and struct_size >= 4).  The
 * values stay, as the options do, until they are set again. */
int ca_fitter_set_adam(ca_fitter *f, const ca_fit_adam *adam);
/* out->struct_size must be set by the caller; on return it is the number of bytes written */
int ca_fitter_get_adam(ca_fitter *f, ca_fit_adam *out);
/* which: CA_SLOT_VHAT or CA_SLOT_AVERAGE, n_floats the fitter's weight count: else CA_ERR_ARG and nothing changes.  A
 * vhat that was never used reads as zeros; an invalid average gives CA_ERR_STATE. */
int ca_fitter_set_slot(ca_fitter *f, int32_t which, const float *values, size_t n_floats);
int ca_fitter_get_slot(ca_fitter *f, int32_t which, float *values, size_t n_floats);
/* exchanges w and a, every entry.  CA_ERR_STATE and nothing changes if the average is invalid. */
int ca_fitter_swap_average(ca_fitter *f);
/* w := a on the trainable weights (Keras's finalize_variable_values); CA_ERR_STATE if the average is invalid */
int ca_fitter_apply_average(ca_fitter *f);

/* ---- loss and metrics: loss weights, Huber value loss, label smoothing, Keras's metrics, and the heads read back ----
 * The other half of the reference's model.compile(...) (wrapper.py:272): loss=, loss_weights= and metrics=.  This comment
 * is the definition.
 *
 * Per row with logits h[0..96), pre-tanh value v, policy target t[0..96) and outcome z, ls = label_smoothing:
 *     t'_j         = t_j (1 - ls) + ls / 96                   Keras CategoricalCrossentropy(label_smoothing=); ls = 0: t' = t
 *     policy term  = -sum_j t'_j log_softmax_j(h)
 *     e            = tanh v - z
 *     value term   = e^2                                      CA_VALUE_LOSS_MSE
 *                  = 0.5 e^2 if |e| <= delta, else delta (|e| - 0.5 delta)     CA_VALUE_LOSS_HUBER (Keras Huber(delta))
 * The batch loss is value_weight * mean(value term) + policy_weight * mean(policy term) over the B rows, and its
 * gradients with respect to the heads' outputs, in float32 and the operation order of the default loss kernel:
 *     Hd[j]  = policy_weight * (softmax_j * sum_j t'_j - t'_j) / B
 *     Hd[96] = value_weight * 2 e (1 - tanh^2 v) / B                           MSE
 *            = value_weight * clamp(e, -delta, delta) (1 - tanh^2 v) / B       Huber
 * The sample weight multiplies last, as without this section.  out_losses[1] and [2] are the means of the two terms
 * (not times their weights) and out_losses[0] = value_weight * [1] + policy_weight * [2] (+ R of the fit options), in
 * ca_fitter_train, its batch_losses, ca_fitter_evaluate and ca_fitter_gradients, whose gradient is that of this
 * weighted data loss.  The values stay until they are set again.  At the defaults a step launches the kernels it launches
 * without this section and writes the same bytes.
 *
 * Metrics, per row from the same head outputs the loss reads (Keras's metric names in brackets), c = argmax_j t_j:
 *     categorical_accuracy        argmax_j h_j == c, the FIRST maximum on both sides, the unsmoothed t
 *     top_k_categorical_accuracy  #{j : h_j > h_c} < top_k      (TensorFlow's in_top_k: ties at the boundary are in)
 *     mean_absolute_error         |tanh v - z|
 *     policy_entropy              -sum_j p_j log p_j, p = softmax(h)
 *     target_entropy              -sum_j t_j log t_j, 0 log 0 = 0
 * A call's metric is sum_r w_r x_r / sum_r w_r (Keras's Mean with sample_weight; w_r = 1 on an unweighted set; 0 if the
 * weights sum to 0).  A batch's six sums (of w x for the five, of w) are float32 in a fixed order without atomics; the
 * batches are added in float64 on the host.  ca_fitter_train reports the step's own forward (batch statistics, the
 * weights from before the step: what Keras logs during an epoch), ca_fitter_evaluate the inference-mode one.  Metrics off:
 * nothing is launched or allocated.  On: the losses, gradients and weights of a fit do not change by a bit. */
#define CA_VALUE_LOSS_MSE 0
#define CA_VALUE_LOSS_HUBER 1
typedef struct ca_fit_loss {
  uint32_t struct_size;  /* as ca_fit_options': min(struct_size, the library's sizeof) bytes are read and written */
  float value_weight;    /* finite, >= 0; default 1 */
  float policy_weight;   /* finite, >= 0; default 0.25; not both 0 */
  float label_smoothing; /* in [0, 1); default 0 */
  int32_t value_loss;    /* CA_VALUE_LOSS_MSE (default) or CA_VALUE_LOSS_HUBER */
  float huber_delta;     /* finite, > 0; default 1; read only with HUBER */
} ca_fit_loss;
/* the defaults: what a new fitter has, and what a caller's shorter struct leaves to the library */
#define CA_FIT_LOSS_INIT {sizeof(ca_fit_loss), 1.0f, 0.25f, 0.0f, 0, 1.0f}
/* CA_ERR_ARG and nothing changes on a value outside what the struct's comments allow, judged in float32 (or a
 * struct_size below 4) */
int ca_fitter_set_loss(ca_fitter *f, const ca_fit_loss *loss);
/* out->struct_size must be set by the caller; on return it is the number of bytes written */
int ca_fitter_get_loss(ca_fitter *f, ca_fit_loss *out);
typedef struct ca_fit_metrics {
  uint32_t struct_size; /* as above */
  int32_t top_k;        /* as set */
  int64_t rows;         /* rows of the call */
  double weight_sum;    /* sum of their sample weights (= rows when unweighted) */
  double categorical_accuracy, top_k_categorical_accuracy, mean_absolute_error, policy_entropy, target_entropy;
} ca_fit_metrics;
/* on != 0: every later ca_fitter_train and ca_fitter_evaluate computes the metrics; top_k in 1..96 (else CA_ERR_ARG and
 * nothing changes; looked at only when switching on).  Off on a new fitter, where top_k is 5. */
int ca_fitter_set_metrics(ca_fitter *f, int32_t on, int32_t top_k);
/* of the last ca_fitter_train or ca_fitter_evaluate since metrics were switched on (rows = 0 before the first);
 * CA_ERR_STATE if metrics are off */
int ca_fitter_metrics(ca_fitter *f, ca_fit_metrics *out);
/* Keras's predict: the heads' outputs of rows[0..n_rows), 1 <= n_rows <= max_batch, of a packed or an expanded set.
 * train = 0: inference mode; train != 0: the rows as one training batch, with batch statistics.  Nothing of the
 * fitter's weights, slots or step count changes.  values are pre-tanh. */
int ca_fitter_predict(ca_fitter *f, const int32_t *rows, int32_t n_rows, int32_t train, float *logits /* [n_rows][96] */,
                      float *values /* [n_rows] */);

#ifdef __cplusplus
}
#endif
#endif
