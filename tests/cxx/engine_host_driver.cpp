// engine_host_driver.cpp -- TEST: the host side of the engine driven through the C ABI (include/corintho_hip.h) by a
// plain program, linked with the emulation build of engine.hip (tests/emu) so that it runs on the CPU under the host
// compiler's sanitizers (tests/emu/sanitize.mk, target host_driver) with nothing loaded into an interpreter.  It walks
// the paths that build networks, pass the protocol's words between "device" and host, and move samples: a fused
// generation, the host-driven protocol with the evaluation cache, a caller-supplied network that works and one that
// fails, a tournament with a logged match, the three sample exits, a stand-alone network, the per-game text logs over
// two generations, an arena, the analysis of given positions, page-locked caller buffers and the read-outs that refuse.
// Exit status 0: every call returned what it should, the sample exits agree and the logs repeat byte for byte.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <stdlib.h>
#include <unistd.h>

#include "../../include/corintho_hip.h"

namespace {
constexpr int GS = 70, NM = 96, NSYM = 8, MLP = 1;

#define EXPECT(rc, call)                                                                              \
  do {                                                                                                \
    const int got_ = (call);                                                                          \
    if (got_ != (rc)) {                                                                               \
      fprintf(stderr, "%s:%d: %s returned %d, expected %d (%s)\n", __FILE__, __LINE__, #call, got_, (rc), ca_last_error()); \
      exit(1);                                                                                        \
    }                                                                                                 \
  } while (0)
#define OK(call) EXPECT(CA_OK, call)
#define REQUIRE(cond)                                                     \
  do {                                                                    \
    if (!(cond)) {                                                        \
      fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                            \
    }                                                                     \
  } while (0)

// mlp12x100 in the flat layout of nn.h: small pseudo-random kernels, BatchNorm at identity
std::vector<float> mlp_weights(uint32_t seed) {
  std::vector<float> w;
  auto next = [&] {
    seed = seed * 1664525u + 1013904223u;
    return ((float)(seed >> 8) / (float)(1 << 24) - 0.5f) * 0.2f;
  };
  for (int l = 0; l < 12; ++l) {
    for (int i = 0; i < (l == 0 ? GS : 100) * 100; ++i) w.push_back(next());
    for (float c : {0.0f, 1.0f, 0.0f, 0.0f, 1.0f})  // bias, gamma, beta, moving mean, moving variance
      w.insert(w.end(), 100, c);
  }
  for (int i = 0; i < 100; ++i) w.push_back(next());
  w.push_back(0.0f);
  for (int i = 0; i < 100 * NM; ++i) w.push_back(next());
  w.insert(w.end(), NM, 0.0f);
  return w;
}

ca_config config(int games, int searches, int spe) {
  ca_config c;
  memset(&c, 0, sizeof c);
  c.num_games = games;
  c.seed = 11;
  c.max_searches = searches;
  c.searches_per_eval = spe;
  c.c_puct = 1.0f;
  c.epsilon = 0.25f;
  c.no_stagger = 1;
  return c;
}

// a caller's network: value 0, uniform priors, for every row of the launch; fails from call `fail_at` on (0: never)
struct UniformNet {
  std::vector<float> states, evals, probs;
  int calls = 0, fail_at = 0;
  explicit UniformNet(int rows) : states((size_t)rows * GS), evals(rows), probs((size_t)rows * NM) {}
};
int uniform_net(void *user, int32_t row0, int32_t cap_rows, const int32_t *d_rows, void *) {
  UniformNet *n = (UniformNet *)user;
  if (n->fail_at && ++n->calls >= n->fail_at) return 1;
  if (*d_rows > cap_rows) return 2;
  for (int r = row0; r < row0 + cap_rows; ++r) {
    n->evals[r] = 0.0f;
    for (int m = 0; m < NM; ++m) n->probs[(size_t)r * NM + m] = 1.0f / NM;
  }
  return 0;
}

// a fresh directory for the files of one scenario, and what a file in it holds ("" if it cannot be read)
std::string temp_dir() {
  char name[] = "/tmp/engine_host_driver_XXXXXX";
  REQUIRE(mkdtemp(name) != nullptr);
  return name;
}
std::string slurp(const std::string &path) {
  std::string s;
  if (FILE *f = fopen(path.c_str(), "rb")) {
    char buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) s.append(buf, n);
    fclose(f);
  }
  return s;
}
void remove_dir(const std::string &dir, const std::vector<std::string> &files) {
  for (const std::string &f : files) remove((dir + "/" + f).c_str());
  rmdir(dir.c_str());
}

void fused_generation_and_sample_exits(const std::vector<float> &w) {
  ca_config c = config(8, 24, 8);
  c.resident = 4;
  ca_trainer *t = nullptr;
  OK(ca_trainer_create(&c, &t));
  OK(ca_trainer_set_net(t, 0, MLP, w.data(), w.size()));
  EXPECT(CA_ERR_ARG, ca_trainer_set_net(t, 0, 99, w.data(), w.size()));
  int32_t done = 0, n = 0, packed = 0;
  OK(ca_trainer_run(t, 0, &done));
  REQUIRE(done == 1);
  OK(ca_trainer_num_samples(t, &n));
  REQUIRE(n > 0);
  // writeSamples, export + expand, pack into "device" memory: the same rows
  std::vector<float> gs((size_t)n * NSYM * GS), ev((size_t)n * NSYM), pr((size_t)n * NSYM * NM);
  OK(ca_trainer_write_samples(t, gs.data(), ev.data(), pr.data()));
  std::vector<float> sp((size_t)n * (GS + NM)), oc(n), dsp(sp.size()), doc(n);
  OK(ca_trainer_export_samples(t, sp.data(), oc.data()));
  EXPECT(CA_ERR_ARG, ca_trainer_pack_samples_device(t, dsp.data(), doc.data(), n - 1, &packed));
  OK(ca_trainer_pack_samples_device(t, dsp.data(), doc.data(), n, &packed));
  REQUIRE(packed == n && sp == dsp && oc == doc);
  std::vector<float> gs2(gs.size()), ev2(ev.size()), pr2(pr.size());
  OK(ca_expand_samples(0, sp.data(), oc.data(), n, gs2.data(), ev2.data(), pr2.data()));
  REQUIRE(gs == gs2 && ev == ev2 && pr == pr2);
  // net_forward and net_bench widen the caller's 70-float rows
  std::vector<float> e(5), p(5 * NM);
  float ms = 0;
  OK(ca_trainer_net_forward(t, 0, gs.data(), 5, e.data(), p.data()));
  OK(ca_trainer_net_bench(t, 0, gs.data(), 5, 1, &ms));
  ca_trainer_destroy(t);
}

void host_cache_iterations() {
  ca_config c = config(8, 24, 8);
  ca_trainer *t = nullptr;
  OK(ca_trainer_create(&c, &t));
  OK(ca_trainer_set_host_cache(t, 0));
  std::vector<float> states((size_t)64 * GS), evals(64, 0.0f), probs((size_t)64 * NM, 1.0f / NM);
  for (int it = 0; it < 3; ++it) {
    int32_t done = 0, n = 0;
    OK(ca_trainer_do_iteration(t, evals.data(), probs.data(), -1, &done));
    OK(ca_trainer_num_requests(t, -1, &n));
    REQUIRE(!done && n > 0 && n <= 64);
    OK(ca_trainer_write_requests(t, states.data(), -1));
  }
  ca_trainer_destroy(t);
}

void caller_supplied_network() {
  ca_config c = config(8, 24, 8);
  ca_trainer *t = nullptr;
  OK(ca_trainer_create(&c, &t));
  int32_t rows = 0, done = 0;
  OK(ca_trainer_request_rows(t, &rows));
  UniformNet net(rows);
  EXPECT(CA_ERR_ARG, ca_trainer_set_net_fn(t, 0, nullptr, &net, net.states.data(), net.evals.data(), net.probs.data(), rows, 0.0));
  EXPECT(CA_ERR_ARG, ca_trainer_set_net_fn(t, 0, uniform_net, &net, net.states.data(), net.evals.data(), net.probs.data(), rows - 1, 0.0));
  OK(ca_trainer_set_net_fn(t, 0, uniform_net, &net, net.states.data(), net.evals.data(), net.probs.data(), rows, 0.0));
  OK(ca_trainer_run(t, 0, &done));
  REQUIRE(done == 1);
  // the same generation again with a function that gives up at its third call
  OK(ca_trainer_reset(t, 12));
  net.fail_at = 3;
  EXPECT(CA_ERR_CALLBACK, ca_trainer_run(t, 0, &done));
  EXPECT(CA_ERR_STATE, ca_trainer_run(t, 0, &done));
  net.fail_at = 0;
  OK(ca_trainer_reset(t, 12));
  OK(ca_trainer_run(t, 4, &done));
  ca_trainer_destroy(t);
}

void tournament(const std::vector<float> &w0, const std::vector<float> &w1) {
  ca_tourney *t = nullptr;
  OK(ca_tourney_create(0, 0, 0, &t));
  OK(ca_tourney_add_player(t, 0, 0, 16, 4, 1.0f, 0.25f, 0));
  OK(ca_tourney_add_player(t, 1, 1, 12, 4, 1.0f, 0.25f, 0));
  const std::string dir = temp_dir();
  OK(ca_tourney_set_log_folder(t, dir.c_str()));
  OK(ca_tourney_add_match(t, 0, 1, 1));  // this one writes match_0_1_0.txt
  OK(ca_tourney_add_match(t, 1, 0, 0));
  int32_t done = 0;
  OK(ca_tourney_set_net(t, 0, MLP, w0.data(), w0.size()));
  EXPECT(CA_ERR_STATE, ca_tourney_run(t, 0, &done));  // no network for model 1
  OK(ca_tourney_set_net(t, 1, 99, w1.data(), w1.size()));
  EXPECT(CA_ERR_ARG, ca_tourney_run(t, 0, &done));  // an unknown kind, as a trainer reports it
  OK(ca_tourney_set_net(t, 1, MLP, w1.data(), w1.size()));
  OK(ca_tourney_run(t, 0, &done));
  REQUIRE(done == 1);
  OK(ca_tourney_all_done(t, &done));
  REQUIRE(done == 1 && !slurp(dir + "/match_0_1_0.txt").empty() && slurp(dir + "/match_1_0_1.txt").empty());
  ca_tourney_destroy(t);
  remove_dir(dir, {"match_0_1_0.txt"});
}

void stand_alone_network(const std::vector<float> &w) {
  ca_net *n = nullptr;
  EXPECT(CA_ERR_ARG, ca_net_create(0, 99, w.data(), w.size(), 16, &n));
  OK(ca_net_create(0, MLP, w.data(), w.size(), 16, &n));
  std::vector<float> states((size_t)16 * GS, 0.25f), evals(16), probs((size_t)16 * NM);
  const int32_t rows = 9;
  OK(ca_net_forward_device(n, states.data(), 16, &rows, evals.data(), probs.data(), nullptr));
  EXPECT(CA_ERR_ARG, ca_net_forward_device(n, states.data(), 17, &rows, evals.data(), probs.data(), nullptr));
  float sum = 0;
  for (int m = 0; m < NM; ++m) sum += probs[(size_t)8 * NM + m];
  REQUIRE(sum > 0.99f && sum < 1.01f);
  // the same rows as a fused run with a cache launches them: read through in_idx, written through out_idx into one array
  // of 100 floats per element; nothing is written for the entries from the count on
  const std::vector<int32_t> in_idx = {8, 3, 15, 0, 0, 0}, out_idx = {5, 0, 19, 7, 7, 7};
  const int32_t three = 3;
  std::vector<float> val((size_t)20 * 100, -7.0f);
  OK(ca_net_forward_device_io(n, states.data(), 16, 6, &three, in_idx.data(), out_idx.data(), val.data(), 100, val.data() + 4, 100, 0, nullptr));
  for (int e = 0; e < 20; ++e)
    for (int f = 0; f < 100; ++f) {
      const bool written = (e == 5 || e == 0 || e == 19) && (f == 0 || f >= 4);
      REQUIRE(written ? val[(size_t)e * 100 + f] == (f == 0 ? evals[8] : probs[(size_t)8 * NM + f - 4]) : val[(size_t)e * 100 + f] == -7.0f);
    }
  EXPECT(CA_ERR_ARG, ca_net_forward_device_io(n, states.data(), 17, 6, &three, in_idx.data(), out_idx.data(), val.data(), 100, val.data() + 4, 100, 0, nullptr));
  EXPECT(CA_ERR_ARG, ca_net_forward_device_io(n, states.data(), 16, 6, &three, in_idx.data(), out_idx.data(), val.data(), 0, val.data() + 4, 100, 0, nullptr));
  EXPECT(CA_ERR_ARG, ca_net_forward_device_io(n, states.data(), 16, 6, &three, in_idx.data(), out_idx.data(), val.data(), 100, val.data() + 4, 95, 0, nullptr));
  EXPECT(CA_ERR_ARG, ca_net_forward_device_io(n, states.data(), 5, 6, &three, nullptr, nullptr, val.data(), 100, val.data() + 4, 100, 0, nullptr));
  ca_net_destroy(n);
}

// the per-game text logs: the first two of six games on four slots, over two generations of the same seed
void text_logs(const std::vector<float> &w) {
  const std::string dir = temp_dir();
  const std::vector<std::string> files = {"game_0.txt", "game_1.txt"};
  ca_config c = config(6, 50, 8);
  c.resident = 4;
  ca_trainer *t = nullptr;
  OK(ca_trainer_create(&c, &t));
  OK(ca_trainer_set_net(t, 0, MLP, w.data(), w.size()));
  EXPECT(CA_ERR_ARG, ca_trainer_set_logging(t, dir.c_str(), 5));  // a logged game starts in a slot of its own
  OK(ca_trainer_set_logging(t, dir.c_str(), 2));
  std::string first[2];
  for (int generation = 0; generation < 2; ++generation) {
    int32_t done = 0;
    OK(ca_trainer_run(t, 0, &done));
    REQUIRE(done == 1);
    for (int k = 0; k < 2; ++k) {
      const std::string text = slurp(dir + "/" + files[k]);
      REQUIRE(!text.empty());
      if (generation == 0) first[k] = text;
      REQUIRE(text == first[k]);
      remove((dir + "/" + files[k]).c_str());
    }
    EXPECT(CA_ERR_STATE, ca_trainer_set_logging(t, dir.c_str(), 2));  // the games have started
    OK(ca_trainer_reset(t, c.seed));
  }
  ca_trainer_destroy(t);
  remove_dir(dir, files);
}

void arena(const std::vector<float> &w0, const std::vector<float> &w1) {
  ca_config c = config(8, 50, 8);
  c.testing = 1;
  ca_trainer *t = nullptr;
  OK(ca_trainer_create(&c, &t));
  int32_t done = 0;
  OK(ca_trainer_set_net(t, 0, MLP, w0.data(), w0.size()));
  EXPECT(CA_ERR_STATE, ca_trainer_run(t, 0, &done));  // arena mode needs both networks
  OK(ca_trainer_set_net(t, 1, MLP, w1.data(), w1.size()));
  OK(ca_trainer_run(t, 0, &done));
  REQUIRE(done == 1);
  float score = -1.0f;
  OK(ca_trainer_score(t, &score));
  REQUIRE(score >= 0.0f && score <= 1.0f);
  const std::string dir = temp_dir();
  OK(ca_trainer_write_scores(t, (dir + "/scores.txt").c_str()));
  const std::string scores = slurp(dir + "/scores.txt");
  int lines = 0;
  for (char ch : scores) lines += ch == '\n';
  REQUIRE(lines == 6);
  float gs[1], ev[1], pr[1];
  EXPECT(CA_ERR_STATE, ca_trainer_write_samples(t, gs, ev, pr));  // a testing trainer keeps no samples
  ca_trainer_destroy(t);
  remove_dir(dir, {"scores.txt"});
}

// three positions: the empty board under two seeds, and one met in a random playout (tests/test_analyse.py _positions)
void analysis(const std::vector<float> &w) {
  const int n = 3;
  std::vector<int32_t> boards((size_t)n * 64, 0), to_play = {0, 0, 1}, seeds = {3, 4, 5};
  std::vector<int32_t> pieces = {4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 3, 3, 3, 3, 4, 3};
  const uint64_t met = 0x4200090100004000ull;
  for (int i = 0; i < 64; ++i) boards[(size_t)2 * 64 + i] = (int32_t)(met >> i & 1);
  ca_config c = config(n, 50, 8);
  c.analyse = 1;
  ca_trainer *t = nullptr;
  OK(ca_trainer_create(&c, &t));
  OK(ca_trainer_set_net(t, 0, MLP, w.data(), w.size()));
  int32_t done = 0;
  std::vector<int32_t> out((size_t)n * 8);
  EXPECT(CA_ERR_STATE, ca_trainer_run(t, 0, &done));  // no positions yet
  boards[5] = 2;
  EXPECT(CA_ERR_ARG, ca_trainer_set_positions(t, boards.data(), to_play.data(), pieces.data(), seeds.data()));
  boards[5] = 0;
  OK(ca_trainer_set_positions(t, boards.data(), to_play.data(), pieces.data(), seeds.data()));
  EXPECT(CA_ERR_STATE, ca_trainer_analysis(t, out.data()));  // nothing searched
  OK(ca_trainer_run(t, 2, &done));
  REQUIRE(done == 0);
  EXPECT(CA_ERR_STATE, ca_trainer_analysis(t, out.data()));  // the searches have not ended
  OK(ca_trainer_finish(t));
  OK(ca_trainer_analysis(t, out.data()));
  for (int i = 0; i < n; ++i) REQUIRE(out[(size_t)i * 8] >= 0 && out[(size_t)i * 8] < NM);
  ca_trainer_destroy(t);
  // a trainer of games takes no positions
  c.analyse = 0;
  OK(ca_trainer_create(&c, &t));
  EXPECT(CA_ERR_STATE, ca_trainer_set_positions(t, boards.data(), to_play.data(), pieces.data(), seeds.data()));
  ca_trainer_destroy(t);
}

void pins_trace_and_info() {
  ca_config c = config(8, 24, 8);
  ca_trainer *t = nullptr;
  OK(ca_trainer_create(&c, &t));
  std::vector<float> a(4096), b(64);
  int32_t pinned = 0, words = 0, info[8];
  OK(ca_trainer_pin_host(t, a.data(), 1024, &pinned));
  REQUIRE(pinned == 1);
  OK(ca_trainer_pin_host(t, a.data(), a.size() * 4, &pinned));  // again, with more bytes
  REQUIRE(pinned == 1);
  OK(ca_trainer_unpin_host(t, a.data()));
  OK(ca_trainer_unpin_host(t, b.data()));  // never pinned
  OK(ca_trainer_pin_host(t, b.data(), b.size() * 4, &pinned));  // still pinned when the trainer goes
  EXPECT(CA_ERR_STATE, ca_trainer_trace(t, 0, nullptr, 0, &words));  // created without ca_config.trace
  EXPECT(CA_ERR_ARG, ca_trainer_game_info(t, c.num_games, info));
  OK(ca_trainer_game_info(t, c.num_games - 1, info));
  ca_trainer_destroy(t);
}
}  // namespace

int main() {
  const std::vector<float> w0 = mlp_weights(1), w1 = mlp_weights(2);
  fused_generation_and_sample_exits(w0);
  host_cache_iterations();
  caller_supplied_network();
  tournament(w0, w1);
  stand_alone_network(w0);
  text_logs(w0);
  arena(w0, w1);
  analysis(w0);
  pins_trace_and_info();
  puts("engine_host_driver: ok");
  return 0;
}
