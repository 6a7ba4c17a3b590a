// Driver of tests/test_net_pack.py: csrc/nn_layout.h's offsets and csrc/nn_split.h's packers (host part, -DCO_EMU), as a
// program of its own.  Binary float32 in on stdin, binary uint32 words out on stdout.
//   net_pack_driver layouts                       "<network> <name> <offset>" per line, in the order of the flat array
//   net_pack_driver step <tiles> <nt> <f16> <st>  stdin: W[128][128] (k-major); one K step of co_pack_step into a buffer
//                                                 pre-filled with 0xDEADBEEF
//   net_pack_driver mlp|trunk|head <nt> <f16>     stdin: the network's flat weights; the whole fragment buffer
// A refused weight (std::invalid_argument): its message on stderr, exit status 3.
#include <stdio.h>
#include <stdlib.h>

#include "../../corintho_ai_amd/csrc/nn_split.h"

static std::vector<float> read_floats(size_t n) {
  std::vector<float> v(n);
  if (fread(v.data(), 4, n, stdin) != n) {
    fprintf(stderr, "net_pack_driver: expected %zu floats on stdin\n", n);
    exit(2);
  }
  return v;
}

static void layouts() {
  constexpr MlpLayout M;
  for (int l = 0; l < M.LAYERS; ++l)
    printf("mlp kernel%d %d\nmlp bias%d %d\nmlp gamma%d %d\nmlp beta%d %d\nmlp mean%d %d\nmlp var%d %d\n", l, M.kernel(l), l, M.bias(l), l,
           M.gamma(l), l, M.beta(l), l, M.mean(l), l, M.var(l));
  printf("mlp kv %d\nmlp bv %d\nmlp kp %d\nmlp bp %d\nmlp nw %d\n", M.kv, M.bv, M.kp, M.bp, M.nw);
  constexpr ResCnnLayout R;
  for (int j = 0; j < R.NBN; ++j) {
    printf("rescnn kernel%d %d\n", j, j < R.CONVS ? R.kernel(j) : j == 9 ? R.p_k : R.v_k);
    printf("rescnn bias%d %d\nrescnn gamma%d %d\nrescnn beta%d %d\nrescnn mean%d %d\nrescnn var%d %d\n", j, R.bias(j), j, R.gamma(j), j,
           R.beta(j), j, R.mean(j), j, R.var(j));
    if (j == 9) printf("rescnn p_dk %d\nrescnn p_db %d\n", R.p_dk, R.p_db);
  }
  printf("rescnn v_d1k %d\nrescnn v_d1b %d\nrescnn v_d2k %d\nrescnn v_d2b %d\nrescnn nw %d\n", R.v_d1k, R.v_d1b, R.v_d2k, R.v_d2b, R.nw);
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  if (mode == "layouts") return layouts(), 0;
  if (argc < 4) return 2;
  std::vector<uint32_t> out;
  try {
    if (mode == "step" && argc == 6) {
      const int tiles = atoi(argv[2]), nt = atoi(argv[3]), st = atoi(argv[5]);
      const std::vector<float> W = read_floats(128 * 128);
      out.assign((size_t)tiles * nt * 256, 0xDEADBEEFu);
      co_pack_step(out.data(), tiles, st, nt, atoi(argv[4]) != 0, F16RangeText{"step: ", " is out of range"},
                   [&](int k, int o) { return W[(size_t)k * 128 + o]; });
    } else {
      const int nt = atoi(argv[2]);
      const bool f16 = atoi(argv[3]) != 0;
      if (mode == "mlp") out = co_pack_mlp_split(read_floats(CO_MLP_NUM_WEIGHTS).data(), nt, f16);
      else if (mode == "trunk") out = co_pack_rescnn_trunk(read_floats(CO_RESCNN4_NUM_WEIGHTS).data(), nt, f16);
      else if (mode == "head") out = co_pack_rescnn_head(read_floats(CO_RESCNN4_NUM_WEIGHTS).data(), nt, f16);
      else return 2;
    }
  } catch (const std::invalid_argument &e) {
    fprintf(stderr, "%s\n", e.what());
    return 3;
  }
  return fwrite(out.data(), 4, out.size(), stdout) == out.size() ? 0 : 1;
}
