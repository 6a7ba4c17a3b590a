// Driver of tests/test_host_terms.py: csrc/nn_split.h's split_terms on the float bit patterns read from stdin.
// usage: split_terms_driver <nt> <f16: 0|1>; one hexadecimal float32 per line in, "t0 t1 [t2]" (hexadecimal) per line out.
#include <stdio.h>
#include <stdlib.h>

#include "../../corintho_ai_amd/csrc/nn_split.h"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  const int nt = atoi(argv[1]);
  const bool f16 = atoi(argv[2]) != 0;
  if (nt < 1 || nt > 3) return 2;
  unsigned u;
  while (scanf("%x", &u) == 1) {
    float v;
    memcpy(&v, &u, 4);
    uint16_t t[3];
    split_terms(v, nt, f16, t);
    for (int i = 0; i < nt; ++i) printf("%04x%c", t[i], i + 1 < nt ? ' ' : '\n');
  }
  return 0;
}
