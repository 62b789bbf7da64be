/*
 * abi_reject_arma.c -- argument / extent rejection harness for the ARMAConv
 * entry points of include/mi355_mp.h (mp_arma_ok, mp_arma_width,
 * mp_arma_workspace, mp_arma_step_f32, mp_arma_step_bwd_f32).
 *
 * Built against the host-only AddressSanitizer build (`make asan_arma`) and run as a plain
 * program with no GPU by tests/test_arma_host.py.  A REJECT case passes one bad argument and
 * expects -MP_ERR_ARG with a text naming it, before any launch; an ACCEPT case passes every
 * check and fails at its first HIP call: the boundary is the documented one.
 * Output: one line per case, then "abi_reject_arma: N cases, M failures".
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "mi355_mp.h"

static int n_cases = 0, n_fail = 0;

#define DEV ((void*)(uintptr_t)0x7f0000000000ull) /* fake device pointer, never dereferenced */
#define DEVF ((float*)DEV)
#define DEVI ((int32_t*)DEV)

static void expect(int line, const char* what, int64_t rc, int want_arg, const char* needle) {
  ++n_cases;
  const char* err = mp_last_error();
  int ok;
  if (want_arg) {
    ok = rc == -MP_ERR_ARG && (!needle || (err && strstr(err, needle)));
  } else {
    ok = rc != -MP_ERR_ARG;
  }
  printf("%s line %d: %s -> rc %lld (%s)\n", ok ? "ok  " : "FAIL", line, what, (long long)rc, err ? err : "");
  if (!ok) ++n_fail;
}

#define REJECT(needle, call) expect(__LINE__, #call, (call), 1, needle)
#define ACCEPT(call) expect(__LINE__, #call, (call), 0, NULL)

int main(void) {
  const int64_t N = 257, E = 3000;
  const int K = 3, C = 7, P = 24; /* K * C = 21 rounded up to 4 */
  mp_csr g;
  memset(&g, 0, sizeof g);
  g.rowptr = g.col = g.eid = g.wave_row = g.wave_slot = g.split_waves = DEVI;
  g.n_rows = N;
  g.n_edges = E;
  g.n_cols = (int32_t)N;
  g.chunk = 64;
  g.n_waves = 51;
  g.n_split = 1;

  const size_t WS = mp_arma_workspace(&g, K, C);
  const size_t ROWS = ((size_t)(N - 1) * P + P) * 4, WB = (size_t)K * C * C * 4, LAP = (size_t)E * 4;
  const size_t OUT = ((size_t)(N - 1) * C + C) * 4;
  /* mp_arma_ok / mp_arma_width / mp_arma_workspace: the example's shapes, the limits on each side */
  const int answers =
      mp_arma_ok(3, 16) == 1 && mp_arma_ok(3, 7) == 1 && mp_arma_ok(1, 64) == 1 && mp_arma_ok(2, 64) == 1 &&
      mp_arma_ok(3, 64) == 0 && mp_arma_ok(8, 32) == 1 && mp_arma_ok(9, 32) == 0 && mp_arma_ok(256, 1) == 1 &&
      mp_arma_ok(257, 1) == 0 && mp_arma_ok(1, 65) == 0 && mp_arma_ok(0, 4) == 0 && mp_arma_ok(4, 0) == 0 &&
      mp_arma_ok(-1, 4) == 0 && mp_arma_width(3, 7) == 24 && mp_arma_width(3, 16) == 48 &&
      mp_arma_width(9, 32) == -MP_ERR_ARG && WS > mp_arma_workspace(NULL, K, C) && WS >= 2u * 51u * 256u * 4u;
  ++n_cases;
  n_fail += !answers;
  printf("%s mp_arma_ok / width / workspace answers\n", answers ? "ok  " : "FAIL");

#define STEP(g_, lap_, lapb, y_, ldy, yb, s_, w_, wb, K_, C_, relu, h_, n_, nb, o_, ldo, ob, ws_, wsb)                  \
  mp_arma_step_f32(g_, lap_, lapb, y_, ldy, yb, s_, P, ROWS, w_, wb, K_, C_, relu, h_, P, ROWS, n_, P, nb, o_, ldo, ob, \
                   ws_, wsb, NULL)
  ACCEPT(STEP(&g, DEVF, LAP, DEVF, P, ROWS, DEVF, DEVF, WB, K, C, 1, DEVF, DEVF, ROWS, NULL, 0, 0, DEV, WS));
  ACCEPT(STEP(&g, DEVF, LAP, DEVF, P, ROWS, DEVF, NULL, 0, K, C, 0, NULL, NULL, 0, DEVF, C, OUT, DEV, WS));
  REJECT("null graph", STEP(NULL, DEVF, LAP, DEVF, P, ROWS, DEVF, DEVF, WB, K, C, 1, DEVF, DEVF, ROWS, NULL, 0, 0, DEV, WS));
  REJECT("lap is NULL", STEP(&g, NULL, LAP, DEVF, P, ROWS, DEVF, DEVF, WB, K, C, 1, DEVF, DEVF, ROWS, NULL, 0, 0, DEV, WS));
  REJECT("lap holds", STEP(&g, DEVF, LAP - 4, DEVF, P, ROWS, DEVF, DEVF, WB, K, C, 1, DEVF, DEVF, ROWS, NULL, 0, 0, DEV, WS));
  REJECT("y is NULL", STEP(&g, DEVF, LAP, NULL, P, ROWS, DEVF, DEVF, WB, K, C, 1, DEVF, DEVF, ROWS, NULL, 0, 0, DEV, WS));
  REJECT("ld of y", STEP(&g, DEVF, LAP, DEVF, P - 4, ROWS, DEVF, DEVF, WB, K, C, 1, DEVF, DEVF, ROWS, NULL, 0, 0, DEV, WS));
  REJECT("multiple of 4", STEP(&g, DEVF, LAP, DEVF, P + 1, 2 * ROWS, DEVF, DEVF, WB, K, C, 1, DEVF, DEVF, ROWS, NULL, 0, 0, DEV, WS));
  REJECT("16-byte aligned", STEP(&g, DEVF, LAP, DEVF + 1, P, ROWS, DEVF, DEVF, WB, K, C, 1, DEVF, DEVF, ROWS, NULL, 0, 0, DEV, WS));
  REJECT("y holds", STEP(&g, DEVF, LAP, DEVF, P, ROWS - 4, DEVF, DEVF, WB, K, C, 1, DEVF, DEVF, ROWS, NULL, 0, 0, DEV, WS));
  REJECT("s is NULL", STEP(&g, DEVF, LAP, DEVF, P, ROWS, NULL, DEVF, WB, K, C, 1, DEVF, DEVF, ROWS, NULL, 0, 0, DEV, WS));
  REJECT("come together", STEP(&g, DEVF, LAP, DEVF, P, ROWS, DEVF, DEVF, WB, K, C, 1, DEVF, NULL, 0, NULL, 0, 0, DEV, WS));
  REJECT("exactly one", STEP(&g, DEVF, LAP, DEVF, P, ROWS, DEVF, DEVF, WB, K, C, 1, DEVF, DEVF, ROWS, DEVF, C, OUT, DEV, WS));
  REJECT("w_next holds", STEP(&g, DEVF, LAP, DEVF, P, ROWS, DEVF, DEVF, WB - 4, K, C, 1, DEVF, DEVF, ROWS, NULL, 0, 0, DEV, WS));
  REJECT("y_next holds", STEP(&g, DEVF, LAP, DEVF, P, ROWS, DEVF, DEVF, WB, K, C, 1, DEVF, DEVF, ROWS - 4, NULL, 0, 0, DEV, WS));
  REJECT("ld of out", STEP(&g, DEVF, LAP, DEVF, P, ROWS, DEVF, NULL, 0, K, C, 0, NULL, NULL, 0, DEVF, C - 1, OUT, DEV, WS));
  REJECT("out holds", STEP(&g, DEVF, LAP, DEVF, P, ROWS, DEVF, NULL, 0, K, C, 0, NULL, NULL, 0, DEVF, C, OUT - 4, DEV, WS));
  REJECT("relu", STEP(&g, DEVF, LAP, DEVF, P, ROWS, DEVF, DEVF, WB, K, C, 2, DEVF, DEVF, ROWS, NULL, 0, 0, DEV, WS));
  REJECT("K = 0", STEP(&g, DEVF, LAP, DEVF, P, ROWS, DEVF, DEVF, WB, 0, C, 1, DEVF, DEVF, ROWS, NULL, 0, 0, DEV, WS));
  REJECT("C <= 64", STEP(&g, DEVF, LAP, DEVF, P, ROWS, DEVF, DEVF, WB, 1, 65, 1, DEVF, DEVF, ROWS, NULL, 0, 0, DEV, WS));
  REJECT("K * C <= 256", STEP(&g, DEVF, LAP, DEVF, P, ROWS, DEVF, DEVF, WB, 9, 32, 1, DEVF, DEVF, ROWS, NULL, 0, 0, DEV, WS));
  REJECT("ws holds", STEP(&g, DEVF, LAP, DEVF, P, ROWS, DEVF, DEVF, WB, K, C, 1, DEVF, DEVF, ROWS, NULL, 0, 0, DEV, WS - 1));
  {
    mp_csr b = g;
    b.col = NULL;
    REJECT("col is NULL", STEP(&b, DEVF, LAP, DEVF, P, ROWS, DEVF, DEVF, WB, K, C, 1, DEVF, DEVF, ROWS, NULL, 0, 0, DEV, WS));
    b = g;
    b.n_split = 52;
    REJECT("n_split", STEP(&b, DEVF, LAP, DEVF, P, ROWS, DEVF, DEVF, WB, K, C, 1, DEVF, DEVF, ROWS, NULL, 0, 0, DEV, WS));
    b = g;
    b.chunk = 8;
    REJECT("bad schedule", STEP(&b, DEVF, LAP, DEVF, P, ROWS, DEVF, DEVF, WB, K, C, 1, DEVF, DEVF, ROWS, NULL, 0, 0, DEV, WS));
  }

#define BWD(g_, dp_, dpb, w_, wb, h_, hb, dy_, dyb, q_, qb, wsb) \
  mp_arma_step_bwd_f32(g_, DEVF, LAP, dp_, P, dpb, w_, wb, h_, P, hb, K, C, dy_, P, dyb, q_, P, qb, DEV, wsb, NULL)
  ACCEPT(BWD(&g, DEVF, ROWS, DEVF, WB, DEVF, ROWS, DEVF, ROWS, DEVF, ROWS, WS));
  ACCEPT(BWD(&g, DEVF, ROWS, DEVF, WB, NULL, 0, DEVF, ROWS, DEVF, ROWS, WS));
  ACCEPT(BWD(&g, DEVF, ROWS, NULL, 0, NULL, 0, DEVF, ROWS, NULL, 0, WS));
  REJECT("dpre is NULL", BWD(&g, NULL, ROWS, DEVF, WB, DEVF, ROWS, DEVF, ROWS, DEVF, ROWS, WS));
  REJECT("dpre holds", BWD(&g, DEVF, ROWS - 4, DEVF, WB, DEVF, ROWS, DEVF, ROWS, DEVF, ROWS, WS));
  REJECT("dy is NULL", BWD(&g, DEVF, ROWS, DEVF, WB, DEVF, ROWS, NULL, ROWS, DEVF, ROWS, WS));
  REJECT("dy holds", BWD(&g, DEVF, ROWS, DEVF, WB, DEVF, ROWS, DEVF, ROWS - 4, DEVF, ROWS, WS));
  REJECT("come together", BWD(&g, DEVF, ROWS, DEVF, WB, DEVF, ROWS, DEVF, ROWS, NULL, 0, WS));
  REJECT("mask source", BWD(&g, DEVF, ROWS, NULL, 0, DEVF, ROWS, DEVF, ROWS, NULL, 0, WS));
  REJECT("h holds", BWD(&g, DEVF, ROWS, DEVF, WB, DEVF, ROWS - 4, DEVF, ROWS, DEVF, ROWS, WS));
  REJECT("w_t holds", BWD(&g, DEVF, ROWS, DEVF, WB - 4, DEVF, ROWS, DEVF, ROWS, DEVF, ROWS, WS));
  REJECT("dpre_prev holds", BWD(&g, DEVF, ROWS, DEVF, WB, DEVF, ROWS, DEVF, ROWS, DEVF, ROWS - 4, WS));
  REJECT("ws holds", BWD(&g, DEVF, ROWS, DEVF, WB, DEVF, ROWS, DEVF, ROWS, DEVF, ROWS, WS - 1));

  printf("abi_reject_arma: %d cases, %d failures\n", n_cases, n_fail);
  return n_fail ? 1 : 0;
}
