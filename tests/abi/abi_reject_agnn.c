/*
 * abi_reject_agnn.c -- argument / extent rejection harness for the AGNNConv entry
 * points of include/mi355_mp.h (mp_agnn_ok, mp_agnn_split_chunk, mp_agnn_workspace,
 * mp_agnn_rnorm_f32, mp_agnn_aggregate_f32, mp_agnn_backward_dst_f32,
 * mp_agnn_backward_src_f32).
 *
 * Built against the host-only AddressSanitizer build (`make asan_agnn`) and run as a plain
 * program with no GPU by tests/test_agnn_host.py.  A REJECT case passes one bad argument and
 * expects -MP_ERR_ARG with a text naming it, before any launch; an ACCEPT case passes every
 * check and fails at its first HIP call: the boundary is the documented one.
 * Output: one line per case, then "abi_reject_agnn: N cases, M failures".
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
  const int64_t N = 300, E = 4300;
  const int F = 18, LD = 20;
  mp_csr g;
  memset(&g, 0, sizeof g);
  g.rowptr = g.col = g.eid = g.wave_row = g.wave_slot = g.split_waves = DEVI;
  g.n_rows = N;
  g.n_edges = E;
  g.n_cols = (int32_t)N;
  g.chunk = 64;
  g.n_waves = 72;
  g.n_split = 1;

  const size_t ROWS = ((size_t)(N - 1) * LD + F) * 4, VEC = (size_t)N * 4, EDG = (size_t)E * 4;
  const size_t W0 = mp_agnn_workspace(&g, F, MP_AGNN_PASS_FWD), W1 = mp_agnn_workspace(&g, F, MP_AGNN_PASS_DST),
               W2 = mp_agnn_workspace(&g, F, MP_AGNN_PASS_SRC);
  mp_csr rows = g; /* a schedule below the split chunk: walked by rows, no slab */
  rows.chunk = 16;
  const int answers = mp_agnn_ok(1) == 1 && mp_agnn_ok(1024) == 1 && mp_agnn_ok(1025) == 0 && mp_agnn_ok(0) == 0 &&
                      mp_agnn_ok(-3) == 0 && mp_agnn_split_chunk() == 64 && W0 >= 2u * 72u * 24u * 4u &&
                      W1 > W0 && W2 >= 2u * 72u * 40u * 4u && mp_agnn_workspace(&rows, F, MP_AGNN_PASS_FWD) < W0 &&
                      mp_agnn_workspace(NULL, F, MP_AGNN_PASS_FWD) > 0;
  ++n_cases;
  n_fail += !answers;
  printf("%s mp_agnn_ok / split_chunk / workspace answers\n", answers ? "ok  " : "FAIL");

#define RN(x_, ld, xb, n_, F_, rn_, rb) mp_agnn_rnorm_f32(x_, ld, xb, n_, F_, rn_, rb, NULL)
  ACCEPT(RN(DEVF, LD, ROWS, N, F, DEVF, VEC));
  REJECT("x is NULL", RN(NULL, LD, ROWS, N, F, DEVF, VEC));
  REJECT("ld of x", RN(DEVF, F - 1, ROWS, N, F, DEVF, VEC));
  REJECT("x holds", RN(DEVF, LD, ROWS - 4, N, F, DEVF, VEC));
  REJECT("rn is NULL", RN(DEVF, LD, ROWS, N, F, NULL, VEC));
  REJECT("rn holds", RN(DEVF, LD, ROWS, N, F, DEVF, VEC - 4));
  REJECT("n = -1", RN(DEVF, LD, ROWS, -1, F, DEVF, VEC));
  REJECT("F = 0", RN(DEVF, LD, ROWS, N, 0, DEVF, VEC));
  REJECT("F <= 1024", RN(DEVF, 1025, (size_t)N * 1025 * 4, N, 1025, DEVF, VEC));

#define FWD(g_, x_, ld, xb, rn_, rb, b_, F_, o_, ldo, ob, l_, lb, ws_, wsb) \
  mp_agnn_aggregate_f32(g_, x_, ld, xb, rn_, rb, b_, F_, o_, ldo, ob, l_, lb, ws_, wsb, NULL)
  ACCEPT(FWD(&g, DEVF, LD, ROWS, DEVF, VEC, DEVF, F, DEVF, LD, ROWS, DEVF, VEC, DEV, W0));
  ACCEPT(FWD(&rows, DEVF, LD, ROWS, DEVF, VEC, DEVF, F, DEVF, LD, ROWS, DEVF, VEC, DEV, W0));
  REJECT("g is NULL", FWD(NULL, DEVF, LD, ROWS, DEVF, VEC, DEVF, F, DEVF, LD, ROWS, DEVF, VEC, DEV, W0));
  REJECT("x is NULL", FWD(&g, NULL, LD, ROWS, DEVF, VEC, DEVF, F, DEVF, LD, ROWS, DEVF, VEC, DEV, W0));
  REJECT("ld of x", FWD(&g, DEVF, F - 1, ROWS, DEVF, VEC, DEVF, F, DEVF, LD, ROWS, DEVF, VEC, DEV, W0));
  REJECT("x holds", FWD(&g, DEVF, LD, ROWS - 4, DEVF, VEC, DEVF, F, DEVF, LD, ROWS, DEVF, VEC, DEV, W0));
  REJECT("rn is NULL", FWD(&g, DEVF, LD, ROWS, NULL, VEC, DEVF, F, DEVF, LD, ROWS, DEVF, VEC, DEV, W0));
  REJECT("rn holds", FWD(&g, DEVF, LD, ROWS, DEVF, VEC - 4, DEVF, F, DEVF, LD, ROWS, DEVF, VEC, DEV, W0));
  REJECT("beta is NULL", FWD(&g, DEVF, LD, ROWS, DEVF, VEC, NULL, F, DEVF, LD, ROWS, DEVF, VEC, DEV, W0));
  REJECT("F = 0", FWD(&g, DEVF, LD, ROWS, DEVF, VEC, DEVF, 0, DEVF, LD, ROWS, DEVF, VEC, DEV, W0));
  REJECT("F <= 1024", FWD(&g, DEVF, LD, ROWS, DEVF, VEC, DEVF, 1025, DEVF, LD, ROWS, DEVF, VEC, DEV, W0));
  REJECT("out is NULL", FWD(&g, DEVF, LD, ROWS, DEVF, VEC, DEVF, F, NULL, LD, ROWS, DEVF, VEC, DEV, W0));
  REJECT("ld of out", FWD(&g, DEVF, LD, ROWS, DEVF, VEC, DEVF, F, DEVF, F - 1, ROWS, DEVF, VEC, DEV, W0));
  REJECT("out holds", FWD(&g, DEVF, LD, ROWS, DEVF, VEC, DEVF, F, DEVF, LD, ROWS - 4, DEVF, VEC, DEV, W0));
  REJECT("lse is NULL", FWD(&g, DEVF, LD, ROWS, DEVF, VEC, DEVF, F, DEVF, LD, ROWS, NULL, VEC, DEV, W0));
  REJECT("lse holds", FWD(&g, DEVF, LD, ROWS, DEVF, VEC, DEVF, F, DEVF, LD, ROWS, DEVF, VEC - 4, DEV, W0));
  REJECT("ws is NULL", FWD(&g, DEVF, LD, ROWS, DEVF, VEC, DEVF, F, DEVF, LD, ROWS, DEVF, VEC, NULL, W0));
  REJECT("ws holds", FWD(&g, DEVF, LD, ROWS, DEVF, VEC, DEVF, F, DEVF, LD, ROWS, DEVF, VEC, DEV, W0 - 1));
  {
    mp_csr b = g;
    b.rowptr = NULL;
    REJECT("rowptr is NULL", FWD(&b, DEVF, LD, ROWS, DEVF, VEC, DEVF, F, DEVF, LD, ROWS, DEVF, VEC, DEV, W0));
    b = g;
    b.col = NULL;
    REJECT("col is NULL", FWD(&b, DEVF, LD, ROWS, DEVF, VEC, DEVF, F, DEVF, LD, ROWS, DEVF, VEC, DEV, W0));
    b = g;
    b.eid = NULL;
    REJECT("eid is NULL", FWD(&b, DEVF, LD, ROWS, DEVF, VEC, DEVF, F, DEVF, LD, ROWS, DEVF, VEC, DEV, W0));
    b = g;
    b.n_rows = -1;
    REJECT("negative", FWD(&b, DEVF, LD, ROWS, DEVF, VEC, DEVF, F, DEVF, LD, ROWS, DEVF, VEC, DEV, W0));
    b = g;
    b.n_cols = (int32_t)N + 1; /* not square: a bipartite CSR, or the wrong one of a pair */
    REJECT("x serves both ends", FWD(&b, DEVF, LD, ROWS, DEVF, VEC, DEVF, F, DEVF, LD, ROWS, DEVF, VEC, DEV, W0));
    b = g;
    b.n_ids = E - 1;
    REJECT("n_ids", FWD(&b, DEVF, LD, ROWS, DEVF, VEC, DEVF, F, DEVF, LD, ROWS, DEVF, VEC, DEV, W0));
    b = g;
    b.wave_slot = NULL;
    REJECT("wave_slot is NULL", FWD(&b, DEVF, LD, ROWS, DEVF, VEC, DEVF, F, DEVF, LD, ROWS, DEVF, VEC, DEV, W0));
    b = g;
    b.n_waves = 0;
    REJECT("n_waves", FWD(&b, DEVF, LD, ROWS, DEVF, VEC, DEVF, F, DEVF, LD, ROWS, DEVF, VEC, DEV, W0));
    b = g;
    b.n_split = 73;
    REJECT("n_split", FWD(&b, DEVF, LD, ROWS, DEVF, VEC, DEVF, F, DEVF, LD, ROWS, DEVF, VEC, DEV, W0));
    b = g;
    b.split_waves = NULL;
    REJECT("split_waves is NULL", FWD(&b, DEVF, LD, ROWS, DEVF, VEC, DEVF, F, DEVF, LD, ROWS, DEVF, VEC, DEV, W0));
  }

#define DST(g_, o_, ob, l_, lb, go_, ldg, gb, a_, ab, s_, sb, u_, ldu, ub, db_, ws_, wsb)                             \
  mp_agnn_backward_dst_f32(g_, DEVF, LD, ROWS, DEVF, VEC, DEVF, F, o_, LD, ob, l_, lb, go_, ldg, gb, a_, ab, s_, sb, \
                           u_, ldu, ub, db_, ws_, wsb, NULL)
  ACCEPT(DST(&g, DEVF, ROWS, DEVF, VEC, DEVF, LD, ROWS, DEVF, EDG, DEVF, EDG, DEVF, LD, ROWS, DEVF, DEV, W1));
  REJECT("g is NULL", DST(NULL, DEVF, ROWS, DEVF, VEC, DEVF, LD, ROWS, DEVF, EDG, DEVF, EDG, DEVF, LD, ROWS, DEVF, DEV, W1));
  REJECT("out is NULL", DST(&g, NULL, ROWS, DEVF, VEC, DEVF, LD, ROWS, DEVF, EDG, DEVF, EDG, DEVF, LD, ROWS, DEVF, DEV, W1));
  REJECT("out holds", DST(&g, DEVF, ROWS - 4, DEVF, VEC, DEVF, LD, ROWS, DEVF, EDG, DEVF, EDG, DEVF, LD, ROWS, DEVF, DEV, W1));
  REJECT("lse is NULL", DST(&g, DEVF, ROWS, NULL, VEC, DEVF, LD, ROWS, DEVF, EDG, DEVF, EDG, DEVF, LD, ROWS, DEVF, DEV, W1));
  REJECT("lse holds", DST(&g, DEVF, ROWS, DEVF, VEC - 4, DEVF, LD, ROWS, DEVF, EDG, DEVF, EDG, DEVF, LD, ROWS, DEVF, DEV, W1));
  REJECT("gout is NULL", DST(&g, DEVF, ROWS, DEVF, VEC, NULL, LD, ROWS, DEVF, EDG, DEVF, EDG, DEVF, LD, ROWS, DEVF, DEV, W1));
  REJECT("ld of gout", DST(&g, DEVF, ROWS, DEVF, VEC, DEVF, F - 1, ROWS, DEVF, EDG, DEVF, EDG, DEVF, LD, ROWS, DEVF, DEV, W1));
  REJECT("gout holds", DST(&g, DEVF, ROWS, DEVF, VEC, DEVF, LD, ROWS - 4, DEVF, EDG, DEVF, EDG, DEVF, LD, ROWS, DEVF, DEV, W1));
  REJECT("alpha is NULL", DST(&g, DEVF, ROWS, DEVF, VEC, DEVF, LD, ROWS, NULL, EDG, DEVF, EDG, DEVF, LD, ROWS, DEVF, DEV, W1));
  REJECT("alpha holds", DST(&g, DEVF, ROWS, DEVF, VEC, DEVF, LD, ROWS, DEVF, EDG - 4, DEVF, EDG, DEVF, LD, ROWS, DEVF, DEV, W1));
  REJECT("bds is NULL", DST(&g, DEVF, ROWS, DEVF, VEC, DEVF, LD, ROWS, DEVF, EDG, NULL, EDG, DEVF, LD, ROWS, DEVF, DEV, W1));
  REJECT("bds holds", DST(&g, DEVF, ROWS, DEVF, VEC, DEVF, LD, ROWS, DEVF, EDG, DEVF, EDG - 4, DEVF, LD, ROWS, DEVF, DEV, W1));
  REJECT("u is NULL", DST(&g, DEVF, ROWS, DEVF, VEC, DEVF, LD, ROWS, DEVF, EDG, DEVF, EDG, NULL, LD, ROWS, DEVF, DEV, W1));
  REJECT("ld of u", DST(&g, DEVF, ROWS, DEVF, VEC, DEVF, LD, ROWS, DEVF, EDG, DEVF, EDG, DEVF, F - 1, ROWS, DEVF, DEV, W1));
  REJECT("u holds", DST(&g, DEVF, ROWS, DEVF, VEC, DEVF, LD, ROWS, DEVF, EDG, DEVF, EDG, DEVF, LD, ROWS - 4, DEVF, DEV, W1));
  REJECT("dbeta is NULL", DST(&g, DEVF, ROWS, DEVF, VEC, DEVF, LD, ROWS, DEVF, EDG, DEVF, EDG, DEVF, LD, ROWS, NULL, DEV, W1));
  REJECT("ws is NULL", DST(&g, DEVF, ROWS, DEVF, VEC, DEVF, LD, ROWS, DEVF, EDG, DEVF, EDG, DEVF, LD, ROWS, DEVF, NULL, W1));
  REJECT("ws holds", DST(&g, DEVF, ROWS, DEVF, VEC, DEVF, LD, ROWS, DEVF, EDG, DEVF, EDG, DEVF, LD, ROWS, DEVF, DEV, W0));

#define SRC(g_, go_, gb, a_, ab, s_, sb, u_, ub, dx_, lddx, dxb, ws_, wsb)                                         \
  mp_agnn_backward_src_f32(g_, DEVF, LD, ROWS, DEVF, VEC, F, go_, LD, gb, a_, ab, s_, sb, u_, LD, ub, dx_, lddx, dxb, \
                           ws_, wsb, NULL)
  ACCEPT(SRC(&g, DEVF, ROWS, DEVF, EDG, DEVF, EDG, DEVF, ROWS, DEVF, LD, ROWS, DEV, W2));
  REJECT("g is NULL", SRC(NULL, DEVF, ROWS, DEVF, EDG, DEVF, EDG, DEVF, ROWS, DEVF, LD, ROWS, DEV, W2));
  REJECT("gout is NULL", SRC(&g, NULL, ROWS, DEVF, EDG, DEVF, EDG, DEVF, ROWS, DEVF, LD, ROWS, DEV, W2));
  REJECT("gout holds", SRC(&g, DEVF, ROWS - 4, DEVF, EDG, DEVF, EDG, DEVF, ROWS, DEVF, LD, ROWS, DEV, W2));
  REJECT("alpha is NULL", SRC(&g, DEVF, ROWS, NULL, EDG, DEVF, EDG, DEVF, ROWS, DEVF, LD, ROWS, DEV, W2));
  REJECT("alpha holds", SRC(&g, DEVF, ROWS, DEVF, EDG - 4, DEVF, EDG, DEVF, ROWS, DEVF, LD, ROWS, DEV, W2));
  REJECT("bds is NULL", SRC(&g, DEVF, ROWS, DEVF, EDG, NULL, EDG, DEVF, ROWS, DEVF, LD, ROWS, DEV, W2));
  REJECT("bds holds", SRC(&g, DEVF, ROWS, DEVF, EDG, DEVF, EDG - 4, DEVF, ROWS, DEVF, LD, ROWS, DEV, W2));
  REJECT("u is NULL", SRC(&g, DEVF, ROWS, DEVF, EDG, DEVF, EDG, NULL, ROWS, DEVF, LD, ROWS, DEV, W2));
  REJECT("u holds", SRC(&g, DEVF, ROWS, DEVF, EDG, DEVF, EDG, DEVF, ROWS - 4, DEVF, LD, ROWS, DEV, W2));
  REJECT("dx is NULL", SRC(&g, DEVF, ROWS, DEVF, EDG, DEVF, EDG, DEVF, ROWS, NULL, LD, ROWS, DEV, W2));
  REJECT("ld of dx", SRC(&g, DEVF, ROWS, DEVF, EDG, DEVF, EDG, DEVF, ROWS, DEVF, F - 1, ROWS, DEV, W2));
  REJECT("dx holds", SRC(&g, DEVF, ROWS, DEVF, EDG, DEVF, EDG, DEVF, ROWS, DEVF, LD, ROWS - 4, DEV, W2));
  REJECT("ws is NULL", SRC(&g, DEVF, ROWS, DEVF, EDG, DEVF, EDG, DEVF, ROWS, DEVF, LD, ROWS, NULL, W2));
  REJECT("ws holds", SRC(&g, DEVF, ROWS, DEVF, EDG, DEVF, EDG, DEVF, ROWS, DEVF, LD, ROWS, DEV, W2 - 1));

  printf("abi_reject_agnn: %d cases, %d failures\n", n_cases, n_fail);
  return n_fail ? 1 : 0;
}
