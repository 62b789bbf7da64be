/*
 * abi_reject_nnconv.c -- argument / extent rejection harness for the NNConv
 * entry points of include/mi355_mp.h (mp_nnconv_ok,
 * mp_nnconv_aggregate_bins_f32, mp_nnconv_aggregate_gather_f32,
 * mp_nnconv_edge_grad_f32).
 *
 * Built against the host-only AddressSanitizer build of the library
 * (`make -C pytorch_geometric-1_amd/csrc asan_nnconv`) and run as a plain
 * program on a machine with no GPU by tests/test_nnconv_host.py.  Every case
 * calls one entry point with one bad argument and expects -MP_ERR_ARG and an
 * error text naming the problem -- no launch, no device access, no host memory
 * error (ASAN aborts the run on one).  ACCEPT cases pass every check (the call
 * then fails at its first HIP call, -MP_ERR_HIP, as there is no GPU): the
 * boundary is the documented one, not a looser one.
 * Output: one line per case, then "abi_reject_nnconv: N cases, M failures".
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "mi355_mp.h"

static int n_cases = 0, n_fail = 0;

#define DEV ((void*)(uintptr_t)0x7f0000000000ull) /* fake device pointer, never dereferenced */
#define DEVF ((float*)DEV)
#define DEVI ((int32_t*)DEV)
#define DEVL ((int64_t*)DEV)

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

static mp_csr graph(int64_t n_rows, int64_t n_edges, int32_t n_cols) {
  mp_csr g;
  memset(&g, 0, sizeof g);
  g.rowptr = DEVI;
  g.col = DEVI;
  g.eid = DEVI;
  g.n_rows = n_rows;
  g.n_edges = n_edges;
  g.n_cols = n_cols;
  return g;
}

int main(void) {
  const int64_t N = 257, E = 3000;
  const int H = 25, C = 33, Q = (25 + 1) * 33;
  mp_csr g = graph(N, E, (int32_t)N);

  /* mp_nnconv_ok: the three example shapes, the limits on each side */
  ++n_cases;
  if (!(mp_nnconv_ok(25, 1, 32) == 1 && mp_nnconv_ok(25, 32, 64) == 1 && mp_nnconv_ok(128, 64, 64) == 1 &&
        mp_nnconv_ok(1, 1, 1) == 1 && mp_nnconv_ok(0, 1, 1) == 0 && mp_nnconv_ok(5, 0, 1) == 0 &&
        mp_nnconv_ok(5, 1, 0) == 0 && mp_nnconv_ok(-1, 4, 4) == 0 && mp_nnconv_ok(1023, 1024, 1) == 1 &&
        mp_nnconv_ok(1024, 1024, 1) == 0 && mp_nnconv_ok(1024, 1, 1024) == 0 && mp_nnconv_ok(1023, 1, 1024) == 1)) {
    printf("FAIL mp_nnconv_ok limits\n");
    ++n_fail;
  } else {
    printf("ok   mp_nnconv_ok limits\n");
  }

  /* bins form */
  REJECT("g is NULL", mp_nnconv_aggregate_bins_f32(NULL, DEVF, E, H, H, DEVF, C, C, NULL, DEVF, Q, NULL));
  REJECT("h is NULL", mp_nnconv_aggregate_bins_f32(&g, NULL, E, H, H, DEVF, C, C, NULL, DEVF, Q, NULL));
  REJECT("x is NULL", mp_nnconv_aggregate_bins_f32(&g, DEVF, E, H, H, NULL, C, C, NULL, DEVF, Q, NULL));
  REJECT("out is NULL", mp_nnconv_aggregate_bins_f32(&g, DEVF, E, H, H, DEVF, C, C, NULL, NULL, Q, NULL));
  REJECT("n_h_edges", mp_nnconv_aggregate_bins_f32(&g, DEVF, E - 1, H, H, DEVF, C, C, NULL, DEVF, Q, NULL));
  REJECT("ldh", mp_nnconv_aggregate_bins_f32(&g, DEVF, E, H - 1, H, DEVF, C, C, NULL, DEVF, Q, NULL));
  REJECT("ldx", mp_nnconv_aggregate_bins_f32(&g, DEVF, E, H, H, DEVF, C - 1, C, NULL, DEVF, Q, NULL));
  REJECT("ldo", mp_nnconv_aggregate_bins_f32(&g, DEVF, E, H, H, DEVF, C, C, NULL, DEVF, Q - 1, NULL));
  REJECT("H = 0", mp_nnconv_aggregate_bins_f32(&g, DEVF, E, H, 0, DEVF, C, C, NULL, DEVF, Q, NULL));
  REJECT("Cin = 0", mp_nnconv_aggregate_bins_f32(&g, DEVF, E, H, H, DEVF, C, 0, NULL, DEVF, Q, NULL));
  REJECT("above the limit", mp_nnconv_aggregate_bins_f32(&g, DEVF, E, 1024, 1024, DEVF, 1024, 1024, NULL, DEVF,
                                                         1025 * 1024, NULL));
  {
    mp_csr b = g;
    b.col = NULL;
    REJECT("col", mp_nnconv_aggregate_bins_f32(&b, DEVF, E, H, H, DEVF, C, C, NULL, DEVF, Q, NULL));
    b = g;
    b.eid = NULL;
    REJECT("eid", mp_nnconv_aggregate_bins_f32(&b, DEVF, E, H, H, DEVF, C, C, NULL, DEVF, Q, NULL));
    b = g;
    b.rowptr = NULL;
    REJECT("rowptr", mp_nnconv_aggregate_bins_f32(&b, DEVF, E, H, H, DEVF, C, C, NULL, DEVF, Q, NULL));
    b = g;
    b.n_cols = 0;
    REJECT("n_cols", mp_nnconv_aggregate_bins_f32(&b, DEVF, E, H, H, DEVF, C, C, NULL, DEVF, Q, NULL));
    b = g;
    b.n_ids = E + 5; /* the slots are a subset of E + 5 edges: h must cover them all */
    REJECT("n_h_edges", mp_nnconv_aggregate_bins_f32(&b, DEVF, E, H, H, DEVF, C, C, NULL, DEVF, Q, NULL));
    ACCEPT(mp_nnconv_aggregate_bins_f32(&b, DEVF, E + 5, H, H, DEVF, C, C, NULL, DEVF, Q, NULL));
  }
  ACCEPT(mp_nnconv_aggregate_bins_f32(&g, DEVF, E, H, H, DEVF, C, C, DEVF, DEVF, Q, NULL));
  ACCEPT(mp_nnconv_aggregate_bins_f32(&g, DEVF, E, 1, 1, DEVF, 1, 1, NULL, DEVF, 2, NULL));
  ACCEPT(mp_nnconv_aggregate_bins_f32(&g, DEVF, E, 1023, 1023, DEVF, 1024, 1024, NULL, DEVF, 1024 * 1024, NULL));

  /* gather form: y is [n_cols, H + 1, F] */
  REJECT("g is NULL", mp_nnconv_aggregate_gather_f32(NULL, DEVF, E, H, H, DEVF, Q, C, NULL, NULL, DEVF, C, NULL));
  REJECT("h is NULL", mp_nnconv_aggregate_gather_f32(&g, NULL, E, H, H, DEVF, Q, C, NULL, NULL, DEVF, C, NULL));
  REJECT("y is NULL", mp_nnconv_aggregate_gather_f32(&g, DEVF, E, H, H, NULL, Q, C, NULL, NULL, DEVF, C, NULL));
  REJECT("out is NULL", mp_nnconv_aggregate_gather_f32(&g, DEVF, E, H, H, DEVF, Q, C, NULL, NULL, NULL, C, NULL));
  REJECT("n_h_edges", mp_nnconv_aggregate_gather_f32(&g, DEVF, 0, H, H, DEVF, Q, C, NULL, NULL, DEVF, C, NULL));
  REJECT("ldh", mp_nnconv_aggregate_gather_f32(&g, DEVF, E, H - 1, H, DEVF, Q, C, NULL, NULL, DEVF, C, NULL));
  REJECT("ldy", mp_nnconv_aggregate_gather_f32(&g, DEVF, E, H, H, DEVF, Q - 1, C, NULL, NULL, DEVF, C, NULL));
  REJECT("ldo", mp_nnconv_aggregate_gather_f32(&g, DEVF, E, H, H, DEVF, Q, C, NULL, NULL, DEVF, C - 1, NULL));
  REJECT("H = 0", mp_nnconv_aggregate_gather_f32(&g, DEVF, E, H, 0, DEVF, Q, C, NULL, NULL, DEVF, C, NULL));
  REJECT("F = 0", mp_nnconv_aggregate_gather_f32(&g, DEVF, E, H, H, DEVF, Q, 0, NULL, NULL, DEVF, C, NULL));
  REJECT("above the limit", mp_nnconv_aggregate_gather_f32(&g, DEVF, E, 1024, 1024, DEVF, 1025 * 1024, 1024, NULL,
                                                           NULL, DEVF, 1024, NULL));
  ACCEPT(mp_nnconv_aggregate_gather_f32(&g, DEVF, E, H, H, DEVF, Q, C, DEVF, DEVF, DEVF, C, NULL));
  ACCEPT(mp_nnconv_aggregate_gather_f32(&g, DEVF, E, H + 3, H, DEVF, Q + 1, C, NULL, NULL, DEVF, C + 1, NULL));

  /* edge grad: dh [E, lddh] travels with its extent */
  const size_t need = ((size_t)(E - 1) * H + H) * 4;
  REJECT("rows is NULL", mp_nnconv_edge_grad_f32(NULL, DEVL, E, DEVF, Q, DEVF, C, H, C, DEVF, H, need, NULL));
  REJECT("cols is NULL", mp_nnconv_edge_grad_f32(DEVL, NULL, E, DEVF, Q, DEVF, C, H, C, DEVF, H, need, NULL));
  REJECT("dz is NULL", mp_nnconv_edge_grad_f32(DEVL, DEVL, E, NULL, Q, DEVF, C, H, C, DEVF, H, need, NULL));
  REJECT("x is NULL", mp_nnconv_edge_grad_f32(DEVL, DEVL, E, DEVF, Q, NULL, C, H, C, DEVF, H, need, NULL));
  REJECT("dh is NULL", mp_nnconv_edge_grad_f32(DEVL, DEVL, E, DEVF, Q, DEVF, C, H, C, NULL, H, need, NULL));
  REJECT("n_edges", mp_nnconv_edge_grad_f32(DEVL, DEVL, -1, DEVF, Q, DEVF, C, H, C, DEVF, H, need, NULL));
  REJECT("lddz", mp_nnconv_edge_grad_f32(DEVL, DEVL, E, DEVF, Q - 1, DEVF, C, H, C, DEVF, H, need, NULL));
  REJECT("ldx", mp_nnconv_edge_grad_f32(DEVL, DEVL, E, DEVF, Q, DEVF, C - 1, H, C, DEVF, H, need, NULL));
  REJECT("lddh", mp_nnconv_edge_grad_f32(DEVL, DEVL, E, DEVF, Q, DEVF, C, H, C, DEVF, H - 1, need, NULL));
  REJECT("dh holds", mp_nnconv_edge_grad_f32(DEVL, DEVL, E, DEVF, Q, DEVF, C, H, C, DEVF, H, need - 1, NULL));
  REJECT("dh holds", mp_nnconv_edge_grad_f32(DEVL, DEVL, E, DEVF, Q, DEVF, C, H, C, DEVF, H, 0, NULL));
  REJECT("dh holds", mp_nnconv_edge_grad_f32(DEVL, DEVL, E, DEVF, Q, DEVF, C, H, C, DEVF, H + 2, need, NULL));
  REJECT("H = 0", mp_nnconv_edge_grad_f32(DEVL, DEVL, E, DEVF, Q, DEVF, C, 0, C, DEVF, H, need, NULL));
  REJECT("Cin = 0", mp_nnconv_edge_grad_f32(DEVL, DEVL, E, DEVF, Q, DEVF, C, H, 0, DEVF, H, need, NULL));
  ACCEPT(mp_nnconv_edge_grad_f32(DEVL, DEVL, E, DEVF, Q, DEVF, C, H, C, DEVF, H, need, NULL));
  ACCEPT(mp_nnconv_edge_grad_f32(DEVL, DEVL, E, DEVF, Q, DEVF, C, H, C, DEVF, H + 2,
                                 ((size_t)(E - 1) * (H + 2) + H) * 4, NULL));
  ACCEPT(mp_nnconv_edge_grad_f32(NULL, NULL, 0, NULL, Q, NULL, C, H, C, NULL, H, 0, NULL)); /* no edges: nothing to do */

  printf("abi_reject_nnconv: %d cases, %d failures\n", n_cases, n_fail);
  return n_fail ? 1 : 0;
}
