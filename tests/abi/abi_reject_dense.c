/*
 * abi_reject_dense.c -- argument / extent rejection harness for the dense
 * family's entry points of include/mi355_mp.h (mp_diff_pool_path,
 * mp_diff_pool_workspace, mp_diff_pool_bwd_workspace, mp_dense_diff_pool_f32,
 * mp_dense_diff_pool_bwd_f32, mp_dense_mean_agg_f32, mp_to_dense_batch_f32,
 * mp_to_dense_batch_bwd_f32, mp_to_dense_adj_workspace, mp_to_dense_adj_f32).
 *
 * Built against the host-only AddressSanitizer build of the library
 * (`make -C pytorch_geometric-1_amd/csrc asan_dense`) and run as a plain program
 * on a machine with no GPU by tests/test_dense_host.py.  Every case calls one
 * entry point with one bad argument and expects -MP_ERR_ARG and an error text
 * naming the problem -- no launch, no device access, no host memory error (ASAN
 * aborts the run on one).  ACCEPT cases pass every check (the call then fails at
 * its first HIP call, -MP_ERR_HIP, as there is no GPU): the boundary is the
 * documented one, not a looser one.
 * Output: one line per case, then "abi_reject_dense: N cases, M failures".
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "mi355_mp.h"

static int n_cases = 0, n_fail = 0;

#define DEV ((void*)(uintptr_t)0x7f0000000000ull) /* fake device pointer, never dereferenced */
#define DEVF ((float*)DEV)
#define DEVL ((int64_t*)DEV)
#define DEVB ((uint8_t*)DEV)
#define ODD ((float*)(uintptr_t)0x7f0000000002ull)  /* not 4-byte aligned */
#define ODDL ((int64_t*)(uintptr_t)0x7f0000000004ull) /* not 8-byte aligned */
#define ODDW ((void*)(uintptr_t)0x7f0000000008ull)  /* not 16-byte aligned */

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
  enum { B = 3, N = 200, C = 33, F = 65, NS = 50, CS = 5 };
  const size_t WS = mp_diff_pool_workspace(B, N, C, F), WS0 = mp_diff_pool_workspace(B, NS, CS, F);
  const size_t WB = mp_diff_pool_bwd_workspace(B, N, C, F);
  const size_t OB = (size_t)B * C * F * 4, OAB = (size_t)B * C * C * 4, LB = 16, PB = (size_t)B * N * C * 4;
  const size_t XB = (size_t)B * N * F * 4;

  /* the path query: both forms, non-decreasing in N, the argument check */
  ++n_cases;
  {
    int ok = mp_diff_pool_path(1, 1, 1) == 0 && mp_diff_pool_path(100, 10, 192) == 0 &&
             mp_diff_pool_path(129, 1, 1) == 1 && mp_diff_pool_path(1000, 100, 64) == 1 &&
             mp_diff_pool_path(NS, CS, F) == 0 && mp_diff_pool_path(N, C, F) == 1 &&
             mp_diff_pool_path(0, 1, 1) == -MP_ERR_ARG && mp_diff_pool_path(1, 0, 1) == -MP_ERR_ARG &&
             mp_diff_pool_path(1, 1, 0) == -MP_ERR_ARG && mp_diff_pool_path(-4, 3, 3) == -MP_ERR_ARG;
    int64_t prev = 0;
    for (int64_t n = 1; n < 400 && ok; ++n) {
      const int64_t p = mp_diff_pool_path(n, C, F);
      ok = p >= prev && p <= 1;
      prev = p;
    }
    printf("%s mp_diff_pool_path\n", ok ? "ok  " : "FAIL");
    if (!ok) ++n_fail;
  }
  /* the workspaces: form 1 holds its tile partials and row entropies, form 0 the per-graph pair alone */
  ++n_cases;
  if (!(WS >= ((size_t)B * 16 + (size_t)B * N) * 4 && WS0 <= 4 * 256 + 256 && WS0 >= 256 &&
        WB >= (size_t)B * C * C * 4 && mp_diff_pool_workspace(0, 0, 0, 0) >= 256 &&
        mp_to_dense_adj_workspace(B, N, 0) <= 512 && mp_to_dense_adj_workspace(B, N, 2) >= (size_t)B * N * N * 8)) {
    printf("FAIL workspaces\n");
    ++n_fail;
  } else {
    printf("ok   workspaces\n");
  }

#define FWD(x, adj, s, m, b, n, c, f, o, ob, oa, oab, l, lb, p, pb, t, tb, v, vb, ws, wsb) \
  mp_dense_diff_pool_f32(x, adj, s, m, b, n, c, f, o, ob, oa, oab, l, lb, p, pb, t, tb, v, vb, ws, wsb, NULL)

  REJECT("x is NULL", FWD(NULL, DEVF, DEVF, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("adj is NULL", FWD(DEVF, NULL, DEVF, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("s is NULL", FWD(DEVF, DEVF, NULL, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("out is NULL", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, F, NULL, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("out_adj is NULL", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, F, DEVF, OB, NULL, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("loss is NULL", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB, NULL, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("P is NULL", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, NULL, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("T is NULL", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, NULL, PB, DEVF, PB, DEV, WS));
  REJECT("V is NULL", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, NULL, PB, DEV, WS));
  REJECT("ws is NULL", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, NULL, WS));
  REJECT("x is not 4-byte aligned", FWD(ODD, DEVF, DEVF, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("adj is not 4-byte aligned", FWD(DEVF, ODD, DEVF, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("s is not 4-byte aligned", FWD(DEVF, DEVF, ODD, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("out is not 4-byte aligned", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, F, ODD, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("out_adj is not 4-byte aligned", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, F, DEVF, OB, ODD, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("loss is not 4-byte aligned", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB, ODD, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("P is not 4-byte aligned", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, ODD, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("T is not 4-byte aligned", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, ODD, PB, DEVF, PB, DEV, WS));
  REJECT("V is not 4-byte aligned", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, ODD, PB, DEV, WS));
  REJECT("ws is not 16-byte aligned", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, ODDW, WS));
  REJECT("B = 0", FWD(DEVF, DEVF, DEVF, DEVB, 0, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("B = -2", FWD(DEVF, DEVF, DEVF, DEVB, -2, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("N = 0", FWD(DEVF, DEVF, DEVF, DEVB, B, 0, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("N = -1", FWD(DEVF, DEVF, DEVF, DEVB, B, -1, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("C = 0", FWD(DEVF, DEVF, DEVF, DEVB, B, N, 0, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("C = -3", FWD(DEVF, DEVF, DEVF, DEVB, B, N, -3, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("F = 0", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, 0, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("F = -1", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, -1, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("grid too large", FWD(DEVF, DEVF, DEVF, DEVB, 70000, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("grid too large", FWD(DEVF, DEVF, DEVF, DEVB, 64, (int64_t)1 << 16, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("out holds", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, F, DEVF, OB - 1, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("out_adj holds", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB - 1, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("loss holds", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB - 1, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("P holds", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB - 1, DEVF, PB, DEVF, PB, DEV, WS));
  REJECT("T holds", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB - 1, DEVF, PB, DEV, WS));
  REJECT("V holds", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB - 1, DEV, WS));
  REJECT("ws holds", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS - 1));
  REJECT("ws holds", FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, 0));
  /* form 0's workspace, one byte short, at its own shape */
  REJECT("ws holds", FWD(DEVF, DEVF, DEVF, NULL, B, NS, CS, F, DEVF, (size_t)B * CS * F * 4, DEVF, (size_t)B * CS * CS * 4, DEVF, LB, DEVF,
                         (size_t)B * NS * CS * 4, DEVF, (size_t)B * NS * CS * 4, DEVF, (size_t)B * NS * CS * 4, DEV, WS0 - 1));
  ACCEPT(FWD(DEVF, DEVF, DEVF, DEVB, B, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  ACCEPT(FWD(DEVF, DEVF, DEVF, NULL, B, N, C, F, DEVF, OB, DEVF, OAB, DEVF, LB, DEVF, PB, DEVF, PB, DEVF, PB, DEV, WS));
  ACCEPT(FWD(DEVF, DEVF, DEVF, NULL, B, NS, CS, F, DEVF, (size_t)B * CS * F * 4, DEVF, (size_t)B * CS * CS * 4, DEVF, LB, DEVF,
             (size_t)B * NS * CS * 4, DEVF, (size_t)B * NS * CS * 4, DEVF, (size_t)B * NS * CS * 4, DEV, WS0));
  ACCEPT(FWD(DEVF, DEVF, DEVF, NULL, 1, 1, 1, 1, DEVF, 4, DEVF, 4, DEVF, LB, DEVF, 4, DEVF, 4, DEVF, 4, DEV, mp_diff_pool_workspace(1, 1, 1, 1)));

#define BWD(go, goa, gl, x, p, t, v, l, b, n, c, f, dx, dxb, ds, dsb, ws, wsb) \
  mp_dense_diff_pool_bwd_f32(go, goa, gl, x, p, t, v, l, b, n, c, f, dx, dxb, ds, dsb, ws, wsb, NULL)

  REJECT("x is NULL", BWD(DEVF, DEVF, DEVF, NULL, DEVF, DEVF, DEVF, DEVF, B, N, C, F, DEVF, XB, DEVF, PB, DEV, WB));
  REJECT("P is NULL", BWD(DEVF, DEVF, DEVF, DEVF, NULL, DEVF, DEVF, DEVF, B, N, C, F, DEVF, XB, DEVF, PB, DEV, WB));
  REJECT("T is NULL", BWD(DEVF, DEVF, DEVF, DEVF, DEVF, NULL, DEVF, DEVF, B, N, C, F, DEVF, XB, DEVF, PB, DEV, WB));
  REJECT("V is NULL", BWD(DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, NULL, DEVF, B, N, C, F, DEVF, XB, DEVF, PB, DEV, WB));
  REJECT("loss is NULL", BWD(DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, NULL, B, N, C, F, DEVF, XB, DEVF, PB, DEV, WB));
  REJECT("ds is NULL", BWD(DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, B, N, C, F, DEVF, XB, NULL, PB, DEV, WB));
  REJECT("ws is NULL", BWD(DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, B, N, C, F, DEVF, XB, DEVF, PB, NULL, WB));
  REJECT("g_out is not 4-byte aligned", BWD(ODD, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, B, N, C, F, DEVF, XB, DEVF, PB, DEV, WB));
  REJECT("g_oa is not 4-byte aligned", BWD(DEVF, ODD, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, B, N, C, F, DEVF, XB, DEVF, PB, DEV, WB));
  REJECT("g_loss is not 4-byte aligned", BWD(DEVF, DEVF, ODD, DEVF, DEVF, DEVF, DEVF, DEVF, B, N, C, F, DEVF, XB, DEVF, PB, DEV, WB));
  REJECT("x is not 4-byte aligned", BWD(DEVF, DEVF, DEVF, ODD, DEVF, DEVF, DEVF, DEVF, B, N, C, F, DEVF, XB, DEVF, PB, DEV, WB));
  REJECT("P is not 4-byte aligned", BWD(DEVF, DEVF, DEVF, DEVF, ODD, DEVF, DEVF, DEVF, B, N, C, F, DEVF, XB, DEVF, PB, DEV, WB));
  REJECT("T is not 4-byte aligned", BWD(DEVF, DEVF, DEVF, DEVF, DEVF, ODD, DEVF, DEVF, B, N, C, F, DEVF, XB, DEVF, PB, DEV, WB));
  REJECT("V is not 4-byte aligned", BWD(DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, ODD, DEVF, B, N, C, F, DEVF, XB, DEVF, PB, DEV, WB));
  REJECT("loss is not 4-byte aligned", BWD(DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, ODD, B, N, C, F, DEVF, XB, DEVF, PB, DEV, WB));
  REJECT("dx is not 4-byte aligned", BWD(DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, B, N, C, F, ODD, XB, DEVF, PB, DEV, WB));
  REJECT("ds is not 4-byte aligned", BWD(DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, B, N, C, F, DEVF, XB, ODD, PB, DEV, WB));
  REJECT("ws is not 16-byte aligned", BWD(DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, B, N, C, F, DEVF, XB, DEVF, PB, ODDW, WB));
  REJECT("B = 0", BWD(DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, 0, N, C, F, DEVF, XB, DEVF, PB, DEV, WB));
  REJECT("N = -7", BWD(DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, B, -7, C, F, DEVF, XB, DEVF, PB, DEV, WB));
  REJECT("C = 0", BWD(DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, B, N, 0, F, DEVF, XB, DEVF, PB, DEV, WB));
  REJECT("F = 0", BWD(DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, B, N, C, 0, DEVF, XB, DEVF, PB, DEV, WB));
  REJECT("dx holds", BWD(DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, B, N, C, F, DEVF, XB - 1, DEVF, PB, DEV, WB));
  REJECT("ds holds", BWD(DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, B, N, C, F, DEVF, XB, DEVF, PB - 1, DEV, WB));
  REJECT("ws holds", BWD(DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, B, N, C, F, DEVF, XB, DEVF, PB, DEV, WB - 1));
  ACCEPT(BWD(DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, DEVF, B, N, C, F, DEVF, XB, DEVF, PB, DEV, WB));
  ACCEPT(BWD(NULL, NULL, NULL, DEVF, DEVF, DEVF, DEVF, DEVF, B, N, C, F, NULL, 0, DEVF, PB, DEV, WB));

#define AGG(adj, x, b, n, f, loop, tr, din, o, ob, dout, db) mp_dense_mean_agg_f32(adj, x, b, n, f, loop, tr, din, o, ob, dout, db, NULL)
  {
    const size_t DB = (size_t)B * N * 4;
    REJECT("adj is NULL", AGG(NULL, DEVF, B, N, F, 1, 0, NULL, DEVF, XB, DEVF, DB));
    REJECT("x is NULL", AGG(DEVF, NULL, B, N, F, 1, 0, NULL, DEVF, XB, DEVF, DB));
    REJECT("out is NULL", AGG(DEVF, DEVF, B, N, F, 1, 0, NULL, NULL, XB, DEVF, DB));
    REJECT("deg_out is NULL", AGG(DEVF, DEVF, B, N, F, 1, 0, NULL, DEVF, XB, NULL, DB));
    REJECT("deg_in is NULL", AGG(DEVF, DEVF, B, N, F, 1, 1, NULL, DEVF, XB, NULL, 0));
    REJECT("deg_in belongs", AGG(DEVF, DEVF, B, N, F, 1, 0, DEVF, DEVF, XB, DEVF, DB));
    REJECT("deg_out is the forward", AGG(DEVF, DEVF, B, N, F, 1, 1, DEVF, DEVF, XB, DEVF, DB));
    REJECT("adj is not 4-byte aligned", AGG(ODD, DEVF, B, N, F, 1, 0, NULL, DEVF, XB, DEVF, DB));
    REJECT("x is not 4-byte aligned", AGG(DEVF, ODD, B, N, F, 1, 0, NULL, DEVF, XB, DEVF, DB));
    REJECT("out is not 4-byte aligned", AGG(DEVF, DEVF, B, N, F, 1, 0, NULL, ODD, XB, DEVF, DB));
    REJECT("deg_out is not 4-byte aligned", AGG(DEVF, DEVF, B, N, F, 1, 0, NULL, DEVF, XB, ODD, DB));
    REJECT("deg_in is not 4-byte aligned", AGG(DEVF, DEVF, B, N, F, 1, 1, ODD, DEVF, XB, NULL, 0));
    REJECT("B = 0", AGG(DEVF, DEVF, 0, N, F, 1, 0, NULL, DEVF, XB, DEVF, DB));
    REJECT("N = 0", AGG(DEVF, DEVF, B, 0, F, 1, 0, NULL, DEVF, XB, DEVF, DB));
    REJECT("F = -1", AGG(DEVF, DEVF, B, N, -1, 1, 0, NULL, DEVF, XB, DEVF, DB));
    REJECT("add_loop = 2", AGG(DEVF, DEVF, B, N, F, 2, 0, NULL, DEVF, XB, DEVF, DB));
    REJECT("transpose = -1", AGG(DEVF, DEVF, B, N, F, 1, -1, NULL, DEVF, XB, DEVF, DB));
    REJECT("out holds", AGG(DEVF, DEVF, B, N, F, 1, 0, NULL, DEVF, XB - 1, DEVF, DB));
    REJECT("deg_out holds", AGG(DEVF, DEVF, B, N, F, 1, 0, NULL, DEVF, XB, DEVF, DB - 1));
    REJECT("out holds", AGG(DEVF, DEVF, B, N, F, 0, 1, DEVF, DEVF, XB - 1, NULL, 0));
    ACCEPT(AGG(DEVF, DEVF, B, N, F, 1, 0, NULL, DEVF, XB, DEVF, DB));
    ACCEPT(AGG(DEVF, DEVF, B, N, F, 0, 1, DEVF, DEVF, XB, NULL, 0));
  }

  {
    enum { NN = 40, G = 4, NM = 17, E = 90, D = 3 };
    const size_t DOB = (size_t)G * NM * F * 4, MB = (size_t)G * NM, DXB = (size_t)NN * F * 4;
#define TDB(x, n, f, st, g, nm, o, ob, m, mb) mp_to_dense_batch_f32(x, n, f, st, g, nm, 0.5f, o, ob, m, mb, NULL)
    REJECT("x is NULL", TDB(NULL, NN, F, DEVL, G, NM, DEVF, DOB, DEVB, MB));
    REJECT("starts is NULL", TDB(DEVF, NN, F, NULL, G, NM, DEVF, DOB, DEVB, MB));
    REJECT("out is NULL", TDB(DEVF, NN, F, DEVL, G, NM, NULL, DOB, DEVB, MB));
    REJECT("mask is NULL", TDB(DEVF, NN, F, DEVL, G, NM, DEVF, DOB, NULL, MB));
    REJECT("x is not 4-byte aligned", TDB(ODD, NN, F, DEVL, G, NM, DEVF, DOB, DEVB, MB));
    REJECT("starts is not 8-byte aligned", TDB(DEVF, NN, F, ODDL, G, NM, DEVF, DOB, DEVB, MB));
    REJECT("out is not 4-byte aligned", TDB(DEVF, NN, F, DEVL, G, NM, ODD, DOB, DEVB, MB));
    REJECT("n = -1", TDB(DEVF, -1, F, DEVL, G, NM, DEVF, DOB, DEVB, MB));
    REJECT("F = 0", TDB(DEVF, NN, 0, DEVL, G, NM, DEVF, DOB, DEVB, MB));
    REJECT("B = -1", TDB(DEVF, NN, F, DEVL, -1, NM, DEVF, DOB, DEVB, MB));
    REJECT("Nmax = -1", TDB(DEVF, NN, F, DEVL, G, -1, DEVF, DOB, DEVB, MB));
    REJECT("out holds", TDB(DEVF, NN, F, DEVL, G, NM, DEVF, DOB - 1, DEVB, MB));
    REJECT("mask holds", TDB(DEVF, NN, F, DEVL, G, NM, DEVF, DOB, DEVB, MB - 1));
    ACCEPT(TDB(DEVF, NN, F, DEVL, G, NM, DEVF, DOB, DEVB, MB));
    ACCEPT(TDB(NULL, 0, F, DEVL, G, 0, NULL, 0, NULL, 0));   /* graphs without nodes: nothing to write */
    ACCEPT(TDB(NULL, 0, F, DEVL, 0, 0, NULL, 0, NULL, 0));
#define TDG(g, n, f, st, b, nm, dx, dxb) mp_to_dense_batch_bwd_f32(g, n, f, st, b, nm, dx, dxb, NULL)
    REJECT("g is NULL", TDG(NULL, NN, F, DEVL, G, NM, DEVF, DXB));
    REJECT("starts is NULL", TDG(DEVF, NN, F, NULL, G, NM, DEVF, DXB));
    REJECT("dx is NULL", TDG(DEVF, NN, F, DEVL, G, NM, NULL, DXB));
    REJECT("g is not 4-byte aligned", TDG(ODD, NN, F, DEVL, G, NM, DEVF, DXB));
    REJECT("dx is not 4-byte aligned", TDG(DEVF, NN, F, DEVL, G, NM, ODD, DXB));
    REJECT("F = -2", TDG(DEVF, NN, -2, DEVL, G, NM, DEVF, DXB));
    REJECT("dx holds", TDG(DEVF, NN, F, DEVL, G, NM, DEVF, DXB - 1));
    ACCEPT(TDG(DEVF, NN, F, DEVL, G, NM, DEVF, DXB));

    const size_t AW0 = mp_to_dense_adj_workspace(G, NM, 0), AWD = mp_to_dense_adj_workspace(G, NM, D);
    const size_t AB0 = (size_t)G * NM * NM * 4, ABD = AB0 * D;
#define TDA(r, c, e, at, d, bt, n, st, g, nm, o, ob, ws, wsb) mp_to_dense_adj_f32(r, c, e, at, d, bt, n, st, g, nm, o, ob, ws, wsb, NULL)
    REJECT("row is NULL", TDA(NULL, DEVL, E, NULL, 0, DEVL, NN, DEVL, G, NM, DEVF, AB0, DEV, AW0));
    REJECT("col is NULL", TDA(DEVL, NULL, E, NULL, 0, DEVL, NN, DEVL, G, NM, DEVF, AB0, DEV, AW0));
    REJECT("starts is NULL", TDA(DEVL, DEVL, E, NULL, 0, DEVL, NN, NULL, G, NM, DEVF, AB0, DEV, AW0));
    REJECT("out is NULL", TDA(DEVL, DEVL, E, NULL, 0, DEVL, NN, DEVL, G, NM, NULL, AB0, DEV, AW0));
    REJECT("ws is NULL", TDA(DEVL, DEVL, E, NULL, 0, DEVL, NN, DEVL, G, NM, DEVF, AB0, NULL, AW0));
    REJECT("batch is NULL", TDA(DEVL, DEVL, E, NULL, 0, NULL, NN, DEVL, G, NM, DEVF, AB0, DEV, AW0));
    REJECT("row is not 8-byte aligned", TDA(ODDL, DEVL, E, NULL, 0, DEVL, NN, DEVL, G, NM, DEVF, AB0, DEV, AW0));
    REJECT("col is not 8-byte aligned", TDA(DEVL, ODDL, E, NULL, 0, DEVL, NN, DEVL, G, NM, DEVF, AB0, DEV, AW0));
    REJECT("batch is not 8-byte aligned", TDA(DEVL, DEVL, E, NULL, 0, ODDL, NN, DEVL, G, NM, DEVF, AB0, DEV, AW0));
    REJECT("starts is not 8-byte aligned", TDA(DEVL, DEVL, E, NULL, 0, DEVL, NN, ODDL, G, NM, DEVF, AB0, DEV, AW0));
    REJECT("out is not 4-byte aligned", TDA(DEVL, DEVL, E, NULL, 0, DEVL, NN, DEVL, G, NM, ODD, AB0, DEV, AW0));
    REJECT("edge_attr is not 4-byte aligned", TDA(DEVL, DEVL, E, ODD, D, DEVL, NN, DEVL, G, NM, DEVF, ABD, DEV, AWD));
    REJECT("ws is not 16-byte aligned", TDA(DEVL, DEVL, E, NULL, 0, DEVL, NN, DEVL, G, NM, DEVF, AB0, ODDW, AW0));
    REJECT("edge_attr NULL with D = 3", TDA(DEVL, DEVL, E, NULL, D, DEVL, NN, DEVL, G, NM, DEVF, ABD, DEV, AWD));
    REJECT("edge_attr given with D = 0", TDA(DEVL, DEVL, E, DEVF, 0, DEVL, NN, DEVL, G, NM, DEVF, AB0, DEV, AW0));
    REJECT("E = -1", TDA(DEVL, DEVL, -1, NULL, 0, DEVL, NN, DEVL, G, NM, DEVF, AB0, DEV, AW0));
    REJECT("D = -1", TDA(DEVL, DEVL, E, NULL, -1, DEVL, NN, DEVL, G, NM, DEVF, AB0, DEV, AW0));
    REJECT("n = -1", TDA(DEVL, DEVL, E, NULL, 0, DEVL, -1, DEVL, G, NM, DEVF, AB0, DEV, AW0));
    REJECT("B = -1", TDA(DEVL, DEVL, E, NULL, 0, DEVL, NN, DEVL, -1, NM, DEVF, AB0, DEV, AW0));
    REJECT("Nmax = -1", TDA(DEVL, DEVL, E, NULL, 0, DEVL, NN, DEVL, G, -1, DEVF, AB0, DEV, AW0));
    REJECT("out holds", TDA(DEVL, DEVL, E, NULL, 0, DEVL, NN, DEVL, G, NM, DEVF, AB0 - 1, DEV, AW0));
    REJECT("out holds", TDA(DEVL, DEVL, E, DEVF, D, DEVL, NN, DEVL, G, NM, DEVF, ABD - 1, DEV, AWD));
    REJECT("ws holds", TDA(DEVL, DEVL, E, NULL, 0, DEVL, NN, DEVL, G, NM, DEVF, AB0, DEV, AW0 - 1));
    REJECT("ws holds", TDA(DEVL, DEVL, E, DEVF, D, DEVL, NN, DEVL, G, NM, DEVF, ABD, DEV, AWD - 1));
    REJECT("ws holds", TDA(DEVL, DEVL, E, DEVF, D, DEVL, NN, DEVL, G, NM, DEVF, ABD, DEV, AW0));
    ACCEPT(TDA(DEVL, DEVL, E, NULL, 0, DEVL, NN, DEVL, G, NM, DEVF, AB0, DEV, AW0));
    ACCEPT(TDA(DEVL, DEVL, E, DEVF, D, DEVL, NN, DEVL, G, NM, DEVF, ABD, DEV, AWD));
    ACCEPT(TDA(DEVL, DEVL, E, NULL, 0, NULL, NN, DEVL, 1, NN, DEVF, (size_t)NN * NN * 4, DEV, mp_to_dense_adj_workspace(1, NN, 0)));
    ACCEPT(TDA(NULL, NULL, 0, NULL, 0, NULL, 0, DEVL, 1, 0, NULL, 0, DEV, mp_to_dense_adj_workspace(1, 0, 0)));
  }

  printf("abi_reject_dense: %d cases, %d failures\n", n_cases, n_fail);
  return n_fail ? 1 : 0;
}
