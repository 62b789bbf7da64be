/*
 * abi_reject_knn.c -- argument / extent rejection harness for the nearest-neighbour
 * entry points of include/mi355_mp.h (mp_knn_search_f32, mp_knn_fill,
 * mp_knn_interpolate_f32 and the host-side mp_knn_path, mp_knn_max_k,
 * mp_knn_max_d, mp_knn_workspace).
 *
 * Built against the host-only AddressSanitizer build of the library
 * (`make -C pytorch_geometric-1_amd/csrc asan_knn`) and run as a plain program
 * on a machine with no GPU by tests/test_knn_host.py.  The entry points return
 * int64_t: a count >= 0, or -(code).  Every REJECT case calls one of them with one
 * bad argument and expects -MP_ERR_ARG and an error text
 * naming the problem -- no launch, no device access, no host memory error (ASAN
 * aborts the run on one).  ACCEPT cases pass every check at the exact documented
 * boundary (the call then fails at its first HIP call, as there is no GPU, or
 * has nothing to launch and returns 0).
 * Output: one line per case, then "abi_reject_knn: N cases, M failures".
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi355_mp.h"

static int n_cases = 0, n_fail = 0;

#define DEV ((void*)(uintptr_t)0x7f0000000000ull) /* fake device pointer, never dereferenced */
#define DF ((float*)DEV)
#define DL ((int64_t*)DEV)

static void expect(int line, const char* what, int64_t rc, int want_arg, const char* needle) {
  ++n_cases;
  const char* err = mp_last_error();
  int ok;
  if (want_arg) {
    ok = rc == -(int64_t)MP_ERR_ARG && needle && err && strstr(err, needle);
  } else {
    ok = rc != -(int64_t)MP_ERR_ARG;
  }
  printf("%s line %d: %s -> rc %lld (%s)\n", ok ? "ok  " : "FAIL", line, what, (long long)rc, err ? err : "");
  if (!ok) ++n_fail;
}

static void check(int line, const char* what, int ok) {
  ++n_cases;
  printf("%s line %d: %s\n", ok ? "ok  " : "FAIL", line, what);
  if (!ok) ++n_fail;
}

#define REJECT(needle, call) expect(__LINE__, #call, (call), 1, needle)
#define ACCEPT(call) expect(__LINE__, #call, (call), 0, NULL)
#define CHECK(cond) check(__LINE__, #cond, (cond))

int main(void) {
  const int64_t N = 20000, M = 1000, G = 7, K = 16, BIG = (int64_t)INT32_MAX;
  const size_t kb = 4 * 8;

  /* the answers and the workspace */
  const int64_t MAXD = mp_knn_max_d(), MAXK = mp_knn_max_k();
  CHECK(MAXK == 64 && MAXD >= 256);
  CHECK(mp_knn_path(1) == 0 && mp_knn_path(3) == 0 && mp_knn_path(8) == 0);
  CHECK(mp_knn_path(9) == 1 && mp_knn_path(64) == 1 && mp_knn_path((int32_t)MAXD) == 1);
  REJECT("D = 0", mp_knn_path(0));
  REJECT("D = -1", mp_knn_path(-1));
  REJECT("is outside [1,", mp_knn_path((int32_t)MAXD + 1));
  CHECK(mp_knn_workspace(0, 1) >= 256);
  CHECK(mp_knn_workspace(M, 64) >= 2 * 1001 * 8 + (size_t)M * 64 * 8);
  CHECK(mp_knn_workspace(M, 64) > mp_knn_workspace(M, 63));
  const size_t kw = mp_knn_workspace(M, K);
  const size_t slab_only = 2 * (size_t)M * K * 4;

  /* mp_knn_search_f32 */
#define SEARCH(x, ldx, nx, y, ldy, ny, D, by, sx, gx, k, cnt, kbytes, wsp, wbytes) \
  mp_knn_search_f32(x, ldx, nx, y, ldy, ny, D, by, sx, gx, k, cnt, kbytes, wsp, wbytes, NULL)
  REJECT("n_x = -1", SEARCH(DF, 3, -1, DF, 3, M, 3, DL, DL, G, K, DL, kb, DEV, kw));
  REJECT("n_x = 2147483647", SEARCH(DF, 3, BIG, DF, 3, M, 3, DL, DL, G, K, DL, kb, DEV, kw));
  REJECT("n_y = -1", SEARCH(DF, 3, N, DF, 3, -1, 3, DL, DL, G, K, DL, kb, DEV, kw));
  REJECT("n_y = 2147483647", SEARCH(DF, 3, N, DF, 3, BIG, 3, DL, DL, G, K, DL, kb, DEV, kw));
  REJECT("k = 0", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, 0, DL, kb, DEV, kw));
  REJECT("k = -1", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, -1, DL, kb, DEV, kw));
  REJECT("k = 65", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, 65, DL, kb, DEV, kw));
  REJECT("is not below 2^31", SEARCH(DF, 3, N, DF, 3, (BIG + 1) / 64, 3, DL, DL, G, 64, DL, kb, DEV, kw));
  REJECT("is not below 2^31", SEARCH(DF, 3, N, DF, 3, BIG - 1, 3, DL, DL, G, 1, DL, kb, DEV, kw));
  REJECT("D = 0", SEARCH(DF, 3, N, DF, 3, M, 0, DL, DL, G, K, DL, kb, DEV, kw));
  REJECT("D = -3", SEARCH(DF, 3, N, DF, 3, M, -3, DL, DL, G, K, DL, kb, DEV, kw));
  REJECT("is outside [1,", SEARCH(DF, MAXD + 1, N, DF, MAXD + 1, M, (int32_t)MAXD + 1, DL, DL, G, K, DL, kb, DEV, kw));
  REJECT("ldx = 2", SEARCH(DF, 2, N, DF, 3, M, 3, DL, DL, G, K, DL, kb, DEV, kw));
  REJECT("ldy = 2", SEARCH(DF, 3, N, DF, 2, M, 3, DL, DL, G, K, DL, kb, DEV, kw));
  REJECT("ldx = 63", SEARCH(DF, 63, N, DF, 64, M, 64, DL, DL, G, K, DL, kb, DEV, kw));
  REJECT("n_graphs_x = -1", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, -1, K, DL, kb, DEV, kw));
  REJECT("n_graphs_x = 2147483647", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, BIG, K, DL, kb, DEV, kw));
  REJECT("starts_x is NULL", SEARCH(DF, 3, N, DF, 3, M, 3, DL, NULL, G, K, DL, kb, DEV, kw));
  REJECT("counts is NULL", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, K, NULL, kb, DEV, kw));
  REJECT("ws is NULL", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, K, DL, kb, NULL, kw));
  REJECT("x is NULL", SEARCH(NULL, 3, N, DF, 3, M, 3, DL, DL, G, K, DL, kb, DEV, kw));
  REJECT("y is NULL", SEARCH(DF, 3, N, NULL, 3, M, 3, DL, DL, G, K, DL, kb, DEV, kw));
  REJECT("counts holds 31", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, K, DL, kb - 1, DEV, kw));
  REJECT("ws holds", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, K, DL, kb, DEV, kw - 1));
  REJECT("ws holds 0", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, K, DL, kb, DEV, 0));
  REJECT("ws holds", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, K, DL, kb, DEV, slab_only));
  REJECT("ws holds", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, K + 1, DL, kb, DEV, kw));   /* a wider slab needs more */
  ACCEPT(SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, K, DL, kb, DEV, kw));
  ACCEPT(SEARCH(DF, 3, N, DF, 3, M, 3, NULL, DL, 1, K, DL, kb, DEV, kw));                  /* one graph */
  ACCEPT(SEARCH(DF, 8, N, DF, 8, M, 8, DL, DL, G, 1, DL, kb, DEV, kw));
  ACCEPT(SEARCH(DF, 9, N, DF, 9, M, 9, DL, DL, G, K, DL, kb, DEV, kw));                    /* the general width */
  ACCEPT(SEARCH(DF, MAXD, N, DF, MAXD + 3, M, (int32_t)MAXD, DL, DL, G, K, DL, kb, DEV, kw));
  ACCEPT(SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, 64, DL, kb, DEV, mp_knn_workspace(M, 64)));
  ACCEPT(SEARCH(NULL, 3, 0, DF, 3, M, 3, DL, DL, 0, K, DL, kb, DEV, kw));                  /* nothing to search */
  ACCEPT(SEARCH(DF, 3, N, NULL, 3, 0, 3, NULL, DL, 1, K, DL, kb, DEV, mp_knn_workspace(0, K)));

  /* mp_knn_fill */
  const int64_t E = 500;
  const size_t ob = (size_t)E * 8, wb = (size_t)E * 4;
  REJECT("n_y = -1", mp_knn_fill(-1, K, E, DL, DL, ob, NULL, 0, DEV, kw, NULL));
  REJECT("n_y = 2147483647", mp_knn_fill(BIG, K, E, DL, DL, ob, NULL, 0, DEV, kw, NULL));
  REJECT("k = 0", mp_knn_fill(M, 0, E, DL, DL, ob, NULL, 0, DEV, kw, NULL));
  REJECT("k = 65", mp_knn_fill(M, 65, E, DL, DL, ob, NULL, 0, DEV, kw, NULL));
  REJECT("is not below 2^31", mp_knn_fill((BIG + 1) / 64, 64, E, DL, DL, ob, NULL, 0, DEV, kw, NULL));
  REJECT("n_edges = -1", mp_knn_fill(M, K, -1, DL, DL, ob, NULL, 0, DEV, kw, NULL));
  REJECT("n_edges = 16001", mp_knn_fill(M, K, M * K + 1, DL, DL, (size_t)(M * K + 1) * 8, NULL, 0, DEV, kw, NULL));
  REJECT("ws is NULL", mp_knn_fill(M, K, E, DL, DL, ob, NULL, 0, NULL, kw, NULL));
  REJECT("out_y is NULL", mp_knn_fill(M, K, E, NULL, DL, ob, NULL, 0, DEV, kw, NULL));
  REJECT("out_x is NULL", mp_knn_fill(M, K, E, DL, NULL, ob, NULL, 0, DEV, kw, NULL));
  REJECT("out_y / out_x holds", mp_knn_fill(M, K, E, DL, DL, ob - 1, NULL, 0, DEV, kw, NULL));
  REJECT("out_w holds", mp_knn_fill(M, K, E, DL, DL, ob, DF, wb - 1, DEV, kw, NULL));
  REJECT("ws holds", mp_knn_fill(M, K, E, DL, DL, ob, NULL, 0, DEV, slab_only, NULL));      /* the slab alone */
  REJECT("ws holds 0", mp_knn_fill(M, K, E, DL, DL, ob, NULL, 0, DEV, 0, NULL));
  ACCEPT(mp_knn_fill(M, K, E, DL, DL, ob, NULL, 0, DEV, kw, NULL));
  ACCEPT(mp_knn_fill(M, K, E, DL, DL, ob, DF, wb, DEV, kw, NULL));
  ACCEPT(mp_knn_fill(M, K, M * K, DL, DL, (size_t)M * K * 8, DF, (size_t)M * K * 4, DEV, kw, NULL));
  {
    const int64_t rc = mp_knn_fill(M, K, 0, NULL, NULL, 0, NULL, 0, DEV, kw, NULL);  /* nothing to launch */
    CHECK(rc == 0);
  }

  /* mp_knn_interpolate_f32 */
  const int32_t C = 130;
  const size_t xb = ((size_t)(M - 1) * 132 + C) * 4;   /* rows of 130 with a stride of 132 */
#define INTERP(x, ldx, nx, c, ny, k, wsp, wbytes, out, ldo, obytes) \
  mp_knn_interpolate_f32(x, ldx, nx, c, ny, k, wsp, wbytes, out, ldo, obytes, NULL)
  REJECT("n_x = -1", INTERP(DF, C, -1, C, M, K, DEV, kw, DF, 132, xb));
  REJECT("n_x = 2147483647", INTERP(DF, C, BIG, C, M, K, DEV, kw, DF, 132, xb));
  REJECT("n_y = -1", INTERP(DF, C, N, C, -1, K, DEV, kw, DF, 132, xb));
  REJECT("k = 0", INTERP(DF, C, N, C, M, 0, DEV, kw, DF, 132, xb));
  REJECT("k = 65", INTERP(DF, C, N, C, M, 65, DEV, kw, DF, 132, xb));
  REJECT("is not below 2^31", INTERP(DF, C, N, C, (BIG + 1) / 64, 64, DEV, kw, DF, 132, xb));
  REJECT("C = 0", INTERP(DF, C, N, 0, M, K, DEV, kw, DF, 132, xb));
  REJECT("C = -4", INTERP(DF, C, N, -4, M, K, DEV, kw, DF, 132, xb));
  REJECT("ldx = 129", INTERP(DF, 129, N, C, M, K, DEV, kw, DF, 132, xb));
  REJECT("ldo = 129", INTERP(DF, C, N, C, M, K, DEV, kw, DF, 129, xb));
  REJECT("ws is NULL", INTERP(DF, C, N, C, M, K, NULL, kw, DF, 132, xb));
  REJECT("x is NULL", INTERP(NULL, C, N, C, M, K, DEV, kw, DF, 132, xb));
  REJECT("out is NULL", INTERP(DF, C, N, C, M, K, DEV, kw, NULL, 132, xb));
  REJECT("out holds", INTERP(DF, C, N, C, M, K, DEV, kw, DF, 132, xb - 1));
  REJECT("out holds", INTERP(DF, C, N, C, M, K, DEV, kw, DF, 133, xb));                   /* a wider row stride needs more */
  REJECT("ws holds", INTERP(DF, C, N, C, M, K, DEV, slab_only, DF, 132, xb));
  REJECT("ws holds", INTERP(DF, C, N, C, M, K + 1, DEV, kw, DF, 132, xb));
  ACCEPT(INTERP(DF, C, N, C, M, K, DEV, kw, DF, 132, xb));
  ACCEPT(INTERP(DF, 1, N, 1, M, K, DEV, kw, DF, 1, (size_t)M * 4));
  ACCEPT(INTERP(DF, 128, N, 128, M, K, DEV, kw, DF, 128, (size_t)M * 128 * 4));          /* the float4 form */
  ACCEPT(INTERP(NULL, C, 0, C, M, K, DEV, kw, DF, 132, xb));                              /* no x: rows of zeros */
  {
    const int64_t rc = INTERP(DF, C, N, C, 0, K, DEV, mp_knn_workspace(0, K), NULL, 132, 0);  /* no rows */
    CHECK(rc == 0);
  }

  printf("abi_reject_knn: %d cases, %d failures\n", n_cases, n_fail);
  return n_fail ? 1 : 0;
}
