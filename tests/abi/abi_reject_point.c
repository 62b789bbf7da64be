/*
 * abi_reject_point.c -- argument / extent rejection harness for the point-set
 * entry points of include/mi355_mp.h (mp_fps_f32, mp_radius_search_f32,
 * mp_radius_fill, mp_point_edge_features_f32 and the host-side mp_fps_path,
 * mp_fps_workspace, mp_radius_workspace).
 *
 * Built against the host-only AddressSanitizer build of the library
 * (`make -C pytorch_geometric-1_amd/csrc asan_point`) and run as a plain program
 * on a machine with no GPU by tests/test_point_host.py.  The entry points return
 * int64_t: a count >= 0, or -(code).  Every REJECT case calls one of them with one
 * bad argument and expects -MP_ERR_ARG and an error text
 * naming the problem -- no launch, no device access, no host memory error (ASAN
 * aborts the run on one).  ACCEPT cases pass every check at the exact documented
 * boundary (the call then fails at its first HIP call, as there is no GPU, or
 * has nothing to launch and returns 0).
 * Output: one line per case, then "abi_reject_point: N cases, M failures".
 */
#include <math.h>
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
  const int64_t N = 20000, G = 7, BIG = (int64_t)INT32_MAX;
  const size_t ib = (size_t)N * 8, kb = 4 * 8;

  /* the paths and the workspaces */
  CHECK(mp_fps_path(0) == 0 && mp_fps_path(1) == 0 && mp_fps_path(64) == 0);
  CHECK(mp_fps_path(1 << 20) == 2);
  {
    int prev = 0, mono = 1, seen = 1;
    for (int64_t n = 1; n <= 40000; ++n) {
      const int p = (int)mp_fps_path(n);
      if (p < prev || p > 2) mono = 0;
      if (p != prev) ++seen;
      prev = p;
    }
    CHECK(mono && seen == 3);
  }
  CHECK(mp_fps_workspace(N, 100) >= 256 && mp_fps_workspace(N, N) >= (size_t)N * 4);
  CHECK(mp_radius_workspace(0, 1) >= 256);
  CHECK(mp_radius_workspace(1000, 64) >= 2 * 1001 * 8 + (size_t)1000 * 64 * 4);
  CHECK(mp_radius_workspace(1000, 65) > mp_radius_workspace(1000, 64));
  const size_t fw = mp_fps_workspace(N, N);

  /* mp_fps_f32 */
#define FPS(pos, ldp, n, D, st, g, mx, os, first, idx, ibytes, cnt, kbytes, wsp, wbytes) \
  mp_fps_f32(pos, ldp, n, D, st, g, mx, os, first, idx, ibytes, cnt, kbytes, wsp, wbytes, NULL)
  REJECT("n = -1", FPS(DF, 3, -1, 3, DL, G, 0, DL, DL, DL, ib, DL, kb, DEV, fw));
  REJECT("not below 2^31", FPS(DF, 3, BIG, 3, DL, G, N, DL, DL, DL, ib, DL, kb, DEV, fw));
  REJECT("D = 0", FPS(DF, 3, N, 0, DL, G, N, DL, DL, DL, ib, DL, kb, DEV, fw));
  REJECT("D = 9", FPS(DF, 9, N, 9, DL, G, N, DL, DL, DL, ib, DL, kb, DEV, fw));
  REJECT("ldp = 2", FPS(DF, 2, N, 3, DL, G, N, DL, DL, DL, ib, DL, kb, DEV, fw));
  REJECT("n_graphs = -1", FPS(DF, 3, N, 3, DL, -1, N, DL, DL, DL, ib, DL, kb, DEV, fw));
  REJECT("n_graphs = 2147483647", FPS(DF, 3, N, 3, DL, BIG, N, DL, DL, DL, ib, DL, kb, DEV, fw));
  REJECT("n_graphs = 0", FPS(DF, 3, N, 3, DL, 0, N, DL, DL, DL, ib, DL, kb, DEV, fw));
  REJECT("max_n = -1", FPS(DF, 3, N, 3, DL, G, -1, DL, DL, DL, ib, DL, kb, DEV, fw));
  REJECT("max_n = 20001", FPS(DF, 3, N, 3, DL, G, N + 1, DL, DL, DL, ib, DL, kb, DEV, fw));
  REJECT("starts is NULL", FPS(DF, 3, N, 3, NULL, G, N, DL, DL, DL, ib, DL, kb, DEV, fw));
  REJECT("out_starts is NULL", FPS(DF, 3, N, 3, DL, G, N, NULL, DL, DL, ib, DL, kb, DEV, fw));
  REJECT("counts is NULL", FPS(DF, 3, N, 3, DL, G, N, DL, DL, DL, ib, NULL, kb, DEV, fw));
  REJECT("ws is NULL", FPS(DF, 3, N, 3, DL, G, N, DL, DL, DL, ib, DL, kb, NULL, fw));
  REJECT("pos is NULL", FPS(NULL, 3, N, 3, DL, G, N, DL, DL, DL, ib, DL, kb, DEV, fw));
  REJECT("idx is NULL", FPS(DF, 3, N, 3, DL, G, N, DL, DL, NULL, ib, DL, kb, DEV, fw));
  REJECT("counts holds 31", FPS(DF, 3, N, 3, DL, G, N, DL, DL, DL, ib, DL, kb - 1, DEV, fw));
  REJECT("ws holds", FPS(DF, 3, N, 3, DL, G, N, DL, DL, DL, ib, DL, kb, DEV, fw - 1));
  REJECT("ws holds 255", FPS(DF, 3, N, 3, DL, G, 100, DL, DL, DL, ib, DL, kb, DEV, 255));
  ACCEPT(FPS(DF, 3, N, 3, DL, G, N, DL, DL, DL, ib, DL, kb, DEV, fw));
  ACCEPT(FPS(DF, 3, N, 3, DL, G, N, DL, NULL, DL, ib, DL, kb, DEV, fw));      /* no starts: offset 0 */
  ACCEPT(FPS(DF, 3, N, 3, DL, G, 100, DL, DL, DL, ib, DL, kb, DEV, 256));     /* on chip: 256 bytes do */
  ACCEPT(FPS(DF, 8, N, 8, DL, G, N, DL, DL, DL, 0, DL, kb, DEV, fw));         /* an idx of no room is never written */
  ACCEPT(FPS(DF, 1, N, 1, DL, G, N, DL, DL, DL, ib, DL, kb, DEV, fw));
  ACCEPT(FPS(NULL, 3, 0, 3, DL, 0, 0, DL, NULL, NULL, 0, DL, kb, DEV, 256));

  /* mp_radius_search_f32 */
  const int64_t M = 1000, CAP = 64;
  const size_t rw = mp_radius_workspace(M, CAP);
#define SEARCH(x, ldx, nx, y, ldy, ny, D, by, sx, gx, r, cap, cnt, kbytes, wsp, wbytes) \
  mp_radius_search_f32(x, ldx, nx, y, ldy, ny, D, by, sx, gx, r, cap, cnt, kbytes, wsp, wbytes, NULL)
  REJECT("n_x = -1", SEARCH(DF, 3, -1, DF, 3, M, 3, DL, DL, G, 0.5f, CAP, DL, kb, DEV, rw));
  REJECT("n_x = 2147483647", SEARCH(DF, 3, BIG, DF, 3, M, 3, DL, DL, G, 0.5f, CAP, DL, kb, DEV, rw));
  REJECT("n_y = -1", SEARCH(DF, 3, N, DF, 3, -1, 3, DL, DL, G, 0.5f, CAP, DL, kb, DEV, rw));
  REJECT("n_y = 2147483647", SEARCH(DF, 3, N, DF, 3, BIG, 3, DL, DL, G, 0.5f, CAP, DL, kb, DEV, rw));
  REJECT("D = 0", SEARCH(DF, 3, N, DF, 3, M, 0, DL, DL, G, 0.5f, CAP, DL, kb, DEV, rw));
  REJECT("D = 9", SEARCH(DF, 9, N, DF, 9, M, 9, DL, DL, G, 0.5f, CAP, DL, kb, DEV, rw));
  REJECT("ldx = 2", SEARCH(DF, 2, N, DF, 3, M, 3, DL, DL, G, 0.5f, CAP, DL, kb, DEV, rw));
  REJECT("ldy = 2", SEARCH(DF, 3, N, DF, 2, M, 3, DL, DL, G, 0.5f, CAP, DL, kb, DEV, rw));
  REJECT("n_graphs_x = -1", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, -1, 0.5f, CAP, DL, kb, DEV, rw));
  REJECT("negative or not finite", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, -0.5f, CAP, DL, kb, DEV, rw));
  REJECT("negative or not finite", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, NAN, CAP, DL, kb, DEV, rw));
  REJECT("negative or not finite", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, INFINITY, CAP, DL, kb, DEV, rw));
  REJECT("cap = 0", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, 0.5f, 0, DL, kb, DEV, rw));
  REJECT("cap = 2147483647", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, 0.5f, BIG, DL, kb, DEV, rw));
  REJECT("is not below 2^31", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, 0.5f, BIG / M, DL, kb, DEV, rw));
  REJECT("starts_x is NULL", SEARCH(DF, 3, N, DF, 3, M, 3, DL, NULL, G, 0.5f, CAP, DL, kb, DEV, rw));
  REJECT("counts is NULL", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, 0.5f, CAP, NULL, kb, DEV, rw));
  REJECT("ws is NULL", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, 0.5f, CAP, DL, kb, NULL, rw));
  REJECT("x is NULL", SEARCH(NULL, 3, N, DF, 3, M, 3, DL, DL, G, 0.5f, CAP, DL, kb, DEV, rw));
  REJECT("y is NULL", SEARCH(DF, 3, N, NULL, 3, M, 3, DL, DL, G, 0.5f, CAP, DL, kb, DEV, rw));
  REJECT("counts holds 31", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, 0.5f, CAP, DL, kb - 1, DEV, rw));
  REJECT("ws holds", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, 0.5f, CAP, DL, kb, DEV, rw - 1));
  REJECT("ws holds 0", SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, 0.5f, CAP, DL, kb, DEV, 0));
  ACCEPT(SEARCH(DF, 3, N, DF, 3, M, 3, DL, DL, G, 0.5f, CAP, DL, kb, DEV, rw));
  ACCEPT(SEARCH(DF, 3, N, DF, 3, M, 3, NULL, DL, 1, 0.f, CAP, DL, kb, DEV, rw));   /* one graph, r = 0 */
  ACCEPT(SEARCH(DF, 8, N, DF, 8, M, 8, DL, DL, G, 3.0e38f, CAP, DL, kb, DEV, rw));
  ACCEPT(SEARCH(NULL, 3, 0, DF, 3, M, 3, DL, DL, 0, 0.5f, CAP, DL, kb, DEV, rw));  /* nothing to search */

  /* mp_radius_fill */
  const size_t ob = (size_t)500 * 8;
  REJECT("n_y = -1", mp_radius_fill(-1, CAP, 500, DL, DL, ob, DEV, rw, NULL));
  REJECT("cap = 0", mp_radius_fill(M, 0, 500, DL, DL, ob, DEV, rw, NULL));
  REJECT("is not below 2^31", mp_radius_fill(M, BIG / M, 500, DL, DL, ob, DEV, rw, NULL));
  REJECT("n_edges = -1", mp_radius_fill(M, CAP, -1, DL, DL, ob, DEV, rw, NULL));
  REJECT("n_edges = 64001", mp_radius_fill(M, CAP, M * CAP + 1, DL, DL, (size_t)(M * CAP + 1) * 8, DEV, rw, NULL));
  REJECT("ws is NULL", mp_radius_fill(M, CAP, 500, DL, DL, ob, NULL, rw, NULL));
  REJECT("out_y is NULL", mp_radius_fill(M, CAP, 500, NULL, DL, ob, DEV, rw, NULL));
  REJECT("out_x is NULL", mp_radius_fill(M, CAP, 500, DL, NULL, ob, DEV, rw, NULL));
  REJECT("out_y / out_x holds", mp_radius_fill(M, CAP, 500, DL, DL, ob - 1, DEV, rw, NULL));
  REJECT("ws holds", mp_radius_fill(M, CAP, 500, DL, DL, ob, DEV, (size_t)M * CAP * 4, NULL));  /* the slab alone */
  ACCEPT(mp_radius_fill(M, CAP, 500, DL, DL, ob, DEV, rw, NULL));
  {
    const int64_t rc = mp_radius_fill(M, CAP, 0, NULL, NULL, 0, DEV, rw, NULL);  /* nothing to launch */
    CHECK(rc == 0);
  }

  /* mp_point_edge_features_f32 */
  const int64_t E = 5000;
  const size_t eb = (size_t)E * (16 + 3) * 4;
#define FEAT(x, ldx, F, ps, ldps, ns, pd, ldpd, nd, D, src, dst, e, out, ldo, obytes) \
  mp_point_edge_features_f32(x, ldx, F, ps, ldps, ns, pd, ldpd, nd, D, src, dst, e, out, ldo, obytes, NULL)
  REJECT("n_edges = -1", FEAT(DF, 16, 16, DF, 3, N, DF, 3, M, 3, DL, DL, -1, DF, 19, eb));
  REJECT("n_edges = 2147483647", FEAT(DF, 16, 16, DF, 3, N, DF, 3, M, 3, DL, DL, BIG, DF, 19, eb));
  REJECT("n_src = -1", FEAT(DF, 16, 16, DF, 3, -1, DF, 3, M, 3, DL, DL, E, DF, 19, eb));
  REJECT("n_dst = -1", FEAT(DF, 16, 16, DF, 3, N, DF, 3, -1, 3, DL, DL, E, DF, 19, eb));
  REJECT("F = -1", FEAT(DF, 16, -1, DF, 3, N, DF, 3, M, 3, DL, DL, E, DF, 19, eb));
  REJECT("D = 0", FEAT(DF, 16, 16, DF, 3, N, DF, 3, M, 0, DL, DL, E, DF, 19, eb));
  REJECT("D = 9", FEAT(DF, 16, 16, DF, 9, N, DF, 9, M, 9, DL, DL, E, DF, 25, eb));
  REJECT("ldx = 15", FEAT(DF, 15, 16, DF, 3, N, DF, 3, M, 3, DL, DL, E, DF, 19, eb));
  REJECT("ldps = 2", FEAT(DF, 16, 16, DF, 2, N, DF, 3, M, 3, DL, DL, E, DF, 19, eb));
  REJECT("ldpd = 2", FEAT(DF, 16, 16, DF, 3, N, DF, 2, M, 3, DL, DL, E, DF, 19, eb));
  REJECT("ldo = 18", FEAT(DF, 16, 16, DF, 3, N, DF, 3, M, 3, DL, DL, E, DF, 18, eb));
  REJECT("x_src is NULL", FEAT(NULL, 16, 16, DF, 3, N, DF, 3, M, 3, DL, DL, E, DF, 19, eb));
  REJECT("pos_src is NULL", FEAT(DF, 16, 16, NULL, 3, N, DF, 3, M, 3, DL, DL, E, DF, 19, eb));
  REJECT("pos_dst is NULL", FEAT(DF, 16, 16, DF, 3, N, NULL, 3, M, 3, DL, DL, E, DF, 19, eb));
  REJECT("src is NULL", FEAT(DF, 16, 16, DF, 3, N, DF, 3, M, 3, NULL, DL, E, DF, 19, eb));
  REJECT("dst is NULL", FEAT(DF, 16, 16, DF, 3, N, DF, 3, M, 3, DL, NULL, E, DF, 19, eb));
  REJECT("out is NULL", FEAT(DF, 16, 16, DF, 3, N, DF, 3, M, 3, DL, DL, E, NULL, 19, eb));
  REJECT("out holds", FEAT(DF, 16, 16, DF, 3, N, DF, 3, M, 3, DL, DL, E, DF, 19, eb - 1));
  REJECT("out holds", FEAT(DF, 16, 16, DF, 3, N, DF, 3, M, 3, DL, DL, E, DF, 20, eb));   /* a wider row stride needs more */
  ACCEPT(FEAT(DF, 16, 16, DF, 3, N, DF, 3, M, 3, DL, DL, E, DF, 19, eb));
  ACCEPT(FEAT(NULL, 0, 0, DF, 3, N, DF, 3, M, 3, DL, DL, E, DF, 3, (size_t)E * 3 * 4));     /* no x: the differences */
  ACCEPT(FEAT(DF, 17, 15, DF, 4, N, DF, 8, M, 3, DL, DL, E, DF, 18, (size_t)E * 18 * 4));   /* strides, odd F */
  {
    const int64_t rc = FEAT(NULL, 0, 0, NULL, 3, N, NULL, 3, M, 3, NULL, NULL, 0, NULL, 3, 0);  /* no edges */
    CHECK(rc == 0);
  }

  printf("abi_reject_point: %d cases, %d failures\n", n_cases, n_fail);
  return n_fail ? 1 : 0;
}
