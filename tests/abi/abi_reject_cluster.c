/*
 * abi_reject_cluster.c -- argument / extent rejection harness for the cluster
 * pooling entry points of include/mi355_mp.h (mp_voxel_keys_f32,
 * mp_cluster_build, mp_cluster_reduce_f32, mp_cluster_edges,
 * mp_cluster_edge_attr_f32, mp_cluster_edge_attr_bwd_f32 and the host-side
 * mp_cluster_max_blocks / workspace queries).
 *
 * Built against the host-only AddressSanitizer build of the library
 * (`make -C pytorch_geometric-1_amd/csrc asan_cluster`) and run as a plain
 * program on a machine with no GPU by tests/test_cluster_host.py.  Every REJECT
 * case calls one entry point with one bad argument and expects MP_ERR_ARG and an
 * error text naming the problem -- no launch, no device access, no host memory
 * error (ASAN aborts the run on one).  ACCEPT cases pass every check at the
 * exact documented boundary (the call then fails at its first HIP call, as
 * there is no GPU).
 * Output: one line per case, then "abi_reject_cluster: N cases, M failures".
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
#define DI ((int32_t*)DEV)

static void expect(int line, const char* what, int rc, int want_arg, const char* needle) {
  ++n_cases;
  const char* err = mp_last_error();
  int ok;
  if (want_arg) {
    ok = rc == MP_ERR_ARG && (!needle || (err && strstr(err, needle)));
  } else {
    ok = rc != MP_ERR_ARG;
  }
  printf("%s line %d: %s -> rc %d (%s)\n", ok ? "ok  " : "FAIL", line, what, rc, err ? err : "");
  if (!ok) ++n_fail;
}

#define REJECT(needle, call) expect(__LINE__, #call, (call), 1, needle)
#define ACCEPT(call) expect(__LINE__, #call, (call), 0, NULL)

int main(void) {
  const int64_t N = 1000, E = 3000, BIG = (int64_t)1 << 31;
  const int32_t F = 33, D = 2, A = 2;
  const size_t nl = (size_t)N * 8, ni = (size_t)N * 4, rp = (size_t)(N + 1) * 4;
  const size_t el = (size_t)E * 8, ei = (size_t)E * 4, sp = (size_t)(E + 1) * 4;
  const int MAXR = MP_REDUCE_MAX, MASK = MP_FLAG_PYG_MASK;

  ++n_cases;
  {
    const int ok = mp_cluster_max_blocks() >= 256 && mp_cluster_build_workspace(N) >= nl + ni &&
                   mp_cluster_build_workspace(0) >= 256 && mp_cluster_edges_workspace(E, N) >= 2 * el + ei &&
                   mp_cluster_edges_workspace(0, 0) >= 256;
    printf("%s mp_cluster_max_blocks / workspace queries\n", ok ? "ok  " : "FAIL");
    if (!ok) ++n_fail;
  }

  /* mp_voxel_keys_f32 */
#define VOX(pos, ldp, n, d, batch, size, start, end, key, kb) \
  mp_voxel_keys_f32(pos, ldp, n, d, batch, size, start, end, key, kb, NULL)
  REJECT("n = -1", VOX(DF, D, -1, D, DL, DF, DF, DF, DL, nl));
  REJECT("not below 2^31", VOX(DF, D, BIG, D, DL, DF, DF, DF, DL, nl));
  REJECT("D = 9", VOX(DF, 9, N, 9, DL, DF, DF, DF, DL, nl));
  REJECT("D = -1", VOX(DF, D, N, -1, DL, DF, DF, DF, DL, nl));
  REJECT("D = 0 and batch is NULL", VOX(DF, D, N, 0, NULL, DF, DF, DF, DL, nl));
  REJECT("ldp = 1", VOX(DF, 1, N, D, DL, DF, DF, DF, DL, nl));
  REJECT("size is NULL", VOX(DF, D, N, D, DL, NULL, DF, DF, DL, nl));
  REJECT("start is NULL", VOX(DF, D, N, D, DL, DF, NULL, DF, DL, nl));
  REJECT("end is NULL", VOX(DF, D, N, D, DL, DF, DF, NULL, DL, nl));
  REJECT("pos is NULL", VOX(NULL, D, N, D, DL, DF, DF, DF, DL, nl));
  REJECT("key is NULL", VOX(DF, D, N, D, DL, DF, DF, DF, NULL, nl));
  REJECT("key holds", VOX(DF, D, N, D, DL, DF, DF, DF, DL, nl - 1));
  ACCEPT(VOX(DF, D, N, D, DL, DF, DF, DF, DL, nl));
  ACCEPT(VOX(DF, 8, N, 8, NULL, DF, DF, DF, DL, nl));
  ACCEPT(VOX(NULL, 0, N, 0, DL, DF, DF, DF, DL, nl));

  /* mp_cluster_build */
  const size_t bw = mp_cluster_build_workspace(N);
#define BUILD(key, n, inv, ib, rowptr, rb, member, mb, perm, pb, counts, ws, wb) \
  mp_cluster_build(key, n, inv, ib, rowptr, rb, member, mb, perm, pb, counts, ws, wb, NULL)
  REJECT("n = -1", BUILD(DL, -1, DL, nl, DI, rp, DI, ni, DL, nl, DL, DEV, bw));
  REJECT("not below 2^31", BUILD(DL, BIG, DL, nl, DI, rp, DI, ni, DL, nl, DL, DEV, bw));
  REJECT("counts is NULL", BUILD(DL, N, DL, nl, DI, rp, DI, ni, DL, nl, NULL, DEV, bw));
  REJECT("rowptr is NULL", BUILD(DL, N, DL, nl, NULL, rp, DI, ni, DL, nl, DL, DEV, bw));
  REJECT("key is NULL", BUILD(NULL, N, DL, nl, DI, rp, DI, ni, DL, nl, DL, DEV, bw));
  REJECT("inv is NULL", BUILD(DL, N, NULL, nl, DI, rp, DI, ni, DL, nl, DL, DEV, bw));
  REJECT("member is NULL", BUILD(DL, N, DL, nl, DI, rp, NULL, ni, DL, nl, DL, DEV, bw));
  REJECT("perm is NULL", BUILD(DL, N, DL, nl, DI, rp, DI, ni, NULL, nl, DL, DEV, bw));
  REJECT("ws is NULL", BUILD(DL, N, DL, nl, DI, rp, DI, ni, DL, nl, DL, NULL, bw));
  REJECT("inv holds", BUILD(DL, N, DL, nl - 1, DI, rp, DI, ni, DL, nl, DL, DEV, bw));
  REJECT("rowptr holds", BUILD(DL, N, DL, nl, DI, rp - 1, DI, ni, DL, nl, DL, DEV, bw));
  REJECT("member holds", BUILD(DL, N, DL, nl, DI, rp, DI, ni - 1, DL, nl, DL, DEV, bw));
  REJECT("perm holds", BUILD(DL, N, DL, nl, DI, rp, DI, ni, DL, nl - 1, DL, DEV, bw));
  REJECT("ws holds 255", BUILD(DL, N, DL, nl, DI, rp, DI, ni, DL, nl, DL, DEV, 255));
  REJECT("ws holds", BUILD(DL, N, DL, nl, DI, rp, DI, ni, DL, nl, DL, DEV, nl + ni + 512));
  ACCEPT(BUILD(DL, N, DL, nl, DI, rp, DI, ni, DL, nl, DL, DEV, bw));

  /* mp_cluster_reduce_f32 */
  const size_t xo = (size_t)N * F * 4, ab = (size_t)N * F * 8, po = (size_t)N * D * 4;
#define RED(x, ldx, f, red, fl, rowptr, member, counts, n, xout, ldo, xb, arg, argb, pos, ldp, dp, pout, pb, batch, \
            perm, bout, bb)                                                                                         \
  mp_cluster_reduce_f32(x, ldx, f, red, fl, rowptr, member, counts, n, xout, ldo, xb, arg, argb, pos, ldp, dp,      \
                        pout, pb, batch, perm, bout, bb, NULL)
  REJECT("n = -1", RED(DF, F, F, MAXR, MASK, DI, DI, DL, -1, DF, F, xo, DL, ab, DF, D, D, DF, po, DL, DL, DL, nl));
  REJECT("not below 2^31",
         RED(DF, F, F, MAXR, MASK, DI, DI, DL, BIG, DF, F, xo, DL, ab, DF, D, D, DF, po, DL, DL, DL, nl));
  REJECT("F = -1", RED(DF, F, -1, MAXR, MASK, DI, DI, DL, N, DF, F, xo, DL, ab, DF, D, D, DF, po, DL, DL, DL, nl));
  REJECT("Dp = -1", RED(DF, F, F, MAXR, MASK, DI, DI, DL, N, DF, F, xo, DL, ab, DF, D, -1, DF, po, DL, DL, DL, nl));
  REJECT("reduce = 0", RED(DF, F, F, 0, MASK, DI, DI, DL, N, DF, F, xo, DL, ab, DF, D, D, DF, po, DL, DL, DL, nl));
  REJECT("reduce = 3", RED(DF, F, F, 3, MASK, DI, DI, DL, N, DF, F, xo, DL, ab, DF, D, D, DF, po, DL, DL, DL, nl));
  REJECT("unknown flags", RED(DF, F, F, MAXR, 1, DI, DI, DL, N, DF, F, xo, DL, ab, DF, D, D, DF, po, DL, DL, DL, nl));
  REJECT("ldx = 32", RED(DF, F - 1, F, MAXR, MASK, DI, DI, DL, N, DF, F, xo, DL, ab, DF, D, D, DF, po, DL, DL, DL, nl));
  REJECT("ldo = 32", RED(DF, F, F, MAXR, MASK, DI, DI, DL, N, DF, F - 1, xo, DL, ab, DF, D, D, DF, po, DL, DL, DL, nl));
  REJECT("ldp = 1", RED(DF, F, F, MAXR, MASK, DI, DI, DL, N, DF, F, xo, DL, ab, DF, 1, D, DF, po, DL, DL, DL, nl));
  REJECT("counts is NULL", RED(DF, F, F, MAXR, MASK, DI, DI, NULL, N, DF, F, xo, DL, ab, DF, D, D, DF, po, DL, DL, DL, nl));
  REJECT("rowptr is NULL", RED(DF, F, F, MAXR, MASK, NULL, DI, DL, N, DF, F, xo, DL, ab, DF, D, D, DF, po, DL, DL, DL, nl));
  REJECT("member is NULL", RED(DF, F, F, MAXR, MASK, DI, NULL, DL, N, DF, F, xo, DL, ab, DF, D, D, DF, po, DL, DL, DL, nl));
  REJECT("x is NULL", RED(NULL, F, F, MAXR, MASK, DI, DI, DL, N, DF, F, xo, DL, ab, DF, D, D, DF, po, DL, DL, DL, nl));
  REJECT("x_out is NULL", RED(DF, F, F, MAXR, MASK, DI, DI, DL, N, NULL, F, xo, DL, ab, DF, D, D, DF, po, DL, DL, DL, nl));
  REJECT("pos is NULL", RED(DF, F, F, MAXR, MASK, DI, DI, DL, N, DF, F, xo, DL, ab, NULL, D, D, DF, po, DL, DL, DL, nl));
  REJECT("pos_out is NULL", RED(DF, F, F, MAXR, MASK, DI, DI, DL, N, DF, F, xo, DL, ab, DF, D, D, NULL, po, DL, DL, DL, nl));
  REJECT("batch_out needs", RED(DF, F, F, MAXR, MASK, DI, DI, DL, N, DF, F, xo, DL, ab, DF, D, D, DF, po, NULL, DL, DL, nl));
  REJECT("batch_out needs", RED(DF, F, F, MAXR, MASK, DI, DI, DL, N, DF, F, xo, DL, ab, DF, D, D, DF, po, DL, NULL, DL, nl));
  REJECT("x_out holds", RED(DF, F, F, MAXR, MASK, DI, DI, DL, N, DF, F, xo - 1, DL, ab, DF, D, D, DF, po, DL, DL, DL, nl));
  REJECT("x_out holds", RED(DF, F, F, MAXR, MASK, DI, DI, DL, N, DF, F + 7, xo, DL, ab, DF, D, D, DF, po, DL, DL, DL, nl));
  REJECT("arg holds", RED(DF, F, F, MAXR, MASK, DI, DI, DL, N, DF, F, xo, DL, ab - 1, DF, D, D, DF, po, DL, DL, DL, nl));
  REJECT("pos_out holds", RED(DF, F, F, MAXR, MASK, DI, DI, DL, N, DF, F, xo, DL, ab, DF, D, D, DF, po - 1, DL, DL, DL, nl));
  REJECT("batch_out holds", RED(DF, F, F, MAXR, MASK, DI, DI, DL, N, DF, F, xo, DL, ab, DF, D, D, DF, po, DL, DL, DL, nl - 1));
  ACCEPT(RED(DF, F, F, MAXR, MASK, DI, DI, DL, N, DF, F, xo, DL, ab, DF, D, D, DF, po, DL, DL, DL, nl));
  ACCEPT(RED(DF, F, F, MP_REDUCE_MEAN, 0, DI, DI, DL, N, DF, F, xo, NULL, 0, NULL, 0, 0, NULL, 0, NULL, NULL, NULL, 0));
  ACCEPT(RED(NULL, 0, 0, MP_REDUCE_MEAN, 0, DI, DI, DL, N, NULL, 0, 0, NULL, 0, DF, D, D, DF, po, NULL, NULL, NULL, 0));

  /* mp_cluster_edges */
  const size_t ew = mp_cluster_edges_workspace(E, N);
#define EDGES(row, col, e, inv, n, counts, orow, ocol, slot, ob, sptr, spb, sedge, seb, ws, wb) \
  mp_cluster_edges(row, col, e, inv, n, counts, orow, ocol, slot, ob, sptr, spb, sedge, seb, ws, wb, NULL)
  REJECT("n_edges = -1", EDGES(DL, DL, -1, DL, N, DL, DL, DL, DL, el, DI, sp, DI, ei, DEV, ew));
  REJECT("not below 2^31", EDGES(DL, DL, BIG, DL, N, DL, DL, DL, DL, el, DI, sp, DI, ei, DEV, ew));
  REJECT("n_nodes = -1", EDGES(DL, DL, E, DL, -1, DL, DL, DL, DL, el, DI, sp, DI, ei, DEV, ew));
  REJECT("not below 2^31", EDGES(DL, DL, E, DL, BIG, DL, DL, DL, DL, el, DI, sp, DI, ei, DEV, ew));
  REJECT("counts is NULL", EDGES(DL, DL, E, DL, N, NULL, DL, DL, DL, el, DI, sp, DI, ei, DEV, ew));
  REJECT("seg_ptr is NULL", EDGES(DL, DL, E, DL, N, DL, DL, DL, DL, el, NULL, sp, DI, ei, DEV, ew));
  REJECT("row is NULL", EDGES(NULL, DL, E, DL, N, DL, DL, DL, DL, el, DI, sp, DI, ei, DEV, ew));
  REJECT("col is NULL", EDGES(DL, NULL, E, DL, N, DL, DL, DL, DL, el, DI, sp, DI, ei, DEV, ew));
  REJECT("inv is NULL", EDGES(DL, DL, E, NULL, N, DL, DL, DL, DL, el, DI, sp, DI, ei, DEV, ew));
  REJECT("out_row is NULL", EDGES(DL, DL, E, DL, N, DL, NULL, DL, DL, el, DI, sp, DI, ei, DEV, ew));
  REJECT("out_col is NULL", EDGES(DL, DL, E, DL, N, DL, DL, NULL, DL, el, DI, sp, DI, ei, DEV, ew));
  REJECT("edge_slot is NULL", EDGES(DL, DL, E, DL, N, DL, DL, DL, NULL, el, DI, sp, DI, ei, DEV, ew));
  REJECT("seg_edge is NULL", EDGES(DL, DL, E, DL, N, DL, DL, DL, DL, el, DI, sp, NULL, ei, DEV, ew));
  REJECT("ws is NULL", EDGES(DL, DL, E, DL, N, DL, DL, DL, DL, el, DI, sp, DI, ei, NULL, ew));
  REJECT("edge_slot holds", EDGES(DL, DL, E, DL, N, DL, DL, DL, DL, el - 1, DI, sp, DI, ei, DEV, ew));
  REJECT("seg_ptr holds", EDGES(DL, DL, E, DL, N, DL, DL, DL, DL, el, DI, sp - 1, DI, ei, DEV, ew));
  REJECT("seg_edge holds", EDGES(DL, DL, E, DL, N, DL, DL, DL, DL, el, DI, sp, DI, ei - 1, DEV, ew));
  REJECT("ws holds 1024", EDGES(DL, DL, E, DL, N, DL, DL, DL, DL, el, DI, sp, DI, ei, DEV, 1024));
  REJECT("ws holds", EDGES(DL, DL, E, DL, N, DL, DL, DL, DL, el, DI, sp, DI, ei, DEV, 2 * el + ei + 255));
  ACCEPT(EDGES(DL, DL, E, DL, N, DL, DL, DL, DL, el, DI, sp, DI, ei, DEV, ew));

  /* mp_cluster_edge_attr_f32 / its backward */
  const size_t ao = (size_t)E * A * 4;
#define ATTR(attr, lda, a, sptr, sedge, counts, e, out, ldo, ob) \
  mp_cluster_edge_attr_f32(attr, lda, a, sptr, sedge, counts, e, out, ldo, ob, NULL)
  REJECT("n_edges = -1", ATTR(DF, A, A, DI, DI, DL, -1, DF, A, ao));
  REJECT("not below 2^31", ATTR(DF, A, A, DI, DI, DL, BIG, DF, A, ao));
  REJECT("A = 0", ATTR(DF, A, 0, DI, DI, DL, E, DF, A, ao));
  REJECT("lda = 1", ATTR(DF, 1, A, DI, DI, DL, E, DF, A, ao));
  REJECT("ldo = 1", ATTR(DF, A, A, DI, DI, DL, E, DF, 1, ao));
  REJECT("counts is NULL", ATTR(DF, A, A, DI, DI, NULL, E, DF, A, ao));
  REJECT("attr is NULL", ATTR(NULL, A, A, DI, DI, DL, E, DF, A, ao));
  REJECT("seg_ptr is NULL", ATTR(DF, A, A, NULL, DI, DL, E, DF, A, ao));
  REJECT("seg_edge is NULL", ATTR(DF, A, A, DI, NULL, DL, E, DF, A, ao));
  REJECT("out is NULL", ATTR(DF, A, A, DI, DI, DL, E, NULL, A, ao));
  REJECT("out holds", ATTR(DF, A, A, DI, DI, DL, E, DF, A, ao - 1));
  ACCEPT(ATTR(DF, A, A, DI, DI, DL, E, DF, A, ao));
#define ATTRB(g, ldg, slot, e, a, nout, ga, ldga, gb) mp_cluster_edge_attr_bwd_f32(g, ldg, slot, e, a, nout, ga, ldga, gb, NULL)
  REJECT("n_edges = -1", ATTRB(DF, A, DL, -1, A, 10, DF, A, ao));
  REJECT("A = 0", ATTRB(DF, A, DL, E, 0, 10, DF, A, ao));
  REJECT("n_out = 3001", ATTRB(DF, A, DL, E, A, E + 1, DF, A, ao));
  REJECT("n_out = -1", ATTRB(DF, A, DL, E, A, -1, DF, A, ao));
  REJECT("ldg = 1", ATTRB(DF, 1, DL, E, A, 10, DF, A, ao));
  REJECT("ldga = 1", ATTRB(DF, A, DL, E, A, 10, DF, 1, ao));
  REJECT("g is NULL", ATTRB(NULL, A, DL, E, A, 10, DF, A, ao));
  REJECT("edge_slot is NULL", ATTRB(DF, A, NULL, E, A, 10, DF, A, ao));
  REJECT("g_attr is NULL", ATTRB(DF, A, DL, E, A, 10, NULL, A, ao));
  REJECT("g_attr holds", ATTRB(DF, A, DL, E, A, 10, DF, A, ao - 1));
  ACCEPT(ATTRB(DF, A, DL, E, A, E, DF, A, ao));
  ACCEPT(ATTRB(NULL, A, DL, E, A, 0, DF, A, ao));

  printf("abi_reject_cluster: %d cases, %d failures\n", n_cases, n_fail);
  return n_fail ? 1 : 0;
}
