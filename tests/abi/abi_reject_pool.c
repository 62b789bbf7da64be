/*
 * abi_reject_pool.c -- argument / extent rejection harness for the TopKPooling
 * entry points of include/mi355_mp.h (mp_batch_stats, mp_batch_starts,
 * mp_pool_score_f32, mp_pool_score_bwd_f32, mp_topk_counts, mp_topk_select_f32,
 * mp_pool_gate_f32, mp_pool_gate_bwd_f32, mp_pool_inverse, mp_pool_compact,
 * mp_pool_filter_adj, and the host-side mp_topk_path).
 *
 * Built against the host-only AddressSanitizer build of the library
 * (`make -C pytorch_geometric-1_amd/csrc asan_pool`) and run as a plain program
 * on a machine with no GPU by tests/test_pool_host.py.  Every REJECT case calls
 * one entry point with one bad argument and expects MP_ERR_ARG and an error
 * text naming the problem -- no launch, no device access, no host memory error
 * (ASAN aborts the run on one).  ACCEPT cases pass every check at the exact
 * documented boundary (the call then fails at its first HIP call, as there is
 * no GPU).
 * Output: one line per case, then "abi_reject_pool: N cases, M failures".
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
#define DB ((uint8_t*)DEV)

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
  const int64_t N = 1000, G = 7, E = 3000, K = 400;
  const int32_t F = 33;
  const size_t nf = (size_t)N * 4, nl = (size_t)N * 8, gl = (size_t)(G + 1) * 8, el = (size_t)E * 8;
  const int T = MP_POOL_SCORE_TANH;

  /* mp_topk_path: the documented limits, and the mp_tune key that moves the second */
  ++n_cases;
  {
    const int64_t L = mp_tune(MP_TUNE_TOPK_WG_LIMIT, -1);
    int ok = L == 2048 && mp_topk_path(0) == 0 && mp_topk_path(64) == 0 && mp_topk_path(65) == 1 &&
             mp_topk_path(L) == 1 && mp_topk_path(L + 1) == 2;
    ok = ok && mp_tune(MP_TUNE_TOPK_WG_LIMIT, 63) == -1 && mp_tune(MP_TUNE_TOPK_WG_LIMIT, 8193) == -1;
    ok = ok && mp_tune(MP_TUNE_TOPK_WG_LIMIT, 1024) == L && mp_topk_path(1025) == 2 &&
         mp_tune(MP_TUNE_TOPK_WG_LIMIT, L) == 1024;
    printf("%s mp_topk_path limits\n", ok ? "ok  " : "FAIL");
    if (!ok) ++n_fail;
  }

  /* mp_batch_stats / mp_batch_starts */
  REJECT("n = -1", mp_batch_stats(DL, -1, DL, 24, NULL));
  REJECT("stats is NULL", mp_batch_stats(DL, N, NULL, 24, NULL));
  REJECT("batch is NULL", mp_batch_stats(NULL, N, DL, 24, NULL));
  REJECT("stats holds 23", mp_batch_stats(DL, N, DL, 23, NULL));
  ACCEPT(mp_batch_stats(DL, N, DL, 24, NULL));
  REJECT("n = -1", mp_batch_starts(DL, -1, G, DL, gl, NULL));
  REJECT("n_graphs = -1", mp_batch_starts(DL, N, -1, DL, gl, NULL));
  REJECT("starts is NULL", mp_batch_starts(DL, N, G, NULL, gl, NULL));
  REJECT("batch is NULL", mp_batch_starts(NULL, N, G, DL, gl, NULL));
  REJECT("starts holds", mp_batch_starts(DL, N, G, DL, gl - 1, NULL));
  ACCEPT(mp_batch_starts(DL, N, G, DL, gl, NULL));

  /* mp_pool_score_f32 */
  REJECT("n = -1", mp_pool_score_f32(DF, F, -1, F, DF, T, DF, nf, NULL));
  REJECT("F = 0", mp_pool_score_f32(DF, F, N, 0, DF, T, DF, nf, NULL));
  REJECT("ld = 32", mp_pool_score_f32(DF, F - 1, N, F, DF, T, DF, nf, NULL));
  REJECT("unknown flags", mp_pool_score_f32(DF, F, N, F, DF, 4, DF, nf, NULL));
  REJECT("w is NULL", mp_pool_score_f32(DF, F, N, F, NULL, T, DF, nf, NULL));
  REJECT("attn is NULL", mp_pool_score_f32(NULL, F, N, F, DF, T, DF, nf, NULL));
  REJECT("score is NULL", mp_pool_score_f32(DF, F, N, F, DF, T, NULL, nf, NULL));
  REJECT("score holds", mp_pool_score_f32(DF, F, N, F, DF, T, DF, nf - 1, NULL));
  ACCEPT(mp_pool_score_f32(DF, F, N, F, DF, T, DF, nf, NULL));
  ACCEPT(mp_pool_score_f32(DF, 1, N, 1, DF, MP_POOL_SCORE_RAW, DF, nf, NULL));

  /* mp_pool_score_bwd_f32 */
  const size_t wsb = mp_pool_score_bwd_workspace(N, F);
  ++n_cases;
  if (!(mp_pool_score_bwd_parts(0) == 1 && mp_pool_score_bwd_parts(256) == 1 && mp_pool_score_bwd_parts(257) == 2 &&
        mp_pool_score_bwd_parts((int64_t)1 << 30) == 512 && wsb >= 2 * nf + 4 * (size_t)(F + 1) * 4)) {
    printf("FAIL mp_pool_score_bwd_parts / workspace\n");
    ++n_fail;
  } else {
    printf("ok   mp_pool_score_bwd_parts / workspace\n");
  }
  REJECT("n = -1", mp_pool_score_bwd_f32(DF, F, -1, F, DF, T, DF, DF, DF, F, DF, F * 4, DEV, wsb, NULL));
  REJECT("F = 0", mp_pool_score_bwd_f32(DF, F, N, 0, DF, T, DF, DF, DF, F, DF, F * 4, DEV, wsb, NULL));
  REJECT("ld = 32", mp_pool_score_bwd_f32(DF, F - 1, N, F, DF, T, DF, DF, DF, F, DF, F * 4, DEV, wsb, NULL));
  REJECT("ldg = 32", mp_pool_score_bwd_f32(DF, F, N, F, DF, T, DF, DF, DF, F - 1, DF, F * 4, DEV, wsb, NULL));
  REJECT("unknown flags", mp_pool_score_bwd_f32(DF, F, N, F, DF, 8, DF, DF, DF, F, DF, F * 4, DEV, wsb, NULL));
  REJECT("w is NULL", mp_pool_score_bwd_f32(DF, F, N, F, NULL, T, DF, DF, DF, F, DF, F * 4, DEV, wsb, NULL));
  REJECT("g_w is NULL", mp_pool_score_bwd_f32(DF, F, N, F, DF, T, DF, DF, DF, F, NULL, F * 4, DEV, wsb, NULL));
  REJECT("attn is NULL", mp_pool_score_bwd_f32(NULL, F, N, F, DF, T, DF, DF, DF, F, DF, F * 4, DEV, wsb, NULL));
  REJECT("g_score is NULL", mp_pool_score_bwd_f32(DF, F, N, F, DF, T, DF, NULL, DF, F, DF, F * 4, DEV, wsb, NULL));
  REJECT("score is NULL", mp_pool_score_bwd_f32(DF, F, N, F, DF, T, NULL, DF, DF, F, DF, F * 4, DEV, wsb, NULL));
  REJECT("ws is NULL", mp_pool_score_bwd_f32(DF, F, N, F, DF, T, DF, DF, DF, F, DF, F * 4, NULL, wsb, NULL));
  REJECT("g_w holds", mp_pool_score_bwd_f32(DF, F, N, F, DF, T, DF, DF, DF, F, DF, F * 4 - 1, DEV, wsb, NULL));
  REJECT("ws holds", mp_pool_score_bwd_f32(DF, F, N, F, DF, T, DF, DF, DF, F, DF, F * 4, DEV, wsb - 1, NULL));
  ACCEPT(mp_pool_score_bwd_f32(DF, F, N, F, DF, T, DF, DF, NULL, 0, DF, F * 4, DEV, wsb, NULL));
  ACCEPT(mp_pool_score_bwd_f32(DF, F, N, F, DF, 0, NULL, DF, DF, F, DF, F * 4, DEV, wsb, NULL));

  /* mp_topk_counts */
  REJECT("n_graphs = -1", mp_topk_counts(DL, -1, 0.5f, N, DL, gl, DL, NULL));
  REJECT("ratio = 0", mp_topk_counts(DL, G, 0.f, N, DL, gl, DL, NULL));
  REJECT("ratio = 1.5", mp_topk_counts(DL, G, 1.5f, N, DL, gl, DL, NULL));
  REJECT("max_n = -1", mp_topk_counts(DL, G, 0.5f, -1, DL, gl, DL, NULL));
  REJECT("starts is NULL", mp_topk_counts(NULL, G, 0.5f, N, DL, gl, DL, NULL));
  REJECT("out_starts is NULL", mp_topk_counts(DL, G, 0.5f, N, NULL, gl, DL, NULL));
  REJECT("counts is NULL", mp_topk_counts(DL, G, 0.5f, N, DL, gl, NULL, NULL));
  REJECT("out_starts holds", mp_topk_counts(DL, G, 0.5f, N, DL, gl - 1, DL, NULL));
  ACCEPT(mp_topk_counts(DL, G, 1.0f, N, DL, gl, DL, NULL));

  /* mp_topk_select_f32: max_n = 64 needs the 256-byte minimum workspace only */
  const size_t sw = mp_topk_workspace(N, G, 64);
  ++n_cases;
  if (sw != 256 || mp_topk_workspace(N, G, 1000) != 256) {
    printf("FAIL mp_topk_workspace below the workgroup limit\n");
    ++n_fail;
  } else {
    printf("ok   mp_topk_workspace below the workgroup limit\n");
  }
#define SELECT(score, n, starts, g, max_n, ratio, perm, pb, os, ob, inv, ib, counts, ws, wb) \
  mp_topk_select_f32(score, n, starts, g, max_n, ratio, perm, pb, os, ob, inv, ib, counts, ws, wb, NULL)
  REJECT("n = -1", SELECT(DF, -1, DL, G, 64, 0.5f, DL, nl, DL, gl, DL, nl, DL, DEV, sw));
  REJECT("n_graphs = -1", SELECT(DF, N, DL, -1, 64, 0.5f, DL, nl, DL, gl, DL, nl, DL, DEV, sw));
  REJECT("n_graphs = 0", SELECT(DF, N, DL, 0, 64, 0.5f, DL, nl, DL, gl, DL, nl, DL, DEV, sw));
  REJECT("ratio = 0", SELECT(DF, N, DL, G, 64, 0.f, DL, nl, DL, gl, DL, nl, DL, DEV, sw));
  REJECT("ratio = 1.5", SELECT(DF, N, DL, G, 64, 1.5f, DL, nl, DL, gl, DL, nl, DL, DEV, sw));
  REJECT("ratio = -0.5", SELECT(DF, N, DL, G, 64, -0.5f, DL, nl, DL, gl, DL, nl, DL, DEV, sw));
  REJECT("max_n = 1001", SELECT(DF, N, DL, G, N + 1, 0.5f, DL, nl, DL, gl, DL, nl, DL, DEV, sw));
  REJECT("max_n = -1", SELECT(DF, N, DL, G, -1, 0.5f, DL, nl, DL, gl, DL, nl, DL, DEV, sw));
  REJECT("starts is NULL", SELECT(DF, N, NULL, G, 64, 0.5f, DL, nl, DL, gl, DL, nl, DL, DEV, sw));
  REJECT("out_starts is NULL", SELECT(DF, N, DL, G, 64, 0.5f, DL, nl, NULL, gl, DL, nl, DL, DEV, sw));
  REJECT("counts is NULL", SELECT(DF, N, DL, G, 64, 0.5f, DL, nl, DL, gl, DL, nl, NULL, DEV, sw));
  REJECT("score is NULL", SELECT(NULL, N, DL, G, 64, 0.5f, DL, nl, DL, gl, DL, nl, DL, DEV, sw));
  REJECT("perm is NULL", SELECT(DF, N, DL, G, 64, 0.5f, NULL, nl, DL, gl, DL, nl, DL, DEV, sw));
  REJECT("inv is NULL", SELECT(DF, N, DL, G, 64, 0.5f, DL, nl, DL, gl, NULL, nl, DL, DEV, sw));
  REJECT("ws is NULL", SELECT(DF, N, DL, G, 64, 0.5f, DL, nl, DL, gl, DL, nl, DL, NULL, sw));
  REJECT("perm holds", SELECT(DF, N, DL, G, 64, 0.5f, DL, nl - 1, DL, gl, DL, nl, DL, DEV, sw));
  REJECT("inv holds", SELECT(DF, N, DL, G, 64, 0.5f, DL, nl, DL, gl, DL, nl - 1, DL, DEV, sw));
  REJECT("out_starts holds", SELECT(DF, N, DL, G, 64, 0.5f, DL, nl, DL, gl - 1, DL, nl, DL, DEV, sw));
  REJECT("ws holds 255", SELECT(DF, N, DL, G, 64, 0.5f, DL, nl, DL, gl, DL, nl, DL, DEV, 255));
  {
    /* the sorted path (a graph above the workgroup limit): the key arrays alone outgrow this */
    const int64_t big = 10000;
    const size_t bl = (size_t)big * 8;
    REJECT("ws holds 4096", SELECT(DF, big, DL, G, big, 0.5f, DL, bl, DL, gl, DL, bl, DL, DEV, 4096));
    REJECT("ws holds 4096", SELECT(DF, big, DL, 1, big, 0.5f, DL, bl, DL, 16, DL, bl, DL, DEV, 4096));
  }
  ACCEPT(SELECT(DF, N, DL, G, 64, 1.0f, DL, nl, DL, gl, DL, nl, DL, DEV, sw));
  ACCEPT(SELECT(DF, N, DL, G, N, 0.001f, DL, nl, DL, gl, DL, nl, DL, DEV, sw));

  /* mp_pool_gate_f32 */
  const size_t xo = (size_t)K * F * 4;
#define GATE(x, ldx, s, perm, k, n, f, xout, ldo, xb, so) \
  mp_pool_gate_f32(x, ldx, s, DL, perm, k, n, f, 1.f, xout, ldo, xb, DL, so, NULL)
  REJECT("n = -1", GATE(DF, F, DF, DL, K, -1, F, DF, F, xo, DF));
  REJECT("k = 1001", GATE(DF, F, DF, DL, N + 1, N, F, DF, F, xo, DF));
  REJECT("k = -1", GATE(DF, F, DF, DL, -1, N, F, DF, F, xo, DF));
  REJECT("F = 0", GATE(DF, F, DF, DL, K, N, 0, DF, F, xo, DF));
  REJECT("ldx = 32", GATE(DF, F - 1, DF, DL, K, N, F, DF, F, xo, DF));
  REJECT("ldo = 32", GATE(DF, F, DF, DL, K, N, F, DF, F - 1, xo, DF));
  REJECT("x is NULL", GATE(NULL, F, DF, DL, K, N, F, DF, F, xo, DF));
  REJECT("score is NULL", GATE(DF, F, NULL, DL, K, N, F, DF, F, xo, DF));
  REJECT("perm is NULL", GATE(DF, F, DF, NULL, K, N, F, DF, F, xo, DF));
  REJECT("x_out is NULL", GATE(DF, F, DF, DL, K, N, F, NULL, F, xo, DF));
  REJECT("score_out is NULL", GATE(DF, F, DF, DL, K, N, F, DF, F, xo, NULL));
  REJECT("x_out holds", GATE(DF, F, DF, DL, K, N, F, DF, F, xo - 1, DF));
  REJECT("x_out holds", GATE(DF, F, DF, DL, K, N, F, DF, F + 7, xo, DF));
  ACCEPT(GATE(DF, F, DF, DL, K, N, F, DF, F, xo, DF));
  ACCEPT(mp_pool_gate_f32(DF, F, DF, NULL, DL, K, N, F, 2.5f, DF, F, xo, NULL, DF, NULL));

  /* mp_pool_gate_bwd_f32 */
  const size_t gx = (size_t)N * F * 4;
#define GATEB(gy, ldgy, x, ldx, s, inv, k, n, f, gxp, ldgx, gxb, gs, gsb) \
  mp_pool_gate_bwd_f32(gy, ldgy, DF, x, ldx, s, inv, k, n, f, 1.f, gxp, ldgx, gxb, gs, gsb, NULL)
  REJECT("n = -1", GATEB(DF, F, DF, F, DF, DL, K, -1, F, DF, F, gx, DF, nf));
  REJECT("k = 1001", GATEB(DF, F, DF, F, DF, DL, N + 1, N, F, DF, F, gx, DF, nf));
  REJECT("F = 0", GATEB(DF, F, DF, F, DF, DL, K, N, 0, DF, F, gx, DF, nf));
  REJECT("ldx = 32", GATEB(DF, F, DF, F - 1, DF, DL, K, N, F, DF, F, gx, DF, nf));
  REJECT("ldgy = 32", GATEB(DF, F - 1, DF, F, DF, DL, K, N, F, DF, F, gx, DF, nf));
  REJECT("ldgx = 32", GATEB(DF, F, DF, F, DF, DL, K, N, F, DF, F - 1, gx, DF, nf));
  REJECT("g_y is NULL", GATEB(NULL, F, DF, F, DF, DL, K, N, F, DF, F, gx, DF, nf));
  REJECT("x is NULL", GATEB(DF, F, NULL, F, DF, DL, K, N, F, DF, F, gx, DF, nf));
  REJECT("score is NULL", GATEB(DF, F, DF, F, NULL, DL, K, N, F, DF, F, gx, DF, nf));
  REJECT("inv is NULL", GATEB(DF, F, DF, F, DF, NULL, K, N, F, DF, F, gx, DF, nf));
  REJECT("g_x is NULL", GATEB(DF, F, DF, F, DF, DL, K, N, F, NULL, F, gx, DF, nf));
  REJECT("g_s is NULL", GATEB(DF, F, DF, F, DF, DL, K, N, F, DF, F, gx, NULL, nf));
  REJECT("g_x holds", GATEB(DF, F, DF, F, DF, DL, K, N, F, DF, F, gx - 1, DF, nf));
  REJECT("g_s holds", GATEB(DF, F, DF, F, DF, DL, K, N, F, DF, F, gx, DF, nf - 1));
  ACCEPT(GATEB(DF, F, DF, F, DF, DL, K, N, F, DF, F, gx, DF, nf));
  ACCEPT(mp_pool_gate_bwd_f32(DF, F, NULL, DF, F, DF, DL, K, N, F, 2.5f, DF, F, gx, DF, nf, NULL));

  /* mp_pool_inverse */
  REJECT("n = -1", mp_pool_inverse(DL, K, NULL, -1, DL, nl, NULL));
  REJECT("k = -1", mp_pool_inverse(DL, -1, NULL, N, DL, nl, NULL));
  REJECT("perm is NULL", mp_pool_inverse(NULL, K, NULL, N, DL, nl, NULL));
  REJECT("inv is NULL", mp_pool_inverse(DL, K, NULL, N, NULL, nl, NULL));
  REJECT("inv holds", mp_pool_inverse(DL, K, NULL, N, DL, nl - 1, NULL));
  ACCEPT(mp_pool_inverse(DL, K, DL, N, DL, nl, NULL));

  /* mp_pool_compact */
  const size_t cw = mp_pool_compact_workspace(N);
  REJECT("n = -1", mp_pool_compact(DB, -1, DL, nl, DL, DEV, cw, NULL));
  REJECT("count_dev is NULL", mp_pool_compact(DB, N, DL, nl, NULL, DEV, cw, NULL));
  REJECT("keep is NULL", mp_pool_compact(NULL, N, DL, nl, DL, DEV, cw, NULL));
  REJECT("out_pos is NULL", mp_pool_compact(DB, N, NULL, nl, DL, DEV, cw, NULL));
  REJECT("ws is NULL", mp_pool_compact(DB, N, DL, nl, DL, NULL, cw, NULL));
  REJECT("out_pos holds", mp_pool_compact(DB, N, DL, nl - 1, DL, DEV, cw, NULL));
  REJECT("ws holds 0", mp_pool_compact(DB, N, DL, nl, DL, DEV, 0, NULL));

  /* mp_pool_filter_adj */
  const size_t fw = mp_pool_filter_workspace(E);
#define FILTER(row, col, e, inv, n, orow, ocol, opos, ob, counts, ws, wb) \
  mp_pool_filter_adj(row, col, e, inv, n, orow, ocol, opos, ob, counts, ws, wb, NULL)
  REJECT("n_edges = -1", FILTER(DL, DL, -1, DL, N, DL, DL, DL, el, DL, DEV, fw));
  REJECT("n_nodes = -1", FILTER(DL, DL, E, DL, -1, DL, DL, DL, el, DL, DEV, fw));
  REJECT("counts is NULL", FILTER(DL, DL, E, DL, N, DL, DL, DL, el, NULL, DEV, fw));
  REJECT("row is NULL", FILTER(NULL, DL, E, DL, N, DL, DL, DL, el, DL, DEV, fw));
  REJECT("col is NULL", FILTER(DL, NULL, E, DL, N, DL, DL, DL, el, DL, DEV, fw));
  REJECT("inv is NULL", FILTER(DL, DL, E, NULL, N, DL, DL, DL, el, DL, DEV, fw));
  REJECT("out_row is NULL", FILTER(DL, DL, E, DL, N, NULL, DL, DL, el, DL, DEV, fw));
  REJECT("out_col is NULL", FILTER(DL, DL, E, DL, N, DL, NULL, DL, el, DL, DEV, fw));
  REJECT("out_pos is NULL", FILTER(DL, DL, E, DL, N, DL, DL, NULL, el, DL, DEV, fw));
  REJECT("ws is NULL", FILTER(DL, DL, E, DL, N, DL, DL, DL, el, DL, NULL, fw));
  REJECT("out_pos holds", FILTER(DL, DL, E, DL, N, DL, DL, DL, el - 1, DL, DEV, fw));
  REJECT("ws holds 1024", FILTER(DL, DL, E, DL, N, DL, DL, DL, el, DL, DEV, 1024));

  printf("abi_reject_pool: %d cases, %d failures\n", n_cases, n_fail);
  return n_fail ? 1 : 0;
}
