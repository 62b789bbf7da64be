/*
 * abi_reject_dna.c -- argument / extent rejection harness for the DNAConv entry
 * points of include/mi355_mp.h (mp_dna_ok, mp_dna_max_layers,
 * mp_dna_split_chunk, mp_dna_workspace, mp_dna_aggregate_f32,
 * mp_dna_backward_dst_f32, mp_dna_backward_src_f32, mp_dna_dropout_keep).
 *
 * Built against the host-only AddressSanitizer build of the library
 * (`make -C pytorch_geometric-1_amd/csrc asan_dna`) and run as a plain program
 * on a machine with no GPU by tests/test_dna_host.py.  Every case calls one
 * entry point with one bad argument and expects -MP_ERR_ARG and an error text
 * naming the problem -- no launch, no device access, no host memory error (ASAN
 * aborts the run on one).  ACCEPT cases pass every check (the call then fails
 * at its first HIP call, -MP_ERR_HIP, as there is no GPU): the boundary is the
 * documented one, not a looser one.
 * Output: one line per case, then "abi_reject_dna: N cases, M failures".
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "mi355_mp.h"

static int n_cases = 0, n_fail = 0;

#define DEV ((void*)(uintptr_t)0x7f0000000000ull) /* fake device pointer, never dereferenced */
#define DEVF ((float*)DEV)
#define DEVI ((int32_t*)DEV)
#define DEVB ((uint8_t*)DEV)

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

/* the workspace every call of the macros below passes (a row-walking CSR needs none) */
static void* WSP = NULL;
static size_t WSB = 0;

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
  const int64_t N = 257, M = 300, E = 3000; /* N rows, M columns */
  const int T = 5, H = 3, C = 66, R = 5 * 66;
  const size_t QN = (size_t)N * C * 4, QM = (size_t)M * C * 4; /* [., C], contiguous */
  const size_t KN = (size_t)N * R * 4, KM = (size_t)M * R * 4; /* [., T, C], contiguous */
  const size_t LB = (size_t)E * H * 4;                         /* lse [E, H] */
  mp_csr g = graph(N, E, (int32_t)M);

  /* mp_dna_ok / mp_dna_max_layers: the example's shape and the limits on each side */
  ++n_cases;
  if (!(mp_dna_ok(5, 8, 128) == 1 && mp_dna_ok(1, 1, 1) == 1 && mp_dna_ok(0, 1, 1) == 0 && mp_dna_ok(1, 0, 1) == 0 &&
        mp_dna_ok(1, 1, 0) == 0 && mp_dna_ok(-1, 1, 1) == 0 && mp_dna_ok(2, 3, 10) == 0 && mp_dna_ok(48, 16, 16) == 1 &&
        mp_dna_ok(49, 16, 16) == 0 && mp_dna_ok(48, 1, 64) == 1 && mp_dna_ok(24, 1, 65) == 1 &&
        mp_dna_ok(25, 1, 65) == 0 && mp_dna_ok(12, 1, 256) == 1 && mp_dna_ok(13, 1, 256) == 0 &&
        mp_dna_ok(1, 1, 257) == 0 && mp_dna_ok(1, 2, 514) == 0 && mp_dna_max_layers(8, 128) == 48 &&
        mp_dna_max_layers(1, 65) == 24 && mp_dna_max_layers(1, 130) == 16 && mp_dna_max_layers(1, 256) == 12 &&
        mp_dna_max_layers(1, 257) == 0 && mp_dna_max_layers(3, 10) == 0 && mp_dna_max_layers(0, 8) == 0 &&
        mp_dna_max_layers(4, 0) == 0 && mp_dna_ok((int32_t)mp_dna_max_layers(7, 154), 7, 154) == 1 &&
        mp_dna_ok((int32_t)mp_dna_max_layers(7, 154) + 1, 7, 154) == 0)) {
    printf("FAIL mp_dna_ok limits\n");
    ++n_fail;
  } else {
    printf("ok   mp_dna_ok limits\n");
  }

  /* forward: q, out by row (N), k, v by column (M) */
#define AGG(g_, q, ldq, qb, k, ldk, kb, v, ldv, vb, nrm, nn, T_, H_, C_, p, out, ldo, ob, lse, lb) \
  mp_dna_aggregate_f32(g_, q, ldq, qb, k, ldk, kb, v, ldv, vb, nrm, nn, T_, H_, C_, 7, p, out, ldo, ob, lse, lb, WSP, WSB, NULL)
  REJECT("g is NULL", AGG(NULL, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
  REJECT("q is NULL", AGG(&g, NULL, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
  REJECT("k is NULL", AGG(&g, DEVF, C, QN, NULL, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
  REJECT("v is NULL", AGG(&g, DEVF, C, QN, DEVF, R, KM, NULL, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
  REJECT("out is NULL", AGG(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, NULL, C, QN, DEVF, LB));
  REJECT("ld of q", AGG(&g, DEVF, C - 1, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
  REJECT("ld of k", AGG(&g, DEVF, C, QN, DEVF, R - 1, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
  REJECT("ld of v", AGG(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R - 1, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
  REJECT("ld of out", AGG(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C - 1, QN, DEVF, LB));
  REJECT("q holds", AGG(&g, DEVF, C, QN - 1, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
  REJECT("k holds", AGG(&g, DEVF, C, QN, DEVF, R, KM - 1, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
  REJECT("k holds", AGG(&g, DEVF, C, QN, DEVF, R, KN, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB)); /* sized by rows */
  REJECT("v holds", AGG(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM - 1, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
  REJECT("v holds", AGG(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R + 1, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
  REJECT("out holds", AGG(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN - 1, DEVF, LB));
  REJECT("out holds", AGG(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C + 3, QN, DEVF, LB));
  REJECT("lse holds", AGG(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB - 1));
  REJECT("n_norm", AGG(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E - 1, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
  REJECT("T = 0", AGG(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, 0, H, C, 0.f, DEVF, C, QN, DEVF, LB));
  REJECT("H = 0", AGG(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, 0, C, 0.f, DEVF, C, QN, DEVF, LB));
  REJECT("C = -4", AGG(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, -4, 0.f, DEVF, C, QN, DEVF, LB));
  REJECT("no multiple", AGG(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, 4, C, 0.f, DEVF, C, QN, DEVF, LB));
  REJECT("above the limit", AGG(&g, DEVF, C, QN, DEVF, 49 * C, (size_t)1 << 40, DEVF, 49 * C, (size_t)1 << 40, DEVF, E, 49, H, C,
                                0.f, DEVF, C, QN, DEVF, LB));
  REJECT("above the limit", AGG(&g, DEVF, 257, (size_t)1 << 40, DEVF, 257, (size_t)1 << 40, DEVF, 257, (size_t)1 << 40, DEVF, E, 1,
                                1, 257, 0.f, DEVF, 257, (size_t)1 << 40, DEVF, LB));
  REJECT("dropout p", AGG(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 1.f, DEVF, C, QN, DEVF, LB));
  REJECT("dropout p", AGG(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, -0.5f, DEVF, C, QN, DEVF, LB));
  {
    mp_csr b = g;
    b.col = NULL;
    REJECT("col", AGG(&b, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
    b = g;
    b.eid = NULL;
    REJECT("eid", AGG(&b, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
    b = g;
    b.rowptr = NULL;
    REJECT("rowptr", AGG(&b, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
    b = g;
    b.n_cols = 0;
    REJECT("n_cols", AGG(&b, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
    b = g;
    b.n_rows = -1;
    REJECT("negative", AGG(&b, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
    b = g;
    b.n_ids = E + 5; /* the slots are a subset of E + 5 edges: norm and lse must cover them all */
    REJECT("n_norm", AGG(&b, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
    REJECT("lse holds", AGG(&b, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E + 5, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
    ACCEPT(AGG(&b, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E + 5, T, H, C, 0.f, DEVF, C, QN, DEVF, LB + 5 * H * 4));
  }
  ACCEPT(AGG(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
  ACCEPT(AGG(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, NULL, 0, T, H, C, 0.5f, DEVF, C, QN, NULL, 0)); /* norm = 1, no lse */
  /* K | V in one buffer [M, 2, T, C]: ld = 2 R, the extents from each pointer on */
  ACCEPT(AGG(&g, DEVF, C + 2, QN + (N - 1) * 8, DEVF, 2 * R, 2 * KM, DEVF, 2 * R, 2 * KM - (size_t)R * 4, DEVF, E, T, H, C, 0.f, DEVF,
             C + 1, QN + (N - 1) * 4, DEVF, LB));
  REJECT("v holds", AGG(&g, DEVF, C, QN, DEVF, 2 * R, 2 * KM, DEVF, 2 * R, 2 * KM - (size_t)R * 4 - 1, DEVF, E, T, H, C, 0.f, DEVF, C,
                        QN, DEVF, LB));
  ACCEPT(AGG(&g, DEVF, 256, (size_t)N * 1024, DEVF, 12 * 256, (size_t)M * 12 * 1024, DEVF, 12 * 256, (size_t)M * 12 * 1024, DEVF, E, 12,
             1, 256, 0.f, DEVF, 256, (size_t)N * 1024, DEVF, (size_t)E * 4));

  /* backward over the destination CSR: gout, dq by row */
#define DST(g_, q, ldq, qb, k, ldk, kb, v, ldv, vb, nrm, nn, go, ldg, gb, lse, lb, T_, H_, C_, p, dq, lddq, dqb) \
  mp_dna_backward_dst_f32(g_, q, ldq, qb, k, ldk, kb, v, ldv, vb, nrm, nn, go, ldg, gb, lse, lb, T_, H_, C_, 7, p, dq, lddq, dqb, WSP, WSB, NULL)
  REJECT("g is NULL", DST(NULL, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, DEVF, C, QN, DEVF, LB, T, H, C, 0.f, DEVF, C, QN));
  REJECT("q is NULL", DST(&g, NULL, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, DEVF, C, QN, DEVF, LB, T, H, C, 0.f, DEVF, C, QN));
  REJECT("k is NULL", DST(&g, DEVF, C, QN, NULL, R, KM, DEVF, R, KM, DEVF, E, DEVF, C, QN, DEVF, LB, T, H, C, 0.f, DEVF, C, QN));
  REJECT("v is NULL", DST(&g, DEVF, C, QN, DEVF, R, KM, NULL, R, KM, DEVF, E, DEVF, C, QN, DEVF, LB, T, H, C, 0.f, DEVF, C, QN));
  REJECT("gout is NULL", DST(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, NULL, C, QN, DEVF, LB, T, H, C, 0.f, DEVF, C, QN));
  REJECT("lse is NULL", DST(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, DEVF, C, QN, NULL, LB, T, H, C, 0.f, DEVF, C, QN));
  REJECT("dq is NULL", DST(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, DEVF, C, QN, DEVF, LB, T, H, C, 0.f, NULL, C, QN));
  REJECT("ld of gout", DST(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, DEVF, C - 1, QN, DEVF, LB, T, H, C, 0.f, DEVF, C, QN));
  REJECT("ld of dq", DST(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, DEVF, C, QN, DEVF, LB, T, H, C, 0.f, DEVF, C - 1, QN));
  REJECT("ld of k", DST(&g, DEVF, C, QN, DEVF, R - 1, KM, DEVF, R, KM, DEVF, E, DEVF, C, QN, DEVF, LB, T, H, C, 0.f, DEVF, C, QN));
  REJECT("gout holds", DST(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, DEVF, C, QN - 1, DEVF, LB, T, H, C, 0.f, DEVF, C, QN));
  REJECT("dq holds", DST(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, DEVF, C, QN, DEVF, LB, T, H, C, 0.f, DEVF, C, QN - 1));
  REJECT("k holds", DST(&g, DEVF, C, QN, DEVF, R, KN, DEVF, R, KM, DEVF, E, DEVF, C, QN, DEVF, LB, T, H, C, 0.f, DEVF, C, QN));
  REJECT("lse holds", DST(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, DEVF, C, QN, DEVF, LB - 4, T, H, C, 0.f, DEVF, C, QN));
  REJECT("n_norm", DST(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, 0, DEVF, C, QN, DEVF, LB, T, H, C, 0.f, DEVF, C, QN));
  REJECT("T = -1", DST(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, DEVF, C, QN, DEVF, LB, -1, H, C, 0.f, DEVF, C, QN));
  REJECT("no multiple", DST(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, DEVF, C, QN, DEVF, LB, T, 5, C, 0.f, DEVF, C, QN));
  REJECT("dropout p", DST(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, DEVF, C, QN, DEVF, LB, T, H, C, 1.5f, DEVF, C, QN));
  ACCEPT(DST(&g, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, DEVF, C, QN, DEVF, LB, T, H, C, 0.8f, DEVF, C, QN));
  ACCEPT(DST(&g, DEVF, C, QN, DEVF, R + 2, KM + (M - 1) * 8, DEVF, R, KM, NULL, 0, DEVF, C + 1, QN + (N - 1) * 4, DEVF, LB, T, H, C,
             0.f, DEVF, C + 7, QN + (N - 1) * 28));

  /* backward over the source-keyed CSR: k, v, dk, dv by row (N), q, gout by column (M) */
#define SRC(g_, q, ldq, qb, k, ldk, kb, v, ldv, vb, nrm, nn, go, ldg, gb, lse, lb, T_, H_, C_, p, dk, lddk, dkb, dv, lddv, dvb)  \
  mp_dna_backward_src_f32(g_, q, ldq, qb, k, ldk, kb, v, ldv, vb, nrm, nn, go, ldg, gb, lse, lb, T_, H_, C_, 7, p, dk, lddk, dkb, dv, \
                          lddv, dvb, WSP, WSB, NULL)
  REJECT("g is NULL", SRC(NULL, DEVF, C, QM, DEVF, R, KN, DEVF, R, KN, DEVF, E, DEVF, C, QM, DEVF, LB, T, H, C, 0.f, DEVF, R, KN, DEVF, R, KN));
  REJECT("q is NULL", SRC(&g, NULL, C, QM, DEVF, R, KN, DEVF, R, KN, DEVF, E, DEVF, C, QM, DEVF, LB, T, H, C, 0.f, DEVF, R, KN, DEVF, R, KN));
  REJECT("k is NULL", SRC(&g, DEVF, C, QM, NULL, R, KN, DEVF, R, KN, DEVF, E, DEVF, C, QM, DEVF, LB, T, H, C, 0.f, DEVF, R, KN, DEVF, R, KN));
  REJECT("v is NULL", SRC(&g, DEVF, C, QM, DEVF, R, KN, NULL, R, KN, DEVF, E, DEVF, C, QM, DEVF, LB, T, H, C, 0.f, DEVF, R, KN, DEVF, R, KN));
  REJECT("gout is NULL", SRC(&g, DEVF, C, QM, DEVF, R, KN, DEVF, R, KN, DEVF, E, NULL, C, QM, DEVF, LB, T, H, C, 0.f, DEVF, R, KN, DEVF, R, KN));
  REJECT("lse is NULL", SRC(&g, DEVF, C, QM, DEVF, R, KN, DEVF, R, KN, DEVF, E, DEVF, C, QM, NULL, LB, T, H, C, 0.f, DEVF, R, KN, DEVF, R, KN));
  REJECT("dk is NULL", SRC(&g, DEVF, C, QM, DEVF, R, KN, DEVF, R, KN, DEVF, E, DEVF, C, QM, DEVF, LB, T, H, C, 0.f, NULL, R, KN, DEVF, R, KN));
  REJECT("dv is NULL", SRC(&g, DEVF, C, QM, DEVF, R, KN, DEVF, R, KN, DEVF, E, DEVF, C, QM, DEVF, LB, T, H, C, 0.f, DEVF, R, KN, NULL, R, KN));
  REJECT("q holds", SRC(&g, DEVF, C, QN, DEVF, R, KN, DEVF, R, KN, DEVF, E, DEVF, C, QM, DEVF, LB, T, H, C, 0.f, DEVF, R, KN, DEVF, R, KN)); /* sized by rows */
  REJECT("gout holds", SRC(&g, DEVF, C, QM, DEVF, R, KN, DEVF, R, KN, DEVF, E, DEVF, C, QM - 1, DEVF, LB, T, H, C, 0.f, DEVF, R, KN, DEVF, R, KN));
  REJECT("k holds", SRC(&g, DEVF, C, QM, DEVF, R, KN - 1, DEVF, R, KN, DEVF, E, DEVF, C, QM, DEVF, LB, T, H, C, 0.f, DEVF, R, KN, DEVF, R, KN));
  REJECT("v holds", SRC(&g, DEVF, C, QM, DEVF, R, KN, DEVF, R, KN - 1, DEVF, E, DEVF, C, QM, DEVF, LB, T, H, C, 0.f, DEVF, R, KN, DEVF, R, KN));
  REJECT("dk holds", SRC(&g, DEVF, C, QM, DEVF, R, KN, DEVF, R, KN, DEVF, E, DEVF, C, QM, DEVF, LB, T, H, C, 0.f, DEVF, R, KN - 1, DEVF, R, KN));
  REJECT("dv holds", SRC(&g, DEVF, C, QM, DEVF, R, KN, DEVF, R, KN, DEVF, E, DEVF, C, QM, DEVF, LB, T, H, C, 0.f, DEVF, R, KN, DEVF, R + 1, KN));
  REJECT("ld of dk", SRC(&g, DEVF, C, QM, DEVF, R, KN, DEVF, R, KN, DEVF, E, DEVF, C, QM, DEVF, LB, T, H, C, 0.f, DEVF, R - 1, KN, DEVF, R, KN));
  REJECT("ld of dv", SRC(&g, DEVF, C, QM, DEVF, R, KN, DEVF, R, KN, DEVF, E, DEVF, C, QM, DEVF, LB, T, H, C, 0.f, DEVF, R, KN, DEVF, R - 1, KN));
  REJECT("ld of q", SRC(&g, DEVF, C - 1, QM, DEVF, R, KN, DEVF, R, KN, DEVF, E, DEVF, C, QM, DEVF, LB, T, H, C, 0.f, DEVF, R, KN, DEVF, R, KN));
  REJECT("lse holds", SRC(&g, DEVF, C, QM, DEVF, R, KN, DEVF, R, KN, DEVF, E, DEVF, C, QM, DEVF, 0, T, H, C, 0.f, DEVF, R, KN, DEVF, R, KN));
  REJECT("n_norm", SRC(&g, DEVF, C, QM, DEVF, R, KN, DEVF, R, KN, DEVF, E - 1, DEVF, C, QM, DEVF, LB, T, H, C, 0.f, DEVF, R, KN, DEVF, R, KN));
  REJECT("above the limit", SRC(&g, DEVF, C, QM, DEVF, 25 * C, (size_t)1 << 40, DEVF, 25 * C, (size_t)1 << 40, DEVF, E, DEVF, C, QM, DEVF,
                                (size_t)E * 4, 25, 1, C, 0.f, DEVF, 25 * C, (size_t)1 << 40, DEVF, 25 * C, (size_t)1 << 40));
  REJECT("dropout p", SRC(&g, DEVF, C, QM, DEVF, R, KN, DEVF, R, KN, DEVF, E, DEVF, C, QM, DEVF, LB, T, H, C, 1.f, DEVF, R, KN, DEVF, R, KN));
  ACCEPT(SRC(&g, DEVF, C, QM, DEVF, R, KN, DEVF, R, KN, DEVF, E, DEVF, C, QM, DEVF, LB, T, H, C, 0.5f, DEVF, R, KN, DEVF, R, KN));
  ACCEPT(SRC(&g, DEVF, C, QM, DEVF, 24 * C, (size_t)N * 24 * C * 4, DEVF, 24 * C, (size_t)N * 24 * C * 4, DEVF, E, DEVF, C, QM, DEVF,
             (size_t)E * 4, 24, 1, C, 0.f, DEVF, 24 * C, (size_t)N * 24 * C * 4, DEVF, 24 * C + 5, (size_t)N * 24 * C * 4 + (N - 1) * 20));

  /* a schedule of chunk >= mp_dna_split_chunk(): the kernels walk tasks, the schedule arrays and the slab are required */
  {
    mp_csr t = g;
    t.wave_row = DEVI;
    t.wave_slot = DEVI;
    t.split_waves = DEVI;
    t.chunk = 64;
    t.n_waves = 40;
    t.n_split = 3;
    const size_t small = mp_dna_workspace(&g, C), fwd = mp_dna_workspace(&t, C), bsrc = mp_dna_workspace(&t, 2 * R);
    ++n_cases;
    mp_csr t32 = t;
    t32.chunk = 32;
    if (!(mp_dna_split_chunk() == 64 && fwd >= (size_t)2 * 40 * C * 4 && fwd > small && bsrc >= (size_t)2 * 40 * 2 * R * 4 &&
          mp_dna_workspace(&t32, C) == small && mp_dna_workspace(NULL, C) == small && mp_dna_workspace(&t, 0) == small)) {
      printf("FAIL mp_dna_workspace\n");
      ++n_fail;
    } else {
      printf("ok   mp_dna_workspace\n");
    }
    WSP = NULL, WSB = fwd;
    REJECT("ws is NULL", AGG(&t, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
    REJECT("ws is NULL", DST(&t, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, DEVF, C, QN, DEVF, LB, T, H, C, 0.f, DEVF, C, QN));
    REJECT("ws is NULL", SRC(&t, DEVF, C, QM, DEVF, R, KN, DEVF, R, KN, DEVF, E, DEVF, C, QM, DEVF, LB, T, H, C, 0.f, DEVF, R, KN, DEVF, R, KN));
    WSP = DEV, WSB = fwd - 1;
    REJECT("ws holds", AGG(&t, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
    REJECT("ws holds", DST(&t, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, DEVF, C, QN, DEVF, LB, T, H, C, 0.f, DEVF, C, QN));
    WSB = bsrc - 1;
    REJECT("ws holds", SRC(&t, DEVF, C, QM, DEVF, R, KN, DEVF, R, KN, DEVF, E, DEVF, C, QM, DEVF, LB, T, H, C, 0.f, DEVF, R, KN, DEVF, R, KN));
    WSB = fwd; /* sized for the forward */
    REJECT("ws holds", SRC(&t, DEVF, C, QM, DEVF, R, KN, DEVF, R, KN, DEVF, E, DEVF, C, QM, DEVF, LB, T, H, C, 0.f, DEVF, R, KN, DEVF, R, KN));
    WSB = bsrc;
    mp_csr b = t;
    b.wave_slot = NULL;
    REJECT("wave_slot", AGG(&b, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
    b = t;
    b.split_waves = NULL;
    REJECT("split_waves", DST(&b, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, DEVF, C, QN, DEVF, LB, T, H, C, 0.f, DEVF, C, QN));
    b = t;
    b.n_waves = 0;
    REJECT("n_waves", SRC(&b, DEVF, C, QM, DEVF, R, KN, DEVF, R, KN, DEVF, E, DEVF, C, QM, DEVF, LB, T, H, C, 0.f, DEVF, R, KN, DEVF, R, KN));
    b = t;
    b.n_split = 41;
    REJECT("n_split", AGG(&b, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
    ACCEPT(AGG(&t, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
    ACCEPT(DST(&t, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, DEVF, C, QN, DEVF, LB, T, H, C, 0.f, DEVF, C, QN));
    ACCEPT(SRC(&t, DEVF, C, QM, DEVF, R, KN, DEVF, R, KN, DEVF, E, DEVF, C, QM, DEVF, LB, T, H, C, 0.f, DEVF, R, KN, DEVF, R, KN));
    b = t;
    b.n_split = 0;
    b.split_waves = NULL;
    ACCEPT(AGG(&b, DEVF, C, QN, DEVF, R, KM, DEVF, R, KM, DEVF, E, T, H, C, 0.f, DEVF, C, QN, DEVF, LB));
    WSP = NULL, WSB = 0;
  }

  /* the keep mask: n_edges * H * T bytes */
  REJECT("dropout p", mp_dna_dropout_keep(1, 0.f, H, T, E, DEVB, (size_t)E * H * T, NULL));
  REJECT("dropout p", mp_dna_dropout_keep(1, 1.f, H, T, E, DEVB, (size_t)E * H * T, NULL));
  REJECT("H = 0", mp_dna_dropout_keep(1, 0.5f, 0, T, E, DEVB, (size_t)E * H * T, NULL));
  REJECT("T = 0", mp_dna_dropout_keep(1, 0.5f, H, 0, E, DEVB, (size_t)E * H * T, NULL));
  REJECT("n_edges", mp_dna_dropout_keep(1, 0.5f, H, T, -1, DEVB, (size_t)E * H * T, NULL));
  REJECT("keep is NULL", mp_dna_dropout_keep(1, 0.5f, H, T, E, NULL, (size_t)E * H * T, NULL));
  REJECT("keep holds", mp_dna_dropout_keep(1, 0.5f, H, T, E, DEVB, (size_t)E * H * T - 1, NULL));
  REJECT("too large", mp_dna_dropout_keep(1, 0.5f, 1 << 20, 1 << 20, E, DEVB, (size_t)1 << 60, NULL));
  ACCEPT(mp_dna_dropout_keep(1, 0.5f, H, T, E, DEVB, (size_t)E * H * T, NULL));
  ACCEPT(mp_dna_dropout_keep(1, 0.5f, H, T, 0, NULL, 0, NULL));

  printf("abi_reject_dna: %d cases, %d failures\n", n_cases, n_fail);
  return n_fail ? 1 : 0;
}
