/*
 * abi_reject_spgemm.c -- argument / extent rejection harness for the sparse product's entry
 * points of include/mi355_mp.h (mp_spgemm_bin_cap, mp_spgemm_workspace, mp_spgemm_count,
 * mp_spgemm_fill_f32).
 *
 * Built and run as abi_reject_agnn.c is (`make asan_spgemm`, tests/test_spgemm_host.py): a REJECT
 * case expects -MP_ERR_ARG naming its one bad argument, an ACCEPT case passes every check.
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

int main(void) {
  const int64_t M = 300, K = 200, N = 500, NA = 4300, NB = 2100, NC = 9000, BIG = 0x7fffffffLL;
  const size_t RA = (size_t)(M + 1) * 4, RB = (size_t)(K + 1) * 4, RC = (size_t)(M + 1) * 8, CA = (size_t)NA * 4,
               CB = (size_t)NB * 4, ST = 32, OI = (size_t)NC * 8, OV = (size_t)NC * 4;
  const size_t WS = mp_spgemm_workspace(M);

  const int64_t wave = mp_spgemm_bin_cap(MP_SPGEMM_CAP_WAVE), wg = mp_spgemm_bin_cap(MP_SPGEMM_CAP_WG);
  const int answers = wave >= 1 && wg > wave && mp_spgemm_bin_cap(MP_SPGEMM_WINDOW) >= 32 &&
                      mp_spgemm_bin_cap(MP_SPGEMM_SLOTS_WAVE) >= 2 * wave &&
                      mp_spgemm_bin_cap(MP_SPGEMM_SLOTS_WG) >= 2 * wg && WS >= (size_t)M * 16 &&
                      mp_spgemm_workspace(2 * M) > WS && mp_spgemm_workspace(0) > 0 &&
                      mp_spgemm_workspace(-5) == mp_spgemm_workspace(0);
  ++n_cases;
  n_fail += !answers;
  printf("%s mp_spgemm_bin_cap / workspace answers\n", answers ? "ok  " : "FAIL");

#define CNT(ra, rab, ca, cab, rb, rbb, cb, cbb, m, k, n, na, nb, fl, rc, rcb, st, stb, ws, wsb) \
  mp_spgemm_count(ra, rab, ca, cab, rb, rbb, cb, cbb, m, k, n, na, nb, fl, rc, rcb, st, stb, ws, wsb, NULL)
  ACCEPT(CNT(DEVI, RA, DEVI, CA, DEVI, RB, DEVI, CB, M, K, N, NA, NB, 0, DEVL, RC, DEVL, ST, DEV, WS));
  ACCEPT(CNT(DEVI, RA, NULL, 0, DEVI, RB, NULL, 0, M, K, N, 0, 0, 0, DEVL, RC, DEVL, ST, DEV, WS));
  REJECT("rowptr_a is NULL", CNT(NULL, RA, DEVI, CA, DEVI, RB, DEVI, CB, M, K, N, NA, NB, 0, DEVL, RC, DEVL, ST, DEV, WS));
  REJECT("rowptr_a holds", CNT(DEVI, RA - 1, DEVI, CA, DEVI, RB, DEVI, CB, M, K, N, NA, NB, 0, DEVL, RC, DEVL, ST, DEV, WS));
  REJECT("col_a is NULL", CNT(DEVI, RA, NULL, CA, DEVI, RB, DEVI, CB, M, K, N, NA, NB, 0, DEVL, RC, DEVL, ST, DEV, WS));
  REJECT("col_a holds", CNT(DEVI, RA, DEVI, CA - 1, DEVI, RB, DEVI, CB, M, K, N, NA, NB, 0, DEVL, RC, DEVL, ST, DEV, WS));
  REJECT("rowptr_b is NULL", CNT(DEVI, RA, DEVI, CA, NULL, RB, DEVI, CB, M, K, N, NA, NB, 0, DEVL, RC, DEVL, ST, DEV, WS));
  REJECT("rowptr_b holds", CNT(DEVI, RA, DEVI, CA, DEVI, RB - 1, DEVI, CB, M, K, N, NA, NB, 0, DEVL, RC, DEVL, ST, DEV, WS));
  REJECT("col_b is NULL", CNT(DEVI, RA, DEVI, CA, DEVI, RB, NULL, CB, M, K, N, NA, NB, 0, DEVL, RC, DEVL, ST, DEV, WS));
  REJECT("col_b holds", CNT(DEVI, RA, DEVI, CA, DEVI, RB, DEVI, CB - 1, M, K, N, NA, NB, 0, DEVL, RC, DEVL, ST, DEV, WS));
  REJECT("m = -1", CNT(DEVI, RA, DEVI, CA, DEVI, RB, DEVI, CB, -1, K, N, NA, NB, 0, DEVL, RC, DEVL, ST, DEV, WS));
  REJECT("k = -1", CNT(DEVI, RA, DEVI, CA, DEVI, RB, DEVI, CB, M, -1, N, NA, NB, 0, DEVL, RC, DEVL, ST, DEV, WS));
  REJECT("n = -1", CNT(DEVI, RA, DEVI, CA, DEVI, RB, DEVI, CB, M, K, -1, NA, NB, 0, DEVL, RC, DEVL, ST, DEV, WS));
  REJECT("nnz_a = -1", CNT(DEVI, RA, DEVI, CA, DEVI, RB, DEVI, CB, M, K, N, -1, NB, 0, DEVL, RC, DEVL, ST, DEV, WS));
  REJECT("nnz_b = -1", CNT(DEVI, RA, DEVI, CA, DEVI, RB, DEVI, CB, M, K, N, NA, -1, 0, DEVL, RC, DEVL, ST, DEV, WS));
  REJECT("m = 2147483647", CNT(DEVI, RA, DEVI, CA, DEVI, RB, DEVI, CB, BIG, K, N, NA, NB, 0, DEVL, RC, DEVL, ST, DEV, WS));
  REJECT("k = 2147483647", CNT(DEVI, RA, DEVI, CA, DEVI, RB, DEVI, CB, M, BIG, N, NA, NB, 0, DEVL, RC, DEVL, ST, DEV, WS));
  REJECT("n = 2147483647", CNT(DEVI, RA, DEVI, CA, DEVI, RB, DEVI, CB, M, K, BIG, NA, NB, 0, DEVL, RC, DEVL, ST, DEV, WS));
  REJECT("nnz_a = 2147483647", CNT(DEVI, RA, DEVI, CA, DEVI, RB, DEVI, CB, M, K, N, BIG, NB, 0, DEVL, RC, DEVL, ST, DEV, WS));
  REJECT("nnz_b = 4294967296", CNT(DEVI, RA, DEVI, CA, DEVI, RB, DEVI, CB, M, K, N, NA, 1LL << 32, 0, DEVL, RC, DEVL, ST, DEV, WS));
  REJECT("unknown flags", CNT(DEVI, RA, DEVI, CA, DEVI, RB, DEVI, CB, M, K, N, NA, NB, 2, DEVL, RC, DEVL, ST, DEV, WS));
  REJECT("rowptr_c is NULL", CNT(DEVI, RA, DEVI, CA, DEVI, RB, DEVI, CB, M, K, N, NA, NB, 0, NULL, RC, DEVL, ST, DEV, WS));
  REJECT("rowptr_c holds", CNT(DEVI, RA, DEVI, CA, DEVI, RB, DEVI, CB, M, K, N, NA, NB, 0, DEVL, RC - 1, DEVL, ST, DEV, WS));
  REJECT("stats is NULL", CNT(DEVI, RA, DEVI, CA, DEVI, RB, DEVI, CB, M, K, N, NA, NB, 0, DEVL, RC, NULL, ST, DEV, WS));
  REJECT("stats holds", CNT(DEVI, RA, DEVI, CA, DEVI, RB, DEVI, CB, M, K, N, NA, NB, 0, DEVL, RC, DEVL, ST - 1, DEV, WS));
  REJECT("ws is NULL", CNT(DEVI, RA, DEVI, CA, DEVI, RB, DEVI, CB, M, K, N, NA, NB, 0, DEVL, RC, DEVL, ST, NULL, WS));
  REJECT("ws holds", CNT(DEVI, RA, DEVI, CA, DEVI, RB, DEVI, CB, M, K, N, NA, NB, 0, DEVL, RC, DEVL, ST, DEV, WS - 1));

/* the operands' shared part is good; one of the fill pass's own arguments is bad */
#define FIL(ea, eab, va, vab, eb, ebb, vb, vbb, m, na, fl, rc, rcb, nc, orow, orb, ocol, ocb, oval, ovb, ws, wsb)       \
  mp_spgemm_fill_f32(DEVI, RA, DEVI, CA, ea, eab, va, vab, DEVI, RB, DEVI, CB, eb, ebb, vb, vbb, m, K, N, na, NB, fl, rc, \
                     rcb, nc, orow, orb, ocol, ocb, oval, ovb, ws, wsb, NULL)
  ACCEPT(FIL(DEVI, CA, DEVF, CA, DEVI, CB, DEVF, CB, M, NA, 0, DEVL, RC, NC, DEVL, OI, DEVL, OI, DEVF, OV, DEV, WS));
  REJECT("eid_a is NULL", FIL(NULL, CA, DEVF, CA, DEVI, CB, DEVF, CB, M, NA, 0, DEVL, RC, NC, DEVL, OI, DEVL, OI, DEVF, OV, DEV, WS));
  REJECT("eid_a holds", FIL(DEVI, CA - 1, DEVF, CA, DEVI, CB, DEVF, CB, M, NA, 0, DEVL, RC, NC, DEVL, OI, DEVL, OI, DEVF, OV, DEV, WS));
  REJECT("val_a is NULL", FIL(DEVI, CA, NULL, CA, DEVI, CB, DEVF, CB, M, NA, 0, DEVL, RC, NC, DEVL, OI, DEVL, OI, DEVF, OV, DEV, WS));
  REJECT("val_a holds", FIL(DEVI, CA, DEVF, CA - 1, DEVI, CB, DEVF, CB, M, NA, 0, DEVL, RC, NC, DEVL, OI, DEVL, OI, DEVF, OV, DEV, WS));
  REJECT("eid_b is NULL", FIL(DEVI, CA, DEVF, CA, NULL, CB, DEVF, CB, M, NA, 0, DEVL, RC, NC, DEVL, OI, DEVL, OI, DEVF, OV, DEV, WS));
  REJECT("eid_b holds", FIL(DEVI, CA, DEVF, CA, DEVI, CB - 1, DEVF, CB, M, NA, 0, DEVL, RC, NC, DEVL, OI, DEVL, OI, DEVF, OV, DEV, WS));
  REJECT("val_b is NULL", FIL(DEVI, CA, DEVF, CA, DEVI, CB, NULL, CB, M, NA, 0, DEVL, RC, NC, DEVL, OI, DEVL, OI, DEVF, OV, DEV, WS));
  REJECT("val_b holds", FIL(DEVI, CA, DEVF, CA, DEVI, CB, DEVF, CB - 1, M, NA, 0, DEVL, RC, NC, DEVL, OI, DEVL, OI, DEVF, OV, DEV, WS));
  REJECT("rowptr_c is NULL", FIL(DEVI, CA, DEVF, CA, DEVI, CB, DEVF, CB, M, NA, 0, NULL, RC, NC, DEVL, OI, DEVL, OI, DEVF, OV, DEV, WS));
  REJECT("rowptr_c holds", FIL(DEVI, CA, DEVF, CA, DEVI, CB, DEVF, CB, M, NA, 0, DEVL, RC - 1, NC, DEVL, OI, DEVL, OI, DEVF, OV, DEV, WS));
  REJECT("nnz_c = -1", FIL(DEVI, CA, DEVF, CA, DEVI, CB, DEVF, CB, M, NA, 0, DEVL, RC, -1, DEVL, OI, DEVL, OI, DEVF, OV, DEV, WS));
  REJECT("nnz_c = 2147483647", FIL(DEVI, CA, DEVF, CA, DEVI, CB, DEVF, CB, M, NA, 0, DEVL, RC, BIG, DEVL, OI, DEVL, OI, DEVF, OV, DEV, WS));
  REJECT("out_row is NULL", FIL(DEVI, CA, DEVF, CA, DEVI, CB, DEVF, CB, M, NA, 0, DEVL, RC, NC, NULL, OI, DEVL, OI, DEVF, OV, DEV, WS));
  REJECT("out_row holds", FIL(DEVI, CA, DEVF, CA, DEVI, CB, DEVF, CB, M, NA, 0, DEVL, RC, NC, DEVL, OI - 1, DEVL, OI, DEVF, OV, DEV, WS));
  REJECT("out_col is NULL", FIL(DEVI, CA, DEVF, CA, DEVI, CB, DEVF, CB, M, NA, 0, DEVL, RC, NC, DEVL, OI, NULL, OI, DEVF, OV, DEV, WS));
  REJECT("out_col holds", FIL(DEVI, CA, DEVF, CA, DEVI, CB, DEVF, CB, M, NA, 0, DEVL, RC, NC, DEVL, OI, DEVL, OI - 1, DEVF, OV, DEV, WS));
  REJECT("out_val is NULL", FIL(DEVI, CA, DEVF, CA, DEVI, CB, DEVF, CB, M, NA, 0, DEVL, RC, NC, DEVL, OI, DEVL, OI, NULL, OV, DEV, WS));
  REJECT("out_val holds", FIL(DEVI, CA, DEVF, CA, DEVI, CB, DEVF, CB, M, NA, 0, DEVL, RC, NC, DEVL, OI, DEVL, OI, DEVF, OV - 1, DEV, WS));
  REJECT("ws is NULL", FIL(DEVI, CA, DEVF, CA, DEVI, CB, DEVF, CB, M, NA, 0, DEVL, RC, NC, DEVL, OI, DEVL, OI, DEVF, OV, NULL, WS));
  REJECT("ws holds", FIL(DEVI, CA, DEVF, CA, DEVI, CB, DEVF, CB, M, NA, 0, DEVL, RC, NC, DEVL, OI, DEVL, OI, DEVF, OV, DEV, WS - 1));

  printf("abi_reject_spgemm: %d cases, %d failures\n", n_cases, n_fail);
  return n_fail ? 1 : 0;
}
