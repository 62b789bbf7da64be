/*
 * abi_reject_ggc.c -- argument / extent rejection harness for GatedGraphConv's GRU cell
 * entry points of include/mi355_mp.h (mp_gru_ok, mp_gru_width, mp_gru_pack_bytes,
 * mp_gru_pack_f32, mp_gru_cell_f32, mp_gru_cell_bwd_f32).
 *
 * Built against the host-only AddressSanitizer build (`make asan_ggc`) and run as a plain
 * program with no GPU by tests/test_ggc_host.py.  A REJECT case passes one bad argument and
 * expects -MP_ERR_ARG with a text naming it, before any launch; an ACCEPT case passes every
 * check and fails at its first HIP call.  Each extent and each limit is rejected once.
 * Output: one line per case, then "abi_reject_ggc: N cases, M failures".
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "mi355_mp.h"

static int n_cases = 0, n_fail = 0;

#define DEV ((void*)(uintptr_t)0x7f0000000000ull) /* fake device pointer, never dereferenced */
#define DEVF ((float*)DEV)

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
  const int64_t N = 193;
  const int C = 20, P = 32; /* C rounded up to 16 */
  const size_t ROWS = (size_t)N * P * 4, G4 = (size_t)N * 4 * P * 4;
  const size_t WB = (size_t)C * 3 * C * 4, BB = (size_t)3 * C * 4, PK = mp_gru_pack_bytes(C);
  const int answers = mp_gru_ok(0) == 0 && mp_gru_ok(1) == 1 && mp_gru_ok(128) == 1 && mp_gru_ok(129) == 0 &&
                      mp_gru_width(1) == 16 && mp_gru_width(16) == 16 && mp_gru_width(17) == 32 &&
                      mp_gru_width(128) == 128 && mp_gru_width(129) == -MP_ERR_ARG && mp_gru_width(0) == -MP_ERR_ARG &&
                      PK == ((size_t)6 * P * P + 4 * P) * 4 && mp_gru_pack_bytes(129) == 0;
  ++n_cases;
  n_fail += !answers;
  printf("%s mp_gru_ok / width / pack_bytes answers\n", answers ? "ok  " : "FAIL");

#define PACK(wc, wcb, wh, rs, cs, whb, bi, bib, bh, bhb, C_, pk, pkb) \
  mp_gru_pack_f32(wc, 3 * C, 1, wcb, wh, rs, cs, whb, bi, bib, bh, bhb, C_, pk, pkb, NULL)
  ACCEPT(PACK(DEVF, WB, DEVF, 1, C, WB, DEVF, BB, DEVF, BB, C, DEVF, PK));
  ACCEPT(PACK(DEVF, WB, DEVF, 3 * C, 1, WB, NULL, 0, NULL, 0, C, DEVF, PK));
  REJECT("wc is NULL", PACK(NULL, WB, DEVF, 1, C, WB, DEVF, BB, DEVF, BB, C, DEVF, PK));
  REJECT("wc holds", PACK(DEVF, WB - 4, DEVF, 1, C, WB, DEVF, BB, DEVF, BB, C, DEVF, PK));
  REJECT("wh is NULL", PACK(DEVF, WB, NULL, 1, C, WB, DEVF, BB, DEVF, BB, C, DEVF, PK));
  REJECT("strides of wh", PACK(DEVF, WB, DEVF, 0, C, WB, DEVF, BB, DEVF, BB, C, DEVF, PK));
  REJECT("wh holds", PACK(DEVF, WB, DEVF, 1, C, WB - 4, DEVF, BB, DEVF, BB, C, DEVF, PK));
  REJECT("b_ih holds", PACK(DEVF, WB, DEVF, 1, C, WB, DEVF, BB - 4, DEVF, BB, C, DEVF, PK));
  REJECT("b_hh holds", PACK(DEVF, WB, DEVF, 1, C, WB, DEVF, BB, DEVF, BB - 4, C, DEVF, PK));
  REJECT("pack is NULL", PACK(DEVF, WB, DEVF, 1, C, WB, DEVF, BB, DEVF, BB, C, NULL, PK));
  REJECT("pack holds", PACK(DEVF, WB, DEVF, 1, C, WB, DEVF, BB, DEVF, BB, C, DEVF, PK - 4));
  REJECT("C <= 128", PACK(DEVF, WB, DEVF, 1, C, WB, DEVF, BB, DEVF, BB, 129, DEVF, PK));
  REJECT("C = 0", PACK(DEVF, WB, DEVF, 1, C, WB, DEVF, BB, DEVF, BB, 0, DEVF, PK));

#define CELL(a, lda, ab, h, hb, N_, C_, pk, pkb, o, ob, g, ldg, gb) \
  mp_gru_cell_f32(a, lda, ab, h, P, hb, N_, C_, pk, pkb, o, P, ob, g, ldg, gb, NULL)
  ACCEPT(CELL(DEVF, P, ROWS, DEVF + 4, ROWS, N, C, DEVF, PK, DEVF + 8, ROWS, DEVF, 4 * P, G4));
  ACCEPT(CELL(DEVF, P, ROWS, DEVF + 4, ROWS, N, C, DEVF, PK, DEVF + 8, ROWS, NULL, 0, 0));
  REJECT("a is NULL", CELL(NULL, P, ROWS, DEVF + 4, ROWS, N, C, DEVF, PK, DEVF + 8, ROWS, NULL, 0, 0));
  REJECT("ld of a", CELL(DEVF, P - 4, ROWS, DEVF + 4, ROWS, N, C, DEVF, PK, DEVF + 8, ROWS, NULL, 0, 0));
  REJECT("multiple of 4", CELL(DEVF, P + 1, 2 * ROWS, DEVF + 4, ROWS, N, C, DEVF, PK, DEVF + 8, ROWS, NULL, 0, 0));
  REJECT("16-byte aligned", CELL(DEVF + 1, P, ROWS, DEVF + 4, ROWS, N, C, DEVF, PK, DEVF + 8, ROWS, NULL, 0, 0));
  REJECT("a holds", CELL(DEVF, P, ROWS - 4, DEVF + 4, ROWS, N, C, DEVF, PK, DEVF + 8, ROWS, NULL, 0, 0));
  REJECT("h holds", CELL(DEVF, P, ROWS, DEVF + 4, ROWS - 4, N, C, DEVF, PK, DEVF + 8, ROWS, NULL, 0, 0));
  REJECT("out holds", CELL(DEVF, P, ROWS, DEVF + 4, ROWS, N, C, DEVF, PK, DEVF + 8, ROWS - 4, NULL, 0, 0));
  REJECT("ld of gates", CELL(DEVF, P, ROWS, DEVF + 4, ROWS, N, C, DEVF, PK, DEVF + 8, ROWS, DEVF, 3 * P, G4));
  REJECT("gates holds", CELL(DEVF, P, ROWS, DEVF + 4, ROWS, N, C, DEVF, PK, DEVF + 8, ROWS, DEVF, 4 * P, G4 - 4));
  REJECT("pack holds", CELL(DEVF, P, ROWS, DEVF + 4, ROWS, N, C, DEVF, PK - 4, DEVF + 8, ROWS, NULL, 0, 0));
  REJECT("alias", CELL(DEVF, P, ROWS, DEVF + 4, ROWS, N, C, DEVF, PK, DEVF + 4, ROWS, NULL, 0, 0));
  REJECT("N = -1", CELL(DEVF, P, ROWS, DEVF + 4, ROWS, -1, C, DEVF, PK, DEVF + 8, ROWS, NULL, 0, 0));
  REJECT("C <= 128", CELL(DEVF, P, ROWS, DEVF + 4, ROWS, N, 129, DEVF, PK, DEVF + 8, ROWS, NULL, 0, 0));

#define BWD(dh, dhb, h, hb, g, gb, C_, q, ldq, qb, d, db) \
  mp_gru_cell_bwd_f32(dh, P, dhb, h, P, hb, g, 4 * P, gb, N, C_, q, ldq, qb, d, P, db, NULL)
  ACCEPT(BWD(DEVF, ROWS, DEVF, ROWS, DEVF, G4, C, DEVF, 4 * P, G4, DEVF, ROWS));
  REJECT("dh is NULL", BWD(NULL, ROWS, DEVF, ROWS, DEVF, G4, C, DEVF, 4 * P, G4, DEVF, ROWS));
  REJECT("dh holds", BWD(DEVF, ROWS - 4, DEVF, ROWS, DEVF, G4, C, DEVF, 4 * P, G4, DEVF, ROWS));
  REJECT("h holds", BWD(DEVF, ROWS, DEVF, ROWS - 4, DEVF, G4, C, DEVF, 4 * P, G4, DEVF, ROWS));
  REJECT("gates is NULL", BWD(DEVF, ROWS, DEVF, ROWS, NULL, G4, C, DEVF, 4 * P, G4, DEVF, ROWS));
  REJECT("gates holds", BWD(DEVF, ROWS, DEVF, ROWS, DEVF, G4 - 4, C, DEVF, 4 * P, G4, DEVF, ROWS));
  REJECT("ld of dG", BWD(DEVF, ROWS, DEVF, ROWS, DEVF, G4, C, DEVF, 3 * P, G4, DEVF, ROWS));
  REJECT("dG holds", BWD(DEVF, ROWS, DEVF, ROWS, DEVF, G4, C, DEVF, 4 * P, G4 - 4, DEVF, ROWS));
  REJECT("dh_dir holds", BWD(DEVF, ROWS, DEVF, ROWS, DEVF, G4, C, DEVF, 4 * P, G4, DEVF, ROWS - 4));
  REJECT("C <= 128", BWD(DEVF, ROWS, DEVF, ROWS, DEVF, G4, 129, DEVF, 4 * P, G4, DEVF, ROWS));

  printf("abi_reject_ggc: %d cases, %d failures\n", n_cases, n_fail);
  return n_fail ? 1 : 0;
}
