/* The comparator form of the device sort functors through the MR_* C API:
 * MR_sort_keys_device with an mr_compare source over 16-byte keys, and
 * MR_sort_multivalues_device over 12-byte values of a KMV. The two sources are
 * read from the files named on the command line. Needs a GPU engine. Exits
 * non-zero on the first failed check. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cmapreduce.h"

static int fails = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      fails++;                                                      \
    }                                                               \
  } while (0)

static char *slurp(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  char *s = (char *)malloc((size_t)n + 1);
  if (fread(s, 1, (size_t)n, f) != (size_t)n) exit(2);
  s[n] = 0;
  fclose(f);
  return s;
}

enum { NKV = 5000, NMV = 6000, NKEY = 5 };

/* keys (int64 a, int64 b) with many ties, value = the row number */
static void gen16(int itask, void *kv, void *app) {
  for (int64_t i = 0; i < NKV; ++i) {
    int64_t k[2] = {i * 7 % 11 - 5, i * 13 % 7 - 3};
    MR_kv_add(kv, (char *)k, 16, (char *)&i, 8);
  }
  (void)itask; (void)app;
}

/* b descending, then a ascending */
static int cmp16(const int64_t *x, const int64_t *y) {
  if (x[1] != y[1]) return x[1] > y[1] ? -1 : 1;
  if (x[0] != y[0]) return x[0] < y[0] ? -1 : 1;
  return 0;
}

static int64_t seen, vsum, prev_key[2], prev_val;

static void scan16(char *key, int kb, char *val, int vb, void *app) {
  int64_t k[2], v;
  CHECK(kb == 16 && vb == 8);
  memcpy(k, key, 16);
  memcpy(&v, val, 8);
  if (seen) {
    const int c = cmp16(prev_key, k);
    if (!(c < 0 || (c == 0 && prev_val < v))) fails++;  /* sorted, ties in input order */
  }
  memcpy(prev_key, k, 16);
  prev_val = v;
  seen++;
  vsum += v;
  (void)app;
}

typedef struct { int a, b; unsigned tag; } Rec;

static void gen12(int itask, void *kv, void *app) {
  for (int i = 0; i < NMV; ++i) {
    int k = i % NKEY;
    Rec r = {i * 31 % 7 - 3, i * 17 % 9 - 4, (unsigned)i};
    MR_kv_add(kv, (char *)&k, 4, (char *)&r, 12);
  }
  (void)itask; (void)app;
}

/* a descending, then b ascending */
static int cmp12(const Rec *x, const Rec *y) {
  if (x->a != y->a) return x->a > y->a ? -1 : 1;
  if (x->b != y->b) return x->b < y->b ? -1 : 1;
  return 0;
}

static int pos_before[NMV]; /* tag -> place in its key's values before the sort */
static int key_order[2][NKEY], nkeys[2], nvals[2];

static void scan12(char *key, int kb, char *mv, int nv, int *vb, void *app) {
  const int after = *(int *)app;
  CHECK(kb == 4 && mv != NULL);
  if (!mv) return;
  if (nkeys[after] < NKEY) key_order[after][nkeys[after]] = *(int *)key;
  nkeys[after]++;
  nvals[after] += nv;
  Rec prev = {0, 0, 0};
  for (int j = 0; j < nv; ++j) {
    Rec r;
    CHECK(vb[j] == 12);
    memcpy(&r, mv + 12 * j, 12);
    CHECK(r.tag < NMV && (int)(r.tag % NKEY) == *(int *)key);
    if (r.tag >= NMV) return;
    if (!after) {
      pos_before[r.tag] = j;
    } else if (j) {
      const int c = cmp12(&prev, &r);
      if (!(c < 0 || (c == 0 && pos_before[prev.tag] < pos_before[r.tag]))) fails++;
    }
    prev = r;
  }
}

int main(int argc, char **argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s cmp16.hip cmp12.hip\n", argv[0]);
    return 2;
  }
  char *code16 = slurp(argv[1]), *code12 = slurp(argv[2]);
  MR_set_error_mode(1); /* failed calls return 0 and leave MR_last_error() */

  void *mr = MR_create(NULL);
  CHECK(MR_map(mr, 1, gen16, NULL) == NKV);
  CHECK(MR_sort_keys_device(mr, code16, 64) == NKV);
  MR_scan_kv(mr, scan16, NULL);
  CHECK(seen == NKV && vsum == (int64_t)NKV * (NKV - 1) / 2);
  /* a source with neither functor is an error that names both */
  CHECK(MR_sort_keys_device(mr, "__device__ int other(int x) { return x; }", 64) == 0);
  CHECK(strstr(MR_last_error(), "mr_sortkey") && strstr(MR_last_error(), "mr_compare"));
  MR_destroy(mr);

  void *mv = MR_create(NULL);
  int after = 0;
  CHECK(MR_map(mv, 1, gen12, NULL) == NMV);
  CHECK(MR_collate(mv, NULL) == NKEY);
  MR_scan_kmv(mv, scan12, &after);
  CHECK(MR_sort_multivalues_device(mv, code12, 64) == NKEY);
  after = 1;
  MR_scan_kmv(mv, scan12, &after);
  CHECK(nkeys[0] == NKEY && nkeys[1] == NKEY && nvals[0] == NMV && nvals[1] == NMV);
  CHECK(memcmp(key_order[0], key_order[1], sizeof(key_order[0])) == 0); /* the keys stay where they were */
  MR_destroy(mv);

  free(code16);
  free(code12);
  if (fails) {
    fprintf(stderr, "%d checks failed; last error: %s\n", fails, MR_last_error());
    return 1;
  }
  printf("ALL OK\n");
  return 0;
}
