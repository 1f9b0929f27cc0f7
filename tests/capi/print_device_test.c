/* MR_print_device through the C API: N pairs from a map functor
 * (MR_map_device_tasks), formatted on the GPU by a print functor and written
 * to a file; the test that runs this program compares the file. The two
 * sources are read from the files named on the command line (GEN and KV_LINE
 * of tests/test_print_device.py). Needs a GPU engine. Exits non-zero on the
 * first failed check. */
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

static char *slurp(const char *path, long *len) {
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
  if (len) *len = n;
  return s;
}

enum { N = 1000 };

static int seen = 0;
static void count_pair(char *key, int kb, char *val, int vb, void *app) {
  (void)key;
  (void)val;
  (void)app;
  if (kb == 8 && vb == 8) seen++;
}

int main(int argc, char **argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s gen.hip print.hip out.txt\n", argv[0]);
    return 2;
  }
  char *gen = slurp(argv[1], NULL), *print = slurp(argv[2], NULL);
  MR_set_error_mode(1); /* failed calls return 0 and leave MR_last_error() */
  void *mr = MR_create(NULL);
  CHECK(MR_map_device_tasks(mr, N, gen, 0) == N);

  uint64_t bytes = MR_print_device(mr, argv[3], 0, -1, print);
  long len = 0;
  char *text = slurp(argv[3], &len);
  CHECK(bytes > 0 && bytes == (uint64_t)len);
  free(text);
  CHECK(MR_scan_kv(mr, count_pair, NULL) == N && seen == N); /* the pairs are still there */

  /* a source without mr_print: 0 and an error that names it */
  CHECK(MR_print_device(mr, argv[3], 1, -1, gen) == 0);
  CHECK(strstr(MR_last_error(), "mr_print") != NULL);
  /* another rank's turn: nothing written */
  CHECK(MR_print_device(mr, argv[3], 1, 1, print) == 0);

  MR_destroy(mr);
  free(gen);
  free(print);
  if (fails) {
    fprintf(stderr, "%d checks failed; last error: %s\n", fails, MR_last_error());
    return 1;
  }
  printf("ALL OK\n");
  return 0;
}
