/* Device functor arguments through the MR_* C API: MR_set_device_args with raw
 * hipMalloc'd buffers the program keeps, a map functor that reads them
 * (MR_map_device_tasks) and MR_scan_device with a functor that writes to
 * them. The two sources are read from the files named on the command line
 * (the map and KV scan functors of tests/test_device_args.py). Needs a GPU
 * engine. Exits non-zero on the first failed check. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

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

enum { N = 1000, NTAB = 97 };

static int64_t tab[NTAB], mod, seen, hist_want[16];

/* the map functor: task t -> (tab[t % NTAB] % mod, t), in task order */
static void check_pair(char *key, int kb, char *val, int vb, void *app) {
  int64_t k, v;
  CHECK(kb == 8 && vb == 8);
  memcpy(&k, key, 8);
  memcpy(&v, val, 8);
  if (v != seen || k != tab[v % NTAB] % mod) fails++;
  hist_want[k % 16]++;
  seen++;
  (void)app;
}

int main(int argc, char **argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s map.hip scan.hip\n", argv[0]);
    return 2;
  }
  char *map_code = slurp(argv[1]), *scan_code = slurp(argv[2]);
  MR_set_error_mode(1); /* failed calls return 0 and leave MR_last_error() */

  void *mr = MR_create(NULL); /* first: the engine picks the device */
  void *dtab = NULL, *dmod = NULL, *dacc = NULL, *dhist = NULL;
  for (int i = 0; i < NTAB; ++i) tab[i] = (i * 31 + 7) % 1009;
  mod = 13;
  CHECK(hipMalloc(&dtab, sizeof(tab)) == hipSuccess && hipMalloc(&dmod, 8) == hipSuccess);
  CHECK(hipMalloc(&dacc, 24) == hipSuccess && hipMalloc(&dhist, 128) == hipSuccess);
  if (fails) return 1;
  CHECK(hipMemcpy(dtab, tab, sizeof(tab), hipMemcpyHostToDevice) == hipSuccess);
  CHECK(hipMemcpy(dmod, &mod, 8, hipMemcpyHostToDevice) == hipSuccess);
  CHECK(hipMemset(dacc, 0, 24) == hipSuccess && hipMemset(dhist, 0, 128) == hipSuccess);
  CHECK(hipDeviceSynchronize() == hipSuccess);

  void *margs[2] = {dtab, dmod};
  uint64_t mbytes[2] = {sizeof(tab), 8};
  MR_set_device_args(mr, 2, margs, mbytes);
  CHECK(MR_map_device_tasks(mr, N, map_code, 0) == N);
  CHECK(MR_scan_kv(mr, check_pair, NULL) == N);
  CHECK(seen == N);

  /* new contents in the same buffers: the next call sees them */
  for (int i = 0; i < NTAB; ++i) tab[i] = (i * 17 + 3) % 997;
  mod = 11;
  CHECK(hipMemcpy(dtab, tab, sizeof(tab), hipMemcpyHostToDevice) == hipSuccess);
  CHECK(hipMemcpy(dmod, &mod, 8, hipMemcpyHostToDevice) == hipSuccess);
  seen = 0;
  memset(hist_want, 0, sizeof(hist_want));
  CHECK(MR_map_device_tasks(mr, N, map_code, 0) == N);
  CHECK(MR_scan_kv(mr, check_pair, NULL) == N);
  CHECK(seen == N);

  /* the scan functor writes {count, sum of index, pairs with value == index} and a histogram of key % 16 */
  void *sargs[2] = {dacc, dhist};
  uint64_t sbytes[2] = {24, 128};
  MR_set_device_args(mr, 2, sargs, sbytes);
  CHECK(MR_scan_device(mr, scan_code) == N);
  CHECK(hipDeviceSynchronize() == hipSuccess);
  uint64_t acc[3] = {0, 0, 0}, hist[16];
  CHECK(hipMemcpy(acc, dacc, 24, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(hipMemcpy(hist, dhist, 128, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(acc[0] == N && acc[1] == (uint64_t)N * (N - 1) / 2 && acc[2] == N);
  for (int i = 0; i < 16; ++i) CHECK(hist[i] == (uint64_t)hist_want[i]);
  seen = 0;
  CHECK(MR_scan_kv(mr, check_pair, NULL) == N && seen == N); /* the pairs are still there, as they were */

  /* more than 8 buffers is an error that leaves the binding as it was */
  void *many[9];
  uint64_t manyb[9];
  for (int i = 0; i < 9; ++i) {
    many[i] = dmod;
    manyb[i] = 8;
  }
  MR_set_device_args(mr, 9, many, manyb);
  CHECK(strstr(MR_last_error(), "at most 8") != NULL);
  CHECK(MR_scan_device(mr, scan_code) == N);
  CHECK(hipDeviceSynchronize() == hipSuccess);
  CHECK(hipMemcpy(acc, dacc, 24, hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(acc[0] == 2 * N);
  MR_set_device_args(mr, 0, NULL, NULL); /* cleared before the buffers go */
  MR_destroy(mr);
  hipFree(dtab);
  hipFree(dmod);
  hipFree(dacc);
  hipFree(dhist);

  free(map_code);
  free(scan_code);
  if (fails) {
    fprintf(stderr, "%d checks failed; last error: %s\n", fails, MR_last_error());
    return 1;
  }
  printf("ALL OK\n");
  return 0;
}
