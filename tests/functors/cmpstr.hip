// byte strings of any length (0 included): longer first, then bytes ascending
__device__ int mr_compare(mrd::Bytes x, mrd::Bytes y) {
  if (x.n != y.n) return x.n > y.n ? -1 : 1;
  for (long long i = 0; i < x.n; ++i)
    if (x.p[i] != y.p[i]) return x.p[i] < y.p[i] ? -1 : 1;
  return 0;
}
