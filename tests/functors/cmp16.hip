// 16-byte rows (int64 a, int64 b): b descending, then a ascending.
// 128 bits of key: no 64-bit sort key expresses it.
__device__ int mr_compare(mrd::Bytes x, mrd::Bytes y) {
  const long long xa = x.as<long long>(0), xb = x.as<long long>(8);
  const long long ya = y.as<long long>(0), yb = y.as<long long>(8);
  if (xb != yb) return xb > yb ? -1 : 1;
  if (xa != ya) return xa < ya ? -1 : 1;
  return 0;
}
