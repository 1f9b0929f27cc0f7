// 12-byte rows {int a; int b; unsigned tag}: a descending, then b ascending (tag not compared)
__device__ int mr_compare(mrd::Bytes x, mrd::Bytes y) {
  const int xa = x.as<int>(0), xb = x.as<int>(4), ya = y.as<int>(0), yb = y.as<int>(4);
  if (xa != ya) return xa > ya ? -1 : 1;
  if (xb != yb) return xb < yb ? -1 : 1;
  return 0;
}
