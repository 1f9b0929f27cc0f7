// 12-byte rows {int a; int b; unsigned tag}: a descending, then b ascending, as a 64-bit key.
// The helper below is named mr_compare and orders the other way round: code
// that defines mr_sortkey takes the radix route and never calls it.
__device__ int mr_compare(mrd::Bytes x, mrd::Bytes y) {
  const int xa = x.as<int>(0), ya = y.as<int>(0);
  return xa < ya ? -1 : xa > ya ? 1 : 0;
}
__device__ unsigned long long mr_sortkey(mrd::Bytes r) {
  const unsigned int a = (unsigned int)r.as<int>(0) ^ 0x80000000u;  // signed -> unsigned order
  const unsigned int b = (unsigned int)r.as<int>(4) ^ 0x80000000u;
  return ((unsigned long long)(~a) << 32) | b;
}
