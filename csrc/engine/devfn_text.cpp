// The device text of the device functors (devfn_text.h): the prelude every
// functor source starts with and the kernels that follow the user's code, as
// raw strings. The host side (kind table, compile, launches) is devfn.cpp.
#include "devfn_text.h"

namespace mrh {
namespace devfn {
namespace text {

const char kPrelude[] = R"MRD(
// ---- mrd: the engine's device-functor prelude (csrc/engine/devfn_text.cpp) ----
namespace mrd {
typedef unsigned char u8;
typedef long long i64;
typedef unsigned long long u64;
// a key or value: p[0 .. n)
struct Bytes {
  const u8* p;
  i64 n;
  template <class T>
  __device__ T as(i64 off = 0) const {
    T v;
    __builtin_memcpy(&v, p + off, sizeof(T));
    return v;
  }
};
// row i of a column: fixed width w (off null) or offsets off[rows + 1]. The
// index keeps the caller's type: with the comparator sort's u32 row numbers
// off[i] and off[i + 1] stay two 8-byte loads, which sort var-width rows
// faster than the one 16-byte load a 64-bit index is compiled to
template <class I>
__device__ inline Bytes row(const u8* d, const i64* off, i64 w, I i) {
  return off ? Bytes{d + off[i], off[i + 1] - off[i]} : Bytes{d + i * w, w};
}
// the same where the column may not be there (d null: the pairs of a task map): empty rows
__device__ inline Bytes row_or_empty(const u8* d, const i64* off, i64 w, i64 i) {
  return d ? row(d, off, w, i) : Bytes{nullptr, 0};
}
// the values of one key (reduce): n values, fixed width w or offsets off[n+1]
struct Values {
  const u8* d;
  const i64* off;
  i64 w;
  i64 n;
  __device__ Bytes operator[](i64 i) const { return row(d, off, w, i); }
  template <class T>
  __device__ T get(i64 i, i64 byte = 0) const { return (*this)[i].template as<T>(byte); }
};
// n bytes to dst: the common widths as single wide copies
__device__ inline void put(u8* dst, const u8* src, i64 n) {
  switch (n) {
    case 0: return;
    case 4: __builtin_memcpy(dst, src, 4); return;
    case 8: __builtin_memcpy(dst, src, 8); return;
    case 12: __builtin_memcpy(dst, src, 12); return;
    case 16: __builtin_memcpy(dst, src, 16); return;
    case 24: __builtin_memcpy(dst, src, 24); return;
    default: for (i64 i = 0; i < n; ++i) dst[i] = src[i];
  }
}
// the emitter: counts in the first pass, writes in the second
struct Emit {
  bool write;
  i64 nrec, kb, vb;
  u64 kmin, kmax, vmin, vmax;
  u8* okd;
  i64* okoff;
  u8* ovd;
  i64* ovoff;
  i64 rlim, klim, vlim;  // write pass: the room the count pass measured (an impure functor cannot overrun it)
  __device__ void emit(const void* k, i64 kn, const void* v, i64 vn) {
    if (write && (nrec >= rlim || kb + kn > klim || vb + vn > vlim)) return;
    if (write) {
      if (okoff) okoff[nrec] = kb;
      if (ovoff) ovoff[nrec] = vb;
      put(okd + kb, (const u8*)k, kn);
      put(ovd + vb, (const u8*)v, vn);
    } else {
      kmin = (u64)kn < kmin ? (u64)kn : kmin;
      kmax = (u64)kn > kmax ? (u64)kn : kmax;
      vmin = (u64)vn < vmin ? (u64)vn : vmin;
      vmax = (u64)vn > vmax ? (u64)vn : vmax;
    }
    ++nrec;
    kb += kn;
    vb += vn;
  }
  template <class K, class V>
  __device__ void emit(const K& k, const V& v) { emit(&k, sizeof(K), &v, sizeof(V)); }
  template <class K>
  __device__ void emit_key(const K& k) { emit(&k, sizeof(K), nullptr, 0); }
};
// the text sink of mr_print: counts in the first pass, writes in the second.
// p is the item's first byte (in HBM, or in the workgroup's LDS stage: a flat
// pointer either way), room what the count pass measured for the item: a
// write pass never stores at or past p + room (an impure functor cannot overrun it)
struct Text {
  bool write;
  u8* p;
  i64 n;     // bytes so far
  i64 room;  // write pass only
  __device__ void put(const void* s, i64 m) {
    if (m <= 0) return;
    if (write) {
      const i64 left = room - n, c = m < left ? m : left;
      for (i64 i = 0; i < c; ++i) p[n + i] = ((const u8*)s)[i];
    }
    n += m;
  }
  __device__ void put(Bytes b) { put(b.p, b.n); }
  __device__ void chr(char c) {
    if (write && n < room) p[n] = (u8)c;
    ++n;
  }
  // a NUL-terminated string (a literal); the NUL is not written
  __device__ void str(const char* s) {
    for (; *s; ++s) chr(*s);
  }
  __device__ void udec(u64 v) {
    char b[20];
    int k = 20;
    do {
      b[--k] = (char)('0' + (int)(v % 10));
      v /= 10;
    } while (v);
    put(b + k, 20 - k);
  }
  // a minus sign, no plus sign; LLONG_MIN through its unsigned magnitude
  __device__ void dec(long long v) {
    if (v < 0) chr('-');
    udec(v < 0 ? 0ull - (u64)v : (u64)v);
  }
  // lower case, no prefix, no leading zeros
  __device__ void hex(u64 v) {
    char b[16];
    int k = 16;
    do {
      b[--k] = "0123456789abcdef"[v & 15];
      v >>= 4;
    } while (v);
    put(b + k, 16 - k);
  }
  // x with d decimals (d clamped into 0 .. 9): n = |x| * 10^d (one IEEE
  // multiply by an exact power) rounded half-even to an integer, "-" iff
  // x < 0 and n != 0, then n / 10^d and, for d > 0, "." and n % 10^d padded
  // to d digits. nan; inf / -inf; ovf / -ovf when |x| * 10^d >= 2^63.
  __device__ void fixed(double x, int d) {
    const double pd[10] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9};
    const u64 pi[10] = {1ull,      10ull,      100ull,      1000ull,      10000ull,
                        100000ull, 1000000ull, 10000000ull, 100000000ull, 1000000000ull};
    d = d < 0 ? 0 : d > 9 ? 9 : d;
    if (x != x) return str("nan");
    const bool neg = x < 0;
    const double a = __builtin_fabs(x);
    if (a == __builtin_inf()) return str(neg ? "-inf" : "inf");
    const double m = a * pd[d];
    if (m >= 9223372036854775808.0) return str(neg ? "-ovf" : "ovf");
    const u64 r = (u64)__builtin_rint(m);  // round to nearest, ties to even
    if (neg && r) chr('-');
    udec(r / pi[d]);
    if (d) {
      chr('.');
      char b[9];
      u64 f = r % pi[d];
      for (int k = d - 1; k >= 0; --k) {
        b[k] = (char)('0' + (int)(f % 10));
        f /= 10;
      }
      put(b, d);
    }
  }
};
// a device buffer bound to the MapReduce object (set_device_args): p[0 .. n)
// bytes, read-only to every functor but mr_scan
struct Arg {
  const u8* p;
  i64 n;
  template <class T>
  __device__ const T* as() const { return reinterpret_cast<const T*>(p); }
  template <class T>
  __device__ i64 count() const { return n / (i64)sizeof(T); }
};
// the bound buffers, one by-value kernel argument; args[i] past n is {nullptr, 0}
struct Args {
  Arg a[8];
  int n;
  __device__ Arg operator[](int i) const { return i >= 0 && i < n ? a[i] : Arg{nullptr, 0}; }
};
// the same for mr_scan, the one functor that runs once per item and may write
struct MutArg {
  u8* p;
  i64 n;
  template <class T>
  __device__ T* as() const { return reinterpret_cast<T*>(p); }
  template <class T>
  __device__ i64 count() const { return n / (i64)sizeof(T); }
};
struct MutArgs {
  MutArg a[8];
  int n;
  __device__ MutArg operator[](int i) const { return i >= 0 && i < n ? a[i] : MutArg{nullptr, 0}; }
};
// the by-value kernel argument the host fills is its devfn::Args (devfn.h)
static_assert(sizeof(Args) == MRD_ARGS_BYTES && sizeof(MutArgs) == MRD_ARGS_BYTES && sizeof(Arg) == 16 &&
                  sizeof(MutArg) == 16 && __builtin_offsetof(Args, n) == MRD_ARGS_BYTES - 8 &&
                  __builtin_offsetof(MutArgs, n) == MRD_ARGS_BYTES - 8,
              "mrd::Args / mrd::MutArgs do not match the host's devfn::Args");
}  // namespace mrd
// Every entry point may take a trailing `const mrd::Args&`, each on its own.
// MRD_SHIM(f, (template parameters), (parameters), (arguments)) makes the pair
// of call shims mrd::call_f for the user's mr_f: the first (tag int, preferred
// for the literal 0) is viable when mr_f takes the bound buffers, the second
// (tag long) when it does not. Both are templates whose call is dependent, so
// the form the user did not write is a substitution failure, not an error.
#define MRD_LIST(...) __VA_ARGS__
#define MRD_SHIM(f, tparams, params, args)                                                             \
  template <MRD_LIST tparams>                                                                          \
  __device__ auto call_##f(MRD_LIST params, const Args& g, int) -> decltype(mr_##f(MRD_LIST args, g)) { \
    return mr_##f(MRD_LIST args, g);                                                                   \
  }                                                                                                    \
  template <MRD_LIST tparams>                                                                          \
  __device__ auto call_##f(MRD_LIST params, const Args&, long) -> decltype(mr_##f(MRD_LIST args)) {    \
    return mr_##f(MRD_LIST args);                                                                      \
  }
// ---- user code ----
)MRD";

// kernels: MRD_REDUCE selects the item kind; seg null = pairs, kd null = tasks
const char kEmitKernels[] = R"MRD(
// ---- mrd kernels ----
namespace mrd {
__device__ inline i64 seg_of(const i64* seg, i64 nseg, i64 j) {
  i64 lo = 0, hi = nseg;
  while (hi - lo > 1) {
    const i64 mid = (lo + hi) >> 1;
    if (seg[mid] <= j) lo = mid;
    else hi = mid;
  }
  return lo;
}
#if MRD_REDUCE == 2
MRD_SHIM(init, (class A), (Bytes k, A& a), (k, a))
MRD_SHIM(add, (class A), (A& a, Bytes v), (a, v))
MRD_SHIM(merge, (class A), (A& a, const A& b), (a, b))
MRD_SHIM(finish, (class A, class E), (Bytes k, const A& a, E& e), (k, a, e))
#elif MRD_REDUCE
MRD_SHIM(reduce, (class E), (Bytes k, Values v, E& e), (k, v, e))
#else
MRD_SHIM(map, (class E), (Bytes k, Bytes v, i64 t, E& e), (k, v, t, e))
#endif
__device__ inline void run_item(const u8* kd, const i64* koff, i64 kw, const u8* vd, const i64* voff, i64 vw,
                                const i64* seg, i64 first, i64 i, Emit& e, const Args& g) {
#if MRD_REDUCE == 2
  // fold: vd = the merged accumulators, voff = each key's first chunk, vw = sizeof(mr_acc)
  mr_acc a;
  __builtin_memcpy(&a, vd + voff[i] * vw, sizeof(mr_acc));
  call_finish(row_or_empty(kd, koff, kw, i), a, e, g, 0);
#elif MRD_REDUCE
  Values vals{vd + 0, voff, vw, seg[i + 1] - seg[i]};
  if (voff) vals.off = voff + seg[i];
  else vals.d = vd + seg[i] * vw;
  call_reduce(row_or_empty(kd, koff, kw, i), vals, e, g, 0);
#else
  call_map(row_or_empty(kd, koff, kw, first + i), row_or_empty(vd, voff, vw, first + i), first + i, e, g, 0);
#endif
}
}  // namespace mrd
extern "C" __global__ __launch_bounds__(256) void
mrd_count(const mrd::u8* kd, const mrd::i64* koff, mrd::i64 kw, const mrd::u8* vd, const mrd::i64* voff,
          mrd::i64 vw, const mrd::i64* seg, mrd::i64 first, mrd::i64 n, mrd::i64* cnt, mrd::u64* wid, int bytes,
          mrd::Args args) {
  mrd::u64 kmin = ~0ull, kmax = 0, vmin = ~0ull, vmax = 0;
  for (mrd::i64 i = (mrd::i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (mrd::i64)gridDim.x * 256) {
    mrd::Emit e{false, 0, 0, 0, ~0ull, 0, ~0ull, 0, nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
    mrd::run_item(kd, koff, kw, vd, voff, vw, seg, first, i, e, args);
    cnt[i] = e.nrec;
    if (bytes) {  // the byte columns only when the widths turned out not uniform (a second count pass)
      cnt[n + i] = e.kb;
      cnt[2 * n + i] = e.vb;
    }
    kmin = e.kmin < kmin ? e.kmin : kmin;
    kmax = e.kmax > kmax ? e.kmax : kmax;
    vmin = e.vmin < vmin ? e.vmin : vmin;
    vmax = e.vmax > vmax ? e.vmax : vmax;
  }
  // the record widths: wave, then block min / max, one set of atomics per block
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const mrd::u64 a = __shfl_xor(kmin, d, 64), b = __shfl_xor(kmax, d, 64);
    const mrd::u64 c = __shfl_xor(vmin, d, 64), e = __shfl_xor(vmax, d, 64);
    kmin = a < kmin ? a : kmin;
    kmax = b > kmax ? b : kmax;
    vmin = c < vmin ? c : vmin;
    vmax = e > vmax ? e : vmax;
  }
  __shared__ mrd::u64 red[4][4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[w][0] = kmin;
    red[w][1] = kmax;
    red[w][2] = vmin;
    red[w][3] = vmax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i) {
      kmin = red[i][0] < kmin ? red[i][0] : kmin;
      kmax = red[i][1] > kmax ? red[i][1] : kmax;
      vmin = red[i][2] < vmin ? red[i][2] : vmin;
      vmax = red[i][3] > vmax ? red[i][3] : vmax;
    }
    if (kmax || kmin != ~0ull) {
      atomicMin(wid + 0, kmin);
      atomicMax(wid + 1, kmax);
      atomicMin(wid + 2, vmin);
      atomicMax(wid + 3, vmax);
    }
  }
}
#if MRD_REDUCE == 2
// fold tier: a key's values in chunks of C, one thread per chunk (so a key
// with millions of values spreads over the whole GPU), then one thread per
// key merges its chunks' accumulators into the first
extern "C" __global__ void mrd_acc_size(mrd::i64* out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = sizeof(mr_acc);
}
extern "C" __global__ __launch_bounds__(256) void
mrd_fold_nchunks(const mrd::i64* seg, mrd::i64 nkey, mrd::i64 C, mrd::i64* cnt, mrd::u64* maxc) {
  mrd::u64 m = 0;
  for (mrd::i64 s = (mrd::i64)blockIdx.x * 256 + threadIdx.x; s < nkey; s += (mrd::i64)gridDim.x * 256) {
    cnt[s] = (seg[s + 1] - seg[s] + C - 1) / C;
    m = (mrd::u64)cnt[s] > m ? (mrd::u64)cnt[s] : m;
  }
  if (m) atomicMax(maxc, m);
}
extern "C" __global__ __launch_bounds__(256) void
mrd_fold_chunks(const mrd::u8* kd, const mrd::i64* koff, mrd::i64 kw, const mrd::u8* vd, const mrd::i64* voff,
                mrd::i64 vw, const mrd::i64* seg, mrd::i64 nkey, const mrd::i64* cstart, mrd::i64 nchunk,
                mrd::i64 C, mrd::u8* accs, mrd::Args args) {
  for (mrd::i64 c = (mrd::i64)blockIdx.x * 256 + threadIdx.x; c < nchunk; c += (mrd::i64)gridDim.x * 256) {
    const mrd::i64 s = mrd::seg_of(cstart, nkey, c);
    const mrd::i64 a0 = seg[s] + (c - cstart[s]) * C;
    const mrd::i64 a1 = a0 + C < seg[s + 1] ? a0 + C : seg[s + 1];
    mr_acc a;
    mrd::call_init(mrd::row_or_empty(kd, koff, kw, s), a, args, 0);
    for (mrd::i64 v = a0; v < a1; ++v) mrd::call_add(a, mrd::row_or_empty(vd, voff, vw, v), args, 0);
    __builtin_memcpy(accs + c * sizeof(mr_acc), &a, sizeof(mr_acc));
  }
}
// one level of a fixed pairwise tree: chunk j of a key (j % 2*stride == 0)
// takes in chunk j + stride; log2(most chunks of a key) levels leave each
// key's total in its first chunk, in the same order on every run
extern "C" __global__ __launch_bounds__(256) void
mrd_fold_merge(const mrd::i64* cstart, mrd::i64 nkey, mrd::i64 nchunk, mrd::i64 stride, mrd::u8* accs,
               mrd::Args args) {
  for (mrd::i64 c = (mrd::i64)blockIdx.x * 256 + threadIdx.x; c < nchunk; c += (mrd::i64)gridDim.x * 256) {
    const mrd::i64 s = mrd::seg_of(cstart, nkey, c);
    const mrd::i64 j = c - cstart[s];
    if (j % (2 * stride) != 0 || c + stride >= cstart[s + 1]) continue;
    mr_acc a, b;
    __builtin_memcpy(&a, accs + c * sizeof(mr_acc), sizeof(mr_acc));
    __builtin_memcpy(&b, accs + (c + stride) * sizeof(mr_acc), sizeof(mr_acc));
    mrd::call_merge(a, b, args, 0);
    __builtin_memcpy(accs + c * sizeof(mr_acc), &a, sizeof(mr_acc));
  }
}
#endif
// okw / ovw >= 0: every record's key / value has that width (the count pass
// said so): byte positions follow from the record position, no offsets
extern "C" __global__ __launch_bounds__(256) void
mrd_write(const mrd::u8* kd, const mrd::i64* koff, mrd::i64 kw, const mrd::u8* vd, const mrd::i64* voff,
          mrd::i64 vw, const mrd::i64* seg, mrd::i64 first, mrd::i64 n, const mrd::i64* pr, const mrd::i64* pk,
          const mrd::i64* pv, mrd::i64 okw, mrd::i64 ovw, mrd::u8* okd, mrd::i64* okoff, mrd::u8* ovd,
          mrd::i64* ovoff, mrd::Args args) {
  // pr / pk / pv: exclusive scans (n + 1) of records, key bytes, value bytes
  // (pk / pv unused when that width is uniform: okw / ovw >= 0)
  for (mrd::i64 i = (mrd::i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (mrd::i64)gridDim.x * 256) {
    const mrd::i64 r = pr[i];
    if (pr[i + 1] == r) continue;
    const mrd::i64 r1 = pr[i + 1];
    const mrd::i64 k0 = okw >= 0 ? r * okw : pk[i], v0 = ovw >= 0 ? r * ovw : pv[i];
    const mrd::i64 k1 = okw >= 0 ? r1 * okw : pk[i + 1], v1 = ovw >= 0 ? r1 * ovw : pv[i + 1];
    mrd::Emit e{true, 0, 0, 0, 0, 0, 0, 0, okd + k0, okw >= 0 ? nullptr : okoff + r, ovd + v0,
                ovw >= 0 ? nullptr : ovoff + r, r1 - r, k1 - k0, v1 - v0};
    mrd::run_item(kd, koff, kw, vd, voff, vw, seg, first, i, e, args);
    const mrd::i64 nw = e.nrec < r1 - r ? e.nrec : r1 - r;
    for (mrd::i64 j = 0; j < nw; ++j) {  // offsets relative to the item -> absolute
      if (okw < 0) okoff[r + j] += k0;
      if (ovw < 0) ovoff[r + j] += v0;
    }
  }
}
)MRD";

// a sort-key functor, __device__ unsigned long long mr_sortkey(mrd::Bytes)
const char kSortKeyKernel[] = R"MRD(
// ---- mrd sort-key kernel ----
namespace mrd {
MRD_SHIM(sortkey, (class B), (B b), (b))
}  // namespace mrd
extern "C" __global__ __launch_bounds__(256) void
mrd_sortkey(const mrd::u8* d, const mrd::i64* off, mrd::i64 w, mrd::i64 n, mrd::u64* key, unsigned int* idx,
            mrd::Args args) {
  for (mrd::i64 i = (mrd::i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (mrd::i64)gridDim.x * 256) {
    key[i] = mrd::call_sortkey(mrd::row(d, off, w, i), args, 0);
    idx[i] = (unsigned int)i;
  }
}
)MRD";

// a comparator functor, __device__ int mr_compare(mrd::Bytes a, mrd::Bytes b)
// (MR-MPI's contract: < 0 a first, 0 equal, > 0 b first). A stable merge sort
// over a u32 row-index permutation; the payload moves once afterwards (gather).
//
//   mrd_cmp_blocksort  one workgroup per tile of MRD_CMP_T rows: every thread
//                      sorts its own rows in registers, then merge-path merges
//                      in LDS double the run width until the tile is one run
//   mrd_cmp_merge      one launch per pass, runs of W -> runs of 2W between two
//                      index buffers; one workgroup per output tile: its split
//                      on the merge-path diagonal (binary search on global
//                      rows), the two sub-ranges into LDS, then the tile step
//
// Rows are ordered by less(i, j) = c < 0 || (c == 0 && i < j), c = mr_compare
// (row i, row j), after the optional segment ids: a total order, so stability
// and the merge-path splits need no special cases. The pass count depends on
// n alone (no host read between passes) and no workgroup waits for another.
//
// Memory safety does not depend on what mr_compare returns: every binary
// search runs a bounded number of steps inside [max(0, d - lb), min(d, la)],
// an end split is clamped to what its start split leaves reachable, and every
// merge consumes exactly the counts its two splits give it. So the index
// buffers only ever hold row numbers that were put in, and a comparator that
// is not a strict weak order gives an unspecified order (possibly with
// repeated rows), never an access outside the columns.
const char kCompareKernels[] = R"MRD(
// ---- mrd comparator merge sort ----
namespace mrd {
typedef unsigned int u32;
enum { CMP_T = MRD_CMP_T, CMP_PER = MRD_CMP_T / 256 };
MRD_SHIM(compare, (class B), (B a, B b), (a, b))
struct Cmp {
  const u8* d;
  const i64* off;
  i64 w;
  const i64* sid;  // segment id of every row, compared first (null: no segments)
  const Args& g;   // the bound buffers (the kernel's own argument)
  __device__ bool less(u32 i, u32 j) const {
    if (sid) {
      const i64 a = sid[i], b = sid[j];
      if (a != b) return a < b;
    }
    const int c = call_compare(row(d, off, w, i), row(d, off, w, j), g, 0);
    return c < 0 || (c == 0 && i < j);
  }
};
// merge path: how many of the first d rows of merge(A[0, la), B[0, lb)) come
// from A. At most 64 steps, every index inside its run whatever less() says.
template <class I>
__device__ inline I cmp_split(const Cmp& c, const u32* A, I la, const u32* B, I lb, I d) {
  I lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
  while (lo < hi) {
    const I mid = (lo + hi) >> 1;
    if (c.less(B[d - 1 - mid], A[mid])) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}
// an end split as the start split a on diagonal d allows it: a <= a1 <= la,
// and the B side likewise (a no-op for a strict weak order)
template <class I>
__device__ inline I cmp_clamp(I a1, I a, I d, I d1, I la, I lb) {
  const I lo = a > d1 - lb ? a : d1 - lb, hi = a + (d1 - d) < la ? a + (d1 - d) : la;
  return a1 < lo ? lo : a1 > hi ? hi : a1;
}
// one merge step of a tile in LDS: the runs A = src[s, s + la) and
// B = src[s + la, s + la + lb) into dst[s, ..); thread t writes the tile's
// rows [CMP_PER * t, CMP_PER * (t + 1)). All 256 threads call it.
__device__ inline void cmp_merge_tile(const Cmp& c, const u32* src, u32* dst, int* split, int s, int la, int lb) {
  const int t = threadIdx.x, tot = la + lb;
  int d = CMP_PER * t - s;
  d = d < tot ? d : tot;
  const int d1 = d + CMP_PER < tot ? d + CMP_PER : tot;
  const u32* A = src + s;
  const u32* B = A + la;
  int a = cmp_split<int>(c, A, la, B, lb, d);
  split[t] = a;
  __syncthreads();
  // the end split is the next thread's start (same pair of runs), or the pair's end
  const int a1 = cmp_clamp<int>(d1 < tot ? split[t + 1] : la, a, d, d1, la, lb);
  int b = d - a;
  const int b1 = d1 - a1;
  for (int k = d; k < d1; ++k) {  // (a1 - a) + (b1 - b) == d1 - k throughout
    if (a < a1 && (b >= b1 || !c.less(B[b], A[a]))) dst[s + k] = A[a++];
    else dst[s + k] = B[b++];
  }
}
}  // namespace mrd
extern "C" __global__ __launch_bounds__(256) void
mrd_cmp_blocksort(const mrd::u8* d, const mrd::i64* off, mrd::i64 w, const mrd::i64* sid, mrd::i64 n, mrd::u32* out,
                  mrd::Args args) {
  using namespace mrd;
  __shared__ u32 buf[2][CMP_T];
  __shared__ int split[257];
  const Cmp c{d, off, w, sid, args};
  const i64 base = (i64)blockIdx.x * CMP_T;
  const int cnt = n - base < CMP_T ? (int)(n - base) : CMP_T;
  const int t = threadIdx.x;
  // the thread's own rows: odd-even transposition in registers
  const int m = cnt - CMP_PER * t < 0 ? 0 : cnt - CMP_PER * t < CMP_PER ? cnt - CMP_PER * t : CMP_PER;
  u32 v[CMP_PER];
#pragma unroll
  for (int k = 0; k < CMP_PER; ++k) v[k] = (u32)(base + CMP_PER * t + k);
#pragma unroll 1
  for (int r = 0; r < (CMP_PER + 1) / 2; ++r) {
#pragma unroll
    for (int k = 0; k + 1 < CMP_PER; k += 2)
      if (k + 1 < m && c.less(v[k + 1], v[k])) {
        const u32 x = v[k];
        v[k] = v[k + 1];
        v[k + 1] = x;
      }
#pragma unroll
    for (int k = 1; k + 1 < CMP_PER; k += 2)
      if (k + 1 < m && c.less(v[k + 1], v[k])) {
        const u32 x = v[k];
        v[k] = v[k + 1];
        v[k + 1] = x;
      }
  }
#pragma unroll
  for (int k = 0; k < CMP_PER; ++k)
    if (k < m) buf[0][CMP_PER * t + k] = v[k];
  int cur = 0;
  for (int W = CMP_PER; W < CMP_T && W < cnt; W <<= 1) {  // cnt is the workgroup's: a uniform trip count
    __syncthreads();
    const int s = CMP_PER * t / (2 * W) * (2 * W);
    const int la = cnt - s < 0 ? 0 : cnt - s < W ? cnt - s : W;
    const int lb = cnt - s - W < 0 ? 0 : cnt - s - W < W ? cnt - s - W : W;
    cmp_merge_tile(c, buf[cur], buf[cur ^ 1], split, s, la, lb);
    cur ^= 1;
  }
  __syncthreads();
  for (int i = t; i < cnt; i += 256) out[base + i] = buf[cur][i];
}
extern "C" __global__ __launch_bounds__(256) void
mrd_cmp_merge(const mrd::u8* d, const mrd::i64* off, mrd::i64 w, const mrd::i64* sid, mrd::i64 n,
              const mrd::u32* src, mrd::u32* dst, mrd::i64 W, mrd::Args args) {
  using namespace mrd;
  __shared__ u32 buf[2][CMP_T];
  __shared__ int split[257];
  __shared__ i64 ends[2];
  const Cmp c{d, off, w, sid, args};
  const int t = threadIdx.x;
  const i64 g0 = (i64)blockIdx.x * CMP_T;  // this workgroup's output tile: dst[g0, g0 + cnt)
  const int cnt = n - g0 < CMP_T ? (int)(n - g0) : CMP_T;
  const i64 s = g0 / (2 * W) * (2 * W);    // its pair of runs: src[s, s + la) and src[s + la, s + la + lb)
  const i64 la = n - s < W ? n - s : W;
  const i64 lb = n - s - W < 0 ? 0 : n - s - W < W ? n - s - W : W;
  if (lb == 0) {  // a last run without a partner: copied through
    for (int i = t; i < cnt; i += 256) dst[g0 + i] = src[g0 + i];
    return;
  }
  const u32* A = src + s;
  const u32* B = A + la;
  const i64 d0 = g0 - s, d1 = d0 + cnt;  // d1 <= la + lb: the tile lies inside the pair
  if (t == 0) ends[0] = cmp_split<i64>(c, A, la, B, lb, d0);
  if (t == 64) ends[1] = cmp_split<i64>(c, A, la, B, lb, d1);
  __syncthreads();
  const i64 a0 = ends[0], a1 = cmp_clamp<i64>(ends[1], a0, d0, d1, la, lb);
  const i64 b0 = d0 - a0;
  const int na = (int)(a1 - a0), nb = cnt - na;  // b0 + nb == d1 - a1 <= lb
  for (int i = t; i < cnt; i += 256) buf[0][i] = i < na ? A[a0 + i] : B[b0 + (i - na)];
  __syncthreads();
  cmp_merge_tile(c, buf[0], buf[1], split, 0, na, nb);
  __syncthreads();
  for (int i = t; i < cnt; i += 256) dst[g0 + i] = buf[1][i];
}
)MRD";

// a scan functor, mr_scan in its KV (MRD_SCAN_KMV 0) or KMV (1) shape.
// One thread per item, every item exactly once; nothing is emitted, the
// functor writes to the bound buffers (mrd::MutArgs).
const char kScanKernel[] = R"MRD(
// ---- mrd scan kernel ----
extern "C" __global__ __launch_bounds__(256) void
mrd_scan(const mrd::u8* kd, const mrd::i64* koff, mrd::i64 kw, const mrd::u8* vd, const mrd::i64* voff, mrd::i64 vw,
         const mrd::i64* seg, mrd::i64 base, mrd::i64 n, mrd::MutArgs args) {
  for (mrd::i64 i = (mrd::i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (mrd::i64)gridDim.x * 256) {
    const mrd::Bytes key = mrd::row(kd, koff, kw, i);
#if MRD_SCAN_KMV
    mrd::Values vals{vd, voff, vw, seg[i + 1] - seg[i]};
    if (voff) vals.off = voff + seg[i];
    else vals.d = vd + seg[i] * vw;
    mr_scan(key, vals, args);
#else
    mr_scan(key, mrd::row(vd, voff, vw, i), base + i, args);
#endif
  }
}
)MRD";

// a partitioner functor, __device__ int mr_hash(mrd::Bytes key) (MR-MPI's
// hash callback): the owner of pair i is its return value reduced into
// [0, P) the way the host route does it, negative returns included
const char kHashKernel[] = R"MRD(
// ---- mrd partitioner kernel ----
namespace mrd {
MRD_SHIM(hash, (class B), (B b), (b))
}  // namespace mrd
extern "C" __global__ __launch_bounds__(256) void
mrd_hash(const mrd::u8* d, const mrd::i64* off, mrd::i64 w, mrd::i64 n, int P, int* dest, mrd::Args args) {
  for (mrd::i64 i = (mrd::i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (mrd::i64)gridDim.x * 256) {
    const int h = mrd::call_hash(mrd::row(d, off, w, i), args, 0);
    dest[i] = (int)(((mrd::i64)h % P + P) % P);
  }
}
)MRD";

// a print functor, mr_print in its KV (MRD_PRINT_KMV 0) or KMV (1) shape: the
// text of every item, in item order, as one contiguous byte range.
//
//   mrd_text_count  one thread per item (grid-stride): the functor with a
//                   counting Text, the item's bytes into cnt
//   mrd_text_write  after the exclusive scan `pre` of cnt: one workgroup per
//                   tile of TEXT_TILE consecutive items (grid-stride over the
//                   tiles), one thread per item. The tile owns out[pre[t0],
//                   pre[t1]). Staged route (the range is at most TEXT_STAGE
//                   bytes): every thread formats into the LDS stage, then the
//                   workgroup copies the range out in the output's 16-byte
//                   lines, whole lines as one 16-byte store each, the partial
//                   first and last line by bytes. Direct route (a longer
//                   range): every thread formats straight into HBM.
//
// The route follows from pre[t0] and pre[t1] alone: uniform over the workgroup
// (so are the barriers) and known without a host read. The stage image starts
// at the 16-byte line of the tile's first output byte: stage[j] is the byte
// for address line0 + j, the stage is TEXT_STAGE + 16 bytes, and a Text gets
// {stage + head + (pre[i] - pre[t0]), pre[i + 1] - pre[i]} exactly as it gets
// {out + pre[i], pre[i + 1] - pre[i]} on the direct route. tiles[0] / tiles[1]
// count the staged / direct tiles (one atomic per tile).
const char kPrintKernels[] = R"MRD(
// ---- mrd print kernels ----
namespace mrd {
enum { TEXT_TILE = 256, TEXT_STAGE = MRD_TEXT_STAGE };
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
#if MRD_PRINT_KMV
MRD_SHIM(print, (class T), (Bytes k, Values v, T& t), (k, v, t))
#else
MRD_SHIM(print, (class T), (Bytes k, Bytes v, i64 x, T& t), (k, v, x, t))
#endif
__device__ inline void print_item(const u8* kd, const i64* koff, i64 kw, const u8* vd, const i64* voff, i64 vw,
                                  const i64* seg, i64 base, i64 i, Text& t, const Args& g) {
  const Bytes key = row_or_empty(kd, koff, kw, i);
#if MRD_PRINT_KMV
  Values vals{vd, voff, vw, seg[i + 1] - seg[i]};
  if (voff) vals.off = voff + seg[i];
  else vals.d = vd + seg[i] * vw;
  call_print(key, vals, t, g, 0);
#else
  call_print(key, row_or_empty(vd, voff, vw, i), base + i, t, g, 0);
#endif
}
}  // namespace mrd
extern "C" __global__ __launch_bounds__(256) void
mrd_text_count(const mrd::u8* kd, const mrd::i64* koff, mrd::i64 kw, const mrd::u8* vd, const mrd::i64* voff,
               mrd::i64 vw, const mrd::i64* seg, mrd::i64 base, mrd::i64 n, mrd::i64* cnt, mrd::Args args) {
  for (mrd::i64 i = (mrd::i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (mrd::i64)gridDim.x * 256) {
    mrd::Text t{false, nullptr, 0, 0};
    mrd::print_item(kd, koff, kw, vd, voff, vw, seg, base, i, t, args);
    cnt[i] = t.n;
  }
}
extern "C" __global__ __launch_bounds__(256) void
mrd_text_write(const mrd::u8* kd, const mrd::i64* koff, mrd::i64 kw, const mrd::u8* vd, const mrd::i64* voff,
               mrd::i64 vw, const mrd::i64* seg, mrd::i64 base, mrd::i64 n, const mrd::i64* pre, mrd::u8* out,
               int stage_ok, unsigned long long* tiles, mrd::Args args) {
  using namespace mrd;
  __shared__ __attribute__((aligned(16))) u8 stage[TEXT_STAGE + 16];
  const i64 ntile = (n + TEXT_TILE - 1) / TEXT_TILE;
  for (i64 tile = blockIdx.x; tile < ntile; tile += gridDim.x) {  // uniform over the workgroup
    const i64 t0 = tile * TEXT_TILE, t1 = t0 + TEXT_TILE < n ? t0 + TEXT_TILE : n;
    const i64 o0 = pre[t0], len = pre[t1] - o0;
    const bool staged = stage_ok && len <= TEXT_STAGE;
    if (threadIdx.x == 0) atomicAdd(tiles + (staged ? 0 : 1), 1ull);
    if (len <= 0) continue;
    const i64 i = t0 + threadIdx.x;
    const i64 a = i < t1 ? pre[i] : 0, room = i < t1 ? pre[i + 1] - a : 0;
    if (!staged) {
      if (room > 0) {
        Text t{true, out + a, 0, room};
        print_item(kd, koff, kw, vd, voff, vw, seg, base, i, t, args);
      }
      continue;
    }
    const int head = (int)((unsigned long long)(out + o0) & 15);
    if (room > 0) {  // a - o0 + room <= len <= TEXT_STAGE: inside the stage
      Text t{true, stage + head + (a - o0), 0, room};
      print_item(kd, koff, kw, vd, voff, vw, seg, base, i, t, args);
    }
    __syncthreads();
    u8* line0 = out + o0 - head;  // 16-byte aligned; stage[j] belongs at line0[j]
    const int end = head + (int)len;
    for (int lo = (int)threadIdx.x * 16; lo < end; lo += 256 * 16) {
      if (lo >= head && lo + 16 <= end) {
        *reinterpret_cast<u32x4*>(line0 + lo) = *reinterpret_cast<const u32x4*>(stage + lo);
      } else {
        const int b0 = lo > head ? lo : head, b1 = lo + 16 < end ? lo + 16 : end;
        for (int b = b0; b < b1; ++b) line0[b] = stage[b];
      }
    }
    __syncthreads();  // the stage is free for the next tile
  }
}
)MRD";

// mr_map over the records of a text in HBM (devfn.h map_records): record i is
// text[off[i], off[i + 1] - trim), read in place; key = the 8 bytes of `file`,
// index = base + off[i]. The two passes of kEmitKernels with records in the
// place of pairs (a source of its own: the other kinds' sources stay as they are).
const char kTextKernels[] = R"MRD(
// ---- mrd record-map kernels ----
namespace mrd {
MRD_SHIM(map, (class E), (Bytes k, Bytes v, i64 t, E& e), (k, v, t, e))
__device__ inline void run_record(const u8* text, const i64* off, i64 trim, i64 file, i64 base, i64 i, Emit& e,
                                  const Args& g) {
  const i64 a = off[i], b = off[i + 1] - trim;
  call_map(Bytes{(const u8*)&file, 8}, Bytes{text + a, b > a ? b - a : 0}, base + a, e, g, 0);
}
}  // namespace mrd
extern "C" __global__ __launch_bounds__(256) void
mrd_count(const mrd::u8* text, const mrd::i64* off, mrd::i64 trim, mrd::i64 file, mrd::i64 base, mrd::i64 first,
          mrd::i64 n, mrd::i64* cnt, mrd::u64* wid, int bytes, mrd::Args args) {
  mrd::u64 kmin = ~0ull, kmax = 0, vmin = ~0ull, vmax = 0;
  for (mrd::i64 i = (mrd::i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (mrd::i64)gridDim.x * 256) {
    mrd::Emit e{false, 0, 0, 0, ~0ull, 0, ~0ull, 0, nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
    mrd::run_record(text, off, trim, file, base, first + i, e, args);
    cnt[i] = e.nrec;
    if (bytes) {
      cnt[n + i] = e.kb;
      cnt[2 * n + i] = e.vb;
    }
    kmin = e.kmin < kmin ? e.kmin : kmin;
    kmax = e.kmax > kmax ? e.kmax : kmax;
    vmin = e.vmin < vmin ? e.vmin : vmin;
    vmax = e.vmax > vmax ? e.vmax : vmax;
  }
  // the record widths: wave, then block min / max, one set of atomics per block
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const mrd::u64 a = __shfl_xor(kmin, d, 64), b = __shfl_xor(kmax, d, 64);
    const mrd::u64 c = __shfl_xor(vmin, d, 64), e = __shfl_xor(vmax, d, 64);
    kmin = a < kmin ? a : kmin;
    kmax = b > kmax ? b : kmax;
    vmin = c < vmin ? c : vmin;
    vmax = e > vmax ? e : vmax;
  }
  __shared__ mrd::u64 red[4][4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[w][0] = kmin;
    red[w][1] = kmax;
    red[w][2] = vmin;
    red[w][3] = vmax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i) {
      kmin = red[i][0] < kmin ? red[i][0] : kmin;
      kmax = red[i][1] > kmax ? red[i][1] : kmax;
      vmin = red[i][2] < vmin ? red[i][2] : vmin;
      vmax = red[i][3] > vmax ? red[i][3] : vmax;
    }
    if (kmax || kmin != ~0ull) {
      atomicMin(wid + 0, kmin);
      atomicMax(wid + 1, kmax);
      atomicMin(wid + 2, vmin);
      atomicMax(wid + 3, vmax);
    }
  }
}
extern "C" __global__ __launch_bounds__(256) void
mrd_write(const mrd::u8* text, const mrd::i64* off, mrd::i64 trim, mrd::i64 file, mrd::i64 base, mrd::i64 first,
          mrd::i64 n, const mrd::i64* pr, const mrd::i64* pk, const mrd::i64* pv, mrd::i64 okw, mrd::i64 ovw,
          mrd::u8* okd, mrd::i64* okoff, mrd::u8* ovd, mrd::i64* ovoff, mrd::Args args) {
  for (mrd::i64 i = (mrd::i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (mrd::i64)gridDim.x * 256) {
    const mrd::i64 r = pr[i];
    if (pr[i + 1] == r) continue;
    const mrd::i64 r1 = pr[i + 1];
    const mrd::i64 k0 = okw >= 0 ? r * okw : pk[i], v0 = ovw >= 0 ? r * ovw : pv[i];
    const mrd::i64 k1 = okw >= 0 ? r1 * okw : pk[i + 1], v1 = ovw >= 0 ? r1 * ovw : pv[i + 1];
    mrd::Emit e{true, 0, 0, 0, 0, 0, 0, 0, okd + k0, okw >= 0 ? nullptr : okoff + r, ovd + v0,
                ovw >= 0 ? nullptr : ovoff + r, r1 - r, k1 - k0, v1 - v0};
    mrd::run_record(text, off, trim, file, base, first + i, e, args);
    const mrd::i64 nw = e.nrec < r1 - r ? e.nrec : r1 - r;
    for (mrd::i64 j = 0; j < nw; ++j) {  // offsets relative to the item -> absolute
      if (okw < 0) okoff[r + j] += k0;
      if (ovw < 0) ovoff[r + j] += v0;
    }
  }
}
)MRD";

}  // namespace text
}  // namespace devfn
}  // namespace mrh
