// Device functors (devfn.h): user map / reduce device code compiled at run
// time by hiprtc for gfx950 into two kernels —
//
//   mrd_count  one thread per item (pair / task / key, grid-stride): runs the
//              functor with a counting Emit, stores the item's records, key
//              bytes and value bytes, and min/max record widths (atomics)
//   mrd_write  runs it again with a writing Emit at the item's offsets (the
//              exclusive scans of the counts) into var-width output columns
//
// A uniform output width (every key, every value the same length) turns
// into a fixed-width KV, so later ops keep their fixed-key fast paths.
// The two sort functors have kernels of their own: mrd_sortkey (a 64-bit key
// per row for the radix sort) and the comparator merge sort (kCompareKernels).
// mr_scan (kind 5) has mrd_scan: one pass, once per item, nothing emitted.
// Every kernel that runs user code takes the bound buffers (devfn.h Args) as
// its last argument, by value. Modules are cached per (device, kind, code).
#include "devfn.h"

#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <unordered_map>
#include <vector>

#include "../kernels/launch.h"

namespace mrh {
namespace devfn {

namespace {
const char* kDevicePrelude = R"MRD(
// ---- mrd: the engine's device-functor prelude (csrc/engine/devfn.cpp) ----
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
// the values of one key (reduce): n values, fixed width w or offsets off[n+1]
struct Values {
  const u8* d;
  const i64* off;
  i64 w;
  i64 n;
  __device__ Bytes operator[](i64 i) const {
    return off ? Bytes{d + off[i], off[i + 1] - off[i]} : Bytes{d + i * w, w};
  }
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
}  // namespace mrd
// ---- user code ----
)MRD";

// kernels: MRD_REDUCE selects the item kind; seg null = pairs, kd null = tasks
const char* kKernels = R"MRD(
// ---- mrd kernels ----
namespace mrd {
__device__ inline Bytes field(const u8* d, const i64* off, i64 w, i64 i) {
  if (!d) return Bytes{nullptr, 0};
  return off ? Bytes{d + off[i], off[i + 1] - off[i]} : Bytes{d + i * w, w};
}
__device__ inline i64 seg_of(const i64* seg, i64 nseg, i64 j) {
  i64 lo = 0, hi = nseg;
  while (hi - lo > 1) {
    const i64 mid = (lo + hi) >> 1;
    if (seg[mid] <= j) lo = mid;
    else hi = mid;
  }
  return lo;
}
// Every entry point may take a trailing `const mrd::Args&`, each on its own.
// Of each pair of call shims the first (tag int, preferred for the literal 0)
// is viable when the user's function takes the bound buffers, the second (tag
// long) when it does not. Both are templates whose call is dependent, so the
// form the user did not write is a substitution failure, not an error.
#if MRD_REDUCE == 2
template <class A>
__device__ auto call_init(Bytes k, A& a, const Args& g, int) -> decltype(mr_init(k, a, g), void()) { mr_init(k, a, g); }
template <class A>
__device__ auto call_init(Bytes k, A& a, const Args&, long) -> decltype(mr_init(k, a), void()) { mr_init(k, a); }
template <class A>
__device__ auto call_add(A& a, Bytes v, const Args& g, int) -> decltype(mr_add(a, v, g), void()) { mr_add(a, v, g); }
template <class A>
__device__ auto call_add(A& a, Bytes v, const Args&, long) -> decltype(mr_add(a, v), void()) { mr_add(a, v); }
template <class A>
__device__ auto call_merge(A& a, const A& b, const Args& g, int) -> decltype(mr_merge(a, b, g), void()) { mr_merge(a, b, g); }
template <class A>
__device__ auto call_merge(A& a, const A& b, const Args&, long) -> decltype(mr_merge(a, b), void()) { mr_merge(a, b); }
template <class A, class E>
__device__ auto call_finish(Bytes k, const A& a, E& e, const Args& g, int) -> decltype(mr_finish(k, a, e, g), void()) {
  mr_finish(k, a, e, g);
}
template <class A, class E>
__device__ auto call_finish(Bytes k, const A& a, E& e, const Args&, long) -> decltype(mr_finish(k, a, e), void()) {
  mr_finish(k, a, e);
}
#elif MRD_REDUCE
template <class E>
__device__ auto call_reduce(Bytes k, Values v, E& e, const Args& g, int) -> decltype(mr_reduce(k, v, e, g), void()) {
  mr_reduce(k, v, e, g);
}
template <class E>
__device__ auto call_reduce(Bytes k, Values v, E& e, const Args&, long) -> decltype(mr_reduce(k, v, e), void()) {
  mr_reduce(k, v, e);
}
#else
template <class E>
__device__ auto call_map(Bytes k, Bytes v, i64 t, E& e, const Args& g, int) -> decltype(mr_map(k, v, t, e, g), void()) {
  mr_map(k, v, t, e, g);
}
template <class E>
__device__ auto call_map(Bytes k, Bytes v, i64 t, E& e, const Args&, long) -> decltype(mr_map(k, v, t, e), void()) {
  mr_map(k, v, t, e);
}
#endif
__device__ inline void run_item(const u8* kd, const i64* koff, i64 kw, const u8* vd, const i64* voff, i64 vw,
                                const i64* seg, i64 first, i64 i, Emit& e, const Args& g) {
#if MRD_REDUCE == 2
  // fold: vd = the merged accumulators, voff = each key's first chunk, vw = sizeof(mr_acc)
  mr_acc a;
  __builtin_memcpy(&a, vd + voff[i] * vw, sizeof(mr_acc));
  call_finish(field(kd, koff, kw, i), a, e, g, 0);
#elif MRD_REDUCE
  Values vals{vd + 0, voff, vw, seg[i + 1] - seg[i]};
  if (voff) vals.off = voff + seg[i];
  else vals.d = vd + seg[i] * vw;
  call_reduce(field(kd, koff, kw, i), vals, e, g, 0);
#else
  call_map(field(kd, koff, kw, first + i), field(vd, voff, vw, first + i), first + i, e, g, 0);
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
    mrd::call_init(mrd::field(kd, koff, kw, s), a, args, 0);
    for (mrd::i64 v = a0; v < a1; ++v) mrd::call_add(a, mrd::field(vd, voff, vw, v), args, 0);
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

// kind 3: a sort-key functor, __device__ unsigned long long mr_sortkey(mrd::Bytes)
const char* kSortKernel = R"MRD(
// ---- mrd sort-key kernel ----
namespace mrd {
// mr_sortkey with or without the trailing `const mrd::Args&` (the call shims of the map / reduce kernels)
template <class B>
__device__ auto call_sortkey(B b, const Args& g, int) -> decltype(mr_sortkey(b, g)) { return mr_sortkey(b, g); }
template <class B>
__device__ auto call_sortkey(B b, const Args&, long) -> decltype(mr_sortkey(b)) { return mr_sortkey(b); }
}  // namespace mrd
extern "C" __global__ __launch_bounds__(256) void
mrd_sortkey(const mrd::u8* d, const mrd::i64* off, mrd::i64 w, mrd::i64 n, mrd::u64* key, unsigned int* idx,
            mrd::Args args) {
  for (mrd::i64 i = (mrd::i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (mrd::i64)gridDim.x * 256) {
    const mrd::Bytes b = off ? mrd::Bytes{d + off[i], off[i + 1] - off[i]} : mrd::Bytes{d + i * w, w};
    key[i] = mrd::call_sortkey(b, args, 0);
    idx[i] = (unsigned int)i;
  }
}
)MRD";

// kind 4: a comparator functor, __device__ int mr_compare(mrd::Bytes a, mrd::Bytes b)
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
const char* kCompareKernels = R"MRD(
// ---- mrd comparator merge sort ----
namespace mrd {
typedef unsigned int u32;
enum { CMP_T = MRD_CMP_T, CMP_PER = MRD_CMP_T / 256 };
// mr_compare with or without the trailing `const mrd::Args&` (the call shims of the map / reduce kernels)
template <class B>
__device__ auto call_compare(B a, B b, const Args& g, int) -> decltype(mr_compare(a, b, g)) { return mr_compare(a, b, g); }
template <class B>
__device__ auto call_compare(B a, B b, const Args&, long) -> decltype(mr_compare(a, b)) { return mr_compare(a, b); }
struct Cmp {
  const u8* d;
  const i64* off;
  i64 w;
  const i64* sid;  // segment id of every row, compared first (null: no segments)
  const Args& g;   // the bound buffers (the kernel's own argument)
  __device__ Bytes row(u32 i) const { return off ? Bytes{d + off[i], off[i + 1] - off[i]} : Bytes{d + i * w, w}; }
  __device__ bool less(u32 i, u32 j) const {
    if (sid) {
      const i64 a = sid[i], b = sid[j];
      if (a != b) return a < b;
    }
    const int c = call_compare(row(i), row(j), g, 0);
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

// kind 5: a scan functor, mr_scan in its KV (MRD_SCAN_KMV 0) or KMV (1) shape.
// One thread per item, every item exactly once; nothing is emitted, the
// functor writes to the bound buffers (mrd::MutArgs).
const char* kScanKernel = R"MRD(
// ---- mrd scan kernel ----
extern "C" __global__ __launch_bounds__(256) void
mrd_scan(const mrd::u8* kd, const mrd::i64* koff, mrd::i64 kw, const mrd::u8* vd, const mrd::i64* voff, mrd::i64 vw,
         const mrd::i64* seg, mrd::i64 base, mrd::i64 n, mrd::MutArgs args) {
  for (mrd::i64 i = (mrd::i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (mrd::i64)gridDim.x * 256) {
    const mrd::Bytes key = koff ? mrd::Bytes{kd + koff[i], koff[i + 1] - koff[i]} : mrd::Bytes{kd + i * kw, kw};
#if MRD_SCAN_KMV
    mrd::Values vals{vd, voff, vw, seg[i + 1] - seg[i]};
    if (voff) vals.off = voff + seg[i];
    else vals.d = vd + seg[i] * vw;
    mr_scan(key, vals, args);
#else
    const mrd::Bytes val = voff ? mrd::Bytes{vd + voff[i], voff[i + 1] - voff[i]} : mrd::Bytes{vd + i * vw, vw};
    mr_scan(key, val, base + i, args);
#endif
  }
}
)MRD";

struct Module {
  hipModule_t mod = nullptr;
  hipFunction_t count = nullptr, write = nullptr;
  hipFunction_t acc_size = nullptr, nchunks = nullptr, chunks = nullptr, merge = nullptr;  // fold tier
};
const char* kind_name(int kind) {
  return kind == 0   ? "mrd_map.hip"
         : kind == 1 ? "mrd_reduce.hip"
         : kind == 2 ? "mrd_fold.hip"
         : kind == 3 ? "mrd_sortkey.hip"
         : kind == 4 ? "mrd_compare.hip"
                     : "mrd_scan.hip";
}
// rows per workgroup tile of the comparator sort (256 threads, 8 rows each)
constexpr int64_t kCompareTile = 2048;
// kind 5 (scan): code = scan_code(user code, kmv), the shape's define in front
std::string scan_code(const std::string& code, bool kmv) {
  return std::string("#define MRD_SCAN_KMV ") + (kmv ? "1\n" : "0\n") + code;
}
std::string source_of(const std::string& code, int kind) {
  if (kind == 5) {  // the define goes before the prelude like the others'
    const size_t nl = code.find('\n');
    return code.substr(0, nl + 1) + kDevicePrelude + code.substr(nl + 1) + "\n" + kScanKernel;
  }
  if (kind == 3) return std::string(kDevicePrelude) + code + "\n" + kSortKernel;
  if (kind == 4)
    return "#define MRD_CMP_T " + std::to_string(kCompareTile) + "\n" + kDevicePrelude + code + "\n" + kCompareKernels;
  return "#define MRD_REDUCE " + std::to_string(kind) + "\n" + kDevicePrelude + code + "\n" + kKernels;
}

std::atomic<int64_t> g_compiles{0};

std::string compile(const std::string& src, const char* name) {
  g_compiles++;
  hiprtcProgram p;
  if (hiprtcCreateProgram(&p, src.c_str(), name, 0, nullptr, nullptr) != HIPRTC_SUCCESS)
    throw std::runtime_error("mrhip: hiprtcCreateProgram failed");
  const char* opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17"};
  const hiprtcResult r = hiprtcCompileProgram(p, 3, opts);
  size_t ls = 0;
  hiprtcGetProgramLogSize(p, &ls);
  std::string log(ls, '\0');
  if (ls) hiprtcGetProgramLog(p, &log[0]);
  if (r != HIPRTC_SUCCESS) {
    hiprtcDestroyProgram(&p);
    throw std::runtime_error("mrhip: device functor does not compile:\n" + log);
  }
  size_t cs = 0;
  hiprtcGetCodeSize(p, &cs);
  std::string code(cs, '\0');
  hiprtcGetCode(p, &code[0]);
  hiprtcDestroyProgram(&p);
  return code;
}

const Module& module_for(const std::string& code, int kind, int device) {
  static std::mutex mu;
  static std::unordered_map<std::string, std::unique_ptr<Module>> cache;
  const std::string key = std::to_string(device) + ":" + std::to_string(kind) + ":" + code;
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find(key);
  if (it != cache.end()) return *it->second;
  const std::string obj = compile(source_of(code, kind), kind_name(kind));
  auto m = std::make_unique<Module>();
  if (kind == 3) {
    if (hipModuleLoadData(&m->mod, obj.data()) != hipSuccess ||
        hipModuleGetFunction(&m->count, m->mod, "mrd_sortkey") != hipSuccess) {
      (void)hipGetLastError();
      throw std::runtime_error("mrhip: loading the sort-key functor's code object failed");
    }
    return *cache.emplace(key, std::move(m)).first->second;
  }
  if (kind == 5) {
    if (hipModuleLoadData(&m->mod, obj.data()) != hipSuccess ||
        hipModuleGetFunction(&m->count, m->mod, "mrd_scan") != hipSuccess) {
      (void)hipGetLastError();
      throw std::runtime_error("mrhip: loading the scan functor's code object failed");
    }
    return *cache.emplace(key, std::move(m)).first->second;
  }
  if (kind == 4) {  // count = the tile sort, write = the merge pass
    if (hipModuleLoadData(&m->mod, obj.data()) != hipSuccess ||
        hipModuleGetFunction(&m->count, m->mod, "mrd_cmp_blocksort") != hipSuccess ||
        hipModuleGetFunction(&m->write, m->mod, "mrd_cmp_merge") != hipSuccess) {
      (void)hipGetLastError();
      throw std::runtime_error("mrhip: loading the comparator functor's code object failed");
    }
    return *cache.emplace(key, std::move(m)).first->second;
  }
  if (hipModuleLoadData(&m->mod, obj.data()) != hipSuccess ||
      hipModuleGetFunction(&m->count, m->mod, "mrd_count") != hipSuccess ||
      hipModuleGetFunction(&m->write, m->mod, "mrd_write") != hipSuccess ||
      (kind == 2 && (hipModuleGetFunction(&m->acc_size, m->mod, "mrd_acc_size") != hipSuccess ||
                     hipModuleGetFunction(&m->nchunks, m->mod, "mrd_fold_nchunks") != hipSuccess ||
                     hipModuleGetFunction(&m->chunks, m->mod, "mrd_fold_chunks") != hipSuccess ||
                     hipModuleGetFunction(&m->merge, m->mod, "mrd_fold_merge") != hipSuccess))) {
    (void)hipGetLastError();
    throw std::runtime_error("mrhip: loading the device functor's code object failed");
  }
  return *cache.emplace(key, std::move(m)).first->second;
}

template <typename T>
T* P0(const at::Tensor& t) {
  return t.defined() && t.numel() ? reinterpret_cast<T*>(t.data_ptr()) : nullptr;
}
at::TensorOptions opt(at::Device d, at::ScalarType t) { return at::TensorOptions().device(d).dtype(t); }

void launch(hipFunction_t f, int64_t n, void** args, hipStream_t s) {
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 65536));
  if (hipModuleLaunchKernel(f, grid, 1, 1, 256, 1, 1, 0, s, args, nullptr) != hipSuccess) {
    (void)hipGetLastError();
    throw std::runtime_error("mrhip: device functor launch failed");
  }
}

struct Items {
  const uint8_t* kd = nullptr;
  const int64_t* koff = nullptr;
  int64_t kw = 0;
  const uint8_t* vd = nullptr;
  const int64_t* voff = nullptr;
  int64_t vw = 0;
  const int64_t* seg = nullptr;
  int64_t first = 0, n = 0;
};

KV run(const Items& it, const std::string& code, int kind, at::Device dev, const Args& bound) {
  if (!dev.is_cuda()) throw std::runtime_error("mrhip: device functors run on a GPU MapReduce (device cuda)");
  KV out;
  out.kw = out.vw = -1;
  if (it.n <= 0) {
    out.kw = out.vw = 0;
    out.kdata = at::empty({0}, opt(dev, at::kByte));
    out.vdata = at::empty({0}, opt(dev, at::kByte));
    return out;
  }
  const Module& m = module_for(code, kind, dev.index());
  hipStream_t s = at::hip::getCurrentHIPStream();
  at::Tensor cnt = at::empty({3 * it.n}, opt(dev, at::kLong));
  at::Tensor wid = at::empty({4}, opt(dev, at::kLong));
  const int64_t w0[4] = {-1, 0, -1, 0};  // ~0 = u64 max for the mins
  if (hipMemcpyAsync(wid.data_ptr(), w0, sizeof(w0), hipMemcpyHostToDevice, s) != hipSuccess)
    throw std::runtime_error("mrhip: hipMemcpyAsync failed");
  auto count = [&](int bytes) {
    const uint8_t* kd = it.kd;
    const int64_t* koff = it.koff;
    int64_t kw = it.kw, vw = it.vw, first = it.first, n = it.n;
    const uint8_t* vd = it.vd;
    const int64_t* voff = it.voff;
    const int64_t* seg = it.seg;
    int64_t* c = P0<int64_t>(cnt);
    int64_t* w = P0<int64_t>(wid);
    int b = bytes;
    Args g = bound;
    void* args[] = {&kd, &koff, &kw, &vd, &voff, &vw, &seg, &first, &n, &c, &w, &b, &g};
    launch(m.count, it.n, args, s);
  };
  count(0);
  // the record widths first: uniform widths need only the record scan (the
  // common case); otherwise a second count pass fills the byte columns
  int64_t wh[4] = {0, 0, 0, 0};
  read_small(s, {{P0<int64_t>(wid), wh, 32}});
  const int64_t okw = (wh[0] == wh[1]) ? wh[0] : -1, ovw = (wh[2] == wh[3]) ? wh[2] : -1;
  if (okw < 0 || ovw < 0) count(1);
  at::Tensor pr = exclusive_scan(cnt.narrow(0, 0, it.n));
  at::Tensor pk = okw < 0 ? exclusive_scan(cnt.narrow(0, it.n, it.n)) : at::Tensor();
  at::Tensor pv = ovw < 0 ? exclusive_scan(cnt.narrow(0, 2 * it.n, it.n)) : at::Tensor();
  int64_t tot[3] = {0, 0, 0};
  {
    const SmallRead rec{P0<int64_t>(pr) + it.n, &tot[0], 8};
    if (okw < 0 && ovw < 0)
      read_small(s, {rec, {P0<int64_t>(pk) + it.n, &tot[1], 8}, {P0<int64_t>(pv) + it.n, &tot[2], 8}});
    else if (okw < 0) read_small(s, {rec, {P0<int64_t>(pk) + it.n, &tot[1], 8}});
    else if (ovw < 0) read_small(s, {rec, {P0<int64_t>(pv) + it.n, &tot[2], 8}});
    else read_small(s, {rec});
  }
  const int64_t nout = tot[0];
  if (okw >= 0) tot[1] = nout * okw;
  if (ovw >= 0) tot[2] = nout * ovw;
  out.n = nout;
  out.kdata = at::empty({tot[1]}, opt(dev, at::kByte));
  out.vdata = at::empty({tot[2]}, opt(dev, at::kByte));
  if (nout && okw >= 0) out.kw = (int)okw;
  else out.koff = at::empty({nout + 1}, opt(dev, at::kLong));
  if (nout && ovw >= 0) out.vw = (int)ovw;
  else out.voff = at::empty({nout + 1}, opt(dev, at::kLong));
  if (nout) {
    const uint8_t* kd = it.kd;
    const int64_t* koff = it.koff;
    int64_t kw = it.kw, vw = it.vw, first = it.first, n = it.n, kwo = okw, vwo = ovw;
    const uint8_t* vd = it.vd;
    const int64_t* voff = it.voff;
    const int64_t* seg = it.seg;
    const int64_t* ppr = P0<int64_t>(pr);
    const int64_t* ppk = P0<int64_t>(pk);
    const int64_t* ppv = P0<int64_t>(pv);
    uint8_t* okd = P0<uint8_t>(out.kdata);
    uint8_t* ovd = P0<uint8_t>(out.vdata);
    int64_t* okoff = P0<int64_t>(out.koff);
    int64_t* ovoff = P0<int64_t>(out.voff);
    Args g = bound;
    void* args[] = {&kd, &koff, &kw, &vd, &voff, &vw,  &seg, &first, &n,     &ppr,
                    &ppk, &ppv, &kwo, &vwo, &okd, &okoff, &ovd, &ovoff, &g};
    launch(m.write, it.n, args, s);
  }
  if (out.koff.defined()) k::fill_i64(P0<int64_t>(out.koff) + nout, 1, tot[1], s);
  if (out.voff.defined()) k::fill_i64(P0<int64_t>(out.voff) + nout, 1, tot[2], s);
  return out;
}
}  // namespace

int kind_of(const std::string& code, bool reduce) {
  return !reduce ? 0 : code.find("mr_finish") != std::string::npos ? 2 : 1;
}

std::string full_source(const std::string& code, bool reduce) { return source_of(code, kind_of(code, reduce)); }

int64_t compile_check_sortkey(const std::string& code) {
  return (int64_t)compile(source_of(code, 3), kind_name(3)).size();
}

std::pair<at::Tensor, at::Tensor> sort_keys_of(const at::Tensor& data, const at::Tensor& off, int w, int64_t n,
                                               const std::string& code, at::Device dev, const Args& bound) {
  if (!dev.is_cuda()) throw std::runtime_error("mrhip: device functors run on a GPU MapReduce (device cuda)");
  at::Tensor key = at::empty({std::max<int64_t>(n, 1)}, opt(dev, at::kLong));
  at::Tensor idx = at::empty({std::max<int64_t>(n, 1)}, opt(dev, at::kInt));
  if (n > 0) {
    const Module& m = module_for(code, 3, dev.index());
    const uint8_t* d = P0<uint8_t>(data);
    const int64_t* o = w >= 0 ? nullptr : P0<int64_t>(off);
    int64_t ww = w >= 0 ? w : 0, nn = n;
    int64_t* k = P0<int64_t>(key);
    int32_t* ix = P0<int32_t>(idx);
    Args g = bound;
    void* args[] = {&d, &o, &ww, &nn, &k, &ix, &g};
    launch(m.count, n, args, at::hip::getCurrentHIPStream());
  }
  return {key.narrow(0, 0, n), idx.narrow(0, 0, n)};
}

int sort_kind_of(const std::string& code) {
  if (code.find("mr_sortkey") != std::string::npos) return 3;
  if (code.find("mr_compare") != std::string::npos) return 4;
  throw std::runtime_error(
      "mrhip: a device sort functor defines `unsigned long long mr_sortkey(mrd::Bytes)` (radix sort by a 64-bit key) "
      "or `int mr_compare(mrd::Bytes, mrd::Bytes)` (merge sort by a comparator); the code has neither");
}

int64_t compile_check_compare(const std::string& code) {
  return (int64_t)compile(source_of(code, 4), kind_name(4)).size();
}

int64_t compare_tile() { return kCompareTile; }

at::Tensor compare_perm(const at::Tensor& data, const at::Tensor& off, int w, int64_t n, const at::Tensor& sid,
                        const std::string& code, at::Device dev, const Args& bound) {
  if (!dev.is_cuda()) throw std::runtime_error("mrhip: device functors run on a GPU MapReduce (device cuda)");
  if (n > (int64_t)UINT32_MAX)
    throw std::runtime_error("mrhip: the comparator sort indexes rows with 32 bits; " + std::to_string(n) +
                             " rows are more than 4294967295");
  if (sid.defined() && sid.numel() < n) throw std::runtime_error("mrhip: compare_perm: fewer segment ids than rows");
  at::Tensor a = at::empty({std::max<int64_t>(n, 1)}, opt(dev, at::kInt));
  if (n <= 0) return a.narrow(0, 0, 0);
  at::Tensor b = n > kCompareTile ? at::empty({n}, opt(dev, at::kInt)) : at::Tensor();
  const Module& m = module_for(code, 4, dev.index());
  hipStream_t s = at::hip::getCurrentHIPStream();
  const unsigned tiles = (unsigned)((n + kCompareTile - 1) / kCompareTile);
  const uint8_t* d = P0<uint8_t>(data);
  const int64_t* o = w >= 0 ? nullptr : P0<int64_t>(off);
  const int64_t* sg = P0<int64_t>(sid);
  int64_t ww = w >= 0 ? w : 0, nn = n;
  uint32_t* src = P0<uint32_t>(a);
  uint32_t* dst = P0<uint32_t>(b);
  Args g = bound;
  auto go = [&](hipFunction_t f, void** args) {
    if (hipModuleLaunchKernel(f, tiles, 1, 1, 256, 1, 1, 0, s, args, nullptr) != hipSuccess) {
      (void)hipGetLastError();
      throw std::runtime_error("mrhip: device functor launch failed");
    }
  };
  {
    void* args[] = {&d, &o, &ww, &sg, &nn, &src, &g};
    go(m.count, args);
  }
  // ceil(log2(tiles)) passes, known from n alone: nothing is read back between them
  for (int64_t W = kCompareTile; W < n; W *= 2) {
    void* args[] = {&d, &o, &ww, &sg, &nn, &src, &dst, &W, &g};
    go(m.write, args);
    std::swap(src, dst);
    std::swap(a, b);
  }
  return a;
}

int64_t compile_check(const std::string& code, bool reduce) {
  return (int64_t)compile(full_source(code, reduce), kind_name(kind_of(code, reduce))).size();
}

KV map_pairs(const KV& kv_in, const std::string& code, at::Device dev, int64_t a, int64_t b, const Args& bound) {
  KV kv = kv_in.device() == dev ? kv_in : kv_to(kv_in, dev);
  if (b < 0 || b > kv.n) b = kv.n;
  Items it;
  it.first = a;
  it.kd = P0<uint8_t>(kv.kdata);
  it.koff = kv.kfixed() ? nullptr : P0<int64_t>(kv.koff);
  it.kw = kv.kfixed() ? kv.kw : 0;
  it.vd = P0<uint8_t>(kv.vdata);
  it.voff = kv.vfixed() ? nullptr : P0<int64_t>(kv.voff);
  it.vw = kv.vfixed() ? kv.vw : 0;
  it.n = std::max<int64_t>(0, b - a);
  return run(it, code, 0, dev, bound);
}

KV map_tasks(int64_t first, int64_t n, const std::string& code, at::Device dev, const Args& bound) {
  Items it;
  it.first = first;
  it.n = n;
  return run(it, code, 0, dev, bound);
}

KV reduce_groups(const KMV& m, const std::string& code, at::Device dev, const Args& bound) {
  if (m.nkey && !m.seg.is_cuda()) throw std::runtime_error("mrhip: reduce_device needs the groups in HBM");
  Items it;
  const KV& k = m.keys;
  it.kd = P0<uint8_t>(k.kdata);
  it.koff = k.kfixed() ? nullptr : P0<int64_t>(k.koff);
  it.kw = k.kfixed() ? k.kw : 0;
  it.vd = P0<uint8_t>(m.vdata);
  it.voff = m.vw >= 0 ? nullptr : P0<int64_t>(m.voff);
  it.vw = m.vw >= 0 ? m.vw : 0;
  it.seg = P0<int64_t>(m.seg);
  it.n = m.nkey;
  if (kind_of(code, true) == 1) return run(it, code, 1, dev, bound);
  // fold tier: accumulators per chunk of values, merged per key, then mr_finish per key
  if (!it.n) return run(it, code, 2, dev, bound);
  const Module& mod = module_for(code, 2, dev.index());
  hipStream_t s = at::hip::getCurrentHIPStream();
  static const int64_t C = [] {
    const char* e = std::getenv("MRH_FOLD_CHUNK");
    return e && std::atoll(e) > 0 ? std::atoll(e) : int64_t(256);
  }();
  at::Tensor asz_t = at::empty({1}, opt(dev, at::kLong));
  {
    int64_t* o = P0<int64_t>(asz_t);
    void* args[] = {&o};
    launch(mod.acc_size, 1, args, s);
  }
  at::Tensor cnt = at::empty({it.n + 1}, opt(dev, at::kLong));  // + the most chunks of one key
  if (hipMemsetAsync(P0<int64_t>(cnt) + it.n, 0, 8, s) != hipSuccess)
    throw std::runtime_error("mrhip: hipMemsetAsync failed");
  {
    const int64_t* seg = it.seg;
    int64_t nkey = it.n, c = C;
    int64_t* o = P0<int64_t>(cnt);
    int64_t* mx = o + it.n;
    void* args[] = {&seg, &nkey, &c, &o, &mx};
    launch(mod.nchunks, it.n, args, s);
  }
  at::Tensor cstart = exclusive_scan(cnt.narrow(0, 0, it.n));
  int64_t asz = 0, nchunk = 0, maxc = 0;
  read_small(s, {{P0<int64_t>(asz_t), &asz, 8}, {P0<int64_t>(cstart) + it.n, &nchunk, 8},
                 {P0<int64_t>(cnt) + it.n, &maxc, 8}});
  at::Tensor accs = at::empty({std::max<int64_t>(1, nchunk * asz)}, opt(dev, at::kByte));
  {
    const uint8_t* kd = it.kd;
    const int64_t* koff = it.koff;
    int64_t kw = it.kw, vw = it.vw, nkey = it.n, nc = nchunk, c = C;
    const uint8_t* vd = it.vd;
    const int64_t* voff = it.voff;
    const int64_t* seg = it.seg;
    const int64_t* cs = P0<int64_t>(cstart);
    uint8_t* a = P0<uint8_t>(accs);
    Args g = bound;
    void* args[] = {&kd, &koff, &kw, &vd, &voff, &vw, &seg, &nkey, &cs, &nc, &c, &a, &g};
    launch(mod.chunks, nchunk, args, s);
    for (int64_t stride = 1; stride < maxc; stride *= 2) {
      int64_t st = stride;
      void* margs[] = {&cs, &nkey, &nc, &st, &a, &g};
      launch(mod.merge, nchunk, margs, s);
    }
  }
  Items f = it;
  f.vd = P0<uint8_t>(accs);
  f.voff = P0<int64_t>(cstart);
  f.vw = asz;
  f.seg = nullptr;
  return run(f, code, 2, dev, bound);
}

Args args_of(const std::vector<at::Tensor>& bufs) {
  if ((int)bufs.size() > kMaxArgs)
    throw std::runtime_error("mrhip: a device functor takes at most 8 bound buffers, " + std::to_string(bufs.size()) +
                             " given");
  Args g{};
  g.n = (int)bufs.size();
  for (int i = 0; i < g.n; ++i) g.a[i] = {bufs[i].numel() ? bufs[i].data_ptr() : nullptr, (int64_t)bufs[i].nbytes()};
  return g;
}

int64_t compile_count() { return g_compiles.load(); }

int64_t compile_check_scan(const std::string& code, bool kmv) {
  return (int64_t)compile(source_of(scan_code(code, kmv), 5), kind_name(5)).size();
}

namespace {
int64_t run_scan(const Items& it, const std::string& code, bool kmv, at::Device dev, const Args& bound) {
  if (!dev.is_cuda()) throw std::runtime_error("mrhip: device functors run on a GPU MapReduce (device cuda)");
  if (it.n <= 0) return 0;
  const Module& m = module_for(scan_code(code, kmv), 5, dev.index());
  const uint8_t* kd = it.kd;
  const int64_t* koff = it.koff;
  int64_t kw = it.kw, vw = it.vw, base = it.first, n = it.n;
  const uint8_t* vd = it.vd;
  const int64_t* voff = it.voff;
  const int64_t* seg = it.seg;
  Args g = bound;
  void* args[] = {&kd, &koff, &kw, &vd, &voff, &vw, &seg, &base, &n, &g};
  launch(m.count, it.n, args, at::hip::getCurrentHIPStream());
  return it.n;
}
}  // namespace

int64_t scan_pairs(const KV& kv_in, int64_t base, const std::string& code, at::Device dev, const Args& bound) {
  if (!dev.is_cuda()) throw std::runtime_error("mrhip: device functors run on a GPU MapReduce (device cuda)");
  KV kv = kv_in.device() == dev ? kv_in : kv_to(kv_in, dev);
  Items it;
  it.first = base;
  it.kd = P0<uint8_t>(kv.kdata);
  it.koff = kv.kfixed() ? nullptr : P0<int64_t>(kv.koff);
  it.kw = kv.kfixed() ? kv.kw : 0;
  it.vd = P0<uint8_t>(kv.vdata);
  it.voff = kv.vfixed() ? nullptr : P0<int64_t>(kv.voff);
  it.vw = kv.vfixed() ? kv.vw : 0;
  it.n = kv.n;
  return run_scan(it, code, false, dev, bound);
}

int64_t scan_groups(const KMV& m, const std::string& code, at::Device dev, const Args& bound) {
  if (!dev.is_cuda()) throw std::runtime_error("mrhip: device functors run on a GPU MapReduce (device cuda)");
  if (m.nkey && !m.seg.is_cuda()) throw std::runtime_error("mrhip: scan_device needs the groups in HBM");
  Items it;
  const KV& k = m.keys;
  it.kd = P0<uint8_t>(k.kdata);
  it.koff = k.kfixed() ? nullptr : P0<int64_t>(k.koff);
  it.kw = k.kfixed() ? k.kw : 0;
  it.vd = P0<uint8_t>(m.vdata);
  it.voff = m.vw >= 0 ? nullptr : P0<int64_t>(m.voff);
  it.vw = m.vw >= 0 ? m.vw : 0;
  it.seg = P0<int64_t>(m.seg);
  it.n = m.nkey;
  return run_scan(it, code, true, dev, bound);
}

}  // namespace devfn
}  // namespace mrh
