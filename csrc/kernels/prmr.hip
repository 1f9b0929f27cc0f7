// pagerank_mr: PageRank as an iterated MapReduce (oinkdoc/pagerank.txt; the
// iteration of gpu_mapreduce_amd/models/pagerank.py) — its two compress
// callbacks as device kernels on the KMV columns. Records are 8-byte words:
//
//   EDGEW   {vj, w (double)}     16 B   an out-edge of the key, w = 1/outdeg
//   CONTRIB {x (double)}          8 B   w * r of one in-edge of the key
//   RANK    {r (double), 0, 0}   24 B   the key's rank (exactly one per group)
//
// Both joins tell their two kinds of value apart by length. An R-MAT hub holds
// millions of values in one group, so everything that reads values is
// value-parallel (a value's key comes from the engine's segment_ids column)
// and every sum is a fixed-order segmented reduction (segred.h): no
// floating-point atomics, results are bitwise reproducible. The per-key RANK
// counts are integer atomics (order-independent).
#include <algorithm>

#include "common.h"
#include "launch.h"
#include "segred.h"

namespace mrh {
namespace k {
namespace {

constexpr int NT = 256;
// memory-bound grid-stride kernels: 256 CUs x 8 blocks
inline unsigned blocks(int64_t n) { return (unsigned)std::min<int64_t>((n + NT - 1) / NT, 2048); }

#define GRID_LOOP(i, n) for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < (n); i += (int64_t)gridDim.x * NT)

__device__ inline double ldd(const uint8_t* p) {
  double v;
  __builtin_memcpy(&v, p, 8);
  return v;
}
__device__ inline double as_d(int64_t b) { return __longlong_as_double(b); }
__device__ inline int64_t as_l(double d) { return __double_as_longlong(d); }
__device__ inline int64_t vlen(const int64_t* __restrict__ voff, int64_t vw, int64_t j) {
  return voff ? voff[j + 1] - voff[j] : vw;
}
__device__ inline int64_t vbeg(const int64_t* __restrict__ voff, int64_t vw, int64_t j) {
  return voff ? voff[j] : j * vw;
}
// a 16-byte record: one dwordx4 access where the address allows it (value
// starts are multiples of 8, so every other EDGEW of a group is 16-aligned)
__device__ inline longlong2 ld16(const uint8_t* p) {
  if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) return *reinterpret_cast<const longlong2*>(p);
  longlong2 v;
  __builtin_memcpy(&v.x, p, 8);
  __builtin_memcpy(&v.y, p + 8, 8);
  return v;
}

// ------------------------------------------------------------------ scatter

// value-parallel: EDGEW values set their flag; the RANK writes rank[key] and
// counts itself (a value of any other length counts twice: never "one RANK")
__global__ __launch_bounds__(NT) void k_pr_scatter_mark(const int64_t* __restrict__ voff, int64_t vw,
                                                       const uint8_t* __restrict__ vd,
                                                       const int64_t* __restrict__ sid, int64_t nval,
                                                       double* __restrict__ rank,
                                                       unsigned long long* __restrict__ cnt,
                                                       int64_t* __restrict__ flag) {
  GRID_LOOP(j, nval) {
    const int64_t l = vlen(voff, vw, j);
    flag[j] = l == 16;
    if (l == 16) continue;
    const int64_t s = sid[j];
    if (l == 24) {
      rank[s] = ldd(vd + vbeg(voff, vw, j));
      atomicAdd(cnt + s, 1ull);
    } else {
      atomicAdd(cnt + s, 2ull);
    }
  }
}
// key-parallel: the keys without exactly one RANK add PRMR_BAD to the flag
// column's tail, so the one scan total read by the host carries the edge count
// (low bits) and the contract check (high bits)
constexpr int64_t PRMR_BAD = int64_t(1) << 40;
__global__ __launch_bounds__(NT) void k_pr_scatter_keys(int64_t nkey, const unsigned long long* __restrict__ cnt,
                                                       int64_t* __restrict__ ktail, int64_t* __restrict__ oneseg) {
  GRID_LOOP(s, nkey) ktail[s] = cnt[s] == 1ull ? 0 : PRMR_BAD;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    oneseg[0] = 0;
    oneseg[1] = nkey;
  }
}
// the rank of a key whose group is its lone RANK (no out-edge), else 0
struct DanglingGet {
  const int64_t* seg;
  const double* rank;
  __device__ __forceinline__ double operator()(int64_t s) const { return seg[s + 1] - seg[s] == 1 ? rank[s] : 0.0; }
};
// value-parallel: every EDGEW goes back as (vi, EDGEW) and sends (vj, w * r_vi)
__global__ __launch_bounds__(NT) void k_pr_scatter_emit(const int64_t* __restrict__ voff,
                                                       const uint8_t* __restrict__ vd,
                                                       const int64_t* __restrict__ sid,
                                                       const int64_t* __restrict__ keys,
                                                       const int64_t* __restrict__ pos,
                                                       const double* __restrict__ rank, int64_t nval,
                                                       int64_t* __restrict__ ekeys, longlong2* __restrict__ edges,
                                                       int64_t* __restrict__ ckeys, int64_t* __restrict__ contrib) {
  GRID_LOOP(j, nval) {
    const int64_t b = voff[j];
    if (voff[j + 1] - b != 16) continue;
    const int64_t p = pos[j], s = sid[j];
    const longlong2 e = ld16(vd + b);
    ekeys[p] = keys[s];
    edges[p] = e;
    ckeys[p] = e.x;
    contrib[p] = as_l(as_d(e.y) * rank[s]);
  }
}

// ------------------------------------------------------------------ update

// value-parallel pre-pass: the RANK writes its value index to its key
__global__ __launch_bounds__(NT) void k_pr_update_mark(const int64_t* __restrict__ voff, int64_t vw,
                                                      const int64_t* __restrict__ sid, int64_t nval,
                                                      int64_t* __restrict__ ridx,
                                                      unsigned long long* __restrict__ cnt) {
  GRID_LOOP(j, nval) {
    const int64_t l = vlen(voff, vw, j);
    if (l == 8) continue;
    const int64_t s = sid[j];
    if (l == 24) {
      ridx[s] = j;
      atomicAdd(cnt + s, 1ull);
    } else {
      atomicAdd(cnt + s, 2ull);
    }
  }
}
// the double of a CONTRIB value, 0 for the RANK
struct ContribGetMR {
  const int64_t* voff;
  int64_t vw;
  const uint8_t* vd;
  __device__ __forceinline__ double operator()(int64_t j) const {
    if (!voff) return vw == 8 ? ldd(vd + j * 8) : 0.0;
    const int64_t b = voff[j];
    return voff[j + 1] - b == 8 ? ldd(vd + b) : 0.0;
  }
};
struct LoadDouble {
  const double* v;
  __device__ __forceinline__ double operator()(int64_t i) const { return v[i]; }
};
// key-parallel: r' = base + alpha * (sum + dterm), RANK{r'} and |r' - r|
__global__ __launch_bounds__(NT) void k_pr_update_keys(int64_t nkey, const int64_t* __restrict__ voff, int64_t vw,
                                                      const uint8_t* __restrict__ vd,
                                                      const int64_t* __restrict__ ridx,
                                                      const unsigned long long* __restrict__ cnt,
                                                      const double* __restrict__ sum, double base, double alpha,
                                                      double dterm, int64_t* __restrict__ ranks,
                                                      double* __restrict__ dcol, unsigned long long* __restrict__ nbad,
                                                      int64_t* __restrict__ oneseg) {
  GRID_LOOP(s, nkey) {
    const int64_t j = ridx[s];
    const bool ok = cnt[s] == 1ull && j >= 0;
    const double r = ok ? ldd(vd + vbeg(voff, vw, j)) : 0.0;
    const double rn = base + alpha * (sum[s] + dterm);
    ranks[3 * s] = as_l(rn);
    ranks[3 * s + 1] = 0;
    ranks[3 * s + 2] = 0;
    dcol[s] = fabs(rn - r);
    if (!ok) atomicAdd(nbad, 1ull);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    oneseg[0] = 0;
    oneseg[1] = nkey;
  }
}

}  // namespace

#define LAUNCH(kern, n, ...)                                                   \
  do {                                                                         \
    if ((n) > 0) {                                                             \
      hipLaunchKernelGGL(kern, dim3(blocks(n)), dim3(NT), 0, s, __VA_ARGS__); \
      MRH_CHECK_LAUNCH();                                                      \
    }                                                                          \
  } while (0)

size_t prmr_carry_entries(int64_t n) { return dev::segred_carry_entries(n); }

void prmr_scatter_mark(const int64_t* seg, int64_t nkey, const int64_t* voff, int64_t vw, const uint8_t* vd,
                       const int64_t* sid, int64_t nval, double* rank, unsigned long long* cnt, int64_t* flag,
                       int64_t* oneseg, double* dsum, int64_t* cs, double* cv, hipStream_t s) {
  if (nkey <= 0) return;
  LAUNCH(k_pr_scatter_mark, nval, voff, vw, vd, sid, nval, rank, cnt, flag);
  LAUNCH(k_pr_scatter_keys, nkey, nkey, cnt, flag + nval, oneseg);
  dev::segred_launch<double, 0>(DanglingGet{seg, rank}, oneseg, 1, nkey, dsum, cs, cv, s);
}
void prmr_scatter_emit(const int64_t* voff, const uint8_t* vd, const int64_t* sid, const int64_t* keys,
                       const int64_t* pos, const double* rank, int64_t nval, int64_t* ekeys, int64_t* edges,
                       int64_t* ckeys, int64_t* contrib, hipStream_t s) {
  check_arg((reinterpret_cast<uintptr_t>(edges) & 15) == 0, "pagerank_mr scatter: edges must be 16-byte aligned");
  LAUNCH(k_pr_scatter_emit, nval, voff, vd, sid, keys, pos, rank, nval, ekeys, reinterpret_cast<longlong2*>(edges),
         ckeys, contrib);
}
void prmr_update(const int64_t* seg, int64_t nkey, const int64_t* voff, int64_t vw, const uint8_t* vd,
                 const int64_t* sid, int64_t nval, double base, double alpha, double dterm, int64_t* ridx,
                 unsigned long long* cnt, double* sum, int64_t* ranks, double* dcol, unsigned long long* nbad,
                 int64_t* oneseg, double* delta, int64_t* cs, double* cv, hipStream_t s) {
  if (nkey <= 0) return;
  LAUNCH(k_pr_update_mark, nval, voff, vw, sid, nval, ridx, cnt);
  dev::segred_launch<double, 0>(ContribGetMR{voff, vw, vd}, seg, nkey, nval, sum, cs, cv, s);
  LAUNCH(k_pr_update_keys, nkey, nkey, voff, vw, vd, ridx, cnt, sum, base, alpha, dterm, ranks, dcol, nbad, oneseg);
  dev::segred_launch<double, 0>(LoadDouble{dcol}, oneseg, 1, nkey, delta, cs, cv, s);
}

}  // namespace k
}  // namespace mrh
