// Distributed KV movement: MapReduce::aggregate / gather / broadcast on the
// communicator's data plane (comm.h: native RCCL over xGMI for the device
// engine, a c10d process group for the host engine). Replaces MR-MPI's
// Irregular class and the collectives embedded in aggregate/gather/broadcast
// (reference src/irregular.cpp:95-363, src/mapreduce.cpp:385-623, 893-1036).
//
// Exchange protocol — at most two host synchronisations per exchange:
//  1. partition (device, shuffle.hip): owner per pair + per-(owner, block)
//     pair/byte tables, scanned, reduced to this rank's header row
//     {pairs, key bytes, value bytes} x P + {key width code, value width code};
//  2. ONE allgather of the header rows (sync #1): every rank now knows the
//     whole P x P traffic matrix, so every rank derives locally, identically:
//     the global column layout, what it receives from whom, and the number of
//     rounds R = max over receivers of ceil(received bytes / chunk_bytes) —
//     the receive cap of the reference (2 pages, src/mapreduce.cpp:418;
//     src/irregular.cpp:113-164), made deterministic: no 0.9x scale-back
//     retry loop (src/mapreduce.cpp:498-513), no INTMAX limits;
//  3. pack (device): one stable scatter into owner buckets; fixed-width
//     columns move straight into the send buffer, variable ones through a
//     lengths scan + one byte copy. The input KV is released here;
//  4. piece table (variable columns and R > 1 only, sync #2): bucket d is cut
//     into R pieces of equal pair count; their byte sizes go to the receivers
//     in one small exchange;
//  5. R lock-step rounds (reference :426-432) of ONE grouped send/recv each
//     (every column of every peer in one RCCL group): piece k of every bucket
//     is sent from where it lies and received straight into its final place in
//     the output (sender-major, then piece order — the same order as a single
//     round, so the aggregate result does not depend on the cap. The
//     pipelined collate (pipeline=1) groups each round as it lands, so there
//     the order of the values inside a key is (round, sender) and DOES change
//     with chunk_bytes once R > 1; the groups themselves do not). With a host sink
//     (out-of-core aggregate) a round lands in one of two HBM staging buffers
//     and drains to pinned host memory on a copy stream while the next round
//     is on the wire: HBM holds the send buffer + 2 rounds, never the output.
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <exception>
#include <stdexcept>

#include "xfer.h"
#include "../kernels/hashfn.h"
#include "../kernels/launch.h"
#include "comm.h"
#include "guard.h"
#include "kv.h"
#include "streams.h"

namespace mrh {

namespace {

at::TensorOptions opt(at::Device d, at::ScalarType t) { return at::TensorOptions().device(d).dtype(t); }
[[noreturn]] void fail(const std::string& m) { throw std::runtime_error("mrhip: " + m); }
template <typename T>
T* P0(const at::Tensor& t) {
  return t.defined() ? reinterpret_cast<T*>(t.data_ptr()) : nullptr;
}
hipStream_t cur_stream() { return at::hip::getCurrentHIPStream(); }

constexpr int64_t kEmpty = -2;  // width code of a rank with no pairs

int global_width(const std::vector<int64_t>& codes) {
  int64_t w = kEmpty;
  for (int64_t c : codes) {
    if (c == kEmpty) continue;
    if (w == kEmpty) w = c;
    else if (w != c) return -1;
  }
  return (int)w;
}

int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---------------------------------------------------------------- host (CPU engine) twins of shuffle.hip
void cpu_part_count(const int32_t* dest_in, const uint8_t* kd, int kw, const int64_t* koff, const int64_t* voff,
                    int64_t n, int P, int nb, int tile, int32_t* dest_out, int64_t* cnt, int64_t* kb, int64_t* vb) {
  std::fill(cnt, cnt + (int64_t)P * nb, 0);
  if (kb) std::fill(kb, kb + (int64_t)P * nb, 0);
  if (vb) std::fill(vb, vb + (int64_t)P * nb, 0);
  for (int64_t i = 0; i < n; ++i) {
    int d;
    if (dest_in) {
      d = dest_in[i];
    } else {
      const uint32_t h = koff ? dev::hashlittle(kd + koff[i], koff[i + 1] - koff[i], (uint32_t)P)
                              : dev::hashlittle(kd + i * kw, kw, (uint32_t)P);
      d = (int)(h % (uint32_t)P);
      dest_out[i] = d;
    }
    if (d < 0 || d >= P) fail("exchange: destination rank out of range");
    const int64_t o = (int64_t)d * nb + i / tile;
    cnt[o]++;
    if (kb) kb[o] += koff[i + 1] - koff[i];
    if (vb) vb[o] += voff[i + 1] - voff[i];
  }
}

void cpu_part_scatter(const int32_t* dest, int64_t n, int P, int nb, int tile, const int64_t* cbase,
                      const uint8_t* kd, int kw, const uint8_t* vd, int vw, const int64_t* koff, const int64_t* voff,
                      uint8_t* ksend, uint8_t* vsend, int64_t* perm, int32_t* klen, int32_t* vlen) {
  std::vector<int64_t> run((size_t)P);
  for (int b = 0; b < nb; ++b) {
    for (int d = 0; d < P; ++d) run[d] = cbase[(int64_t)d * nb + b];
    for (int64_t i = (int64_t)b * tile; i < std::min<int64_t>(n, (int64_t)(b + 1) * tile); ++i) {
      const int64_t pos = run[dest[i]]++;
      if (kw > 0) std::memcpy(ksend + pos * kw, kd + i * kw, kw);
      if (vw > 0) std::memcpy(vsend + pos * vw, vd + i * vw, vw);
      if (perm) perm[pos] = i;
      if (klen) klen[pos] = (int32_t)(koff[i + 1] - koff[i]);
      if (vlen) vlen[pos] = (int32_t)(voff[i + 1] - voff[i]);
    }
  }
}

// ---------------------------------------------------------------- one variable column of the send side
struct VarCol {
  at::Tensor len;   // int32 [n] in send order
  at::Tensor soff;  // int64 [n+1] send byte offsets
  at::Tensor data;  // send bytes
};

VarCol pack_var(const at::Tensor& data, const at::Tensor& off, const at::Tensor& perm, const at::Tensor& len,
                int64_t n, int64_t total_bytes, at::Device dev) {
  VarCol c;
  c.len = len;
  c.soff = exclusive_scan(len);
  c.data = at::empty({total_bytes}, opt(dev, at::kByte));
  if (dev.is_cuda()) {
    k::copy_var_i64(P0<uint8_t>(data), P0<int64_t>(off), P0<int64_t>(perm), n, P0<uint8_t>(c.data),
                    P0<int64_t>(c.soff), cur_stream());
  } else {
    const uint8_t* s = P0<uint8_t>(data);
    const int64_t* so = P0<int64_t>(off);
    const int64_t* pm = P0<int64_t>(perm);
    const int64_t* doff = P0<int64_t>(c.soff);
    uint8_t* d = P0<uint8_t>(c.data);
    for (int64_t j = 0; j < n; ++j) std::memcpy(d + doff[j], s + so[pm[j]], (size_t)(so[pm[j] + 1] - so[pm[j]]));
  }
  return c;
}

// piece k of a bucket of c pairs covers [c*k/R, c*(k+1)/R)
int64_t piece_lo(int64_t c, int k, int R) { return c * k / R; }

}  // namespace

// =========================================================================== exchange

KV exchange(KV kv, const at::Tensor& dest_given, const Comm& comm, const ExchangeOpts& o, ShuffleStats* st) {
  const auto t0 = std::chrono::steady_clock::now();
  const at::Device dev = comm.device();
  if (!comm.distributed()) {
    if (st) st->send_pairs = st->recv_pairs = kv.n;
    return kv;
  }
  const int P = comm.size(), me = comm.rank();
  const int64_t n = kv.n;
  if (kv.n && kv.device() != dev) kv = kv_to(kv, dev);
  const bool cuda = dev.is_cuda();
  const hipStream_t s = cuda ? cur_stream() : nullptr;
  const int tile = cuda ? k::part_tile() : 4096;
  const int nb = (int)cdiv(n, tile);

  // ---- 1. partition tables
  const bool kvar0 = !kv.kfixed(), vvar0 = !kv.vfixed();
  at::Tensor dest;
  at::Tensor cnt = at::empty({(int64_t)P * nb}, opt(dev, at::kLong));
  at::Tensor kbt = kvar0 ? at::empty({(int64_t)P * nb}, opt(dev, at::kLong)) : at::Tensor();
  at::Tensor vbt = vvar0 ? at::empty({(int64_t)P * nb}, opt(dev, at::kLong)) : at::Tensor();
  const bool hashing = !dest_given.defined();
  if (!hashing) {
    dest = dest_given.to(dev).to(at::kInt).contiguous();
    if (dest.numel() != n) fail("exchange: dest must have one entry per pair");
  } else {
    dest = at::empty({n}, opt(dev, at::kInt));
  }
  if (cuda) {
    k::part_count(hashing ? nullptr : P0<int32_t>(dest), P0<uint8_t>(kv.kdata), kv.kw,
                  kvar0 ? P0<int64_t>(kv.koff) : nullptr, vvar0 ? P0<int64_t>(kv.voff) : nullptr, n, P, nb,
                  hashing ? P0<int32_t>(dest) : nullptr, P0<int64_t>(cnt), P0<int64_t>(kbt), P0<int64_t>(vbt), s);
  } else {
    cpu_part_count(hashing ? nullptr : P0<int32_t>(dest), P0<uint8_t>(kv.kdata), kv.kw,
                   kvar0 ? P0<int64_t>(kv.koff) : nullptr, vvar0 ? P0<int64_t>(kv.voff) : nullptr, n, P, nb, tile,
                   hashing ? P0<int32_t>(dest) : nullptr, P0<int64_t>(cnt), P0<int64_t>(kbt), P0<int64_t>(vbt));
  }
  at::Tensor cs = exclusive_scan(cnt);
  at::Tensor ks = kvar0 ? exclusive_scan(kbt) : at::Tensor();
  at::Tensor vs = vvar0 ? exclusive_scan(vbt) : at::Tensor();
  const int64_t kcode = n ? kv.kw : kEmpty, vcode = n ? kv.vw : kEmpty;
  const int64_t H = 3 * (int64_t)P + 2;
  at::Tensor hdr = at::empty({H}, opt(dev, at::kLong));
  if (cuda) {
    k::part_header(P0<int64_t>(cs), P0<int64_t>(ks), P0<int64_t>(vs), P, nb, kv.kfixed() ? kv.kw : -1,
                   kv.vfixed() ? kv.vw : -1, kcode, vcode, P0<int64_t>(hdr), s);
  } else {
    int64_t* h = P0<int64_t>(hdr);
    const int64_t *c = P0<int64_t>(cs), *kk = P0<int64_t>(ks), *vv = P0<int64_t>(vs);
    for (int d = 0; d < P; ++d) {
      const int64_t a = (int64_t)d * nb, b = a + nb, cc = c[b] - c[a];
      h[3 * d] = cc;
      h[3 * d + 1] = kvar0 ? kk[b] - kk[a] : cc * kv.kw;
      h[3 * d + 2] = vvar0 ? vv[b] - vv[a] : cc * kv.vw;
    }
    h[3 * P] = kcode;
    h[3 * P + 1] = vcode;
  }

  // ---- 2. one allgather of the header rows (host sync #1)
  at::Tensor all = at::empty({P * H}, opt(dev, at::kLong));
  comm.allgather_bytes(hdr.data_ptr(), all.data_ptr(), H * 8);
  comm.host_wait();
  at::Tensor allh = all.to(at::kCPU);
  const int64_t* A = allh.data_ptr<int64_t>();
  auto C = [&](int src, int d) { return A[src * H + 3 * d]; };
  auto KB = [&](int src, int d) { return A[src * H + 3 * d + 1]; };
  auto VB = [&](int src, int d) { return A[src * H + 3 * d + 2]; };
  std::vector<int64_t> kcodes(P), vcodes(P);
  for (int r = 0; r < P; ++r) {
    kcodes[r] = A[r * H + 3 * P];
    vcodes[r] = A[r * H + 3 * P + 1];
  }
  int kw = global_width(kcodes), vw = global_width(vcodes);
  if (kw == kEmpty && vw == kEmpty) {
    // nobody has pairs: no column traffic at all (every rank takes this branch)
    if (st) st->seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return empty_kv(dev, kv.kw, kv.vw);
  }
  if (kw < 0 && kv.kfixed()) kv = to_var_keys(kv);  // same bytes, now with offsets
  if (vw < 0 && kv.vfixed()) kv = to_var_values(kv);
  const bool kvar = kw < 0, vvar = vw < 0;
  std::vector<int64_t> rcount(P), rkb(P), rvb(P);
  int64_t nrecv = 0, rkb_tot = 0, rvb_tot = 0, sent_pairs = 0, sent_bytes = 0;
  for (int r = 0; r < P; ++r) {
    rcount[r] = C(r, me);
    rkb[r] = KB(r, me);
    rvb[r] = VB(r, me);
    nrecv += rcount[r];
    rkb_tot += rkb[r];
    rvb_tot += rvb[r];
    sent_pairs += C(me, r);
    sent_bytes += KB(me, r) + VB(me, r);
  }
  const int64_t lenb = (kvar ? 4 : 0) + (vvar ? 4 : 0);
  int R = 1;
  if (o.chunk_bytes > 0) {
    int64_t worst = 1;
    for (int r = 0; r < P; ++r) {
      int64_t b = 0, c = 0;
      for (int src = 0; src < P; ++src) {
        b += KB(src, r) + VB(src, r);
        c += C(src, r);
      }
      worst = std::max<int64_t>(worst, cdiv(b + c * lenb, o.chunk_bytes));
    }
    R = (int)std::min<int64_t>(worst, 1 << 16);
  }

  // ---- 3. pack: stable scatter into owner buckets
  int64_t my_kb = 0, my_vb = 0;
  for (int d = 0; d < P; ++d) {
    my_kb += KB(me, d);
    my_vb += VB(me, d);
  }
  at::Tensor ksend, vsend, perm, klen, vlen;
  if (!kvar) ksend = at::empty({n * kw}, opt(dev, at::kByte));
  if (!vvar) vsend = at::empty({n * vw}, opt(dev, at::kByte));
  if (kvar || vvar) perm = at::empty({n}, opt(dev, at::kLong));
  if (kvar) klen = at::empty({n}, opt(dev, at::kInt));
  if (vvar) vlen = at::empty({n}, opt(dev, at::kInt));
  if (n) {
    if (cuda) {
      k::part_scatter(P0<int32_t>(dest), n, P, nb, P0<int64_t>(cs), P0<uint8_t>(kv.kdata), kvar ? -1 : kw,
                      P0<uint8_t>(kv.vdata), vvar ? -1 : vw, kvar ? P0<int64_t>(kv.koff) : nullptr,
                      vvar ? P0<int64_t>(kv.voff) : nullptr, P0<uint8_t>(ksend), P0<uint8_t>(vsend),
                      P0<int64_t>(perm), P0<int32_t>(klen), P0<int32_t>(vlen), s);
    } else {
      cpu_part_scatter(P0<int32_t>(dest), n, P, nb, tile, P0<int64_t>(cs), P0<uint8_t>(kv.kdata), kvar ? -1 : kw,
                       P0<uint8_t>(kv.vdata), vvar ? -1 : vw, kvar ? P0<int64_t>(kv.koff) : nullptr,
                       vvar ? P0<int64_t>(kv.voff) : nullptr, P0<uint8_t>(ksend), P0<uint8_t>(vsend),
                       P0<int64_t>(perm), P0<int32_t>(klen), P0<int32_t>(vlen));
    }
  }
  VarCol kc, vc;
  if (kvar) kc = pack_var(kv.kdata, kv.koff, perm, klen, n, my_kb, dev);
  if (vvar) vc = pack_var(kv.vdata, kv.voff, perm, vlen, n, my_vb, dev);
  if (kvar) ksend = kc.data;
  if (vvar) vsend = vc.data;
  kv = KV();  // the input is no longer needed: HBM now holds the send buffer, not both
  dest = perm = cnt = kbt = vbt = cs = ks = vs = at::Tensor();

  // ---- 4. piece byte tables (variable columns, R > 1; host sync #2)
  // mine[d][c][k] (bytes of my piece k to d, column c in {K, V}), theirs[s][c][k]
  std::vector<int64_t> mine, theirs;
  const bool need_tab = (kvar || vvar) && R > 1;
  if (need_tab) {
    std::vector<int64_t> start(P + 1, 0);
    for (int d = 0; d < P; ++d) start[d + 1] = start[d] + C(me, d);
    at::Tensor tab = at::zeros({(int64_t)P * 2 * R}, opt(dev, at::kLong));
    at::Tensor rtab = at::empty({(int64_t)P * 2 * R}, opt(dev, at::kLong));
    at::Tensor kt = at::zeros({(int64_t)P * R}, opt(dev, at::kLong)), vt = at::zeros({(int64_t)P * R}, opt(dev, at::kLong));
    at::Tensor sdev = at::tensor(start, opt(at::kCPU, at::kLong)).to(dev);
    for (int c = 0; c < 2; ++c) {
      const VarCol& col = c == 0 ? kc : vc;
      if (!(c == 0 ? kvar : vvar)) continue;
      at::Tensor& t = c == 0 ? kt : vt;
      if (cuda) {
        k::piece_bytes(P0<int64_t>(col.soff), P0<int64_t>(sdev), P, R, P0<int64_t>(t), s);
      } else {
        const int64_t* so = P0<int64_t>(col.soff);
        int64_t* tp = P0<int64_t>(t);
        for (int d = 0; d < P; ++d)
          for (int k = 0; k < R; ++k) {
            const int64_t cc = start[d + 1] - start[d];
            tp[(int64_t)d * R + k] = so[start[d] + piece_lo(cc, k + 1, R)] - so[start[d] + piece_lo(cc, k, R)];
          }
      }
    }
    tab.view({P, 2, R}).select(1, 0).copy_(kt.view({P, R}));
    tab.view({P, 2, R}).select(1, 1).copy_(vt.view({P, R}));
    std::vector<Xfer> xs, xr;
    for (int p = 0; p < P; ++p) {
      xs.push_back({p, P0<int64_t>(tab) + (int64_t)p * 2 * R, 16 * (int64_t)R});
      xr.push_back({p, P0<int64_t>(rtab) + (int64_t)p * 2 * R, 16 * (int64_t)R});
    }
    comm.sendrecv(xs, xr);
    comm.host_wait();
    at::Tensor both = at::cat({tab, rtab}).to(at::kCPU);
    const int64_t* bp = both.data_ptr<int64_t>();
    mine.assign(bp, bp + (int64_t)P * 2 * R);
    theirs.assign(bp + (int64_t)P * 2 * R, bp + (int64_t)P * 4 * R);
  }
  auto pairs_of = [&](int src, int d, int k) { return piece_lo(C(src, d), k + 1, R) - piece_lo(C(src, d), k, R); };
  // bytes of piece k from src to d in column c (fixed: pairs x width)
  auto bytes_of = [&](int src, int d, int c, int k) -> int64_t {
    const int w = c == 0 ? kw : vw;
    if (w >= 0) return pairs_of(src, d, k) * w;
    if (R == 1) return c == 0 ? KB(src, d) : VB(src, d);
    if (src == me) return mine[((int64_t)d * 2 + c) * R + k];
    if (d == me) return theirs[((int64_t)src * 2 + c) * R + k];
    fail("exchange: piece table lookup");
  };

  // ---- 5. output
  const bool round_sink = (bool)o.round_sink;
  const bool host_sink = !round_sink && cuda &&
                         (o.host_sink || (o.hbm_budget > 0 && rkb_tot + rvb_tot + nrecv * (lenb + 8) > o.hbm_budget));
  const at::Device odev = host_sink ? at::Device(at::kCPU) : dev;
  auto oopt = [&](at::ScalarType t) {
    auto x = opt(odev, t);
    return host_sink ? x.pinned_memory(true) : x;
  };
  KV out;
  const int64_t nout = round_sink ? 0 : nrecv;  // a round sink gets the pairs instead
  out.n = nout;
  out.kw = kw;
  out.vw = vw;
  out.kdata = at::empty({round_sink ? 0 : kvar ? rkb_tot : nrecv * std::max(kw, 0)}, oopt(at::kByte));
  out.vdata = at::empty({round_sink ? 0 : vvar ? rvb_tot : nrecv * std::max(vw, 0)}, oopt(at::kByte));
  at::Tensor rklen = kvar ? at::empty({nout}, oopt(at::kInt)) : at::Tensor();
  at::Tensor rvlen = vvar ? at::empty({nout}, oopt(at::kInt)) : at::Tensor();

  // per-column send bases (bytes) of bucket d, piece k; receive bases of (src, k)
  // columns: 0 key bytes, 1 value bytes, 2 key lengths, 3 value lengths
  struct Col {
    uint8_t* send;  // this rank's bucketed send buffer
    uint8_t* recv;  // final output (device sink) or host output (host sink)
    bool on;
    int c;          // 0 key, 1 value
    bool lens;      // int32 lengths column
  };
  std::vector<Col> cols = {
      {P0<uint8_t>(ksend), P0<uint8_t>(out.kdata), kw != 0, 0, false},
      {P0<uint8_t>(vsend), P0<uint8_t>(out.vdata), vw != 0, 1, false},
      {kvar ? P0<uint8_t>(kc.len) : nullptr, P0<uint8_t>(rklen), kvar, 0, true},
      {vvar ? P0<uint8_t>(vc.len) : nullptr, P0<uint8_t>(rvlen), vvar, 1, true},
  };
  // running offsets: send side per (col, d), receive side per (col, src)
  std::vector<std::vector<int64_t>> soff(4, std::vector<int64_t>(P, 0)), roff(4, std::vector<int64_t>(P, 0));
  for (int ci = 0; ci < 4; ++ci) {
    if (!cols[ci].on) continue;
    int64_t a = 0, b = 0;
    for (int p = 0; p < P; ++p) {
      soff[ci][p] = a;
      roff[ci][p] = b;
      const int c = cols[ci].c;
      if (cols[ci].lens) {
        a += C(me, p) * 4;
        b += C(p, me) * 4;
      } else {
        a += c == 0 ? KB(me, p) : VB(me, p);
        b += c == 0 ? KB(p, me) : VB(p, me);
      }
    }
  }
  auto piece_col_bytes = [&](int ci, int src, int d, int k) -> int64_t {
    return cols[ci].lens ? pairs_of(src, d, k) * 4 : bytes_of(src, d, cols[ci].c, k);
  };

  // ---- 6a. pipelined rounds into a consumer: round k lands in device staging
  // buffer k%2 on the communication stream while the compute stream hands
  // round k-1 to the sink (two rounds in flight); a staging buffer is posted
  // again only behind the sink's work on it (the RCCL fence on the compute
  // stream orders it)
  if (round_sink) {
    int64_t stage_bytes = 1;
    for (int k = 0; k < R; ++k) {
      int64_t b = 0;
      for (int ci = 0; ci < 4; ++ci)
        if (cols[ci].on)
          for (int src = 0; src < P; ++src) b += piece_col_bytes(ci, src, me, k);
      stage_bytes = std::max(stage_bytes, b + 4 * 16);  // each column starts 16-byte aligned
    }
    at::Tensor stage[2] = {at::empty({stage_bytes}, opt(dev, at::kByte)), at::empty({stage_bytes}, opt(dev, at::kByte))};
    struct RoundLayout {
      int64_t start[4] = {0, 0, 0, 0}, bytes[4] = {0, 0, 0, 0}, n = 0;
      hipEvent_t landed = nullptr;
    } lay[2];
    auto post = [&](int k) {
      guard::fault_point("exchange_round", me);
      RoundLayout& L = lay[k % 2];
      L = RoundLayout();
      std::vector<Xfer> xs, xr;
      int64_t sbuf = 0;
      for (int src = 0; src < P; ++src) L.n += pairs_of(src, me, k);
      for (int ci = 0; ci < 4; ++ci) {
        if (!cols[ci].on) continue;
        sbuf = (sbuf + 15) & ~int64_t(15);  // the int32 length columns are viewed in place
        L.start[ci] = sbuf;
        for (int p = 0; p < P; ++p) {
          const int64_t sb = piece_col_bytes(ci, me, p, k);
          xs.push_back({p, cols[ci].send + soff[ci][p], sb});
          soff[ci][p] += sb;
          const int64_t rb = piece_col_bytes(ci, p, me, k);
          xr.push_back({p, P0<uint8_t>(stage[k % 2]) + sbuf, rb});
          sbuf += rb;
        }
        L.bytes[ci] = sbuf - L.start[ci];
      }
      if (comm.uses_rccl()) L.landed = comm.rccl()->sendrecv_async(xs, xr, s);
      else comm.sendrecv(xs, xr);
    };
    post(0);
    if (R > 1) post(1);
    for (int k = 0; k < R; ++k) {
      RoundLayout& L = lay[k % 2];
      if (L.landed) guard::hip_check(hipStreamWaitEvent(s, L.landed, 0), "round_wait", me);
      if (L.n > 0) {
        KV r;
        r.n = L.n;
        r.kw = kw;
        r.vw = vw;
        r.kdata = stage[k % 2].narrow(0, L.start[0], L.bytes[0]);
        r.vdata = stage[k % 2].narrow(0, L.start[1], L.bytes[1]);
        if (kvar) r.koff = exclusive_scan(stage[k % 2].narrow(0, L.start[2], L.bytes[2]).view(at::kInt));
        if (vvar) r.voff = exclusive_scan(stage[k % 2].narrow(0, L.start[3], L.bytes[3]).view(at::kInt));
        o.round_sink(r);
      }
      if (k + 2 < R) post(k + 2);
    }
    for (auto& L : lay) L.landed = nullptr;  // events belong to the communicator's ring
  }

  // ---- 6. rounds
  const hipStream_t cs_ = s;
  at::Tensor stage[2];
  Event drained[2];  // staging buffer k%2 has been copied to the host
  // the checked-HIP-call sites of the drains (MRH_FAULT=hip:<site>:<rank>)
  auto site = [me](const char* name) { guard::hip_check(hipSuccess, name, me); };
  c10::optional<c10::hip::HIPStream> copy_stream;
  int64_t stage_bytes = 0;
  if (host_sink) {
    for (int k = 0; k < R; ++k) {
      int64_t b = 0;
      for (int ci = 0; ci < 4; ++ci)
        if (cols[ci].on)
          for (int src = 0; src < P; ++src) b += piece_col_bytes(ci, src, me, k);
      stage_bytes = std::max(stage_bytes, b);
    }
    for (auto& t : stage) t = at::empty({std::max<int64_t>(stage_bytes, 1)}, opt(dev, at::kByte));
    copy_stream = c10::hip::getStreamFromPool(false, dev.index());
  }
  // an exception out of the rounds (a failed drain, a peer failure) must not
  // unwind while drain copies still write into the output being freed
  struct DrainFence {
    c10::optional<c10::hip::HIPStream>* cs;
    ~DrainFence() {
      if (std::uncaught_exceptions() > 0 && cs->has_value()) (void)hipStreamSynchronize((*cs)->stream());
    }
  } drain_fence{&copy_stream};
  for (int k = 0; k < R && !round_sink; ++k) {
    guard::fault_point("exchange_round", me);
    std::vector<Xfer> xs, xr;
    struct Drain {
      uint8_t* dst;
      int64_t stage_off, bytes;
    };
    std::vector<Drain> drains;
    int64_t sbuf = 0;
    for (int ci = 0; ci < 4; ++ci) {
      if (!cols[ci].on) continue;
      for (int p = 0; p < P; ++p) {
        const int64_t sb = piece_col_bytes(ci, me, p, k);
        xs.push_back({p, cols[ci].send + soff[ci][p], sb});
        soff[ci][p] += sb;
        const int64_t rb = piece_col_bytes(ci, p, me, k);
        if (host_sink) {
          xr.push_back({p, P0<uint8_t>(stage[k % 2]) + sbuf, rb});
          drains.push_back({cols[ci].recv + roff[ci][p], sbuf, rb});
          sbuf += rb;
        } else {
          xr.push_back({p, cols[ci].recv + roff[ci][p], rb});
        }
        roff[ci][p] += rb;
      }
    }
    if (!host_sink) {
      if (o.all2all) {
        comm.sendrecv(xs, xr);
      } else {
        for (int j = 0; j < P; ++j) {  // ring order: step j pairs me -> me+j with me-j -> me
          const int to = (me + j) % P, from = (me - j + P) % P;
          std::vector<Xfer> s1, r1;
          for (const Xfer& x : xs)
            if (x.peer == to) s1.push_back(x);
          for (const Xfer& x : xr)
            if (x.peer == from) r1.push_back(x);
          comm.sendrecv(s1, r1);
        }
      }
      continue;
    }
    // staging buffer k%2 is free once the drain of round k-2 finished
    site("drain_wait");
    drained[k % 2].wait_on(cs_, "mrhip: exchange drain_wait");  // (unset in rounds 0 and 1)
    const hipStream_t cp = copy_stream->stream();
    if (comm.uses_rccl()) {  // `landed` belongs to the communicator's ring
      const hipEvent_t landed = comm.rccl()->sendrecv_async(xs, xr, cs_);
      guard::hip_check(hipStreamWaitEvent(cp, landed, 0), "drain_wait", me);
    } else {
      comm.sendrecv(xs, xr);
      site("landed_event");
      order_after(cp, cs_, "mrhip: exchange landed_event");
    }
    for (const Drain& d : drains) {
      note_xfer_bytes(false, d.bytes);
      if (d.bytes)
        guard::hip_check(hipMemcpyAsync(d.dst, P0<uint8_t>(stage[k % 2]) + d.stage_off, (size_t)d.bytes,
                                        hipMemcpyDeviceToHost, cp),
                         "drain_copy", me);
    }
    site("drain_event");
    drained[k % 2].record(cp, "mrhip: exchange drain_event");
  }
  if (host_sink) {
    for (const Event& e : drained) e.wait_on(cs_, "mrhip: exchange drain_wait");
    comm.host_wait();  // pinned host output complete before the host reads it
  }

  // ---- 7. offsets of variable columns
  if (kvar) out.koff = round_sink ? at::zeros({1}, opt(dev, at::kLong)) : exclusive_scan(rklen);
  if (vvar) out.voff = round_sink ? at::zeros({1}, opt(dev, at::kLong)) : exclusive_scan(rvlen);
  if (st) {
    st->send_pairs += sent_pairs;
    st->recv_pairs += nrecv;
    st->send_bytes += sent_bytes;
    st->recv_bytes += rkb_tot + rvb_tot;
    st->rounds += R;
    st->seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  return out;
}

// ------------------------------------------------------------------ local partition
Buckets bucket_local(const KV& kv_in, const at::Tensor& dest_in, int P) {
  const at::Device dev = kv_in.device();
  const bool cuda = dev.is_cuda();
  const hipStream_t s = cuda ? cur_stream() : nullptr;
  const int64_t n = kv_in.n;
  const int tile = cuda ? k::part_tile() : 4096;
  const int nb = (int)cdiv(n, tile);
  const KV& kv = kv_in;
  const bool kvar = !kv.kfixed(), vvar = !kv.vfixed();
  at::Tensor dest = dest_in.to(dev).to(at::kInt).contiguous();
  if (dest.numel() != n) fail("bucket_local: one destination per pair");
  at::Tensor cnt = at::empty({(int64_t)P * nb}, opt(dev, at::kLong));
  at::Tensor kbt = kvar ? at::empty({(int64_t)P * nb}, opt(dev, at::kLong)) : at::Tensor();
  at::Tensor vbt = vvar ? at::empty({(int64_t)P * nb}, opt(dev, at::kLong)) : at::Tensor();
  if (cuda) {
    k::part_count(P0<int32_t>(dest), P0<uint8_t>(kv.kdata), kv.kw, kvar ? P0<int64_t>(kv.koff) : nullptr,
                  vvar ? P0<int64_t>(kv.voff) : nullptr, n, P, nb, nullptr, P0<int64_t>(cnt), P0<int64_t>(kbt),
                  P0<int64_t>(vbt), s);
  } else {
    cpu_part_count(P0<int32_t>(dest), P0<uint8_t>(kv.kdata), kv.kw, kvar ? P0<int64_t>(kv.koff) : nullptr,
                   vvar ? P0<int64_t>(kv.voff) : nullptr, n, P, nb, tile, nullptr, P0<int64_t>(cnt),
                   P0<int64_t>(kbt), P0<int64_t>(vbt));
  }
  at::Tensor cs = exclusive_scan(cnt);
  at::Tensor ks = kvar ? exclusive_scan(kbt) : at::Tensor();
  at::Tensor vs = vvar ? exclusive_scan(vbt) : at::Tensor();
  // per-bucket totals to the host (one sync)
  at::Tensor hdr = at::empty({3 * (int64_t)P + 2}, opt(dev, at::kLong));
  if (cuda) {
    k::part_header(P0<int64_t>(cs), P0<int64_t>(ks), P0<int64_t>(vs), P, nb, kvar ? -1 : kv.kw, vvar ? -1 : kv.vw, 0,
                   0, P0<int64_t>(hdr), s);
  } else {
    int64_t* h = P0<int64_t>(hdr);
    const int64_t *c = P0<int64_t>(cs), *kk = P0<int64_t>(ks), *vv = P0<int64_t>(vs);
    for (int d = 0; d < P; ++d) {
      const int64_t a = (int64_t)d * nb, b = a + nb, cc = c[b] - c[a];
      h[3 * d] = cc;
      h[3 * d + 1] = kvar ? kk[b] - kk[a] : cc * kv.kw;
      h[3 * d + 2] = vvar ? vv[b] - vv[a] : cc * kv.vw;
    }
  }
  at::Tensor hh = hdr.to(at::kCPU);
  Buckets out;
  int64_t kb_tot = 0, vb_tot = 0;
  for (int d = 0; d < P; ++d) {
    out.count.push_back(hh[3 * d].item<int64_t>());
    kb_tot += hh[3 * d + 1].item<int64_t>();
    vb_tot += hh[3 * d + 2].item<int64_t>();
  }
  at::Tensor ksend, vsend, perm, klen, vlen;
  if (!kvar) ksend = at::empty({n * kv.kw}, opt(dev, at::kByte));
  if (!vvar) vsend = at::empty({n * kv.vw}, opt(dev, at::kByte));
  if (kvar || vvar) perm = at::empty({n}, opt(dev, at::kLong));
  if (kvar) klen = at::empty({n}, opt(dev, at::kInt));
  if (vvar) vlen = at::empty({n}, opt(dev, at::kInt));
  if (n) {
    if (cuda) {
      k::part_scatter(P0<int32_t>(dest), n, P, nb, P0<int64_t>(cs), P0<uint8_t>(kv.kdata), kvar ? -1 : kv.kw,
                      P0<uint8_t>(kv.vdata), vvar ? -1 : kv.vw, kvar ? P0<int64_t>(kv.koff) : nullptr,
                      vvar ? P0<int64_t>(kv.voff) : nullptr, P0<uint8_t>(ksend), P0<uint8_t>(vsend),
                      P0<int64_t>(perm), P0<int32_t>(klen), P0<int32_t>(vlen), s);
    } else {
      cpu_part_scatter(P0<int32_t>(dest), n, P, nb, tile, P0<int64_t>(cs), P0<uint8_t>(kv.kdata), kvar ? -1 : kv.kw,
                       P0<uint8_t>(kv.vdata), vvar ? -1 : kv.vw, kvar ? P0<int64_t>(kv.koff) : nullptr,
                       vvar ? P0<int64_t>(kv.voff) : nullptr, P0<uint8_t>(ksend), P0<uint8_t>(vsend),
                       P0<int64_t>(perm), P0<int32_t>(klen), P0<int32_t>(vlen));
    }
  }
  out.kv.n = n;
  out.kv.kw = kv.kw;
  out.kv.vw = kv.vw;
  if (kvar) {
    VarCol c = pack_var(kv.kdata, kv.koff, perm, klen, n, kb_tot, dev);
    out.kv.kdata = c.data;
    out.kv.koff = c.soff;
  } else {
    out.kv.kdata = ksend;
  }
  if (vvar) {
    VarCol c = pack_var(kv.vdata, kv.voff, perm, vlen, n, vb_tot, dev);
    out.kv.vdata = c.data;
    out.kv.voff = c.soff;
  } else {
    out.kv.vdata = vsend;
  }
  return out;
}

KV aggregate(KV kv, const Comm& comm, const ExchangeOpts& o, ShuffleStats* st) {
  if (!comm.distributed()) return kv;
  return exchange(std::move(kv), at::Tensor(), comm, o, st);
}

KV gather_to(KV kv, int nprocs, const Comm& comm, const ExchangeOpts& o, ShuffleStats* st) {
  if (!comm.distributed()) return kv;
  const int target = comm.rank() % nprocs;
  at::Tensor dest = at::full({kv.n}, target, opt(comm.device(), at::kInt));
  return exchange(std::move(kv), dest, comm, o, st);
}

KV broadcast(const KV& kv_in, int root, const Comm& comm) {
  if (!comm.distributed()) return kv_in;
  const at::Device dev = comm.device();
  const bool me_root = comm.rank() == root;
  KV kv = kv_in.n && kv_in.device() != dev ? kv_to(kv_in, dev) : kv_in;
  at::Tensor hdr = at::zeros({5}, opt(at::kCPU, at::kLong));
  if (me_root) {
    int64_t* h = hdr.data_ptr<int64_t>();
    h[0] = kv.n;
    h[1] = kv.kw;
    h[2] = kv.vw;
    h[3] = kv.kdata.defined() ? kv.kdata.numel() : 0;
    h[4] = kv.vdata.defined() ? kv.vdata.numel() : 0;
  }
  hdr = hdr.to(dev);
  comm.broadcast_tensor(hdr, root);
  comm.host_wait();
  at::Tensor h = hdr.to(at::kCPU);
  KV o;
  o.n = h[0].item<int64_t>();
  o.kw = (int)h[1].item<int64_t>();
  o.vw = (int)h[2].item<int64_t>();
  const int64_t kb = h[3].item<int64_t>(), vb = h[4].item<int64_t>();
  auto bc = [&](const at::Tensor& t, int64_t numel, at::ScalarType ty) {
    at::Tensor x = me_root ? t.contiguous() : at::empty({numel}, opt(dev, ty));
    if (numel) comm.broadcast_tensor(x, root);
    return x;
  };
  o.kdata = bc(kv.kdata, kb, at::kByte);
  o.vdata = bc(kv.vdata, vb, at::kByte);
  if (o.kw < 0) o.koff = bc(kv.koff, o.n + 1, at::kLong);
  if (o.vw < 0) o.voff = bc(kv.voff, o.n + 1, at::kLong);
  return o;
}

at::Tensor partition_dest(const KV& kv, int P, at::Tensor* counts) {
  const at::Device dev = kv.device();
  at::Tensor h = hash32_keys(kv, (uint32_t)P);
  at::Tensor dest = at::empty({kv.n}, opt(dev, at::kInt));
  *counts = at::zeros({P}, opt(dev, at::kLong));
  if (dev.is_cuda()) {
    k::partition_dest(P0<uint32_t>(h), kv.n, P, P0<int32_t>(dest), P0<int64_t>(*counts), cur_stream());
  } else {
    const uint32_t* hp = P0<uint32_t>(h);
    int32_t* d = P0<int32_t>(dest);
    int64_t* c = P0<int64_t>(*counts);
    for (int64_t i = 0; i < kv.n; ++i) {
      d[i] = (int32_t)(hp[i] % (uint32_t)P);
      c[d[i]]++;
    }
  }
  return dest;
}

}  // namespace mrh
